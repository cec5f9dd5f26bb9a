"""The DFT data interface without a device: exported symbols, named tuples, aliases, and the
error of scaling an object whose simulation holds no fields."""
import pytest

import meep_nl_amd as mp
from meep_nl_amd import _lib, core, simulation

NEW = ["mnl_fields_dft_get", "mnl_fields_dft_load", "mnl_fields_dft_scale", "mnl_fields_dft_save",
       "mnl_fields_dft_load_file"]


def test_exported_symbols():
    names = _lib.exported_symbols()
    for n in NEW:
        assert n in names
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "meep_nl_amd.h")).read()
    for n in NEW:
        assert f"int {n}(mnl_fields *f, int handle" in header


def test_fields_methods():
    for n in ("dft_get", "dft_load", "dft_scale", "dft_save", "dft_load_file"):
        assert callable(getattr(core.Fields, n))


def test_named_tuples_and_aliases():
    assert mp.FluxData._fields == ("E", "H") and mp.NearToFarData._fields == ("F",)
    d = mp.FluxData(E=1, H=2)
    assert d.E == 1 and d.H == 2 and mp.NearToFarData(F=3).F == 3
    S = mp.Simulation
    assert S.get_mode_data is S.get_flux_data
    assert S.load_mode_data is S.load_flux_data
    assert S.load_minus_mode_data is S.load_minus_flux_data
    assert S.save_mode is S.save_flux and S.load_mode is S.load_flux
    assert S.load_minus_mode is S.load_minus_flux
    for n in ("get_flux_data", "load_flux_data", "load_minus_flux_data", "save_flux", "load_flux",
              "load_minus_flux", "display_fluxes", "get_near2far_data", "load_near2far_data",
              "load_minus_near2far_data", "save_near2far", "load_near2far", "load_minus_near2far"):
        assert callable(getattr(S, n)), n
    for n in ("scale_flux_fields", "scale_near2far_fields", "FluxData", "NearToFarData"):
        assert getattr(mp, n) is getattr(simulation, n)
    for cls in (mp.DftFlux, mp.DftFields, mp.DftNear2Far):
        assert callable(cls.scale_dfts)


def test_scale_without_fields_raises():
    """add_flux always builds the fields (init_sim), so an object without them was made by hand
    or belongs to a simulation that was reset: a clear error, no device needed."""
    sim = mp.Simulation(cell_size=mp.Vector3(0, 0, 4), resolution=10, dimensions=1)
    flux = mp.DftFlux(sim, [0.3], [mp.FluxRegion(center=mp.Vector3())], 0)
    n2f = mp.DftNear2Far(sim, [0.3], [], 0, 1)
    with pytest.raises(RuntimeError, match="meep:.*never initialised"):
        mp.scale_flux_fields(-1, flux)
    with pytest.raises(RuntimeError, match="meep:.*never initialised"):
        mp.scale_near2far_fields(2, n2f)
    with pytest.raises(RuntimeError, match="meep:"):
        sim.get_flux_data(flux)
    assert sim.fields is None
