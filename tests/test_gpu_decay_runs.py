"""Simulation.run with the three decay conditions: the batched run stops
after the same step as the one-step loop (forced by a no-op step function), with the same flux
bits and the same field at the end, in fewer fields.step calls -- and in pairs of steps on the
3-D grid, which the one-step loop never reaches."""
import threading

import numpy as np
import pytest

import meep_nl_amd as mp
from scenarios import GroupSim, random_init
from test_gpu_tb import SRCS, sc_tb

pytestmark = pytest.mark.gpu


def noop(sim):
    pass


def _count_steps(fields, paired=None):
    """Count the fields.step calls; paired: tb_info()["active"] right after every call of at
    least two steps (a reader that leaves the fused mode afterwards, as field_energy_in_box
    does to materialise E, makes tb_info answer False until the next call)."""
    calls = []
    orig = fields.step

    def step(n=1):
        calls.append(int(n))
        r = orig(n)
        if paired is not None and int(n) >= 2:
            paired.append(fields.tb_info()["active"])
        return r
    fields.step = step
    return calls


def _result(sim, flux, pt, c, calls):
    f = sim.fields
    return dict(t=sim.timestep, flux=np.array(mp.get_fluxes(flux)),
                E=f.dft_get(flux.handle, 0), H=f.dft_get(flux.handle, 1),
                v=sim.get_field_point(c, pt), calls=calls)


def _same(one, batched):
    assert batched["t"] == one["t"]
    for k in ("flux", "E", "H"):
        assert np.array_equal(batched[k], one[k]), k
    assert batched["v"] == one["v"] and one["v"] != 0
    assert one["calls"] == [1] * one["t"]
    assert len(batched["calls"]) < len(one["calls"]) and sum(batched["calls"]) == one["t"]


@pytest.fixture(autouse=True)
def _quiet():
    old = mp.verbosity.get()
    mp.verbosity(0)
    yield
    mp.verbosity(old)


# ---- the 1-D Kerr cell of test_gpu_dft.test_simulation_flux_until_after_sources
PT1 = mp.Vector3(0, 0, 8.0)
PTC = mp.Vector3(0, 0, -7.5)  # the conditions' point: beside the source


def kerr_1d(step_funcs, **run):
    fcen, df = 1 / 3, 0.2
    sim = mp.Simulation(cell_size=mp.Vector3(0, 0, 20), resolution=20, dimensions=1,
                        boundary_layers=[mp.PML(1.0)],
                        default_material=mp.Medium(index=1, chi3=1e-2),
                        sources=[mp.Source(mp.GaussianSource(fcen, fwidth=df), component=mp.Ex,
                                           center=mp.Vector3(0, 0, -8.0))])
    trans = sim.add_flux(fcen, 4 * df, 7, mp.FluxRegion(center=PT1))
    calls = _count_steps(sim.fields)
    sim.run(*step_funcs, **run)
    return _result(sim, trans, PTC, mp.Ex, calls)


CONDS_1D = {
    "fields": lambda: mp.stop_when_fields_decayed(5, mp.Ex, PTC, 1e-3),
    "energy": lambda: mp.stop_when_energy_decayed(5, 1e-3),
    "dft": lambda: mp.stop_when_dft_decayed(1e-3, minimum_run_time=20),
}


@pytest.mark.parametrize("cond", sorted(CONDS_1D))
@pytest.mark.parametrize("how", ["until_after_sources", "until_list"])
def test_kerr_1d_batched_equals_one_step_loop(cond, how):
    def run(step_funcs):
        c = CONDS_1D[cond]()
        if how == "until_list":
            return kerr_1d(step_funcs, until=[40, c])
        return kerr_1d(step_funcs, until_after_sources=c)
    one, batched = run((noop,)), run(())
    _same(one, batched)
    assert one["t"] > 100


# ---- the pair tests' 3-D grid with a flux plane
PT3 = mp.Vector3(0.513, -0.287, 0.731)


def slab_3d(step_funcs, **run):
    src = [mp.Source(mp.GaussianSource(0.25, fwidth=0.25, start_time=0, cutoff=5.0),
                     component=(mp.Ex, mp.Ey, mp.Ez)[i % 3], center=mp.Vector3(*p),
                     amplitude=1.0 - 0.1 * i) for i, p in enumerate(SRCS)]
    sim = mp.Simulation(cell_size=mp.Vector3(9.6, 6.4, 8.0), resolution=10,
                        boundary_layers=[mp.PML(0.7)], eps_averaging=False, sources=src,
                        geometry=[mp.Block(size=mp.Vector3(mp.inf, 1.6, 3.4),
                                           center=mp.Vector3(0, 0, 1.3),
                                           material=mp.Medium(epsilon=6.0))])
    flux = sim.add_flux(0.25, 0.2, 5, mp.FluxRegion(center=mp.Vector3(0, 0, -1.05),
                                                    size=mp.Vector3(2.2, 1.9, 0)))
    f = sim.fields

    class Init:
        shape = staticmethod(lambda: f.gv.shape())
        initialize_field = staticmethod(f.initialize_field)
    random_init(Init, (6, 7, 8, 9, 10, 11), scale=0.05)
    paired = []
    calls = _count_steps(f, paired)
    sim.run(*step_funcs, **run)
    active = f.tb_info()["active"]  # before any reader of this test
    out = _result(sim, flux, PT3, mp.Ez, calls)
    out["active"], out["paired"] = active, paired
    out["sim"], out["flux_obj"] = sim, flux
    return out


CONDS_3D = {
    "fields": lambda: mp.stop_when_fields_decayed(2, mp.Ez, PT3, 3e-1),
    "energy": lambda: mp.stop_when_energy_decayed(2, 3e-1),
    "dft": lambda: mp.stop_when_dft_decayed(3e-1),
}


@pytest.mark.parametrize("cond", sorted(CONDS_3D))
def test_slab_3d_batched_runs_in_pairs(cond):
    # until_after_sources (the sources end at t = 40), at most 10 time units more
    one = slab_3d((noop,), until_after_sources=[10, CONDS_3D[cond]()])
    batched = slab_3d((), until_after_sources=[10, CONDS_3D[cond]()])
    _same(one, batched)
    assert one["t"] >= 800
    # pairs of steps: only the batched run, in every call of at least two steps
    assert batched["paired"] and all(batched["paired"]) and not one["paired"]
    assert not one["active"]
    if cond != "energy":  # (its last check read the energy, which leaves the fused mode)
        assert batched["active"]


def test_slab_3d_until_list():
    one = slab_3d((noop,), until=[12, CONDS_3D["fields"]()])
    batched = slab_3d((), until=[12, CONDS_3D["fields"]()])
    _same(one, batched)
    assert batched["active"] and all(batched["paired"])


def test_slab_3d_same_condition_twice():
    """Two runs with conditions at the same point on one Simulation: the second run's probe
    sits where the first one's was (removed at the end of the first run)."""
    def two_runs(step_funcs):
        out = slab_3d(step_funcs, until=[12, CONDS_3D["fields"]()])
        sim, flux, calls = out["sim"], out["flux_obj"], out["calls"]
        cond = CONDS_3D["fields"]()
        sim.run(*step_funcs, until=[9, cond])
        res = _result(sim, flux, PT3, mp.Ez, calls)
        res["closure"], res["paired"] = dict(cond.closure), out["paired"]
        return res
    one, batched = two_runs((noop,)), two_runs(())
    _same(one, batched)
    assert batched["closure"] == one["closure"] and one["t"] > 240  # (the second run stepped too)
    assert batched["paired"] and all(batched["paired"])


# ---- two slabs, one host thread per rank (the GroupSim of scenarios.py)
class RankSim(mp.Simulation):
    """A Simulation around one rank's existing Fields."""

    def __init__(self, fields):
        self.fields = fields
        self.progress_interval = 1e9
        self.run_index = 0
        self.cell_size = mp.Vector3(9.6, 6.4, 9.6)
        self.dft_objects = []

    def init_sim(self):
        pass


def slabs_run(step_funcs):
    o = sc_tb(GroupSim, sizes=(9.6, 6.4, 9.6), steps=())
    h = o.add_dft_flux([([-1.0, -1.0, 0.05], [1.2, 0.9, 0.05], 2, 1.0)], [0.2, 0.25, 0.31], 1)
    pt = mp.Vector3(0.31, 0.27, 0.02)  # straddles the slab face
    sims = [RankSim(f) for f in o._all()]
    calls = [_count_steps(f) for f in o._all()]
    err = []

    def run(s):
        try:
            s.run(*step_funcs, until=[12, mp.stop_when_fields_decayed(2, mp.Ez, pt, 3e-1)])
        except Exception as e:  # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=run, args=(s,)) for s in sims]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    assert calls[0] == calls[1]
    return dict(t=sims[0].timestep, flux=o.flux(h), E=o.dft_data(h, 0), H=o.dft_data(h, 1),
                v=o.get_field(2, tuple(pt)), calls=calls[0])


def test_two_slabs_fields_decayed():
    _same(slabs_run((noop,)), slabs_run(()))
