"""CPU checks of the DFT energy / force feature: the C-ABI entries in the header and the ctypes
table, the argument handling of Simulation.add_force / add_energy against a stub fields object,
the numpy weight restatement of tests/dft_restate.py against hand-computed weights, and the
run table of the pair sums as a stand-alone program built with the address and
undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import dft_restate as R
import meep_nl_amd as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mnl_fields_add_dft_energy", "mnl_fields_add_dft_force", "mnl_fields_dft_energy",
       "mnl_fields_dft_force", "mnl_fields_dft_points", "mnl_fields_dft_list_size"]


def test_abi_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "meep_nl_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from meep_nl_amd import _lib
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*mnl_fields\s*\*", code), name
        assert name in _lib.exported_symbols(), name
    for name, src in zip(NEW[:4], ("src/dft.cpp:701-727", "src/stress.cpp:153-191",
                                   "src/dft.cpp:657-699", "src/stress.cpp:90-114")):
        doc = hdr[:hdr.index("int " + name)]
        assert src in doc[doc.rindex("/*"):], name  # the entry cites the reference lines
    assert re.search(r"mnl_fields_dft_points\([^)]*int which,\s*double \*out,\s*long long n\)", code)
    for name in ("add_dft_energy", "add_dft_force", "dft_energy", "dft_force", "dft_points"):
        assert callable(getattr(mp.Fields, name))


class StubFields:
    nranks = 1

    def __init__(self):
        self.added = []

    def add_dft_force(self, regs, freqs, decimation):
        self.added.append(("force", regs, list(freqs), decimation))
        return 3

    def add_dft_energy(self, regs, freqs, decimation):
        self.added.append(("energy", regs, list(freqs), decimation))
        return 4

    def dft_force(self, h):
        return np.array([h + 0.5, -1.0])

    def dft_energy(self, h, which):
        return np.array([1.0, 2.0]) * (1 + which if which < 2 else 3)

    def dft_get(self, h, which):
        return np.full(2, h + 1j * which)


def stub_sim(dims=3):
    size = mp.Vector3(4, 4, 4) if dims == 3 else mp.Vector3(4, 4)
    sim = mp.Simulation(cell_size=size, resolution=10)
    sim.fields = StubFields()
    sim.init_sim = lambda: None  # the stub stands for initialised fields
    return sim


def test_add_force_argument_forms():
    r = mp.ForceRegion(mp.Vector3(y=1.27), direction=mp.Y, size=mp.Vector3(4.38), weight=-2.0)
    assert isinstance(r, mp.FluxRegion) and r.direction == mp.Y and r.weight == -2.0
    sim = stub_sim()
    f = sim.add_force(0.3, 0.2, 5, r, mp.ForceRegion(volume=mp.Volume(mp.Vector3(0.5),
                                                                     size=mp.Vector3(0, 1, 2)),
                                                     direction=mp.X), decimation_factor=3)
    assert isinstance(f, mp.DftForce) and f.handle == 3 and f in sim.dft_objects
    kind, regs, freqs, dec = sim.fields.added[0]
    assert kind == "force" and dec == 3
    np.testing.assert_allclose(freqs, np.linspace(0.2, 0.4, 5))
    assert mp.get_force_freqs(f) == freqs
    assert regs[0] == ([-2.19, 1.27, 0.0], [2.19, 1.27, 0.0], 1, -2.0)
    assert regs[1] == ([0.5, -0.5, -1.0], [0.5, 0.5, 1.0], 0, 1.0)
    assert mp.get_forces(f) == [3.5, -1.0] and f.force() == [3.5, -1.0]
    lst = sim.add_force([0.1, 0.15], r)  # the frequency-list form, automatic decimation
    assert lst.freq == [0.1, 0.15] and sim.fields.added[1][3] == 0
    assert sim.add_force(0.25, 0, 1, r).freq == [0.25]
    d = sim.get_force_data(f)
    assert isinstance(d, mp.ForceData) and d._fields == ("offdiag1", "offdiag2", "diag")
    assert [v[0] for v in d] == [3 + 0j, 3 + 1j, 3 + 2j]
    with pytest.raises(RuntimeError, match="meep: NO_DIRECTION dft_force is invalid"):
        sim.add_force(0.3, 0, 1, mp.ForceRegion(mp.Vector3(), size=mp.Vector3(1, 1)))
    with pytest.raises(NotImplementedError, match="complex force weights"):
        sim.add_force(0.3, 0, 1, mp.ForceRegion(mp.Vector3(), direction=mp.X, weight=1j))
    with pytest.raises(TypeError):
        sim.add_force("0.3", r)
    two = stub_sim(2)  # a 2-D cell: z is dropped
    two.add_force(1.0, 0, 1, mp.ForceRegion(mp.Vector3(0.1, 0.2, 0.7), direction=mp.X,
                                            size=mp.Vector3(0, 1, 5)))
    assert two.fields.added[0][1][0] == ([0.1, -0.3, 0.0], [0.1, 0.7, 0.0], 0, 1.0)


def test_add_energy_argument_forms(capsys):
    r = mp.EnergyRegion(mp.Vector3(0.1), size=mp.Vector3(1, 2, 0.5), weight=7.0)
    sim = stub_sim()
    e = sim.add_energy(0.5, 0.5, 2, r, decimation_factor=2)
    assert isinstance(e, mp.DftEnergy) and e.handle == 4 and e in sim.dft_objects
    kind, regs, freqs, dec = sim.fields.added[0]
    assert kind == "energy" and dec == 2 and freqs == [0.25, 0.75]
    assert regs == [([-0.4, -1.0, -0.25], [0.6, 1.0, 0.25], 0, 7.0)]
    assert mp.get_energy_freqs(e) == [0.25, 0.75]
    assert mp.get_electric_energy(e) == [1.0, 2.0]
    assert mp.get_magnetic_energy(e) == [2.0, 4.0]
    assert mp.get_total_energy(e) == [3.0, 6.0]
    sim.display_electric_energy(e)
    sim.display_total_energy(e, e)
    out = capsys.readouterr().out
    assert "electric_energy0:, 0.25, 1.0" in out and "total_energy0:, 0.75, 6.0, 6.0" in out
    with pytest.raises(NotImplementedError, match="complex energy weights"):
        sim.add_energy(0.3, 0, 1, mp.EnergyRegion(mp.Vector3(), weight=1j))
    # an object of a simulation that was reset refuses to read
    e.handle = None
    with pytest.raises(RuntimeError, match="meep:.*reset"):
        e.total()


def test_weight_restatement_by_hand():
    a = 10.0
    # long region on the centred grid (points at odd half-pixel coordinates): [0.12, 0.58] has
    # points 0.05 .. 0.65, the first and last weight quadratic in the overlap with the edge pixel
    i0, w, br = R.boundary_weights_1d(0.12, 0.58, a, 1)
    assert (i0, len(w), br) == (1, 7, 0)
    np.testing.assert_allclose(w, [0.3 ** 2 / 2, 1 - 0.7 ** 2 / 2, 1, 1, 1, 1 - 0.7 ** 2 / 2,
                                   0.3 ** 2 / 2], rtol=0, atol=1e-14)
    assert abs(w.sum() / a - 0.46) < 1e-14  # the weights integrate 1 over the region
    # three points: the middle one loses to both edges
    i0, w, br = R.boundary_weights_1d(0.12, 0.18, a, 1)
    assert (i0, len(w), br) == (1, 3, 1)
    np.testing.assert_allclose(w, [0.3 ** 2 / 2, 1 - 0.7 ** 2 / 2 - 0.7 ** 2 / 2, 0.3 ** 2 / 2],
                               rtol=0, atol=1e-14)
    assert abs(w.sum() / a - 0.06) < 1e-14
    # an empty extent: linear interpolation between the two neighbours
    i0, w, br = R.boundary_weights_1d(0.12, 0.12, a, 1)
    assert (i0, len(w), br) == (1, 2, 2)
    np.testing.assert_allclose(w, [0.3, 0.7], rtol=0, atol=1e-14)
    # under one pixel between two points
    i0, w, br = R.boundary_weights_1d(0.07, 0.11, a, 1)
    assert (i0, len(w), br) == (1, 2, 3)
    np.testing.assert_allclose(w, [0.8 ** 2 / 2 - 0.4 ** 2 / 2, 0.6 ** 2 / 2 - 0.2 ** 2 / 2],
                               rtol=0, atol=1e-14)
    assert abs(w.sum() / a - 0.04) < 1e-14
    # loop_weights: the product over the directions times dV, at shuffled points; the Yee grid
    # of Ex is shifted along x only
    lo, hi = [0.12, -0.2, 0.33], [0.58, 0.2, 0.33]
    for comp in (None, R.EX):
        ax = []
        for d in range(3):
            sh = 1 if comp is None else R.shift(comp, d)
            j0, wd, _ = R.boundary_weights_1d(lo[d], hi[d], a, sh)
            ax.append(((j0 + 2 * np.arange(len(wd))) * (0.5 / a), wd))
        g = np.stack(np.meshgrid(*[x for x, _ in ax], indexing="ij"), -1).reshape(-1, 3)
        wg = np.einsum("i,j,k->ijk", *[w for _, w in ax]).ravel() / a ** 2
        perm = np.random.default_rng(3).permutation(len(g))
        got = R.loop_weights(g[perm], lo, hi, a, comp)
        np.testing.assert_allclose(got, wg[perm], rtol=1e-15, atol=0)
        assert abs(got.sum() - 0.46 * 0.4) < 1e-14  # the area of the surface
    s, S, n = R.pair_sum(np.array([1 + 2j, 3j]), np.array([2 - 1j, 1 + 1j]), [0.5, -2.0], 1)
    assert (s[0], S[0], n) == (0.5 * 0.0 + -2.0 * 3.0, 6.0, 2)


def test_pair_run_table_under_sanitizers(tmp_path):
    """The zip of two chunk lists into slot runs (mnl_pair_runs.hpp) as a stand-alone program
    with its own main, built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "pair_runs")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "meep_nl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "pair_runs_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
