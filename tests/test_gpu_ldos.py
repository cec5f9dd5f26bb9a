"""LDOS spectra on the device: core.Fields.add_ldos / ldos_update /
ldos_record / ldos_data / ldos_points and meep_nl_amd.dft_ldos against the restatement of
dft_ldos::update / ldos() in tests/ldos_ref.py.

The restatement is driven by the oracle's arrays, one step at a time, on the small cells (3-D 24 x
24 x 30 and 2-D 24 x 24 with PML 0.6 at resolution 10; the line source's cells are 66 cells
long).  A 3-D cell of that size steps fused but not in pairs (the smallest cell that pairs is
test_gpu_tb's 96 x 64 x 80), so the source layouts run once more on that cell, in pairs, against
the oracle-driven restatement (test_parity_in_pairs), and the mode test there shows that the
same run gives the same bits unfused, fused, in pairs and with explicit updates.

Currents: non-integrated custom sources, whose current(t, dt) is func(t) exactly.  Tolerance of
F and J: the project's accumulation bound (N + U + 64) 2^-53 sum|term| over N points and U
updates (ldos_ref.LdosRef.tol_F / tol_J); that of ldos follows from the two (tol_ldos)."""
import math

import numpy as np
import pytest

from ldos_ref import LdosRef, custom_current
from scenarios import GroupSim, GroupSim3, ProductSim, make_oracle, vol

pytestmark = pytest.mark.gpu

FREQS = (0.2, 0.3, 0.4)
STEPS = 70  # two flush blocks of 32 and a partial one (71 updates with the starting state's)
RES = 10


def _pulse(t):
    return math.exp(-((t - 1.5) / 0.6) ** 2) * math.cos(2 * math.pi * 0.3 * t)


def _pulse2(t):
    return 0.7 * math.exp(-((t - 2.0) / 0.5) ** 2) * math.sin(2 * math.pi * 0.25 * t)


def _camp(r):  # a complex amplitude function: A has both parts
    return complex(1.0 + 0.3 * r[0], 0.5 * r[1] - 0.2 * r[0] * r[1])


def _p(dim, x, y, z):
    return (x, y, z) if dim == 3 else (x, y)


# ---- the cases: name -> (cell sizes 3-D, cell sizes 2-D, sources(o, dim), first time function,
#      number of list points 3-D, 2-D)
def _src_on_grid(o, dim):
    o.add_custom_source(2, _pulse, 0.0, 1e9, _p(dim, 0.0, 0.0, 0.05), 0.8)


def _src_off_grid(o, dim):
    o.add_custom_source(2, _pulse, 0.0, 1e9, _p(dim, 0.113, -0.087, 0.131), 0.8)


def _src_line(o, dim):  # 65 Ez points along x: more than one wave
    o.add_custom_volume_source(2, _pulse, 0.0, 1e9, _p(dim, -3.2, 0.0, 0.05),
                               _p(dim, 3.2, 0.0, 0.05), 0.5)


def _src_plane(o, dim):  # 576 points, complex amplitudes
    if dim == 3:
        o.add_custom_volume_source(2, _pulse, 0.0, 1e9, (-1.2, -1.2, 0.05), (1.2, 1.2, 0.05),
                                   complex(0.4, 0.1), amp_func=_camp)
    else:
        o.add_custom_volume_source(2, _pulse, 0.0, 1e9, (-1.2, -1.2), (1.2, 1.2),
                                   complex(0.4, 0.1), amp_func=_camp)


def _src_e_and_h(o, dim):  # both lists, both phases; the H source keeps the step unfused
    o.add_custom_source(2, _pulse, 0.0, 1e9, _p(dim, 0.113, -0.087, 0.131), 0.8)
    o.add_custom_source(3, _pulse, 0.0, 1e9, _p(dim, -0.31, 0.22, 0.4), 0.6)  # Hx


def _src_two_times(o, dim):  # J follows the first
    o.add_custom_source(2, _pulse, 0.0, 1e9, _p(dim, 0.0, 0.0, 0.05), 0.8)
    o.add_custom_source(0, _pulse2, 0.0, 1e9, _p(dim, 0.33, -0.21, 0.27), 0.5)


BOX3, BOX2 = (2.4, 2.4, 3.0), (2.4, 2.4)
CASES = {
    "on_grid": (BOX3, BOX2, _src_on_grid, 1, 1),
    "off_grid": (BOX3, BOX2, _src_off_grid, 8, 4),
    "line65": ((6.6, 2.0, 2.0), (6.6, 2.0), _src_line, -65, -65),  # (at least)
    "plane576": (BOX3, BOX2, _src_plane, 576, 576),
    "e_and_h": (BOX3, BOX2, _src_e_and_h, 16, 8),
    "two_times": (BOX3, BOX2, _src_two_times, 9, 5),
}


def _cell(make, dim, sizes, sources):
    o = vol(make, dim, list(sizes), RES, center_origin=True)
    o.add_pml(0.6)
    if dim == 3:  # the fused step needs every component
        for c in range(6):
            o.require_component(c)
    sources(o, dim)
    return o


def _fields_of(o):
    return o._all() if hasattr(o, "_all") else [o._fields()]


def _add(o, freqs=FREQS):
    hs = [f.add_ldos(freqs) for f in _fields_of(o)]
    assert all(h == hs[0] for h in hs) and (1 << 29) <= hs[0] < (1 << 30)
    return hs[0]


def _each(o, fn):
    return [fn(f) for f in _fields_of(o)]


def _data(o, h):
    if hasattr(o, "_all"):
        out = o._par(lambda f: f.ldos_data(h))  # collective: every rank gets the same
        for d in out[1:]:
            for x, y in zip(d[:3], out[0][:3]):
                assert np.array_equal(x, y, equal_nan=True)
            assert d[3] == out[0][3]
        return out[0]
    return o._fields().ldos_data(h)


def _run_recorded(o, h, calls):
    """The updates of a run: the starting state's, then one after every step."""
    _each(o, lambda f: f.ldos_update(h))
    _each(o, lambda f: f.ldos_record(h, True))
    for n in calls:
        o.step(n)
    _each(o, lambda f: f.ldos_record(h, False))


def _restate(src, dim, points, func, steps=STEPS, freqs=FREQS):
    """src: an oracle (or a product that steps one step per call) with the same sources."""
    comp, ijk, amp = points
    nE = int(np.sum(comp < 3))
    ref = LdosRef(freqs, src.dt, RES, dim)
    for s in range(steps + 1):
        ref.update(src.t, src.get_array, points, nE, custom_current(func, src.t, src.dt))
        if s < steps:
            src.step(1)
    return ref


def _check(got, ref, what):
    ld, F, J, scale = got
    dF, dJ = np.abs(F - ref.F()), np.abs(J - ref.J())
    print(what, "max|dF|", dF.max(), "tol", ref.tol_F(), "max|dJ|", dJ.max(), "tol", ref.tol_J())
    assert np.all(np.abs(ref.F()) > 0) and np.all(np.abs(ref.J()) > 0), what
    assert np.all(dF <= ref.tol_F()), (what, dF, ref.tol_F())
    assert np.all(dJ <= ref.tol_J()), (what, dJ, ref.tol_J())
    # Jsum through overall_scale = -2 / (pi Jsum^2): N + 8 roundings of the sum and the formula
    rel = (ref.npoints + 8) * 2.0 ** -52
    assert math.isclose(scale, ref.overall_scale(), rel_tol=2 * rel), (what, scale)
    dl, tl = np.abs(ld - ref.ldos()), ref.tol_ldos()
    print(what, "max|dldos|", dl.max(), "tol", tl.max(), "ldos", ld)
    assert np.all(dl <= tl), (what, dl, tl)


# ------------------------------------------------------------------ 1. the point lists
def test_points_on_grid_off_grid_and_plane():
    for dim in (3, 2):
        o = _cell(ProductSim, dim, BOX3 if dim == 3 else BOX2, _src_on_grid)
        comp, ijk, amp = o._fields().ldos_points(_add(o))
        assert comp.tolist() == [2] and amp.tolist() == [0.8 * RES ** dim]  # A = amp a^dim
        assert ijk.tolist() == [[12, 12, 15 if dim == 3 else 0]]
        q = _cell(ProductSim, dim, BOX3 if dim == 3 else BOX2, _src_off_grid)
        comp, ijk, amp = q._fields().ldos_points(_add(q))
        assert len(comp) == 2 ** dim and set(comp.tolist()) == {2}
        assert len({tuple(r) for r in ijk.tolist()}) == 2 ** dim
        assert np.all(amp.imag == 0) and np.all(amp.real > 0)
        assert math.isclose(float(np.sum(amp.real)), 0.8 * RES ** dim, rel_tol=4 * 2.0 ** -52)
    o = _cell(ProductSim, 3, BOX3, _src_plane)
    comp, ijk, amp = o._fields().ldos_points(_add(o))
    assert len(comp) == 576 and set(comp.tolist()) == {2} and set(ijk[:, 2].tolist()) == {15}
    assert len({tuple(r) for r in ijk.tolist()}) == 576
    assert np.any(amp.imag != 0) and np.any(amp.real != 0)


@pytest.mark.parametrize("make", [GroupSim, GroupSim3], ids=["2slabs", "3slabs"])
def test_points_identical_on_slabs(make):
    one = _cell(ProductSim, 3, BOX3, _src_plane)
    want = one._fields().ldos_points(_add(one))
    o = _cell(make, 3, BOX3, _src_plane)
    h = _add(o)
    for got in _each(o, lambda f: f.ldos_points(h)):
        for x, y in zip(got, want):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------ 2-7. parity
@pytest.mark.parametrize("dim", [3, 2], ids=["3d", "2d"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_restatement(case, dim):
    """plane576: 576 slots = 288 pairs of slots, 128 pairs per workgroup of the reduce kernel:
    3 workgroups.  line65: 65 slots padded to 66, two waves of one workgroup."""
    box3, box2, sources, n3, n2 = CASES[case]
    sizes = box3 if dim == 3 else box2
    o = _cell(ProductSim, dim, sizes, sources)
    f = o._fields()
    h = _add(o)
    points = f.ldos_points(h)
    n = n3 if dim == 3 else n2
    assert len(points[0]) == n or (n < 0 and len(points[0]) >= -n), len(points[0])
    assert np.all(np.isnan(f.ldos_data(h)[0]))  # before any update (19.)
    _run_recorded(o, h, (1, STEPS - 1))
    if case == "e_and_h":
        assert not f.fused_active()
        assert sorted(set(points[0].tolist())) == [2, 3]
    elif dim == 3:
        assert f.fused_active()
    ref = _restate(_cell(make_oracle, dim, sizes, sources), dim, points, _pulse)
    _check(f.ldos_data(h), ref, (case, dim))


# ------------------------------------------------------------------ 8. modes
PAIR_BOX = (9.6, 6.4, 8.0)


def _src_pair_cell(o, dim):
    # an off-grid dipole and a plane of about 31 x 31 points (4 workgroups of the reduce kernel),
    # inside the two-step region
    o.add_custom_source(2, _pulse, 0.0, 1e9, (0.37, -0.21, 0.05), 0.8)
    o.add_custom_volume_source(0, _pulse, 0.0, 1e9, (-1.45, -1.5, 0.3), (1.55, 1.5, 0.3),
                               complex(0.2, 0.05), amp_func=_camp)


def _mode_run(mode):
    o = _cell(ProductSim, 3, PAIR_BOX, _src_pair_cell)
    f = o._fields()
    if mode == "unfused":
        f.set_fused(False)
    if mode == "fused":
        f.set_temporal_blocking(False)
    h = _add(o)
    reads = []
    if mode in ("unfused", "fused", "pairs"):
        _run_recorded(o, h, (1, STEPS - 1))
    elif mode == "steps_of_one":
        _run_recorded(o, h, (1,) * STEPS)
    elif mode == "explicit":
        f.ldos_update(h)
        for _ in range(STEPS):
            o.step(1)
            f.ldos_update(h)
    elif mode == "reads":
        f.ldos_update(h)
        f.ldos_record(h, True)
        for n in (1, 30, 1, 1, STEPS - 33):
            o.step(n)
            reads.append(f.ldos_data(h))
    if mode == "unfused":
        assert not f.fused_active()
    if mode == "fused":
        assert f.fused_active() and not f.tb_info()["active"]
    if mode in ("pairs", "reads"):
        assert f.tb_info()["active"]
    return f.ldos_data(h), reads, f.ldos_points(h)


@pytest.fixture(scope="module")
def pairs_run():
    return _mode_run("pairs")


@pytest.mark.parametrize("mode", ["unfused", "fused", "steps_of_one", "explicit", "reads"])
def test_modes_bit_for_bit(pairs_run, mode):
    want = pairs_run[0]
    got, reads, _ = _mode_run(mode)
    for x, y in zip(got[:3], want[:3]):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y), (mode, x, y)
    assert got[3] == want[3]
    if mode == "reads":  # read at steps 31, 32 and 33: the running sums, none lost or doubled
        assert len(reads) == 5 and np.array_equal(reads[-1][1], want[1])
        assert not np.array_equal(reads[1][1], reads[2][1])


def test_pair_cell_against_restatement(pairs_run):
    """The restatement on the arrays of a product run that steps one step per call (the
    product's arrays are the oracle's bit for bit, test_gpu_tb)."""
    got, _, points = pairs_run
    assert len(points[0]) > 8 + 768  # more than three workgroups of 256 slots
    src = _cell(ProductSim, 3, PAIR_BOX, _src_pair_cell)
    ref = _restate(src, 3, points, _pulse)
    _check(got, ref, "pair cell")


@pytest.mark.parametrize("case", ["on_grid", "off_grid", "line65", "plane576", "two_times"])
def test_parity_in_pairs(case):
    """The source layouts of the parity cases on the cell that steps in pairs, against the
    restatement driven by the oracle's arrays (e_and_h keeps the step unfused, so it has no
    pairs to run in)."""
    sources = CASES[case][2]
    o = _cell(ProductSim, 3, PAIR_BOX, sources)
    f = o._fields()
    h = _add(o)
    points = f.ldos_points(h)
    _run_recorded(o, h, (1, STEPS - 1))
    assert f.fused_active() and f.tb_info()["active"]
    ref = _restate(_cell(make_oracle, 3, PAIR_BOX, sources), 3, points, _pulse)
    _check(f.ldos_data(h), ref, (case, "pairs"))


# ------------------------------------------------------------------ 9-12. Simulation
def _pulse0(t):
    # odd about t = 1.5, a sample time of both the B and the D currents: no net charge is left
    # behind, so the field decays instead of settling on a static one
    return math.exp(-((t - 1.5) / 0.5) ** 2) * math.sin(2 * math.pi * 0.8 * (t - 1.5))


def _sim(func=_pulse, end=4.0):
    import meep_nl_amd as mp
    return mp, mp.Simulation(
        cell_size=mp.Vector3(*BOX3), resolution=RES, boundary_layers=[mp.PML(0.6)],
        sources=[mp.Source(mp.CustomSource(func, start_time=0.0, end_time=end), mp.Ez,
                           center=mp.Vector3(0.0, 0.0, 0.05), amplitude=0.8)])


def _count_steps(sim):
    sim.init_sim()
    calls = []
    step = sim.fields.step

    def counted(n=1):
        calls.append(n)
        return step(n)
    sim.fields.step = counted
    return calls


def _results(sim):
    return (np.array(sim.ldos_data), np.array(sim.ldos_Fdata), np.array(sim.ldos_Jdata),
            sim.ldos_scale)


def _same_results(a, b):
    for x, y in zip(a[:3], b[:3]):
        assert np.all(np.isfinite(x)) and np.array_equal(x, y), (x, y)
    assert a[3] == b[3]


def test_simulation_run_is_batched_and_equals_one_step_loop(capsys):
    mp, sim = _sim()
    calls = _count_steps(sim)
    sim.run(mp.dft_ldos(0.3, 0.2, 3), until=3.0)
    assert sim.batched_runs == 1 and len(calls) < 8 and sum(calls) == 60, calls
    out = capsys.readouterr().out
    assert len([l for l in out.splitlines() if l.startswith("ldos0:, ")]) == 3
    mp, one = _sim()
    calls1 = _count_steps(one)
    one.run(mp.dft_ldos(0.3, 0.2, 3), lambda s: None, until=3.0)
    assert one.batched_runs == 0 and calls1 == [1] * 60
    _same_results(_results(sim), _results(one))
    # wrapped, the object is an ordinary step function of the one-step loop
    mp, wrapped = _sim()
    calls2 = _count_steps(wrapped)
    wrapped.run(mp.at_every(0.0, mp.dft_ldos(0.3, 0.2, 3)), until=3.0)
    assert wrapped.batched_runs == 0 and calls2 == [1] * 60
    _same_results(_results(sim), _results(wrapped))


def test_simulation_decay_stopped_run_is_batched():
    res, steps = [], []
    for extra in ((), (lambda s: None,)):
        mp, sim = _sim(_pulse0, 3.0)
        calls = _count_steps(sim)
        cond = mp.stop_when_fields_decayed(1.0, mp.Ez, mp.Vector3(0.3, 0.2, 0.15), 1e-2)
        # (the number only bounds the run: 20 time units after the sources, 460 steps in all)
        sim.run(mp.dft_ldos(0.8, 0.4, 3), *extra, until_after_sources=[cond, 20.0])
        assert sim.batched_runs == (0 if extra else 1)
        assert (max(calls) == 1) == bool(extra), calls
        res.append(_results(sim))
        steps.append(sim.fields.t)
    assert steps[0] == steps[1] and 60 < steps[0] < 460, steps  # the decay stopped it
    _same_results(res[0], res[1])


def test_simulation_second_run_counts_the_boundary_state_twice():
    """Two runs on one Ldos: the state between them is updated by the first run's last update
    and by the second run's first, as in the reference.  The restatement does the same on the
    arrays of a one-step-loop run."""
    mp, sim = _sim()
    ld = mp.Ldos(0.3, 0.2, 3)
    sim.run(mp.dft_ldos(ldos=ld), until=1.0)
    sim.run(mp.dft_ldos(ldos=ld), until=1.0)
    assert sim.batched_runs == 2 and sim.fields.t == 40
    points = sim.fields.ldos_points(ld._handle)
    mp, src = _sim()
    src.init_sim()
    ref = LdosRef(mp.get_ldos_freqs(ld), src.fields.dt, RES, 3)

    def update(s):
        t = s.fields.t
        ref.update(t, s.fields.get_array, points, 1,
                   custom_current(_pulse, t, s.fields.dt, 0.0, 4.0))
    src.run(update, until=1.0)
    src.run(update, until=1.0)
    assert ref.updates == 42
    _check(_results(sim), ref, "two runs")


# ------------------------------------------------------------------ known answer
def test_purcell_factor_of_planar_cavity():
    """The reference's own test_ldos_3D (python/tests/test_ldos.py:97-183, 411-437): the Purcell
    factor of a dipole parallel to the lossless metallic walls of a planar cavity 0.75
    wavelengths thick against the bulk medium, theory 1.444 (Abram et al., eq. 7), delta 0.1.
    Its parameters (resolution 25, n = 2.4, PML 0.5, Gaussian fwidth 0.2, decay 1e-8 checked
    every 20) on the full cell without the mirror symmetries, with L reduced from 6 to 1 so
    that the CPU oracle could run it: 50^3 and 50 x 50 x 8 cells.  tests/golden/
    ldos_purcell.json holds the two ldos values the restatement (tests/ldos_ref.py) gave on the
    CPU oracle stepped one step at a time, with the step counts at which the runs stopped."""
    import json
    import os
    mp = __import__("meep_nl_amd")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                           "ldos_purcell.json")) as fh:
        gold = json.load(fh)
    L, dpml, n, res = gold["L"], 0.5, 2.4, 25
    sxy = L + 2 * dpml
    got = {}
    for which, sz, pml in (("bulk", sxy, [mp.PML(dpml)]),
                           ("cavity", 0.75 * 1.0 / n, [mp.PML(dpml, direction=mp.X),
                                                       mp.PML(dpml, direction=mp.Y)])):
        sim = mp.Simulation(resolution=res, cell_size=mp.Vector3(sxy, sxy, sz),
                            boundary_layers=pml, default_material=mp.Medium(index=n),
                            sources=[mp.Source(mp.GaussianSource(1.0, fwidth=0.2),
                                               component=mp.Ex, center=mp.Vector3())])
        sim.run(mp.dft_ldos(1.0, 0, 1),
                until_after_sources=mp.stop_when_fields_decayed(20, mp.Ex, mp.Vector3(), 1e-8))
        assert sim.batched_runs == 1, which
        assert sim.fields.t == gold["steps_" + which], (which, sim.fields.t)
        got[which] = sim.ldos_data[0]
        rel = abs(got[which] - gold["ldos_" + which]) / abs(gold["ldos_" + which])
        print("purcell", which, got[which], "recorded", gold["ldos_" + which], "rel", rel)
        assert rel <= 1e-9, (which, got[which], gold["ldos_" + which])
    c = 0.75
    theory = 3 * np.fix(c + 0.5) / (4 * c) + (4 * np.fix(c + 0.5) ** 3 - np.fix(c + 0.5)) / (
        16 * c ** 3)
    ratio = got["cavity"] / got["bulk"]
    print("purcell ratio", ratio, "theory", theory)
    assert abs(theory - 1.444) < 1e-3 and abs(ratio - theory) <= 0.1, (ratio, theory)


# ------------------------------------------------------------------ 13. ranks
def _src_xz_plane(o, dim):  # 24 x 19 Ez points at y = 0, -1.45 <= z <= 0.35
    o.add_custom_volume_source(2, _pulse, 0.0, 1e9, (-1.2, 0.0, -1.45), (1.2, 0.0, 0.35),
                               complex(0.4, 0.1), amp_func=_camp)


@pytest.fixture(scope="module")
def one_rank_plane():
    o = _cell(ProductSim, 3, BOX3, _src_xz_plane)
    h = _add(o)
    points = o._fields().ldos_points(h)
    _run_recorded(o, h, (1, STEPS - 1))
    ref = _restate(_cell(make_oracle, 3, BOX3, _src_xz_plane), 3, points, _pulse)
    return o._fields().ldos_data(h), ref


@pytest.mark.parametrize("make", [GroupSim, GroupSim3], ids=["2slabs", "3slabs"])
def test_slabs_agree_with_one_rank(one_rank_plane, make):
    """z-slabs of 15 / 10 cells: the plane's points lie in both slabs / in the lower two of
    three, the third owns none.  Each rank's F is a sub-sum of the one-rank sum: the same
    accumulation bound."""
    one, ref = one_rank_plane
    _check(one, ref, "one rank")
    o = _cell(make, 3, BOX3, _src_xz_plane)
    h = _add(o)
    owned = []
    for f in o._all():
        comp, ijk, amp = f.ldos_points(h)
        lo, hi = f.rank * 30 // f.nranks, (f.rank + 1) * 30 // f.nranks
        owned.append(int(np.sum((ijk[:, 2] >= lo) & (ijk[:, 2] < hi))))
    assert sum(owned) == len(comp) and (min(owned) == 0) == (make is GroupSim3), owned
    _run_recorded(o, h, (1, STEPS - 1))
    got = _data(o, h)
    _check(got, ref, make.__name__)
    assert np.array_equal(got[2], one[2]) and got[3] == one[3]  # J and Jsum: the same everywhere
    assert np.all(np.abs(got[1] - one[1]) <= 2 * ref.tol_F())


# ------------------------------------------------------------------ 15-19
def test_sources_changed_mid_run():
    """remove_sources + another source after 30 steps: the rows buffered until then are
    accumulated with the old list, later updates use the new one (and the new first source)."""
    def build():
        return _cell(ProductSim, 3, BOX3, _src_off_grid)

    def change(o):
        f = o._fields()
        f.remove_sources()
        f.add_custom_source(0, _pulse2, 0.0, 1e9, (0.33, -0.21, 0.27), 0.5)
    o = build()
    f = o._fields()
    h = _add(o)
    p_old = f.ldos_points(h)
    _run_recorded(o, h, (1, 29))
    change(o)
    p_new = f.ldos_points(h)
    assert len(p_old[0]) == 8 and set(p_new[0].tolist()) == {0}
    f.ldos_record(h, True)
    o.step(40)
    got = f.ldos_data(h)
    src = build()
    ref = LdosRef(FREQS, src.dt, RES, 3)
    for s in range(STEPS + 1):
        # (the state after 30 steps was recorded before the change)
        pts, fn = (p_old, _pulse) if s <= 30 else (p_new, _pulse2)
        ref.update(src.t, src.get_array, pts, len(pts[0]), custom_current(fn, src.t, src.dt))
        if s == 30:
            change(src)
        if s < STEPS:
            src.step(1)
    _check(got, ref, "sources changed")


def test_remove_bad_handle_complex_and_nan():
    o = _cell(ProductSim, 3, BOX3, _src_on_grid)
    f = o._fields()
    h1, h2 = f.add_ldos(FREQS), f.add_ldos([0.3])
    assert h2 == h1 + 1
    assert np.all(np.isnan(f.ldos_data(h1)[0])) and f.ldos_data(h1)[3] == -2.0 / math.pi
    f.ldos_record(h1, True), f.ldos_record(h2, True)
    o.step(1), o.step(4)
    f.remove_ldos(h1)  # rows still buffered
    with pytest.raises(RuntimeError, match="bad ldos handle"):
        f.ldos_data(h1)
    with pytest.raises(RuntimeError, match="bad ldos handle"):
        f.ldos_update(h1)
    with pytest.raises(RuntimeError, match="bad ldos handle"):
        f.ldos_record(5, True)
    with pytest.raises(RuntimeError, match="bad dft handle"):
        f.dft_get(h2, 0)
    o.step(3)
    ld, F, J, _ = f.ldos_data(h2)  # the other object kept its handle
    assert F.shape == (1,) and np.all(np.isfinite(ld)) and abs(F[0]) > 0
    f.remove_ldoses()
    with pytest.raises(RuntimeError, match="bad ldos handle"):
        f.ldos_data(h2)
    o.step(2)
    c = vol(ProductSim, 3, list(BOX3), RES, center_origin=True)
    c._fields().use_complex_fields()
    with pytest.raises(RuntimeError, match="add_ldos is not supported on complex fields"):
        c._fields().add_ldos(FREQS)
