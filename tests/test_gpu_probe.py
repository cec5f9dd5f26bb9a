"""Field probes: the series a probe records on the device, in every
stepping mode, is bit for bit what get_field returns after each step of a run that steps one
step per call (a -0.0 may read +0.0), and t_first names the step of the first value.

Grid: the smallest of the pair tests (test_gpu_tb.sc_tb: 9.6 x 6.4 x 8.0 at resolution 10, PML
0.7, the dielectric slab, the four sources, random initial fields); the slab runs use 9.6 x 6.4
x 9.6."""
import numpy as np
import pytest

from scenarios import GroupSim, GroupSim3, ProductSim, random_init, vol
from test_gpu_tb import SRCS, sc_tb

pytestmark = pytest.mark.gpu

COMPS = (0, 2, 4, 8, 9)  # Ex, Ez, Hy, Dz, Bx
CALLS = (1, 10, 7, 2, 20)
T = sum(CALLS)
SIZES = (9.6, 6.4, 8.0)
SLAB_SIZES = (9.6, 6.4, 9.6)
# L2 (the two-step region) is the PML-free box shrunk by two cells: |y| < 2.3, |z| < 3.1 here
POINTS = {
    "generic": (0.513, -0.287, 0.731),      # off-grid inside the two-step region: 8 weights
    "yee_ez": (1.0, 0.5, 0.25),             # exactly an Ez point: 1 weight
    "yee_ex": (1.05, 0.5, 0.3),             # exactly an Ex point
    "l2_edge_y": (0.31, -2.33, 1.02),       # neighbours on both sides of the L2 / rim border
    "l2_edge_y2": (0.31, -2.27, 1.02),
    "l2_edge_z": (0.33, 0.21, 3.08),
    "l2_edge_z2": (-1.17, 0.21, 3.13),
    "source": SRCS[0],
    "pml": (4.45, 0.12, -0.33),
    "low_wall_x": (-4.77, 0.33, 0.41),      # first cell: an H sample on the not-owned plane 0
    "low_wall_z": (0.3, 0.2, -3.97),
    "slab_face_2": (0.31, 0.27, 0.02),      # straddles z = 0 (two slabs of 48 cells)
    "slab_face_3": (0.31, 0.27, 1.62),      # straddles z = 1.6 (three slabs of 32 cells)
    "slab_face_3b": (-0.4, 0.1, -1.58),
    "outside": (5.5, 0.0, 0.0),             # all zeros
}
PROBES = [(c, name) for c in COMPS for name in sorted(POINTS)]


def _fields_of(o):
    return o._all() if hasattr(o, "_all") else [o._fields()]


def _add_probes(o, probes=PROBES, points=POINTS):
    hs = []
    for c, name in probes:
        h = [f.add_probe(c, points[name]) for f in _fields_of(o)]
        assert all(x == h[0] for x in h)
        hs.append(h[0])
    return hs


def _read(o, h):
    if hasattr(o, "_all"):
        out = o._par(lambda f: f.probe_read(h))  # collective: every rank gets the sum
        for t0, v in out[1:]:
            assert t0 == out[0][0] and np.array_equal(v, out[0][1])
        return out[0]
    return o._fields().probe_read(h)


def _reference(sizes, nsteps, probes=PROBES, points=POINTS, build=None):
    """Run A: one step per call, get_field after each step -> {probe: values[nsteps]}."""
    o = build() if build else sc_tb(ProductSim, sizes=sizes, steps=())
    out = {p: np.zeros(nsteps) for p in probes}
    for s in range(nsteps):
        o.step(1)
        for c, name in probes:
            out[(c, name)][s] = o.get_field(c, points[name])
    return out


@pytest.fixture(scope="module")
def ref():
    return _reference(SIZES, T + 3)


def _same_series(got, want, what):
    # bit for bit, except that a -0.0 may read +0.0
    assert got.shape == want.shape, what
    assert np.array_equal((got + 0.0).view(np.uint64), (want + 0.0).view(np.uint64)), (
        what, np.flatnonzero(got != want)[:5])


def _check_all(o, hs, want, probes=PROBES, t_first=1, lo=0, hi=T):
    for (c, name), h in zip(probes, hs):
        t0, v = _read(o, h)
        assert t0 == t_first, (c, name, t0)
        _same_series(v, want[(c, name)][lo:hi], (c, name))


def _run(make, sizes, probes=PROBES, fused=True, **kw):
    o = sc_tb(make, sizes=sizes, steps=(), **kw)
    if not fused:
        for f in _fields_of(o):
            f.set_fused(False)
    hs = _add_probes(o, probes)
    for n in CALLS:
        o.step(n)
    return o, hs


def test_reference_is_not_trivial(ref):
    for (c, name), v in ref.items():
        assert (name == "outside") == (not v.any()), (c, name)


def test_probe_unfused(ref):
    o, hs = _run(ProductSim, SIZES, fused=False)
    assert not o._fields().fused_active()
    _check_all(o, hs, ref)


def test_probe_fused_no_pairs(ref):
    o, hs = _run(ProductSim, SIZES, tb=False)
    assert o._fields().fused_active() and not o._fields().tb_info()["active"]
    _check_all(o, hs, ref)


def test_probe_pairs(ref):
    """Every probe; the first four have compact boxes, the others sample the mid set."""
    o, hs = _run(ProductSim, SIZES)
    assert o._fields().tb_info()["active"]
    _check_all(o, hs, ref)


COMPACT = [(2, "generic"), (4, "l2_edge_y"), (8, "source"), (9, "l2_edge_z")]


def test_probe_pairs_compact_boxes(ref):
    """Four probes: each gets a compact box in the pair plan."""
    o, hs = _run(ProductSim, SIZES, probes=COMPACT)
    assert o._fields().tb_info()["active"]
    _check_all(o, hs, ref, COMPACT)


def test_probe_pairs_without_compact_boxes(ref):
    o, hs = _run(ProductSim, SIZES, schedule=(("dft_cmp", 0),))
    assert o._fields().tb_info()["active"]
    _check_all(o, hs, ref)


def _four_flux(o):
    fr = [0.2, 0.25, 0.31]
    return [o.add_dft_flux([([-1.0, -1.0, z], [1.2, 0.9, z], 2, 1.0)], fr, 1)
            for z in (-1.05, 0.45, 1.55, 2.05)]


def test_probe_beside_four_flux_monitors(ref):
    """The monitors take the pair plan's compact boxes: the probes fall beyond them.  A probe
    moves no DFT handle and changes no DFT value."""
    o = sc_tb(ProductSim, sizes=SIZES, steps=())
    h0 = o._fields().add_probe(2, POINTS["generic"])
    flux = _four_flux(o)
    assert flux == [0, 1, 2, 3] and h0 >= 1 << 30
    hs = [h0] + _add_probes(o, COMPACT)
    for n in CALLS:
        o.step(n)
    assert o._fields().tb_info()["active"]
    _check_all(o, hs, ref, [(2, "generic")] + COMPACT)
    q = sc_tb(ProductSim, sizes=SIZES, steps=())
    assert _four_flux(q) == flux
    for n in CALLS:
        q.step(n)
    for h in flux:
        for which in (0, 1):
            assert np.array_equal(o.dft_data(h, which), q.dft_data(h, which))
        assert np.array_equal(o.flux(h), q.flux(h))
    with pytest.raises(RuntimeError, match="meep:.*probe"):
        o._fields().dft_get(h0, 0)
    with pytest.raises(RuntimeError, match="meep:.*probe"):
        o._fields().dft_scale(h0, 2.0)


@pytest.mark.parametrize("make", [GroupSim, GroupSim3], ids=["2slabs", "3slabs"])
def test_probe_slabs(make):
    """Each rank adds up the points it owns and the partial sums are added over the ranks, as
    get_field does on the same slabs (run A is stepped on them too: one rank would add the
    eight terms in one chain, which rounds differently)."""
    probes = [p for p in PROBES if p[1] in ("generic", "slab_face_2", "slab_face_3",
                                            "slab_face_3b", "low_wall_z", "pml", "outside")]
    want = _reference(None, T, probes, build=lambda: sc_tb(make, sizes=SLAB_SIZES, steps=()))
    o, hs = _run(make, SLAB_SIZES, probes=probes)
    _check_all(o, hs, want, probes)


def test_probe_read_in_halves_remove_and_restart(ref, tmp_path):
    probes = [(2, "generic"), (4, "pml")]
    o = sc_tb(ProductSim, sizes=SIZES, steps=())
    f = o._fields()
    hs = _add_probes(o, probes)
    o.step(1), o.step(10)
    _check_all(o, hs, ref, probes, 1, 0, 11)
    t0, v = f.probe_read(hs[0])
    assert t0 == 12 and v.size == 0  # nothing since the last read
    o.step(7), o.step(2), o.step(20)
    _check_all(o, hs, ref, probes, 12, 11, T)
    o.step(1)
    f.probe_reset(hs[0])
    f.remove_probe(hs[1])
    with pytest.raises(RuntimeError, match="bad probe handle"):
        f.probe_read(hs[1])
    o.step(1)
    t0, v = f.probe_read(hs[0])  # the other probe kept its handle
    assert t0 == T + 2
    _same_series(v, ref[probes[0]][T + 1:T + 2], "after reset")
    f.remove_probes()
    with pytest.raises(RuntimeError, match="bad probe handle"):
        f.probe_read(hs[0])
    h = f.add_probe(2, POINTS["generic"])  # starts at the current step
    o.step(1)
    t0, v = f.probe_read(h)
    assert t0 == T + 3
    _same_series(v, ref[probes[0]][T + 2:T + 3], "after remove_probes")
    # probes are not part of a dump: after load the probe is empty at the loaded step
    path = str(tmp_path / "state")
    o.dump(path)
    o.step(2)
    o.load(path)
    t0, v = f.probe_read(h)
    assert (t0, v.size) == (T + 4, 0)


def test_probe_removed_and_added_again_in_pairs(ref):
    """A probe removed and added again at the same point between calls that step in pairs: the
    pair plan must not keep the removed probe's compact box (freed with it), and the new probe
    must get one of its own -- every value bitwise get_field's, the middle states of the pairs
    included."""
    p = (2, "generic")
    o = sc_tb(ProductSim, sizes=SIZES, steps=())
    f = o._fields()
    h = f.add_probe(p[0], POINTS[p[1]])
    o.step(1), o.step(10)
    assert f.tb_info()["active"]
    _check_all(o, [h], ref, [p], 1, 0, 11)
    f.remove_probe(h)
    h = f.add_probe(p[0], POINTS[p[1]])
    o.step(7), o.step(2)
    assert f.tb_info()["active"]
    _check_all(o, [h], ref, [p], 12, 11, 20)
    f.remove_probes()
    h2 = f.add_probe(9, POINTS["source"])  # another box in the same place of the plan
    h = f.add_probe(p[0], POINTS[p[1]])
    o.step(20)
    assert f.tb_info()["active"]
    _check_all(o, [h, h2], ref, [p, (9, "source")], 21, 20, T)


def test_probe_overrun_report(ref, monkeypatch):
    """A series of 16 entries: a read delivers the last 16 steps and says which they are (the
    last flush holds more buffered rows than the series has entries)."""
    monkeypatch.setenv("MNL_PROBE_CAP", "16")
    probes = [(2, "generic"), (9, "source")]
    o, hs = _run(ProductSim, SIZES, probes=probes)
    _check_all(o, hs, ref, probes, T - 15, T - 16, T)
    o.step(3)
    _check_all(o, hs, ref, probes, T + 1, T, T + 3)


def _small(dim):
    def build():
        if dim == 2:
            o = vol(ProductSim, 2, [6.4, 4.8], 10, center_origin=True)
            o.add_pml(1.0)
            o.add_gaussian_source(2, 0.25, 4.0, 0.0, 40.0, (0.37, -0.21), 1.0)
            o.add_gaussian_source(0, 0.25, 4.0, 0.0, 40.0, (-1.3, 0.6), 0.8)
            random_init(o, (6, 7, 8, 9, 10, 11))
        else:
            o = vol(ProductSim, 1, [20.0], 10, center_origin=True)
            o.add_pml(1.0)
            o.add_gaussian_source(0, 0.25, 4.0, 0.0, 40.0, (0, 0, 0.37), 1.0)
            random_init(o, (6, 10))  # a 1-D cell has Ex, Dx, Hy, By
        o._fields().set_fused(False)
        return o
    return build


@pytest.mark.parametrize("dim", [2, 1])
def test_probe_2d_and_1d_unfused(dim):
    if dim == 2:
        assert _small(2)().shape() == (65, 49)
        points = {"generic": (0.513, -0.287), "yee": (1.0, 0.5), "low_wall": (-3.17, 0.33),
                  "pml": (2.9, 0.12), "outside": (9.0, 0.0)}
        comps = COMPS
    else:
        assert _small(1)().shape() == (201,)
        points = {"generic": (0, 0, 0.513), "yee": (0, 0, 1.05), "low_wall": (0, 0, -9.97),
                  "pml": (0, 0, 9.4), "outside": (0, 0, 12.0)}
        comps = (0, 4, 6, 10)  # Ex, Hy, Dx, By
    probes = [(c, n) for c in comps for n in sorted(points)]
    want = _reference(None, 30, probes, points, _small(dim))
    assert any(v.any() for v in want.values())
    o = _small(dim)()
    hs = _add_probes(o, probes, points)
    for n in (1, 10, 7, 2, 10):
        o.step(n)
    _check_all(o, hs, want, probes, 1, 0, 30)


def test_probe_periodic_seam():
    """A cell periodic in x and y (case 4 of periodic_cases) with probes half a pixel from the
    seam."""
    from periodic_cases import A, Scene, configure, product_makers
    maker = product_makers()[0]

    def build():
        sc = Scene(4, "plain", 1)
        return configure(sc.make(maker), sc)
    points = {"seam_x": (0.5 / A, 1.3, 2.1), "seam_xy": (24 / A - 0.5 / A, 0.5 / A, 1.7),
              "inside": (1.51, 1.27, 2.03)}
    probes = [(c, n) for c in COMPS for n in sorted(points)]
    want = _reference(None, 20, probes, points, build)
    assert all(v.any() for v in want.values())
    o = build()
    hs = _add_probes(o, probes, points)
    for n in (1, 10, 7, 2):
        o.step(n)
    _check_all(o, hs, want, probes, 1, 0, 20)
