"""Periodic boundaries (fields::use_bloch with k = 0, real fields) on the GPU.

A, B: a periodic cell against the CPU oracle on a metal-walled supercell of 3 replicas per
periodic axis, bit for bit on every array of the central replica with its ghost planes, for
step counts inside the light-cone bound s * T <= m - 2 (tests/periodic_cases.py; the bound is
checked on the oracle alone by tests/test_periodic_cpu.py).  C: product against product over
300 steps, past that horizon.  D: DFT monitors.  E: in-process slabs.  F: plumbing.

One rank steps periodic 3-D runs in the fused mode wherever a metal run
of the same content would: every such case asserts that mode through mnl_fields_mode right
after stepping, and is repeated with set_fused(0) and with one step per call and reads in
between (a read leaves the fused mode, the next step enters it again), bitwise equal."""
import numpy as np
import pytest

import periodic_cases as pc
from dft_restate import U

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

FREQS = [0.6, 0.8, 1.0]


def _arrays(o):
    return {c: o.get_array(c) for c in pc.ALL_COMPS}


def _same(a, b, what):
    for c in pc.ALL_COMPS:
        assert a[c].shape == b[c].shape, (what, c)
        assert np.array_equal(a[c], b[c]), (what, c, float(np.max(np.abs(a[c] - b[c]))))


def _mode(o):
    fs = o._all() if hasattr(o, "_all") else [o._fields()]
    return [int(f.fused_active()) for f in fs]


# ---------------------------------------------------------------- A. supercell parity, 3-D
@pytest.mark.parametrize("case", [1, 2, 3, 4, 5])
def test_supercell_parity(case):
    T = pc.steps_bound(case, 3, "plain")
    want = pc.oracle_central(case, "plain", T)
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)
    sc, p = pc.run_product(case, "plain", T)
    assert [p._fields().boundary(d) for d in range(3)] == \
        ["periodic" if d in sc.per else "metallic" for d in range(3)]
    assert _mode(p) == [1]  # the fused step (queried before any read)
    got = _arrays(p)
    _same(got, want, "T steps, fused")
    # one step at a time with reads in between: in and out of the fused mode at every step
    _, q = pc.run_product(case, "plain", T, chunks=[1] * T)
    _same(_arrays(q), got, "one step per call")
    _, q = pc.run_product(case, "plain", T, chunks=[2, 1, T - 3])
    _same(_arrays(q), got, "ragged split")
    _, q = pc.run_product(case, "plain", T, before=lambda o: o._fields().set_fused(False))
    assert _mode(q) == [0]
    _same(_arrays(q), got, "set_fused(0)")


def test_supercell_parity_after_every_step():
    """Case 5 (all three axes periodic): equal to the oracle after each single step."""
    T = pc.steps_bound(5, 3, "plain")
    sc = pc.Scene(5, "plain", 1)
    p = pc.configure(sc.make(pc.product_makers()[0]), sc)
    for t in range(1, T + 1):
        p.step(1)
        assert _mode(p) == [int(t > 1)]  # the first step runs unfused (the lazy copies)
        _same(_arrays(p), pc.oracle_central(5, "plain", t), "step %d" % t)


# ---------------------------------------------------------------- B. families on case 4's cell
@pytest.mark.parametrize("family", [f for f in pc.FAMILIES if f != "plain"])
def test_family_parity(family):
    T = pc.steps_bound(4, 3, family)
    want = pc.oracle_central(4, family, T)
    _, p = pc.run_product(4, family, T)
    # a Lorentzian slab steps fused (polarization chunks in the general kernel); the other
    # families have no fused step in any cell
    assert _mode(p) == [int(family == "lorentz")]
    got = _arrays(p)
    _same(got, want, family)
    _, q = pc.run_product(4, family, T, chunks=[1] * T)
    _same(_arrays(q), got, family + ", one step per call")
    if family == "lorentz":
        _, q = pc.run_product(4, family, T, before=lambda o: o._fields().set_fused(False))
        assert _mode(q) == [0]
        _same(_arrays(q), got, family + ", set_fused(0)")


def test_parity_2d():
    """TM and TE together, x periodic with y PML."""
    T = pc.steps_bound("2d", 3, "plain")
    want = pc.oracle_central("2d", "plain", T)
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)
    _, p = pc.run_product("2d", "plain", T)
    _same(_arrays(p), want, "2-D")


# ---------------------------------------------------------------- C. long-time properties
LONG = 300


@pytest.fixture(scope="module")
def long_base():
    sc, p = pc.run_product(4, "lorentz", LONG, planar_comp=2)
    assert _mode(p) == [1]
    base = _arrays(p)
    _, q = pc.run_product(4, "lorentz", LONG, planar_comp=2,
                          before=lambda o: o._fields().set_fused(False))
    assert _mode(q) == [0]
    _same(_arrays(q), base, "300 steps, fused against unfused")
    return sc, base


def test_replication(long_base):
    """A period of n against a period of 2 n holding the content twice."""
    sc, base = long_base
    s2, p2 = pc.run_product(4, "lorentz", LONG, R=2, planar_comp=2)
    for c in pc.ALL_COMPS:
        big = p2.get_array(c)
        assert np.any(base[c] != 0)
        for j0 in (0, sc.n[0]):
            for j1 in (0, sc.n[1]):
                blk = big[j0:j0 + sc.n[0] + 1, j1:j1 + sc.n[1] + 1]
                assert np.array_equal(blk, base[c]), (c, j0, j1)


def test_translation(long_base):
    """Everything moved cyclically by (-1, 3) cells: the fields move with it.  The point source
    lands on the seam plane, so its points come from the image chunk, and the planar source's
    period sticks out of the cell on both axes, so the lattice-shift loop folds it back."""
    sc, base = long_base
    tr = (-1, 3, 0)
    _, pt = pc.run_product(4, "lorentz", LONG, trans=tr, planar_comp=2)
    for c in pc.ALL_COMPS:
        got = pt.get_array(c)
        want = base[c]
        for k, d in enumerate((0, 1)):
            want = np.take(want, (np.arange(sc.n[d] + 1) - tr[d]) % sc.n[d], axis=k)
        assert np.array_equal(got, want), (c, float(np.max(np.abs(got - want))))


# ---------------------------------------------------------------- D. monitors on case 4
def _monitor_run(maker_obj, sc, T, chunks=None, fused=True):
    o = pc.configure(maker_obj, sc)
    if not fused:
        o._fields().set_fused(False)
    # strictly inside the cell of the central replica
    lo = [3 / pc.A, 4 / pc.A, 8 / pc.A]
    hi = [(sc.n[0] - 3) / pc.A, (sc.n[1] - 5) / pc.A, 20 / pc.A]
    hf = o.add_dft_fields([0, 1, 2, 4], lo, hi, FREQS)
    # a full-period flux plane, normal z
    z = 22 / pc.A
    hx = o.add_dft_flux([([0.0, 0.0, z], [sc.L[0], sc.L[1], z], 2, 1.0)], FREQS, 1)
    for k in (chunks or [T]):
        o.step(k)
    return o, hf, hx


def test_monitors():
    T = pc.steps_bound(4, 3, "plain")
    s3 = pc.Scene(4, "plain", 3)
    from scenarios import make_oracle
    o, ohf, ohx = _monitor_run(s3.make(make_oracle), s3, T)
    s1 = pc.Scene(4, "plain", 1)
    p, phf, phx = _monitor_run(s1.make(pc.product_makers()[0]), s1, T)
    assert _mode(p) == [1]
    for c in (0, 1, 2, 4):
        for k in range(len(FREQS)):
            a, b = p.dft_array(phf, c, k), o.dft_array(ohf, c, k)
            assert a.shape == b.shape and np.any(b != 0)
            assert np.array_equal(a, b), (c, k)
    # positions and weights of the flux plane's lists against the numpy restatement: every
    # point of the plane's centred grid once over the period, image chunks included
    from dft_restate import check_weights, loop_weights
    f = p._fields()
    for which in (0, 1):
        pts = f.dft_points(phx, which)
        lo, hi = [0.0, 0.0, 22 / pc.A], [s1.L[0], s1.L[1], 22 / pc.A]
        # two components per list: each covers the region's centred points exactly once (the
        # plane lies between two centred z planes, half the weight on each)
        for comp in np.unique(pts[:, 3]):
            sel = pts[pts[:, 3] == comp]
            half = np.rint(sel[:, :3] * 2 * pc.A).astype(int)
            assert len({tuple(h) for h in half}) == len(half) == \
                2 * (s1.n[0] + 2) * (s1.n[1] + 2)
            assert half[:, :2].min() == -1 and half[:, 0].max() == 2 * s1.n[0] + 1
            assert sorted(set(half[:, 2])) == [43, 45]
            if which == 0:  # the E list carries the loop weight, the H list none
                assert np.any(sel[:, 4] != 1.0)
                check_weights(sel[:, 4], loop_weights(sel[:, :3], lo, hi, pc.A, None), sel[:, :3])
                # the period's area: every centred point of the period counted once
                assert abs(sel[:, 4].sum() - s1.L[0] * s1.L[1]) < 1e-12
    # flux over the period against the supercell oracle's flux over the central period
    got, want = np.asarray(p.flux(phx)), np.asarray(o.flux(ohx))
    e, h = o.dft_data(ohx, 0), o.dft_data(ohx, 1)
    nf = len(FREQS)
    terms = (e.reshape(-1, nf) * np.conj(h.reshape(-1, nf))).real
    s, n = np.abs(terms).sum(axis=0), terms.shape[0]
    print("flux", got, want, "err / bound", np.abs(got - want) / ((n + 64) * U * s))
    assert np.all(want != 0) and np.all(np.abs(got - want) <= (n + 64) * U * s)
    # the same bits unfused and one step per call
    for kw in (dict(fused=False), dict(chunks=[1] * T)):
        q, qhf, qhx = _monitor_run(s1.make(pc.product_makers()[0]), s1, T, **kw)
        assert _mode(q) == [int("fused" not in kw)]
        assert np.array_equal(np.asarray(q.flux(qhx)), got), kw
        for which in (0, 1):
            assert np.array_equal(q.dft_data(qhx, which), p.dft_data(phx, which)), kw
        assert np.array_equal(q.dft_array(qhf, 1, 0), p.dft_array(phf, 1, 0)), kw


# ---------------------------------------------------------------- E. several ranks
@pytest.mark.parametrize("nranks", [2, 3])
def test_slabs(nranks):
    """Case 4 (x and y periodic, z the slab direction) on in-process slabs, bitwise equal to
    one rank."""
    T = pc.steps_bound(4, 3, "lorentz")
    want = pc.oracle_central(4, "lorentz", T)
    _, g = pc.run_product(4, "lorentz", T, maker=pc.product_makers()[nranks - 1])
    assert _mode(g) == [0] * nranks  # several ranks decline the fused mode collectively
    _same(_arrays(g), want, "%d slabs" % nranks)


# ---------------------------------------------------------------- F. plumbing
def test_checkpoint_resume(tmp_path):
    T = pc.steps_bound(4, 3, "lorentz")
    _, p = pc.run_product(4, "lorentz", T)
    want = _arrays(p)
    _, a = pc.run_product(4, "lorentz", T // 2)
    path = str(tmp_path / "per.ck")
    a.dump(path)
    sc = pc.Scene(4, "lorentz", 1)
    b = pc.configure(sc.make(pc.product_makers()[0]), sc, init=False)
    b.load(path)
    _same(_arrays(b), _arrays(a), "loaded state")
    b.step(T - T // 2)
    _same(_arrays(b), want, "resumed")


def test_tune_then_step_is_plain_stepping():
    """The tuner steps its candidates for real (tests/test_gpu_tune.py): a periodic run that
    tunes first equals plain stepping bit for bit (product against product: past the horizon of
    the supercell)."""
    total = 240
    sc = pc.Scene(4, "lorentz", 1, planar_comp=2)
    p = pc.configure(sc.make(pc.product_makers()[0]), sc)
    zc, gc = p._fields().tune(reps=1)
    t = p.t
    assert 1 + 6 * 4 <= t <= total, t  # every z-chunk candidate stepped: the fused mode was on
    assert zc in (0, 16, 20, 24, 32, 48)
    p.step(total - t)
    assert _mode(p) == [1]
    _, q = pc.run_product(4, "lorentz", total, planar_comp=2)
    _same(_arrays(p), _arrays(q), "tuned")


def test_metal_checkpoint_is_the_parents_bytes(tmp_path):
    """The checkpoint of a non-periodic run, byte for byte what the parent commit wrote
    (tests/golden/ckpt_metal_parent.mnl, made by periodic_cases.metal_checkpoint_run there)."""
    import os
    from meep_nl_amd import core
    path = str(tmp_path / "metal.mnl")
    f = pc.metal_checkpoint_run(core, path)
    assert f.fused_active() is False  # dump leaves the fused mode
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                          "ckpt_metal_parent.mnl")
    a, b = open(path, "rb").read(), open(golden, "rb").read()
    assert len(a) == len(b) and a == b


def test_checkpoint_needs_the_same_boundaries(tmp_path):
    """A dump records the boundary kinds: loading it into fields with other kinds fails."""
    _, a = pc.run_product(4, "plain", 4)
    path = str(tmp_path / "per.ck")
    a.dump(path)
    from scenarios import ProductSim
    sc = pc.Scene(4, "plain", 1)
    b = pc.configure(sc.make(ProductSim), sc, init=False)  # no make_periodic: metal walls
    with pytest.raises(RuntimeError, match="meep:.*boundary"):
        b.load(path)
    _, m = pc.run_product(4, "plain", 0, maker=ProductSim)
    m.step(4)
    mpath = str(tmp_path / "metal.ck")
    m.dump(mpath)
    c = pc.configure(sc.make(pc.product_makers()[0]), sc, init=False)
    with pytest.raises(RuntimeError, match="meep:.*boundary"):
        c.load(mpath)


def test_device_side_errors():
    from meep_nl_amd import core
    def fields(dim=3, n=(8, 8, 8), pml=None):
        s = core.Structure(core.GridVolume(dim, list(n), pc.A, [0, 0, 0]))
        if pml is not None:
            s.add_pml(0.25, dirs=(pml[0],), sides=pml[1])
        return core.Fields(s)
    f = fields()
    with pytest.raises(RuntimeError, match="meep:.*complex fields"):
        f.use_bloch(0, 0.25)
    with pytest.raises(RuntimeError, match="meep:.*complex fields"):
        f.use_bloch(0, 0.25j)
    with pytest.raises(RuntimeError, match="meep:.*direction"):
        f.use_bloch(3)
    f.use_bloch(1)
    f.use_bloch(1)  # again: nothing changes
    assert [f.boundary(d, s) for d in range(3) for s in (0, 1)] == \
        ["metallic"] * 2 + ["periodic"] * 2 + ["metallic"] * 2
    with pytest.raises(RuntimeError, match="meep:.*no such direction"):
        fields(dim=2, n=(8, 8, 0)).boundary(2)
    for sides in ((0, 1), (0,), (1,)):
        with pytest.raises(RuntimeError, match="meep:.*PML along a periodic direction"):
            fields(pml=(2, sides)).use_bloch(2)
    with pytest.raises(RuntimeError, match="meep:.*1-D"):
        fields(dim=1, n=(0, 0, 16)).use_bloch(2)
    with pytest.raises(RuntimeError, match="meep:.*no such direction"):
        fields(dim=2, n=(8, 8, 0)).use_bloch(2)
    # wall-plane neighbour reads across PML chunks of two directions
    s2 = core.Structure(core.GridVolume(3, [8, 10, 10], pc.A, [0, 0, 0]))
    s2.add_pml(0.25, dirs=(1, 2))
    sig = [[None] * 3 for _ in range(3)]
    for c in range(3):
        sig[c][c] = np.full(s2.gv.shape(), 0.3)
    sig[0][1] = sig[1][0] = np.full(s2.gv.shape(), 0.1)
    s2.add_lorentzian_tensor(1.0, 0.05, sig)
    with pytest.raises(RuntimeError, match="meep:.*PML along two directions"):
        core.Fields(s2).use_bloch(0)
    g = fields()
    g.add_gaussian_source(2, 0.5, 1.0, 0.0, 4.0, (0.5, 0.5, 0.5), 1.0)
    with pytest.raises(RuntimeError, match="meep:.*before sources"):
        g.use_bloch(0)
    h = fields()
    h.require_component(2)
    h.step(1)
    with pytest.raises(RuntimeError, match="meep:.*before the first step"):
        h.use_bloch(0)
    # the slab direction on more than one rank
    s = core.Structure(core.GridVolume(3, [8, 8, 8], pc.A, [0, 0, 0]))
    hub = core.LocalHub(2)
    fs = [core.Fields(s, rank=r, nranks=2, hub=hub) for r in range(2)]
    for r in range(2):
        fs[r].use_bloch(0)
        with pytest.raises(RuntimeError, match="meep:.*slab direction"):
            fs[r].use_bloch(2)
    # near2far images stay refused, and the message still says why
    with pytest.raises(RuntimeError, match="meep:.*periodic"):
        f.add_dft_near2far([([0.2, 0.2, 0.5], [0.8, 0.8, 0.5], 2, 1.0)], FREQS, 1, nperiods=2)
    # get_dft_array over image chunks is refused, not answered wrongly
    f.require_component(0)
    hx = f.add_dft_flux([([0.0, 0.0, 0.5], [1.0, 1.0, 0.5], 2, 1.0)], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep:.*periodic face"):
        f.dft_array(hx, 0, 0)


def test_simulation_end_to_end():
    """Simulation(k_point=Vector3(), boundary_layers=[PML(direction=Z)]) against the same run
    through core."""
    import meep_nl_amd as mp
    from meep_nl_amd import core
    n, T = (16, 12, 24), 40
    cell = mp.Vector3(n[0] / pc.A, n[1] / pc.A, n[2] / pc.A)
    sim = mp.Simulation(cell_size=cell, resolution=pc.A, k_point=mp.Vector3(),
                        boundary_layers=[mp.PML(0.5, direction=mp.Z)], eps_averaging=False,
                        geometry=[mp.Block(size=mp.Vector3(mp.inf, 0.5, 0.5),
                                           material=mp.Medium(epsilon=4))],
                        sources=[mp.Source(mp.GaussianSource(0.8, fwidth=0.6), mp.Ex,
                                           center=mp.Vector3(0, 0, -0.5),
                                           size=mp.Vector3(cell.x, cell.y, 0))])
    sim.init_sim()
    assert [sim.fields.boundary(d) for d in range(3)] == ["periodic", "periodic", "metallic"]
    sim.fields.step(T)
    s = core.Structure(sim.fields.gv)
    s.add_pml(0.5, (2,), (0, 1))
    for c in (0, 1, 2):
        s.set_chi1inv(c, c, sim.structure.get_chi1inv(c, c))
    f = core.Fields(s)
    f.use_bloch(0)
    f.use_bloch(1)
    for src in sim.sources:
        src.add_source(f)
    f.step(T)
    for c in pc.ALL_COMPS:
        a, b = sim.fields.get_array(c), f.get_array(c)
        assert np.array_equal(a, b), c
    assert np.any(sim.fields.get_array(0) != 0)
    # the block and the source are uniform along x and both x faces are periodic: so is every
    # field, to rounding (a seam point adds the source as two halves, an inner point at once;
    # with metal x faces the planes would differ by the size of the field itself)
    arrs = {c: sim.fields.get_array(c) for c in pc.ALL_COMPS}
    for c in pc.ALL_COMPS:  # against the largest component of the same field type
        scale = max(np.max(np.abs(arrs[k])) for k in pc.ALL_COMPS if k // 3 == c // 3)
        assert np.max(np.abs(arrs[c] - arrs[c][:1])) <= 1e-12 * scale, c
