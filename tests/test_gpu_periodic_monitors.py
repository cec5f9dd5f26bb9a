"""Periodic cells with everything that samples D or B, or integrates over a periodic face: DFT
energy and force monitors and D / B dft_fields (the D wrap before a DFT update, the pair sum
over image chunks), field energies (the B half step's own wraps, boxes that reach a periodic
face), the longest list of arrays one wrap can get, and the neighbour-reading families
on the cells with three periodic axes and with y periodic in 2-D.

References.  Arrays: the CPU oracle on the metal supercell of 3 replicas, as
tests/test_gpu_periodic.py (the light-cone bound of every configuration here is checked on the
oracle alone by tests/test_periodic_cpu.py).  Monitors: the oracle has no energy or force
objects, so the same monitors run on the product's own metal supercell of 3 replicas, a path
that tests/test_gpu_dft_energy.py and tests/test_gpu_dft_force.py pin to the oracle; points are
matched by position and component, values compared bit for bit, sums within dft_restate's
tolerance (c).  Energies: the oracle's energy of the same box around the central replica, rel
1e-12 as tests/test_gpu_energy.py."""
import numpy as np
import pytest

import dft_restate as R
import periodic_cases as pc
from test_gpu_periodic import _arrays, _mode, _same

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

FREQS = [0.6, 0.8, 1.0]
NF = len(FREQS)
REL = 1e-12
A = pc.A


def _product(case, family, R_=1):
    """The periodic product (R_ = 1) or the product on the metal supercell (R_ = 3)."""
    from scenarios import ProductSim
    sc = pc.Scene(case, family, R_)
    maker = pc.product_makers()[0] if R_ == 1 else ProductSim
    return sc, pc.configure(sc.make(maker), sc)


def _oracle(case, family, R_=3):
    from scenarios import make_oracle
    sc = pc.Scene(case, family, R_)
    return sc, pc.configure(sc.make(make_oracle), sc)


def _fused_family(family):
    return family in ("plain", "lorentz")


# ---------------------------------------------------------------- 1. D / B sampling monitors
def _regions(sc):
    """(interior, full-period) boxes of the cell and planes with normal z (3-D) in them."""
    n, L = sc.n, sc.L
    nd = 3 if sc.dim == 3 else 2
    lo_in = [3 / A, 4 / A, 7 / A][:nd] + [0.0] * (3 - nd)
    hi_in = [(n[0] - 3) / A, (n[1] - 5) / A, (n[2] - 6) / A][:nd] + [0.0] * (3 - nd)
    lo_fp, hi_fp = list(lo_in), list(hi_in)
    for d in sc.per:
        lo_fp[d], hi_fp[d] = 0.0, L[d]
    return (lo_in, hi_in), (lo_fp, hi_fp)


def _add_monitors(o, sc):
    """Energy, force (one off-diagonal, one diagonal plane) and centred / Yee D, B dft_fields,
    each over the interior box and over the full-period box.  Returns [(kind, handle, nlists,
    region)].

    The samples that need the D wrap of kind 3: in a full-period region the centred points half
    a pixel above the seam (x = 0.5 / A along a periodic x, likewise y, z) average planes 0 and
    1 of the components unshifted along that axis (Dy, Dz along x; Dx, Dz along y; Dx, Dy along
    z), and plane 0 is the not-owned plane that only wrap(F, 3) with dft_samples_d fills.  The
    image chunk's points half a pixel below the seam average planes n - 1 and n, both owned."""
    f = o._fields()
    out = []
    for name, (lo, hi) in zip(("inside", "period"), _regions(sc)):
        out.append(("dfields " + name, f.add_dft_fields([6, 7, 8, 9, 10, 11], lo, hi, FREQS, False, 1),
                    1, (lo, hi)))
        out.append(("dfields yee " + name, f.add_dft_fields([6, 7, 8, 9, 10, 11], lo, hi, FREQS,
                                                            True, 1), 1, (lo, hi)))
        if sc.dim != 3:
            continue
        out.append(("energy " + name, f.add_dft_energy([(lo, hi, 0, 1.0)], FREQS, 1), 4, (lo, hi)))
        zc = 0.5 * (lo[2] + hi[2])
        zc = np.floor(zc * 2 * A) / (2 * A)  # a multiple of half a pixel
        plo, phi = [lo[0], lo[1], zc], [hi[0], hi[1], zc]
        out.append(("force offdiag " + name, f.add_dft_force([(plo, phi, 0, 1.0)], FREQS, 1), 3,
                    (plo, phi)))
        out.append(("force diag " + name, f.add_dft_force([(plo, phi, 2, -0.5)], FREQS, 1), 3,
                    (plo, phi)))
    return out


def _lists(f, mons):
    """per monitor and list: {(half-pixel position, component): values per frequency}, the raw
    list, and the points"""
    out = []
    for kind, h, nl, _ in mons:
        row = []
        for w in range(nl):
            pts = f.dft_points(h, w)
            vals = f.dft_get(h, w).reshape(-1, NF)
            assert len(pts) == len(vals), (kind, w)
            half = np.rint(pts[:, :3] * 2 * A).astype(int)
            assert np.max(np.abs(half - pts[:, :3] * 2 * A), initial=0.0) < 1e-9
            keys = [tuple(hh) + (int(c),) for hh, c in zip(half, pts[:, 3])]
            d = dict(zip(keys, range(len(keys))))
            assert len(d) == len(keys), (kind, w, "a point twice in one list")
            row.append((d, vals, pts))
        out.append(row)
    return out


def _sums(f, mons):
    out = []
    for kind, h, nl, _ in mons:
        if kind.startswith("energy"):
            out.append([f.dft_energy(h, w) for w in range(3)])
        elif kind.startswith("force"):
            out.append([f.dft_force(h)])
        else:
            out.append([])
    return out


def _run(case, family, R_, T, chunks=None, fused=True):
    sc, o = _product(case, family, R_)
    if not fused:
        o._fields().set_fused(False)
    mons = _add_monitors(o, sc)
    for k in (chunks or [T]):
        o.step(k)
    mode = _mode(o)
    f = o._fields()
    return sc, o, mons, mode, _lists(f, mons), _sums(f, mons)


def _restated(kind, lists):
    """the sum of a monitor from its own lists (tests/dft_restate.py's sequential pair sum)"""
    raw = [l[1].ravel() for l in lists]
    if kind.startswith("energy"):
        return [R.pair_sum(raw[0], raw[2], 0.5, NF), R.pair_sum(raw[1], raw[3], 0.5, NF)]
    a = R.pair_sum(raw[0], raw[1], 1.0, NF) if raw[0].size else (0.0, 0.0, 0)
    b = (0.0, 0.0, 0)
    if raw[2].size:
        comp = lists[2][2][:, 3].astype(int)
        wgt = -0.5  # the diagonal region's weight in _add_monitors
        b = R.pair_sum(raw[2], raw[2], wgt * np.where(comp % 3 == 2, 0.5, -0.5), NF)
    return [tuple(x + y for x, y in zip(a, b))]


@pytest.mark.parametrize("case,family", [(4, "lorentz"), (5, "plain"), ("2dy", "lorentz")])
def test_d_and_b_monitors_against_the_metal_supercell(case, family, monkeypatch):
    T = pc.steps_bound(case, 3, family)
    sc, p, mons, mode, got, gsum = _run(case, family, 1, T)
    assert mode == [int(sc.dim == 3)]
    s3, q, mons3, _, want, wsum = _run(case, family, 3, T)
    seam_reads = 0
    for (kind, h, nl, (lo, hi)), g, w, gs, ws in zip(mons, got, want, gsum, wsum):
        for k in range(nl):
            (gd, gv, gp), (wd, wv, wp) = g[k], w[k]
            assert set(gd) == set(wd), (kind, k, len(gd), len(wd))
            if not gd:
                continue
            order = np.array([wd[key] for key in gd])
            assert np.any(wv != 0), (kind, k)
            assert np.array_equal(gv, wv[order]), (kind, k, float(np.max(np.abs(gv - wv[order]))))
            assert np.array_equal(gp[:, 4], wp[order, 4]), (kind, k, "weights")
            # the centred D samples half a pixel above a seam: they read the wrapped plane 0
            if "period" in kind and "yee" not in kind:
                for d in sc.per:
                    sel = [i for key, i in gd.items() if key[d] == 1 and 6 <= key[3] < 9
                           and (key[3] - 6) != d]
                    if sel:
                        seam_reads += 1
                        assert np.any(gv[sel] != 0), (kind, k, d)
        if kind.startswith("dfields") and "yee" not in kind:
            # weights of the centred lists are 1 (dft_fields); of the energy's E list the loop's
            assert np.all(g[0][2][:, 4] == 1.0)
        if kind.startswith("energy"):
            pts = g[0][2]
            R.check_weights(pts[:, 4], R.loop_weights(pts[:, :3], lo, hi, A), pts[:, :3])
        for j, (want_s, S, n) in enumerate(_restated(kind, g) if gs else []):
            R.check_sum(gs[j], want_s, S, n, f"{case} {kind} sum {j}")
        if kind.startswith("energy"):
            assert np.array_equal(gs[2], gs[0] + gs[1])
        for a, b in zip(gs, ws):
            if "inside" in kind:  # the same chunk lists: the same bits
                assert np.array_equal(a, b), (kind, a, b)
    assert seam_reads >= len(sc.per)
    # the same bits unfused, one step per call, and with one DFT update per accumulation
    for kw in (dict(fused=False), dict(chunks=[1] * T), dict(block="1")):
        if "block" in kw:
            monkeypatch.setenv("MNL_DFT_BLOCK", kw.pop("block"))
        _, _, _, m2, l2, s2 = _run(case, family, 1, T, **kw)
        assert m2 == [int(sc.dim == 3 and kw.get("fused", True))], kw
        for g, g2, a, b in zip(got, l2, gsum, s2):
            for x, y in zip(g, g2):
                assert np.array_equal(x[1], y[1]), kw
            for x, y in zip(a, b):
                assert np.array_equal(x, y), kw


def _by_position(f, h, which):
    """a list as {(half-pixel position, component): values}, its values and its points"""
    pts = f.dft_points(h, which)
    vals = f.dft_get(h, which).reshape(-1, NF)
    half = np.rint(pts[:, :3] * 2 * A).astype(int)
    keys = [tuple(int(v) for v in hh) + (int(c),) for hh, c in zip(half, pts[:, 3])]
    assert len(set(keys)) == len(keys) == len(vals)
    return dict(zip(keys, vals)), vals, pts


def test_full_period_lists_against_the_oracle():
    """Case 5, plain: a full-period energy box and a full-period off-diagonal force plane
    against the R = 3 oracle's centred dft_fields of the same regions, built as
    tests/test_gpu_dft_energy.py and tests/test_gpu_dft_force.py build them: the weighted E / H
    lists are loop_weights x oracle values within 1e-12 max, the unweighted lists (D, B,
    offdiag2) the oracle's bit for bit.  The oracle has no dft_points, so positions come from
    the same monitors on the product's metal supercell, whose chunks and loop order are the
    oracle's (the lists are compared element by element there); the periodic cell's lists,
    image chunks first, are then matched to those by position, bit for bit.  The regions lie
    in z = 6 .. 12 cells, outside the block (it keeps within 3 cells of every seam), where
    chi1inv is 1.0 and so D = E bit for bit."""
    T = pc.steps_bound(5, 3, "plain")
    sc = pc.Scene(5, "plain", 1)
    lo, hi = [0.0, 0.0, 6 / A], [sc.L[0], sc.L[1], 12 / A]
    plo, phi = [0.0, 0.0, 9 / A], [sc.L[0], sc.L[1], 9 / A]
    fd, nd = 0, 2
    runs = []
    for R_ in (1, 3):
        _, p = _product(5, "plain", R_)
        f = p._fields()
        he = f.add_dft_energy([(lo, hi, 0, 1.0)], FREQS, 1)
        hf = f.add_dft_force([(plo, phi, fd, 1.0)], FREQS, 1)
        p.step(T)
        runs.append((f, he, hf))
    _, o = _oracle(5, "plain")
    oe = o.add_dft_fields([0, 1, 2, 3, 4, 5], lo, hi, FREQS, False, 1)
    o1 = o.add_dft_fields([fd, 3 + fd], plo, phi, FREQS, False, 1)
    o2 = o.add_dft_fields([nd, 3 + nd], plo, phi, FREQS, False, 1)
    o.step(T)
    od = o.dft_data(oe, 0).reshape(6, -1, NF)  # every add_dft call prepends its chunk
    (fp, hep, hfp), (fs, hes, hfs) = runs

    def weighted(got, want, pts, region, what):
        R.check_weights(pts[:, 4], R.loop_weights(pts[:, :3], region[0], region[1], A), pts[:, :3])
        want = pts[:, 4:5] * want
        big, err = np.max(np.abs(want)), np.max(np.abs(got - want))
        print(f"{what}: err {err:.3e}, max {big:.3e}")
        assert big > 0 and err <= 1e-12 * big, what

    # ---- the supercell product's lists, element by element in the oracle's order
    for which, c0 in ((0, 0), (1, 3), (2, 0), (3, 3)):  # E, H weighted; D, B unweighted
        _, vals, pts = _by_position(fs, hes, which)
        v3, p3 = vals.reshape(3, -1, NF), pts.reshape(3, -1, 5)
        for d in range(3):  # the chunks were prepended per direction
            want = od[5 - (c0 + d)]
            assert np.all(p3[2 - d][:, 3] == (c0 if which < 2 else c0 + 6) + d)
            assert v3[2 - d].shape == want.shape and np.any(want != 0)
            if which < 2:
                weighted(v3[2 - d], want, p3[2 - d], (lo, hi), f"energy list {which} dir {d}")
            else:
                assert np.all(p3[2 - d][:, 4] == 1.0)
                assert np.array_equal(v3[2 - d], want), (which, d)
    _, v1, p1 = _by_position(fs, hfs, 0)
    _, v2, p2 = _by_position(fs, hfs, 1)
    n = len(v1)
    assert np.all(p1[:n // 2, 3] == 3 + fd) and np.all(p1[n // 2:, 3] == fd)
    assert np.all(p2[:n // 2, 3] == 3 + nd) and np.all(p2[n // 2:, 3] == nd)
    weighted(v1, o.dft_data(o1, 0).reshape(-1, NF), p1, (plo, phi), "force offdiag1")
    assert np.all(p2[:, 4] == 1.0) and np.array_equal(p2[:, :3], p1[:, :3])
    assert np.array_equal(v2, o.dft_data(o2, 0).reshape(-1, NF))
    # ---- the periodic cell's lists against those, by position
    for h_p, h_s, nl in ((hep, hes, 4), (hfp, hfs, 2)):
        for which in range(nl):
            got, _, gp = _by_position(fp, h_p, which)
            want, _, _ = _by_position(fs, h_s, which)
            assert set(got) == set(want), (nl, which)
            assert all(np.array_equal(got[k], want[k]) for k in got), (nl, which)
            if which == 0:  # image chunks: points outside the cell on both sides of each axis
                half = np.rint(gp[:, :3] * 2 * A).astype(int)
                assert half[:, :2].min() == -1 and half[:, 0].max() == 2 * sc.n[0] + 1


# ---------------------------------------------------------------- 3. field energy
def _boxes(sc):
    n, L = sc.n, sc.L
    ax = pc.axes_of(sc.dim)
    inside = ([2.5 / A if d in ax else 0.0 for d in range(3)],
              [(n[d] - 3) / A if d in ax else 0.0 for d in range(3)])
    whole = ([0.0] * 3, [L[d] if d in ax else 0.0 for d in range(3)])
    p0 = sc.per[0]
    low, high, period = ([list(v) for v in inside] for _ in range(3))
    low[0][p0], low[1][p0] = 0.0, (n[p0] // 2) / A           # reaches the low periodic face
    high[0][p0], high[1][p0] = (n[p0] // 2 + 0.5) / A, L[p0]  # reaches the high one
    for d in sc.per:
        period[0][d], period[1][d] = 0.0, L[d]
    return {"inside": inside, "low face": tuple(low), "high face": tuple(high),
            "period": tuple(period), "cell": whole}


NAMES = ("electric_energy_in_box", "magnetic_energy_in_box", "field_energy_in_box")


@pytest.mark.parametrize("case,family", [(4, "lorentz"), (4, "mu"), (5, "plain")])
def test_field_energy(case, family):
    T = pc.steps_bound(case, 3, family)
    sc, p = _product(case, family)
    s3, o = _oracle(case, family)
    boxes = _boxes(sc)

    def energies(first):
        for label, (lo, hi) in boxes.items():
            for name in NAMES:
                want = getattr(o, name)(lo, hi)
                before = None if first else _arrays(p)
                got = getattr(p, name)(lo, hi)
                print(case, family, p.t, label, name, got, want, abs(got - want))
                assert first or want != 0  # (E is 0 before the first step)
                assert got == pytest.approx(want, rel=REL), (label, name, p.t)
                if label == "cell":  # the defaults are the whole cell
                    assert getattr(p, name)() == got, (label, name)
                if before is not None:
                    _same(_arrays(p), before, "after " + name)
        assert p.field_energy() == pytest.approx(o.field_energy_in_box(*boxes["cell"]), rel=REL)

    # before the first step the synchronisation is the first B step: H is created and stays,
    # in the oracle too (tests/test_gpu_energy.py::test_energy_first_step_semantics)
    energies(True)
    p.step(T - 1)
    o.step(T - 1)
    assert _mode(p) == [int(_fused_family(family))]
    # straight out of the stepping mode, no array read before it: the B half step finds the E
    # ghosts as the last step left them
    assert p.field_energy() == pytest.approx(o.field_energy_in_box(*boxes["cell"]), rel=REL)
    energies(False)
    p.step(1)
    o.step(1)
    assert _mode(p) == [int(_fused_family(family))]  # the next step enters the fused mode again
    want = {c: s3.central(o.get_array(c)) for c in pc.ALL_COMPS}
    _same(_arrays(p), want, "continued after the energies")
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)


# ---------------------------------------------------------------- 4. many susceptibilities
def test_four_lorentzian_terms(tmp_path):
    """As many susceptibilities as a structure takes (MAX_POL = 4): with E, f_w, B, H, D and
    their ping-pong sets the wrap before a read or a checkpoint lists 36 arrays, the longest
    list a run can reach (one launch holds 40; a longer list would take several).  A fifth term
    is refused when it is added, by name."""
    from meep_nl_amd import core
    s = core.Structure(core.GridVolume(3, [8, 8, 8], pc.A, [0, 0, 0]))
    for k in range(4):
        s.add_lorentzian(1.0 + 0.1 * k, 0.05, [np.full(s.gv.shape(), 0.1)] * 3)
    with pytest.raises(RuntimeError, match="meep: too many susceptibilities"):
        s.add_lorentzian(1.5, 0.05, [np.full(s.gv.shape(), 0.1)] * 3)
    T = pc.steps_bound(4, 3, "lorentz4")
    want = pc.oracle_central(4, "lorentz4", T)
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)
    sc, p = pc.run_product(4, "lorentz4", T)  # configure: initialize_field wraps every array
    assert _mode(p) == [1]
    got = _arrays(p)
    _same(got, want, "4 terms")
    _, a = pc.run_product(4, "lorentz4", T // 2)
    path = str(tmp_path / "four.ck")
    a.dump(path)
    b = pc.configure(sc.make(pc.product_makers()[0]), sc, init=False)
    b.load(path)
    _same(_arrays(b), _arrays(a), "loaded state")
    b.step(T - T // 2)
    _same(_arrays(b), got, "resumed")


# ---------------------------------------------------------------- 5. neighbour-reading families
@pytest.mark.parametrize("case", [5, "2dy"])
@pytest.mark.parametrize("family", pc.REACH2)
def test_neighbour_reading_families(case, family):
    """Wrap kinds 2 (D and P before a Newton-Raphson / upstream E update) and 4 (E and f_w
    before update_pols with anisotropic sigma) where edges and corners map along several axes
    at once, and on the two-axis device grid with y periodic."""
    T = pc.steps_bound(case, 3, family)
    assert T >= 3
    want = pc.oracle_central(case, family, T)
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)
    _, p = pc.run_product(case, family, T)
    assert _mode(p) == [0]
    got = _arrays(p)
    _same(got, want, family)
    _, q = pc.run_product(case, family, T, chunks=[1] * T)
    _same(_arrays(q), got, family + ", one step per call")


def test_parity_2d_y_periodic():
    T = pc.steps_bound("2dy", 3, "plain")
    want = pc.oracle_central("2dy", "plain", T)
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)
    _, p = pc.run_product("2dy", "plain", T)
    _same(_arrays(p), want, "2-D, y periodic")


# ---------------------------------------------------------------- 2. the normalisation workflow
STEPS_W = 60


def _workflow_cell(with_block):
    """Case 4's cell, empty or with the dielectric block, an Ey current sheet over the period,
    a full-period flux plane and a full-period energy monitor."""
    sc = pc.Scene(4, "plain", 1)
    o = sc.make(pc.product_makers()[0])
    o.add_pml(pc.PML_CELLS / A, dirs=(2,))
    block = sc.mask() if with_block else np.zeros_like(sc.mask())
    pc.materials(o, sc, block, block)
    o.make_periodic(sc.per)
    o.add_gaussian_volume_source(1, 0.8, 0.6, -3.0, 3.0, [0.0, 0.0, 8 / A], [sc.L[0], sc.L[1], 8 / A],
                                 1.0)
    f = o._fields()
    hx = f.add_dft_flux([([0.0, 0.0, 22 / A], [sc.L[0], sc.L[1], 22 / A], 2, 1.0)], FREQS, 1)
    he = f.add_dft_energy([([0.0, 0.0, 18 / A], [sc.L[0], sc.L[1], 21 / A], 0, 1.0)], FREQS, 1)
    return o, f, ((hx, 2), (he, 4))


def _data(f, mons):
    return {(h, w): f.dft_get(h, w) for h, nl in mons for w in range(nl)}


@pytest.fixture(scope="module")
def workflow():
    o, f, mons = _workflow_cell(False)
    o.step(STEPS_W)
    norm = _data(f, mons)
    o2, f2, _ = _workflow_cell(True)
    o2.step(STEPS_W)
    return dict(norm=norm, f=f, mons=mons, flux=f.flux(mons[0][0]),
                energy=[f.dft_energy(mons[1][0], w) for w in range(3)],
                plain=_data(f2, mons))


def test_workflow_load_minus(workflow):
    """dft_load(sign = -1) of the empty cell's data into the run with the block: the lists start
    at -data bit for bit, the quadratic sums are unchanged by the sign ((-a) conj(-b) = a
    conj(b) exactly), and after the run every list is (run without the load) - data to the
    roundings of U updates: 2 U 2^-53 max(|data|, |run|), the bound of
    tests/test_gpu_dft_data.py::test_subtraction_against_oracle.  That difference is not bit
    for bit and cannot be: U additions that start from -data round differently from the same
    additions started from 0 with data subtracted at the end."""
    w = workflow
    o, f, mons = _workflow_cell(True)
    for (h, k), d in w["norm"].items():
        assert np.any(d != 0), (h, k)
        f.dft_load(h, k, d, sign=-1)
        assert np.array_equal(f.dft_get(h, k), -d)
    assert np.array_equal(f.flux(mons[0][0]), w["flux"]) and np.all(w["flux"] != 0)
    for k in range(3):
        assert np.array_equal(f.dft_energy(mons[1][0], k), w["energy"][k])
    o.step(STEPS_W)
    assert _mode(o) == [1]
    got = _data(f, mons)
    for key, d in w["norm"].items():
        want = w["plain"][key] - d
        M = max(np.max(np.abs(d.real)), np.max(np.abs(d.imag)),
                np.max(np.abs(w["plain"][key].real)), np.max(np.abs(w["plain"][key].imag)))
        diff = got[key] - want
        err = max(np.max(np.abs(diff.real)), np.max(np.abs(diff.imag)))
        bound = 2 * STEPS_W * 2.0 ** -53 * M
        print(f"list {key}: max err {err:.3e}, bound {bound:.3e}, bitwise {np.array_equal(got[key], want)}")
        assert np.any(want != 0) and err <= bound
    # the flux of the difference, summed in list order over the product's own lists
    e, hh = (got[(mons[0][0], k)].reshape(-1, NF) for k in (0, 1))
    want, S, n = R.pair_sum(e, hh, 1.0, NF)
    R.check_sum(f.flux(mons[0][0]), want, S, n, "flux of the difference")


def test_workflow_scale_and_files(workflow, tmp_path):
    w = workflow
    o, f, mons = _workflow_cell(True)
    for (h, k), d in w["norm"].items():
        f.dft_load(h, k, d)
    for h, nl in mons:
        f.dft_scale(h, 2.0)
        for k in range(nl):
            assert np.array_equal(f.dft_get(h, k), 2.0 * w["norm"][(h, k)])
    assert np.array_equal(f.flux(mons[0][0]), 4.0 * w["flux"])
    for k in range(3):
        assert np.array_equal(f.dft_energy(mons[1][0], k), 4.0 * w["energy"][k])
    for h, nl in mons:
        path = str(tmp_path / ("mon%d.dft" % h))
        w["f"].dft_save(h, path)
        f.dft_scale(h, 0.0)
        f.dft_load_file(h, path)
        for k in range(nl):
            assert np.array_equal(f.dft_get(h, k), w["norm"][(h, k)])
        f.dft_load_file(h, path, sign=-1)
        for k in range(nl):
            assert np.array_equal(f.dft_get(h, k), -w["norm"][(h, k)])
    with pytest.raises(RuntimeError, match="meep: dft file holds a different kind of dft object"):
        f.dft_load_file(mons[1][0], str(tmp_path / ("mon%d.dft" % mons[0][0])))


def test_workflow_through_simulation():
    """Simulation(k_point=Vector3()) with add_flux / get_flux_data / load_minus_flux_data
    against the same through core, bit for bit."""
    import meep_nl_amd as mp
    from meep_nl_amd import core
    n, T = (16, 12, 24), 40
    cell = mp.Vector3(n[0] / A, n[1] / A, n[2] / A)

    def sim_of(block):
        geom = [mp.Block(size=mp.Vector3(mp.inf, 0.5, 0.5), material=mp.Medium(epsilon=4))]
        return mp.Simulation(cell_size=cell, resolution=A, k_point=mp.Vector3(),
                             boundary_layers=[mp.PML(0.5, direction=mp.Z)], eps_averaging=False,
                             geometry=geom if block else [],
                             sources=[mp.Source(mp.GaussianSource(0.8, fwidth=0.6), mp.Ex,
                                                center=mp.Vector3(0, 0, -0.5),
                                                size=mp.Vector3(cell.x, cell.y, 0))])

    def plane(sim):
        return sim.add_flux(0.8, 0.4, NF, mp.FluxRegion(center=mp.Vector3(0, 0, 0.75),
                                                        size=mp.Vector3(cell.x, cell.y, 0)),
                            decimation_factor=1)
    a = sim_of(False)
    fa = plane(a)
    assert [a.fields.boundary(d) for d in range(3)] == ["periodic", "periodic", "metallic"]
    a.fields.step(T)
    data = a.get_flux_data(fa)
    assert np.any(data.E != 0) and np.any(data.H != 0)
    b = sim_of(True)
    fb = plane(b)
    b.load_minus_flux_data(fb, data)
    assert np.array_equal(b.get_flux_data(fb).E, -data.E)
    b.fields.step(T)
    # the same through core
    s = core.Structure(b.fields.gv)
    s.add_pml(0.5, (2,), (0, 1))
    for c in (0, 1, 2):
        s.set_chi1inv(c, c, b.structure.get_chi1inv(c, c))
    f = core.Fields(s)
    f.use_bloch(0)
    f.use_bloch(1)
    for src in b.sources:
        src.add_source(f)
    z = 0.75
    h = f.add_dft_flux([([-cell.x / 2, -cell.y / 2, z], [cell.x / 2, cell.y / 2, z], 2, 1.0)],
                       mp.get_flux_freqs(fb), 1)
    f.dft_load(h, 0, data.E, sign=-1)
    f.dft_load(h, 1, data.H, sign=-1)
    f.step(T)
    got = b.get_flux_data(fb)
    assert np.array_equal(got.E, f.dft_get(h, 0)) and np.array_equal(got.H, f.dft_get(h, 1))
    assert np.array_equal(np.array(mp.get_fluxes(fb)), f.flux(h)) and np.all(f.flux(h) != 0)
