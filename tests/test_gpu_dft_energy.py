"""DFT energy monitors (fields::add_dft_energy, dft_energy::electric / magnetic / total,
src/dft.cpp:630-790) and D / B components of dft-fields objects on the GPU.

The oracle has no energy objects, so the expectation is built from what it has: centred
dft_fields over the same volumes (the identical add_dft arithmetic for the unweighted lists),
its per-step field arrays, and the numpy restatements of tests/dft_restate.py.  Tolerances
(a), (b), (c) are those of that file.
"""
import numpy as np
import pytest

import dft_restate as R
from dft_restate import (A, BX, DX, EX, EY, EZ, FREQS, HX, HY, HZ, STEPS, U, add_all, build_cell,
                         collective, lists_of)
from scenarios import GroupSim, GroupSim3, ProductSim, make_oracle

gpu = pytest.mark.gpu
NF = len(FREQS)

# (lo, hi, direction, weight): direction and weight are ignored by add_dft_energy
REGIONS = [
    ([-0.5, -0.4, -0.3], [0.6, 0.5, 0.4], 0, 1.0),        # edges on lattice points
    ([-0.73, -0.61, -0.77], [0.52, 0.33, 0.77], 1, -2.0),  # edges at arbitrary positions
    ([0.06, -0.55, -0.31], [0.19, 0.41, 0.22], 2, 0.5),    # 1.3 pixels along x: three points
    # the two-step region (y < 0.8) and the rim; 0.6 pixels along z: two points
    ([-0.3, 0.55, 0.07], [0.4, 0.93, 0.13], 0, 1.0),
]


def build(make, tb=None, regions=REGIONS, medium="uniform"):
    o = build_cell(make, medium, tb)
    return o, add_all(o, "add_dft_energy", [[r] for r in regions])


def sums(o, h):
    return [collective(o, lambda f: f.dft_energy(h, w)) for w in range(3)]


def snapshot(o, hs):
    return {"lists": [lists_of(o, h, 4) for h in hs], "sums": [sums(o, h) for h in hs]}


def same(a, b):
    for la, lb in zip(a["lists"], b["lists"]):
        for x, y in zip(la, lb):
            assert x.size == y.size and np.array_equal(x, y)
    for sa, sb in zip(a["sums"], b["sums"]):
        for x, y in zip(sa, sb):
            assert np.array_equal(x, y)


@pytest.fixture(scope="module")
def base():
    """fused with temporal blocking, one call of 40 steps and one of 40"""
    o, hs = build(ProductSim, tb=True)
    o.step(STEPS // 2)
    o.step(STEPS - STEPS // 2)
    f = o._fields()
    out = snapshot(o, hs)
    out.update(o=o, hs=hs, fused=f.fused_active(), tb=f.tb_info())
    return out


@pytest.fixture(scope="module")
def oracle():
    """per region the centred E and H dft_fields of the oracle: [comp] -> (N, NF)"""
    o = build_cell(make_oracle)
    comps = [EX, EY, EZ, HX, HY, HZ]
    hs = [o.add_dft_fields(comps, lo, hi, FREQS, False, 1) for lo, hi, _, _ in REGIONS]
    o.step(STEPS)
    out = []
    for h in hs:
        d = o.dft_data(h, 0).reshape(6, -1, NF)  # every add_dft call prepends its chunk
        out.append({c: d[5 - c] for c in comps})
    return out


def by_dir(lst):
    """a list of an energy object as [direction] -> (N, NF): chunks were prepended per d"""
    d = lst.reshape(3, -1, NF)
    return [d[2], d[1], d[0]]


# ------------------------------------------------------------------ 1. unweighted lists
@gpu
def test_mode_is_fused_with_pairs(base):
    assert base["fused"] and base["tb"]["active"], base["tb"]


@gpu
def test_d_and_b_lists_bitwise_against_oracle(base, oracle):
    f = base["o"]._fields()
    for h, lists, orc in zip(base["hs"], base["lists"], oracle):
        D, B = by_dir(lists[2]), by_dir(lists[3])
        assert np.array_equal(f.dft_data(h, 2), lists[2])
        for d in range(3):
            e = orc[EX + d]
            parts = np.concatenate([e.real.ravel(), e.imag.ravel()])
            assert np.any(parts != 0)
            assert np.all(np.abs(parts[parts != 0]) > 1e-290)  # no subnormal: 2 x is exact
            assert np.array_equal(D[d], 2.0 * e), (h, d)  # chi1inv = 0.5: E = 0.5 D bit for bit
            assert np.array_equal(B[d], orc[HX + d]), (h, d)  # mu = 1: H is B
            pts = f.dft_points(h, 2).reshape(3, -1, 5)
            assert np.all(pts[2 - d][:, 3] == DX + d) and np.all(pts[2 - d][:, 4] == 1.0)
            assert np.all(f.dft_points(h, 3).reshape(3, -1, 5)[2 - d][:, 3] == BX + d)


# ------------------------------------------------------------------ 2. weighted lists
@gpu
def test_e_and_h_lists_are_the_weighted_oracle_lists(base, oracle):
    f = base["o"]._fields()
    branches = set()
    for h, lists, orc, (lo, hi, _, _) in zip(base["hs"], base["lists"], oracle, REGIONS):
        for d in range(3):
            branches.add(R.boundary_weights_1d(lo[d], hi[d], A, 1)[2])
        for which, c0 in ((0, EX), (1, HX)):
            pts = f.dft_points(h, which)
            want_w = R.loop_weights(pts[:, :3], lo, hi, A)
            R.check_weights(pts[:, 4], want_w, pts[:, :3])
            got = by_dir(lists[which])
            wd = by_dir(np.repeat(pts[:, 4], NF))
            cd = pts[:, 3].reshape(3, -1)
            for d in range(3):
                assert np.all(cd[2 - d] == c0 + d)
                want = wd[d] * orc[c0 + d]
                big = np.max(np.abs(want))
                err = np.max(np.abs(got[d] - want))
                print(f"object {h} list {which} dir {d}: err {err:.3e}, max {big:.3e}")
                assert big > 0 and err <= 1e-12 * big
    assert {0, 1, 3} <= branches, branches  # the long branch and the two short ones


# ------------------------------------------------------------------ 4. sums
@gpu
def test_sums_against_sequential_numpy(base):
    p = base["o"]._fields()
    for h, lists, s in zip(base["hs"], base["lists"], base["sums"]):
        for which, (a, b) in enumerate(((0, 2), (1, 3))):
            want, S, n = R.pair_sum(lists[a], lists[b], 0.5, NF)
            R.check_sum(s[which], want, S, n, f"object {h} energy {which}")
        assert np.array_equal(s[2], s[0] + s[1])
        for w in range(3):
            assert np.array_equal(p.dft_energy(h, w), s[w])  # two calls: the same bits
    # several workgroups of the pair-sum kernel and a masked tail in at least one object
    n = [p.dft_list_size(h, 0) // NF for h in base["hs"]]
    assert max(n) > 4096 and any(k % 64 for k in n), n


# ------------------------------------------------------------------ 5. modes
def run_variant(tb=None, calls=(STEPS,), regions=REGIONS, read=False):
    o, hs = build(ProductSim, tb=tb, regions=regions)
    for k, n in enumerate(calls):
        o.step(n)
        if read and k == len(calls) // 2:
            mid = o._fields().dft_energy(hs[0], 2)
            assert np.all(np.isfinite(mid)) and np.any(mid != 0)
    return o, hs


@gpu
def test_mode_fused_without_pairs(base):
    o, hs = run_variant(tb=False)
    assert o._fields().fused_active() and not o._fields().tb_info()["active"]
    same(snapshot(o, hs), base)


@gpu
def test_mode_unfused(base, monkeypatch):
    monkeypatch.setenv("MNL_NO_FUSED", "1")
    o, hs = run_variant()
    assert not o._fields().fused_active()
    same(snapshot(o, hs), base)


@gpu
def test_mode_single_steps_with_read_in_the_middle(base):
    o, hs = run_variant(calls=(1,) * STEPS, read=True)
    same(snapshot(o, hs), base)


@gpu
@pytest.mark.parametrize("kb", ["1", "3"])
def test_mode_dft_block(base, monkeypatch, kb):
    monkeypatch.setenv("MNL_DFT_BLOCK", kb)
    o, hs = run_variant(tb=True, calls=(40, 40))
    same(snapshot(o, hs), base)


@gpu
def test_mode_fifth_monitor_has_no_compact_box(base):
    o, hs = run_variant(tb=True, calls=(40, 40), regions=REGIONS + [REGIONS[3]])
    assert o._fields().tb_info()["active"]
    snap = snapshot(o, hs)
    same({"lists": snap["lists"][:4], "sums": snap["sums"][:4]}, base)
    same({"lists": snap["lists"][4:], "sums": snap["sums"][4:]},
         {"lists": base["lists"][3:], "sums": base["sums"][3:]})


# ------------------------------------------------------------------ 6. slabs
@gpu
@pytest.mark.parametrize("group", [GroupSim, GroupSim3])
def test_slabs_match_one_rank(base, group):
    o, hs = build(group)
    o.step(STEPS)
    for h, lists, s in zip(hs, base["lists"], base["sums"]):
        got = lists_of(o, h, 4)
        for x, y in zip(got, lists):
            assert np.array_equal(x, y)
        gs = sums(o, h)
        for which, (a, b) in enumerate(((0, 2), (1, 3))):
            want, S, n = R.pair_sum(lists[a], lists[b], 0.5, NF)
            R.check_sum(gs[which], want, S, n, f"{group.__name__} object {h} energy {which}")
        assert np.array_equal(gs[2], gs[0] + gs[1])


# ------------------------------------------------------------------ 7. data workflow
@gpu
def test_data_workflow(base, tmp_path):
    """get -> load into a fresh run -> the same sums; scale; load_minus; file round trip; a
    wrong size.  load_minus leaves the sums unchanged bit for bit, not 0: the lists become
    -data and the sums are quadratic in them ((-a) conj(-b) = a conj(b) exactly)."""
    h0, lists, s = base["hs"][1], base["lists"][1], base["sums"][1]
    o, hs = build(ProductSim)
    f, h = o._fields(), hs[1]
    assert all(np.all(x == 0) for x in lists_of(o, h, 4))
    for w in range(4):
        f.dft_load(h, w, lists[w])
    for w in range(3):
        assert np.array_equal(f.dft_energy(h, w), s[w])
    f.dft_scale(h, 2.0)
    for w in range(3):
        assert np.array_equal(f.dft_energy(h, w), 4.0 * s[w])
    for w in range(4):
        f.dft_load(h, w, lists[w])
    f.dft_scale(h, 1j)
    for which, (a, b) in enumerate(((0, 2), (1, 3))):
        want, S, n = R.pair_sum(lists[a], lists[b], 0.5, NF)
        R.check_sum(f.dft_energy(h, which), want, S, n, f"scale(1j) energy {which}")
    for w in range(4):
        f.dft_load(h, w, lists[w], sign=-1)
        assert np.array_equal(f.dft_get(h, w), -lists[w])
    for w in range(3):
        assert np.array_equal(f.dft_energy(h, w), s[w])
    path = str(tmp_path / "energy.dft")
    base["o"]._fields().dft_save(h0, path)
    f.dft_scale(h, 0.0)
    f.dft_load_file(h, path)
    for w in range(4):
        assert np.array_equal(f.dft_get(h, w), lists[w])
    f.dft_load_file(h, path, sign=-1)
    for w in range(4):
        assert np.array_equal(f.dft_get(h, w), -lists[w])
    with pytest.raises(RuntimeError, match=r"meep: incorrect dataset size \(.*\) in load_dft .*:D"):
        f.dft_load(h, 2, lists[2][:-1])
    with pytest.raises(RuntimeError, match="meep: incorrect dataset size"):
        f.dft_load_file(hs[0], path)


@gpu
def test_checkpoint_resume(base, tmp_path):
    a, _ = build(ProductSim)
    a.step(40)
    path = str(tmp_path / "energy.mnl")
    a.dump(path)
    b, hb = build(ProductSim)
    b.load(path)
    b.step(STEPS - 40)
    same(snapshot(b, hb), base)


# ------------------------------------------------------------------ 3. D != eps E
@pytest.fixture(scope="module")
def stepped_oracle():
    """D and B of every step of the oracle in the cell with an eps = 4 block and a Lorentzian
    slab, sampled by the numpy restatement at the given points"""
    o = build_cell(make_oracle, "blocks")
    io = [-64, -40, -40]
    frames = []
    for t in range(1, STEPS + 1):
        o.step(1)
        frames.append([o.get_array(c).copy() for c in range(DX, DX + 6)])
    return {"dt": o.dt, "io": io, "frames": frames,
            "E": [o.get_array(c).copy() for c in (EX, EY, EZ)]}


BLOCK_BOX = ([-0.45, -0.3, -0.65], [0.75, 0.35, 0.3], 0, 1.0)  # crosses the slab and the block


def accumulate(st, pos, comp, centred):
    dft = np.zeros((len(pos), NF), dtype=complex)
    for t, fr in enumerate(st["frames"], start=1):
        arr = fr[comp - DX]
        if centred:
            v, fac = R.centred_sample(arr, pos, comp, st["io"], A)
            v = fac * v
        else:
            v = R.yee_sample(arr, pos, comp, st["io"], A)
        dft += v[:, None] * R.phases(t, st["dt"], comp >= BX)[None, :]
    return dft


@gpu
@pytest.mark.parametrize("tb", [True, False])
def test_d_is_not_eps_e(stepped_oracle, tb):
    o, hs = build(ProductSim, tb=tb, regions=[BLOCK_BOX], medium="blocks")
    o.step(STEPS // 2)
    o.step(STEPS - STEPS // 2)
    f, h = o._fields(), hs[0]
    assert f.tb_info()["active"] == tb
    lists = lists_of(o, h, 4)
    for which, c0 in ((2, DX), (3, BX)):
        pts = f.dft_points(h, which).reshape(3, -1, 5)
        got = by_dir(lists[which])
        for d in range(3):
            want = accumulate(stepped_oracle, pts[2 - d][:, :3], c0 + d, True)
            big, err = np.max(np.abs(want)), np.max(np.abs(got[d] - want))
            print(f"tb {tb} comp {c0 + d}: err {err:.3e}, max {big:.3e}")
            assert big > 0 and err <= 1e-12 * big
    # and D really is not eps E here: the E list over the D list is not one constant
    ratio = np.abs(lists[2][np.abs(lists[2]) > 1e-3 * np.max(np.abs(lists[2]))])
    e = np.abs(lists[0][np.abs(lists[2]) > 1e-3 * np.max(np.abs(lists[2]))])
    assert np.ptp(e / ratio) > 0.01 * np.max(e / ratio)


# ------------------------------------------------------------------ 8. dft-fields of D and B
@gpu
def test_dft_fields_of_d_and_b_on_the_yee_grid(stepped_oracle):
    lo, hi = BLOCK_BOX[0], BLOCK_BOX[1]
    o = build_cell(ProductSim, "blocks", True)
    f = o._fields()
    comps = list(range(DX, DX + 6))
    h = f.add_dft_fields(comps, lo, hi, FREQS, True, 1)
    o.step(STEPS // 2)
    o.step(STEPS - STEPS // 2)
    got, pts = f.dft_get(h, 0).reshape(-1, NF), f.dft_points(h, 0)
    assert sorted(set(pts[:, 3].astype(int))) == comps and np.all(pts[:, 4] == 1.0)
    for c in comps:
        m = pts[:, 3] == c
        want = accumulate(stepped_oracle, pts[m, :3], c, False)
        big, err = np.max(np.abs(want)), np.max(np.abs(got[m] - want))
        print(f"yee comp {c}: err {err:.3e}, max {big:.3e}")
        assert big > 0 and err <= 1e-12 * big


@gpu
def test_dft_fields_d_is_twice_e_in_the_uniform_medium():
    o = build_cell(ProductSim, "uniform", True)
    f = o._fields()
    lo, hi = REGIONS[1][0], REGIONS[1][1]
    hd = f.add_dft_fields([DX, DX + 1, DX + 2], lo, hi, FREQS, True, 1)
    he = f.add_dft_fields([EX, EY, EZ], lo, hi, FREQS, True, 1)
    o.step(STEPS)
    d, e = f.dft_get(hd, 0), f.dft_get(he, 0)
    assert d.size == e.size and np.any(e != 0)
    assert np.array_equal(d, 2.0 * e)


# ------------------------------------------------------------------ 10. errors
@gpu
def test_errors(base):
    f, h = base["o"]._fields(), base["hs"][0]
    with pytest.raises(RuntimeError, match="meep:.*no regions"):
        f.add_dft_energy([], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep: bad dft handle"):
        f.dft_energy(99, 0)
    with pytest.raises(RuntimeError, match="meep:.*which must be"):
        f.dft_energy(h, 3)
    with pytest.raises(RuntimeError, match="meep:.*no such list"):
        f.dft_get(h, 4)
    with pytest.raises(RuntimeError, match="meep:.*no such list"):
        f.dft_points(h, -1)
    hf = f.add_dft_flux([([0.5, -0.6, -0.4], [0.5, 0.6, 0.7], 0, 1.0)], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep:.*not an energy object"):
        f.dft_energy(hf, 0)
    with pytest.raises(RuntimeError, match="meep:.*not available for energy and force"):
        f.dft_array(h, EX, 0)
