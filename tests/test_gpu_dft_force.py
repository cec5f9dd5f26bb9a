"""DFT force monitors (fields::add_dft_force, dft_force::force, src/stress.cpp) on the GPU.

The oracle has no force objects, so the expectation is built from its centred and Yee-grid
dft_fields over the same regions (the identical add_dft arithmetic for offdiag2), the numpy
restatement of the loop weights in tests/dft_restate.py evaluated at the positions dft_points
returns, and the reference's own force test (python/tests/test_force.py).  Tolerances (a),
(b), (c) are those of tests/dft_restate.py.
"""
import json
import os

import numpy as np
import pytest

import dft_restate as R
from dft_restate import A, EX, FREQS, HX, STEPS, add_all, build_cell, collective, lists_of
from scenarios import GroupSim, GroupSim3, ProductSim, flux_box_faces, make_oracle

gpu = pytest.mark.gpu
NF = len(FREQS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "force_energy.json")

# per object the regions (lo, hi, force direction, weight); the normal is the region's
OBJECTS = [
    # a closed box, force along x: two diagonal faces and four off-diagonal ones
    [(lo, hi, 0, w) for lo, hi, _, w in flux_box_faces([-0.52, -0.47, -0.43], [0.54, 0.57, 0.48], 3)],
    [([-0.73, 0.23, -0.73], [0.73, 0.23, 0.73], 1, -0.5)],  # one diagonal face, arbitrary edges
    [([0.06, -0.55, -0.31], [0.19, 0.41, -0.31], 0, 0.5)],  # off-diagonal, 1.3 pixels along x
    # off-diagonal, edges on lattice points, across the two-step region (z < 0.8) and the rim
    [([0.5, -0.6, 0.5], [0.5, 0.6, 0.9], 1, 1.0)],
]


def normal(lo, hi):
    (nd,) = [d for d in range(3) if hi[d] == lo[d]]
    return nd


def build(make, tb=None, objects=OBJECTS):
    o = build_cell(make, "uniform", tb)
    return o, add_all(o, "add_dft_force", objects)


def force(o, h):
    return collective(o, lambda f: f.dft_force(h))


def snapshot(o, hs):
    return {"lists": [lists_of(o, h, 3) for h in hs], "sums": [force(o, h) for h in hs]}


def same(a, b):
    for la, lb in zip(a["lists"], b["lists"]):
        for x, y in zip(la, lb):
            assert x.size == y.size and np.array_equal(x, y)
    for x, y in zip(a["sums"], b["sums"]):
        assert np.array_equal(x, y)


@pytest.fixture(scope="module")
def base():
    o, hs = build(ProductSim, tb=True)
    o.step(STEPS // 2)
    o.step(STEPS - STEPS // 2)
    f = o._fields()
    out = snapshot(o, hs)
    out.update(o=o, hs=hs, fused=f.fused_active(), tb=f.tb_info())
    return out


@pytest.fixture(scope="module")
def oracle():
    """per object and region the oracle's unweighted lists in the force lists' own chunk
    order: off-diagonal regions (first [H_fd, E_fd], second [H_nd, E_nd]) on the centred grid,
    diagonal regions [Hz, Ez, Hy, Ey, Hx, Ex] on the Yee grid"""
    o = build_cell(make_oracle)
    hs = []
    for regs in OBJECTS:
        row = []
        for lo, hi, fd, _ in regs:
            nd = normal(lo, hi)
            if fd != nd:
                row.append((o.add_dft_fields([EX + fd, HX + fd], lo, hi, FREQS, False, 1),
                            o.add_dft_fields([EX + nd, HX + nd], lo, hi, FREQS, False, 1)))
            else:
                row.append((o.add_dft_fields([EX, HX, EX + 1, HX + 1, EX + 2, HX + 2], lo, hi,
                                             FREQS, True, 1),))
        hs.append(row)
    o.step(STEPS)
    return [[tuple(o.dft_data(h, 0) for h in t) for t in row] for row in hs]


def expected(f, h, regs, orc):
    """The three lists of object h as the oracle and the weight restatement give them, the
    per-point factor x of the force sum for the diag list, and the weights checked."""
    want = [[], [], []]
    xdiag = []
    at = [0, 0, 0]
    pts = [f.dft_points(h, w) for w in range(3)]
    for (lo, hi, fd, wgt), data in reversed(list(zip(regs, orc))):  # every call prepends
        nd = normal(lo, hi)
        if fd != nd:
            n = data[0].size // NF
            p = pts[0][at[0]:at[0] + n]
            assert np.all(p[:n // 2, 3] == HX + fd) and np.all(p[n // 2:, 3] == EX + fd)
            w = R.loop_weights(p[:, :3], lo, hi, A)
            R.check_weights(p[:, 4], w, p[:, :3])
            want[0].append(wgt * np.repeat(p[:, 4], NF) * data[0])
            q = pts[1][at[1]:at[1] + n]
            assert np.all(q[:, 4] == 1.0) and np.array_equal(q[:, :3], p[:, :3])
            assert np.all(q[:n // 2, 3] == HX + nd) and np.all(q[n // 2:, 3] == EX + nd)
            want[1].append(data[1])
            at[0] += n
            at[1] += n
        else:
            n = data[0].size // NF
            p = pts[2][at[2]:at[2] + n]
            w = np.empty(n)
            for c in set(p[:, 3].astype(int)):
                m = p[:, 3] == c
                w[m] = np.sqrt(R.loop_weights(p[m, :3], lo, hi, A, comp=c))
            R.check_weights(p[:, 4], w, p[:, :3])
            want[2].append(np.repeat(p[:, 4], NF) * data[0])
            xdiag.append(wgt * np.where(p[:, 3].astype(int) % 3 == fd, 0.5, -0.5))
            at[2] += n
    for w in range(3):
        assert at[w] == len(pts[w]), (w, at, len(pts[w]))
    cat = [np.concatenate(x) if x else np.zeros(0, dtype=complex) for x in want]
    return cat, (np.concatenate(xdiag) if xdiag else np.zeros(0))


# ------------------------------------------------------------------ 1, 2. lists
@gpu
def test_mode_is_fused_with_pairs(base):
    assert base["fused"] and base["tb"]["active"], base["tb"]


@gpu
def test_lists_against_oracle(base, oracle):
    f = base["o"]._fields()
    seen = [0, 0, 0]
    for h, lists, regs, orc in zip(base["hs"], base["lists"], OBJECTS, oracle):
        want, _ = expected(f, h, regs, orc)
        for w in range(3):
            assert lists[w].size == want[w].size == f.dft_list_size(h, w)
            if not want[w].size:
                continue
            seen[w] += 1
            big = np.max(np.abs(want[w]))
            err = np.max(np.abs(lists[w] - want[w]))
            print(f"object {h} list {w}: {want[w].size} values, err {err:.3e}, max {big:.3e}")
            assert big > 0
            if w == 1:
                assert np.array_equal(lists[w], want[w])  # the same add_dft arithmetic
            else:
                assert err <= 1e-12 * big
    assert all(seen), seen


# ------------------------------------------------------------------ 4. sums
def restated_force(f, h, lists, regs, orc):
    _, xdiag = expected(f, h, regs, orc)
    a, sa, na = R.pair_sum(lists[0], lists[1], 1.0, NF) if lists[0].size else (0.0, 0.0, 0)
    b, sb, nb = R.pair_sum(lists[2], lists[2], xdiag, NF) if lists[2].size else (0.0, 0.0, 0)
    return a + b, sa + sb, na + nb


@gpu
def test_force_against_sequential_numpy(base, oracle):
    f = base["o"]._fields()
    for h, lists, s, regs, orc in zip(base["hs"], base["lists"], base["sums"], OBJECTS, oracle):
        want, S, n = restated_force(f, h, lists, regs, orc)
        R.check_sum(s, want, S, n, f"object {h} force")
        assert np.array_equal(f.dft_force(h), s)  # two calls: the same bits


# ------------------------------------------------------------------ 5. modes
def run_variant(tb=None, calls=(STEPS,), objects=OBJECTS, read=False):
    o, hs = build(ProductSim, tb=tb, objects=objects)
    for k, n in enumerate(calls):
        o.step(n)
        if read and k == len(calls) // 2:
            mid = o._fields().dft_force(hs[0])
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
    o, hs = run_variant(tb=True, calls=(40, 40), objects=OBJECTS + [OBJECTS[3]])
    assert o._fields().tb_info()["active"]
    snap = snapshot(o, hs)
    same({"lists": snap["lists"][:4], "sums": snap["sums"][:4]}, base)
    same({"lists": snap["lists"][4:], "sums": snap["sums"][4:]},
         {"lists": base["lists"][3:], "sums": base["sums"][3:]})


# ------------------------------------------------------------------ 6. slabs
@gpu
@pytest.mark.parametrize("group", [GroupSim, GroupSim3])
def test_slabs_match_one_rank(base, oracle, group):
    o, hs = build(group)
    o.step(STEPS)
    p = base["o"]._fields()
    for h, hb, lists, regs, orc in zip(hs, base["hs"], base["lists"], OBJECTS, oracle):
        for x, y in zip(lists_of(o, h, 3), lists):
            assert np.array_equal(x, y)
        want, S, n = restated_force(p, hb, lists, regs, orc)
        R.check_sum(force(o, h), want, S, n, f"{group.__name__} object {h} force")


# ------------------------------------------------------------------ 7. data workflow
@gpu
def test_data_workflow(base, oracle, tmp_path):
    """As tests/test_gpu_dft_energy.py's: load_minus leaves the (quadratic) force unchanged
    bit for bit while the lists change sign."""
    h0, lists, s = base["hs"][0], base["lists"][0], base["sums"][0]
    o, hs = build(ProductSim)
    f, h = o._fields(), hs[0]
    for w in range(3):
        f.dft_load(h, w, lists[w])
    assert np.array_equal(f.dft_force(h), s)
    f.dft_scale(h, 2.0)
    assert np.array_equal(f.dft_force(h), 4.0 * s)
    for w in range(3):
        f.dft_load(h, w, lists[w], sign=-1)
        assert np.array_equal(f.dft_get(h, w), -lists[w])
    assert np.array_equal(f.dft_force(h), s)
    f.dft_scale(h, 1j)
    want, S, n = restated_force(base["o"]._fields(), h0, lists, OBJECTS[0], oracle[0])
    R.check_sum(f.dft_force(h), want, S, n, "scale(1j) force")
    path = str(tmp_path / "force.dft")
    base["o"]._fields().dft_save(h0, path)
    f.dft_load_file(h, path)
    for w in range(3):
        assert np.array_equal(f.dft_get(h, w), lists[w])
    assert np.array_equal(f.dft_force(h), s)
    with pytest.raises(RuntimeError,
                       match=r"meep: incorrect dataset size \(.*\) in load_dft .*:diag"):
        f.dft_load(h, 2, lists[2][:-1])
    with pytest.raises(RuntimeError, match="meep: incorrect dataset size"):
        f.dft_load_file(hs[1], path)


@gpu
def test_checkpoint_resume(base, tmp_path):
    a, _ = build(ProductSim)
    a.step(40)
    path = str(tmp_path / "force.mnl")
    a.dump(path)
    b, hb = build(ProductSim)
    b.load(path)
    b.step(STEPS - 40)
    same(snapshot(b, hb), base)


# ------------------------------------------------------------------ 10. errors
@gpu
def test_errors(base):
    f, h = base["o"]._fields(), base["hs"][0]
    with pytest.raises(RuntimeError, match="meep: cannot determine dft_force normal"):
        f.add_dft_force([([-0.3, -0.3, -0.3], [0.3, 0.3, 0.3], 0, 1.0)], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep: NO_DIRECTION dft_force is invalid"):
        f.add_dft_force([([0.3, -0.3, -0.3], [0.3, 0.3, 0.3], -1, 1.0)], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep:.*no regions"):
        f.add_dft_force([], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep: bad dft handle"):
        f.dft_force(99)
    with pytest.raises(RuntimeError, match="meep:.*no such list"):
        f.dft_get(h, 3)
    he = f.add_dft_energy([([-0.3, -0.3, -0.3], [0.3, 0.3, 0.3], 0, 1.0)], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep:.*not a force object"):
        f.dft_force(he)
    with pytest.raises(RuntimeError, match="meep:.*not available for energy and force"):
        f.dft_array(h, EX, 0)


# ------------------------------------------------------------------ 9. the reference's test
@gpu
def test_reference_force_value():
    """python/tests/test_force.py: -0.11039089113393187 to 7 places, and its decimation-10
    twin."""
    import meep_nl_amd as mp
    with open(GOLDEN) as fp:
        want = json.load(fp)["test_force"]["force"]
    assert want == -0.11039089113393187
    sim = mp.Simulation(cell_size=mp.Vector3(10, 10), resolution=20,
                        boundary_layers=[mp.PML(1.0)],
                        sources=[mp.Source(mp.GaussianSource(1.0, fwidth=1.0), component=mp.Ez,
                                           center=mp.Vector3())])
    fr = mp.ForceRegion(mp.Vector3(y=1.27), direction=mp.Y, size=mp.Vector3(4.38))
    myforce = sim.add_force(1.0, 0, 1, fr, decimation_factor=1)
    myforce_decimated = sim.add_force(1.0, 0, 1, fr, decimation_factor=10)
    sim.run(until_after_sources=mp.stop_when_fields_decayed(50, mp.Ez, mp.Vector3(), 1e-6))
    fdata = sim.get_force_data(myforce)
    assert isinstance(fdata, mp.ForceData) and fdata.offdiag1.size == 0 and np.any(fdata.diag != 0)
    sim.load_force_data(myforce, fdata)
    sim.display_forces(myforce)
    f = mp.get_forces(myforce)
    f10 = mp.get_forces(myforce_decimated)
    print(f"force {f[0]!r}, decimated {f10[0]!r}, reference {want!r}")
    assert mp.get_force_freqs(myforce) == [1.0]
    assert round(abs(f[0] - want), 7) == 0  # assertAlmostEqual (7 places)
    assert round(abs(f[0] - f10[0]), 7) == 0
