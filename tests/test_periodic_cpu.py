"""Periodic boundaries (k = 0, real fields), the checks that need no device: the light-cone
bound of the supercell parity tests on the oracle alone, the lattice-shift loop of
loop_in_chunks against a hand-worked case, the Python argument handling, and the wrap kernel's
thread table as a stand-alone program under the address and undefined-behaviour sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import periodic_cases as pc
import periodic_fuzz as pf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every (case, family) the GPU file uses, with its step count
GPU_CONFIGS = [(1, "plain"), (2, "plain"), (3, "plain"), (4, "plain"), (5, "plain"),
               ("2d", "plain")] + [(4, f) for f in pc.FAMILIES if f != "plain"]
# and tests/test_gpu_periodic_monitors.py
GPU_CONFIGS += [(4, "lorentz4"), ("2dy", "plain"), ("2dy", "lorentz")] + \
    [(c, f) for c in (5, "2dy") for f in pc.REACH2]


def test_steps_bound_is_the_stated_condition():
    # s * T <= m - 2 with m = (R - 1) / 2 * n_d
    assert pc.steps_bound(1, 3, "plain") == 68 and pc.steps_bound(2, 3, "plain") == 31
    assert pc.steps_bound(3, 3, "plain") == 38 and pc.steps_bound(4, 3, "plain") == 18
    assert pc.steps_bound(5, 3, "plain") == 12 and pc.steps_bound(4, 3, "nr") == 9
    assert pc.steps_bound(4, 5, "plain") == 38


@pytest.mark.parametrize("case,family", GPU_CONFIGS)
def test_light_cone_bound_on_the_oracle(case, family):
    """R against R + 2 replicas: bitwise equal on the central replica through T, every array
    (ghost planes of the replica included), and not a comparison of zeros."""
    T = pc.steps_bound(case, 3, family)
    s3, o3 = pc.run_oracle(case, family, 3, T)
    s5, o5 = pc.run_oracle(case, family, 5, T)
    nonzero = 0
    for c in pc.ALL_COMPS:
        a, b = s3.central(o3.get_array(c)), s5.central(o5.get_array(c))
        assert a.shape == b.shape
        assert np.array_equal(a, b), (case, family, c, float(np.max(np.abs(a - b))))
        nonzero += bool(np.any(a != 0))
    assert nonzero == 12


ALL_SEEDS = [(r, s) for r in (1, 2, 3) for s in pf.SEEDS[r]]


@pytest.mark.parametrize("ranks,seed", ALL_SEEDS)
def test_light_cone_bound_of_the_random_family(ranks, seed):
    """Every seed of tests/test_gpu_periodic_fuzz.py: 3 against 5 replicas on the oracle alone,
    the central replica bitwise equal through the seed's T, all 12 arrays non-zero."""
    from scenarios import make_oracle
    cfg = pf.draw(seed, ranks)
    got = []
    for R in (3, 5):
        sc, o, _ = pf.build(make_oracle, cfg, R, monitors=False)
        o.step(cfg["T"])
        got.append({c: sc.central(o.get_array(c)).copy() for c in pc.ALL_COMPS})
    for c in pc.ALL_COMPS:
        assert np.array_equal(got[0][c], got[1][c]), (seed, c)
        assert np.any(got[0][c] != 0), (seed, c)


def test_draw_is_a_function_of_the_seed():
    assert pf.draw(7) == pf.draw(7) and pf.draw(7) != pf.draw(8)
    assert pf.draw(100, 2)["ranks"] == 2 and pf.draw(100, 2) != pf.draw(100, 3)


def test_random_family_coverage():
    """What the committed seed lists cover, counted from draw alone."""
    one = [pf.draw(s, 1) for s in pf.SEEDS[1]]
    cfgs = one + [pf.draw(s, r) for r in (2, 3) for s in pf.SEEDS[r]]
    assert len(one) == 40 and [len(pf.SEEDS[r]) for r in (2, 3)] == [4, 4]

    def count(pred, over=cfgs):
        return sum(bool(pred(c)) for c in over)
    for dim, per in pf.SUBSETS:
        assert count(lambda c: c["dim"] == dim and c["per"] == per) >= (3 if dim == 3 else 2), per
    for fam in pc.FAMILIES:
        assert count(lambda c: c["family"] == fam) >= 4, fam
    for fam in pf.FAMILIES[len(pc.FAMILIES):]:  # the two combinations
        assert count(lambda c: c["family"] == fam) >= 3, fam
    # each clause of the fused rule decides the mode of a seed that is otherwise fusable
    alone = [c for c in one if c["dim"] == 3 and c["family"] in pf.FUSABLE and not c["fused_expected"]]
    assert any(all(not s["in_pml"] for s in c["sources"]) for c in alone)       # an H source
    assert any(all(s["comp"] < 3 for s in c["sources"]) for c in alone)         # an E_d in PML

    def on_seam(c):
        return any(s["kind"] == "point" and any(s["pos"][d] == 0 for d in c["per"])
                   for s in c["sources"])

    def sides(c):  # per non-periodic axis the set of sides with PML
        out = {d: set() for d in pc.axes_of(c["dim"]) if d not in c["per"]}
        for d, s, _ in c["pml"]:
            out[d].add(s)
        return out

    def sticks_out(c):
        return any(s["kind"] == "volume" and any(
            (s["lo"][d] < 0) != (s["hi"][d] > 2 * c["n"][d]) for d in c["per"])
            for s in c["sources"])
    assert count(on_seam) >= 8
    assert count(lambda c: any(s["comp"] >= 3 for s in c["sources"])) >= 5
    assert count(lambda c: any(len(v) == 1 for v in sides(c).values())) >= 6
    assert count(lambda c: any(len(v) < 2 for v in sides(c).values())) >= 4  # a metal wall
    assert count(lambda c: c["n"][0] > 64) >= 4
    assert count(lambda c: c["n"][0] % 2 == 0) >= 10  # odd point count (n + 1)
    assert count(lambda c: c["n"][0] % 2 == 1) >= 10
    assert count(sticks_out) >= 6
    assert count(lambda c: c["fused_expected"], one) >= 20
    # the rules of the product
    for c in cfgs:
        assert not any(d in c["per"] for d, _, _ in c["pml"])
        if pc.reach(c["family"]) == 2:
            assert len({d for d, _, _ in c["pml"]}) <= 1
        for d, v in sides(c).items():
            assert c["n"][d] - sum(t for dd, _, t in c["pml"] if dd == d) >= 6
        assert all(10 <= c["n"][d] for d in c["per"]) and sum(c["schedule"]) == c["T"] >= 1


def test_light_cone_is_sharp_enough_to_matter():
    """Well past the bound the wall is felt: the supercells differ, so the comparison above can
    fail."""
    T = 3 * pc.steps_bound(5, 3, "plain")
    s3, o3 = pc.run_oracle(5, "plain", 3, T)
    s5, o5 = pc.run_oracle(5, "plain", 5, T)
    assert any(not np.array_equal(s3.central(o3.get_array(c)), s5.central(o5.get_array(c)))
               for c in pc.ALL_COMPS)


def test_shift_loop_hand_worked():
    """A full-period region of 4 cells (a = 1, cell [0, 4]) on a grid unshifted along the axis:
    grid points 0, 2, .., 8 (half-pixels) with weights 1/2, 1, 1, 1, 1/2.  Point 0 is not
    owned.  Shift -1 comes first and gives the image chunk: the low plane's weight 1/2 on the
    owned point 8; shift 0 gives the chunk over the owned points 2 .. 8 with 1, 1, 1, 1/2;
    shift +1 is empty."""
    chunks = pc.shift_loop_1d(0.0, 4.0, 4, 1.0, sh=0)
    assert [(c[0], c[1]) for c in chunks] == [(8, -8), (2, 0)]
    assert chunks[0][2].tolist() == [0.5]
    assert chunks[1][2].tolist() == [1.0, 1.0, 1.0, 0.5]
    # the seam point gets 1/2 + 1/2, every point of the period weight 1: the period's length
    assert sum(c[2].sum() for c in chunks) == 4.0
    # a grid shifted along the axis (points 1, 3, 5, 7 owned): the region's grid points are
    # -1 .. 9; the images of -1 and 9 land on 7 and 1 with the two end weights
    chunks = pc.shift_loop_1d(0.0, 4.0, 4, 1.0, sh=1)
    assert [(c[0], c[1]) for c in chunks] == [(7, -8), (1, 0), (1, 8)]
    assert abs(sum(c[2].sum() for c in chunks) - 4.0) < 1e-15
    # a region strictly inside the cell has no image
    assert [c[1] for c in pc.shift_loop_1d(1.0, 3.0, 4, 1.0, sh=0)] == [0]


def test_simulation_k_point_arguments():
    import meep_nl_amd as mp
    src = [mp.Source(mp.GaussianSource(0.5, fwidth=0.2), mp.Ex, center=mp.Vector3())]
    kw = dict(cell_size=mp.Vector3(2, 2, 4), resolution=8, sources=src)
    assert mp.Simulation(**kw).periodic_directions == ()
    assert mp.Simulation(k_point=False, **kw).periodic_directions == ()
    sim = mp.Simulation(k_point=mp.Vector3(), boundary_layers=[mp.PML(0.5, direction=mp.Z)], **kw)
    assert sim.periodic_directions == (0, 1)
    assert mp.Simulation(k_point=mp.Vector3(), **kw).periodic_directions == (0, 1, 2)
    assert mp.Simulation(k_point=mp.Vector3(), boundary_layers=[mp.PML(0.5)],
                         **kw).periodic_directions == ()
    with pytest.raises(NotImplementedError, match="complex fields"):
        mp.Simulation(k_point=mp.Vector3(0.1, 0, 0), **kw)
    with pytest.raises(RuntimeError, match="meep:.*PML along a periodic direction"):
        mp.Simulation(k_point=mp.Vector3(), boundary_layers=[mp.PML(0.5, direction=mp.X,
                                                                     side=mp.Low)], **kw)
    with pytest.raises(RuntimeError, match="meep:.*1-D"):
        mp.Simulation(cell_size=mp.Vector3(0, 0, 4), resolution=8, k_point=mp.Vector3())
    with pytest.raises(NotImplementedError):
        mp.Simulation(force_complex_fields=True, **kw)
    with pytest.raises(NotImplementedError):
        mp.Simulation(symmetries=[object()], **kw)
    sim2 = mp.Simulation(cell_size=mp.Vector3(2, 3, 0), resolution=8, k_point=mp.Vector3(),
                         boundary_layers=[mp.PML(0.5, direction=mp.Y)])
    assert sim2.periodic_directions == (0,)


def test_abi_declares_use_bloch():
    hdr = open(os.path.join(ROOT, "include", "meep_nl_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int mnl_fields_use_bloch\(mnl_fields \*f, int dir, double k_re, "
                     r"double k_im\);", code)
    assert re.search(r"int mnl_fields_boundary\(mnl_fields \*f, int dir, int side, int \*kind\);",
                     code)
    assert "fields::use_bloch" in hdr
    from meep_nl_amd import _lib, core
    assert {"mnl_fields_use_bloch", "mnl_fields_boundary"} <= set(_lib.exported_symbols())
    assert callable(core.Fields.use_bloch) and callable(core.Fields.boundary)


def test_near2far_refusal_still_names_periodic_boundaries():
    src = open(os.path.join(ROOT, "meep_nl_amd", "csrc", "mnl_dft.cpp")).read()
    msg = re.search(r'nperiods > 1\)\s*return fail\(("[^;]*)\);', src, re.S).group(1)
    assert re.search(r"periodic", msg)


def test_wrap_table_under_sanitizers(tmp_path):
    """The wrap kernel's thread table (mnl_wrap.hpp) as a stand-alone program with its own
    main, built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "wrap_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "meep_nl_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpu", "wrap_table_main.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
