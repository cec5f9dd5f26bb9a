"""Seeded random family for the pair-step path: tb_plan's arithmetic
(where L2 starts and ends in x, lane origins, item widths, source holes, rim faces, rim z
cuts, narrow strips and their pairing, the DFT stores of step n+1) on grids nobody wrote down,
GPU against the CPU oracle bit for bit on every array.

draw(seed, ranks) returns the configuration as a plain dict and touches no backend; build()
applies it to the oracle or the product.  Everything is drawn in cell indices of the whole
grid (index j of an axis with n cells lies at (io / 2 + j) / 10, io = 0 or -(n - (n & 1)) with
center_origin) and turned into coordinates when it is applied.

Rules of the generator that keep every seed on the pair path (each one is a condition of
fused_possible / tb_usable, not a filter on results):
  * PML: cells(t) = int(10 t + 1.5) cells per face; the PML-free extent n - cells(lo) -
    cells(hi) is at least 48 along x and 16 along y and z (the lean box L is [cells(lo) + 1,
    n - cells(hi) - 1], L2 is L shrunk by 2 and x-aligned by at most 15 columns per side, and
    needs 8 points per axis); a thickness that violates it is drawn again;
  * an E_d current is not placed in the PML along d (a D source on a W-form point leaves the
    fused step, any_dsrc_w); along the other axes it lies anywhere, PML included;
  * no source point within two planes of the Lorentzian slab or of a slab (rank) face;
  * the slab and a volume source leave part of L2: checked with a conservative mirror of the
    planner's holes (_two_lower_bound), drawn again otherwise.
"""
import numpy as np
import pytest

from scenarios import ALL_COMPS, E_COMPS, GroupSim, GroupSim3, ProductSim, make_oracle, random_init, vol
from test_gpu_dft import _same_dft
from test_gpu_tb import _same

RES = 10
THICK = (0.1, 0.3, 0.5, 0.7, 1.0, 1.3)
FREQS = [0.2, 0.27, 0.33]
SEEDS = list(range(48))
SLAB_SEEDS = list(range(12))  # 0-5 two slabs, 6-11 three; 6 and 9 with a rim-only outer rank
BASE = {1: 41000, 2: 42000, 3: 43000}
TB_ZCHUNKS = (0, 1, 2, 3, 7, 33)
RIM_ZCHUNKS = (0, 5, 12, 40)
# DFT monitors keep this many cells from the cell's walls, so that no centred sample averages a
# wall row.  fields::initialize_field adds its values to every entry of a chunk's array
# (LOOP_OVER_VOL, src/initialize.cpp:154), entries no chunk owns included; nothing refreshes
# those, and the reference's (and the oracle's) DFT averages read them at the wall rows, where
# the product's one global grid holds none.  Measured with planes from wall to wall: a constant
# contribution per DFT update to the H list of one wall row, the same with pairs switched off,
# absent without initialize_field of B -- a property of initialize_field, not of the pair path.
WALL = 1.6


def _cells(t):
    """Cells of a PML chunk of thickness t (structure::use_pml: int(t a + 1 + 0.5))."""
    return int(t * RES + 1.5) if t > 0 else 0


def _pml_cells(pml):
    return [[_cells(t) if s in sides else 0 for s in (0, 1)] for t, sides in pml]


def lean_box(n, pml):
    """The lean box L (inclusive point indices per axis) of a one-rank grid."""
    pc = _pml_cells(pml)
    return [(pc[k][0] + 1, n[k] - pc[k][1] - 1) for k in range(3)]


def l2_box(n, pml, narrow=True):
    """tb_plan's L2 of a one-rank grid, before the holes: L shrunk by 2; in x the low edge at
    the next multiple of 16 (narrow strips) or at 4 mod 8, the high edge at 15 mod 16."""
    b = [[lo + 2, hi - 2] for lo, hi in lean_box(n, pml)]
    a16 = (b[0][0] + 15) // 16 * 16
    a4 = b[0][0] + (4 - b[0][0]) % 8
    b[0][0] = a16 if narrow and a16 <= a4 else a4
    b[0][1] = (b[0][1] + 1) // 16 * 16 - 1
    return [tuple(v) for v in b]


def slab_cells(nz, ranks):
    """The z cells [lo, hi) of every rank (slab_range: equal split, the first ranks one more)."""
    base, rem = divmod(nz, ranks)
    out = []
    for r in range(ranks):
        lo = r * base + min(r, rem)
        out.append((lo, lo + base + (1 if r < rem else 0)))
    return out


def rank_l2_planes(nz, pmlz, ranks):
    """Per rank the number of planes of its L2 (local planes 0 .. hi - lo; L is the interior
    clipped to [1, N - 2], L2 two planes inside it)."""
    pc = _pml_cells([pmlz])[0]
    out = []
    for lo, hi in slab_cells(nz, ranks):
        n2 = hi - lo + 1
        l_lo = max(max(pc[0] + 1 - lo, 0), 1)
        l_hi = min(min(nz - pc[1] - 1 - lo, n2 - 1), n2 - 2)
        out.append(max(0, (l_hi - 2) - (l_lo + 2) + 1))
    return out


def _pick(rng, lo, hi, bands=()):
    """A uniform draw from [lo, hi] minus the closed bands; None when nothing is left."""
    iv = [(lo, hi)]
    for a, b in bands:
        nxt = []
        for p, q in iv:
            if b < p or a > q:
                nxt.append((p, q))
                continue
            if a - p > 1e-9:
                nxt.append((p, a))
            if q - b > 1e-9:
                nxt.append((b, q))
        iv = nxt
    iv = [(p, q) for p, q in iv if q - p >= 0.5]
    if not iv:
        return None
    w = np.array([q - p for p, q in iv])
    p, q = iv[int(rng.choice(len(iv), p=w / w.sum()))]
    return float(rng.uniform(p + 0.05, q - 0.05))


def _two_lower_bound(d):
    """Points of L2 (default schedule) outside a conservative version of tb_plan's holes: every
    source point's hole taken one point wider than the planner's on each side, the x widening
    and the < 8 clamps as the planner does them.  Positive: the seed has a two-step region."""
    l2 = d["l2"]
    if any(hi - lo < 7 for lo, hi in l2):
        return 0
    two = np.ones([hi - lo + 1 for lo, hi in l2], dtype=bool)

    def carve(lo, hi):  # inclusive index box of source points
        h = [[int(np.floor(lo[k])) - 3, int(np.floor(hi[k])) + 4] for k in range(3)]
        if any(h[k][1] < l2[k][0] or h[k][0] > l2[k][1] for k in range(3)):
            return
        h[0][0] = max(h[0][0], 0) // 16 * 16
        while (h[0][1] + 1) % 8 != 4:
            h[0][1] += 1
        for k in range(3):
            h[k] = [max(h[k][0], l2[k][0]), min(h[k][1], l2[k][1])]
        if h[0][0] - l2[0][0] < 8:
            h[0][0] = l2[0][0]
        if l2[0][1] - h[0][1] < 8:
            h[0][1] = l2[0][1]
        two[tuple(slice(h[k][0] - l2[k][0], h[k][1] - l2[k][0] + 1) for k in range(3))] = False

    for s in d["srcs"]:
        carve(s["idx"], s["idx"])
    if d["vsrc"]:
        carve(d["vsrc"]["lo"], d["vsrc"]["hi"])
    if d["pol"]:
        pa, pb = d["pol"]["planes"]
        lo, hi = max(pa - 4, l2[2][0]), min(pb + 4, l2[2][1])
        if lo <= hi:
            two[:, :, lo - l2[2][0]:hi - l2[2][0] + 1] = False
    return int(two.sum())


def draw(seed, ranks=1):
    """The configuration of one seed: a plain dict of numbers (see the module docstring)."""
    rng = np.random.default_rng(BASE[ranks] + seed)
    rim_only = ranks == 3 and seed % 3 == 0
    wide = rng.random() < 0.3  # L2 wider than one two-step item: little x PML on a wide grid
    nx = int(rng.integers(146, 151)) if wide else int(rng.integers(72, 151))
    ny = int(rng.integers(36, 73))
    nz = int(rng.integers(60, 91)) if ranks > 1 else int(rng.integers(40, 91))
    if rim_only:
        nz = int(rng.integers(60, 73))
    n = [nx, ny, nz]
    d = {"seed": seed, "ranks": ranks, "n": n, "center_origin": bool(rng.integers(0, 2))}
    pml = []
    for ax in range(3):
        need = 48 if ax == 0 else 16
        absent = rng.random() < 0.25
        sides = ((0, 1), (0,), (1,))[int(rng.choice(3, p=[0.4, 0.3, 0.3]))]
        # (x: 1.0 more often -- the one thickness whose left rim is 16 columns, narrow strips)
        t = 1.0 if ax == 0 and rng.random() < 0.25 else float(rng.choice(THICK))
        while n[ax] - len(sides) * _cells(t) < need:
            t = float(rng.choice(THICK))
        if wide and ax == 0:  # L2's high edge at column 143 (no high-x PML), its low one <= 16
            absent, sides, t = rng.random() < 0.4, (0,), float(rng.choice(THICK[:5]))
        if rim_only and ax == 2:  # rank 0 keeps fewer than 8 planes inside its z PML
            absent, t, sides = False, 1.3, ((0, 1) if seed % 2 else (0,))
        pml.append((0.0, ()) if absent else (t, sides))
    d["pml"] = pml
    pc = _pml_cells(pml)
    d["lean"], d["l2"] = lean_box(n, pml), l2_box(n, pml)
    l2 = d["l2"]
    # dielectric: none, boxes (palette), or more than 256 distinct values (f64 chi1inv)
    d["diel"] = ("none", "boxes", "f64")[int(rng.integers(0, 3))]
    d["boxes"] = []
    for _ in range(int(rng.integers(1, 4)) if d["diel"] == "boxes" else 1 if d["diel"] == "f64" else 0):
        lo, hi = [], []
        for k in range(3):
            a, b = sorted(rng.uniform(0, n[k], 2))
            if d["diel"] == "f64":  # a third of every axis at least: thousands of values
                a, b = rng.uniform(0, n[k] / 3.0), rng.uniform(2.0 * n[k] / 3.0, n[k])
            lo.append(float(a))
            hi.append(float(b) + 1.5)
        d["boxes"].append({"lo": lo, "hi": hi, "eps": float(rng.uniform(1.5, 12.0))})
    # Lorentzian z slab over all of x-y (one rank only: multi-rank polarization chunks do not pair)
    d["pol"] = None
    if ranks == 1 and rng.random() < 0.3:
        for _ in range(50):
            nplanes = int(rng.integers(8, 26))
            pa = int(rng.integers(1, nz - nplanes))
            pb = pa + nplanes - 1
            left = max(0, (pa - 5) - l2[2][0] + 1) + max(0, l2[2][1] - (pb + 5) + 1)
            if left >= 4:
                d["pol"] = {"planes": (pa, pb), "omega": float(rng.uniform(0.6, 1.4)),
                            "gamma": float(rng.uniform(0.02, 0.2)), "sigma": float(rng.uniform(0.2, 1.0))}
                break
    # z bands no source point may lie in: the slab +- 2 planes, the rank faces +- 2 planes
    zbands = []
    if d["pol"]:
        zbands.append((d["pol"]["planes"][0] - 3.0, d["pol"]["planes"][1] + 3.0))
    for lo, _ in slab_cells(nz, ranks)[1:]:
        zbands.append((lo - 3.0, lo + 3.0))

    def bands(c, k):  # of an E_c current along axis k
        b = list(zbands) if k == 2 else []
        if k == c:  # not in the PML along its own direction
            b += [(-1e9, pc[k][0] + 1.0), (n[k] - pc[k][1] - 1.0, 1e9)]
        return b

    while True:  # sources, drawn again if they leave no two-step region (one rank)
        srcs, near = [], False
        want_near = rng.random() < 0.4
        for i in range(int(rng.integers(0, 5))):
            c = int(rng.integers(0, 3))
            idx = [_pick(rng, 1.0, n[k] - 1.0, bands(c, k)) for k in range(3)]
            if want_near and i == 0:  # within 3 cells of an L2 face
                k = int(rng.integers(0, 3 if ranks == 1 else 2))
                face = l2[k][int(rng.integers(0, 2))]
                for j in range(3):
                    v = _pick(rng, l2[j][0] + 0.0, l2[j][1] + 0.0, bands(c, j))
                    idx[j] = v if v is not None else idx[j]
                v = _pick(rng, face - 3.0, face + 3.0, bands(c, k))
                if v is not None:
                    idx[k], near = v, True
            srcs.append({"comp": c, "idx": idx, "freq": float(rng.uniform(0.15, 0.5)),
                         "width": float(rng.uniform(2.0, 10.0)), "end": float(rng.uniform(20.0, 100.0)),
                         "amp": float(rng.uniform(0.5, 2.0))})
        vsrc = None
        if rng.random() < 0.3:  # a volume source: a thin plane or a box of > 30 x 30 x 12 points
            c = int(rng.integers(0, 3))
            long_box = rng.random() < 0.55
            k0 = int(rng.integers(0, 3))  # the plane's normal
            lo, hi = [0.0] * 3, [0.0] * 3
            ok = True
            for k in range(3):
                if long_box:
                    size = float(rng.uniform(*((30.2, 40.0), (30.2, min(40.0, ny - 4.0)), (12.2, 20.0))[k]))
                elif k == k0:
                    size = 0.0
                else:  # part of the cross-section, or all of it
                    size = n[k] - 2.0 if rng.random() < 0.3 else float(rng.uniform(8.0, n[k] - 2.0))
                b = bands(c, k)
                if k == 2 and ranks > 1:  # inside one rank, away from its faces
                    size = min(size, 8.0)
                a = _pick(rng, 1.0, n[k] - 1.0, b)
                if a is None:
                    ok = False
                    break
                # slide the range until it fits [1, n - 1] minus the bands, shrink it otherwise
                lim_lo = max([1.0] + [q for p, q in b if q <= a])
                lim_hi = min([n[k] - 1.0] + [p for p, q in b if p >= a])
                size = min(size, lim_hi - lim_lo - 0.2)
                if long_box and size < (30.2, 30.2, 12.2)[k]:
                    ok = False
                    break
                lo[k] = float(rng.uniform(lim_lo + 0.05, lim_hi - size - 0.05)) if k != k0 or long_box else a
                hi[k] = lo[k] + size
            if ok:
                vsrc = {"comp": c, "lo": lo, "hi": hi, "long": bool(long_box),
                        "amp": float(rng.uniform(0.3, 1.0))}
        d["srcs"], d["near_face"], d["vsrc"] = srcs, near, vsrc
        d["two_lower_bound"] = _two_lower_bound(d)
        if ranks > 1 or d["two_lower_bound"] > 0:
            break
    # monitors: 1-5 flux planes (five: one more than the compact boxes), or one DFT-fields box
    d["flux"], d["dft_fields"] = [], None
    if rng.random() < 0.4:
        if rng.random() < 0.25:
            lo, hi = [], []
            for k in range(3):
                size = float(rng.uniform(4.0, min(40.0, n[k] - 2 * WALL - 1.0)))
                a = float(rng.uniform(WALL, n[k] - WALL - size))
                lo.append(a)
                hi.append(a + size)
            comps = sorted(int(c) for c in rng.choice(6, int(rng.integers(1, 4)), replace=False))
            d["dft_fields"] = {"comps": comps, "lo": lo, "hi": hi, "yee": bool(rng.integers(0, 2))}
        else:
            for _ in range(int(rng.choice([1, 2, 3, 4, 5, 5, 5]))):
                k0 = int(rng.integers(0, 3))
                lo, hi = [], []
                for k in range(3):
                    a, b = sorted(rng.uniform(WALL, n[k] - WALL, 2))
                    if k == k0:
                        b = a
                    elif rng.random() < 0.3:  # across the cell, through the PML on both sides
                        a, b = WALL, n[k] - WALL
                    lo.append(float(a))
                    hi.append(float(b))
                d["flux"].append({"lo": lo, "hi": hi, "dir": k0, "weight": float(rng.choice([1.0, -1.0, 0.5]))})
    # step calls: 3-6 calls, at most 30 steps, a one-step call, an even and an odd count among them
    while True:
        calls = [int(v) for v in rng.choice([1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], int(rng.integers(3, 7)))]
        if sum(calls) <= 30 and 1 in calls and any(v % 2 == 0 for v in calls) and \
                any(v % 2 and v > 1 for v in calls):
            break
    d["calls"] = calls
    # schedule (product only): half the seeds the default
    d["schedule"] = {}
    if rng.random() < 0.5:
        d["schedule"] = {"tb_ox": int(rng.integers(4, 125)), "tb_zchunk": int(rng.choice(TB_ZCHUNKS)),
                         "rim_zchunk": int(rng.choice(RIM_ZCHUNKS))}
        for name in ("narrow", "r1_beside", "src_guard", "dft_cmp"):
            d["schedule"][name] = int(rng.integers(0, 2))
    return d


def _coord(d, idx):
    """Coordinates of a position given in cell indices."""
    out = []
    for k in range(3):
        io = -(d["n"][k] - (d["n"][k] & 1)) if d["center_origin"] else 0
        out.append((0.5 * io + idx[k]) / RES)
    return out


def _inside(o, c, lo, hi):
    m = None
    for k, v in enumerate(o.coords(c)):
        mk = (v >= lo[k]) & (v <= hi[k])
        m = mk if m is None else m & mk
    return m


def build(make, seed, tb=True, schedule=None, ranks=1):
    """Apply draw(seed, ranks) to the oracle or the product and step it.  schedule: None for the
    seed's own drawn schedule, a dict for that one instead ({}: the default).  Returns (sim,
    flux handles, DFT-fields handle or None, the drawn dict)."""
    d = draw(seed, ranks)
    n = d["n"]
    o = vol(make, 3, [v / RES for v in n], RES, center_origin=d["center_origin"])
    assert tuple(o.shape()) == tuple(v + 1 for v in n)
    for ax, (t, sides) in enumerate(d["pml"]):
        if t > 0:
            o.add_pml(t, dirs=(ax,), sides=sides)
    if d["diel"] != "none":
        inv = {c: np.ones(o.shape()) for c in E_COMPS}
        for i, b in enumerate(d["boxes"]):
            lo, hi = _coord(d, b["lo"]), _coord(d, b["hi"])
            for c in E_COMPS:
                val = 1.0 / b["eps"]
                if d["diel"] == "f64":
                    val = 1.0 / np.random.default_rng(seed + 977 * c).uniform(1.0, 12.0, size=o.shape())
                inv[c] = np.where(_inside(o, c, lo, hi), val, inv[c])
        for c in E_COMPS:
            o.set_chi1inv(c, c, inv[c])
    if d["pol"]:
        pa, pb = d["pol"]["planes"]
        sig = np.zeros(o.shape())
        sig[:, :, pa:pb + 1] = d["pol"]["sigma"]
        o.add_lorentzian(d["pol"]["omega"], d["pol"]["gamma"], [sig, sig, sig])
    for s in d["srcs"]:
        o.add_gaussian_source(s["comp"], s["freq"], s["width"], -s["end"], s["end"],
                              tuple(_coord(d, s["idx"])), s["amp"])
    if d["vsrc"]:
        v = d["vsrc"]
        o.add_gaussian_volume_source(v["comp"], 0.25, 4.0, -40.0, 40.0, tuple(_coord(d, v["lo"])),
                                     tuple(_coord(d, v["hi"])), v["amp"])
    random_init(o, (6, 7, 8, 9, 10, 11), seed=seed)
    hs = [o.add_dft_flux([(_coord(d, f["lo"]), _coord(d, f["hi"]), f["dir"], f["weight"])], FREQS, 1)
          for f in d["flux"]]
    hf = None
    if d["dft_fields"]:
        f = d["dft_fields"]
        hf = o.add_dft_fields(f["comps"], _coord(d, f["lo"]), _coord(d, f["hi"]), FREQS, f["yee"], 1)
    if isinstance(o, ProductSim):
        sched = d["schedule"] if schedule is None else schedule
        for f in (o._all() if hasattr(o, "_all") else [o._fields()]):
            f.set_temporal_blocking(tb)
            for opt, val in sched.items():
                f.set_schedule(opt, val)
    for k in d["calls"]:
        o.step(k)
    return o, hs, hf, d


def _same_monitors(p, o, hs, hf, d, flux_exact=True):
    if hs:
        _same_dft(p, o, hs, flux_exact=flux_exact)
    if hf is not None:
        for c in d["dft_fields"]["comps"]:
            for i in range(len(FREQS)):
                a, b = p.dft_array(hf, c, i), o.dft_array(hf, c, i)
                assert a.shape == b.shape and a.size > 0, (c, a.shape, b.shape)
                np.testing.assert_array_equal(a, b, err_msg=f"DFT fields comp {c} freq {i}")


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", SEEDS)
def test_tb_fuzz_one_gpu(seed):
    """Pairs active with two-step and rim items on every seed; all twelve components, the
    per-point DFT values and the fluxes bitwise the oracle.

    Cell partition (seeds without a Lorentzian slab, whose chunks are no rim items): the own
    cells of the two-step items and of the rim items add up to the fused domain G, the product
    of (device extent - 1) over the axes.  On one rank the device extents are the grid's
    shape(), one more than the drawn cell counts, so G holds nx * ny * nz cells.  (Bitwise
    equality cannot see two items writing one point with the same value; the count can.)"""
    p, hs, hf, d = build(ProductSim, seed)
    f = p._fields()
    info = f.tb_info()
    print(seed, {k: d[k] for k in ("n", "pml", "l2", "calls", "schedule")}, info)
    assert f.fused_active() and info["active"], (d, info)
    assert info["tb_items"] > 0 and info["rim_items"] > 0, info
    if d["pol"]:
        assert info["tb_pol"], info
    else:
        g_cells = int(np.prod([v - 1 for v in p.shape()]))
        assert g_cells == int(np.prod(d["n"]))
        assert info["tb_cells"] + info["rim_cells"] == g_cells, (info, g_cells)
    if d["diel"] == "f64":
        assert not f.fused_palette()
    o, ho, hfo, _ = build(make_oracle, seed)
    assert p.t == o.t == sum(d["calls"])
    assert any(np.any(o.get_array(c) != 0) for c in ALL_COMPS)
    assert hs == ho and hf == hfo
    _same(p, o)
    _same_monitors(p, o, hs, hf, d)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", SEEDS[::3])
def test_tb_fuzz_equals_one_step(seed):
    """The seed one step at a time in the default schedule equals its pair run bit for bit (no
    oracle): with the test above failing too, a difference here is the pairs', none is the
    tile bodies'."""
    p = build(ProductSim, seed)[0]
    assert p._fields().tb_info()["active"]
    q = build(ProductSim, seed, tb=False, schedule={})[0]
    assert not q._fields().tb_info()["active"]
    _same(p, q)


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("seed", SLAB_SEEDS)
def test_tb_fuzz_slabs(seed):
    """Two (seeds 0-5) and three (6-11) z slabs: every rank steps pairs -- a rank whose slab
    holds fewer than 8 PML-free planes as two rim launches -- fields and per-point DFT values
    bitwise the oracle, flux sums (added over ranks) to 1e-12.  The ranks' own cells add up to
    nx * ny * nz (a rank's G spans its hi - lo planes).

    Seeds 5 and 11 (tb_ox 46 and 11: items with two-step neighbours on all six sides, inside
    a monitor's compact box) found the two-step kernel storing only the second step of such
    items for the monitor: 5856 of 49392 values of a flux plane and 928 of 5104 Ez values of
    a DFT-fields box differed, the fields did not (test_gpu_tb.py::
    test_tb_dft_compact_interior_items keeps the case)."""
    group = GroupSim if seed < 6 else GroupSim3
    p, hs, hf, d = build(group, seed, ranks=group.NRANKS)
    infos = [f.tb_info() for f in p._all()]
    print(seed, {k: d[k] for k in ("n", "pml", "calls", "schedule")}, infos)
    assert all(f.fused_active() for f in p._all())
    assert all(i["active"] for i in infos), infos
    planes = rank_l2_planes(d["n"][2], d["pml"][2], d["ranks"])
    for i, k in zip(infos, planes):
        assert (i["tb_items"] > 0) == (k >= 8), (infos, planes)
    assert sum(i["tb_cells"] + i["rim_cells"] for i in infos) == int(np.prod(d["n"])), infos
    o, ho, hfo, _ = build(make_oracle, seed, ranks=group.NRANKS)
    assert any(np.any(o.get_array(c) != 0) for c in ALL_COMPS)
    _same(p, o)
    _same_monitors(p, o, hs, hf, d, flux_exact=False)


def test_family_covers():
    """The draws alone (no backend): the family reaches the cases it was written for."""
    one = [draw(s) for s in SEEDS]
    slabs = [draw(s, 2 if s < 6 else 3) for s in SLAB_SEEDS]
    assert one[5] == draw(5)  # deterministic in the seed

    def count(ds, cond):
        return sum(1 for d in ds if cond(d))

    for d in one + slabs:
        pc = _pml_cells(d["pml"])
        assert 72 <= d["n"][0] <= 150 and 36 <= d["n"][1] <= 72 and 40 <= d["n"][2] <= 90
        assert d["n"][0] - sum(pc[0]) >= 48 and all(d["n"][k] - sum(pc[k]) >= 16 for k in (1, 2))
        assert all(hi - lo >= 7 for lo, hi in d["l2"]) and np.prod(d["n"]) <= 1.0e6
        assert 3 <= len(d["calls"]) <= 6 and sum(d["calls"]) <= 30
        for s in d["srcs"]:  # an E_c current outside the PML along c; away from slab and faces
            c, z = s["comp"], s["idx"][2]
            assert pc[c][0] + 1 <= s["idx"][c] <= d["n"][c] - pc[c][1] - 1
            if d["pol"]:
                assert not d["pol"]["planes"][0] - 3 < z < d["pol"]["planes"][1] + 3
            for lo, _ in slab_cells(d["n"][2], d["ranks"])[1:]:
                assert abs(z - lo) >= 3
        if d["vsrc"]:
            for lo, _ in slab_cells(d["n"][2], d["ranks"])[1:]:
                assert d["vsrc"]["hi"][2] <= lo - 3 or d["vsrc"]["lo"][2] >= lo + 3
    for d in one:
        assert d["two_lower_bound"] > 0, d["seed"]
    xs = [d["n"][0] for d in one]
    assert count(one, lambda d: d["n"][0] % 8) >= len(one) // 2 and sum(x % 2 for x in xs) >= len(one) // 4
    assert count(one, lambda d: 0 not in d["pml"][0][1]) >= 6  # no PML on the low-x face
    assert count(one, lambda d: 1 not in d["pml"][0][1]) >= 6
    assert count(one, lambda d: d["n"][0] - sum(_pml_cells(d["pml"])[0]) >= 131) >= 6
    # two x items per row for certain: L2 wider than 124 columns in the default schedule
    assert count(one, lambda d: d["l2"][0][1] - d["l2"][0][0] + 1 > 124 and not d["schedule"]) >= 2
    assert count(one, lambda d: d["l2"][0][0] == 4) >= 4  # the 4-column left rim
    assert count(one, lambda d: d["l2"][0][0] == 16) >= 4  # the 16-column one (narrow strips)
    assert count(one, lambda d: d["n"][0] % 8) >= 10
    assert count(one, lambda d: len({t for t, s in d["pml"] if t > 0}) > 1) >= 6
    assert count(one, lambda d: any(t == 0.1 for t, s in d["pml"])) >= 4
    assert count(one, lambda d: d["pol"]) >= 8
    assert count(one, lambda d: d["near_face"]) >= 8
    assert count(one, lambda d: d["vsrc"] and d["vsrc"]["long"]) >= 4
    assert count(one, lambda d: len(d["flux"]) == 5) >= 4
    assert count(one, lambda d: d["dft_fields"]) >= 2
    assert count(one, lambda d: not d["schedule"]) >= 16 and count(one, lambda d: d["schedule"]) >= 16
    assert {d["diel"] for d in one} == {"none", "boxes", "f64"}
    assert not any(d["pol"] for d in slabs)
    assert all(60 <= d["n"][2] <= 90 for d in slabs)
    rim_only = [d for d in slabs[6:]
                if min(rank_l2_planes(d["n"][2], d["pml"][2], 3)[0::2]) < 8]
    assert len(rim_only) >= 2
