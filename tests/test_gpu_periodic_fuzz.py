"""The seeded random family of periodic cells (tests/periodic_fuzz.py: the generator and its
rules) on the GPU against the CPU oracle's metal supercell of 3 replicas per periodic axis.

Per seed: every one of the 12 arrays of the cell, ghost planes included, bit for bit; the run
in the seed's schedule of calls with reads in between, and the run with set_fused(False), bit
for bit equal to the single call; the fused mode exactly where the generator's rule expects it;
the interior dft_fields box bit for bit (E and H against the oracle; the oracle's dft_fields
take no D or B, those compare with the product's own metal supercell, which
tests/test_gpu_dft_energy.py pins to the oracle); the flux within (N + 64) 2^-53 sum |term| of
the oracle's, the sum taken over the oracle's lists; and the flux plane's dft_points against
the region's centred points.  The light-cone bound of every seed is checked on the oracle
alone by tests/test_periodic_cpu.py, which also counts what the seed lists cover."""
import functools
import itertools

import numpy as np
import pytest

import periodic_cases as pc
import periodic_fuzz as pf
from dft_restate import U, boundary_weights_1d
from test_gpu_periodic import _arrays, _mode, _same

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

NF = len(pf.FREQS)


def _monitors(o, hs, cfg):
    """what the monitors hold: dft_fields arrays per (component, frequency), flux, flux lists"""
    out = {}
    for key in ("eh", "db"):
        if key in hs:
            for c in cfg["dft"]["comps"]:
                if (c < 6) == (key == "eh"):
                    for k in range(NF):
                        out[(c, k)] = o.dft_array(hs[key], c, k)
    out["flux"] = np.asarray(o.flux(hs["flux"]))
    out["lists"] = [o.dft_data(hs["flux"], w) for w in (0, 1)]
    return out


@functools.lru_cache(maxsize=None)
def _oracle(seed, ranks):
    from scenarios import make_oracle
    cfg = pf.draw(seed, ranks)
    sc, o, hs = pf.build(make_oracle, cfg, 3)
    o.step(cfg["T"])
    return {c: sc.central(o.get_array(c)).copy() for c in pc.ALL_COMPS}, _monitors(o, hs, cfg)


def _run(cfg, maker, R=1, schedule=None, fused=True):
    sc, p, hs = pf.build(maker, cfg, R, fused=fused)
    if schedule is None:
        p.step(cfg["T"])
    else:
        for k in schedule:
            p.step(k)
            for c in (0, 4, 8):
                p.get_array(c)
    mode = _mode(p) if R == 1 else None
    return sc, p, hs, mode


def _region_points(cfg):
    """the centred points (half-pixels) of the flux region, every one once"""
    f = cfg["flux"]
    per_axis = []
    for d in range(3):
        if d not in pc.axes_of(cfg["dim"]):
            per_axis.append([0])
            continue
        i0, w, _ = boundary_weights_1d(f["lo"][d] / (2 * pc.A), f["hi"][d] / (2 * pc.A), pc.A, 1)
        per_axis.append([i0 + 2 * k for k in range(len(w))])
    return sorted(itertools.product(*per_axis))


def _check_seed(seed, ranks):
    cfg = pf.draw(seed, ranks)
    print(cfg)
    maker = pc.product_makers()[ranks - 1]
    T = cfg["T"]
    want, wmon = _oracle(seed, ranks)
    assert all(np.any(want[c] != 0) for c in pc.ALL_COMPS)
    sc, p, hs, mode = _run(cfg, maker)
    assert mode == [int(cfg["fused_expected"])] * ranks, (mode, cfg["fused_expected"])
    got, gmon = _arrays(p), _monitors(p, hs, cfg)
    _same(got, want, "seed %d, %d steps" % (seed, T))
    # ---- monitors against the oracle
    for key, a in gmon.items():
        if isinstance(key, tuple) and key[0] < 6:
            b = wmon[key]
            assert a.shape == b.shape and np.any(b != 0), key
            assert np.array_equal(a, b), (key, float(np.max(np.abs(a - b))))
    e, h = (x.reshape(-1, NF) for x in wmon["lists"])
    terms = (e * np.conj(h)).real
    s, n = np.abs(terms).sum(axis=0), terms.shape[0]
    err = np.abs(gmon["flux"] - wmon["flux"])
    print("flux", gmon["flux"], wmon["flux"], "err / bound", err / ((n + 64) * U * s))
    assert np.all(wmon["flux"] != 0) and np.all(err <= (n + 64) * U * s)
    # ---- the flux plane's points: the region's centred points, every one once.  Image chunks
    # report the region's own positions, not the owned points they sample, so this is the
    # statement before folding by the period; a full-period region's two half-weight end points
    # fold onto each other by construction
    region = _region_points(cfg)
    f0 = p._fields()
    for which in (0, 1):
        pts = f0.dft_points(hs["flux"], which)
        assert len(pts) == gmon["lists"][which].size // NF
        for comp in np.unique(pts[:, 3]):
            sel = pts[pts[:, 3] == comp]
            half = np.rint(sel[:, :3] * 2 * pc.A).astype(int)
            assert np.max(np.abs(half - sel[:, :3] * 2 * pc.A)) < 1e-9
            assert sorted(tuple(int(v) for v in hh) for hh in half) == region, (which, comp)
    # ---- D and B of the dft_fields box against the product's own metal supercell
    if "db" in hs:
        from scenarios import ProductSim
        _, q, qhs, _ = _run(cfg, ProductSim, R=3)
        qmon = _monitors(q, qhs, cfg)
        for key, a in gmon.items():
            if isinstance(key, tuple) and key[0] >= 6:
                b = qmon[key]
                assert a.shape == b.shape and np.any(b != 0), key
                assert np.array_equal(a, b), (key, float(np.max(np.abs(a - b))))
    # ---- the same bits in the seed's schedule of calls and without the fused step

    def same_run(other, what):
        _, q, qhs, qmode = other
        _same(_arrays(q), got, what)
        qmon = _monitors(q, qhs, cfg)
        for key, a in gmon.items():
            b = qmon[key]
            for x, y in zip(a, b) if key == "lists" else [(a, b)]:
                assert np.array_equal(x, y), (what, key)
        return qmode
    same_run(_run(cfg, maker, schedule=cfg["schedule"]), "schedule %s" % cfg["schedule"])
    assert same_run(_run(cfg, maker, fused=False), "set_fused(False)") == [0] * ranks


@pytest.mark.parametrize("seed", pf.SEEDS[1])
def test_one_rank(seed):
    _check_seed(seed, 1)


@pytest.mark.parametrize("ranks,seed", [(r, s) for r in (2, 3) for s in pf.SEEDS[r]])
def test_slabs(ranks, seed):
    _check_seed(seed, ranks)


def test_h_dft_on_the_centred_row_beside_a_low_pml_wall():
    """What seed 14 of an earlier draw found, in a metal cell: a flux plane and an H dft_fields
    box whose first centred row along y (PML on both sides) averages H_y on the wall plane
    y = 0.  No step updates that plane; it belongs to the low PML chunk, where H is an array of
    its own, and initialize_field(B_y) adds to B there after the first H update has made H's
    copy.  The sampler has to read the chunk's H, as the reference does: bit for bit the
    oracle's lists, with B random and non-zero on the wall plane."""
    from scenarios import ProductSim, make_oracle
    case = dict(dim=3, n=(12, 14, 16), per=(), pml=(1,))
    res = []
    for mk in (ProductSim, make_oracle):
        sc = pc.Scene(case, "plain", 1)
        o = pc.configure(sc.make(mk), sc)
        lo, hi = [2 / pc.A, 1 / pc.A, 6 / pc.A], [10 / pc.A, 8 / pc.A, 6 / pc.A]
        hx = o.add_dft_flux([(lo, hi, 2, 1.0)], pf.FREQS, 1)
        hf = o.add_dft_fields([3, 4, 5], lo, [10 / pc.A, 8 / pc.A, 9 / pc.A], pf.FREQS, False, 1)
        o.step(12)
        res.append(([o.dft_data(hx, w) for w in (0, 1)], np.asarray(o.flux(hx)),
                    [o.dft_array(hf, c, 1) for c in (3, 4, 5)], o.get_array(10)))
    (pl, pflux, pa, pb), (ol, oflux, oa, ob) = res
    assert np.array_equal(pb, ob)
    for a, b in zip(pl + pa, ol + oa):
        assert a.shape == b.shape and np.any(b != 0)
        assert np.array_equal(a, b), float(np.max(np.abs(a - b)))
    e, h = (x.reshape(-1, NF) for x in ol)
    terms = (e * np.conj(h)).real
    bound = (terms.shape[0] + 64) * U * np.abs(terms).sum(axis=0)
    assert np.all(oflux != 0) and np.all(np.abs(pflux - oflux) <= bound)


@pytest.mark.parametrize("family", ["aniso", "nr+lorentz"])
def test_pml_along_two_directions_is_refused(family):
    """The combination the generator never draws (its rule "Walls"): refused by name."""
    case = dict(dim=3, n=(12, 14, 14), per=(0,), pml=(1, 2))
    sc = pc.Scene(case, family, 1)
    with pytest.raises(RuntimeError, match="meep:.*PML along two directions"):
        pc.configure(sc.make(pc.product_makers()[0]), sc)
