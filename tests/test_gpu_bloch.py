"""Complex fields and Bloch boundaries with k != 0 on the GPU.

1. Complex fields at k = 0, bit for bit: part 0 is the real-field run (and the oracle's metal
   supercell), part 1 the real run with the amplitude -i A and the imaginary initial fields.
2. The zone edge k = a / (2 n_d): every phase is exactly +-1, the parts decouple, and each
   equals the central replica of the oracle's supercell whose replicas' sources carry
   (-1)^(odd shifts), bit for bit on every array with its negated ghost planes.
3. The reference's own known answers with use_bloch(k != 0) (tests/known_results.cpp), rel 1e-5.
4. A generic k against the oracle's two phased supercell runs, within 1e-9 of each array's
   largest magnitude (the tolerance of tests/three_d.cpp:35-39 of the reference).
4b. A complex k on the device: every ghost point is the table's phase times its owner.
5. (-k, conjugate initial fields) gives the conjugate fields, bit for bit.
5b. Period n against 2 n at a generic k, within 1e-9.
6. DFT on complex fields: dft_fields against two real runs, buffered updates, an image chunk's
   phase, the full-period flux plane and an interior box against the phased supercell,
   Simulation's flux calls.
7. 2 and 3 in-process slabs, bit for bit one rank.
8. Every new error.

Every cell is one of tests/periodic_cases.py; the 3-D ones step in the fused mode (asserted),
and are repeated with set_fused(False) and with one step per call, bit for bit.
"""
import json
import math
import os

import numpy as np
import pytest

import bloch_cases as bc
import periodic_cases as pc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parts(o):
    return {p: {c: o.get_array(c, p) for c in pc.ALL_COMPS} for p in (0, 1)}


def _same(a, b, what):
    for c in pc.ALL_COMPS:
        assert a[c].shape == b[c].shape, (what, c)
        assert np.array_equal(a[c], b[c]), (what, c, float(np.max(np.abs(a[c] - b[c]))))


def _mode(o):
    return int(o._fields().fused_active())


def _nofuse(o):
    o._fields().set_fused(False)


def _fused_expected(case, family):
    # the rule of tests/test_gpu_periodic.py: 3-D cells step fused, plain and with a
    # Lorentzian slab; the other families and 2-D cells have no fused step
    return int(pc.case_of(case)["dim"] == 3 and family in ("plain", "lorentz"))


def _variants(case, family, T, want, **kw):
    """The complex run in T steps per call (fused where expected), with set_fused(False) and
    with one step per call: each part bit for bit `want`."""
    _, p = bc.run_bloch(case, family, T, **kw)
    assert not p._fields().is_real
    assert _mode(p) == _fused_expected(case, family)
    assert not p._fields().tb_info()["active"]  # no pairs of steps on complex fields
    got = _parts(p)
    for part in (0, 1):
        _same(got[part], want[part], "part %d" % part)
    if _fused_expected(case, family):
        _, q = bc.run_bloch(case, family, T, before=_nofuse, **kw)
        assert _mode(q) == 0
        g2 = _parts(q)
        for part in (0, 1):
            _same(g2[part], got[part], "set_fused(False), part %d" % part)
    _, q = bc.run_bloch(case, family, T, chunks=[1] * T, **kw)
    g2 = _parts(q)
    for part in (0, 1):
        _same(g2[part], got[part], "one step per call, part %d" % part)
    return got


# ---------------------------------------------------------------- 1. complex fields, k = 0
K0_CASES = [(4, f) for f in bc.FAMILIES] + [(1, "plain"), (5, "plain"), ("2d", "plain")]


@pytest.mark.parametrize("case, family", K0_CASES)
def test_complex_k0_is_two_real_runs(case, family):
    """Amplitude 1 and complex initial fields: part 0 is the real-field product run and the
    oracle's metal supercell of tests/periodic_cases.py; part 1 the real run of -i A with the
    imaginary initial fields (product and oracle)."""
    T = pc.steps_bound(case, 3, family)
    kw = dict(planar=True, init=True)
    want = bc.oracle_parts(case, family, T, 1.0, (0, 0, 0), **kw)
    _same(want[0], pc.oracle_central(case, family, T), "the scene of periodic_cases")
    assert all(np.any(want[1][c] != 0) for c in pc.ALL_COMPS)
    got = _variants(case, family, T, want, **kw)
    for part in (0, 1):
        _, r = bc.run_real(case, family, T, part, **kw)
        _same({c: r.get_array(c) for c in pc.ALL_COMPS}, got[part], "real product run %d" % part)


def test_imaginary_amplitude_goes_to_part_1():
    """A = i b: imag((0, b) s) = b real(s) exactly, so part 1 is the real run with b."""
    T = pc.steps_bound(4, 3, "plain")
    _, p = bc.run_bloch(4, "plain", T, amp=0.7j, planar=True)
    _, r = bc.run_real(4, "plain", T, 0, amp=0.7, planar=True)
    got = _parts(p)
    _same(got[1], {c: r.get_array(c) for c in pc.ALL_COMPS}, "part 1")
    f, at = p._fields(), (2 / bc.A, 2.2 / bc.A, 16.5 / bc.A)
    z = f.get_field_complex(1, at)
    assert z.real == f.get_field(1, at)
    assert z.imag == r._fields().get_field(1, at) and z.imag != 0
    lo, hi = (0.0, 0.0, 2.0), (1.0, 1.0, 2.0)
    sl = f.get_array_slice(1, lo, hi, cmplx=True)
    assert np.array_equal(sl.imag, r._fields().get_array_slice(1, lo, hi))
    assert np.array_equal(sl.real, f.get_array_slice(1, lo, hi)) and np.any(sl.imag != 0)


@pytest.mark.parametrize("case", [4, "2d"])
def test_general_amplitude_k0(case):
    """A general complex amplitude: part 0 is the oracle with A, part 1 the oracle with -i A,
    bit for bit (the library hands part 1 the amplitude (imag A, -real A), whose product with
    the current is imag(A J) with the same two products and one addition)."""
    T = pc.steps_bound(case, 3, "plain")
    want = bc.oracle_parts(case, "plain", T, bc.AMP, (0, 0, 0), planar=True)
    _variants(case, "plain", T, want, amp=bc.AMP, planar=True)


def test_energy_adds_both_parts():
    T = pc.steps_bound(4, 3, "plain")
    _, p = bc.run_bloch(4, "plain", T, amp=bc.AMP, planar=True)
    e = p.field_energy()
    parts = []
    for part in (0, 1):
        _, r = bc.run_real(4, "plain", T, part, amp=bc.AMP, planar=True)
        parts.append(r.field_energy())
    assert parts[0] > 0 and parts[1] > 0 and e == parts[0] + parts[1]
    z = p._fields().get_array(1, cmplx=True)
    assert z.dtype == np.complex128 and np.array_equal(z.imag, p.get_array(1, 1))


# ---------------------------------------------------------------- 2. the zone edge
@pytest.mark.parametrize("case, axes", bc.ZONE_CASES)
def test_zone_edge_parity(case, axes):
    k = bc.zone_edge_k(case, axes)
    T = pc.steps_bound(case, 3, "plain")
    want = bc.oracle_parts(case, "plain", T, bc.AMP, k)
    assert all(np.any(want[part][c] != 0) for part in (0, 1) for c in pc.ALL_COMPS)
    got = _variants(case, "plain", T, want, amp=bc.AMP, k=k)
    # x is at the zone edge in every case; Ez is unshifted along x: ghost plane 0 = -plane n
    for part in (0, 1):
        ez = got[part][2]
        assert np.array_equal(ez[0], -ez[-1]) and np.any(ez[0] != 0)


@pytest.mark.parametrize("family", [f for f in bc.FAMILIES if f != "plain"])
def test_zone_edge_families(family):
    k = bc.zone_edge_k(bc.FAMILY_CASE, (0, 1))
    T = pc.steps_bound(bc.FAMILY_CASE, 3, family)
    want = bc.oracle_parts(bc.FAMILY_CASE, family, T, bc.AMP, k)
    _variants(bc.FAMILY_CASE, family, T, want, amp=bc.AMP, k=k)


# ---------------------------------------------------------------- 3. the reference's answers
with open(os.path.join(ROOT, "tests", "golden", "bloch_known_results.json")) as _f:
    KNOWN = json.load(_f)


@pytest.mark.parametrize("g", KNOWN["cases"], ids=[g["name"] for g in KNOWN["cases"]])
def test_known_results(g):
    from scenarios import vol
    o = vol(bc.bloch_maker(), g["dim"], g["size"], KNOWN["a"])
    if g["pml_y"]:
        o.add_pml(g["pml_y"], dirs=(1,))
    f = o._fields()
    f.use_complex_fields()
    for d, k in enumerate(g["k"]):
        if k is not None:
            f.use_bloch(d, k)
    o.legacy_point_source(2, 0.2, 3.0, 0.0, 2.0, o.center(), complex(0, -2 * math.pi * 0.2))
    n = 0
    while float(np.float32(n * o.dt)) < KNOWN["ttot"]:
        n += 1
    assert n <= 601
    o.step(n)
    got = o.get_field(2, o.center())
    print(g["name"], got, g["value"], abs(got - g["value"]) / abs(g["value"]))
    assert abs(got - g["value"]) <= abs(g["value"]) * KNOWN["rel"], (got, g["value"])
    assert f.get_field_complex(2, o.center()).real == got


# ---------------------------------------------------------------- 4. a generic k
def _close(got, want, what):
    """Within 1e-9 of the array's largest magnitude; returns the largest ratio seen."""
    worst = 0.0
    for part in (0, 1):
        for c in pc.ALL_COMPS:
            scale = float(np.max(np.abs(want[part][c])))
            err = float(np.max(np.abs(got[part][c] - want[part][c])))
            assert scale > 0, (what, part, c)
            worst = max(worst, err / scale)
            assert err <= 1e-9 * scale, (what, part, c, err, scale)
    return worst


@pytest.mark.parametrize("case, family", [(c, "plain") for c in bc.GENERIC_CASES] +
                         [(bc.FAMILY_CASE, f) for f in bc.FAMILIES if f != "plain"])
def test_generic_k_against_the_oracle(case, family):
    T = pc.steps_bound(case, 3, family)
    want = bc.oracle_parts(case, family, T, bc.AMP, bc.GENERIC_K, planar=True)
    kw = dict(amp=bc.AMP, k=bc.GENERIC_K, planar=True)
    _, p = bc.run_bloch(case, family, T, **kw)
    assert _mode(p) == _fused_expected(case, family)
    got = _parts(p)
    print(case, family, "largest |diff| / max|array|:", _close(got, want, "T steps"))
    if _fused_expected(case, family):  # the same bits without the fused step
        _, q = bc.run_bloch(case, family, T, before=_nofuse, **kw)
        assert _mode(q) == 0
        g2 = _parts(q)
        for part in (0, 1):
            _same(g2[part], got[part], "set_fused(False), part %d" % part)
    _, q = bc.run_bloch(case, family, T, chunks=[1] * T, **kw)
    g2 = _parts(q)
    for part in (0, 1):
        _same(g2[part], got[part], "one step per call, part %d" % part)


# ---------------------------------------------------------------- 4b. a complex k on the device
def _shifted(c, d):
    """Component c (0..11: E, H, D, B) is shifted along direction d."""
    return (d == c % 3) if c // 3 in (0, 2) else (d != c % 3)


def test_complex_k_ghost_planes_are_the_table_times_the_owners():
    """A complex k has no lattice to compare with (the reference's conj(eikna) and eikna are
    not inverses when |eikna| != 1), so the kernel's product branch with |phase| != 1 is
    checked on the device directly: after a few steps every ghost point of every array of both
    parts is the NumPy table's phase times its owned point, bit for bit (two products and one
    sum per part, formed here as separate real operations)."""
    k = (0.1 + 0.02j, -0.05j, 0.3 - 0.01j)
    sc, p = bc.run_bloch(5, "plain", 4, amp=bc.AMP, k=k)
    tab = bc.phase_table_np([bc.eikna_np(k[d], sc.n[d], bc.A) for d in range(3)])
    assert any(abs(abs(t) - 1) > 1e-3 for t in tab)
    got = _parts(p)
    for c in pc.ALL_COMPS:
        re, im = got[0][c], got[1][c]
        idx, code = [], 0
        for d in range(3):
            j = np.arange(sc.n[d] + 1)
            ghost, owner = (sc.n[d], 0) if _shifted(c, d) else (0, sc.n[d])
            s = np.where(j == ghost, 2 if _shifted(c, d) else 1, 0)
            idx.append(np.where(j == ghost, owner, j))
            shp = [1, 1, 1]
            shp[d] = -1
            code = code + (3 ** d) * s.reshape(shp)
        src = np.ix_(*idx)
        pr = np.array([t.real for t in tab])[code]
        pi = np.array([t.imag for t in tab])[code]
        vr, vi = re[src], im[src]
        want_re = np.where(code == 0, re, pr * vr - pi * vi)
        want_im = np.where(code == 0, im, pr * vi + pi * vr)
        assert np.any(re[code != 0] != 0), c
        assert np.array_equal(re, want_re) and np.array_equal(im, want_im), c


# ---------------------------------------------------------------- 5. a property without the oracle
def _init_run(k, conj):
    """No sources: complex random D and B, all three axes periodic with k."""
    sc = pc.Scene(5, "plain", 1)
    o = sc.make(bc.bloch_maker())
    pc.materials(o, sc, sc.mask(), sc.mask(0.6, 0.85, seam=2))
    o.make_bloch(sc.per, k)
    for c in pc.D_COMPS + pc.B_COMPS:
        z = sc.cell_array(np.random.default_rng(3 + c), 0.1) + \
            1j * sc.cell_array(np.random.default_rng(40 + c), 0.1)
        o.initialize_field(c, np.conj(z) if conj else z)
    o.step(12)
    return _parts(o)


def test_conjugate_run():
    """(-k, conj of the initial fields) gives the conjugate fields, bit for bit: part 0 equal
    and part 1 negated on all arrays.  (With sources the property needs conj(A J(t)), which no
    amplitude gives while the source's current is complex, so the run is driven by
    initialize_field.)"""
    k = bc.GENERIC_K
    a = _init_run(k, False)
    b = _init_run(tuple(-x for x in k), True)
    for c in pc.ALL_COMPS:
        assert np.any(a[1][c] != 0), c
        assert np.array_equal(a[0][c], b[0][c]), c
        assert np.array_equal(a[1][c], -b[1][c]), c


# ---------------------------------------------------------------- 6. DFT on complex fields
DFT_FREQS = [0.6, 0.9, 1.1]
DFT_COMPS = [1, 3]  # Ey, Hx


def _dft_before(box, store):
    def before(o):
        for c in DFT_COMPS:
            o.require_component(c)
        store["h"] = o.add_dft_fields(DFT_COMPS, box[0], box[1], DFT_FREQS)
    return before


def _dft_arrays(o, h):
    return {(c, i): o.dft_array(h, c, i) for c in DFT_COMPS for i in range(len(DFT_FREQS))}


def _dft_bound(T, fmax):
    """|error| of a sum of N = T terms accumulated in another grouping: (N + 64) 2^-53 times
    the sum of the terms' magnitudes (the bound of tests/test_gpu_periodic.py), each term at
    most |scale| (|re| + |im| of the phase <= sqrt 2) times the largest field value of both
    parts, scale = dt / sqrt(2 pi)."""
    scale = (0.5 / bc.A) / math.sqrt(2 * math.pi)
    return (T + 64) * 2.0 ** -53 * T * scale * math.sqrt(2.0) * 2 * fmax


def test_dft_fields_complex_k0_is_the_sum_of_two_real_runs():
    """An interior dft_fields box of E and H at k = 0: DFT(real run with A) + i DFT(real run
    with -i A), within the accumulation bound (the complex accumulation adds phase * (f_re +
    i f_im) per update, the two real runs their own terms: another grouping of the same sum);
    updates buffered across one-step calls equal one call bit for bit."""
    T = pc.steps_bound(4, 3, "plain")
    box = ((0.5, 0.5, 1.5), (2.0, 1.5, 2.5))
    st = {}
    _, p = bc.run_bloch(4, "plain", T, amp=bc.AMP, planar=True, before=_dft_before(box, st))
    got = _dft_arrays(p, st["h"])
    parts, fmax = [], 0.0
    for part in (0, 1):
        sc = pc.Scene(4, "plain", 1)
        r = bc.configure(sc.make(pc.product_makers()[0]), sc, bc.AMP, part=part, planar=True)
        s2 = {}
        _dft_before(box, s2)(r)
        for _ in range(T):
            r.step(1)
            fmax = max([fmax] + [float(np.max(np.abs(r.get_array(c)))) for c in DFT_COMPS])
        parts.append(_dft_arrays(r, s2["h"]))
    bound = _dft_bound(T, fmax)
    for key in got:
        want = parts[0][key] + 1j * parts[1][key]
        assert got[key].shape == want.shape and np.any(want != 0), key
        err = float(np.max(np.abs(got[key] - want)))
        print(key, "dft |diff|", err, "bound", bound, "max", float(np.max(np.abs(want))))
        assert err <= bound, (key, err, bound)
    s3 = {}
    _, q = bc.run_bloch(4, "plain", T, amp=bc.AMP, planar=True, before=_dft_before(box, s3),
                        chunks=[1] * T)
    g2 = _dft_arrays(q, s3["h"])
    for key in got:
        assert np.array_equal(g2[key], got[key]), key


def test_dft_image_chunk_carries_the_bloch_phase():
    """A dft_fields region one period beyond the cell along x stands on image chunks alone
    (lattice shift 1): its values are eikna[x] times those of the same region inside the cell
    (dft_chunk folds the shift's phase into scale), within the accumulation bound; dft_points
    names the region's own coordinates."""
    T = pc.steps_bound(4, 3, "plain")
    k = bc.GENERIC_K
    Lx = pc.case_of(4)["n"][0] / bc.A
    lo, hi = (0.5, 0.5, 1.5), (2.0, 1.5, 2.5)
    st = {}

    def before(o):
        o.require_component(1)
        st["in"] = o.add_dft_fields([1], lo, hi, DFT_FREQS)
        st["out"] = o.add_dft_fields([1], (lo[0] + Lx,) + lo[1:], (hi[0] + Lx,) + hi[1:], DFT_FREQS)
    sc = pc.Scene(4, "plain", 1)
    p = bc.configure(sc.make(bc.bloch_maker()), sc, bc.AMP, k, planar=True)
    before(p)
    fmax = 0.0
    for _ in range(T):  # one step per call: the field's largest value over the run
        p.step(1)
        fmax = max([fmax] + [float(np.max(np.abs(p.get_array(1, part)))) for part in (0, 1)])
    a, b = p.dft_data(st["in"], 0), p.dft_data(st["out"], 0)
    assert a.shape == b.shape and np.any(a != 0)
    eik = bc.eikna_np(k[0], pc.case_of(4)["n"][0], bc.A)
    # (twice: both objects' sums are compared, and the phase is a rounded product itself)
    bound = 2 * _dft_bound(T, fmax)
    err = float(np.max(np.abs(b - eik * a)))
    print("image chunk |diff|", err, "bound", bound, "max", float(np.max(np.abs(a))))
    assert err <= bound and float(np.max(np.abs(b - a))) > 1e3 * bound
    f = p._fields()
    pin, pout = f.dft_points(st["in"], 0), f.dft_points(st["out"], 0)
    assert np.allclose(pout[:, 0] - pin[:, 0], Lx) and np.array_equal(pout[:, 1:], pin[:, 1:])


def test_flux_plane_reaching_the_periodic_faces():
    """A full-period flux plane at a generic k, whose ends lie on the periodic faces (image
    chunks with their phase), against the same plane moved by 5 cells along x, which sticks out
    of the cell: both are the flux through one period (E and conj(H) carry the same phase)."""
    T = pc.steps_bound(4, 3, "plain")
    c4 = pc.case_of(4)
    Lx, Ly = c4["n"][0] / bc.A, c4["n"][1] / bc.A
    st = {}

    def before(o):
        st["a"] = o.add_dft_flux([((0.0, 0.0, 2.5), (Lx, Ly, 2.5), 2, 1.0)], DFT_FREQS)
        st["b"] = o.add_dft_flux([((5 / bc.A, 0.0, 2.5), (Lx + 5 / bc.A, Ly, 2.5), 2, 1.0)],
                                 DFT_FREQS)
    _, p = bc.run_bloch(4, "plain", T, amp=bc.AMP, k=bc.GENERIC_K, planar=True, before=before)
    fa, fb = p.flux(st["a"]), p.flux(st["b"])
    print("flux", fa, fb)
    assert np.all(fa != 0) and np.allclose(fa, fb, rtol=1e-9, atol=0)


def _monitored(o, sc, st):
    """The full-period flux plane and an interior dft_fields box, added before stepping."""
    plane = [((0.0, 0.0, 22 / bc.A), (sc.L[0], sc.L[1], 22 / bc.A), 2, 1.0)]
    st["flux"] = o.add_dft_flux(plane, DFT_FREQS)
    st["box"] = o.add_dft_fields(DFT_COMPS, (0.5, 0.5, 1.5), (2.0, 1.5, 2.5), DFT_FREQS)


def test_flux_and_dft_against_the_phased_supercell():
    """A full-period flux plane (its ends on the periodic faces: image chunks) and an interior
    dft_fields box at a generic k against the oracle's two phased supercell runs of check 4.
    The oracle's lists of part 0 and part 1 have the same order (the same supercell), so
    E = E0 + i E1, H = H0 + i H1 and want = sum real(E conj(H)) over the central period.

    Tolerance.  The fields agree within tol = 1e-9 of their largest magnitude F (check 4), so a
    DFT value of N updates differs by at most dD = N |scale| sqrt(2) 2 tol F w (both parts;
    w <= 1 / a^2 the loop weight of the flux plane's E list, 1 elsewhere), plus the
    accumulation bound _dft_bound.  For the flux, with e_k = dD_E + bound and h_k likewise,
    |got - want| <= sum_k (e |H_k| + |E_k| h + e h) + (n + 64) 2^-53 sum_k |E_k conj H_k|."""
    T = pc.steps_bound(4, 3, "plain")
    k, nf = bc.GENERIC_K, len(DFT_FREQS)
    from scenarios import make_oracle
    lists, boxes, fmax = [], [], 0.0
    for part in (0, 1):
        s3 = pc.Scene(4, "plain", 3)
        o = bc.configure(s3.make(make_oracle), s3, bc.AMP, k, part=part, planar=True)
        st = {}
        _monitored(o, s3, st)
        for _ in range(T):
            o.step(1)
            fmax = max([fmax] + [float(np.max(np.abs(o.get_array(c)))) for c in range(6)])
        lists.append((o.dft_data(st["flux"], 0).reshape(-1, nf),
                      o.dft_data(st["flux"], 1).reshape(-1, nf)))
        boxes.append(_dft_arrays(o, st["box"]))
    E, H = lists[0][0] + 1j * lists[1][0], lists[0][1] + 1j * lists[1][1]
    terms = (E * np.conj(H)).real
    want, n = terms.sum(axis=0), terms.shape[0]
    s1 = pc.Scene(4, "plain", 1)
    p = bc.configure(s1.make(bc.bloch_maker()), s1, bc.AMP, k, planar=True)
    sp = {}
    _monitored(p, s1, sp)
    p.step(T)
    assert _mode(p) == 1
    scale = (0.5 / bc.A) / math.sqrt(2 * math.pi)
    dD = T * scale * math.sqrt(2.0) * 2 * 1e-9 * fmax
    acc = _dft_bound(T, fmax)
    # the interior box: no weights
    for key, got in _dft_arrays(p, sp["box"]).items():
        wantb = boxes[0][key] + 1j * boxes[1][key]
        err = float(np.max(np.abs(got - wantb)))
        print(key, "box |diff|", err, "bound", dD + acc, "max", float(np.max(np.abs(wantb))))
        assert got.shape == wantb.shape and np.any(wantb != 0) and err <= dD + acc, key
    # the flux
    e, h = dD / bc.A ** 2 + acc, dD + acc
    bound = (e * np.abs(H).sum(axis=0) + h * np.abs(E).sum(axis=0) + n * e * h +
             (n + 64) * 2.0 ** -53 * np.abs(terms).sum(axis=0))
    got = np.asarray(p.flux(sp["flux"]))
    print("flux", got, want, "|diff|", np.abs(got - want), "bound", bound)
    print("flux bound / |want|", bound / np.abs(want))
    assert np.all(want != 0)
    assert np.all(np.abs(got - want) <= bound)
    # the same flux unfused
    q = bc.configure(s1.make(bc.bloch_maker()), s1, bc.AMP, k, planar=True)
    sq = {}
    _monitored(q, s1, sq)
    _nofuse(q)
    q.step(T)
    assert _mode(q) == 0 and np.array_equal(np.asarray(q.flux(sq["flux"])), got)


# ---------------------------------------------------------------- 5b. period n against 2 n
def test_period_doubling_generic_k():
    """A period of 2 n holding the content twice, the second copy's sources times eikna, with
    the same k: the first copy's fields are the period-n run's, the second's eikna times them.
    Not bit for bit (eikna times a field is a rounded product unless eikna = +-1, and no k makes
    eikna of n and of 2 n both exact): within check 4's 1e-9 of each array's largest
    magnitude."""
    T, k = 40, bc.GENERIC_K
    sc, p = bc.run_bloch(4, "plain", T, amp=bc.AMP, k=k)
    _, q = bc.run_bloch(4, "plain", T, amp=bc.AMP, k=k, R=2)
    base, big = _parts(p), _parts(q)
    ex, ey = (bc.eikna_np(k[d], sc.n[d], bc.A) for d in (0, 1))
    worst = 0.0
    for c in pc.ALL_COMPS:
        z, Z = base[0][c] + 1j * base[1][c], big[0][c] + 1j * big[1][c]
        scale = float(np.max(np.abs(z)))
        assert scale > 0 and Z.shape[0] == 2 * sc.n[0] + 1 and Z.shape[1] == 2 * sc.n[1] + 1
        for jx in (0, 1):
            for jy in (0, 1):
                blk = Z[jx * sc.n[0]:jx * sc.n[0] + sc.n[0] + 1,
                        jy * sc.n[1]:jy * sc.n[1] + sc.n[1] + 1]
                err = float(np.max(np.abs(blk - z * ex ** jx * ey ** jy)))
                worst = max(worst, err / scale)
                assert err <= 1e-9 * scale, (c, jx, jy, err, scale)
    print("period doubling: largest |diff| / max|array|", worst)


# ---------------------------------------------------------------- 7. in-process slabs
@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("case", [4, "2d"])
@pytest.mark.parametrize("which", ["zone", "generic"])
def test_slabs_equal_one_rank(nranks, case, which):
    """Checks 2 and 4 on 2 and 3 in-process slabs (z slabs in 3-D, y slabs in 2-D; x / y wrap
    rank-local, both parts' planes in one exchange group): every array of both parts bit for
    bit the one-rank run's.  Several ranks step complex fields unfused."""
    k = bc.zone_edge_k(case, (0, 1) if case == 4 else (0,)) if which == "zone" else bc.GENERIC_K
    T = pc.steps_bound(case, 3, "lorentz")
    kw = dict(amp=bc.AMP, k=k, planar=which == "generic")
    _, one = bc.run_bloch(case, "lorentz", T, **kw)
    want = _parts(one)
    _, g = bc.run_bloch(case, "lorentz", T, maker=bc.bloch_group_makers()[nranks - 2], **kw)
    assert [int(f.fused_active()) for f in g._all()] == [0] * nranks
    assert all(not f.is_real for f in g._all())
    got = _parts(g)
    for part in (0, 1):
        assert all(np.any(want[part][c] != 0) for c in pc.ALL_COMPS)
        _same(got[part], want[part], "%d slabs, part %d" % (nranks, part))


def test_simulation_flux_on_complex_fields():
    import meep_nl_amd as mp
    sim = mp.Simulation(cell_size=mp.Vector3(1, 1, 0), resolution=10, complex_fields=True,
                        k_point=mp.Vector3(0.1, 0, 0),
                        boundary_layers=[mp.PML(0.2, direction=mp.Y)],
                        sources=[mp.Source(mp.GaussianSource(0.8, fwidth=0.6), mp.Ez,
                                           center=mp.Vector3(0, -0.1), size=mp.Vector3(1, 0))])
    fl = sim.add_flux(0.8, 0.4, 3, mp.FluxRegion(center=mp.Vector3(0, 0.2), size=mp.Vector3(1, 0)))
    sim.run(until=6)
    v = np.array(mp.get_fluxes(fl))
    assert v.shape == (3,) and np.all(v != 0)
    data = sim.get_flux_data(fl)
    assert np.iscomplexobj(data.E) and np.any(np.asarray(data.E).imag != 0)
    sim.load_minus_flux_data(fl, data)  # the negated fields: the same flux, the data negated
    back = sim.get_flux_data(fl)
    assert np.array_equal(np.asarray(back.E), -np.asarray(data.E))
    assert np.array_equal(np.asarray(back.H), -np.asarray(data.H))
    assert np.array_equal(np.array(mp.get_fluxes(fl)), v)


# ---------------------------------------------------------------- 8. errors
def _fields(case=4, family="plain", pml=True):
    from meep_nl_amd import core
    sc = pc.Scene(case, family, 1)
    o = sc.make(bc.bloch_maker())
    if pml and sc.pml:
        o.add_pml(pc.PML_CELLS / bc.A, dirs=tuple(sc.pml))
    return core, sc, o


def test_real_fields_still_refuse_k():
    _, sc, o = _fields()
    f = o._fields()
    assert f.is_real
    with pytest.raises(RuntimeError, match="meep:.*complex fields"):
        f.use_bloch(0, 0.1)
    with pytest.raises(RuntimeError, match="meep:.*real fields"):
        f.get_array(0, 1)
    assert f.get_field_complex(0, (0.5, 0.5, 0.5)) == 0


def test_calls_out_of_order():
    _, sc, o = _fields()
    f = o._fields()
    f.use_bloch(0)
    with pytest.raises(RuntimeError, match="meep:.*before use_bloch"):
        f.use_complex_fields()
    _, sc, o = _fields()
    f = o._fields()
    f.add_gaussian_source(1, 0.9, 0.7, -3.0, 3.0, (1.0, 1.0, 1.0), 1.0)
    with pytest.raises(RuntimeError, match="meep:.*before sources"):
        f.use_complex_fields()
    _, sc, o = _fields()
    f = o._fields()
    f.require_component(1)
    with pytest.raises(RuntimeError, match="meep:.*before initialize_field"):
        f.use_complex_fields()
    _, sc, o = _fields()
    f = o._fields()
    f.use_complex_fields()
    f.use_complex_fields()  # again: nothing to do
    f.add_gaussian_source(1, 0.9, 0.7, -3.0, 3.0, (1.0, 1.0, 1.0), 1.0)
    with pytest.raises(RuntimeError, match="meep:.*before sources"):
        f.use_bloch(0, 0.1)
    _, sc, o = _fields()
    f = o._fields()
    f.use_complex_fields()
    f.step(1)
    with pytest.raises(RuntimeError, match="meep:.*before the first step"):
        f.use_bloch(0, 0.1)
    with pytest.raises(RuntimeError, match="meep:.*PML along a periodic direction"):
        _fields()[2]._fields().use_bloch(2)  # (real or complex: the same rule)
    _, sc, o = _fields()
    f = o._fields()
    f.use_complex_fields()
    with pytest.raises(RuntimeError, match="meep:.*PML along a periodic direction"):
        f.use_bloch(2, 0.1)


@pytest.mark.parametrize("family, what", [("nr", "chi"), ("upstream", "chi"),
                                          ("aniso", "anisotropic")])
def test_declined_media(family, what):
    _, sc, o = _fields(family=family)
    pc.materials(o, sc, sc.mask(), sc.mask(0.6, 0.85, seam=2))
    with pytest.raises(RuntimeError, match="meep: use_complex_fields:.*" + what):
        o._fields().use_complex_fields()


def test_declined_cells_and_ranks():
    from meep_nl_amd import core
    s = core.Structure(core.GridVolume(1, [0, 0, 16], bc.A, [0, 0, 0]))
    with pytest.raises(RuntimeError, match="meep:.*1-D"):
        core.Fields(s).use_complex_fields()
    # several ranks take complex fields; the slab direction still cannot be periodic
    hub = core.LocalHub(2)
    s = core.Structure(core.GridVolume(3, [8, 8, 16], bc.A, [0, 0, 0]))
    for f in [core.Fields(s, rank=r, nranks=2, hub=hub) for r in range(2)]:
        f.use_complex_fields()
        with pytest.raises(RuntimeError, match="meep:.*slab direction"):
            f.use_bloch(2, 0.1)


def test_declined_objects(tmp_path):
    _, sc, o = _fields()
    f = o._fields()
    f.use_complex_fields()
    for d in sc.per:
        f.use_bloch(d, 0.1)
    f.add_gaussian_source(1, 0.9, 0.7, -3.0, 3.0, (1.0, 1.0, 2.0), 1.0)
    lo, hi = (0.5, 0.5, 2.0), (2.0, 2.0, 2.0)
    reg = [(lo, hi, 2, 1.0)]
    nope = "meep:.*not supported on complex fields"
    with pytest.raises(RuntimeError, match="meep: add_dft_near2far" + nope[5:]):
        f.add_dft_near2far(reg, [0.8])
    with pytest.raises(RuntimeError, match=nope):
        f.add_dft_energy(reg, [0.8])
    with pytest.raises(RuntimeError, match=nope):
        f.add_dft_force(reg, [0.8])
    with pytest.raises(RuntimeError, match=nope):
        f.add_probe(1, (1.0, 1.0, 2.0))
    with pytest.raises(RuntimeError, match=nope):
        f.dft_norm()
    with pytest.raises(RuntimeError, match=nope):
        f.tune(2)
    f.step(3)
    with pytest.raises(RuntimeError, match="meep: dump.*follow-up"):
        f.dump(str(tmp_path / "f.mnl"))
    with pytest.raises(RuntimeError, match="meep: load.*follow-up"):
        f.load(str(tmp_path / "f.mnl"))


def test_simulation_complex_fields():
    import meep_nl_amd as mp
    kw = dict(cell_size=mp.Vector3(1, 1, 0), resolution=10,
              sources=[mp.Source(mp.GaussianSource(0.2, fwidth=0.3), mp.Ez,
                                 center=mp.Vector3(0.05, 0.05), amplitude=1 + 0.5j)])
    sim = mp.Simulation(complex_fields=True, k_point=mp.Vector3(0.1, 0.3, 0), **kw)
    sim.run(until=5)
    z = sim.get_field_point(mp.Ez, mp.Vector3(0.2, 0.1))
    assert isinstance(z, complex) and z.real != 0 and z.imag != 0
    assert not sim.fields.is_real and sim.fields.boundary(0) == "periodic"
    arr = sim.get_array(mp.Ez, cmplx=True)
    assert arr.dtype == np.complex128 and np.any(arr.imag != 0)
    assert np.array_equal(sim.get_array(mp.Ez), arr.real)
    real = mp.Simulation(**kw)
    real.run(until=5)
    assert isinstance(real.get_field_point(mp.Ez, mp.Vector3(0.2, 0.1)), float)
