"""Mode coefficients of diffraction orders on the device:
core.Fields.mode_coefficients / mode_table and Simulation.get_eigenmode_coefficients with
DiffractedPlanewave modes.

The reference for the eight overlap sums of fields::get_overlap (src/dft.cpp:1377-1427) is a
NumPy restatement of dft_chunk::process_dft_component's integral (src/dft.cpp:977-1027) built
from dft_get (the E and H lists), dft_points (position, component, applied weight) and the
library's own mode_table (tested against closed forms in tests/test_mode_coeff_cpu.py).

u = 2^-53.  "The bound" is the project's accumulation bound (N + 64) u sum|term| for a sum of N
terms against a float64 sum in another order.  The coefficients follow
from the library's sums by src/mpb.cpp:984-999 -- two half-sums, one hypot, one sqrt, one
product -- within 8 u relative.  Resolutions are powers of two and the planes lie on
centred-grid planes, so every coordinate is exact."""
import numpy as np
import pytest

import dft_restate as R
from scenarios import GroupSim, GroupSim3, ProductSim, vol

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
EX, EY, EZ, HX, HY, HZ = range(6)
# (cE[0], cH[0]), (cE[1], cH[1]) per normal direction (src/dft.cpp:1380-1412)
SUMS = {0: ((EY, HZ), (EZ, HY)), 1: ((EZ, HX), (EX, HZ)), 2: ((EX, HY), (EY, HX))}


# ------------------------------------------------------------------ the restatement
def fields_of(o):
    return o._all() if hasattr(o, "_all") else [o._fields()]


def restate(o, h, nd, modes, a, weight=1.0, eig_vol=None, kpoint=None):
    """sums[nm, nf, 8], sum|term|[nm, nf, 8], N[8], the table: the four mode-flux sums
    w conj(mode[c_conjugate](x)) dft_val, dft_val = dft / stored_weight (/ w where the chunk
    stored the weight), and the four mode-mode sums w conj(mode[c_conjugate](x)) mode[c](x)."""
    fs = fields_of(o)
    f = fs[0]
    tab = f.mode_table(h, modes, eig_vol, kpoint)
    nf = f._dft_nf[h]
    lists = [sum(x.dft_get(h, w) for x in fs) for w in (0, 1)]
    pts = [f.dft_points(h, 0), f.dft_points(h, 1)]
    half = [np.rint(p[:, :3] * 2 * a).astype(int) for p in pts]
    for p, hh in zip(pts, half):
        assert np.array_equal(hh * (0.5 / a), p[:, :3])  # exact coordinates
    loopw = {}  # the loop weight of a position: what the E list (which stores it) applied
    for hh, w in zip(half[0], pts[0][:, 4]):
        assert loopw.setdefault(tuple(hh), w) == w
    (e0, h0), (e1, h1) = SUMS[nd]
    spec = [(e0, h0, weight, 0), (e1, h1, -weight, 0), (h0, e0, 1.0, 1), (h1, e1, 1.0, 1)]
    da, db = tab["dirs"]
    nm = len(modes)
    sums = np.zeros((nm, nf, 8), dtype=complex)
    sabs = np.zeros((nm, nf, 8))
    N = np.zeros(8, dtype=int)
    for j, (c, cc, sw, which) in enumerate(spec):
        sel = pts[which][:, 3] == c
        N[j] = N[4 + j] = sel.sum()
        if not N[j]:
            continue
        hh = half[which][sel]
        w = np.array([loopw[tuple(x)] for x in hh])
        ia = np.searchsorted(tab["coords_a"], hh[:, da])
        assert np.array_equal(tab["coords_a"][ia], hh[:, da])
        ph = tab["pa"][:, ia]
        if db is not None:
            ib = np.searchsorted(tab["coords_b"], hh[:, db])
            assert np.array_equal(tab["coords_b"][ib], hh[:, db])
            ph = ph * tab["pb"][:, ib]
        layer = np.searchsorted(tab["layers"], hh[:, nd])
        assert np.array_equal(tab["layers"][layer], hh[:, nd])
        phase = ph[:, None, :] * tab["pl"][:, :, layer]          # [mode, freq, point]
        mc = tab["amp"][:, :, cc, None] * phase
        mo = tab["amp"][:, :, c, None] * phase
        d = lists[which].reshape(-1, nf)[sel].T[None] / sw
        if which == 0:  # include_dV_and_interp_weights
            d = np.where(d != 0, d / w, d)
        wc = w * np.conj(mc)
        t, u = wc * d, wc * mo
        sums[:, :, j], sabs[:, :, j] = t.sum(-1), np.abs(t).sum(-1)
        sums[:, :, 4 + j], sabs[:, :, 4 + j] = u.sum(-1), np.abs(u).sum(-1)
    return sums, sabs, N, tab


def check_sums(got, want, sabs, N, label):
    """the bound, per sum; a sum without terms (or of zeros) is exactly 0"""
    bound = (N + 64) * U * sabs
    err = np.abs(got - want)
    ratio = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))
    print(f"{label}: N = {N[:4]}, max |sum| = {np.max(np.abs(want)):.3e}, "
          f"max err / bound = {ratio:.3e}")
    assert np.all(np.isfinite(got.view(float)))
    assert np.all(err <= bound), (label, np.max(err - bound))
    assert np.any(want[..., :4] != 0) and np.any(want[..., 4:] != 0), label


def coefficients(ov, vgrp, evan):
    """src/mpb.cpp:957-999 applied to the eight sums"""
    o0, o1 = ov[..., 0] - ov[..., 1], ov[..., 2] - ov[..., 3]
    m0, m1 = ov[..., 4] - ov[..., 5], ov[..., 6] - ov[..., 7]
    cplus, cminus = 0.5 * (o0 + o1), 0.5 * (o0 - o1)
    normfac = 0.5 * (m0 + m1)
    normfac = np.where(normfac == 0, 1.0, normfac)
    csc = np.sqrt(1.0 / np.abs(normfac))
    alpha = np.zeros(ov.shape[:2] + (2,), dtype=complex)
    fwd = vgrp > 0
    alpha[..., 0] = np.where(fwd, cplus, cminus) * csc
    alpha[..., 1] = np.where(fwd, cminus, cplus) * csc
    alpha[evan] = 0
    return alpha, np.where(evan, 0.0, csc)


def check_coefficients(r, tab, label):
    evan = ~np.any(tab["k"] != 0, axis=-1)
    alpha, csc = coefficients(r["overlaps"], tab["vgrp"], evan)
    assert np.array_equal(r["vgrp"], np.where(evan, 0.0, tab["vgrp"]))
    assert np.array_equal(r["kpoints"], tab["k"])
    assert np.all(r["alpha"][evan] == 0) and np.all(r["cscale"][evan] == 0)
    assert np.all(r["kpoints"][evan] == 0) and np.all(r["vgrp"][evan] == 0)
    err = np.abs(r["alpha"] - alpha)
    print(f"{label}: max |alpha| = {np.max(np.abs(alpha)):.3e}, "
          f"max err / (u |alpha|) = {np.max(err / np.maximum(np.abs(alpha), 1e-300)) / U:.2f}")
    assert np.all(err <= 8 * U * np.abs(alpha)), label
    assert np.all(np.abs(r["cscale"] - csc) <= 8 * U * csc), label
    return evan


def check_all(o, h, nd, modes, a, label, **kw):
    sums, sabs, N, tab = restate(o, h, nd, modes, a, **kw)
    ev, kp = kw.get("eig_vol"), kw.get("kpoint")
    rs = collective(o, lambda f: f.mode_coefficients(h, modes, ev, kp))
    check_sums(rs["overlaps"], sums, sabs, N, label)
    evan = check_coefficients(rs, tab, label)
    return rs, tab, evan, (sums, sabs, N)


def collective(o, fn):
    """fn(fields) on every rank at once; every rank returns the same bits"""
    if not hasattr(o, "_all"):
        return fn(o._fields())
    o._all()
    vals = o._par(fn)
    for v in vals[1:]:
        for k in v:
            assert np.array_equal(v[k], vals[0][k]), k
    return vals[0]


# ------------------------------------------------------------------ the 3-D grating period
A3 = 8.0
N3 = (40, 36, 24)                      # cells: 5 x 4.5 x 3
LO3, HI3 = (-2.5, -2.25, -1.5), (2.5, 2.25, 1.5)
ZMON = 0.5625                           # a centred-grid plane (9 half-pixels)
# (+-1, 0): k = 0.2, evanescent at 0.15 and propagating from 0.21 on; (0, 1): 0.2222; (1, 1): 0.299
FREQS3 = [0.15, 0.21, 0.25, 0.32, 0.4]
MODES3 = [((0, 0, 0), None, 1, 0), ((0, 0, 0), None, 0, 1), ((1, 0, 0), None, 1, 0),
          ((-1, 0, 0), None, 0, 1), ((0, 1, 0), None, 0.6, 0.8), ((1, 1, 0), (0, 1, 0), 0.8, -0.6),
          ((1, 0, 0), (0.3, 1.0, 0.5), 0.5 - 0.25j, 0.125 + 0.75j)]
STEPS3 = 200


def grating(make, scatterer=True, n=N3):
    sizes = [v / A3 for v in n]
    o = vol(make, 3, sizes, A3, center_origin=True)
    o.add_pml(0.5, dirs=(2,))
    if scatterer:
        for c in (EX, EY, EZ):
            x, y, z = o.coords(c)
            inside = (x > 0.1) & (x < 1.3) & (y > -0.9) & (y < 0.4) & (np.abs(z) < 0.3)
            o.set_chi1inv(c, c, np.where(inside, 0.25, 1.0))
    for f in fields_of(o):
        f.use_bloch(0)
        f.use_bloch(1)
    lo, hi = [-0.5 * s for s in sizes], [0.5 * s for s in sizes]
    o.add_gaussian_volume_source(EX, 0.3, 1.0, 0.0, 8.0, [lo[0], lo[1], -0.75],
                                 [hi[0], hi[1], -0.75], 1.0)
    return o, lo, hi


def add_plane(o, lo, hi, z, freqs, weight=1.0):
    reg = [([lo[0], lo[1], z], [hi[0], hi[1], z], 2, weight)]
    hs = [f.add_dft_flux(reg, freqs, 1) for f in fields_of(o)]
    assert all(x == hs[0] for x in hs)
    return hs[0]


@pytest.fixture(scope="module")
def grating_run():
    """the one-rank run tests 1, 2, 3 and 7 share: planes on the grid (one layer) and a quarter
    cell off it (two layers)"""
    o, lo, hi = grating(ProductSim)
    h1 = add_plane(o, lo, hi, ZMON, FREQS3)
    h2 = add_plane(o, lo, hi, ZMON + 0.25 / A3, FREQS3, weight=-0.5)
    o.step(STEPS3)
    return o, h1, h2


def test_restatement_and_coefficients(grating_run):
    """Test 1.  4 x 1440 slots and the seam's image chunks; every sum spans three workgroups."""
    o, h, _ = grating_run
    f = o._fields()
    npts = len(f.dft_points(h, 0)) + len(f.dft_points(h, 1))
    assert npts > 4 * 1440 and npts % 64 != 0
    assert 1440 > 2 * 512  # MO_WG_SLOTS: at least three slot ranges per sum
    rs, tab, evan, _ = check_all(o, h, 2, MODES3, A3, "grating")
    assert tab["layers"].size == 1
    assert evan[2, 0] and evan[3, 0] and not evan[2, -1] and not evan[3, -1]
    assert not evan[0].any() and evan.sum() >= 4
    assert np.all(np.abs(rs["alpha"][~evan]).max(axis=-1) > 0)
    # the same bits in a second call (the reduction order is fixed)
    again = f.mode_coefficients(h, MODES3)
    for k in rs:
        assert np.array_equal(rs[k], again[k]), k


def test_two_layers(grating_run):
    """Test 2.  A quarter cell off the centred grid: two layers, weight -0.5."""
    o, _, h = grating_run
    sums, sabs, N, tab = restate(o, h, 2, MODES3, A3, weight=-0.5)
    assert list(tab["layers"]) == [9, 11]
    r = o._fields().mode_coefficients(h, MODES3)
    check_sums(r["overlaps"], sums, sabs, N, "two layers")
    assert np.any(tab["pl"][:, :, 0] != tab["pl"][:, :, 1])


def fourier_sums(f, h, kins, cen):
    """F_c[order, freq] = sum_p w dft_val_c exp(-2 pi i k.(x - cen)) of Ex, Ey, Hx, Hy on a z plane
    for the in-plane wavevectors kins[order, 2], the bound of each sum per frequency (the phase
    has modulus 1, so it is the same for every order) and the plane's weight sum W."""
    nf = f._dft_nf[h]
    kins = np.atleast_2d(np.asarray(kins, dtype=float))
    pE, pH = f.dft_points(h, 0), f.dft_points(h, 1)
    assert np.array_equal(pE[:, :3], pH[:, :3])
    w = pE[:, 4]
    out, tol = {}, {}
    for which, pts, sw in ((0, pE, {EX: 1.0, EY: -1.0}), (1, pH, {HX: 1.0, HY: 1.0})):
        vals = f.dft_get(h, which).reshape(-1, nf)
        for c, s in sw.items():
            sel = pts[:, 3] == c
            d = vals[sel] / s
            if which == 0:
                d = np.where(d != 0, d / w[sel, None], d)
            e = np.exp(-2j * np.pi * (np.outer(kins[:, 0], pts[sel, 0] - cen[0])
                                      + np.outer(kins[:, 1], pts[sel, 1] - cen[1])))
            wd = w[sel, None] * d
            out[c], tol[c] = e @ wd, (sel.sum() + 64) * U * np.abs(wd).sum(0)
    return out, tol, w[pE[:, 3] == EX].sum()


def order_flux(F, W):
    return (F[EX] * np.conj(F[HY]) - F[EY] * np.conj(F[HX])).real / W


def order_flux_tol(F, T, W):
    """the bounds T of the four Fourier sums through the quadratic form of order_flux"""
    return (np.abs(F[HY]) * T[EX] + np.abs(F[EX]) * T[HY] + np.abs(F[HX]) * T[EY]
            + np.abs(F[EY]) * T[HX]) / W


def test_per_order_power(grating_run):
    """Test 3.  The identity: on a one-layer full-period plane the discrete plane waves are
    orthogonal under the loop weights (a seam point and its image chunk's copy one period away
    carry the two halves of one weight) and s+, s-, p+, p- of one order span its tangential
    (Ex, Ey, Hx, Hy) space, so |a+s|^2 + |a+p|^2 - |a-s|^2 - |a-p|^2 is the order's flux
    Re(F_Ex conj(F_Hy) - F_Ey conj(F_Hx)) / W of the weighted Fourier sums F at the order's
    in-plane k.  Tolerance: the device's overlap sums are those Fourier sums times the mode's
    amplitudes in another order, so the difference is within the bound of each F through the
    quadratic form (order_flux_tol), plus 64 u sum |alpha|^2 for the roundings between the sums
    and |alpha|^2 (8 u relative per alpha, squared and added).

    All orders: the 40 x 36 grid points of the period carry 1440 discrete orders, and by exact
    Parseval dft_flux is the sum of order_flux over all of them.  So dft_flux minus the power of
    the propagating orders among |g| <= 1, taken from the coefficients, equals the sum of
    NumPy's order_flux over every other discrete order, within the sum of the tolerances above
    for the former, order_flux_tol for each of the latter, and the bound of the flux sum itself.
    Nothing physical is assumed (the orders (+-2, 0) at f = 0.4, where k2 == 0, are among the
    latter)."""
    o, h, _ = grating_run
    f = o._fields()
    nf = len(FREQS3)
    near = [(gx, gy, 0) for gx in (0, 1, -1) for gy in (0, 1, -1)]
    modes = [(g, None, s, p) for g in near for s, p in ((1, 0), (0, 1))]
    r = f.mode_coefficients(h, modes)
    tab = f.mode_table(h, modes)
    a2 = np.abs(r["alpha"]) ** 2
    # every discrete order of the grid, the nine near ones first
    every = near + [(gx, gy, 0) for gx in range(-20, 20) for gy in range(-18, 18)
                    if max(abs(gx), abs(gy)) > 1]
    assert len(every) == 40 * 36
    kins = np.array([[g[0] / 5.0, g[1] / 4.5] for g in every])
    F, T, W = fourier_sums(f, h, kins, (0.0, 0.0))
    want, tol = order_flux(F, W), order_flux_tol(F, T, W)   # [order, freq]
    prop = np.zeros((len(every), nf), dtype=bool)
    from_alpha, from_alpha_tol = np.zeros(nf), np.zeros(nf)
    seen = 0
    for i, g in enumerate(near):
        # (the in-plane k does not depend on the frequency)
        assert np.array_equal(tab["k"][2 * i, -1, :2], kins[i])
        for i_f in range(nf):
            if not np.any(tab["k"][2 * i, i_f] != 0):
                continue  # evanescent
            got = (a2[2 * i, i_f, 0] + a2[2 * i + 1, i_f, 0] - a2[2 * i, i_f, 1]
                   - a2[2 * i + 1, i_f, 1])
            t = tol[i, i_f] + 64 * U * a2[2 * i:2 * i + 2, i_f].sum()
            print(f"order {g} f {FREQS3[i_f]}: flux {want[i, i_f]:.6e}, diff / tol = "
                  f"{abs(got - want[i, i_f]) / t:.3e}")
            assert abs(got - want[i, i_f]) <= t, (g, i_f)
            prop[i, i_f] = True
            from_alpha[i_f] += got
            from_alpha_tol[i_f] += t
            seen += 1
    assert seen == 5 + 2 * 4 + 2 * 3 + 4 * 2  # the propagating (order, frequency) pairs
    flux = f.flux(h)
    e, hh = f.dft_get(h, 0), f.dft_get(h, 1)
    flux_tol = (e.size // nf + 64) * U * np.abs(e * np.conj(hh)).reshape(-1, nf).sum(0)
    rest = np.where(prop, 0.0, want).sum(0)
    rest_tol = np.where(prop, 0.0, tol).sum(0)
    total_tol = flux_tol + from_alpha_tol + rest_tol
    diff = np.abs((flux - from_alpha) - rest)
    print("all orders: flux", flux, "from coefficients", from_alpha, "other orders", rest,
          "diff / tol", diff / total_tol)
    assert np.all(diff <= total_tol)
    assert np.all(np.abs(rest) > 0) and np.all(from_alpha > 0)


# ------------------------------------------------------------------ 5. normal incidence
def test_normal_incidence_in_vacuum():
    """Test 5.  No scatterer: the field is uniform over the plane and the (0, 0) mode space is
    the whole uniform field space, so |a+|^2 - |a-|^2 of the (0, 0) mode with the source's
    polarisation (p for the default axis x and E along x) is dft_flux: with the overlaps o0, o1
    and normfac it is Re(o0 conj(o1)) / |normfac|.  Tolerance: 64 u relative plus the bound of
    every sum through that form, d = (|o1| d_o0 + |o0| d_o1) / |normfac| + |P| d_nf / |normfac|,
    plus the bound of the flux sum itself.  Every other coefficient is at most the bound of
    its sums through alpha = csc (o0 +- o1) / 2."""
    o, lo, hi = grating(ProductSim, scatterer=False, n=(16, 12, 24))
    freqs = [0.25, 0.3, 0.6]
    h = add_plane(o, lo, hi, ZMON, freqs)
    o.step(STEPS3)
    modes = [((0, 0, 0), None, 0, 1), ((0, 0, 0), None, 1, 0), ((1, 0, 0), None, 1, 0),
             ((1, 0, 0), None, 0, 1), ((0, 1, 0), None, 0, 1), ((-1, -1, 0), None, 1, 1),
             ((-1, 0, 0), None, 1, 1)]
    rs, tab, evan, (sums, sabs, N) = check_all(o, h, 2, modes, A3, "vacuum")
    # (+-1, 0): k = 0.5, propagating at 0.6; (0, 1) and (-1, -1) are evanescent throughout
    assert not evan[0].any() and not evan[2, 2] and not evan[6, 2] and evan[5].all()
    f = o._fields()
    flux = f.flux(h)
    bound = (N + 64) * U * sabs                           # [mode, freq, 8]
    ov = rs["overlaps"]
    o0, o1 = ov[..., 0] - ov[..., 1], ov[..., 2] - ov[..., 3]
    nfac = np.abs(0.5 * (ov[..., 4] - ov[..., 5] + ov[..., 6] - ov[..., 7]))
    d0, d1 = bound[..., 0] + bound[..., 1], bound[..., 2] + bound[..., 3]
    dn = 0.5 * bound[..., 4:].sum(-1)
    a2 = np.abs(rs["alpha"]) ** 2
    P = a2[0, :, 0] - a2[0, :, 1]
    pE, pH = f.dft_points(h, 0), f.dft_points(h, 1)
    e, hh = f.dft_get(h, 0).reshape(len(pE), -1), f.dft_get(h, 1).reshape(len(pH), -1)
    dflux = (len(pE) + 64) * U * np.abs(e * np.conj(hh)).sum(0)
    tol = (64 * U * np.abs(flux) + (np.abs(o1[0]) * d0[0] + np.abs(o0[0]) * d1[0]) / nfac[0]
           + np.abs(P) * dn[0] / nfac[0] + dflux)
    print("flux", flux, "P", P, "diff / tol", np.abs(P - flux) / tol)
    assert np.all(flux > 0) and np.all(np.abs(P - flux) <= tol)
    small = 0.5 * rs["cscale"] * (d0 + d1)
    for m in range(1, len(modes)):
        assert np.all(np.abs(rs["alpha"][m]) <= small[m][:, None]), m


# ------------------------------------------------------------------ 4. oblique, complex fields
A2 = 16.0
KX = 0.1


def oblique():
    o = vol(ProductSim, 2, [2.0, 3.0], A2, center_origin=True)
    o.add_pml(0.5, dirs=(1,))
    x, y = o.coords(EZ)
    o.set_chi1inv(EZ, EZ, np.where((np.abs(y + 0.1) < 0.2) & (x > -0.7) & (x < 0.2), 0.25, 1.0))
    f = o._fields()
    f.use_complex_fields()
    f.use_bloch(0, KX)
    f.add_gaussian_volume_source(EZ, 1.0, 1.0, 0.0, 8.0, [-1.0, -0.75], [1.0, -0.75], 1.0,
                                 amp_func=lambda r: np.exp(2j * np.pi * KX * r[0]))
    return o, f


def test_oblique_incidence_on_complex_fields():
    """Test 4.  2-D, 32 x 48 cells, periodic in x with Bloch k = 0.1, complex fields, a phased
    line source and a dielectric strip; orders 0 and +-1 on the transmitted line.  The Bloch k
    enters the in-plane k only where the eigenmode volume spans the periodic direction: a
    monitor shorter than the period takes kpoint (0)."""
    o, f = oblique()
    freqs = [0.5, 1.05, 1.3]  # order +1 (k_x = 0.6) is evanescent at the first
    ymon = 17 / 32.0
    full = f.add_dft_flux([([-1.0, ymon, 0.0], [1.0, ymon, 0.0], 1, 1.0)], freqs, 1)
    short = f.add_dft_flux([([-0.5, ymon, 0.0], [0.5, ymon, 0.0], 1, 1.0)], freqs, 1)
    o.step(400)
    # s and p of the orders 0, +1, -1 (modes 2 i, 2 i + 1), and one mixed mode
    modes = [((0, 0, 0), None, 1, 0), ((0, 0, 0), None, 0, 1), ((1, 0, 0), None, 1, 0),
             ((1, 0, 0), None, 0, 1), ((-1, 0, 0), None, 1, 0), ((-1, 0, 0), None, 0, 1),
             ((-1, 0, 0), None, 0.6, 0.8j)]
    rs, tab, evan, _ = check_all(o, full, 1, modes, A2, "oblique full period")
    assert tab["dirs"] == (0, None) and tab["layers"].size == 1
    assert tab["coords_a"][0] < -32 or tab["coords_a"][-1] > 32  # the seam's image chunk
    for m, (g, *_rest) in enumerate(modes):
        assert tab["k"][m, -1, 0] == KX + g[0] / 2.0
    assert evan[2, 0] and not evan[2, -1] and not evan[0].any()
    assert np.min(np.abs(rs["alpha"][0, :, 0])) > 0  # Ez is the s polarisation
    rs2, tab2, evan2, _ = check_all(o, short, 1, modes, A2, "oblique short monitor")
    for m, (g, *_rest) in enumerate(modes):
        if not evan2[m, -1]:
            assert tab2["k"][m, -1, 0] == g[0] / 1.0
    # the caller's kpoint is used there instead
    tab3 = f.mode_table(short, modes, None, (0.25, 0, 0))
    assert tab3["k"][0, -1, 0] == 0.25 and f.mode_table(full, modes, None, (0.25, 0, 0))["k"][0, -1, 0] == KX
    # per-order power on the full-period line: test 3's identity for the orders 0 and +-1 at
    # their propagating frequencies, with its tolerance.  The normal is y and only Ez and Hx
    # exist: the order's flux is Re(F_Ez conj(F_Hx)) / W at k_x = KX + g / 2; a point of the
    # seam's image chunk carries the field's Bloch phase, which the mode's phase one period on
    # cancels, so the orders stay orthogonal under the loop weights.
    a2 = np.abs(rs["alpha"]) ** 2
    pE, pH = f.dft_points(full, 0), f.dft_points(full, 1)
    assert np.array_equal(pE[:, :3], pH[:, :3]) and set(pE[:, 3]) == {EZ} and set(pH[:, 3]) == {HX}
    w = pE[:, 4]
    e = f.dft_get(full, 0).reshape(len(pE), -1)
    e = np.where(e != 0, e / w[:, None], e)
    hx = f.dft_get(full, 1).reshape(len(pH), -1)
    Te = (len(w) + 64) * U * np.abs(w[:, None] * e).sum(0)
    Th = (len(w) + 64) * U * np.abs(w[:, None] * hx).sum(0)
    W = w.sum()
    seen = 0
    for i, g in enumerate((0, 1, -1)):
        assert modes[2 * i][0][0] == g and modes[2 * i + 1][0][0] == g
        ph = np.exp(-2j * np.pi * (KX + g / 2.0) * pE[:, 0])[:, None]   # the centre is x = 0
        Fe, Fh = (w[:, None] * ph * e).sum(0), (w[:, None] * ph * hx).sum(0)
        want = (Fe * np.conj(Fh)).real / W                     # normal y: Ez Hx* - Ex Hz*
        tol = (np.abs(Fh) * Te + np.abs(Fe) * Th) / W + 64 * U * a2[2 * i:2 * i + 2].sum((0, 2))
        got = (a2[2 * i, :, 0] + a2[2 * i + 1, :, 0] - a2[2 * i, :, 1] - a2[2 * i + 1, :, 1])
        ok = ~evan[2 * i]
        print(f"order {g} power", want, "propagating", ok, "diff / tol", np.abs(got - want) / tol)
        assert np.all(np.abs(got - want)[ok] <= tol[ok]) and np.all(want[ok] != 0)
        seen += ok.sum()
    assert seen == 3 + 2 + 3


# ------------------------------------------------------------------ 6. same bits in every mode
PAIR_FREQS = R.FREQS
PAIR_REG = [([-1.0, -0.8, 0.55], [1.0, 0.8, 0.55], 2, 1.0)]
PAIR_VOL = ([-2.0, -0.8, 0.55], [2.0, 0.8, 0.55])
PAIR_MODES = [((1, 0, 0), None, 1, 0), ((-1, 0, 0), None, 0, 1), ((0, 0, 0), (0, 1, 0), 0.6, 0.8j)]


def pair_variant(tb=None, calls=(40, 40), read=False):
    o = R.build_cell(ProductSim, "uniform", tb)
    f = o._fields()
    h = f.add_dft_flux(PAIR_REG, PAIR_FREQS, 1)
    for k, n in enumerate(calls):
        o.step(n)
        if read and k % 16 == 7:
            mid = f.mode_coefficients(h, PAIR_MODES, PAIR_VOL)
            assert np.all(np.isfinite(mid["alpha"].view(float)))
    return f, h, f.mode_coefficients(h, PAIR_MODES, PAIR_VOL)


@pytest.fixture(scope="module")
def pair_base():
    f, h, r = pair_variant(tb=True)
    assert f.fused_active() and f.tb_info()["active"]
    assert np.all(r["vgrp"] > 0) and np.all(np.abs(r["alpha"]) > 0)
    return r


def same_bits(r, base):
    for k in base:
        assert np.array_equal(r[k], base[k]), k


def test_mode_fused_without_pairs(pair_base):
    f, _, r = pair_variant(tb=False)
    assert f.fused_active() and not f.tb_info()["active"]
    same_bits(r, pair_base)


def test_mode_unfused(pair_base, monkeypatch):
    monkeypatch.setenv("MNL_NO_FUSED", "1")
    f, _, r = pair_variant()
    assert not f.fused_active()
    same_bits(r, pair_base)


def test_mode_single_steps_with_reads(pair_base):
    _, _, r = pair_variant(calls=(1,) * 80, read=True)
    same_bits(r, pair_base)


@pytest.mark.parametrize("kb", ["1", "3"])
def test_mode_dft_block(pair_base, monkeypatch, kb):
    monkeypatch.setenv("MNL_DFT_BLOCK", kb)
    _, _, r = pair_variant(tb=True)
    same_bits(r, pair_base)


# ------------------------------------------------------------------ 7. ranks
@pytest.mark.parametrize("group", [GroupSim, GroupSim3])
def test_slabs_match_one_rank(grating_run, group):
    """The partial sums are all-reduced: equal to one rank's within the bound, not bitwise."""
    o1, h1, _ = grating_run
    _, sabs, N, _ = restate(o1, h1, 2, MODES3, A3)
    one = o1._fields().mode_coefficients(h1, MODES3)
    o, lo, hi = grating(group)
    h = add_plane(o, lo, hi, ZMON, FREQS3)
    o.step(STEPS3)
    rs, tab, evan, _ = check_all(o, h, 2, MODES3, A3, f"{group.NRANKS} slabs")
    bound = (N + 64) * U * sabs
    assert np.all(np.abs(rs["overlaps"] - one["overlaps"]) <= bound)
    assert np.array_equal(rs["vgrp"], one["vgrp"])


# ------------------------------------------------------------------ 8. through Simulation
def test_through_simulation():
    import meep_nl_amd as mp
    cell = mp.Vector3(2, 1.5, 3)

    def make(block):
        geo = [mp.Block(center=mp.Vector3(0.25, 0, 0), size=mp.Vector3(0.5, 0.5, 0.5),
                        material=mp.Medium(epsilon=4))] if block else []
        s = mp.Simulation(cell_size=cell, resolution=8, k_point=mp.Vector3(),
                          boundary_layers=[mp.PML(0.5, direction=mp.Z)], eps_averaging=False,
                          geometry=geo,
                          sources=[mp.Source(mp.GaussianSource(0.8, fwidth=0.8), mp.Ex,
                                             center=mp.Vector3(0, 0, -0.75),
                                             size=mp.Vector3(cell.x, cell.y, 0))])
        m = s.add_mode_monitor(0.8, 0.4, 3, mp.FluxRegion(center=mp.Vector3(0, 0, ZMON),
                                                          size=mp.Vector3(cell.x, cell.y, 0)))
        return s, m

    sim, mon = make(True)
    assert isinstance(mon, mp.DftFlux)
    sim.run(until=12)
    one = mp.DiffractedPlanewave((0, 0, 0), None, 0, 1)
    r1 = sim.get_eigenmode_coefficients(mon, one)
    assert r1.alpha.shape == (1, 3, 2) and r1.vgrp.shape == (3,) and len(r1.kdom) == 3
    for i, fr in enumerate(mon.freq):
        assert r1.kdom[i] == mp.Vector3(0, 0, fr) and r1.kpoints[i] == r1.kdom[i]
    assert np.all(r1.vgrp == 1.0) and np.all(np.abs(r1.alpha[0, :, 0]) > 0)
    lst = [one, mp.DiffractedPlanewave((1, 0, 0), mp.Vector3(0, 1, 0), 1, 0),
           mp.DiffractedPlanewave((0, -1, 0), None, 0.5, 0.5j)]
    r3 = sim.get_eigenmode_coefficients(mon, lst, eig_parity=3)
    assert r3.alpha.shape == (3, 3, 2) and r3.vgrp.shape == (9,) and len(r3.kpoints) == 9
    assert np.array_equal(r3.alpha[0], r1.alpha[0])  # a mode's sums do not depend on the others
    k10 = r3.kdom[3 + 2]
    assert k10.x == 0.5 and k10.y == 0 and k10.z == np.sqrt(mon.freq[2] ** 2 - 0.25)
    # kpoint_func (the flux region spans the periodic cell, so only k2 == 0 would read it)
    rk = sim.get_eigenmode_coefficients(mon, lst, kpoint_func=lambda f, b: mp.Vector3(0, 0, f))
    assert np.array_equal(rk.alpha, r3.alpha)
    # the normalisation workflow with two runs: the incident run's data (no block), loaded
    # negated into the scattering run before it steps.  The coefficients are those of the
    # restatement on the object's data (the scattered field: accumulated - incident), and
    # not those of the run without the load.
    ref, mref = make(False)
    ref.run(until=12)
    incident = ref.get_flux_data(mref)
    sca, msca = make(True)
    sca.load_minus_flux_data(msca, incident)
    sca.run(until=12)

    class Wrap:
        def _fields(self):
            return sca.fields
    tuples = [(b.g, b.axis, b.s, b.p) for b in lst]
    rsc, _, _, _ = check_all(Wrap(), msca.handle, 2, tuples, 8.0, "scattered field")
    got = sca.get_eigenmode_coefficients(msca, lst)
    assert np.array_equal(got.alpha, rsc["alpha"])
    assert np.all(got.alpha[0, :, 0] != r3.alpha[0, :, 0])
    total = sum(x.dft_get(msca.handle, 0) for x in [sca.fields])
    plain = sim.fields.dft_get(mon.handle, 0)
    assert np.max(np.abs(total)) < np.max(np.abs(plain))  # the incident wave is gone
    # and with the monitor's own data: negation is exact in every product and sum
    data = sim.get_flux_data(mon)
    sim.load_minus_flux_data(mon, data)
    rm = sim.get_eigenmode_coefficients(mon, lst)
    assert np.array_equal(rm.alpha, -r3.alpha) and np.array_equal(rm.cscale, r3.cscale)
    with pytest.raises(NotImplementedError, match="MPB"):
        sim.get_eigenmode_coefficients(mon, [1])


# ------------------------------------------------------------------ 9. errors
def test_refusals():
    o, lo, hi = grating(ProductSim, scatterer=False, n=(16, 12, 24))
    f = o._fields()
    freqs = [0.3]
    h = add_plane(o, lo, hi, ZMON, freqs)
    m = [((0, 0, 0), None, 1, 0)]
    reg = ([lo[0], lo[1], ZMON], [hi[0], hi[1], ZMON], 2, 1.0)
    two = f.add_dft_flux([reg, ([lo[0], lo[1], -ZMON], [hi[0], hi[1], -ZMON], 2, -1.0)], freqs, 1)
    en = f.add_dft_energy([([-0.5, -0.5, 0.0], [0.5, 0.5, 0.5], 0, 1.0)], freqs, 1)
    for call in (f.mode_coefficients, f.mode_table):
        with pytest.raises(RuntimeError, match="meep: .*not a flux object"):
            call(en, m)
        with pytest.raises(RuntimeError, match="meep: .*not a flux object"):
            call(97, m)
        with pytest.raises(RuntimeError, match="meep: .*several regions"):
            call(two, m)
        with pytest.raises(RuntimeError, match="meep: .*nmodes < 1"):
            call(h, [])
        with pytest.raises(RuntimeError, match="meep: .*parallel to the wavevector"):
            call(h, [((0, 0, 0), (0, 0, 1), 1, 0)])
    f.mode_coefficients(h, m)  # (the object still answers)
    # a 1-D cell
    o1 = vol(ProductSim, 1, [4.0], A3)
    o1.add_pml(0.5, dirs=(2,))
    f1 = o1._fields()
    h1 = f1.add_dft_flux([([0.0, 0.0, 2.5], [0.0, 0.0, 2.5], 2, 1.0)], freqs, 1)
    with pytest.raises(RuntimeError, match="meep: .*1-D cells"):
        f1.mode_coefficients(h1, m)
    # a susceptibility at the monitor
    od = vol(ProductSim, 3, [2.0, 1.5, 3.0], A3, center_origin=True)
    od.add_pml(0.5, dirs=(2,))
    od.add_lorentzian(0.5, 0.05, [np.ones(od.shape())] * 3)
    fd = od._fields()
    hd = fd.add_dft_flux([([-1.0, -0.75, ZMON], [1.0, 0.75, ZMON], 2, 1.0)], freqs, 1)
    with pytest.raises(RuntimeError, match="meep: .*susceptibility or a conductivity"):
        fd.mode_coefficients(hd, m)
