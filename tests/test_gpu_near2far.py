"""Near-to-far-field monitors (fields::add_dft_near2far, dft_near2far::farfield / flux,
src/near2far.cpp) on the GPU.

The oracle has no near2far, so the expectation is built from what it has (Yee-grid
dft_fields over the same volumes), from numpy restatements of the reference's formulas held
in this file (compute_boundary_weights, green3d) and from physics (the reference's own
tests/near2far.cpp check against the analytic dipole field).

Tolerances (u = 2^-53):
  * DFT values: 1e-12 of the largest value, the project's margin for two DFT objects that
    differ only in their weights (tests/test_gpu_dft_fields.py).
  * weights: rounding of the sums only, 64 u sum |w_i| max(1, |x0|).
  * transform: (N + 2 k r_max + 64) u S with S = sum_i |term_i| of the restatement: N u bounds
    any two summation orders, 2 k r_max u the phase rounding of sincos(k r) in two
    implementations, 64 u the remaining roundings per term.
  * physics: the reference's 0.05 * 30 / a (tests/near2far.cpp:107, 173, 238); twice that for
    the flux, which is quadratic in the field.
"""
import math

import numpy as np
import pytest

from scenarios import GroupSim3, ProductSim, flux_box_faces, make_oracle, vol

gpu = pytest.mark.gpu
U = 2.0 ** -53
FREQS = [0.25, 0.3, 0.37]
SIZES = [6.4, 4.0, 4.0]  # the smallest shape with a two-step region (temporal blocking)
STEPS = 80
EX, EY, EZ, HX, HY, HZ = range(6)
WG_SLOTS = 1024  # slots per workgroup of the far-field kernel for objects this small

# one single-region object per normal direction: (lo, hi, normal, weight)
SINGLE = [
    ([0.5, -0.6, -0.4], [0.5, 0.6, 0.7], 0, 1.0),        # edges on lattice points
    ([-0.73, 0.23, -0.73], [0.73, 0.23, 0.73], 1, -1.0),  # edges at arbitrary positions
    ([0.02, -0.55, -0.31], [0.19, 0.41, -0.31], 2, 0.5),  # 1.7 pixels wide along x
]
BOX = flux_box_faces([-0.52, -0.47, -0.43], [0.54, 0.57, 0.48], 3)
FAR = np.array([[0.7, 0.1, 0.05], [-0.6, -0.62, 0.3], [5.0, 0.3, -0.2], [-3.0, 4.0, 1.0],
                [0.2, -0.1, 5.3], [0.0, 0.0, 4.0], [2.0, -6.0, 0.5]])


def comps_of(nd):
    """(c, c0, s) in add_dft_near2far's loop order (src/near2far.cpp:583-636)."""
    fd = ((nd + 1) % 3, (nd + 2) % 3)
    out = []
    for i in range(2):
        for j in range(2):
            c = (EX if i == 0 else HX) + fd[j]
            c0 = (HX if i == 0 else EX) + fd[1 - j]
            s = 1.0 if j == 0 else -1.0
            if i == 0:
                s = -s
            out.append((c, c0, s))
    return out


def build(make, n2f=True, tb=None):
    """sc_flux_3d's shape (64 x 40 x 40 cells with PML), uniform eps = 2, two Gaussian
    currents."""
    o = vol(make, 3, SIZES, 10, center_origin=True)
    o.add_pml(1.0)
    for c in (EX, EY, EZ):
        o.set_chi1inv(c, c, np.full(o.shape(), 0.5))
    o.add_gaussian_source(2, 0.3, 1.0, 0.0, 8.0, (0.05, 0.05, 0.05), 1.0)
    o.add_gaussian_source(1, 0.27, 0.8, 0.0, 6.0, (-0.33, 0.12, 0.41), 0.7)
    if not n2f:
        return o, []
    fs = o._all() if hasattr(o, "_all") else [o._fields()]
    hs = []
    for regs in [[r] for r in SINGLE] + [BOX]:
        h = [f.add_dft_near2far(regs, FREQS, 1) for f in fs]
        assert all(x == h[0] for x in h)
        hs.append(h[0])
    if tb is not None:
        for f in fs:
            f.set_temporal_blocking(tb)
    return o, hs


def farfields(o, h, pts):
    if hasattr(o, "_all"):
        vals = o._par(lambda f: f.near2far_farfields(h, pts))  # collective, every rank the sum
        assert all(np.array_equal(v, vals[0]) for v in vals)
        return vals[0]
    return o._fields().near2far_farfields(h, pts)


@pytest.fixture(scope="module")
def base():
    """(a) of the modes: fused with temporal blocking, one call of 40 steps and one of 40."""
    o, hs = build(ProductSim, tb=True)
    o.step(STEPS // 2)
    o.step(STEPS - STEPS // 2)
    f = o._fields()
    return {"o": o, "hs": hs, "fused": f.fused_active(), "tb": f.tb_info(),
            "dft": o.dft_data(hs[3], 0), "far": farfields(o, hs[3], FAR)}


# ------------------------------------------------------------------ 1. DFT values
@gpu
def test_dft_values_against_oracle(base):
    p, hs = base["o"], base["hs"]
    o, _ = build(make_oracle, n2f=False)
    ho = [o.add_dft_fields([c for c, _, _ in comps_of(nd)], lo, hi, FREQS, True, 1)
          for lo, hi, nd, _ in SINGLE]
    o.step(STEPS)
    for h, g in zip(hs[:3], ho):
        got, ref = p.dft_data(h, 0), o.dft_data(g, 0)
        w = np.repeat(p._fields().near2far_points(h)[:, 4], len(FREQS))
        assert got.size == ref.size == w.size and got.size > 0
        assert p.dft_decimation(h) == o.dft_decimation(g) == 1
        want = w * ref
        err = np.max(np.abs(got - want))
        print(f"object {h}: {got.size} values, max |n2f - w o| = {err:.3e}, "
              f"max |w o| = {np.max(np.abs(want)):.3e}")
        assert np.max(np.abs(want)) > 0
        assert err <= 1e-12 * np.max(np.abs(want))


# ------------------------------------------------------------------ 2. geometry and weights
def boundary_weights_1d(wmin, wmax, a, sh):
    """compute_boundary_weights (src/loop_in_chunks.cpp:257-300) for one direction of a grid
    whose points sit at half-pixel coordinates of parity sh; returns (positions, weights)."""
    yc, iyc = (1 - sh) * 0.5 / a, 1 - sh
    i0 = 1 + 2 * int(math.floor((wmin + yc) * a - .5)) - iyc
    i1 = 1 + 2 * int(math.ceil((wmax + yc) * a - .5)) - iyc
    w0, w1 = 1. - wmin * a + 0.5 * i0, 1. + wmax * a - 0.5 * i1
    s0 = s1 = e0 = e1 = 1.0
    branch = -1
    if i1 >= i0 + 6:
        s0, s1, e0, e1 = w0 * w0 / 2, 1 - (1 - w0) * (1 - w0) / 2, w1 * w1 / 2, 1 - (1 - w1) * (1 - w1) / 2
        branch = 0
    elif i1 == i0 + 4:
        s0 = w0 * w0 / 2
        s1 = 1 - (1 - w0) * (1 - w0) / 2 - (1 - w1) * (1 - w1) / 2
        e0, e1 = w1 * w1 / 2, s1
        branch = 1
    elif wmin == wmax:
        s0, s1, e0, e1 = w0, w1, w1, w0
        branch = 2
    elif i1 == i0 + 2:
        s0 = w0 * w0 / 2 - (1 - w1) * (1 - w1) / 2
        e0 = w1 * w1 / 2 - (1 - w0) * (1 - w0) / 2
        s1, e1 = e0, s0
        branch = 3
    n = (i1 - i0) // 2 + 1
    w = np.ones(n)
    for i in range(n):  # IVEC_LOOP_WEIGHT1: the first match of i == 0, 1, n - 1, n - 2
        if 1 < i < n - 2:
            continue
        w[i] = s0 if i == 0 else s1 if i == 1 else e0 if i == n - 1 else e1 if i == n - 2 else 1.0
    return (i0 + 2 * np.arange(n)) * (0.5 / a), w, branch


def test_boundary_weights_integrate_linear_interpolant():
    """sum_i w_i / a = length and sum_i w_i x_i / a = length * centre (a point: 1 and x) for
    20 000 random regions, every branch of compute_boundary_weights."""
    rng = np.random.default_rng(7)
    a = 10.0
    seen = set()
    worst = 0.0
    for k in range(20000):
        lo = rng.uniform(-1, 1)
        kind = k % 4
        ln = (0.0 if kind == 0 else rng.uniform(0, 0.1) if kind == 1 else rng.uniform(0.1, 0.35)
              if kind == 2 else rng.uniform(0, 1.5))
        hi = lo + ln
        x, w, br = boundary_weights_1d(lo, hi, a, k // 4 % 2)
        seen.add(br)
        if ln == 0.0:
            m0, m1 = 1.0, lo
            got0, got1 = w.sum(), (w * x).sum()
        else:
            m0, m1 = hi - lo, (hi - lo) * 0.5 * (hi + lo)
            got0, got1 = w.sum() / a, (w * x).sum() / a
        worst = max(worst, abs(got0 - m0), abs(got1 - m1))
    assert seen == {0, 1, 2, 3}
    assert worst <= 5e-15, worst


@gpu
def test_points_and_weights(base):
    p, hs = base["o"], base["hs"]
    a = 10.0
    for h, (lo, hi, nd, weight) in zip(hs[:3], SINGLE):
        pts = p._fields().near2far_points(h)
        x0, c0s, w = pts[:, :3], pts[:, 3].astype(int), pts[:, 4]
        area = np.prod([hi[d] - lo[d] for d in range(3) if d != nd])
        centre = [0.5 * (lo[d] + hi[d]) for d in range(3)]
        assert sorted(set(c0s)) == sorted(c0 for _, c0, _ in comps_of(nd))
        for c, c0, s in comps_of(nd):
            m = c0s == c0
            # the points sit on c's Yee grid: odd half-pixel coordinates where c is shifted
            half = np.rint(x0[m] * 2 * a).astype(int)
            assert np.max(np.abs(half - x0[m] * 2 * a)) < 1e-9
            for d in range(3):
                shifted = (d == c % 3) if c < 3 else (d != c % 3)
                assert np.all(half[:, d] % 2 == int(shifted)), (h, c, d)
            assert np.all(np.sign(w[m][w[m] != 0]) == np.sign(s * weight))
            tol = 64 * U * np.sum(np.abs(w[m]))
            assert abs(np.sum(w[m]) - s * weight * area) <= tol, (h, c)
            for d in range(3):
                told = 64 * U * np.sum(np.abs(w[m]) * np.maximum(1.0, np.abs(x0[m, d])))
                got = np.sum(w[m] * x0[m, d])
                assert abs(got - s * weight * area * centre[d]) <= told, (h, c, d, got)


# ------------------------------------------------------------------ 3. transform
def green3d(x, freq, eps, mu, x0, c0, f0):
    """green3d (src/near2far.cpp:133-187) for arrays of near points x0 (N, 3), equivalent
    currents c0 (N,) and amplitudes f0 (N,): EH (N, 6) at the far point x."""
    rhat = x[None, :] - x0
    r = np.sqrt(rhat[:, 0] * rhat[:, 0] + rhat[:, 1] * rhat[:, 1] + rhat[:, 2] * rhat[:, 2])
    rhat = rhat / r[:, None]
    n = math.sqrt(eps * mu)
    k = 2 * math.pi * freq * n
    ikr = 1j * (k * r)
    ikr2 = -(k * r) * (k * r)
    amp = k * n / (4 * math.pi * r)
    th = k * r + math.pi * 0.5
    expfac = f0 * (amp * np.cos(th) + 1j * (amp * np.sin(th)))
    Z = math.sqrt(mu / eps)
    p = np.zeros_like(x0)
    p[np.arange(len(x0)), c0 % 3] = 1.0
    pdotrhat = np.sum(p * rhat, axis=1)
    rxp = np.cross(rhat, p)
    term1 = 1.0 - 1.0 / ikr + 1.0 / ikr2
    term2 = (-1.0 + 3.0 / ikr - 3.0 / ikr2) * pdotrhat
    term3 = 1.0 - 1.0 / ikr
    elec = c0 < 3
    expfac = np.where(elec, expfac / eps, expfac / mu)
    main = expfac[:, None] * (term1[:, None] * p + term2[:, None] * rhat)
    cross = (expfac * term3)[:, None] * rxp
    EH = np.empty((len(x0), 6), dtype=complex)
    EH[:, 0:3] = np.where(elec[:, None], main, -cross * Z)
    EH[:, 3:6] = np.where(elec[:, None], cross / Z, main)
    return EH


def restated(points, dft, far, eps=2.0, mu=1.0):
    """(sum, S = sum of |term|, k r_max) per far point and frequency."""
    x0, c0 = points[:, :3], points[:, 3].astype(int)
    nf = len(FREQS)
    f = dft.reshape(-1, nf)
    want = np.zeros((len(far), nf, 6), dtype=complex)
    S = np.zeros((len(far), nf, 6))
    kr = np.zeros((len(far), nf))
    for ip, x in enumerate(far):
        rmax = np.max(np.linalg.norm(x[None, :] - x0, axis=1))
        for i, fr in enumerate(FREQS):
            t = green3d(x, fr, eps, mu, x0, c0, f[:, i])
            want[ip, i] = t.sum(axis=0)
            S[ip, i] = np.abs(t).sum(axis=0)
            kr[ip, i] = 2 * math.pi * fr * math.sqrt(eps * mu) * rmax
    return want, S, kr


def check_far(got, points, dft, far, label):
    want, S, kr = restated(points, dft, far)
    n = len(points)
    bound = (n + 2 * kr[:, :, None] + 64) * U * S
    err = np.abs(got - want)
    print(f"{label}: N = {n}, max |got - want| / bound = {np.max(err / bound):.3e}, "
          f"max |got - want| / S = {np.max(err / S):.3e}")
    assert np.all(S > 0) and np.all(np.isfinite(got))
    assert np.all(err <= bound)


@gpu
def test_farfields_against_restatement(base):
    p, h = base["o"], base["hs"][3]
    pts = p._fields().near2far_points(h)
    n = len(pts)
    assert n >= 3 * WG_SLOTS and n % 64 != 0, n  # several workgroups and a masked tail
    eps, mu = p._fields().near2far_medium(h)
    assert abs(eps - 2.0) <= 1e-14 and abs(mu - 1.0) <= 1e-14
    check_far(base["far"], pts, base["dft"], FAR, "box")


# ------------------------------------------------------------------ 4. determinism
@gpu
def test_farfields_deterministic_and_batch_independent(base):
    p, h = base["o"], base["hs"][3]
    again = farfields(p, h, FAR)
    assert np.array_equal(again, base["far"])
    for i in range(len(FAR)):
        assert np.array_equal(farfields(p, h, FAR[i:i + 1])[0], base["far"][i]), i
    for trio in ([0, 1, 2], [3, 4, 5], [6, 0, 3], [2, 6, 4], [5, 3, 1]):
        got = farfields(p, h, FAR[trio])
        for k, i in enumerate(trio):
            assert np.array_equal(got[k], base["far"][i]), (trio, i)


# ------------------------------------------------------------------ 5. modes
@gpu
def test_mode_fused_temporal_blocking(base):
    assert base["fused"] and base["tb"]["active"], base["tb"]
    assert np.any(base["dft"] != 0)


@gpu
def test_mode_unfused(base, monkeypatch):
    monkeypatch.setenv("MNL_NO_FUSED", "1")
    o, hs = build(ProductSim)
    o.step(STEPS)
    assert not o._fields().fused_active()
    assert np.array_equal(o.dft_data(hs[3], 0), base["dft"])
    assert np.array_equal(farfields(o, hs[3], FAR), base["far"])


@gpu
def test_mode_three_slabs(base):
    o, hs = build(GroupSim3)
    o.step(STEPS)
    assert np.array_equal(o.dft_data(hs[3], 0), base["dft"])  # assembled over the ranks
    pts = base["o"]._fields().near2far_points(base["hs"][3])
    for f in o._all():
        assert np.array_equal(f.near2far_points(hs[3]), pts)
    check_far(farfields(o, hs[3], FAR), pts, base["dft"], FAR, "three slabs")


@gpu
def test_mode_single_steps_with_read_in_the_middle(base):
    o, hs = build(ProductSim)
    for k in range(STEPS):
        o.step(1)
        if k == STEPS // 2:
            mid = farfields(o, hs[3], FAR[:1])
            assert np.all(np.isfinite(mid)) and np.any(mid != 0)
    assert np.array_equal(o.dft_data(hs[3], 0), base["dft"])
    assert np.array_equal(farfields(o, hs[3], FAR), base["far"])


# ------------------------------------------------------------------ 6. checkpoint
@gpu
def test_checkpoint_resume(base, tmp_path):
    a, ha = build(ProductSim)
    a.step(40)
    path = str(tmp_path / "n2f.mnl")
    a.dump(path)
    b, hb = build(ProductSim)
    b.load(path)
    b.step(STEPS - 40)
    assert np.array_equal(b.dft_data(hb[3], 0), base["dft"])
    assert np.array_equal(farfields(b, hb[3], FAR), base["far"])


# ------------------------------------------------------------------ 7. errors
@gpu
def test_errors():
    o = vol(ProductSim, 3, SIZES, 10, center_origin=True)
    o.add_pml(1.0)
    for c in (EX, EY, EZ):
        x, y, z = o.coords(c)
        o.set_chi1inv(c, c, np.where(z < -0.3, 0.25, 0.5) + 0 * x + 0 * y)  # eps 4 under one face
    f = o._fields()
    with pytest.raises(RuntimeError, match="meep: dft_near2far requires surfaces in a homogeneous medium"):
        f.add_dft_near2far(BOX, FREQS, 1)
    p, hs = build(ProductSim)
    f = p._fields()
    with pytest.raises(RuntimeError, match="meep:.*periodic"):
        f.add_dft_near2far(BOX, FREQS, 1, nperiods=2)
    hf = f.add_dft_flux([SINGLE[0]], FREQS, 1)
    with pytest.raises(RuntimeError, match="meep:.*not a near2far object"):
        f.near2far_farfields(hf, FAR)
    with pytest.raises(RuntimeError, match="meep:.*not a near2far object"):
        f.near2far_points(hf)
    q = vol(ProductSim, 2, [3.2, 3.2], 10, center_origin=True)
    q.add_pml(1.0)
    with pytest.raises(RuntimeError, match="meep:.*3-D only"):
        q._fields().add_dft_near2far([([0.5, -0.5, 0], [0.5, 0.5, 0], 0, 1.0)], FREQS, 1)


# ------------------------------------------------------------------ 8. physics
def yee_axis(lo, hi, a, shifted):
    """Positions of a Yee-grid dft_fields object along one direction (loop_in_chunks with
    cgrid = c, src/loop_in_chunks.cpp:350-356)."""
    if shifted:
        i0, i1 = 1 + 2 * math.floor(lo * a - .5), 1 + 2 * math.ceil(hi * a - .5)
    else:
        i0, i1 = 2 * math.floor(lo * a), 2 * math.ceil(hi * a)
    return np.arange(i0, i1 + 1, 2) * (0.5 / a)


def trilinear(arr, axes, x):
    out, idx, wts = 0.0, [], []
    for d in range(3):
        ax = axes[d]
        i = int(np.clip(np.searchsorted(ax, x[d]) - 1, 0, len(ax) - 2))
        t = (x[d] - ax[i]) / (ax[i + 1] - ax[i])
        idx.append(i)
        wts.append(t)
    for b in range(8):
        k = [(b >> d) & 1 for d in range(3)]
        w = np.prod([wts[d] if k[d] else 1 - wts[d] for d in range(3)])
        out = out + w * arr[idx[0] + k[0], idx[1] + k[1], idx[2] + k[2]]
    return out


@gpu
def test_point_dipole_green_and_near2far():
    """tests/near2far.cpp check_2d_3d(D3, 4, 10, Ez): the DFT fields of a point dipole in
    eps = 2 against green3d inside the cell (GREEN), the far fields of a near2far box
    against it outside the cell (NEAR2FAR), and the far-field flux through a closed box
    against the analytic dipole power."""
    import meep_nl_amd as mp
    xmax, a, w = 4.0, 10.0, 0.3
    tol = 0.05 * 30 / a
    cell = xmax + 2
    sim = mp.Simulation(cell_size=mp.Vector3(cell, cell, cell), resolution=a,
                        boundary_layers=[mp.PML(1.0)], default_material=mp.Medium(epsilon=2.0),
                        eps_averaging=False,
                        sources=[mp.Source(mp.GaussianSource(w, fwidth=0.3), mp.Ez,
                                           center=mp.Vector3())])
    L = xmax / 4
    faces = []
    for d in range(3):
        for sgn in (1.0, -1.0):
            c, s = [0.0, 0.0, 0.0], [2 * L, 2 * L, 2 * L]
            c[d], s[d] = sgn * L, 0.0
            faces.append(mp.Near2FarRegion(center=mp.Vector3(*c), size=mp.Vector3(*s), weight=sgn))
    n2f = sim.add_near2far(w, 0, 1, *faces, decimation_factor=1)
    comps = [mp.Ex, mp.Ey, mp.Ez, mp.Hx, mp.Hy, mp.Hz]
    mon = sim.add_dft_fields(comps, w, 0, 1, center=mp.Vector3(), size=mp.Vector3(xmax, xmax, xmax),
                             yee_grid=True, decimation_factor=1)
    sim.run(until=20)
    assert sim.fields.fused_active() and sim.fields.tb_info()["active"], sim.fields.tb_info()
    sim.run(until_after_sources=mp.stop_when_fields_decayed(5, mp.Ez, mp.Vector3(0.5 * xmax), 1e-7))
    N = 20
    dx = 0.75 * (xmax / 4) / N
    x0 = np.zeros((1, 3))
    src = np.array([EZ])

    def g(x):
        return green3d(np.asarray(x), w, 2.0, 1.0, x0, src, np.ones(1, dtype=complex))[0]

    # stage 1: GREEN
    pts1 = [np.array([s, 0.5 * s, 0.3 * s]) for s in (xmax / 4 + dx * i for i in range(N))]
    F = np.zeros((N, 6), dtype=complex)
    for c in comps:
        arr = sim.get_dft_array(mon, c, 0)
        axes = [yee_axis(-0.5 * xmax, 0.5 * xmax, a, (d == c % 3) if c < 3 else (d != c % 3))
                for d in range(3)]
        assert arr.shape == tuple(len(ax) for ax in axes), (c, arr.shape)
        for i, x in enumerate(pts1):
            F[i, c] = trilinear(arr, axes, x)
    F0 = np.array([g(x) for x in pts1])
    A = np.vdot(F0, F) / np.vdot(F0, F0)
    for c in comps:
        if np.linalg.norm(F0[:, c]) == 0:
            continue
        rel = np.linalg.norm(F[:, c] - A * F0[:, c]) / np.linalg.norm(A * F0[:, c])
        print(f"GREEN    comp {c}: relerr = {rel:.4f} (bound {tol})")
        assert rel <= tol, (c, rel)
    # stage 2: NEAR2FAR
    pts2 = [np.array([s, 0.5 * s, 0.3 * s]) for s in (xmax + dx * i for i in range(N))]
    G = np.array([np.array(sim.get_farfield(n2f, mp.Vector3(*x))).reshape(1, 6)[0] for x in pts2])
    G0 = np.array([g(x) for x in pts2])
    for c in comps:
        if np.linalg.norm(G0[:, c]) == 0:
            continue
        rel = np.linalg.norm(G[:, c] - A * G0[:, c]) / np.linalg.norm(A * G0[:, c])
        print(f"NEAR2FAR comp {c}: relerr = {rel:.4f} (bound {tol})")
        assert rel <= tol, (c, rel)
    # far-field flux through the closed box of half-size xmax against the dipole power:
    # |E x H*| = |expfac|^2 sin^2(theta) / Z far away, integrated over the sphere (8 pi / 3)
    n, Z = math.sqrt(2.0), math.sqrt(1 / 2.0)
    k = 2 * math.pi * w * n
    p_dipole = (k * n / (4 * math.pi * 2.0)) ** 2 / Z * 8 * math.pi / 3
    total = 0.0
    for d in range(3):
        for sgn in (1.0, -1.0):
            c, s = [0.0, 0.0, 0.0], [2 * xmax, 2 * xmax, 2 * xmax]
            c[d], s[d] = sgn * xmax, 0.0
            total += sgn * n2f.flux(d, mp.Volume(center=mp.Vector3(*c), size=mp.Vector3(*s)), a)[0]
    want = abs(A) ** 2 * p_dipole
    print(f"far-field flux {total:.6e}, |A|^2 P_dipole {want:.6e}, ratio {total / want:.4f}")
    assert abs(total - want) <= 2 * tol * want
    ff = sim.get_farfields(n2f, 1, center=mp.Vector3(xmax), size=mp.Vector3(0, 3, 2))
    assert ff["Ez"].shape == (3, 2) and np.all(np.isfinite(ff["Ez"]))
    assert mp.get_near2far_freqs(n2f) == [w]
