"""Shared helpers of the DFT energy / force tests: numpy restatements of the reference's loop
weights (compute_boundary_weights x dV, src/loop_in_chunks.cpp:257-300, 400-500), of the centred
average and the accumulation of dft_chunk::update_dft (src/dft.cpp:265-300), and of the sums
dft_energy::electric / magnetic (src/dft.cpp:657-687) and stress_sum (src/stress.cpp:90-99),
plus the one 3-D scene the tests share (tests/test_gpu_near2far.py's shape).

Tolerances (u = 2^-53):
  (a) 0 where product and oracle perform the same add_dft arithmetic;
  (b) 1e-12 of the largest expected value where two DFTs differ only by per-point weights
      (the margin of tests/test_gpu_dft_fields.py);
  (c) (N + 64) u sum |term| for a sum of N terms against a float64 sum in another order.
"""
import math

import numpy as np

U = 2.0 ** -53
FREQS = [0.25, 0.3, 0.37]
SIZES = [6.4, 4.0, 4.0]  # the smallest shape with a two-step region (temporal blocking)
A = 10.0
STEPS = 80
EX, EY, EZ, HX, HY, HZ, DX, DY, DZ, BX, BY, BZ = range(12)


def shift(c, d):
    """1 where component c sits at odd half-pixel coordinates along d (3-D)."""
    return int(d == c % 3) if c // 3 in (0, 2) else int(d != c % 3)


def boundary_weights_1d(wmin, wmax, a, sh):
    """compute_boundary_weights for one direction of a grid whose points sit at half-pixel
    coordinates of parity sh: (first half-pixel coordinate, weights per point, branch)."""
    yc, iyc = (1 - sh) * 0.5 / a, 1 - sh
    i0 = 1 + 2 * int(math.floor((wmin + yc) * a - .5)) - iyc
    i1 = 1 + 2 * int(math.ceil((wmax + yc) * a - .5)) - iyc
    w0, w1 = 1. - wmin * a + 0.5 * i0, 1. + wmax * a - 0.5 * i1
    s0 = s1 = e0 = e1 = 1.0
    branch = -1
    if i1 >= i0 + 6:
        s0, s1 = w0 * w0 / 2, 1 - (1 - w0) * (1 - w0) / 2
        e0, e1 = w1 * w1 / 2, 1 - (1 - w1) * (1 - w1) / 2
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
    return i0, w, branch


def loop_weights(pos, lo, hi, a, comp=None):
    """The loop weight of every point of pos (N, 3) of a region [lo, hi] of a 3-D cell: the
    product of the three directions' boundary weights and dV = a^-(non-empty directions).
    comp None: the centred grid; else the Yee grid of that component."""
    w = np.ones(len(pos))
    dv = 1.0
    for d in range(3):
        sh = 1 if comp is None else shift(comp, d)
        i0, wd, _ = boundary_weights_1d(lo[d], hi[d], a, sh)
        half = np.rint(pos[:, d] * 2 * a).astype(int)
        assert np.max(np.abs(half - pos[:, d] * 2 * a)) < 1e-9
        k = (half - i0) // 2
        assert np.all((half - i0) % 2 == 0) and k.min() >= 0 and k.max() < len(wd), (d, comp)
        w = w * wd[k]
        if hi[d] - lo[d] > 0:
            dv /= a
    return w * dv


def check_weights(got, want, pos):
    """dft_points' weights against the restatement: the roundings of the products only."""
    tol = 64 * U * np.maximum(1.0, np.max(np.abs(pos), axis=1)) * np.abs(want)
    assert np.all(np.abs(got - want) <= tol), float(np.max(np.abs(got - want) - tol))


def pair_sum(a, b, x, nf):
    """sum over the points of x * real(a conj(b)) per frequency and the sum of |term| (lists
    in list order [point][freq]; x a scalar or per point)."""
    a, b = a.reshape(-1, nf), b.reshape(-1, nf)
    t = np.reshape(x, (-1, 1)) * (a.real * b.real + a.imag * b.imag)
    return t.sum(axis=0), np.abs(t).sum(axis=0), len(a)


def check_sum(got, want, s, n, label=""):
    """tolerance (c)"""
    bound = (n + 64) * U * s
    err = np.abs(got - want)
    print(f"{label}: N = {n}, sum = {want}, max err / bound = {np.max(err / bound):.3e}")
    assert np.all(s > 0) and np.all(want != 0) and np.all(np.isfinite(got))
    assert np.all(err <= bound), (label, err, bound)


def centred_sample(arr, pos, comp, io, a):
    """The centred average of update_dft without its weight: the sum of the 1, 2 or 4 Yee
    values of component comp (whole-cell array arr) around each centred point of pos, and the
    factor 1, 0.5 or 0.25."""
    half = np.rint(pos * 2 * a).astype(int)
    j = [(half[:, d] - 1 - io[d]) // 2 for d in range(3)]
    un = [d for d in range(3) if not shift(comp, d)]
    v = arr[j[0], j[1], j[2]]
    if len(un) >= 1:
        k = [j[d] + (d == un[0]) for d in range(3)]
        v = v + arr[k[0], k[1], k[2]]
    if len(un) == 2:
        k = [j[d] + (d == un[1]) for d in range(3)]
        v = v + arr[k[0], k[1], k[2]]
        k = [j[d] + (d in un) for d in range(3)]
        v = v + arr[k[0], k[1], k[2]]
    return v, (1.0, 0.5, 0.25)[len(un)]


def yee_sample(arr, pos, comp, io, a):
    half = np.rint(pos * 2 * a).astype(int)
    j = [(half[:, d] - io[d] - shift(comp, d)) // 2 for d in range(3)]
    return arr[j[0], j[1], j[2]]


def phases(t, dt, magnetic, freqs=FREQS):
    """polar(1, omega time) * dt / sqrt(2 pi) after step t: time t dt for E and D, half a
    step earlier for H and B (is_H_or_B, src/dft.cpp:260)."""
    time = t * dt - (0.5 * dt if magnetic else 0.0)
    om = 2 * math.pi * np.asarray(freqs)
    return np.exp(1j * om * time) * (dt / math.sqrt(2 * math.pi))


def build_cell(make, medium="uniform", tb=None):
    """64 x 40 x 40 cells with PML 1.0 and two Gaussian currents.  uniform: chi1inv = 0.5 on
    every E component.  blocks: an eps = 4 block and a Lorentzian slab (a few z planes, so
    that a two-step region remains above it) in eps = 2, so that D != eps E."""
    from scenarios import vol
    o = vol(make, 3, SIZES, A, center_origin=True)
    o.add_pml(1.0)
    for c in (EX, EY, EZ):
        u = np.full(o.shape(), 0.5)
        if medium == "blocks":
            x, y, z = o.coords(c)
            u = np.where((x > 0.1) & (x < 0.6) & (np.abs(y) < 0.45) & (np.abs(z) < 0.5), 0.25, 0.5)
        o.set_chi1inv(c, c, u)
    if medium == "blocks":
        sig = []
        for c in (EX, EY, EZ):
            x, y, z = o.coords(c)
            sig.append(np.where((z > -0.75) & (z < -0.55), 1.5, 0.0) + 0 * x + 0 * y)
        o.add_lorentzian(0.4, 0.05, sig)
    o.add_gaussian_source(2, 0.3, 1.0, 0.0, 8.0, (0.05, 0.05, 0.05), 1.0)
    o.add_gaussian_source(1, 0.27, 0.8, 0.0, 6.0, (-0.33, 0.12, 0.41), 0.7)
    if tb is not None:
        for f in (o._all() if hasattr(o, "_all") else [o._fields()]):
            f.set_temporal_blocking(tb)
    return o


def all_fields(o):
    return o._all() if hasattr(o, "_all") else [o._fields()]


def add_all(o, name, regions_list, freqs=FREQS, decimation=1):
    """One object of kind `name` (add_dft_energy / add_dft_force) per region list, on every
    rank; the handles."""
    hs = []
    for regs in regions_list:
        h = [getattr(f, name)(regs, freqs, decimation) for f in all_fields(o)]
        assert all(x == h[0] for x in h)
        hs.append(h[0])
    return hs


def lists_of(o, h, nlists):
    """Every list of object h, summed over the ranks (each point has one owner)."""
    return [sum(f.dft_get(h, w) for f in all_fields(o)) for w in range(nlists)]


def collective(o, fn):
    """fn(fields) on every rank at once; every rank must return the same bits."""
    if hasattr(o, "_all"):
        o._all()
        vals = o._par(fn)
        assert all(np.array_equal(v, vals[0]) for v in vals)
        return vals[0]
    return fn(o._fields())
