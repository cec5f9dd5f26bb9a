#!/usr/bin/env python3
"""Time the near-to-far-field transform (Fields.near2far_farfields) on the GPU.

Builds bench.py's C3 waveguide (or plain vacuum) at --size cells per side, adds a six-face
near2far box just inside the PML, runs a few steps so the DFT arrays hold data, then times
one batched near2far_farfields call for a --far x --far grid of far points.

Prints one JSON line: near points, frequencies, far points, the wall time of the call (host clock around a call that ends in a device synchronise), the HIP-event times
of the far-field and the reduce kernel (Fields.kernel_stats 9 / 10), Green's-function
evaluations per second, and the shares of the reduce kernel and of the host (wall minus the
two kernels: copies, batching, the Python wrapper).  For scale it also times a plain
single-thread numpy evaluation of the same sum on a small sub-case (--cpu-near near points,
one frequency, --cpu-far far points) and reports the ratio of the evaluation rates; the ratio
is a record, not a gate.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def green3d_sum(x, freq, eps, mu, x0, c0, f0):
    """sum over the near points of green3d (src/near2far.cpp:133-187) at one far point."""
    rhat = x[None, :] - x0
    r = np.sqrt(np.sum(rhat * rhat, axis=1))
    rhat = rhat / r[:, None]
    n = math.sqrt(eps * mu)
    k = 2 * math.pi * freq * n
    ikr = 1j * (k * r)
    ikr2 = -(k * r) * (k * r)
    expfac = f0 * (k * n / (4 * math.pi * r)) * np.exp(1j * (k * r + math.pi * 0.5))
    Z = math.sqrt(mu / eps)
    p = np.zeros_like(x0)
    p[np.arange(len(x0)), c0 % 3] = 1.0
    pdr = np.sum(p * rhat, axis=1)
    rxp = np.cross(rhat, p)
    t1 = 1.0 - 1.0 / ikr + 1.0 / ikr2
    t2 = (-1.0 + 3.0 / ikr - 3.0 / ikr2) * pdr
    t3 = 1.0 - 1.0 / ikr
    elec = c0 < 3
    expfac = np.where(elec, expfac / eps, expfac / mu)
    main = expfac[:, None] * (t1[:, None] * p + t2[:, None] * rhat)
    cross = (expfac * t3)[:, None] * rxp
    eh = np.concatenate([np.where(elec[:, None], main, -cross * Z),
                         np.where(elec[:, None], cross / Z, main)], axis=1)
    return eh.sum(axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="cells per side")
    ap.add_argument("--vacuum", action="store_true", help="plain vacuum instead of the C3 waveguide")
    ap.add_argument("--nfreq", type=int, default=20)
    ap.add_argument("--far", type=int, default=32, help="far grid is far x far points")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3, help="timed calls (the best counts)")
    ap.add_argument("--cpu-near", type=int, default=20000)
    ap.add_argument("--cpu-far", type=int, default=4)
    args = ap.parse_args()

    import bench
    gv, s, f = bench.build_fields("vacuum" if args.vacuum else "waveguide", args.size, 0, 1, -1, None)
    half = 0.5 * args.size / 10.0
    if args.vacuum:
        b = half - 1.2  # just inside the PML
        lo, hi = [-b, -b, -b], [b, b, b]
    else:  # the waveguide core crosses the x faces: keep the box in the cladding beside it
        b = half - 1.2
        lo, hi = [-b, 0.7, -b], [b, b, b]
    regions = []
    for d in range(3):
        for sgn, at in ((1.0, hi[d]), (-1.0, lo[d])):
            rl, rh = list(lo), list(hi)
            rl[d] = rh[d] = at
            regions.append((rl, rh, d, sgn))
    freqs = np.linspace(0.1, 0.2, args.nfreq)
    t0 = time.time()
    h = f.add_dft_near2far(regions, freqs, 1)
    t_add = time.time() - t0
    f.step(args.steps)
    f.dft_flush()
    pts = f.near2far_points(h)
    near = len(pts)
    eps, mu = f.near2far_medium(h)
    R = 100.0 * half
    th = np.linspace(0.05, math.pi - 0.05, args.far)
    ph = np.linspace(0.0, 2 * math.pi, args.far, endpoint=False)
    T, P = np.meshgrid(th, ph, indexing="ij")
    far = np.stack([R * np.sin(T) * np.cos(P), R * np.sin(T) * np.sin(P), R * np.cos(T)],
                   axis=-1).reshape(-1, 3)
    evals = float(near) * args.nfreq * len(far)
    res = {"workload": "vacuum" if args.vacuum else "waveguide", "size": args.size,
           "near_points": near, "nfreq": args.nfreq, "far_points": len(far),
           "green_evaluations": evals, "eps": eps, "mu": mu, "add_near2far_s": round(t_add, 3),
           }
    f.near2far_farfields(h, far[:8])  # warm-up: code object, scratch buffers
    f.near2far_farfields(h, far)
    best = None
    for _ in range(args.reps):
        k0, r0 = f.kernel_stats("n2f_far"), f.kernel_stats("n2f_reduce")
        w0 = time.perf_counter()
        f.near2far_farfields(h, far)
        wall = (time.perf_counter() - w0) * 1e3
        k1, r1 = f.kernel_stats("n2f_far"), f.kernel_stats("n2f_reduce")
        cur = {"wall_ms": wall, "farfield_kernel_ms": k1[1] - k0[1],
               "reduce_kernel_ms": r1[1] - r0[1], "batches": k1[0] - k0[0]}
        if best is None or cur["wall_ms"] < best["wall_ms"]:
            best = cur
    best["evaluations_per_s"] = evals / (best["wall_ms"] * 1e-3)
    best["kernel_evaluations_per_s"] = evals / (best["farfield_kernel_ms"] * 1e-3)
    best["reduce_share"] = best["reduce_kernel_ms"] / best["wall_ms"]
    best["host_share"] = (best["wall_ms"] - best["farfield_kernel_ms"] -
                          best["reduce_kernel_ms"]) / best["wall_ms"]
    res.update({k: (round(v, 6) if isinstance(v, float) and v < 1e6 else v)
                for k, v in best.items()})
    # scale: the same sum in single-thread numpy on a sub-case
    n = min(args.cpu_near, near)
    x0, c0 = pts[:n, :3].copy(), pts[:n, 3].astype(int)
    f0 = np.ones(n, dtype=complex)  # timing only: any amplitudes cost the same
    w0 = time.perf_counter()
    for x in far[:args.cpu_far]:
        green3d_sum(x, freqs[0], eps, mu, x0, c0, f0)
    cpu_s = time.perf_counter() - w0
    cpu_rate = n * args.cpu_far / cpu_s
    res["numpy_single_thread"] = {"near_points": n, "far_points": args.cpu_far, "nfreq": 1,
                                  "seconds": round(cpu_s, 4), "evaluations_per_s": cpu_rate}
    res["gpu_over_numpy"] = res["evaluations_per_s"] / cpu_rate
    print(json.dumps(res))


if __name__ == "__main__":
    main()
