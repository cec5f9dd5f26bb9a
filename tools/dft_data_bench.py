#!/usr/bin/env python3
"""Time get / load / scale of the DFT data of one flux plane (Fields.dft_get, dft_load,
dft_scale) against the whole-array reader (Fields.dft_data).

Builds bench.py's vacuum cell at --size cells per side, adds one x-normal flux plane across the
whole cell (two E and two H components, through the PML) with --nfreq frequencies, runs a few
steps so the array holds data, then times, best of --reps:
  * dft_data(h, 0): the whole padded array to the host, permuted there by one thread;
  * dft_get(h, 0): the gather kernel and a device-to-host copy of that list only;
  * dft_load(h, 0, d): a host-to-device copy of the list and the scatter kernel;
  * dft_scale(h, s): one pass over the object's array.
Wall times are host clocks around calls that end in a device synchronise.  The kernels' own
times come from HIP events (Fields.kernel_stats 11 / 12 / 13) and are reported as GB/s of their
algorithmic bytes and as a fraction of the 6.3 TB/s copy rate of DESIGN.md section 7,
separately from the host copies.  Prints one JSON line; the figures are a record, not a gate.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COPY_RATE_GBS = 6300.0


def best_of(reps, fn):
    best = None
    for _ in range(reps):
        w0 = time.perf_counter()
        out = fn()
        ms = (time.perf_counter() - w0) * 1e3
        if best is None or ms < best[0]:
            best = (ms, out)
    return best


def kernel_rate(f, kind, reps, fn):
    """Best HIP-event time of the kernel `kind` over reps calls of fn, with its bytes."""
    best = None
    for _ in range(reps):
        n0, ms0, _ = f.kernel_stats(kind)
        fn()
        n1, ms1, nbytes = f.kernel_stats(kind)
        ms = (ms1 - ms0) / max(n1 - n0, 1)
        if best is None or ms < best[0]:
            best = (ms, nbytes)
    ms, nbytes = best
    gbs = nbytes / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    return {"kernel_ms": round(ms, 4), "bytes": nbytes, "GBps": round(gbs, 1),
            "fraction_of_copy_rate": round(gbs / COPY_RATE_GBS, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256, help="cells per side")
    ap.add_argument("--nfreq", type=int, default=50)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import bench
    gv, s, f = bench.build_fields("vacuum", args.size, 0, 1, -1, None)
    half = 0.5 * args.size / 10.0
    freqs = np.linspace(0.1, 0.2, args.nfreq)
    h = f.add_dft_flux([([0.05, -half, -half], [0.05, half, half], 0, 1.0)], freqs, 1)
    f.step(args.steps)
    f.dft_flush()
    ref = f.dft_data(h, 0)
    d = f.dft_get(h, 0)  # warm-up: inverse map, list buffer
    same = bool(np.array_equal(ref, d)) and bool(np.any(d != 0))
    res = {"size": args.size, "nfreq": args.nfreq, "list_points": d.size // args.nfreq,
           "list_MB": round(d.nbytes / 1e6, 1), "dft_get_equals_dft_data": same}
    t_data, _ = best_of(args.reps, lambda: f.dft_data(h, 0))
    t_get, _ = best_of(args.reps, lambda: f.dft_get(h, 0))
    t_load, _ = best_of(args.reps, lambda: f.dft_load(h, 0, d))
    t_scale, _ = best_of(args.reps, lambda: f.dft_scale(h, 1.0))
    res.update({"dft_data_ms": round(t_data, 3), "dft_get_ms": round(t_get, 3),
                "dft_get_over_dft_data": round(t_get / t_data, 4),
                "dft_load_ms": round(t_load, 3), "dft_scale_ms": round(t_scale, 3)})
    res["gather"] = kernel_rate(f, 11, args.reps, lambda: f.dft_get(h, 0))
    res["scatter"] = kernel_rate(f, 12, args.reps, lambda: f.dft_load(h, 0, d))
    res["scale"] = kernel_rate(f, 13, args.reps, lambda: f.dft_scale(h, 1.0))
    res["unchanged_after_load_and_scale"] = bool(np.array_equal(f.dft_get(h, 0), d))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
