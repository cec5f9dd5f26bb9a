#!/usr/bin/env python3
"""Cost of the DFT energy and force monitors on bench.py's waveguide.

Builds the C3 waveguide at --size cells per side twice in one process: plain, and with a
--box^3-cell energy box x --nfreq frequencies around the centre plus a six-face force box
just inside the PML.  Steps the two in alternating segments of --steps steps and reports the
median ms/step of each (the difference is the sampling and accumulation of the monitors), then
times the sums: the wall time of dft_energy(h, 0) and dft_force(h) (pair-sum kernel, reduce
kernel, one small copy and the Python wrapper) and the bytes the pair sum reads (32 B per pair
point and frequency) over that wall time, a lower bound of the kernel's rate.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512, help="cells per side")
    ap.add_argument("--box", type=int, default=64, help="cells per side of the energy box")
    ap.add_argument("--nfreq", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40, help="steps per segment")
    ap.add_argument("--segments", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5, help="timed calls of each sum")
    args = ap.parse_args()

    import bench
    _, _, plain = bench.build_fields("waveguide", args.size, 0, 1, -1, None)
    _, _, mon = bench.build_fields("waveguide", args.size, 0, 1, -1, None)
    half = 0.5 * args.size / 10.0
    e = 0.5 * args.box / 10.0
    freqs = np.linspace(0.1, 0.2, args.nfreq)
    he = mon.add_dft_energy([([-e, -e, -e], [e, e, e], 0, 1.0)], freqs, 1)
    b = half - 1.2  # the core crosses the x faces: keep the force box in the cladding
    lo, hi = [-b, 0.7, -b], [b, b, b]
    faces = []
    for d in range(3):
        for sgn, at in ((1.0, hi[d]), (-1.0, lo[d])):
            rl, rh = list(lo), list(hi)
            rl[d] = rh[d] = at
            faces.append((rl, rh, 0, sgn))
    hf = mon.add_dft_force(faces, freqs, 1)
    for f in (plain, mon):  # warm-up: tuner, plans, code objects
        f.step(args.steps)
    ms = {"plain": [], "monitors": []}
    for _ in range(args.segments):
        for name, f in (("plain", plain), ("monitors", mon)):
            t0 = time.perf_counter()
            f.step(args.steps)
            f.dft_flush()
            ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
    res = {"size": args.size, "energy_box_cells": args.box, "nfreq": args.nfreq,
           "steps_per_segment": args.steps,
           "ms_per_step": {k: [round(v, 4) for v in vals] for k, vals in ms.items()},
           "median_ms_per_step": {k: round(statistics.median(v), 4) for k, v in ms.items()},
           "pairs_active": bool(mon.tb_info()["active"])}
    res["monitors_ms_per_step"] = round(res["median_ms_per_step"]["monitors"] -
                                        res["median_ms_per_step"]["plain"], 4)
    sums = {}
    for name, call, lists in (("electric", lambda: mon.dft_energy(he, 0), (he, 0)),
                              ("force", lambda: mon.dft_force(hf), None)):
        call()  # warm-up: the run table, the scratch buffers
        wall = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            v = call()
            wall.append((time.perf_counter() - t0) * 1e3)
        if lists:
            pairs = mon.dft_list_size(*lists) // args.nfreq
        else:  # (offdiag1, offdiag2) and (diag, diag)
            pairs = (mon.dft_list_size(hf, 0) + mon.dft_list_size(hf, 2)) // args.nfreq
        nbytes = 32.0 * pairs * args.nfreq
        best = min(wall)
        sums[name] = {"pair_points": pairs, "bytes_read": nbytes, "best_wall_ms": round(best, 4),
                      "bytes_per_s_over_wall": nbytes / (best * 1e-3), "finite": bool(np.all(np.isfinite(v)))}
    res["sums"] = sums
    print(json.dumps(res))


if __name__ == "__main__":
    main()
