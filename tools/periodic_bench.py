#!/usr/bin/env python3
"""Cost of periodic x / y faces: one process steps a vacuum cell with PML in z four ways --
metal or periodic x / y faces, each in the unfused mode and in the fused mode one step at a
time -- with pairs of steps off everywhere (periodic runs have none yet), so that each pair of
runs takes the same step path.  Segments of the four alternate, so drift and allocation
placement hit them alike (allocations alone spread results by up to
14 %); medians are reported.

wrap_ms_per_step is the library's halo phase timer (HIP events around the launches that fill
ghost planes) of a profiled segment of each periodic run: on one rank those launches are the
wrap launches alone, two per step (E before curl B, B / H after the H update).

    python tools/periodic_bench.py --size 256 --steps 40 --segments 7 --out profiles/periodic/x.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from meep_nl_amd import core  # noqa: E402


def make(size, a, dpml, periodic, fused):
    gv = core.GridVolume(3, [size, size, size], a, [-size, -size, -size])
    s = core.Structure(gv)
    s.add_pml(dpml, (2,), (0, 1))
    f = core.Fields(s)
    if periodic:
        f.use_bloch(0)
        f.use_bloch(1)
    f.set_temporal_blocking(False)
    f.set_fused(fused)
    L = size / a
    f.add_gaussian_volume_source(0, 0.15, 0.1, 0.0, 1e9,
                                 [-L / 2, -L / 2, 0.25 * L], [L / 2, L / 2, 0.25 * L], 1.0)
    f.step(4)  # past the first (lazy-copy) step and the mode switch
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    res, dpml = 10.0, 1.0
    runs = {"metal_unfused": make(a.size, res, dpml, False, False),
            "periodic_unfused": make(a.size, res, dpml, True, False),
            "metal_fused": make(a.size, res, dpml, False, True),
            "periodic_fused": make(a.size, res, dpml, True, True)}
    ms = {k: [] for k in runs}
    for _ in range(a.segments):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f.step(a.steps)  # returns after the stream is synchronized
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    modes = {k: bool(f.fused_active()) for k, f in runs.items()}
    out = {"size": a.size, "steps_per_segment": a.steps, "segments": a.segments, "fused": modes,
           "ms_per_step_median": {k: statistics.median(v) for k, v in ms.items()},
           "ms_per_step_all": ms, "wrap_ms_per_step": {}, "wrap_launches_per_step": 2}
    for k in ("periodic_unfused", "periodic_fused"):
        f = runs[k]
        f.set_profiling(True)
        f.step(a.steps)
        out["wrap_ms_per_step"][k] = f.timers()["BoundarySteppingHalo"] / a.steps
        f.set_profiling(False)
    m = out["ms_per_step_median"]
    out["periodic_over_metal_unfused"] = m["periodic_unfused"] / m["metal_unfused"]
    out["periodic_over_metal_fused"] = m["periodic_fused"] / m["metal_fused"]
    assert np.isfinite(runs["periodic_fused"].get_array(0)).all()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
