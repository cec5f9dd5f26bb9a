#!/usr/bin/env python3
"""Cost of complex fields and the Bloch-phase wrap: one process steps a
vacuum cell with PML in z and periodic x / y faces three ways -- real fields at k = 0, complex
fields at k = 0, complex fields at k = (0.1, 0.2, 0) -- each in the unfused mode and in the fused
mode one step at a time (pairs of steps off: complex fields have none).  Segments of the six
alternate, so drift and allocation placement hit them alike; medians are reported.

The expectation is two real steps plus the wrap: complex fields step the same kernels once per
part.  wrap_ms_per_step is the library's halo phase timer (HIP events around the launches that
fill ghost planes) of a profiled segment: on one rank those are the wrap launches alone, two
per step (real fields: wrap_kernel; complex: wrap_phase_kernel over both parts).

    python tools/bloch_bench.py --size 256 --steps 40 --segments 7 --out profiles/bloch/x.json
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


def make(size, a, dpml, k, fused):
    """k=None: real fields at k = 0; else complex fields with that (kx, ky)."""
    gv = core.GridVolume(3, [size, size, size], a, [-size, -size, -size])
    s = core.Structure(gv)
    s.add_pml(dpml, (2,), (0, 1))
    f = core.Fields(s)
    if k is not None:
        f.use_complex_fields()
    for d in (0, 1):
        f.use_bloch(d, 0 if k is None else k[d])
    f.set_temporal_blocking(False)
    f.set_fused(fused)
    L = size / a
    f.add_gaussian_volume_source(0, 0.15, 0.1, 0.0, 1e9,
                                 [-L / 2, -L / 2, 0.25 * L], [L / 2, L / 2, 0.25 * L], 1.0 + 0.5j)
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
    ks = {"real_k0": None, "complex_k0": (0.0, 0.0), "complex_k": (0.1, 0.2)}
    runs = {"%s_%s" % (name, "fused" if fused else "unfused"): make(a.size, res, dpml, k, fused)
            for fused in (False, True) for name, k in ks.items()}
    ms = {k: [] for k in runs}
    for _ in range(a.segments):
        for k, f in runs.items():
            t0 = time.perf_counter()
            f.step(a.steps)  # returns after the stream is synchronized
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.steps)
    out = {"size": a.size, "steps_per_segment": a.steps, "segments": a.segments,
           "fused": {k: bool(f.fused_active()) for k, f in runs.items()},
           "ms_per_step_median": {k: statistics.median(v) for k, v in ms.items()},
           "ms_per_step_all": ms, "wrap_ms_per_step": {}, "wrap_launches_per_step": 2}
    for k, f in runs.items():
        f.set_profiling(True)
        f.step(a.steps)
        out["wrap_ms_per_step"][k] = f.timers()["BoundarySteppingHalo"] / a.steps
        f.set_profiling(False)
    m = out["ms_per_step_median"]
    for mode in ("unfused", "fused"):
        for name in ("complex_k0", "complex_k"):
            out["%s_over_real_%s" % (name, mode)] = m["%s_%s" % (name, mode)] / m["real_k0_" + mode]
    assert np.isfinite(runs["complex_k_fused"].get_array(0, 1)).all()
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
