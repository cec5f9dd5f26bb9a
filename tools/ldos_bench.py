#!/usr/bin/env python3
"""Cost of LDOS spectra: configuration C2 (a 256^3 vacuum cell with PML)
run through Simulation.run five ways in one process --

    none        a point dipole, no LDOS object: what the parent commit runs
    point       the same with dft_ldos at 50 frequencies, batched (the updates on the device)
    point_one   the same in the one-step loop, forced by a no-op step function: one
                fields.step(1) and one explicit update per step
    point_idle  the point dipole with an LDOS object added that never records or updates
    none_1 / point_1   none and point with pairs of steps off (one fused step at a time): the
                cost of sampling every step without the pairs' middle-state sample
    plane_none  a full x-y plane source, no LDOS object
    plane       the same with dft_ldos at 50 frequencies, batched (size^2 source points)

Every batched run makes one fields.step call per segment (the runs without an LDOS object go
through the same batched runner, so that the call pattern is the same).  Each segment runs the
same number of steps in each; segments alternate, so drift and allocation
placement hit them alike, and medians are reported.  none's spread over its segments is the
run-to-run spread to hold a difference against.

dft_phase_ms_per_step is the DFT phase of the library's HIP-event timers (the sampling launch
of every step, the reduce / accumulate launches of every flush) per step, and
reduce_bytes_per_flush the algorithmic bytes of one flush of 32 updates: per point 32 sampled
values (8 B), the amplitude once per tile of 8 updates (16 B) and the owner flag (4 B of a
12-byte stride) with it.

    python tools/ldos_bench.py --size 256 --segments 7 --out profiles/ldos/c2_256.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import meep_nl_amd as mp  # noqa: E402

NFREQ = 50


def noop(sim):
    pass


def make(size, res, plane, pairs=True):
    L = size / res
    sim = mp.Simulation(cell_size=mp.Vector3(L, L, L), resolution=res,
                        boundary_layers=[mp.PML(1.0)],
                        sources=[mp.Source(mp.ContinuousSource(0.15), component=mp.Ez,
                                           center=mp.Vector3(0.05, 0.05, 0.05),
                                           size=mp.Vector3(L, L, 0) if plane else mp.Vector3())])
    sim.init_sim()
    if not pairs:
        sim.fields.set_temporal_blocking(False)
    sim.fields.step(4)  # past the first (lazy-copy) step and the mode switch
    return sim


def dft_ms(f, steps):
    f.set_profiling(True)
    before = f.kernel_stats(3)[1]
    f.step(steps)
    ms = (f.kernel_stats(3)[1] - before) / steps
    f.set_profiling(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--time", type=float, default=10.0, help="Meep time units per segment")
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    mp.verbosity(0)
    res = 10.0
    kinds = ("none", "point", "point_one", "point_idle", "none_1", "point_1", "plane_none",
             "plane")
    sims = {k: make(a.size, res, k.startswith("plane"), not k.endswith("_1")) for k in kinds}
    ldos = {k: mp.Ldos(0.15, 0.1, NFREQ)
            for k in ("point", "point_one", "point_idle", "point_1", "plane")}
    ldos["point_idle"]._attach(sims["point_idle"])  # added, never used
    ms = {k: [] for k in kinds}
    steps = {k: [] for k in kinds}
    for _ in range(a.segments):
        for k, sim in sims.items():
            t_before = sim.timestep
            t0 = time.perf_counter()
            if k in ("none", "plane_none", "point_idle", "none_1"):
                # the batched runner itself, as the dft_ldos runs get it (one fields.step call
                # per segment; run(until=<number>) alone would step in calls of 64, 128, ...)
                sim._run_until_batched([a.time], sim.round_time())
            elif k == "point_one":
                sim.run(mp.dft_ldos(ldos=ldos[k]), noop, until=a.time)
            else:
                sim.run(mp.dft_ldos(ldos=ldos[k]), until=a.time)  # (ends with ldos_data: flushed)
            el = time.perf_counter() - t0
            n = sim.timestep - t_before
            steps[k].append(n)
            ms[k].append(el * 1e3 / n)
    assert len({tuple(v) for v in steps.values()}) == 1, steps
    m = {k: statistics.median(v) for k, v in ms.items()}
    out = {"size": a.size, "nfreq": NFREQ, "time_per_segment": a.time,
           "steps_per_segment": steps["none"][0], "segments": a.segments,
           "batched_runs": {k: sims[k].batched_runs for k in kinds},
           "stepped_in_pairs": {k: bool(sims[k].fields.tb_info()["active"]) for k in kinds},
           "ms_per_step_median": m, "ms_per_step_all": ms,
           "none_spread": (max(ms["none"]) - min(ms["none"])) / m["none"],
           "point_minus_none_ms": m["point"] - m["none"],
           "point_one_minus_none_ms": m["point_one"] - m["none"],
           "point_idle_minus_none_ms": m["point_idle"] - m["none"],
           "point_1_minus_none_1_ms": m["point_1"] - m["none_1"],
           "plane_minus_none_ms": m["plane"] - m["none"],
           "plane_minus_plane_none_ms": m["plane"] - m["plane_none"]}
    # the LDOS objects' own cost: the DFT phase of the same number of steps while they record
    n = steps["none"][0]
    out["dft_phase_ms_per_step"] = {}
    out["points"] = {}
    for k in ("point", "plane"):
        f = sims[k].fields
        h = ldos[k]._attach(sims[k])
        npts = len(f.ldos_points(h)[0])
        f.ldos_record(h, True)
        out["dft_phase_ms_per_step"][k] = dft_ms(f, n)
        f.ldos_record(h, False)
        f.ldos_data(h)
        out["points"][k] = npts
    np_ = out["points"]["plane"]
    out["reduce_bytes_per_flush"] = np_ * (32 * 8 + 4 * (16 + 4))
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
