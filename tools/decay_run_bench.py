#!/usr/bin/env python3
"""Cost of a decay-stopped run: configuration C2 (a 256^3 vacuum cell
with PML and a point source) with one flux plane, run through Simulation.run with
stop_when_fields_decayed three ways in one process --

    one_step   the one-step loop (what every condition function got before the batched loop),
               forced by a no-op step function: one fields.step(1) and one get_field per step
    batched    the batched loop: one fields.step(n) per check interval, the values from a probe
    until      until=<the same time>: no condition at all

Each segment runs the same number of steps in each of the three (the condition's decay_by is 0,
so it never holds and the number ends the run); segments alternate, so drift and allocation
placement hit them alike, and medians are reported.  until's spread over its segments is the
run-to-run spread to hold a difference against.

probe_ms_per_step is the DFT phase of the library's HIP-event timers (sampling and flush
launches) per step with the probe, against the same steps without it.

    python tools/decay_run_bench.py --size 256 --segments 7 --out profiles/decay_runs/c2_256.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import meep_nl_amd as mp  # noqa: E402


def noop(sim):
    pass


def watch_pairs(fields, seen):
    """seen: tb_info()["active"] right after every fields.step call of at least two steps"""
    orig = fields.step

    def step(n=1):
        r = orig(n)
        if int(n) >= 2:
            seen.append(bool(fields.tb_info()["active"]))
        return r
    fields.step = step


def make(size, res):
    L = size / res
    sim = mp.Simulation(cell_size=mp.Vector3(L, L, L), resolution=res,
                        boundary_layers=[mp.PML(1.0)],
                        sources=[mp.Source(mp.ContinuousSource(0.15), component=mp.Ez,
                                           center=mp.Vector3(0.05, 0.05, 0.05))])
    sim.add_flux(0.15, 0.1, 5, mp.FluxRegion(center=mp.Vector3(0, 0, 0.25 * L),
                                             size=mp.Vector3(0.5 * L, 0.5 * L, 0)))
    sim.fields.step(4)  # past the first (lazy-copy) step and the mode switch
    return sim


def dft_ms(f, steps):
    f.set_profiling(True)
    before = f.kernel_stats(3)[1]
    f.step(steps)
    f.dft_flush()
    ms = (f.kernel_stats(3)[1] - before) / steps
    f.set_profiling(False)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--time", type=float, default=10.0, help="Meep time units per segment")
    ap.add_argument("--check", type=float, default=5.0, help="the condition's dt")
    ap.add_argument("--segments", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    mp.verbosity(0)
    res = 10.0
    pt = mp.Vector3(0.513, -0.287, 0.731)
    sims = {k: make(a.size, res) for k in ("one_step", "batched", "until")}
    conds = {k: mp.stop_when_fields_decayed(a.check, mp.Ez, pt, 0.0) for k in sims}
    ms = {k: [] for k in sims}
    pairs = {k: [] for k in sims}
    for k, sim in sims.items():  # (after make's warm-up call)
        watch_pairs(sim.fields, pairs[k])
    steps = {k: [] for k in sims}
    for _ in range(a.segments):
        for k, sim in sims.items():
            t_before = sim.timestep
            t0 = time.perf_counter()
            if k == "one_step":
                sim.run(noop, until=[a.time, conds[k]])
            elif k == "batched":
                sim.run(until=[a.time, conds[k]])
            else:
                sim.run(until=a.time)
            sim.fields.dft_flush()  # every run ends with its DFT updates accumulated
            el = time.perf_counter() - t0
            n = sim.timestep - t_before
            steps[k].append(n)
            ms[k].append(el * 1e3 / n)
    assert steps["one_step"] == steps["batched"] == steps["until"], steps
    out = {"size": a.size, "time_per_segment": a.time, "check_interval": a.check,
           "steps_per_segment": steps["until"][0], "segments": a.segments,
           # whether the step calls of at least two steps inside the runs stepped in pairs
           # (None: the run made no such call)
           "stepped_in_pairs": {k: (all(v) if v else None) for k, v in pairs.items()},
           "ms_per_step_median": {k: statistics.median(v) for k, v in ms.items()},
           "ms_per_step_all": ms}
    m = out["ms_per_step_median"]
    out["until_spread"] = (max(ms["until"]) - min(ms["until"])) / m["until"]
    out["batched_over_one_step"] = m["batched"] / m["one_step"]
    out["batched_over_until"] = m["batched"] / m["until"]
    # the probe's own cost: the DFT phase with and without it, the same steps of the same run
    f = sims["until"].fields
    n = steps["until"][0]
    without = dft_ms(f, n)
    h = f.add_probe(mp.Ez, tuple(pt))
    with_probe = dft_ms(f, n)
    f.remove_probe(h)
    out["dft_phase_ms_per_step"] = {"flux_plane": without, "flux_plane_and_probe": with_probe}
    out["probe_ms_per_step"] = with_probe - without
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
