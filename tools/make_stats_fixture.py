"""The fixture of tests/test_gpu_stats_model.py: the algorithmic-byte model and the diagnostic
read-outs of the build in this tree, for the six scenarios of that test.

For each scenario (tests/test_gpu_stats_model.SCENARIOS: the 96 x 64 x 80 grids of
tests/test_gpu_tb.py, profiling on, stepped as their tests step them) the bytes per launch of
kernel_stats(0 .. 13), traffic_model(), the tb_info() dict and the raw mnl_fields_mode word are
written to tests/golden/stats_model.json, with the CU count of the device (plans, and so cell
counts, follow it) and the commit of the build.  Run it on the build whose numbers are to be
kept -- before a change to the model, not after:

  python tools/make_stats_fixture.py [commit]
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_gpu_stats_model as m
    from meep_nl_amd import core
    core.set_verbosity(0)
    if len(sys.argv) > 1:
        commit = sys.argv[1]
    else:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True,
                                capture_output=True, text=True).stdout.strip()
    out = {"commit": commit, "cu_count": m.cu_count(), "scenarios": {}}
    for name, run in m.SCENARIOS.items():
        out["scenarios"][name] = m.record(run()._fields())
        print(f"{name}: {out['scenarios'][name]}", flush=True)
    with open(m.FIXTURE, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(f"-> {os.path.relpath(m.FIXTURE, ROOT)}", flush=True)


if __name__ == "__main__":
    main()
