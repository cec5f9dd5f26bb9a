"""bench.py as it is run for every change: a plain single-GPU run carries the headline figure
alone (everything else waits for --full), --steps sets the timed steps, and --dump-outputs
writes the same arrays from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--size",
                        "64", "--warmup", "2"] + list(args),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines  # stdout carries the one JSON line
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_repeatably(tmp_path):
    from meep_nl_amd import core
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    line = _bench("--steps", "6", "--dump-outputs", d1)
    assert line["steps"] == 6 and line["warmup"] == 2 and line["full"] is False
    assert line["unit"] == "Mcells*steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0
    # value and ms_per_step say the same thing: all cells x steps over the timed region
    assert line["value"] == pytest.approx(64 ** 3 / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-2)
    for key in ("cpu_baseline", "configs", "c5_parity", "c5_parity_check"):
        assert line[key] is None, key
    assert line["gpu_state"] == {"while_stepping": None, "after": None}
    _bench("--steps", "6", "--dump-outputs", d2)
    names = sorted(os.listdir(d1))
    assert names == sorted(f"{n}_{k}.npy" for n in core.COMPONENT_NAMES
                           for k in ("center", "sample")) == sorted(os.listdir(d2))
    moved = 0
    for n in names:
        a, b = np.load(os.path.join(d1, n)), np.load(os.path.join(d2, n))
        assert a.dtype == np.float64 and np.isfinite(a).all()
        assert np.array_equal(a, b), n
        moved += int(np.count_nonzero(a))
    assert moved > 0  # 2 + 6 steps of the Ez source have reached the centre block
    # two more timed steps: other arrays (--steps is the number of steps really taken)
    d3 = str(tmp_path / "c")
    line8 = _bench("--steps", "8", "--dump-outputs", d3)
    assert line8["steps"] == 8
    assert not np.array_equal(np.load(os.path.join(d1, "ez_center.npy")),
                              np.load(os.path.join(d3, "ez_center.npy")))
