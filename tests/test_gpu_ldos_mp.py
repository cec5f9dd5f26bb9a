"""LDOS over the IPC transport: two processes, one z-slab each, as
tests/test_gpu_mp.py runs the distributed path.  F is summed over the ranks by ldos_data; each
rank's partial F is a sub-sum of the one-rank sum, so the bound is the accumulation bound of
tests/test_gpu_ldos.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_ldos as T
from scenarios import ProductSim, make_oracle

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

HERE = os.path.dirname(os.path.abspath(__file__))


def test_ldos_two_processes_ipc(tmp_path):
    from meep_nl_amd import core
    nranks = 2
    nid = core.ipc_id(nranks).hex()
    env = dict(os.environ, MNL_IPC_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "ldos_mp_worker.py"),
                               str(r), str(nranks), nid, str(tmp_path)], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(nranks)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=400)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o or "")
    for p, o in zip(procs, logs):
        assert p.returncode == 0, o[-3000:]
    ranks = [dict(np.load(os.path.join(tmp_path, f"ldos.rank{r}.npz"))) for r in range(nranks)]
    assert all(str(r["transport"]) == "ipc" for r in ranks)
    assert all(int(r["t"][0]) == T.STEPS for r in ranks)
    for k in ("ldos", "F", "J", "scale", "comp", "ijk", "amp"):  # collective: the same everywhere
        assert np.array_equal(ranks[1][k], ranks[0][k]), k
    one = T._cell(ProductSim, 3, T.BOX3, T._src_xz_plane)
    h = T._add(one)
    points = one._fields().ldos_points(h)
    for x, y in zip(points, (ranks[0]["comp"], ranks[0]["ijk"], ranks[0]["amp"])):
        assert np.array_equal(x, y)
    ref = T._restate(T._cell(make_oracle, 3, T.BOX3, T._src_xz_plane), 3, points, T._pulse)
    r = ranks[0]
    T._check((r["ldos"], r["F"], r["J"], float(r["scale"][0])), ref, "2 processes")
