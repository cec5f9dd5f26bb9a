"""The algorithmic-byte model behind bench.py's roofline and the diagnostic read-outs beside it
(mnl_stats.cpp: mnl_fields_kernel_stats, mnl_fields_traffic_model, mnl_fields_tb_info,
mnl_fields_mode), pinned to tests/golden/stats_model.json.

The fixture is the product's own output (tools/make_stats_fixture.py), written by the build of
the commit named in it, before the model moved out of mnl_host.cpp.  Every value is a product
of integer counts and small integers held in a double (the bytes per cell of traffic_model one
quotient of two such), so the comparison is exact: a difference is a changed formula, a changed
order of floating-point operations or a changed plan, never rounding noise."""
import ctypes
import json
import os

import pytest

from scenarios import ProductSim
from test_gpu_tb import sc_tb, sc_tb_lorentz

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stats_model.json")
NUM_KSTATS = 14


def _unfused():
    """sc_tb stepped with the fused step forbidden from the first step on: the interior-curl
    bytes of kernel ids 0 / 1 and the unfused branch of traffic_model."""
    p = sc_tb(ProductSim, steps=(), profile=True)
    p._fields().set_fused(False)
    for n in (1, 10):
        p.step(n)
    return p


# 96 x 64 x 80 cells each, stepped as tests/test_gpu_tb.py steps them, profiling on
SCENARIOS = {
    "tb": lambda: sc_tb(ProductSim, profile=True),
    "tb_random_eps": lambda: sc_tb(ProductSim, random_eps=True, profile=True),
    "tb_lorentz": lambda: sc_tb_lorentz(ProductSim, profile=True),
    "tb_lorentz_one_step": lambda: sc_tb_lorentz(ProductSim, schedule=(("tb_pol", 0),),
                                                 profile=True),
    "one_step": lambda: sc_tb(ProductSim, tb=False, profile=True),
    "unfused": _unfused,
}


def cu_count():
    """k_cu_count() of the library (mnl_internal.hpp, namespace mnl): the count its plans use."""
    from meep_nl_amd._lib import lib
    fn = getattr(lib(), "_ZN3mnl10k_cu_countEv")
    fn.restype, fn.argtypes = ctypes.c_int, []
    return int(fn())


def record(f):
    """What the fixture keeps of one stepped Fields."""
    from meep_nl_amd._lib import check, lib
    mode = ctypes.c_int()
    check(lib().mnl_fields_mode(f.h, ctypes.byref(mode)))
    return {"kernel_bytes": [f.kernel_stats(k)[2] for k in range(NUM_KSTATS)],
            "traffic_model": list(f.traffic_model()),
            "tb_info": f.tb_info(),
            "mode": mode.value}


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        fx = json.load(fh)
    cus = cu_count()
    if cus != fx["cu_count"]:  # item and cell counts follow the CU count
        pytest.skip(f"stats_model.json was recorded on a device with {fx['cu_count']} CUs, "
                    f"this one has {cus}: the plans, and so the byte counts, differ")
    return fx


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_stats_model_equals_fixture(fixture, name):
    want = fixture["scenarios"][name]
    got = record(SCENARIOS[name]()._fields())
    bad = []
    for k in range(NUM_KSTATS):
        if got["kernel_bytes"][k] != want["kernel_bytes"][k]:
            bad.append(f"kernel_stats({k}) bytes: {got['kernel_bytes'][k]!r}, "
                       f"fixture {want['kernel_bytes'][k]!r}")
    for i, what in enumerate(("bytes per cell", "cells")):
        if got["traffic_model"][i] != want["traffic_model"][i]:
            bad.append(f"traffic_model {what}: {got['traffic_model'][i]!r}, "
                       f"fixture {want['traffic_model'][i]!r}")
    assert list(got["tb_info"]) == list(want["tb_info"]), "tb_info keys"
    for key, v in want["tb_info"].items():
        if got["tb_info"][key] != v or type(got["tb_info"][key]) is not type(v):
            bad.append(f"tb_info[{key!r}]: {got['tb_info'][key]!r}, fixture {v!r}")
    if got["mode"] != want["mode"]:
        bad.append(f"mode word: {got['mode']:#x}, fixture {want['mode']:#x}")
    assert not bad, f"scenario {name}: " + "; ".join(bad)
