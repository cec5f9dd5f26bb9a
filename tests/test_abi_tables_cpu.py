"""The numbers of the diagnostic ABI are written down twice, as enums in include/meep_nl_amd.h
and as tables in meep_nl_amd/core.py: the two agree, name for name and value for value."""
import os
import re

from meep_nl_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "meep_nl_amd.h"), encoding="utf-8") as f:
        return f.read()


def _enumerators(prefix):
    """[(name in lower case without the prefix, value)] of the header's `PREFIX_NAME = value`
    enumerators, in the order they are written."""
    found = re.findall(r"\b" + prefix + r"_([A-Z0-9_]+)\s*=\s*(-?\d+)\s*[,}/\n]", _header())
    return [(name.lower(), int(value)) for name, value in found]


def _constant(name):
    (value,) = re.findall(r"\b" + name + r"\s*=\s*(\d+)", _header())
    return int(value)


def test_abi_tables_match_the_header():
    sched = _enumerators("MNL_SCHED")
    assert len(sched) >= 13  # the scan found the enum at all
    assert len(dict(sched)) == len(sched) == len(set(v for _, v in sched))
    assert dict(sched) == core.SCHEDULE
    assert set(core.SCHEDULE_INT) <= set(core.SCHEDULE)

    kstat = _enumerators("MNL_KSTAT")
    assert len(kstat) >= 14
    assert dict(kstat) == core.KERNEL_STATS
    n = _constant("MNL_NUM_KSTATS")
    assert sorted(v for _, v in kstat) == list(range(n)) and len(core.KERNEL_STATS) == n

    slots = _enumerators("MNL_TBINFO")
    assert len(slots) >= 14
    assert [v for _, v in slots] == list(range(len(slots)))  # written in slot order
    assert tuple(k for k, _ in slots) == core.TB_INFO_KEYS
    assert _constant("MNL_NUM_TBINFO") == len(core.TB_INFO_KEYS)

    mode = _enumerators("MNL_MODE")
    assert len(mode) >= 6
    ours = {k[len("MODE_"):].lower(): v for k, v in vars(core).items() if k.startswith("MODE_")}
    assert dict(mode) == ours
