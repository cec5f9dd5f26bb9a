"""INTEGRATION.md's environment table lists exactly the MNL_* variables the library reads."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"(MNL_[A-Z0-9_]+)"


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _variables_read():
    """Names passed to getenv / env_is in the host sources and read from os.environ in the
    Python package."""
    names = set()
    csrc = os.path.join(ROOT, "meep_nl_amd", "csrc")
    for path in glob.glob(os.path.join(csrc, "*.cpp")) + glob.glob(os.path.join(csrc, "*.hpp")):
        names.update(re.findall(r"\b(?:getenv|env_is)\(\s*\"" + NAME + "\"", _read(path)))
    for path in glob.glob(os.path.join(ROOT, "meep_nl_amd", "*.py")):
        names.update(re.findall(r"os\.environ(?:\.get\(|\[)\s*[\"']" + NAME + "[\"']", _read(path)))
    return names


def _variables_listed():
    """Names in the first column of the table under "## Environment settings"."""
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text.split("## Environment settings", 1)[1].split("\n## ", 1)[0]
    rows = [ln for ln in section.splitlines() if ln.startswith("|")]
    assert len(rows) > 2 and set(rows[1]) <= set("|-: "), "table header not found"
    names = set()
    for row in rows[2:]:
        names.update(re.findall(NAME, row.split("|")[1]))
    return names


def test_env_table_matches_the_code():
    read, listed = _variables_read(), _variables_listed()
    assert len(read) > 10  # the scan found the reads at all
    assert read == listed, (f"read but not in the table: {sorted(read - listed)}; "
                            f"in the table but not read: {sorted(listed - read)}")
