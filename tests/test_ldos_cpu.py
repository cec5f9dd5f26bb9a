"""LDOS spectra, the checks that need no GPU: the C ABI's entries, the
argument forms of Ldos / dft_ldos / get_ldos_freqs, and the restatement of dft_ldos::update /
ldos() (tests/ldos_ref.py) on a small oracle cell."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from ldos_ref import LdosRef, custom_current
from scenarios import make_oracle, vol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["mnl_fields_add_ldos", "mnl_fields_ldos_update", "mnl_fields_ldos_record",
           "mnl_fields_ldos_data", "mnl_fields_ldos_points", "mnl_fields_remove_ldos",
           "mnl_fields_remove_ldoses"]


def test_abi_entries_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "meep_nl_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
    lib = os.path.join(ROOT, "meep_nl_amd", "libmnl.so")
    if not os.path.exists(lib):
        subprocess.run(["bash", os.path.join(ROOT, "meep_nl_amd", "csrc", "build.sh")], check=True)
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (mnl_\w+)", out))
    assert not [n for n in ENTRIES if n not in exported]
    from meep_nl_amd import _lib, core
    assert not [n for n in ENTRIES if n not in _lib.exported_symbols()]
    for m in ("add_ldos", "ldos_update", "ldos_record", "ldos_data", "ldos_points", "remove_ldos"):
        assert callable(getattr(core.Fields, m)), m
    # what replaces what is written at the declarations
    for what in ("dft_ldos::dft_ldos", "dft_ldos::update", "dft_ldos::ldos()"):
        assert what in hdr, what


def test_ldos_argument_forms():
    import meep_nl_amd as mp
    a = mp.Ldos(1.0, 0.2, 3)
    assert np.allclose(mp.get_ldos_freqs(a), [0.9, 1.0, 1.1])
    assert mp.get_ldos_freqs(mp.Ldos(0.7, 0.2, 1)) == [0.7]
    assert mp.get_ldos_freqs(mp.Ldos(freq=[0.3, 0.5])) == [0.3, 0.5]
    assert mp.get_ldos_freqs(mp.Ldos(np.array([0.25, 0.5]))) == [0.25, 0.5]
    with pytest.raises(TypeError, match="add_dft functions only accept"):
        mp.Ldos("x")
    for step in (mp.dft_ldos(1.0, 0.2, 3), mp.dft_ldos(freq=[0.9, 1.0, 1.1]),
                 mp.dft_ldos([0.9, 1.0, 1.1]), mp.dft_ldos(ldos=a)):
        assert type(step).__name__ == "_DftLdosStep"
        assert np.allclose(mp.get_ldos_freqs(step.ldos), [0.9, 1.0, 1.1])
    assert mp.dft_ldos(ldos=a).ldos is a
    msg = "dft_ldos only accepts freq_min,freq_max,nfreq"
    with pytest.raises(TypeError, match=msg):
        mp.dft_ldos()
    with pytest.raises(TypeError, match=msg):
        mp.dft_ldos((0.9, 1.0))  # a tuple is neither three numbers nor an array / list
    with pytest.raises(TypeError, match="add_dft functions only accept"):
        mp.dft_ldos("x")
    # the step function takes (sim, todo): a run calls it with "finish" too
    from meep_nl_amd.simulation import _num_args
    assert _num_args(mp.dft_ldos(ldos=a)) == 2


def _pulse(t):
    return math.exp(-((t - 2.0) / 0.7) ** 2) * math.cos(2 * math.pi * 0.9 * t)


FREQS = (0.7, 0.9, 1.1)
N, A, STEPS = 24, 10, 60


def _restate(amp):
    """2-D 24 x 24 oracle cell, metal walls, an Ez custom point source at the origin (a grid
    point of Ez): one update before every step and one after the last, as a run does."""
    o = vol(make_oracle, 2, [N / A, N / A], A, center_origin=True)
    o.add_custom_source(2, _pulse, 0.0, 1e9, (0.0, 0.0), amp)
    Apt = complex(amp) * A ** 2  # delta-function units: amp * a^dim (src/sources.cpp:481-484)
    points = (np.array([2]), np.array([[N // 2, N // 2, 0]]), np.array([Apt]))
    ref = LdosRef(FREQS, o.dt, A, 2)
    for s in range(STEPS + 1):
        ref.update(o.t, o.get_array, points, 1, custom_current(_pulse, o.t, o.dt))
        if s < STEPS:
            o.step(1)
    return ref, Apt


def test_restatement_point_dipole_2d():
    r1, A1 = _restate(0.8)
    assert A1 == 80.0
    assert math.isclose(r1.Jsum, abs(A1) * math.sqrt((1.0 / A) ** 2), rel_tol=4 * 2.0 ** -52)
    assert math.isclose(r1.overall_scale(), -2.0 / math.pi / r1.Jsum ** 2, rel_tol=4 * 2.0 ** -52)
    ld = r1.ldos()
    assert np.all(np.isfinite(ld)) and np.all(np.abs(r1.F()) > 0) and np.all(np.abs(r1.J()) > 0)
    # the field is linear in the amplitude and F carries one more factor conj(A): F scales by
    # 3^2, J does not change, Jsum scales by 3 and ldos is invariant
    r3, A3 = _restate(2.4)
    assert math.isclose(abs(A3), 3 * abs(A1), rel_tol=2.0 ** -51)
    assert np.array_equal(r3.J(), r1.J())
    tolF = r3.tol_F() + 9 * r1.tol_F()
    assert np.all(np.abs(r3.F() - 9 * r1.F()) <= tolF), (r3.F() - 9 * r1.F(), tolF)
    tol = r1.tol_ldos() + r3.tol_ldos()
    assert np.all(np.abs(r3.ldos() - ld) <= tol), (r3.ldos() - ld, tol)
    assert np.all(tol < 1e-9 * np.abs(ld))  # (the bound is tight enough to mean something)


def test_ldos_before_any_update_is_nan():
    ref = LdosRef(FREQS, 0.05, A, 2)
    assert ref.Jsum == 1.0 and np.all(np.isnan(ref.ldos()))
