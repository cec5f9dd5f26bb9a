"""CPU checks of the decay conditions and the batched run loop on a stub
`fields`: the batched loop stops after the same step and leaves the conditions in the same
state as the one-step loop, with one fields.step call per check interval instead of one per
step; stop_when_dft_decayed / stop_when_energy_decayed against a step-by-step model of what the
reference's conditions do; the new C-ABI entries; the fallbacks to the one-step loop."""
import math
import os
import re

import numpy as np
import pytest

import meep_nl_amd as mp
from meep_nl_amd import simulation as msim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class StubFields:
    """t / dt / round_time of its own, a value per step for get_field and the probes, a
    dft_norm per step, and counters."""
    rank = 0

    def __init__(self, value, dt=0.05, t=0, norm=None, maxfreq=0.4, maxdec=1, last_source=0.0):
        self.value, self.norm = value, norm
        self.dt, self.t = dt, t
        self.maxfreq, self.maxdec, self.last_source = maxfreq, maxdec, last_source
        self.step_calls = self.get_field_calls = self.norm_calls = 0
        self.probes = {}

    def step(self, n=1):
        self.step_calls += 1
        for _ in range(int(n)):
            self.t += 1
            for series in self.probes.values():
                series.append((self.t, self.value(self.t)))

    def time(self):
        return self.t * self.dt

    def round_time(self):
        return float(np.float32(self.t * self.dt))

    def last_source_time(self):
        return self.last_source

    def get_field(self, c, pt):
        self.get_field_calls += 1
        return self.value(self.t)

    def add_probe(self, c, pt):
        h = (1 << 30) + len(self.probes)
        self.probes[h] = []
        return h

    def probe_read(self, h):
        s, self.probes[h] = self.probes[h], []
        return (s[0][0] if s else self.t + 1), np.array([v for _, v in s])

    def remove_probe(self, h):
        del self.probes[h]

    def dft_norm(self):
        self.norm_calls += 1
        return self.norm(self.t)

    def dft_maxfreq(self):
        return self.maxfreq

    def max_decimation(self):
        return self.maxdec


class StubSim(mp.Simulation):
    def __init__(self, fields, energy=None):
        self.fields = fields
        self.energy = energy
        self.energy_calls = 0
        self.progress_interval = 1e9
        self.run_index = 0
        self.cell_size = mp.Vector3(1, 1, 1)

    def init_sim(self):
        pass

    def field_energy_in_box(self, box=None, center=None, size=None):
        self.energy_calls += 1
        return self.energy(self.fields.t)


@pytest.fixture(autouse=True)
def _quiet():
    old = mp.verbosity.get()
    mp.verbosity(0)
    yield
    mp.verbosity(old)


def noop(sim):
    pass


SEQS = {
    "decaying": lambda t: math.exp(-t / 150.0) * math.cos(0.31 * t),
    "revival": lambda t: (math.exp(-t / 90.0) + 0.8 * math.exp(-((t - 900) / 60.0) ** 2))
    * math.cos(0.29 * t),
    "zero": lambda t: 0.0,
}


def run_kind(kind, cond, sim, step_funcs):
    if kind == "until":
        sim.run(*step_funcs, until=cond)
    elif kind == "after_sources":
        sim.run(*step_funcs, until_after_sources=cond)
    elif kind == "until_list":
        sim.run(*step_funcs, until=[40, cond])
    elif kind == "until_list_first":
        sim.run(*step_funcs, until=[cond, 1e4])
    else:
        sim.run(*step_funcs, until_after_sources=[12, cond])


@pytest.mark.parametrize("kind", ["until", "after_sources", "until_list", "until_list_first",
                                  "after_sources_list"])
@pytest.mark.parametrize("seq", sorted(SEQS))
def test_fields_decayed_replay_equivalence(kind, seq):
    for dt_c in (0.05, 1.0, 3.7, 10.0):
        for decay_by in (1e-1, 1e-3, 1e-9):
            out = []
            for step_funcs in ((noop,), ()):
                f = StubFields(SEQS[seq], last_source=23.0)
                sim = StubSim(f)
                cond = mp.stop_when_fields_decayed(dt_c, mp.Ez, mp.Vector3(), decay_by)
                run_kind(kind, cond, sim, step_funcs)
                out.append((f.t, dict(cond.closure), f.step_calls, f.get_field_calls))
                assert not f.probes  # the batched run removed its probe
            (t1, c1, calls1, _), (tb, cb, callsb, gfb) = out
            assert tb == t1, (dt_c, decay_by)
            assert cb == c1, (dt_c, decay_by)
            assert calls1 == t1  # the one-step loop: one call per step
            # batched: one call per check interval (and per number / source end), plus the
            # split of stretches longer than the largest batch
            intervals = math.ceil(t1 * f.dt / dt_c)
            assert callsb <= intervals + 3 + t1 // msim._BATCH_MAX, (dt_c, decay_by, callsb)
            assert gfb == 1  # the starting state through get_field, the rest from the probe


def model_energy(energy, dt_step, t_start, dt_c, decay_by, max_steps=10 ** 6):
    """Step by step what the reference's stop_when_energy_decayed does: every state looks at
    the clock; past t0 + dt it reads the energy, updates the maximum and t0, and compares."""
    t, t0, max_abs, reads = t_start, 0, 0, 0
    while t - t_start < max_steps:
        rt = float(np.float32(t * dt_step))
        if rt > dt_c + t0:
            cur = abs(energy(t))
            reads += 1
            max_abs = max(max_abs, cur)
            t0 = rt
            if cur <= max_abs * decay_by:
                break
        t += 1
    return t, {"max_abs": max_abs, "t0": t0}, reads


@pytest.mark.parametrize("t_start", [0, 7])
def test_energy_decayed_matches_the_model(t_start):
    energy = lambda t: 3.0 * math.exp(-t / 200.0) * (1 + 0.3 * math.sin(0.1 * t))  # noqa: E731
    for dt_c in (0.5, 2.0, 11.0):
        for decay_by in (1e-2, 1e-5):
            want = model_energy(energy, 0.05, t_start, dt_c, decay_by)
            for step_funcs in ((noop,), ()):
                f = StubFields(SEQS["zero"], t=t_start)
                sim = StubSim(f, energy)
                cond = mp.stop_when_energy_decayed(dt_c, decay_by)
                sim.run(*step_funcs, until=cond)
                assert (f.t, cond.closure, sim.energy_calls) == want
                if not step_funcs:
                    assert f.step_calls <= want[2] + 1
                else:
                    assert f.step_calls == f.t - t_start


def model_dft(norm, dt_step, t_start, maxfreq, maxdec, tol, tmin, tmax, max_steps=10 ** 6):
    """Step by step what the reference's stop_when_dft_decayed does.  The interval is set only
    when a state with t == 0 is looked at (otherwise it stays 0: a check at every state)."""
    t, t0, interval, prev, maxchange = t_start, 0, 0, 0, 0
    while t - t_start < max_steps:
        rt = float(np.float32(t * dt_step))
        if t == 0:
            interval = max(1 / maxfreq / dt_step, maxdec)
        if tmax and rt > tmax:
            break
        if t > interval + t0:
            cur = norm(t)
            change = abs(prev - cur)
            maxchange = max(maxchange, change)
            was = prev
            prev = cur
            if was != 0:
                t0 = t
                if change / maxchange <= tol and rt >= tmin:
                    break
        t += 1
    return t, {"previous_fields": prev, "t0": t0, "dt": interval, "maxchange": maxchange}


@pytest.mark.parametrize("t_start,tmin,tmax,maxdec", [(0, 0, None, 1), (0, 60.0, None, 1),
                                                      (0, 0, 31.0, 1), (5, 0, None, 1),
                                                      (0, 0, None, 90), (5, 0, 12.0, 3)])
def test_dft_decayed_matches_the_model(t_start, tmin, tmax, maxdec):
    norm = lambda t: 2.0 * (1 - math.exp(-t / 120.0))  # noqa: E731  (a DFT that converges)
    for tol in (1e-3, 1e-7):
        want = model_dft(norm, 0.05, t_start, 0.4, maxdec, tol, tmin, tmax)
        for step_funcs in ((noop,), ()):
            f = StubFields(SEQS["zero"], t=t_start, norm=norm, maxfreq=0.4, maxdec=maxdec)
            sim = StubSim(f)
            cond = mp.stop_when_dft_decayed(tol, tmin, tmax)
            sim.run(*step_funcs, until=cond)
            assert (f.t, cond.closure) == want
            if not step_funcs and t_start == 0:  # (interval 0 otherwise: a check every step)
                assert f.step_calls <= f.norm_calls + 2


def test_conditions_reject_missing_arguments():
    with pytest.raises(ValueError):
        mp.stop_when_energy_decayed(dt=1.0)
    with pytest.raises(ValueError):
        mp.stop_when_fields_decayed(1.0, mp.Ez, None, 1e-3)


def test_step_functions_and_plain_callables_select_the_one_step_loop():
    def plain(sim):
        return sim.fields.t >= 50

    cases = [((noop,), mp.stop_when_fields_decayed(1.0, mp.Ez, mp.Vector3(), 1e-3)),
             ((), plain),
             ((), [mp.stop_when_fields_decayed(1.0, mp.Ez, mp.Vector3(), 1e-3), plain])]
    for step_funcs, cond in cases:
        f = StubFields(SEQS["decaying"])
        sim = StubSim(f)
        sim.run(*step_funcs, until=cond)
        assert f.step_calls == f.t > 0
        assert not f.probes
    # through until_after_sources a plain callable stays plain
    f = StubFields(SEQS["decaying"], last_source=1.0)
    StubSim(f).run(until_after_sources=plain)
    assert f.step_calls == f.t == 50


def test_per_step_call_is_unchanged():
    """cond(sim) one state at a time: one get_field per call, the closure's three entries."""
    f = StubFields(SEQS["decaying"])
    sim = StubSim(f)
    cond = mp.stop_when_fields_decayed(1.0, mp.Ez, mp.Vector3(), 1e-3)
    cur = 0.0
    for _ in range(20):
        assert cond(sim) is False
        cur = max(cur, SEQS["decaying"](f.t) ** 2)
        f.step(1)
    assert f.get_field_calls == 20 and cond.closure == {"max_abs": 0, "cur_max": cur, "t0": 0}
    f.step(1)  # the first state past t0 + dt
    assert cond(sim) is False and cond.closure["t0"] == f.round_time()
    assert cond.closure["cur_max"] == 0 and cond.closure["max_abs"] > 0


NEW_ENTRIES = ["mnl_fields_add_probe", "mnl_fields_probe_read", "mnl_fields_probe_reset",
               "mnl_fields_remove_probe", "mnl_fields_remove_probes", "mnl_fields_dft_norm",
               "mnl_fields_dft_maxfreq", "mnl_fields_max_decimation"]


def test_new_abi_entries_are_declared_and_bound():
    from meep_nl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "meep_nl_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*mnl_fields\s*\*", code), name
        assert name in _lib.exported_symbols(), name
    # each cites the reference API it stands for
    assert "fields::get_field" in hdr and "src/monitor.cpp" in hdr
    assert "fields::dft_norm" in hdr and "fields::max_decimation" in hdr
    for name in ("add_probe", "probe_read", "remove_probes", "dft_norm", "dft_maxfreq",
                 "max_decimation"):
        assert callable(getattr(mp.core.Fields, name))
