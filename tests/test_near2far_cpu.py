"""CPU checks of the near2far Python layer: the get_farfields grid and the flux assembly
(dft_near2far::get_farfields_array / flux, src/near2far.cpp:400-554) against a stub fields
object that returns a known analytic field, the argument forms of Near2FarRegion /
add_near2far, and the four C-ABI entries in the header and the ctypes table."""
import math
import os
import re

import numpy as np
import pytest

import meep_nl_amd as mp
from meep_nl_amd import simulation as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mnl_fields_add_dft_near2far", "mnl_fields_near2far_farfields",
       "mnl_fields_near2far_medium", "mnl_fields_near2far_points"]


def analytic(p, freqs):
    """(npts, nfreq, 6) complex: a smooth field that tells components, points and
    frequencies apart."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.zeros((len(p), len(freqs), 6), dtype=complex)
    for i, f in enumerate(freqs):
        for k in range(6):
            out[:, i, k] = (1 + k) * np.cos(f * x) + 1j * (2 + k) * y * f + (k - 2.5) * z * z
    return out


class StubFields:
    def __init__(self):
        self.calls = []
        self.added = []

    def add_dft_near2far(self, regs, freqs, decimation, nperiods):
        self.added.append((regs, list(freqs), decimation, nperiods))
        return 7

    def near2far_farfields(self, h, pts):
        pts = np.asarray(pts, dtype=float).reshape(-1, 3)
        self.calls.append((h, pts.copy()))
        return analytic(pts, self.freqs)

    def near2far_medium(self, h):
        return 2.0, 1.0


def stub_sim(freqs):
    sim = mp.Simulation(cell_size=mp.Vector3(4, 4, 4), resolution=10)
    sim.fields = StubFields()
    sim.fields.freqs = list(freqs)
    sim.init_sim = lambda: None  # the stub stands for initialised fields
    return sim


def test_region_and_add_near2far_argument_forms():
    r = mp.Near2FarRegion(center=mp.Vector3(0.5), size=mp.Vector3(0, 1, 2), weight=-1.0)
    assert r.direction == mp.AUTOMATIC and r.weight == -1.0
    sim = stub_sim([0.0])
    n2f = sim.add_near2far(0.3, 0.2, 5, r, mp.Near2FarRegion(mp.Vector3(z=-1), size=mp.Vector3(1, 1),
                                                             direction=mp.Z, weight=0.5),
                           nperiods=1, decimation_factor=3)
    assert isinstance(n2f, mp.DftNear2Far) and n2f.handle == 7 and n2f in sim.dft_objects
    regs, freqs, dec, nper = sim.fields.added[0]
    np.testing.assert_allclose(freqs, np.linspace(0.2, 0.4, 5))
    assert mp.get_near2far_freqs(n2f) == freqs and n2f.nfreqs == 5
    assert (dec, nper) == (3, 1)
    assert regs[0] == ([0.5, -0.5, -1.0], [0.5, 0.5, 1.0], 0, -1.0)  # AUTOMATIC -> the x normal
    assert regs[1] == ([-0.5, -0.5, -1.0], [0.5, 0.5, -1.0], 2, 0.5)
    assert (n2f.eps, n2f.mu) == (2.0, 1.0)
    lst = sim.add_near2far([0.1, 0.15], r)  # the frequency-list form
    assert lst.freq == [0.1, 0.15] and sim.fields.added[1][2:] == (0, 1)
    one = sim.add_near2far(0.25, 0, 1, r)
    assert one.freq == [0.25]
    with pytest.raises(RuntimeError, match="normal direction"):
        sim.add_near2far(0.3, 0, 1, mp.Near2FarRegion(mp.Vector3(), size=mp.Vector3(1, 1, 1)))
    with pytest.raises(TypeError):
        sim.add_near2far("0.3", r)


@pytest.mark.parametrize("nfreq", [1, 3])
def test_get_farfields_grid(nfreq):
    freqs = [0.2, 0.3, 0.45][:nfreq]
    sim = stub_sim(freqs)
    n2f = sim.add_near2far(freqs, mp.Near2FarRegion(mp.Vector3(0.5), size=mp.Vector3(0, 1, 1)))
    res = 2.5
    center, size = mp.Vector3(1.0, -2.0, 3.0), mp.Vector3(2.1, 0.0, 0.7)
    out = sim.get_farfields(n2f, res, center=center, size=size)
    # dims = floor(size * res): 5, 0 -> 1, 1 -> 1; dx = 2.1 / 4
    assert len(sim.fields.calls) == 1  # one batched call
    h, pts = sim.fields.calls[0]
    assert h == 7 and pts.shape == (5, 3)
    np.testing.assert_allclose(pts[:, 0], 1.0 - 1.05 + np.arange(5) * (2.1 / 4), rtol=0, atol=1e-15)
    assert np.all(pts[:, 1] == -2.0) and np.all(pts[:, 2] == 3.0 - 0.35)  # the volume's min corner
    want = analytic(pts, freqs)
    assert sorted(out) == ["Ex", "Ey", "Ez", "Hx", "Hy", "Hz"]
    for k, name in enumerate(("Ex", "Ey", "Ez", "Hx", "Hy", "Hz")):
        assert out[name].shape == ((5,) if nfreq == 1 else (5, nfreq))  # singletons collapsed
        np.testing.assert_array_equal(out[name], want[:, :, k].reshape(out[name].shape))
    # a full 3-D grid: x-major point order, frequency the last axis
    vol3 = mp.Volume(center=mp.Vector3(), size=mp.Vector3(1.0, 2.0, 1.5))
    out = sim.get_farfields(n2f, 2.0, where=vol3)
    _, pts = sim.fields.calls[-1]
    assert pts.shape == (2 * 4 * 3, 3)
    assert out["Hy"].shape == ((2, 4, 3) if nfreq == 1 else (2, 4, 3, nfreq))
    want = analytic(pts, freqs)[:, :, 4].reshape(out["Hy"].shape)
    np.testing.assert_array_equal(out["Hy"], want)
    np.testing.assert_allclose(pts[1], [-0.5, -1.0, -0.75 + 0.75], atol=1e-15)  # z fastest
    pt = sim.get_farfield(n2f, mp.Vector3(0.3, 0.2, 0.1))
    assert len(pt) == 6 * nfreq
    np.testing.assert_array_equal(pt, analytic(np.array([[0.3, 0.2, 0.1]]), freqs)[0].ravel())
    with pytest.raises(ValueError):
        sim.get_farfields(n2f, 2.0)


@pytest.mark.parametrize("direction", [0, 1, 2])
def test_flux_assembly(direction):
    freqs = [0.2, 0.37]
    sim = stub_sim(freqs)
    n2f = sim.add_near2far(freqs, mp.Near2FarRegion(mp.Vector3(0.5), size=mp.Vector3(0, 1, 1)))
    size = [1.3, 2.2, 0.9]
    size[direction] = 0.0
    where = mp.Volume(center=mp.Vector3(0.2, -0.1, 0.4), size=mp.Vector3(*size))
    res = 3.0
    got = n2f.flux(direction, where, res)
    _, pts = sim.fields.calls[-1]
    dims = [max(1, int(math.floor(s * res))) for s in size]
    assert len(pts) == int(np.prod(dims))
    eh = analytic(pts, freqs)
    table = {0: ((1, 2), (5, 4)), 1: ((2, 0), (3, 5)), 2: ((0, 1), (4, 3))}  # near2far.cpp:529-533
    ce, ch = table[direction]
    dv = np.prod([s / (n - 1) for s, n in zip(size, dims) if n > 1])
    for i in range(len(freqs)):
        want = 0.0
        for j in range(2):
            want += np.sum((eh[:, i, ce[j]] * np.conj(eh[:, i, ch[j]])).real) * (1 - 2 * j)
        assert got[i] == pytest.approx(want * dv, rel=1e-13)
    assert isinstance(got, list) and len(got) == len(freqs)


def test_abi_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "meep_nl_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = open(os.path.join(ROOT, "meep_nl_amd", "_lib.py")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*mnl_fields\s*\*", code), name
        assert f'"{name}"' in lib, name
    for name in NEW[:2]:  # the entries with a reference counterpart cite it
        doc = hdr[:hdr.index("int " + name)]
        assert "src/near2far.cpp" in doc[doc.rindex("/*"):], name
    assert re.search(r"mnl_fields_add_dft_near2far\([^)]*int nperiods,\s*int \*handle\)", code)
    assert re.search(r"mnl_fields_near2far_farfields\([^)]*long long npts,\s*const double \*xyz,"
                     r"\s*double \*out\)", code)
    from meep_nl_amd import _lib
    for name in NEW:
        assert name in _lib.exported_symbols()


def test_farfield_grid_function():
    pts, dims, dx = sm.farfield_grid([0, 0, 0], [0.99, 2.0, 0.0], 2.0)
    assert dims == [1, 4, 1] and dx == [0.0, 2.0 / 3, 0.0]
    np.testing.assert_allclose(pts[:, 1], [0, 2 / 3, 4 / 3, 2.0])
