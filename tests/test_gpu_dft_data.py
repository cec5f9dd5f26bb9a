"""get / load / scale / save of the DFT data of flux, dft-fields and near2far objects
(save_dft_hdf5 / load_dft_hdf5 / dft_chunk::scale_dft, src/dft.cpp:401-496; Python
get_flux_data / load_minus_flux_data / scale_flux_fields) on the GPU.

Every comparison is bitwise unless it says otherwise:
  * the gather (dft_get) against mnl_fields_dft_data's host permutation and against the oracle;
  * the scatter (dft_load) by reading back, and through flux(), which sums the loaded values;
  * the scale against re = a c - b d, im = a d + b c with every product and sum rounded once --
    std::complex<double>::operator*= on finite values (libgcc's __muldc3), stated here with real
    numpy arrays.  numpy's own complex128 product contracts one product of each pair into a
    fused multiply-add on hosts with AVX-512, so `d * s` is compared only for the scale factors
    whose products are exact (2, -1, 1j);
  * subtraction (load with sign -1, then a run): 2 U 2^-53 M per real and imaginary part, the
    reassociation bound of two sums of U terms (U updates, M the largest magnitude the list
    reaches in either oracle run at any step).
Per-slab results: every point has one owner, so the sum over the slabs is exact.
"""
import numpy as np
import pytest

from scenarios import (E_COMPS, GroupSim, GroupSim3, ProductSim, flux_box_faces, make_oracle,
                       sc_dft_fields_3d, sc_flux_2d, sc_flux_3d, vol)
import test_gpu_near2far as n2f

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]
FREQS = [0.1, 0.15, 0.2, 0.27]  # scenarios.FLUX3D_FREQS
STEPS = 80


def fields_of(p):
    return p._all() if hasattr(p, "_all") else [p._fields()]


def get_sum(p, h, which):
    return sum(f.dft_get(h, which) for f in fields_of(p))


def load_all(p, h, which, d, sign=1):
    for f in fields_of(p):
        f.dft_load(h, which, d, sign)


def flux_build(make, block=False, freqs=FREQS):
    """sc_flux_3d's set-up, not stepped; block: an extra eps = 6 block beside the guide."""
    o = vol(make, 3, [3.2, 3.2, 3.2], 10, center_origin=True)
    o.add_pml(1.0)
    for c in E_COMPS:
        x, y, z = o.coords(c)
        inv = np.where((np.abs(y) < 0.5) & (np.abs(z) < 0.5), 1 / 12.0, 1.0)
        if block:
            inv = np.where((np.abs(x - 0.2) < 0.4) & (y >= 0.5) & (y < 1.0) & (np.abs(z) < 0.4),
                           1 / 6.0, inv)
        o.set_chi1inv(c, c, inv)
    o.add_gaussian_source(2, 0.15, 10.0, 0.0, 100.0, (0.05, 0.05, 0.05), 1.0)
    o.add_gaussian_source(1, 0.2, 6.0, 0.0, 60.0, (-0.33, 0.12, 0.41), 0.7)
    hx = hy = hz = 0.5 * 3.2
    hs = [o.add_dft_flux(flux_box_faces([-0.42, -0.37, -0.33], [0.44, 0.51, 0.38], 3), freqs, 1),
          o.add_dft_flux([([0.83, -hy, -hz], [0.83, hy, hz], 0, 1.0)], freqs, 1),
          o.add_dft_flux([([-hx + 0.1, -hy + 0.3, -hz + 0.35], [hx - 0.2, hy - 0.1, -hz + 0.35],
                           2, -0.5)], freqs, 1),
          o.add_dft_flux([([-0.61, -0.23, -0.17], [0.57, 0.29, 0.66], 1, 1.0)], freqs, 0)]
    return o, hs


class OracleRun:
    """One oracle run stepped one step at a time: the data of every list after every step."""

    def __init__(self, block):
        o, self.hs = flux_build(make_oracle, block)
        self.data = [{(h, w): o.dft_data(h, w) for h in self.hs for w in (0, 1)}]
        self.flux = {}
        for t in range(1, STEPS + 1):
            o.step(1)
            self.data.append({(h, w): o.dft_data(h, w) for h in self.hs for w in (0, 1)})
            if t in (5, STEPS):
                self.flux[t] = [o.flux(h) for h in self.hs]
        self.decim = [o.dft_decimation(h) for h in self.hs]

    def peak(self, h, w):
        return max(float(np.max(np.abs(d[(h, w)]))) for d in self.data)


@pytest.fixture(scope="module")
def run1():
    return OracleRun(False)


@pytest.fixture(scope="module")
def run2():
    return OracleRun(True)


def test_oracle_run_is_sc_flux_3d(run1):
    """flux_build restates sc_flux_3d: same objects, same values."""
    o, hs = sc_flux_3d(make_oracle, steps=STEPS)
    assert hs == run1.hs
    for h in hs:
        for w in (0, 1):
            np.testing.assert_array_equal(o.dft_data(h, w), run1.data[STEPS][(h, w)])
    # padded tails of the last 64-slot block
    assert sum((run1.data[STEPS][(h, 0)].size // len(FREQS)) % 64 != 0 for h in hs) >= 2


# ------------------------------------------------------------------ 1. gather
_ORACLE_NF = {}


def oracle_nfreq(nfreq):
    if nfreq not in _ORACLE_NF:
        o, hs = sc_flux_3d(make_oracle, freqs=list(np.linspace(0.05, 0.3, nfreq)), steps=40)
        _ORACLE_NF[nfreq] = {(h, w): o.dft_data(h, w) for h in hs for w in (0, 1)}
    return _ORACLE_NF[nfreq]


@pytest.mark.parametrize("make", [ProductSim, GroupSim, GroupSim3])
@pytest.mark.parametrize("nfreq", [1, 21, 40])
def test_gather(make, nfreq):
    """dft_get = dft_data = the oracle, both lists of the four objects; full and partial
    frequency tiles (8 per tile).  On slabs: per slab dft_get = dft_data (0 at the other
    ranks' points, which are never accumulated), no point is non-zero on two slabs, and the
    slabs' sum is the oracle's list."""
    ref = oracle_nfreq(nfreq)
    p, hs = sc_flux_3d(make, freqs=list(np.linspace(0.05, 0.3, nfreq)), steps=40)
    for h in hs:
        for w in (0, 1):
            got = [f.dft_get(h, w) for f in fields_of(p)]
            for f, g in zip(fields_of(p), got):
                assert g.dtype == np.complex128 and g.shape == ref[(h, w)].shape
                np.testing.assert_array_equal(g, f.dft_data(h, w))
            assert np.max(sum((g != 0).astype(int) for g in got)) <= 1
            assert np.any(ref[(h, w)] != 0) or h == hs[3]  # (its decimation can exceed the run)
            np.testing.assert_array_equal(sum(got), ref[(h, w)], err_msg=f"object {h} list {w}")
            if h == hs[1]:  # the plane across the whole cell has points on every slab
                assert all(np.any(g != 0) for g in got)


def test_gather_2d():
    p, h1, h2 = sc_flux_2d(ProductSim, ttot=10.0)
    o, _, _ = sc_flux_2d(make_oracle, ttot=10.0)
    for h in (h1, h2):
        for w in (0, 1):
            ref = o.dft_data(h, w)
            assert np.any(ref != 0)
            np.testing.assert_array_equal(p._fields().dft_get(h, w), ref)
            np.testing.assert_array_equal(p.dft_data(h, w), ref)


# ------------------------------------------------------------------ 2. scatter
@pytest.mark.parametrize("make", [ProductSim, GroupSim])
def test_scatter(run1, make):
    p, hs = flux_build(make)
    d = run1.data[STEPS]
    for h in hs:
        for w in (0, 1):
            load_all(p, h, w, d[(h, w)])
    for h in hs:
        for w in (0, 1):
            np.testing.assert_array_equal(get_sum(p, h, w), d[(h, w)])
            np.testing.assert_array_equal(p.dft_data(h, w), d[(h, w)])
    if make is ProductSim:  # flux() sums in list order on one GPU: the oracle's bits
        for h, fo in zip(hs, run1.flux[STEPS]):
            np.testing.assert_array_equal(p.flux(h), fo)
    else:
        for h, fo in zip(hs, run1.flux[STEPS]):
            np.testing.assert_allclose(p.flux(h), fo, rtol=1e-12, atol=1e-300)
    for h in hs:
        load_all(p, h, 0, d[(h, 0)], -1)
        np.testing.assert_array_equal(get_sum(p, h, 0), -d[(h, 0)])
        np.testing.assert_array_equal(get_sum(p, h, 1), d[(h, 1)])  # the other list is untouched


def test_scatter_wrong_size(run1):
    p, hs = flux_build(ProductSim)
    f = p._fields()
    d = run1.data[STEPS][(hs[1], 0)]
    with pytest.raises(RuntimeError, match=r"meep:.*incorrect dataset size \(%d vs\. %d\)"
                       % (2 * d.size - 2, 2 * d.size)):
        f.dft_load(hs[1], 0, d[:-1])
    with pytest.raises(RuntimeError, match=r"meep:.*incorrect dataset size"):
        f.dft_load(hs[1], 1, np.concatenate([d, d]))
    with pytest.raises(RuntimeError, match="meep:.*sign"):
        f.dft_load(hs[1], 0, d, 2)
    with pytest.raises(RuntimeError, match="meep:.*bad dft handle"):
        f.dft_get(17, 0)
    assert not np.any(f.dft_get(hs[1], 0))  # a refused load changes nothing


# ------------------------------------------------------------------ 3. scale
def cmul(d, s):
    """std::complex<double>::operator*= on finite values: four products and two sums, each
    rounded once (real numpy arrays: no contraction)."""
    a, b, c, e = d.real.copy(), d.imag.copy(), s.real, s.imag
    out = np.empty_like(d)
    out.real = a * c - b * e
    out.imag = a * e + b * c
    return out


@pytest.mark.parametrize("s", [2, -1, 1j, 0.3 - 1.7j])
def test_scale(run1, s):
    p, hs = flux_build(ProductSim)
    f = p._fields()
    d = run1.data[STEPS]
    for h in hs[:2]:
        for w in (0, 1):
            f.dft_load(h, w, d[(h, w)])
        f.dft_scale(h, s)
        for w in (0, 1):
            got = f.dft_get(h, w)
            np.testing.assert_array_equal(got, cmul(d[(h, w)], complex(s)))
            if s != 0.3 - 1.7j:  # exact products: every way of multiplying agrees
                np.testing.assert_array_equal(got, d[(h, w)] * s)
            np.testing.assert_array_equal(f.dft_data(h, w), got)
    for w in (0, 1):  # the objects not scaled are untouched
        np.testing.assert_array_equal(f.dft_get(hs[2], w), 0 * d[(hs[2], w)])


def test_scale_dft_fields():
    p, objs = sc_dft_fields_3d(ProductSim)
    o, _ = sc_dft_fields_3d(make_oracle)
    f = p._fields()
    for h, comps in objs:
        before = f.dft_get(h, 0)
        f.dft_scale(h, -1)
        np.testing.assert_array_equal(f.dft_get(h, 0), -before)
        for c in comps:
            for i in (0, 1):
                want = o.dft_array(h, c, i)
                assert np.any(want != 0)
                np.testing.assert_array_equal(p.dft_array(h, c, i), -1 * want)


# ------------------------------------------------------------------ 4. buffering
def single_steps(p, n):
    for _ in range(n):
        p.step(1)


def test_buffered_scale(run1, monkeypatch):
    monkeypatch.setenv("MNL_DFT_BLOCK", "32")
    p, hs = flux_build(ProductSim)
    single_steps(p, 5)
    f = p._fields()
    for h in hs:
        f.dft_scale(h, 2)
        for w in (0, 1):
            assert np.any(run1.data[5][(h, w)] != 0) or h != hs[0]  # the box round the source
            np.testing.assert_array_equal(f.dft_get(h, w), 2 * run1.data[5][(h, w)])


def test_buffered_load_zeros(run1, monkeypatch):
    monkeypatch.setenv("MNL_DFT_BLOCK", "32")
    p, hs = flux_build(ProductSim)
    single_steps(p, 5)
    f = p._fields()
    for h in hs:
        for w in (0, 1):
            f.dft_load(h, w, np.zeros_like(run1.data[5][(h, w)]))
        for w in (0, 1):
            assert not np.any(f.dft_get(h, w)) and not np.any(f.dft_data(h, w))


def test_buffered_identity_load(run1, monkeypatch):
    monkeypatch.setenv("MNL_DFT_BLOCK", "32")
    p, hs = flux_build(ProductSim)
    single_steps(p, 5)
    f = p._fields()
    for h in hs:
        d = [f.dft_get(h, w) for w in (0, 1)]
        for w in (0, 1):
            np.testing.assert_array_equal(d[w], run1.data[5][(h, w)])
            f.dft_load(h, w, d[w])
    single_steps(p, STEPS - 5)
    for h, fo in zip(hs, run1.flux[STEPS]):
        for w in (0, 1):
            np.testing.assert_array_equal(f.dft_get(h, w), run1.data[STEPS][(h, w)])
        np.testing.assert_array_equal(p.flux(h), fo)


# ------------------------------------------------------------------ 5. load, then accumulate
def test_load_then_accumulate(run1, monkeypatch):
    """Product against product (the oracle cannot start from non-zero accumulators): the
    updates after a load are added one at a time in update order whatever the block."""
    res = {}
    for block in ("1", "32", "5"):
        monkeypatch.setenv("MNL_DFT_BLOCK", block)
        p, hs = flux_build(ProductSim)
        f = p._fields()
        for h in hs:
            for w in (0, 1):
                f.dft_load(h, w, run1.data[3][(h, w)])
        single_steps(p, 40)
        res[block] = {(h, w): f.dft_get(h, w) for h in hs for w in (0, 1)}
    for k, v in res["1"].items():
        assert np.any(v != run1.data[3][k])
        np.testing.assert_array_equal(res["32"][k], v)
        np.testing.assert_array_equal(res["5"][k], v)


# ------------------------------------------------------------------ 6. subtraction
def test_subtraction_against_oracle(run1, run2):
    p, hs = flux_build(ProductSim, block=True)
    f = p._fields()
    d1, d2 = run1.data[STEPS], run2.data[STEPS]
    for h in hs:
        for w in (0, 1):
            f.dft_load(h, w, d1[(h, w)], -1)
    p.step(STEPS // 2)
    p.step(STEPS - STEPS // 2)
    for h, dec in zip(hs, run1.decim):
        got = [f.dft_get(h, w) for w in (0, 1)]
        for w in (0, 1):
            U = STEPS // dec
            M = max(run1.peak(h, w), run2.peak(h, w))
            bound = 2 * U * 2.0 ** -53 * M
            diff = got[w] - (d2[(h, w)] - d1[(h, w)])
            err = max(np.max(np.abs(diff.real)), np.max(np.abs(diff.imag)))
            print(f"object {h} list {w}: U = {U}, M = {M:.3e}, max err = {err:.3e}, "
                  f"bound = {bound:.3e}, max |d2 - d1| = {np.max(np.abs(d2[(h, w)] - d1[(h, w)])):.3e}")
            assert M > 0 and np.any(d2[(h, w)] != d1[(h, w)])
            assert err <= bound
        # dft_flux::flux over the product's own arrays, summed in list order
        e, hh = (g.reshape(-1, len(FREQS)) for g in got)
        t = e.real * hh.real + e.imag * hh.imag
        np.testing.assert_array_equal(p.flux(h), np.cumsum(t, axis=0)[-1])


# ------------------------------------------------------------------ 7. near2far
@pytest.fixture(scope="module")
def n2f_base():
    o, hs = n2f.build(ProductSim)
    o.step(n2f.STEPS)
    f = o._fields()
    return {"o": o, "hs": hs, "dft": f.dft_get(hs[3], 0), "far": n2f.farfields(o, hs[3], n2f.FAR)}


def test_near2far_get_is_dft_data(n2f_base):
    o, hs = n2f_base["o"], n2f_base["hs"]
    for h in hs:
        d = o._fields().dft_get(h, 0)
        assert np.any(d != 0)
        np.testing.assert_array_equal(d, o.dft_data(h, 0))


def test_near2far_load(n2f_base):
    d, far = n2f_base["dft"], n2f_base["far"]
    o, hs = n2f.build(ProductSim)
    f = o._fields()
    f.dft_load(hs[3], 0, d)
    np.testing.assert_array_equal(f.dft_get(hs[3], 0), d)
    np.testing.assert_array_equal(n2f.farfields(o, hs[3], n2f.FAR), far)
    f.dft_load(hs[3], 0, d, -1)
    np.testing.assert_array_equal(n2f.farfields(o, hs[3], n2f.FAR), -far)
    assert np.any(far != 0)


def test_near2far_load_two_slabs(n2f_base):
    """The far fields of loaded data on two slabs, at the near2far tests' tolerance for slabs
    (the partial sums of the slabs are added in another order)."""
    d = n2f_base["dft"]
    o, hs = n2f.build(GroupSim)
    load_all(o, hs[3], 0, d)
    np.testing.assert_array_equal(get_sum(o, hs[3], 0), d)
    pts = n2f_base["o"]._fields().near2far_points(n2f_base["hs"][3])
    n2f.check_far(n2f.farfields(o, hs[3], n2f.FAR), pts, d, n2f.FAR, "two slabs, loaded")


# ------------------------------------------------------------------ 8. files
def test_file_flux(run1, tmp_path):
    d = run1.data[STEPS]
    a, hs = flux_build(ProductSim)
    for h in hs[:2]:
        for w in (0, 1):
            a._fields().dft_load(h, w, d[(h, w)])
    b, _ = flux_build(ProductSim)
    for h in hs[:2]:
        path = str(tmp_path / f"flux{h}.mnl")
        a._fields().dft_save(h, path)
        b._fields().dft_load_file(h, path)
        for w in (0, 1):
            np.testing.assert_array_equal(b._fields().dft_get(h, w), d[(h, w)])
        b._fields().dft_load_file(h, path, -1)
        for w in (0, 1):
            np.testing.assert_array_equal(b._fields().dft_get(h, w), -d[(h, w)])


def test_file_near2far(n2f_base, tmp_path):
    path = str(tmp_path / "n2f.mnl")
    n2f_base["o"]._fields().dft_save(n2f_base["hs"][3], path)
    o, hs = n2f.build(ProductSim)
    o._fields().dft_load_file(hs[3], path)
    np.testing.assert_array_equal(o._fields().dft_get(hs[3], 0), n2f_base["dft"])
    np.testing.assert_array_equal(n2f.farfields(o, hs[3], n2f.FAR), n2f_base["far"])


def test_file_from_two_slabs(run1, tmp_path):
    d = run1.data[STEPS]
    g, hs = flux_build(GroupSim)
    h = hs[1]  # the plane across the whole cell: points on both slabs
    for w in (0, 1):
        load_all(g, h, w, d[(h, w)])
        assert all(np.any(f.dft_get(h, w) != 0) for f in g._all())
    path = str(tmp_path / "slabs.mnl")
    g._par(lambda f: f.dft_save(h, path))
    p, _ = flux_build(ProductSim)
    p._fields().dft_load_file(h, path)
    for w in (0, 1):
        np.testing.assert_array_equal(p._fields().dft_get(h, w), d[(h, w)])
    g2, _ = flux_build(GroupSim)  # and back onto slabs: every rank reads the file
    g2._par(lambda f: f.dft_load_file(h, path))
    for w in (0, 1):
        np.testing.assert_array_equal(get_sum(g2, h, w), d[(h, w)])


def test_file_errors(run1, tmp_path):
    d = run1.data[STEPS]
    a, hs = flux_build(ProductSim)
    h = hs[1]
    for w in (0, 1):
        a._fields().dft_load(h, w, d[(h, w)])
    path = str(tmp_path / "plane.mnl")
    a._fields().dft_save(h, path)
    b, _ = flux_build(ProductSim, freqs=FREQS[:3])
    n4, n3 = 2 * d[(h, 0)].size, 2 * d[(h, 0)].size // 4 * 3
    with pytest.raises(RuntimeError, match=r"meep:.*incorrect dataset size \(%d vs\. %d\)" % (n4, n3)):
        b._fields().dft_load_file(h, path)
    raw = open(path, "rb").read()
    cut, foreign = str(tmp_path / "cut.mnl"), str(tmp_path / "foreign.mnl")
    open(cut, "wb").write(raw[:len(raw) // 2])
    open(foreign, "wb").write(b"not a dft file, " * 64)
    c, _ = flux_build(ProductSim)
    with pytest.raises(RuntimeError, match="meep:.*truncated"):
        c._fields().dft_load_file(h, cut)
    with pytest.raises(RuntimeError, match="meep:.*not a dft data file"):
        c._fields().dft_load_file(h, foreign)
    with pytest.raises(RuntimeError, match="meep:.*cannot open"):
        c._fields().dft_load_file(h, str(tmp_path / "missing.mnl"))
    a2, objs = sc_dft_fields_3d(ProductSim, steps=0)
    with pytest.raises(RuntimeError, match="meep:.*different kind"):
        a2._fields().dft_load_file(objs[0][0], path)
    for w in (0, 1):  # refused loads change nothing
        assert not np.any(c._fields().dft_get(h, w))


# ------------------------------------------------------------------ 9. checkpoint
def test_checkpoint_after_load(run1, tmp_path):
    d = run1.data[STEPS]

    def start():
        p, hs = flux_build(ProductSim)
        for h in hs:
            for w in (0, 1):
                p._fields().dft_load(h, w, d[(h, w)], -1)
        return p, hs

    a, hs = start()
    a.step(10)
    path = str(tmp_path / "ck.mnl")
    a.dump(path)
    b, _ = flux_build(ProductSim)
    b.load(path)
    b.step(10)
    c, _ = start()
    c.step(10)
    c.step(10)
    for h in hs:
        for w in (0, 1):
            got = b._fields().dft_get(h, w)
            assert np.any(got != -d[(h, w)]) or run1.decim[h] > 20
            np.testing.assert_array_equal(got, c._fields().dft_get(h, w))


# ------------------------------------------------------------------ 10. the workflow itself
FCEN, DF, NF = 0.3, 0.1, 5


def guide_sim(mp, obstacle):
    """An eps = 12 guide along x in an 8 x 4 x 4 cell with PML, resolution 8, an Ey current sheet
    at x = -2.5; the obstacle is a 0.6-long gap in the guide at x = 0.5.  Reflection plane at
    x = -1.5 (between source and obstacle), transmission plane at x = 2."""
    geom = [mp.Block(size=mp.Vector3(mp.inf, 1, 1), material=mp.Medium(epsilon=12))]
    if obstacle:
        geom.append(mp.Block(size=mp.Vector3(0.6, 1, 1), center=mp.Vector3(0.5),
                             material=mp.Medium(epsilon=1)))
    sim = mp.Simulation(cell_size=mp.Vector3(8, 4, 4), resolution=8, geometry=geom,
                        boundary_layers=[mp.PML(1.0)],
                        sources=[mp.Source(mp.GaussianSource(FCEN, fwidth=0.3), component=mp.Ey,
                                           center=mp.Vector3(-2.5), size=mp.Vector3(0, 1, 1))])
    return sim


def add_planes(mp, sim):
    refl = sim.add_flux(FCEN, DF, NF, mp.FluxRegion(center=mp.Vector3(-1.5), size=mp.Vector3(0, 2, 2)),
                        decimation_factor=1)
    tran = sim.add_flux(FCEN, DF, NF, mp.FluxRegion(center=mp.Vector3(2.0), size=mp.Vector3(0, 2, 2)),
                        decimation_factor=1)
    return refl, tran


@pytest.fixture(scope="module")
def run_a():
    import meep_nl_amd as mp
    sim = guide_sim(mp, False)
    refl, tran = add_planes(mp, sim)
    sim.run(until=50)
    return {"sim": sim, "refl": refl, "tran": tran, "data": sim.get_flux_data(refl),
            "inc": np.array(mp.get_fluxes(refl)), "tran0": np.array(mp.get_fluxes(tran)),
            "steps": sim.timestep}


def test_simulation_reflectance(run_a, tmp_path, capsys):
    import meep_nl_amd as mp
    a = run_a
    assert isinstance(a["data"], mp.FluxData) and a["data"].E.size == a["data"].H.size > 0
    np.testing.assert_array_equal(a["data"].E, a["sim"].fields.dft_data(a["refl"].handle, 0))
    np.testing.assert_array_equal(a["data"].H, a["sim"].fields.dft_data(a["refl"].handle, 1))

    # B': the same run with the incident fields subtracted -> zero up to rounding, bounded by
    # the product of two reassociation errors (U 2^-52 |E|) (U 2^-52 |H|) summed over the plane
    c = guide_sim(mp, False)
    refl_c, _ = add_planes(mp, c)
    c.load_minus_flux_data(refl_c, a["data"])
    got = c.get_flux_data(refl_c)
    np.testing.assert_array_equal(got.E, -a["data"].E)
    np.testing.assert_array_equal(got.H, -a["data"].H)
    c.run(until=50)
    assert c.timestep == a["steps"]
    U = a["steps"]
    E, H = (v.reshape(-1, NF) for v in a["data"])
    bound = (U * 2.0 ** -52) ** 2 * np.sum(np.abs(E) * np.abs(H), axis=0)
    resid = np.array(mp.get_fluxes(refl_c))
    with capsys.disabled():
        print(f"control: U = {U}, |residual flux| = {np.abs(resid)}, bound = {bound}, "
              f"incident = {a['inc']}")
    assert np.all(np.abs(resid) <= bound)

    # B: the obstacle, in memory
    b = guide_sim(mp, True)
    refl_b, tran_b = add_planes(mp, b)
    b.load_minus_flux_data(refl_b, a["data"])
    np.testing.assert_array_equal(b.get_flux_data(refl_b).E, -a["data"].E)
    b.run(until=50)
    refl_flux, tran_flux = np.array(mp.get_fluxes(refl_b)), np.array(mp.get_fluxes(tran_b))
    R, T = -refl_flux / a["inc"], tran_flux / a["tran0"]
    with capsys.disabled():
        print(f"freqs = {mp.get_flux_freqs(refl_b)}\nR = {R}\nT = {T}\nR + T = {R + T}")
    mid = NF // 2
    assert a["inc"][mid] > 0 and a["tran0"][mid] > 0
    assert refl_flux[mid] < 0  # power flowing back, against the plane's +x direction
    assert T[mid] > 0

    # B again through a file: save_flux, reset_meep, load_minus_flux
    s = a["sim"]
    name = str(tmp_path / "refl-flux")
    s.save_flux(name, a["refl"])
    capsys.readouterr()
    s.display_fluxes(a["refl"], a["tran"])
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith("flux1:, ")]
    assert len(lines) == NF and lines[0].count(",") == 3, out
    assert float(lines[mid].split(",")[2]) == a["inc"][mid]
    s.reset_meep()
    with pytest.raises(RuntimeError, match="meep:.*reset"):
        mp.scale_flux_fields(2, a["refl"])
    s.geometry = guide_sim(mp, True).geometry
    refl_f, tran_f = add_planes(mp, s)
    s.load_minus_flux(name, refl_f)
    s.run(until=50)
    np.testing.assert_array_equal(np.array(mp.get_fluxes(refl_f)), refl_flux)
    np.testing.assert_array_equal(np.array(mp.get_fluxes(tran_f)), tran_flux)

    # scale_flux_fields(2, f): the data doubles, the flux quadruples, both exactly
    before = b.get_flux_data(tran_b)
    mp.scale_flux_fields(2, tran_b)
    after = b.get_flux_data(tran_b)
    np.testing.assert_array_equal(after.E, 2 * before.E)
    np.testing.assert_array_equal(after.H, 2 * before.H)
    np.testing.assert_array_equal(np.array(mp.get_fluxes(tran_b)), 4 * tran_flux)
    # the mode aliases are the flux functions themselves
    assert mp.Simulation.load_minus_mode_data is mp.Simulation.load_minus_flux_data


def test_simulation_near2far_data():
    """get / load_minus / scale of a near2far object through Simulation."""
    import meep_nl_amd as mp
    sim = mp.Simulation(cell_size=mp.Vector3(4, 4, 4), resolution=8, boundary_layers=[mp.PML(1.0)],
                        sources=[mp.Source(mp.GaussianSource(0.4, fwidth=0.4), component=mp.Ez,
                                           center=mp.Vector3(0.1, 0.05, 0))])
    box = [mp.Near2FarRegion(center=mp.Vector3(0.7), size=mp.Vector3(0, 1.4, 1.4)),
           mp.Near2FarRegion(center=mp.Vector3(-0.7), size=mp.Vector3(0, 1.4, 1.4), weight=-1)]
    nf = sim.add_near2far(0.4, 0.1, 3, *box, decimation_factor=1)
    sim.run(until=12)
    d = sim.get_near2far_data(nf)
    assert isinstance(d, mp.NearToFarData) and np.any(d.F != 0)
    far = np.array(sim.get_farfield(nf, mp.Vector3(9, 2, 1)))
    mp.scale_near2far_fields(1j, nf)
    np.testing.assert_array_equal(sim.get_near2far_data(nf).F, 1j * d.F)
    sim.load_minus_near2far_data(nf, d)
    np.testing.assert_array_equal(sim.get_near2far_data(nf).F, -d.F)
    np.testing.assert_array_equal(np.array(sim.get_farfield(nf, mp.Vector3(9, 2, 1))), -far)
    sim.load_near2far_data(nf, d)
    np.testing.assert_array_equal(np.array(sim.get_farfield(nf, mp.Vector3(9, 2, 1))), far)
