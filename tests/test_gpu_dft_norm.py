"""fields::dft_norm / dft_maxfreq / max_decimation (src/dft.cpp:312-399):
the device reduction over every DFT array against numpy over the lists dft_get returns.

All terms of the sum are non-negative, so with N complex values a sum in any order is within
(N + 2) u of the exact one and the square root within (N / 2 + 2) u, u = 2^-53; two such
results differ by at most (2 N + 4) u, relative."""
import numpy as np
import pytest

from scenarios import FLUX3D_FREQS, GroupSim, GroupSim3, ProductSim, sc_dft_fields_3d, sc_flux_3d

pytestmark = pytest.mark.gpu

STEPS = 24
FR = [0.13, 0.21, 0.3]


def _fields_of(o):
    return o._all() if hasattr(o, "_all") else [o._fields()]


def _add_more(o):
    """dft_fields of D and B, near2far, energy and force objects beside sc_flux_3d's four flux
    objects: (handle, lists) of every object."""
    objs = []
    for f in _fields_of(o):
        objs = [(f.add_dft_fields([6, 7, 8, 9, 10, 11], [-0.9, -0.7, -1.1], [1.0, 0.8, 0.6], FR,
                                  False, 1), 1),
                (f.add_dft_near2far([([-0.7, -0.6, 0.75], [0.7, 0.6, 0.75], 2, 1.0),
                                     ([0.7, -0.6, 0.75], [0.7, 0.6, 1.3], 0, 1.0)], FR, 1), 1),
                (f.add_dft_energy([([-0.5, -0.4, -0.3], [0.6, 0.5, 0.4], 0, 1.0)], FR, 2), 4),
                (f.add_dft_force([([-0.5, -0.5, 0.45], [0.5, 0.5, 0.45], 2, 1.0),
                                  ([-0.5, -0.5, 0.45], [0.5, 0.5, 0.45], 0, 1.0)], FR, 1), 3)]
    return objs


def _numpy_norm(o, objs):
    """sqrt(sum |dft_get|^2) over every list of every object (summed over the ranks' points)."""
    total, n = 0.0, 0
    for h, nlists in objs:
        for which in range(nlists):
            d = sum(f.dft_get(h, which) for f in _fields_of(o))
            total += float(np.sum(d.real * d.real + d.imag * d.imag))
            n += d.size
    return np.sqrt(total), n


def _norm(o):
    if hasattr(o, "_all"):
        v = o._par(lambda f: f.dft_norm())  # collective
        assert all(x == v[0] for x in v)
        return v[0]
    return o._fields().dft_norm()


def _close(a, b, n):
    assert abs(a - b) <= (2 * n + 4) * 2.0 ** -53 * max(a, b), (a, b, n, abs(a - b) / max(a, b))


def _scene(make, calls=(STEPS,), sizes=None, setup=None):
    box = {}

    def extra(o):
        box["objs"] = _add_more(o)
        box["zero"] = _norm(o)
        if setup:
            setup(o)
    o, hs = sc_flux_3d(make, sizes=sizes, extra=extra, calls=[None] + list(calls))
    return o, [(h, 2) for h in hs] + box["objs"], box["zero"]


@pytest.fixture(scope="module")
def scene():
    return _scene(ProductSim)


def test_norm_against_numpy_every_kind(scene):
    o, objs, zero = scene
    assert zero == 0.0  # before the first step
    want, n = _numpy_norm(o, objs)
    got = _norm(o)
    assert want > 0 and n > 10000
    _close(got, want, n)
    assert _norm(o) == got  # the same bits in every call
    f = o._fields()
    fmax = max(max(FLUX3D_FREQS), max(FR))  # (2 pi f) / (2 pi): two roundings
    assert abs(f.dft_maxfreq() - fmax) <= 4 * 2.0 ** -53 * fmax
    # the factors given: 1 everywhere, 2 for the energy object, and the automatic one (0) of
    # the fourth flux object, fields::add_dft's rule (src/dft.cpp:190-213) worked out here from
    # sc_flux_3d's two Gaussian sources (frequency, width) and the monitor's frequencies: no
    # nonlinearity, so floor(1 / (dt * (largest monitor frequency + largest source frequency
    # plus half its bandwidth)))
    src_max = max(fr + 0.5 * np.sqrt(-2.0 * np.log(1e-7)) / (w * np.pi)
                  for fr, w in ((0.15, 10.0), (0.2, 6.0)))
    auto = max(1, int(np.floor(1 / (o.dt * (max(FLUX3D_FREQS) + src_max)))))
    assert auto > 2  # so that it is the largest
    assert [f.dft_decimation(h) for h, _ in objs] == [1, 1, 1, auto, 1, 1, 2, 1]
    assert f.max_decimation() == auto


def test_norm_dft_fields_scenario():
    o, objs = sc_dft_fields_3d(ProductSim, steps=STEPS)
    objs = [(h, 2 if h == objs[-1][0] else 1) for h, _ in objs]
    want, n = _numpy_norm(o, objs)
    _close(_norm(o), want, n)
    f = o._fields()
    assert f.max_decimation() == max(f.dft_decimation(h) for h, _ in objs) >= 1


def test_norm_without_objects():
    from test_gpu_tb import sc_tb
    f = sc_tb(ProductSim, sizes=(3.2, 3.2, 3.2), srcs=((0.05, 0.05, 0.05),), steps=(2,))._fields()
    assert (f.dft_norm(), f.dft_maxfreq(), f.max_decimation()) == (0.0, 0.0, 1)


def test_norm_probes_scale_and_load():
    o, objs, _ = _scene(ProductSim)
    f = o._fields()
    before = _norm(o)
    h = f.add_probe(2, (0.1, 0.2, 0.3))
    assert _norm(o) == before  # probes are not DFT objects
    f.remove_probes()
    s = -0.75 + 0.5j
    f.dft_scale(objs[1][0], s)
    want, n = _numpy_norm(o, objs)
    _close(_norm(o), want, n)
    f.dft_scale(objs[1][0], 1 / s)
    for hh, nlists in objs:
        f.dft_scale(hh, s)
    want, n = _numpy_norm(o, objs)
    _close(_norm(o), want, n)
    _close(_norm(o), abs(s) * before, 3 * n)  # (beside it: three roundings more per value)
    # load of the object's own data with sign -1: the values change sign, compared with numpy
    hh = objs[0][0]
    data = [f.dft_get(hh, w) for w in (0, 1)]
    for w in (0, 1):
        f.dft_load(hh, w, data[w], -1)
    assert np.array_equal(f.dft_get(hh, 0), -data[0])
    want, n = _numpy_norm(o, objs)
    _close(_norm(o), want, n)
    # ... and of zeros: that object's share of the norm drops out
    for w in (0, 1):
        f.dft_load(hh, w, np.zeros_like(data[w]), -1)
    want2, n = _numpy_norm(o, objs)
    assert want2 < want
    _close(_norm(o), want2, n)
    assert h >= 1 << 30


def test_norm_same_bits_in_every_mode():
    sizes = [9.6, 6.4, 8.0]  # the pair tests' grid: the two-step kernel runs

    def tb(on):
        return lambda o: o._fields().set_temporal_blocking(on)

    def unfused(o):
        o._fields().set_fused(False)
    pairs, objs, _ = _scene(ProductSim, sizes=sizes, setup=tb(True))
    assert pairs._fields().tb_info()["active"]
    want = _norm(pairs)
    ref, n = _numpy_norm(pairs, objs)
    _close(want, ref, n)
    fused, _, _ = _scene(ProductSim, sizes=sizes, setup=tb(False))
    assert fused._fields().fused_active() and not fused._fields().tb_info()["active"]
    plain, _, _ = _scene(ProductSim, sizes=sizes, setup=unfused)
    assert not plain._fields().fused_active()
    single, _, _ = _scene(ProductSim, calls=[1] * STEPS, sizes=sizes)
    for o in (fused, plain, single):
        assert _norm(o) == want


@pytest.mark.parametrize("make", [GroupSim, GroupSim3], ids=["2slabs", "3slabs"])
def test_norm_slabs(scene, make):
    one, objs, _ = scene
    n = sum(one._fields().dft_list_size(h, w) for h, k in objs for w in range(k))
    o, _, zero = _scene(make)
    assert zero == 0.0
    _close(_norm(o), _norm(one), n)
