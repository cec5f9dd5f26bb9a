"""Shared by tests/test_bloch_cpu.py and tests/test_gpu_bloch.py: complex fields and Bloch
boundaries with k != 0 on the cells of tests/periodic_cases.py.

The oracle has real fields and no periodic boundaries.  A Bloch-periodic run with sources of
amplitude A equals the infinite lattice whose replica at R (cells r_d along the periodic
axes) carries the sources A * prod_d eikna[d]^r_d; its real and imaginary parts are two real
problems, whose sources are the real and the imaginary part of those amplitudes.  The oracle
runs the metal-walled supercell of periodic_cases.Scene twice, and inside the light cone
(periodic_cases.steps_bound) its central replica is that lattice.

Only a real k has such a lattice: for a complex k the reference brings a point in from below
with conj(eikna) and from above with eikna (src/boundaries.cpp:201-224), which are not
inverses of each other, so the complex-k phases are checked on the phase table and, on the
device, ghost point against owned point (tests/test_gpu_bloch.py).
"""
import itertools
import math

import numpy as np

import periodic_cases as pc

A = pc.A
PI = 3.141592653589793238462643383276  # meep::pi


# what the GPU tests run with k != 0 (tests/test_bloch_cpu.py checks the light cone for each)
AMP = complex(0.8, -0.6)
ZONE_CASES = (("2d", (0,)), (1, (0,)), (4, (0, 1)), (5, (0, 1, 2)))  # case, axes at the zone edge
GENERIC_K = (0.1, 0.2, 0.0)
GENERIC_CASES = ("2d", 4, 5)   # one 2-D cell and two 3-D cells
FAMILIES = ("plain", "lorentz", "cond", "mu")
FAMILY_CASE = 4                # the families run on the metasurface cell


def k_cases():
    """(case, family, k, planar) of every k != 0 comparison against the oracle."""
    out = [(case, "plain", zone_edge_k(case, axes), False) for case, axes in ZONE_CASES]
    out += [(case, "plain", GENERIC_K, True) for case in GENERIC_CASES]
    out += [(FAMILY_CASE, f, GENERIC_K, True) for f in FAMILIES if f != "plain"]
    out += [(FAMILY_CASE, f, zone_edge_k(FAMILY_CASE, (0, 1)), False) for f in FAMILIES
            if f != "plain"]
    return out


# ---------------------------------------------------------------- the phases, restated
def eikna_np(k, n, a):
    """fields::use_bloch (src/boundaries.cpp:88-99): eikna of one direction."""
    k = complex(k)
    if k.real * n == 0.5 * a:  # check b.z. edge exactly
        return complex(-math.exp(-k.imag * ((2 * PI / a) * n)))
    z, x = 1j * k, (2 * PI / a) * n
    return np.exp(complex(z.real * x, z.imag * x)).item()  # complex * double scales both parts


def phase_table_np(eikna):
    """locate_point_in_user_volume (src/boundaries.cpp:201-224) for the all-axes-at-once
    mapping: index s0 + 3 s1 + 9 s2 with s = 0 none, 1 brought in from below (conj), 2 from
    above; the product over the directions in order, starting from 1."""
    tab = []
    for s2, s1, s0 in itertools.product(range(3), repeat=3):
        ph = complex(1.0)
        for d, s in enumerate((s0, s1, s2)):
            if s == 1:
                ph = ph * np.conj(eikna[d])
            elif s == 2:
                ph = ph * eikna[d]
        tab.append(complex(ph))
    return tab


def zone_edge_k(case, axes):
    """k = a / (2 n_d) along the given periodic axes: eikna = -1 exactly."""
    c = pc.case_of(case)
    return tuple(A / (2 * c["n"][d]) if d in axes else 0.0 for d in range(3))


# ---------------------------------------------------------------- one scene on both sides
def replica_factor(sc, k, s):
    """prod_d eikna[d]^r_d of the replica shifted by s (length units), formed from the same
    eikna as the product's table; r_d < 0 takes the conjugate (a real k: |eikna| = 1)."""
    f = complex(1.0)
    for d in sc.per:
        r = int(round(s[d] / sc.L[d]))
        e = eikna_np(k[d], sc.n[d], A)
        for _ in range(abs(r)):
            f = f * (e if r > 0 else np.conj(e))
    return f


def configure(o, sc, amp=1.0, k=(0.0, 0.0, 0.0), seed=11, part=None, planar=False, init=False):
    """periodic_cases.configure with complex amplitudes: PML, the family's materials, a point
    source one cell from the seam (two in 2-D), optionally the full-period planar source and
    random initial D and B (k = 0 only: they are replicated without a phase).

    part=None: the complex product run (o makes its fields complex and periodic with k).
    part=0 / 1: a real run (the oracle's supercell or a real product run) of the real /
    imaginary part: every replica's sources scaled by Re / Im of amp * replica_factor, which a
    real run takes as the amplitudes f and -i f (real(-i f J) = imag(f J))."""
    dim = sc.dim
    if sc.pml:
        o.add_pml(pc.PML_CELLS / A, dirs=tuple(sc.pml))
    pc.materials(o, sc, sc.mask(), sc.mask(0.6, 0.85, seam=2))
    if hasattr(o, "make_bloch"):
        o.make_bloch(sc.per, k)
    elif hasattr(o, "make_periodic"):
        o.make_periodic(sc.per)
    nd = len(pc.axes_of(dim))
    pt = [(1.0 / A) if d in sc.per else (int(0.5 * sc.n[d]) + 0.5) / A for d in range(nd)]
    lo = [0.0 if d in sc.per else (int(0.4 * sc.n[d]) / A) for d in range(nd)]
    hi = [sc.L[d] if d in sc.per else lo[d] for d in range(nd)]
    if len(sc.per) == nd:
        lo[nd - 1] = hi[nd - 1] = 5 / A
    src_c = 2 if dim == 2 else 1
    for s in sc.shifts():
        f = complex(amp) * replica_factor(sc, k, s)
        if part == 1:
            f = complex(f.imag, -f.real)  # -i f
        o.add_gaussian_source(src_c, 0.9, 0.7, -3.0, 3.0,
                              tuple(pt[d] + s[d] for d in range(nd)), f)
        if planar:
            o.add_gaussian_volume_source(0, 0.7, 0.9, -3.0, 3.0,
                                         [lo[d] + s[d] for d in range(nd)],
                                         [hi[d] + s[d] for d in range(nd)], 0.5 * f)
        if dim == 2:
            o.add_gaussian_source(5, 0.8, 0.7, -3.0, 3.0,
                                  tuple(pt[d] + s[d] + 0.5 / A for d in range(nd)), f)
    if init:
        assert all(x == 0 for x in k)
        for c in pc.D_COMPS + pc.B_COMPS:
            re = sc.tile(sc.cell_array(np.random.default_rng(seed + 31 * c), 0.1))
            im = sc.tile(sc.cell_array(np.random.default_rng(seed + 31 * c + 7), 0.1))
            o.initialize_field(c, re + 1j * im if part is None else (re, im)[part])
    return o


def bloch_maker():
    """ProductSim with complex fields: make_bloch(per, k) before the sources; get_array(c,
    part)."""
    from scenarios import ProductSim

    class B(ProductSim):
        def make_bloch(self, per, k):
            f = self._fields()
            f.use_complex_fields()
            for d in per:
                f.use_bloch(d, k[d])

        def get_array(self, c, part=0):
            return self._fields().get_array(c, part)

    return B


def bloch_group_makers():
    """GroupSim / GroupSim3 (2 / 3 in-process slabs) with complex fields on every rank."""
    from scenarios import GroupSim, GroupSim3

    def mk(base):
        class G(base):
            def make_bloch(self, per, k):
                for f in self._all():
                    f.use_complex_fields()
                    for d in per:
                        f.use_bloch(d, k[d])

            def get_array(self, c, part=0):
                return sum(f.get_array(c, part) for f in self._all())
        return G
    return mk(GroupSim), mk(GroupSim3)


def run_bloch(case, family, T, amp=1.0, k=(0.0, 0.0, 0.0), before=None, chunks=None, R=1,
              maker=None, **kw):
    """The complex product run on the periodic cell (R = 2: a period of two replicas, the
    second one's sources times eikna, periodic with the same k over 2 n cells)."""
    sc = pc.Scene(case, family, R)
    o = configure(sc.make(maker or bloch_maker()), sc, amp, k, **kw)
    if before:
        before(o)
    if chunks is None:
        o.step(T)
    else:
        assert sum(chunks) == T
        for n in chunks:
            o.step(n)
            for c in (0, 4, 8):
                o.get_array(c, 0), o.get_array(c, 1)
    return sc, o


def run_real(case, family, T, part, amp=1.0, **kw):
    """A real product run of one part at k = 0 (periodic, real fields)."""
    sc = pc.Scene(case, family, 1)
    o = configure(sc.make(pc.product_makers()[0]), sc, amp, part=part, **kw)
    o.step(T)
    return sc, o


_ORACLE = {}


def oracle_parts(case, family, T, amp, k, R=3, **kw):
    """The central replica of the oracle's supercell for both parts: {part: {comp: array}},
    computed once."""
    key = (case, family, T, complex(amp), tuple(k), R, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        from scenarios import make_oracle
        assert T <= pc.steps_bound(case, R, family), (case, family, T)
        out = {}
        for part in (0, 1):
            sc = pc.Scene(case, family, R)
            o = configure(sc.make(make_oracle), sc, amp, k, part=part, **kw)
            o.step(T)
            out[part] = {c: sc.central(o.get_array(c)).copy() for c in pc.ALL_COMPS}
        _ORACLE[key] = out
    return _ORACLE[key]
