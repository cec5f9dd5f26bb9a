"""Shared by tests/test_periodic_cpu.py and tests/test_gpu_periodic.py: one periodic unit cell
and its metal-walled supercell, built from the same seeded arrays.

The oracle has no periodic boundaries, so parity comes from a domain-of-dependence argument.
The oracle runs a supercell of R replicas (R odd) of the cell along every periodic axis, with
the materials, the sources and the initial fields replicated.  A Yee step moves information by
at most one cell along an axis; an E update that reads neighbouring components (chi(2)
Newton-Raphson, upstream off-diagonal chi1inv, anisotropic sigma) by one more.  With s = 1 (2
for those families) and m = (R - 1) / 2 * n_d cells between the central replica and the wall,
the central replica equals the infinite lattice bit for bit through step T whenever
s * T <= m - 2.  steps_bound() is that condition; the cases choose T inside it, and the CPU
test compares R against R + 2.

Everything that enters the arithmetic is replicated exactly: the resolution is a power of two
and every position a multiple of half a pixel, so the replicas' coordinates and source weights
are the same dyadic numbers shifted by whole periods; the arrays are indexed modulo the period.
"""
import itertools

import numpy as np

A = 8.0          # pixels per unit length (a power of two: replicated positions are exact)
PML_CELLS = 4    # PML thickness in pixels
E_COMPS, H_COMPS, D_COMPS, B_COMPS = (0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11)
ALL_COMPS = tuple(range(12))

# the cases of the 3-D table: periodic axes, cells, PML axes
CASES = {
    1: dict(dim=3, n=(70, 18, 20), per=(0,), pml=(1, 2)),      # two tile columns, ragged
    2: dict(dim=3, n=(20, 33, 18), per=(1,), pml=(0, 2)),      # three tile rows: 14 + 14 + 5
    3: dict(dim=3, n=(18, 16, 40), per=(2,), pml=(0, 1)),      # several z chunks
    4: dict(dim=3, n=(24, 20, 32), per=(0, 1), pml=(2,)),      # the metasurface cell
    5: dict(dim=3, n=(16, 14, 18), per=(0, 1, 2), pml=()),     # all three
    "2d": dict(dim=2, n=(20, 18, 0), per=(0,), pml=(1,)),      # x periodic, y PML
    "2dy": dict(dim=2, n=(19, 22, 0), per=(1,), pml=(0,)),     # y periodic, x PML
}
# families whose E update reads neighbouring components: reach 2 per step
REACH2 = ("nr", "upstream", "aniso")
FAMILIES = ("plain", "lorentz", "nr", "upstream", "aniso", "cond", "mu")


def reach(family):
    return 2 if any(f in REACH2 for f in family.split("+")) else 1


def case_of(case):
    """A key of CASES, or a dict of the same form (the random family draws its own cells)."""
    return case if isinstance(case, dict) else CASES[case]


def steps_bound(case, R, family):
    """The largest T with s * T <= m - 2, m the cells from the central replica to the wall."""
    c = case_of(case)
    m = min((R - 1) // 2 * c["n"][d] for d in c["per"])
    return (m - 2) // reach(family)


def axes_of(dim):
    return (0, 1) if dim == 2 else (0, 1, 2)


def _mod_take(arr, n, per, dim, R=1, trans=(0, 0, 0)):
    """arr over the cell's (n + 1)-point axes -> the same values indexed modulo the period over
    R periods along every periodic axis (plane n is plane 0 of the next replica), moved
    cyclically by trans cells."""
    for k, d in enumerate(axes_of(dim)):
        if d in per:
            arr = np.take(arr, (np.arange(R * n[d] + 1) - trans[d]) % n[d], axis=k)
    return arr


def _index_mask(n, per, dim, lo_frac, hi_frac, seam):
    """A block in index space: along a periodic axis the cells within `seam` of the seam (it
    crosses the seam), along the others the fractions [lo_frac, hi_frac) of the axis."""
    shape = tuple(n[d] + 1 for d in axes_of(dim))
    m = np.ones(shape, dtype=bool)
    for k, d in enumerate(axes_of(dim)):
        j = np.arange(n[d] + 1)
        if d in per:
            jm = j % n[d]
            ok = (jm >= n[d] - seam) | (jm < seam + 1)
        else:
            ok = (j >= int(lo_frac * n[d])) & (j < int(hi_frac * n[d]))
        sh = [1] * len(shape)
        sh[k] = -1
        m &= ok.reshape(sh)
    return m


class Scene:
    """What configure() needs about one case: `R` replicas of the cell along the periodic axes
    (R = 1: the periodic product run itself)."""

    def __init__(self, case, family, R, trans=(0, 0, 0), planar_comp=0):
        c = case_of(case)
        self.case, self.family, self.R = case, family, R
        self.trans = tuple(trans)  # everything moved cyclically by so many cells (periodic axes)
        # the planar source's component.  Ex is shifted along x: where x is periodic its end
        # weights differ (1/8 from the image, 7/8 from the period itself), which the parity
        # cases want.  A period of 2 n adds those two in the other order on one of the seams,
        # so the replication property holds bit for bit only for a component unshifted along
        # the periodic axes (1/2 + 1/2)
        self.planar_comp = planar_comp
        self.dim, self.n, self.per, self.pml = c["dim"], tuple(c["n"]), tuple(c["per"]), c.get("pml", ())
        self.k = (R - 1) // 2
        self.n_super = [self.n[d] * (R if d in self.per else 1) for d in range(3)]
        # the central replica sits at the same coordinates as the periodic cell [0, L]
        self.io = [-2 * self.k * self.n[d] if d in self.per else 0 for d in range(3)]
        self.L = [self.n[d] / A for d in range(3)]

    def make(self, maker):
        if self.dim == 2:
            return maker(2, [self.n_super[0], self.n_super[1], 0], A, 0.5, self.io)
        return maker(3, self.n_super, A, 0.5, self.io)

    def tile(self, arr):
        return _mod_take(arr, self.n, self.per, self.dim, self.R, self.trans)

    def cell_array(self, rng, scale=1.0):
        shape = tuple(self.n[d] + 1 for d in axes_of(self.dim))
        return _mod_take(scale * rng.standard_normal(shape), self.n, self.per, self.dim)

    def mask(self, lo=0.3, hi=0.7, seam=3):
        return _index_mask(self.n, self.per, self.dim, lo, hi, seam)

    def shifts(self):
        """The replicas' offsets (length units per direction), in the order in which the
        periodic run's lattice-shift loop (src/loop_in_chunks.cpp:406-532: shifts ascending, the
        first direction fastest) meets their contributions: a shift s brings in what replica -s
        holds, so the replicas go in descending order, x fastest.  Where two replicas' sources
        meet on a seam point with different weights, the order of the two additions is then the
        periodic run's."""
        rng = [tuple(reversed(range(-self.k, self.R - self.k))) if d in self.per else (0,)
               for d in (2, 1, 0)]
        return [[j[2 - d] * self.L[d] for d in range(3)] for j in itertools.product(*rng)]

    def central(self, arr):
        """The central replica's (n + 1)-point block of a supercell array."""
        sl = []
        for d in axes_of(self.dim):
            lo = self.k * self.n[d] if d in self.per else 0
            sl.append(slice(lo, lo + self.n[d] + 1))
        return arr[tuple(sl)]


def materials(o, sc, block, slab):
    """The family's materials (sc.family; several joined with "+") with the dielectric block
    and the slab as masks over the cell's (n + 1)-point axes."""
    fams = sc.family.split("+")
    ecomps = E_COMPS
    if "upstream" in fams:
        o.set_upstream_nl(True)
    for c in ecomps:
        o.set_chi1inv(c, c, sc.tile(np.where(block, 0.25, 1.0)))
        if ("nr" in fams or "upstream" in fams):
            for d in range(3):
                if d != c:
                    o.set_chi1inv(c, d, sc.tile(np.where(block, 1e-3, 0.0)))
        if "nr" in fams:
            o.set_chi2(c, sc.tile(np.where(block, 0.5, 0.0)))
        if "upstream" in fams:
            o.set_chi3(c, sc.tile(np.where(block, 2e-2, 0.0)))
            o.set_chi2(c, sc.tile(np.where(block, 3e-2, 0.0)))
    # (above the sources' planes: a D source inside a polarization box keeps a run unfused)
    if "lorentz" in fams:
        o.add_lorentzian(1.1, 0.05, [sc.tile(np.where(slab, 0.6, 0.0)) for _ in ecomps])
    if "lorentz4" in fams:  # as many terms as a structure takes: 12 polarization arrays to wrap
        for k in range(4):
            o.add_lorentzian(0.7 + 0.1 * k, 0.05 + 0.01 * k,
                             [sc.tile(np.where(slab, 0.1 + 0.05 * k, 0.0)) for _ in ecomps])
    if "aniso" in fams:
        sig = [[None] * 3 for _ in range(3)]
        for c in ecomps:
            sig[c][c] = sc.tile(np.where(slab, 0.4, 0.0))
        sig[0][1] = sc.tile(np.where(slab, 0.1, 0.0))
        sig[1][0] = sc.tile(np.where(slab, 0.1, 0.0))
        o.add_lorentzian_tensor(1.0, 0.05, sig)
    if "cond" in fams:
        for c in D_COMPS + B_COMPS:
            o.set_conductivity(c, sc.tile(np.where(slab, 0.7, 0.0)))
    if "mu" in fams:
        for c in H_COMPS:
            o.set_chi1inv(c, c % 3, sc.tile(np.where(block, 1 / 2.5, 1.0)))
        o.add_magnetic_lorentzian(1.0, 0.1, [sc.tile(np.where(slab, 0.3, 0.0)) for _ in H_COMPS])


def configure(o, sc, seed=11, init=True):
    """The same content on a periodic cell (sc.R == 1, o periodic already) or its supercell:
    PML on the non-periodic axes, a dielectric block across the seam, the family's materials, a
    point source one cell from the seam, a full-period planar Gaussian source, random D and B."""
    rng = np.random.default_rng(seed)
    fam, dim = sc.family, sc.dim
    if sc.pml:
        o.add_pml(PML_CELLS / A, dirs=tuple(sc.pml))
    materials(o, sc, sc.mask(), sc.mask(0.6, 0.85, seam=2))
    if hasattr(o, "make_periodic"):  # the product: fields::use_bloch before the sources
        o.make_periodic(sc.per)
    # sources: every replica gets its own copy (the periodic run: one, with its image chunks)
    nd = len(axes_of(dim))
    # (a translated run moves it across the seam: its stencil then needs the image chunks)
    pt = [((1.0 + sc.trans[d]) / A) % sc.L[d] if d in sc.per else (int(0.5 * sc.n[d]) + 0.5) / A
          for d in range(nd)]
    z_like = [d for d in axes_of(dim) if d not in sc.per]
    # the planar source's period moves with a translation (its two half-weight ends must stay
    # on the same material plane: where D is not 0, D - X/2 - X/2 and D - X round differently),
    # so a translated run's region sticks out of the cell and the lattice-shift loop folds it
    lo = [sc.trans[d] / A if d in sc.per else (int(0.4 * sc.n[d]) / A) for d in range(nd)]
    hi = [sc.L[d] + sc.trans[d] / A if d in sc.per else lo[d] for d in range(nd)]
    if not z_like:  # all axes periodic: a full-period plane at a fixed z
        lo[2] = hi[2] = 5 / A
    src_c = 2 if dim == 2 else 1
    for s in sc.shifts():
        o.add_gaussian_source(src_c, 0.9, 0.7, -3.0, 3.0,
                              tuple(pt[d] + s[d] for d in range(nd)), 1.0)
        o.add_gaussian_volume_source(sc.planar_comp, 0.7, 0.9, -3.0, 3.0, [lo[d] + s[d] for d in range(nd)],
                                     [hi[d] + s[d] for d in range(nd)], 0.5)
        if dim == 2:  # a TE source beside the TM one
            o.add_gaussian_source(5, 0.8, 0.7, -3.0, 3.0,
                                  tuple(pt[d] + s[d] + 0.5 / A for d in range(nd)), 1.0)
    if init:
        for c in D_COMPS + B_COMPS:
            o.initialize_field(c, sc.tile(sc.cell_array(np.random.default_rng(seed + 31 * c), 0.1)))
    return o


def product_makers():
    """ProductSim / GroupSim / GroupSim3 with make_periodic (imported lazily: they load the
    library)."""
    from scenarios import GroupSim, GroupSim3, ProductSim

    def periodic(base):
        class P(base):
            def make_periodic(self, per):
                fs = self._all() if hasattr(self, "_all") else [self._fields()]
                for f in fs:
                    for d in per:
                        f.use_bloch(d)
        return P
    return periodic(ProductSim), periodic(GroupSim), periodic(GroupSim3)


def run_product(case, family, T, seed=11, maker=None, chunks=None, before=None, R=1,
                trans=(0, 0, 0), planar_comp=0):
    """The periodic product run: T steps in one call, or in the given chunks with a read of
    every array in between.  R = 2: a period of two replicas; trans: everything moved."""
    sc = Scene(case, family, R, trans, planar_comp)
    o = configure(sc.make(maker or product_makers()[0]), sc, seed)
    if before:
        before(o)
    if chunks is None:
        o.step(T)
    else:
        assert sum(chunks) == T
        for k in chunks:
            o.step(k)
            for c in (0, 4, 8):
                o.get_array(c)
    return sc, o


def run_oracle(case, family, R, T, seed=11):
    from scenarios import make_oracle
    sc = Scene(case, family, R)
    o = configure(sc.make(make_oracle), sc, seed)
    o.step(T)
    return sc, o


_ORACLE = {}


def oracle_central(case, family, T, R=3, seed=11):
    """The central replica's arrays of the supercell oracle after T steps, computed once."""
    key = (case, family, T, R, seed)
    if key not in _ORACLE:
        assert T <= steps_bound(case, R, family), (case, family, T)
        sc, o = run_oracle(case, family, R, T, seed)
        _ORACLE[key] = {c: sc.central(o.get_array(c)).copy() for c in ALL_COMPS}
    return _ORACLE[key]


# ---------------------------------------------------------------- lattice-shift loop (1 axis)
def shift_loop_1d(wmin, wmax, n, a, sh, io=0):
    """loop_in_chunks' loop over lattice shifts (src/loop_in_chunks.cpp:390-532) restated for
    one periodic axis of n cells whose little corner sits at half-pixel coordinate io, on a grid
    whose points have half-pixel parity sh: the chunks in list order as (first owned index
    point in half-pixels, shift in half-pixels, weights per point)."""
    import math
    from dft_restate import boundary_weights_1d
    i0, w, _ = boundary_weights_1d(wmin, wmax, a, sh)
    i1 = i0 + 2 * (len(w) - 1)
    L = n / a
    gmin, gmax = io * 0.5 / a, io * 0.5 / a + L
    lo_s = int(math.floor((wmin - gmax) / L))
    hi_s = int(math.ceil((wmax - gmin) / L))
    own_lo, own_hi = io + 2 - sh, io + 2 * n - sh  # little / big owned corner
    out = []
    for s in range(lo_s, hi_s + 1):
        shifti = 2 * n * s
        isc, iec = max(i0 - shifti, own_lo), min(i1 - shifti, own_hi)
        if isc > iec:
            continue
        k0 = (isc + shifti - i0) // 2
        npt = (iec - isc) // 2 + 1
        out.append((isc, shifti, w[k0:k0 + npt].copy()))
    return out


# ---------------------------------------------------------------- non-periodic checkpoint
def metal_checkpoint_run(core, path, steps=9):
    """A small run with metal x / y walls and PML in z, nothing periodic, dumped after `steps`
    steps: tests/golden/ckpt_metal_parent.mnl holds the bytes the parent commit wrote for it,
    and a checkpoint of a non-periodic run must stay byte for byte what it was."""
    gv = core.GridVolume(3, [6, 5, 12], A, [0, 0, 0])
    s = core.Structure(gv)
    s.add_pml(2 / A, (2,), (0, 1))
    shape = gv.shape()
    j = np.indices(shape)
    for c in E_COMPS:
        s.set_chi1inv(c, c, np.where((j[0] >= 2) & (j[0] < 5) & (j[2] >= 4) & (j[2] < 8), 0.25, 1.0))
    f = core.Fields(s)
    f.add_gaussian_source(2, 0.9, 0.7, -3.0, 3.0, (3.25 / A, 2.5 / A, 6.5 / A), 1.0)
    for c in D_COMPS + B_COMPS:
        f.initialize_field(c, 0.1 * np.random.default_rng(5 + c).standard_normal(shape))
    f.step(steps)
    f.dump(path)
    return f
