"""Low-level mirror of the reference C++ API (meep::structure / meep::fields).

Mirrors src/meep.hpp:809-920 (structure) and 1731-2330 (fields) for the
hot-path subset: grid_volume construction (vol1d/vol2d/vol3d +
center_origin), pml(), set_chi1inv / set_epsilon, set_chi2 / set_chi3,
add_susceptibility(lorentzian), add_point_source / add_volume_source (point),
step(), time()/round_time(), get_field(), and raw component arrays.

Arrays use the reference's own per-chunk layout for the whole cell
((n+1) points per present direction, Z fastest; src/vec.cpp:482-494).
"""
import ctypes
import os
import math

import numpy as np

from . import _lib
from ._lib import check, dptr, iptr, llptr, lib, ptr

Ex, Ey, Ez, Hx, Hy, Hz, Dx, Dy, Dz, Bx, By, Bz = range(12)
Dielectric, Permeability = 12, 13  # derived slice components (src/meep/vec.hpp:52-53)
X, Y, Z = 0, 1, 2

# meep::time_sink (src/meep.hpp:1610-1633) and the print_times labels
# (DescriptionByTimeSink, src/time.cpp:28-51), in enum order
TIME_SINKS = (
    ("Connecting", "connecting chunks"), ("Stepping", "time stepping"),
    ("Boundaries", "copying boundaries"), ("MpiAllTime", "all-all communication"),
    ("MpiOneTime", "1-1 communication"), ("FieldOutput", "outputting fields"),
    ("FourierTransforming", "Fourier transforming"), ("MPBTime", "MPB mode solver"),
    ("GetFarfieldsTime", "far-field transform"), ("Other", "everything else"),
    ("FieldUpdateB", "updating B field"), ("FieldUpdateH", "updating H field"),
    ("FieldUpdateD", "updating D field"), ("FieldUpdateE", "updating E field"),
    ("BoundarySteppingB", "boundary stepping B"), ("BoundarySteppingWH", "boundary stepping WH"),
    ("BoundarySteppingPH", "boundary stepping PH"), ("BoundarySteppingH", "boundary stepping H"),
    ("BoundarySteppingD", "boundary stepping D"), ("BoundarySteppingWE", "boundary stepping WE"),
    ("BoundarySteppingPE", "boundary stepping PE"), ("BoundarySteppingE", "boundary stepping E"),
)


# The numbers of the diagnostic ABI, mirrors of the enums of include/meep_nl_amd.h
# (tests/test_abi_tables_cpu.py holds the two together).
# MNL_SCHED_*: Fields.set_schedule's options; 10, 13, 14 and 15 are retired
SCHEDULE = {"narrow": 0, "dft_pal": 1, "res": 2, "res_tb2": 3, "res_rim": 4, "dft_cmp": 5,
            "rim_zchunk": 6, "nr_early": 7, "tb_zchunk": 8, "tb_ox": 9, "tb_pol": 11,
            "r1_beside": 12, "src_guard": 16}
# the options that take a count (CUs left free, -1: the default; planes; columns), not a switch
SCHEDULE_INT = ("res", "res_tb2", "res_rim", "rim_zchunk", "tb_zchunk", "tb_ox")
# MNL_KSTAT_*: Fields.kernel_stats' kernel groups
KERNEL_STATS = {"tile": 0, "curl_d": 1, "general": 2, "dft": 3, "e_update": 4, "pairs": 5,
                "rim": 6, "chain": 7, "ghost_wait": 8, "n2f_far": 9, "n2f_reduce": 10,
                "dft_get": 11, "dft_load": 12, "dft_scale": 13}
# MNL_TBINFO_*: the slots of Fields.tb_info, in order
TB_INFO_KEYS = ("active", "tb_cells", "tb_border", "tb_cells_mixed", "rim_cells",
                "rim_cells_mixed", "tb_items", "rim_items", "tb_planes", "narrow_items", "enabled",
                "tb_zchunk", "tb_width", "tb_pol")
# MNL_MODE_*: the bits of mnl_fields_mode
MODE_FUSED, MODE_PALETTE, MODE_CONTIG, MODE_TILE, MODE_CONCURRENT = 1, 2, 4, 16, 32
MODE_FALLBACKS_SHIFT = 8


def set_verbosity(level):
    """meep::verbosity of the native library (rank 0's "on time step" lines)."""
    lib().mnl_set_verbosity(int(level))


def get_verbosity():
    return lib().mnl_get_verbosity()
COMPONENT_NAMES = ["ex", "ey", "ez", "hx", "hy", "hz", "dx", "dy", "dz", "bx", "by", "bz"]


class GridVolume:
    """grid_volume for Cartesian D1 (Z), D2 (X,Y), D3 (X,Y,Z)."""

    def __init__(self, dim, n, a, io=(0, 0, 0)):
        self.dim = int(dim)
        self.has = [dim >= 2, dim >= 2, dim != 2]
        self.n = [int(n[d]) if self.has[d] else 0 for d in range(3)]
        self.io = [int(io[d]) if self.has[d] else 0 for d in range(3)]
        self.a = float(a)

    @classmethod
    def vol(cls, dim, sizes, a, center_origin=False):
        """vol1d/vol2d/vol3d (src/vec.cpp:904-931) [+ center_origin (vec.hpp:1150)]."""
        n = [0, 0, 0]
        if dim == 1:
            n[2] = int(sizes[0] * a + 0.5)
        elif dim == 2:
            n[0] = 1 if sizes[0] == 0 else int(sizes[0] * a + 0.5)
            n[1] = 1 if sizes[1] == 0 else int(sizes[1] * a + 0.5)
        else:
            n = [1 if s == 0 else int(s * a + 0.5) for s in sizes]
        io = [-(v - (v & 1)) for v in n] if center_origin else [0, 0, 0]
        return cls(dim, n, a, io)

    def shape(self):
        return tuple(self.n[d] + 1 for d in range(3) if self.has[d])

    def ntot(self):
        return int(np.prod(self.shape()))

    def shift(self, c, d):
        if not self.has[d]:
            return 0
        t = c // 3
        if t in (0, 2):
            return 1 if d == c % 3 else 0
        return 1 if d != c % 3 else 0

    def coords(self, c):
        axes = []
        for d in range(3):
            if self.has[d]:
                j = np.arange(self.n[d] + 1)
                axes.append((self.io[d] + 2 * j + self.shift(c, d)) * (0.5 / self.a))
        return np.meshgrid(*axes, indexing="ij")

    def center(self):
        """grid_volume::center() (src/vec.cpp:1089-1103)."""
        out = []
        for d in range(3):
            if self.has[d]:
                n = self.n[d] - (self.n[d] & 1)
                out.append((self.io[d] + n) * (0.5 / self.a))
            else:
                out.append(0.0)
        return out


class Structure:
    """meep::structure for one grid_volume (no symmetry, PML chunks implicit)."""

    def __init__(self, gv, courant=0.5):
        self.gv = gv
        self.courant = float(courant)
        na = (ctypes.c_int * 3)(*gv.n)
        ia = (ctypes.c_int * 3)(*gv.io)
        self.h = lib().mnl_structure_create(gv.dim, na, gv.a, self.courant, ia)
        if not self.h:
            raise RuntimeError(lib().mnl_last_error().decode())
        self._nsus = 0

    def __del__(self):
        if getattr(self, "h", None):
            lib().mnl_structure_destroy(self.h)
            self.h = None

    def add_pml(self, thickness, dirs=(0, 1, 2), sides=(0, 1), R=1e-15, mean_stretch=1.0):
        for d in dirs:
            for s in sides:
                check(lib().mnl_structure_add_pml(self.h, d, s, float(thickness), R, mean_stretch))

    def _arr(self, a):
        return np.ascontiguousarray(np.broadcast_to(a, self.gv.shape()), dtype=np.float64).ravel()

    def set_chi1inv(self, comp, d, arr):
        check(lib().mnl_structure_set_chi1inv(self.h, comp, d, None if arr is None else ptr(self._arr(arr))))

    def set_epsilon_fn(self, fn):
        """set_epsilon without averaging: chi1inv = 1/eps(location) per E component."""
        for c in (Ex, Ey, Ez):
            if self.gv.dim == 1 and c != Ex:
                continue
            self.set_chi1inv(c, c % 3, 1.0 / fn(*self.gv.coords(c)))

    def set_mu_fn(self, fn):
        """structure::set_mu without averaging: chi1inv of the H components =
        1/mu(location) (set_chi1inv(H_stuff), src/anisotropic_averaging.cpp:221-298)."""
        for c in (Hx, Hy, Hz):
            if self.gv.dim == 1 and c != Hy:
                continue
            self.set_chi1inv(c, c % 3, 1.0 / fn(*self.gv.coords(c)))

    def set_epsilon_geometry(self, objects, default_eps=1.0, use_anisotropic_averaging=True,
                             tol=1e-4, maxeval=100000, device=-1):
        """structure::set_epsilon(material_function &, use_anisotropic_averaging, tol,
        maxeval) (src/structure.cpp:397-401; subpixel averaging of
        src/anisotropic_averaging.cpp:58-298) for a material function made of
        geometric objects, computed on a HIP device.  objects: rows
        {kind, eps, cx, cy, cz, p0, p1, p2} (include/meep_nl_amd.h), later rows win."""
        o = np.ascontiguousarray(np.asarray(objects, dtype=np.float64).reshape(-1, 8))
        check(lib().mnl_structure_set_epsilon_geometry(
            self.h, int(device), o.shape[0], ptr(o) if o.shape[0] else None, float(default_eps),
            int(bool(use_anisotropic_averaging)), float(tol), int(maxeval)))

    def get_chi1inv(self, comp, d):
        """chi1inv[comp][d] over the whole cell (canonical layout); None if trivial."""
        out = np.empty(self.gv.shape(), dtype=np.float64)
        rc = lib().mnl_structure_get_chi1inv(self.h, comp, d, ptr(out))
        if rc == 1:
            return None
        check(rc)
        return out

    def set_chi2(self, comp, arr):
        check(lib().mnl_structure_set_chi2(self.h, comp, ptr(self._arr(arr))))

    def set_chi3(self, comp, arr):
        check(lib().mnl_structure_set_chi3(self.h, comp, ptr(self._arr(arr))))

    def set_conductivity(self, comp, arr):
        """structure::set_conductivity(c, C) (src/structure.cpp:868-905): D or B
        component (E / H name their D / B array; E values are multiplied by the
        diagonal chi1inv set so far).  None resets to zero."""
        a = None if arr is None else self._arr(arr)
        check(lib().mnl_structure_set_conductivity(self.h, comp, None if a is None else ptr(a)))

    def dump(self, fname):
        """structure::dump (src/structure_dump.cpp): the host-side material
        description (flat binary, not HDF5)."""
        check(lib().mnl_structure_dump(self.h, os.fsencode(fname)))

    def load(self, fname):
        """structure::load: replace the materials / PML / susceptibilities by a
        dumped description of the same grid volume (before creating fields)."""
        check(lib().mnl_structure_load(self.h, os.fsencode(fname)))

    def add_lorentzian(self, omega0, gamma, sigmas, drude=False):
        s = [None if v is None else self._arr(v) for v in sigmas]
        check(lib().mnl_structure_add_lorentzian(self.h, omega0, gamma, int(drude),
                                                 *[ptr(v) for v in s]))
        self._nsus += 1
        return self._nsus - 1

    def add_lorentzian_tensor(self, omega0, gamma, sigma, drude=False):
        """add_susceptibility with a sigma tensor (src/anisotropic_averaging.cpp:
        300-372): sigma[c][d] (3x3 nested, None = 0) per E component row c at c's
        Yee points; off-diagonal entries sampled half a pixel back along c."""
        arrs = [None if sigma[c][d] is None else self._arr(sigma[c][d])
                for c in range(3) for d in range(3)]
        ptrs = (dptr * 9)(*[ptr(a) if a is not None else None for a in arrs])
        check(lib().mnl_structure_add_lorentzian_tensor(self.h, float(omega0), float(gamma),
                                                         int(drude), ptrs))

    def add_magnetic_lorentzian(self, omega0, gamma, sigmas, drude=False):
        """add_susceptibility(sigma, H_stuff, lorentzian_susceptibility): diagonal
        sigma per H component at its Yee points (None = 0)."""
        s = [None if v is None else self._arr(v) for v in sigmas]
        check(lib().mnl_structure_add_magnetic_lorentzian(self.h, float(omega0), float(gamma),
                                                          int(drude), *[ptr(v) for v in s]))

    def set_box(self, kind, box, value, index=0):
        b = np.ascontiguousarray(box, dtype=np.float64)
        check(lib().mnl_structure_set_box(self.h, kind, index, ptr(b), float(value)))

    def set_nonlinear_mode(self, mode):
        """'fork' (default: chi2 through Newton-Raphson, chi3 inert) or 'upstream'
        (upstream Meep's Pade chi2/chi3 update, src/step_generic.cpp:546-553)."""
        m = {"fork": 0, "upstream": 1}[mode] if isinstance(mode, str) else int(mode)
        check(lib().mnl_structure_set_nonlinear_mode(self.h, m))


def _src_last_time(kind, params):
    """src_time::last_time(): gaussian float(peak_time + cutoff) with the cutoff
    shrink of gaussian_src_time(f, w, st, et) (src/sources.cpp:85-96,
    src/meep.hpp:1024); continuous end_time (src/meep.hpp:1046)."""
    if kind == 0:
        w, st, et = params[1], params[2], params[3]
        peak, cutoff = 0.5 * (st + et), (et - st) * 0.5
        while math.exp(-cutoff * cutoff / (2 * w * w)) < 1e-100:
            cutoff *= 0.9
        cutoff = float(np.float32(cutoff))
        return float(np.float32(peak + cutoff))
    return float(params[4])


class Fields:
    """meep::fields with use_real_fields() on one MI355X (or one z-slab of it)."""

    def __init__(self, structure, device=-1, rank=0, nranks=1, nccl_id=None, hub=None):
        self.s = structure
        self.gv = structure.gv
        if nranks > 1 and hub is not None:
            self.h = lib().mnl_fields_create_local(structure.h, device, rank, nranks, hub.h)
        elif nranks > 1:
            self.h = lib().mnl_fields_create_dist(structure.h, device, rank, nranks, nccl_id)
        else:
            self.h = lib().mnl_fields_create(structure.h, device)
        if not self.h:
            raise RuntimeError(lib().mnl_last_error().decode())
        self.rank, self.nranks = rank, nranks
        self._hub = hub  # the hub must outlive the fields of its slabs

    def __del__(self):
        if getattr(self, "h", None):
            lib().mnl_fields_destroy(self.h)
            self.h = None

    # -- boundaries
    def use_complex_fields(self):
        """The inverse of fields::use_real_fields (src/fields.cpp:140-160): a second set of
        every time-stepped array (the imaginary part), after which use_bloch takes any complex
        k.  Before use_bloch, sources, monitors, initialize_field and the first step."""
        check(lib().mnl_fields_use_complex_fields(self.h))

    @property
    def is_real(self):
        """fields::is_real: True until use_complex_fields()."""
        v = ctypes.c_int(1)
        check(lib().mnl_fields_is_real(self.h, ctypes.byref(v)))
        return bool(v.value)

    def use_bloch(self, d, k=0):
        """fields::use_bloch(d, k) (src/boundaries.cpp:88-103): both boundaries of direction d
        (0 X, 1 Y, 2 Z) become periodic with Bloch wavevector k (units of 2 pi; complex).  Real
        fields take k = 0 only; after use_complex_fields() any k.  Before sources, DFT monitors
        and the first step."""
        k = complex(k)
        check(lib().mnl_fields_use_bloch(self.h, int(d), k.real, k.imag))

    def boundary(self, d, side=0):
        """'periodic' or 'metallic': the boundary condition of one side of direction d."""
        v = ctypes.c_int(0)
        check(lib().mnl_fields_boundary(self.h, int(d), int(side), ctypes.byref(v)))
        return "periodic" if v.value == 0 else "metallic"

    # -- sources
    def add_point_source(self, comp, kind, params, pos, amp=1.0, is_integrated=False):
        p = np.ascontiguousarray(params, dtype=np.float64)
        pos = np.ascontiguousarray(list(pos) + [0.0] * (3 - len(pos)), dtype=np.float64)
        amp = complex(amp)
        check(lib().mnl_fields_add_point_source(self.h, comp, kind, ptr(p), len(p), ptr(pos),
                                                amp.real, amp.imag, int(is_integrated)))
        self._last_times = getattr(self, "_last_times", [])
        self._last_times.append(_src_last_time(kind, list(params)))

    def add_custom_source(self, comp, func, start, end, pos, amp=1.0, is_integrated=False):
        """custom_src_time(func, data, start, end) (src/meep.hpp:1059-1092): func(t) ->
        complex dipole, called on the host at every step.  One callback per Python
        function, so sources sharing a function merge as in custom_src_time::is_equal."""
        cbs = self.__dict__.setdefault("_custom_cbs", {})
        if id(func) not in cbs:
            def _cb(t, _data, re, im, func=func):
                v = complex(func(t))
                re[0] = v.real
                im[0] = v.imag
            cbs[id(func)] = (func, _lib.SRC_FUNC(_cb))
        cf = cbs[id(func)][1]
        pos = np.ascontiguousarray(list(pos) + [0.0] * (3 - len(pos)), dtype=np.float64)
        amp = complex(amp)
        check(lib().mnl_fields_add_custom_point_source(self.h, comp, cf, None, float(start),
                                                       float(end), ptr(pos), amp.real, amp.imag,
                                                       int(is_integrated)))
        self._last_times = getattr(self, "_last_times", [])
        self._last_times.append(float(np.float32(end)))

    def _amp_cb(self, amp_func):
        """ctypes callback for a volume source's amplitude function A(r) (r relative
        to the volume centre, 3 coordinates) -> complex; kept alive with the fields."""
        if amp_func is None:
            return _lib.AMP_FUNC()
        def _cb(rel, _data, re, im, f=amp_func):
            v = complex(f((rel[0], rel[1], rel[2])))
            re[0] = v.real
            im[0] = v.imag
        cb = _lib.AMP_FUNC(_cb)
        self.__dict__.setdefault("_amp_cbs", []).append(cb)
        return cb

    def add_volume_source(self, comp, kind, params, vmin, vmax, amp=1.0, is_integrated=False,
                          amp_func=None):
        """fields::add_volume_source(c, src, volume(vmin, vmax), A, amp)
        (src/sources.cpp:455-494); amp_func(r) -> complex, r relative to the centre."""
        p = np.ascontiguousarray(params, dtype=np.float64)
        lo = np.ascontiguousarray(list(vmin) + [0.0] * (3 - len(vmin)), dtype=np.float64)
        hi = np.ascontiguousarray(list(vmax) + [0.0] * (3 - len(vmax)), dtype=np.float64)
        amp = complex(amp)
        check(lib().mnl_fields_add_volume_source(self.h, comp, kind, ptr(p), len(p), ptr(lo),
                                                 ptr(hi), amp.real, amp.imag, int(is_integrated),
                                                 self._amp_cb(amp_func), None))
        self._last_times = getattr(self, "_last_times", [])
        self._last_times.append(_src_last_time(kind, list(params)))

    def add_custom_volume_source(self, comp, func, start, end, vmin, vmax, amp=1.0,
                                 is_integrated=False, amp_func=None):
        cbs = self.__dict__.setdefault("_custom_cbs", {})
        if id(func) not in cbs:
            def _cb(t, _data, re, im, func=func):
                v = complex(func(t))
                re[0] = v.real
                im[0] = v.imag
            cbs[id(func)] = (func, _lib.SRC_FUNC(_cb))
        lo = np.ascontiguousarray(list(vmin) + [0.0] * (3 - len(vmin)), dtype=np.float64)
        hi = np.ascontiguousarray(list(vmax) + [0.0] * (3 - len(vmax)), dtype=np.float64)
        amp = complex(amp)
        check(lib().mnl_fields_add_custom_volume_source(
            self.h, comp, cbs[id(func)][1], None, float(start), float(end), ptr(lo), ptr(hi),
            amp.real, amp.imag, int(is_integrated), self._amp_cb(amp_func), None))
        self._last_times = getattr(self, "_last_times", [])
        self._last_times.append(float(np.float32(end)))

    def add_gaussian_volume_source(self, comp, freq, width, start, end, vmin, vmax, amp=1.0,
                                   is_integrated=False, amp_func=None):
        self.add_volume_source(comp, 0, [freq, width, start, end], vmin, vmax, amp, is_integrated,
                               amp_func)

    def add_gaussian_source(self, comp, freq, width, start, end, pos, amp=1.0,
                            is_integrated=False):
        """gaussian_src_time(f, w, start, end) (src/sources.cpp:85-96)."""
        self.add_point_source(comp, 0, [freq, width, start, end], pos, amp, is_integrated)

    def add_continuous_source(self, comp, freq, width, start, end, slowness, pos, amp=1.0,
                              is_integrated=False):
        f = complex(freq)
        self.add_point_source(comp, 1, [f.real, f.imag, width, start, end, slowness], pos, amp,
                              is_integrated)

    def legacy_point_source(self, comp, freq, width, peaktime, cutoff, pos, amp):
        """Deprecated C++ fields::add_point_source(c, freq, width, peaktime, cutoff,
        vec, amp) (src/sources.cpp:189-211); C++ sources are integrated by default
        (src/meep.hpp:950-951), magnetic ones are not."""
        width = width / freq
        dt = self.dt
        cutoff = (1.0 / self.gv.a) + cutoff * width
        if peaktime <= 0.0:
            peaktime = self.t * dt + cutoff
        peaktime += (-dt * 0.5) if comp in (Hx, Hy, Hz) else dt
        self.add_gaussian_source(comp, freq, width, peaktime - cutoff, peaktime + cutoff, pos,
                                 amp, is_integrated=comp not in (Hx, Hy, Hz))

    def require_component(self, comp):
        check(lib().mnl_fields_require_component(self.h, comp))

    def initialize_field(self, comp, values):
        """fields::initialize_field(c, func) (src/initialize.cpp:135-161): values is
        the whole-cell array of func at the points of comp (real part used), or a
        callable f(*coords) vectorised over the coordinate arrays of comp."""
        if callable(values):
            values = values(*self.gv.coords(comp))
        if not self.is_real:  # imag(val) goes to part 1 (src/initialize.cpp:155-160)
            z = np.broadcast_to(values, self.gv.shape())
            re = np.ascontiguousarray(np.real(z), dtype=np.float64).ravel()
            im = np.ascontiguousarray(np.imag(z), dtype=np.float64).ravel()
            check(lib().mnl_fields_initialize_field_complex(self.h, comp, ptr(re), ptr(im),
                                                            re.size))
            return
        v = np.ascontiguousarray(np.real(np.broadcast_to(values, self.gv.shape())),
                                 dtype=np.float64).ravel()
        check(lib().mnl_fields_initialize_field(self.h, comp, ptr(v), v.size))

    def set_nan_check(self, every):
        """NaN / Inf guard cadence in steps (src/step.cpp:138-139 checks every step)."""
        check(lib().mnl_fields_set_nan_check(self.h, int(every)))

    def last_source_time(self):
        """fields::last_source_time (src/bands.cpp:35-41): latest src_time::last_time()."""
        return max([0.0] + getattr(self, "_last_times", []))

    # -- stepping
    def step(self, n=1):
        check(lib().mnl_fields_step(self.h, int(n)))

    def tune(self, reps=8):
        """Time the fused step's knobs over real steps and keep the fastest (mnl_fields_tune:
        the tile kernel's z-chunk length, then on one rank with polarization chunks the CUs
        of their general kernel beside the tile kernel; with temporal blocking the planes and
        widths of its two-step items and pairs against one-step stepping).  A run is two
        warm-up steps and r timed ones, r = reps rounded up to even: 6 runs for the z-chunk
        (automatic, 16, 20, 24, 32, 48), up to 6 for the CUs (0 and five splits), 38 for the
        two-step items (124 columns x automatic, 12, 16, 20, 24, 32, 40, 48, 64, 96, 128
        planes and 60 columns x automatic, 12 .. 48 planes: 19 candidates, forward and
        backward) and the three best again with 2 * reps timed steps, one for one-step
        stepping and one more with 2 * reps.  At most 2 + 51 * (2 + r) + 4 * (2 + 2 * reps)
        steps (112 + 59 * reps for even reps), results identical to plain stepping (round 6: 8 timed steps by default, 4 gave choices off by up to 10 %
        at 256^3).  Returns (zchunk, gen_cus); -1 = not tuned (not in the fused mode)."""
        z, g = ctypes.c_int(0), ctypes.c_int(0)
        check(lib().mnl_fields_tune(self.h, int(reps), ctypes.byref(z), ctypes.byref(g)))
        return z.value, g.value

    def _time(self):
        t = ctypes.c_longlong()
        dt = ctypes.c_double()
        check(lib().mnl_fields_time(self.h, ctypes.byref(t), ctypes.byref(dt)))
        return t.value, dt.value

    @property
    def t(self):
        return self._time()[0]

    @t.setter
    def t(self, value):  # the SWIG binding's fields.t assignment
        check(lib().mnl_fields_set_time(self.h, int(value)))

    def zero_fields(self):
        """fields::zero_fields (src/fields.cpp:638-664); DFT accumulators are kept."""
        check(lib().mnl_fields_zero_fields(self.h))

    def remove_sources(self):
        """fields::remove_sources (src/fields.cpp:601-610)."""
        check(lib().mnl_fields_remove_sources(self.h))
        self._last_times = []

    @property
    def dt(self):
        return self._time()[1]

    def time(self):
        t, dt = self._time()
        return t * dt

    def round_time(self):
        t, dt = self._time()
        return float(np.float32(t * dt))

    # -- energy (src/energy_and_flux.cpp:48-178)
    def _energy(self, which, vmin=None, vmax=None):
        out = ctypes.c_double()
        lo = None if vmin is None else np.ascontiguousarray(vmin, dtype=np.float64)
        hi = None if vmax is None else np.ascontiguousarray(vmax, dtype=np.float64)
        check(lib().mnl_fields_energy_in_box(self.h, which, ptr(lo), ptr(hi), ctypes.byref(out)))
        return out.value

    def electric_energy_in_box(self, vmin=None, vmax=None):
        """fields::electric_energy_in_box: sum over E comps of (1/2) integral E.D."""
        return self._energy(0, vmin, vmax)

    def magnetic_energy_in_box(self, vmin=None, vmax=None):
        """fields::magnetic_energy_in_box with the current (unsynchronized) B, H."""
        return self._energy(1, vmin, vmax)

    def field_energy_in_box(self, vmin=None, vmax=None):
        """fields::field_energy_in_box: electric + magnetic energy of B / H
        synchronized to E's time (synchronize_magnetic_fields)."""
        return self._energy(2, vmin, vmax)

    def field_energy(self):
        """fields::field_energy (src/energy_and_flux.cpp:48): the whole cell."""
        return self._energy(2)

    # -- monitors
    def get_field(self, comp, pos):
        pos = np.ascontiguousarray(list(pos) + [0.0] * (3 - len(pos)), dtype=np.float64)
        out = ctypes.c_double()
        check(lib().mnl_fields_get_field(self.h, comp, ptr(pos), ctypes.byref(out)))
        return out.value

    def get_field_complex(self, comp, pos):
        """fields::get_field(c, loc) (src/monitor.cpp:115-160) as a complex number; get_field
        returns its real part."""
        pos = np.ascontiguousarray(list(pos) + [0.0] * (3 - len(pos)), dtype=np.float64)
        out = np.zeros(2)
        check(lib().mnl_fields_get_field_complex(self.h, comp, ptr(pos), ptr(out)))
        return complex(out[0], out[1])

    def get_array(self, comp, part=0, cmplx=False):
        """The whole-cell array of comp: the real part (part 0), the imaginary part (part 1,
        complex fields only), or with cmplx=True both as a complex array."""
        if cmplx:
            re = self.get_array(comp, 0)
            return re + 1j * (0.0 if self.is_real else self.get_array(comp, 1))
        nt = lib().mnl_fields_ntot(self.h)
        out = np.zeros(nt, dtype=np.float64)
        check(lib().mnl_fields_copy_component_part(self.h, int(part), comp, ptr(out), nt))
        return out.reshape(self.gv.shape())

    def get_array_slice(self, comp, vmin, vmax, snap=False, part=0, cmplx=False):
        """fields::get_array_slice(volume, c) (src/array_slice.cpp:611-704) over
        [vmin, vmax] (3 coordinates): Centered-grid values, empty dimensions
        interpolated and collapsed; shape = kept directions in X, Y, Z order.  part selects
        the real (0) or the imaginary (1) part of complex fields; cmplx=True returns a complex
        array."""
        if cmplx:
            re = self.get_array_slice(comp, vmin, vmax, snap, 0)
            # (epsilon and mu are real: src/array_slice.cpp:385-408)
            derived = comp in (Dielectric, Permeability)
            im = 0.0 if self.is_real or derived else self.get_array_slice(comp, vmin, vmax, snap, 1)
            return re + 1j * im
        lo = np.ascontiguousarray(vmin, dtype=np.float64)
        hi = np.ascontiguousarray(vmax, dtype=np.float64)
        rank = ctypes.c_int(0)
        dims = (ctypes.c_longlong * 3)()
        check(lib().mnl_fields_array_slice_part(self.h, int(part), comp, ptr(lo), ptr(hi),
                                                int(snap), ctypes.byref(rank), dims, None, 0))
        shape = tuple(dims[k] for k in range(rank.value))
        out = np.zeros(int(np.prod(shape)) if shape else 1)
        check(lib().mnl_fields_array_slice_part(self.h, int(part), comp, ptr(lo), ptr(hi),
                                                int(snap), ctypes.byref(rank), dims, ptr(out),
                                                out.size))
        return out.reshape(shape) if shape else out[0]

    def center(self):
        return self.gv.center()

    # -- instrumentation
    def timers(self):
        out = np.zeros(6)
        check(lib().mnl_fields_timers(self.h, ptr(out)))
        return dict(zip(["FieldUpdateB", "FieldUpdateH", "FieldUpdateD", "FieldUpdateE",
                         "Sources", "BoundarySteppingHalo"], out.tolist()))

    def time_spent(self):
        """This rank's seconds per time sink, in meep::time_sink order
        (TIME_SINKS; mnl_fields_time_spent)."""
        out = np.zeros(len(TIME_SINKS))
        check(lib().mnl_fields_time_spent(self.h, ptr(out)))
        return out

    def reset_timers(self):
        check(lib().mnl_fields_reset_timers(self.h))

    def sum_to_all(self, values):
        """Sum of a float64 vector over the ranks of distributed fields (collective)."""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(lib().mnl_fields_allreduce(self.h, ptr(v), v.size))
        return v

    def nr_fallbacks(self):
        v = ctypes.c_longlong()
        check(lib().mnl_fields_nr_fallbacks(self.h, ctypes.byref(v)))
        return v.value

    def transport(self):
        """'single', 'rccl', 'ipc' or 'local' (how ghost planes travel)."""
        return lib().mnl_fields_transport(self.h).decode()

    def _mode(self):
        """The mnl_fields_mode word (MODE_* bits)."""
        v = ctypes.c_int()
        check(lib().mnl_fields_mode(self.h, ctypes.byref(v)))
        return v.value

    def fused_active(self):
        return bool(self._mode() & MODE_FUSED)

    def tile_mode(self):
        """True if the fused step runs as one tile kernel (lean + PML bodies): always, in the
        fused mode (it is the only fused step)."""
        return bool(self._mode() & MODE_TILE)

    def fused_concurrent(self):
        """True if the last fused step ran the polarization chunks' general kernel beside the
        tile kernel on a CU split: kernel_stats("tile") then spans both launches."""
        return bool(self._mode() & MODE_CONCURRENT)

    def fused_palette(self):
        """True if the fused kernel reads chi1inv through the byte palette."""
        return bool(self._mode() & MODE_PALETTE)

    def alloc_info(self):
        """(contiguous field allocations requested, requests that fell back)."""
        m = self._mode()
        return bool(m & MODE_CONTIG), (m >> MODE_FALLBACKS_SHIFT) & 255

    def set_fused(self, allow=True):
        check(lib().mnl_fields_set_fused(self.h, int(allow)))

    def set_profiling(self, on=True):
        check(lib().mnl_fields_set_profiling(self.h, int(on)))

    def kernel_stats(self, which=0):
        """(launches, total ms, algorithmic bytes per launch) of one kernel group since
        set_profiling: a name of KERNEL_STATS or its number (mnl_fields_kernel_stats)."""
        if isinstance(which, str):
            which = KERNEL_STATS[which]
        n = ctypes.c_longlong()
        ms = ctypes.c_double()
        b = ctypes.c_double()
        check(lib().mnl_fields_kernel_stats(self.h, which, ctypes.byref(n), ctypes.byref(ms),
                                            ctypes.byref(b)))
        return n.value, ms.value, b.value

    def set_temporal_blocking(self, on=True):
        """Allow / forbid stepping pairs of steps with the two-step kernel (identical
        results either way)."""
        check(lib().mnl_fields_set_temporal_blocking(self.h, 1 if on else 0))

    def set_schedule(self, which, value):
        """Scheduling option of the fused step (identical results): which is a name of SCHEDULE,
        value a count for the names of SCHEDULE_INT and a switch for the others.  What each
        option does, and its range: the MNL_SCHED_* enum of include/meep_nl_amd.h
        (mnl_fields_set_schedule)."""
        value = int(value) if which in SCHEDULE_INT else (1 if value else 0)
        check(lib().mnl_fields_set_schedule(self.h, SCHEDULE[which], value))

    def tb_info(self):
        """Temporal blocking of the current fused geometry: dict of
        active (the last call of >= 2 steps stepped in pairs), two-step own cells / border
        points / mixed-palette cells, rim cells / mixed-palette rim cells, item counts, the
        first item's planes, the narrow x-face strip items among the rim items, the
        two-step chunk setting (0: automatic), the most own columns of a two-step item and
        whether polarization chunks step inside the pairs (TB_INFO_KEYS)."""
        v = (ctypes.c_double * len(TB_INFO_KEYS))()
        check(lib().mnl_fields_tb_info(self.h, v, len(TB_INFO_KEYS)))
        flags = ("active", "enabled", "tb_pol")
        return {k: (bool(x) if k in flags else int(x)) for k, x in zip(TB_INFO_KEYS, v)}

    def traffic_model(self):
        b = ctypes.c_double()
        c = ctypes.c_double()
        check(lib().mnl_fields_traffic_model(self.h, ctypes.byref(b), ctypes.byref(c)))
        return b.value, c.value


    # -- DFT flux (fields::add_dft_flux, src/dft.cpp:578-640; dft_flux, src/dft.cpp:482-547)
    def dump(self, fname):
        """fields::dump (src/fields_dump.cpp:108-145): t and every per-point state
        array (one file per rank: fname.rank<r> when distributed)."""
        check(lib().mnl_fields_dump(self.h, os.fsencode(fname)))

    def load(self, fname):
        """fields::load (src/fields_dump.cpp:232-270) into fields built the same
        way (structure, sources, flux objects); resumes bit for bit."""
        check(lib().mnl_fields_load(self.h, os.fsencode(fname)))

    def add_dft_flux(self, regions, freqs, decimation=0):
        """regions: [(min xyz, max xyz, direction, weight)]; returns a handle.
        The DFT is accumulated on the GPU after every decimated step."""
        r = np.ascontiguousarray([list(lo) + list(hi) + [d, w] for lo, hi, d, w in regions],
                                 dtype=np.float64).ravel()
        f = np.ascontiguousarray(freqs, dtype=np.float64)
        h = ctypes.c_int()
        check(lib().mnl_fields_add_dft_flux(self.h, len(regions), ptr(r), ptr(f), len(f),
                                            int(decimation), ctypes.byref(h)))
        self._dft_nf = getattr(self, "_dft_nf", {})
        self._dft_nf[h.value] = len(f)
        return h.value

    def flux(self, h):
        """dft_flux::flux (src/dft.cpp:533-547), summed over ranks."""
        out = np.zeros(self._dft_nf[h], dtype=np.float64)
        check(lib().mnl_fields_dft_flux(self.h, h, ptr(out)))
        return out

    def _dft_n(self, h, which):
        # list 0's size (flux, fields, near2far: every list answers with it, as before);
        # the list's own for energy and force objects, whose lists differ in length
        n = ctypes.c_longlong()
        if h in getattr(self, "_dft_multi", ()):
            check(lib().mnl_fields_dft_list_size(self.h, h, int(which), ctypes.byref(n)))
        else:
            check(lib().mnl_fields_dft_size(self.h, h, ctypes.byref(n)))
        return n

    def dft_data(self, h, which):
        """DFT values of the E (0) or H (1) chunk list, list order (complex); points
        another rank owns read 0."""
        n = self._dft_n(h, which)
        out = np.zeros(2 * n.value, dtype=np.float64)
        check(lib().mnl_fields_dft_data(self.h, h, int(which), ptr(out), n.value))
        return out[0::2] + 1j * out[1::2]

    # -- DFT data of any DFT object (save_dft_hdf5 / load_dft_hdf5 / scale_dft, src/dft.cpp:401-496)
    def dft_get(self, h, which=0):
        """The values dft_data returns, gathered into list order on the GPU and copied for
        this list only (mnl_fields_dft_get); points another rank owns read 0."""
        n = self._dft_n(h, which)
        out = np.zeros(2 * n.value, dtype=np.float64)
        check(lib().mnl_fields_dft_get(self.h, h, int(which), ptr(out), n.value))
        return out.view(np.complex128)

    def dft_load(self, h, which, data, sign=1):
        """The list's values become sign * data (sign +-1; load_dft_hdf5, and with -1 the
        reference's load followed by scale_dfts(-1)).  data is the full list on every rank;
        a rank keeps the points it owns."""
        d = np.ascontiguousarray(data, dtype=np.complex128).ravel()
        check(lib().mnl_fields_dft_load(self.h, h, int(which), ptr(d.view(np.float64)), d.size,
                                        int(sign)))

    def dft_scale(self, h, s):
        """Every value of every list of the object times the complex s (scale_dfts)."""
        s = complex(s)
        check(lib().mnl_fields_dft_scale(self.h, h, s.real, s.imag))

    def dft_save(self, h, fname):
        """The object's lists to a flat binary file (collective: rank 0 writes the lists
        assembled over the ranks)."""
        check(lib().mnl_fields_dft_save(self.h, h, os.fsencode(fname)))

    def dft_load_file(self, h, fname, sign=1):
        """sign * the lists of a dft_save file into this object (every rank reads the file)."""
        check(lib().mnl_fields_dft_load_file(self.h, h, os.fsencode(fname), int(sign)))

    def dft_flush(self):
        """Accumulate every buffered DFT update now and wait for the device
        (mnl_fields_dft_flush; readers flush by themselves, updates stay buffered between
        step calls)."""
        check(lib().mnl_fields_dft_flush(self.h))

    # -- field probes and the DFT norm
    def add_probe(self, comp, pos):
        """get_field(comp, pos) recorded after every step on the device, in whatever stepping
        mode is active; returns a probe handle (not a DFT handle)."""
        pos = np.ascontiguousarray(list(pos) + [0.0] * (3 - len(pos)), dtype=np.float64)
        h = ctypes.c_int()
        check(lib().mnl_fields_add_probe(self.h, int(comp), ptr(pos), ctypes.byref(h)))
        return h.value

    def probe_read(self, h):
        """(t_first, values): the probe's values since the last read, oldest first, values[k]
        that of the state after t_first + k steps (collective; summed over the ranks).  Only
        the last 65536 steps are kept: t_first shows what was dropped."""
        n, t0 = ctypes.c_longlong(), ctypes.c_longlong()
        check(lib().mnl_fields_probe_read(self.h, h, 0, ctypes.byref(n), ctypes.byref(t0), None))
        out = np.zeros(max(n.value, 1), dtype=np.float64)
        check(lib().mnl_fields_probe_read(self.h, h, out.size, ctypes.byref(n), ctypes.byref(t0),
                                          ptr(out)))
        return t0.value, out[:n.value]

    def probe_reset(self, h):
        check(lib().mnl_fields_probe_reset(self.h, h))

    def remove_probe(self, h):
        check(lib().mnl_fields_remove_probe(self.h, h))

    def remove_probes(self):
        check(lib().mnl_fields_remove_probes(self.h))

    # -- LDOS spectra (dft_ldos)
    def add_ldos(self, freqs):
        """dft_ldos(freq): an LDOS object over the current and future sources; returns its
        handle (not a DFT handle)."""
        freqs = np.ascontiguousarray(np.atleast_1d(freqs), dtype=np.float64)
        h = ctypes.c_int()
        check(lib().mnl_fields_add_ldos(self.h, ptr(freqs), int(freqs.size), ctypes.byref(h)))
        self._ldos_nfreq = getattr(self, "_ldos_nfreq", {})
        self._ldos_nfreq[h.value] = int(freqs.size)
        return h.value

    def ldos_update(self, h):
        """dft_ldos::update(fields): one update of the current state."""
        check(lib().mnl_fields_ldos_update(self.h, h))

    def ldos_record(self, h, on):
        """While on, every step appends the update of the state after it (on the device, in
        whatever stepping mode is active)."""
        check(lib().mnl_fields_ldos_record(self.h, h, 1 if on else 0))

    def ldos_data(self, h):
        """(ldos[nfreq], F[nfreq] complex, J[nfreq] complex, overall_scale): dft_ldos::ldos(),
        F(), J() and overall_scale() (collective; buffered updates are accumulated first)."""
        nf = getattr(self, "_ldos_nfreq", {}).get(h, 1)
        ld = np.zeros(nf, dtype=np.float64)
        F = np.zeros(2 * nf, dtype=np.float64)
        J = np.zeros(2 * nf, dtype=np.float64)
        s = ctypes.c_double()
        check(lib().mnl_fields_ldos_data(self.h, h, ptr(ld), ptr(F), ptr(J), ctypes.byref(s)))
        return ld, F[0::2] + 1j * F[1::2], J[0::2] + 1j * J[1::2], s.value

    def ldos_points(self, h):
        """(comp[n], ijk[n, 3], amp[n] complex): the object's global point list in list order,
        the electric sources' points, then the magnetic ones' (a diagnostic)."""
        n = ctypes.c_longlong()
        check(lib().mnl_fields_ldos_points(self.h, h, 0, ctypes.byref(n), None, None, None))
        m = max(n.value, 1)
        comp = np.zeros(m, dtype=np.int32)
        ijk = np.zeros(3 * m, dtype=np.int32)
        amp = np.zeros(2 * m, dtype=np.float64)
        check(lib().mnl_fields_ldos_points(
            self.h, h, m, ctypes.byref(n), comp.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
            ijk.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ptr(amp)))
        k = n.value
        return comp[:k], ijk[:3 * k].reshape(k, 3), (amp[0::2] + 1j * amp[1::2])[:k]

    def remove_ldos(self, h):
        check(lib().mnl_fields_remove_ldos(self.h, h))
        getattr(self, "_ldos_nfreq", {}).pop(h, None)

    def remove_ldoses(self):
        check(lib().mnl_fields_remove_ldoses(self.h))
        self._ldos_nfreq = {}

    def dft_norm(self):
        """fields::dft_norm(): sqrt of the sum of |dft|^2 over every DFT object (collective)."""
        v = ctypes.c_double()
        check(lib().mnl_fields_dft_norm(self.h, ctypes.byref(v)))
        return v.value

    def dft_maxfreq(self):
        v = ctypes.c_double()
        check(lib().mnl_fields_dft_maxfreq(self.h, ctypes.byref(v)))
        return v.value

    def max_decimation(self):
        v = ctypes.c_int()
        check(lib().mnl_fields_max_decimation(self.h, ctypes.byref(v)))
        return v.value

    def dft_decimation(self, h):
        v = ctypes.c_int()
        check(lib().mnl_fields_dft_decimation(self.h, h, ctypes.byref(v)))
        return v.value

    # -- DFT fields (fields::add_dft_fields / get_dft_array, src/dft.cpp:889-903, 1240-1280)
    def add_dft_fields(self, comps, vmin, vmax, freqs, yee_grid=False, decimation=0):
        """E / H components over [vmin, vmax] on the centered grid (or each
        component's Yee grid); returns a handle (shared with the flux handles)."""
        cs = np.ascontiguousarray(comps, dtype=np.int32)
        lo = np.ascontiguousarray(vmin, dtype=np.float64)
        hi = np.ascontiguousarray(vmax, dtype=np.float64)
        f = np.ascontiguousarray(freqs, dtype=np.float64)
        h = ctypes.c_int()
        check(lib().mnl_fields_add_dft_fields(self.h, len(cs), cs.ctypes.data_as(
            ctypes.POINTER(ctypes.c_int)), ptr(lo), ptr(hi), ptr(f), len(f), int(bool(yee_grid)),
            int(decimation), ctypes.byref(h)))
        self._dft_nf = getattr(self, "_dft_nf", {})
        self._dft_nf[h.value] = len(f)
        return h.value

    def dft_array(self, h, comp, num_freq):
        """fields::get_dft_array(obj, comp, num_freq) for flux and fields handles:
        complex array over the object's volume, empty dimensions collapsed (an empty
        array when the object holds no chunk of comp).  Collective on several ranks."""
        rank = ctypes.c_int()
        dims = (ctypes.c_longlong * 3)()
        check(lib().mnl_fields_dft_array(self.h, h, comp, num_freq, ctypes.byref(rank), dims,
                                         None, 0))
        shape = tuple(dims[k] for k in range(rank.value))
        n = int(np.prod(shape)) if rank.value else 0
        out = np.zeros(2 * max(n, 1), dtype=np.float64)
        check(lib().mnl_fields_dft_array(self.h, h, comp, num_freq, ctypes.byref(rank), dims,
                                         ptr(out), n))
        if not rank.value:
            return np.zeros(0, dtype=np.complex128)
        return (out[0:2 * n:2] + 1j * out[1:2 * n:2]).reshape(shape)

    # -- energy and force (fields::add_dft_energy, src/dft.cpp:630-790; add_dft_force,
    # src/stress.cpp).  Lists: energy 0..3 = E, H, D, B; force 0..2 = offdiag1, offdiag2, diag.
    def _add_dft_regions(self, fn, regions, freqs, decimation):
        r = np.ascontiguousarray([list(lo) + list(hi) + [d, w] for lo, hi, d, w in regions],
                                 dtype=np.float64).ravel()
        f = np.ascontiguousarray(freqs, dtype=np.float64)
        h = ctypes.c_int()
        check(fn(self.h, len(regions), ptr(r), ptr(f), len(f), int(decimation), ctypes.byref(h)))
        self._dft_nf = getattr(self, "_dft_nf", {})
        self._dft_nf[h.value] = len(f)
        self._dft_multi = getattr(self, "_dft_multi", set()) | {h.value}
        return h.value

    def add_dft_energy(self, regions, freqs, decimation=0):
        """regions: [(min xyz, max xyz, direction, weight)], direction and weight ignored (as
        in the reference); returns a handle shared with the other DFT objects."""
        return self._add_dft_regions(lib().mnl_fields_add_dft_energy, regions, freqs, decimation)

    def add_dft_force(self, regions, freqs, decimation=0):
        """regions: [(min xyz, max xyz, force direction, weight)]; the normal is the region's."""
        return self._add_dft_regions(lib().mnl_fields_add_dft_force, regions, freqs, decimation)

    def dft_energy(self, h, which=2):
        """dft_energy::electric (0) / magnetic (1) / total (2) per frequency, summed on the
        GPU and over ranks."""
        out = np.zeros(getattr(self, "_dft_nf", {}).get(h, 1), dtype=np.float64)
        check(lib().mnl_fields_dft_energy(self.h, h, int(which), ptr(out)))
        return out

    def dft_force(self, h):
        """dft_force::force per frequency, summed on the GPU and over ranks."""
        out = np.zeros(getattr(self, "_dft_nf", {}).get(h, 1), dtype=np.float64)
        check(lib().mnl_fields_dft_force(self.h, h, ptr(out)))
        return out

    def dft_list_size(self, h, which=0):
        """Complex values (points x frequencies) of list `which` of a DFT object."""
        n = ctypes.c_longlong()
        check(lib().mnl_fields_dft_list_size(self.h, h, int(which), ctypes.byref(n)))
        return n.value

    def dft_points(self, h, which=0):
        """Per point of list `which` (the order of dft_get(h, which)): array (points, 5) of
        x, y, z, the component and the loop weight as applied (any DFT object)."""
        npts = self.dft_list_size(h, which) // self._dft_nf[h]
        out = np.zeros((max(npts, 1), 5), dtype=np.float64)
        check(lib().mnl_fields_dft_points(self.h, h, int(which), ptr(out), npts))
        return out[:npts]

    # -- near2far (fields::add_dft_near2far / dft_near2far::farfield, src/near2far.cpp)
    def add_dft_near2far(self, regions, freqs, decimation=0, nperiods=1):
        """regions: [(min xyz, max xyz, normal direction, weight)]; returns a handle shared
        with the other DFT objects (dft_data, dft_decimation, dft_array, dump / load)."""
        r = np.ascontiguousarray([list(lo) + list(hi) + [d, w] for lo, hi, d, w in regions],
                                 dtype=np.float64).ravel()
        f = np.ascontiguousarray(freqs, dtype=np.float64)
        h = ctypes.c_int()
        check(lib().mnl_fields_add_dft_near2far(self.h, len(regions), ptr(r), ptr(f), len(f),
                                                int(decimation), int(nperiods), ctypes.byref(h)))
        self._dft_nf = getattr(self, "_dft_nf", {})
        self._dft_nf[h.value] = len(f)
        return h.value

    def near2far_farfields(self, h, points):
        """dft_near2far::farfield at every point (one batched call, the transform runs on the
        GPU), summed over ranks: complex (npts, nfreq, 6) of Ex, Ey, Ez, Hx, Hy, Hz."""
        p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        nf = self._dft_nf.get(h, 1) if hasattr(self, "_dft_nf") else 1
        out = np.zeros((len(p), nf, 12), dtype=np.float64)
        check(lib().mnl_fields_near2far_farfields(self.h, h, len(p), ptr(p), ptr(out)))
        return out[..., 0::2] + 1j * out[..., 1::2]

    def near2far_points(self, h):
        """Per point of the list (the order of dft_data(h, 0)): array (points, 5) of x, y, z,
        the equivalent current's component c0 and the weight."""
        n = ctypes.c_longlong()
        check(lib().mnl_fields_dft_size(self.h, h, ctypes.byref(n)))
        npts = n.value // self._dft_nf[h]
        out = np.zeros((max(npts, 1), 5), dtype=np.float64)
        check(lib().mnl_fields_near2far_points(self.h, h, ptr(out), npts))
        return out[:npts]

    def near2far_medium(self, h):
        """(eps, mu) of the medium around the near2far surfaces."""
        e, m = ctypes.c_double(), ctypes.c_double()
        check(lib().mnl_fields_near2far_medium(self.h, h, ctypes.byref(e), ctypes.byref(m)))
        return e.value, m.value

    # -- mode coefficients of diffraction orders (fields::get_eigenmode_coefficients with a
    #    DiffractedPlanewave, src/mpb.cpp:925-1004)
    @staticmethod
    def _mode_args(modes, eig_vol, kpoint):
        """modes: [(g, axis or None, s, p)] -> the arrays of the two mode calls."""
        modes = list(modes)
        g = np.ascontiguousarray([[int(x) for x in m[0]] for m in modes],
                                 dtype=np.intc).reshape(-1, 3)
        axis = np.ascontiguousarray([[0.0, 0.0, 0.0] if m[1] is None else [float(x) for x in m[1]]
                                     for m in modes], dtype=np.float64).reshape(-1, 3)
        sp = np.ascontiguousarray([[complex(m[2]).real, complex(m[2]).imag, complex(m[3]).real,
                                    complex(m[3]).imag] for m in modes],
                                  dtype=np.float64).reshape(-1, 4)
        ev = None if eig_vol is None else np.ascontiguousarray(
            list(eig_vol[0]) + list(eig_vol[1]), dtype=np.float64)
        kp = None if kpoint is None else np.ascontiguousarray(kpoint, dtype=np.float64)
        return len(modes), g, axis, sp, ev, kp

    def mode_coefficients(self, h, modes, eig_vol=None, kpoint=None):
        """Coefficients of the flux object h in the plane waves modes = [(g, axis or None, s,
        p)] (one launch for all of them), eig_vol = (min xyz, max xyz) or None for the flux
        region, kpoint or None for 0.  Returns a dict: alpha complex (nmodes, nfreq, 2), vgrp
        and cscale (nmodes, nfreq), kpoints (nmodes, nfreq, 3), overlaps complex (nmodes,
        nfreq, 8): the four mode-flux and the four mode-mode sums of fields::get_overlap.
        The sums are taken on the GPU and summed over ranks (collective)."""
        nm, g, axis, sp, ev, kp = self._mode_args(modes, eig_vol, kpoint)
        nf = getattr(self, "_dft_nf", {}).get(h, 1)
        alpha = np.zeros((max(nm, 1), nf, 2), dtype=np.complex128)
        vgrp = np.zeros((max(nm, 1), nf))
        cscale = np.zeros((max(nm, 1), nf))
        kpts = np.zeros((max(nm, 1), nf, 3))
        ov = np.zeros((max(nm, 1), nf, 8), dtype=np.complex128)
        check(lib().mnl_fields_mode_coefficients(
            self.h, int(h), nm, g.ctypes.data_as(iptr), ptr(axis), ptr(sp), ptr(ev), ptr(kp),
            ptr(alpha.view(np.float64)), ptr(vgrp), ptr(kpts), ptr(cscale),
            ptr(ov.view(np.float64))))
        return {"alpha": alpha, "vgrp": vgrp, "kpoints": kpts, "cscale": cscale, "overlaps": ov}

    def mode_table(self, h, modes, eig_vol=None, kpoint=None):
        """The host table mode_coefficients hands to the GPU (diagnostic).  Returns a dict:
        dirs (da, db; db None when the plane is a line), coords_a, coords_b, layers (integer
        half-pixel coordinates; a position is coordinate * 0.5 / a), k (nmodes, nfreq, 3), vgrp,
        amp complex (nmodes, nfreq, 6), pa (nmodes, na), pb (nmodes, nb), pl (nmodes, nfreq, 2)."""
        nm, g, axis, sp, ev, kp = self._mode_args(modes, eig_vol, kpoint)
        nf = getattr(self, "_dft_nf", {}).get(h, 1)
        dims = np.zeros(4, dtype=np.int64)
        args = (self.h, int(h), nm, g.ctypes.data_as(iptr), ptr(axis), ptr(sp), ptr(ev), ptr(kp),
                dims.ctypes.data_as(llptr))
        check(lib().mnl_fields_mode_table(*args, None, None, None, None, None, None, None))
        na, nb, nl = int(dims[0]), int(dims[1]), int(dims[2])
        coords = np.zeros(na + nb + 2, dtype=np.intc)
        k = np.zeros((nm, nf, 3))
        vgrp = np.zeros((nm, nf))
        amp = np.zeros((nm, nf, 6), dtype=np.complex128)
        pa = np.zeros((nm, na), dtype=np.complex128)
        pb = np.zeros((nm, nb), dtype=np.complex128)
        pl = np.zeros((nm, nf, 2), dtype=np.complex128)
        check(lib().mnl_fields_mode_table(
            *args, coords.ctypes.data_as(iptr), ptr(k), ptr(vgrp), ptr(amp.view(np.float64)),
            ptr(pa.view(np.float64)), ptr(pb.view(np.float64)), ptr(pl.view(np.float64))))
        da, db = int(dims[3]) // 4, int(dims[3]) % 4
        return {"dirs": (da, None if db == 3 else db), "coords_a": coords[:na].copy(),
                "coords_b": coords[na:na + nb].copy(), "layers": coords[na + nb:na + nb + nl].copy(),
                "k": k, "vgrp": vgrp, "amp": amp, "pa": pa, "pb": pb, "pl": pl}


class LocalHub:
    """In-process slab group (mnl_local_hub_create): several z-slabs of one grid on
    one GPU, stepped by one host thread each."""

    def __init__(self, nranks):
        self.h = lib().mnl_local_hub_create(int(nranks))
        self.nranks = nranks

    def __del__(self):
        if getattr(self, "h", None):
            lib().mnl_local_hub_destroy(self.h)
            self.h = None


def device_count():
    n = ctypes.c_int()
    try:
        check(lib().mnl_device_count(ctypes.byref(n)))
    except (RuntimeError, OSError):
        return 0
    return n.value


def slab_range(ncell, rank, nranks):
    lo, hi = ctypes.c_int(), ctypes.c_int()
    check(lib().mnl_slab_range(ncell, rank, nranks, ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def unique_id():
    """128-byte RCCL unique id (rank 0; broadcast it to the other ranks)."""
    buf = ctypes.create_string_buffer(128)
    check(lib().mnl_comm_unique_id(buf))
    return buf.raw


def ipc_id(nranks):
    """128-byte id of the IPC transport (ranks sharing one GPU): creates the
    shared-memory control block; pass it as nccl_id to every rank's Fields."""
    buf = ctypes.create_string_buffer(128)
    check(lib().mnl_comm_ipc_id(buf, int(nranks)))
    raw = buf.raw
    # rank 0 unlinks the segment once every rank has joined (mnl_comm.cpp init_ipc); if
    # the group never forms (a rank fails before creating its Fields) the creator removes
    # it at exit instead, so nothing stays in /dev/shm
    import atexit

    def _unlink(r=raw):
        try:
            lib().mnl_comm_ipc_unlink(ctypes.create_string_buffer(r, 128))
        except Exception:
            pass
    atexit.register(_unlink)
    return raw


def pick_transport(world, local_rank):
    """Transport and device of one rank: RCCL over xGMI when every local rank has
    its own GPU, the IPC transport when ranks must share one.  Overrides:
    MNL_COMM=rccl|ipc, MNL_BENCH_DEVICE=<device for every rank>.
    Returns (transport, device)."""
    ndev = device_count()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    forced = os.environ.get("MNL_BENCH_DEVICE")
    device = int(forced) if forced else local_rank % max(ndev, 1)
    tr = os.environ.get("MNL_COMM")
    if not tr:
        tr = "ipc" if (forced or ndev < local_world) else "rccl"
    if tr not in ("ipc", "rccl"):
        raise ValueError(f"MNL_COMM must be ipc or rccl, not {tr!r}")
    return tr, device


def comm_id(nranks, transport):
    """Rank-0 side of communicator setup: 'rccl' or 'ipc'."""
    return ipc_id(nranks) if transport == "ipc" else unique_id()


def rccl_selftest(device=0, n=4096):
    """One-rank RCCL send/recv-to-self + allreduce through the slab Comm wrappers."""
    check(lib().mnl_comm_rccl_selftest(int(device), int(n)))


__all__ = ["GridVolume", "Structure", "Fields", "device_count", "unique_id", "ipc_id", "comm_id",
           "math"]
