// mnl_kernels_io.hip -- gfx950 kernels behind mnl_io.cpp and the ABI's getters: the energy
// integral, device layout -> a box of the whole-cell array (and the canonical layout), and the
// elementwise average / copy / fill, and the periodic ghost wrap (real fields, and complex
// fields with their Bloch phases), with their launchers.
#include "mnl_device.hpp"

namespace mnl {

__global__ void fill_kernel(double *p, double v, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

// Rank-owned entries of one component into a box of the whole-cell array
// (global indices blo..bhi per direction, strides bs); the launch covers the
// local index range lo.. of that box.
__global__ void to_box_kernel(double *dst, const double *src, const double *hsep, DevGrid g,
                              DevFields f, int type, int c, int l0, int l1, int l2, int n0, int n1,
                              long long bs0, long long bs1, long long bs2, int blo0, int blo1,
                              int blo2, int use_fb, const double *dsrc, const double *usrc) {
  const int i0 = l0 + blockIdx.x * MNL_BX + threadIdx.x;
  const int i1 = l1 + blockIdx.y * MNL_BY + threadIdx.y;
  const int i2 = l2 + blockIdx.z;
  if (i0 >= l0 + n0 || i1 >= l1 + n1) return;
  int ii[3] = {i0, i1, i2};
  Pt p;
  for (int d = 0; d < 3; d++) p.j[d] = g.ax[d] >= 0 ? ii[g.ax[d]] : 0;
  // rank-owned planes only along every axis (ghost entries are filled by
  // their owner; non-owned boundary entries are 0 in the reference).
  for (int d = 0; d < 3; d++) {
    if (g.ax[d] < 0) continue;
    int sh = shift_of(type, c, d);
    int lo = sh ? g.owned_lo_sh[d] : g.owned_lo_un[d];
    int hi = sh ? g.owned_hi_sh[d] : g.owned_hi_un[d];
    if (!sh && g.wall[d] && p.j[d] + g.off[d] == g.nglob[d]) hi = p.j[d];  // wall plane (= 0)
    if (!g.wall[d]) lo = 0, hi = g.nglob[d];  // periodic: the not-owned plane is the owner's copy
    if (p.j[d] < lo || p.j[d] > hi) return;
  }
  const long long bs[3] = {bs0, bs1, bs2};
  const int blo[3] = {blo0, blo1, blo2};
  long long cidx = 0;
  for (int d = 0; d < 3; d++)
    if (g.ax[d] >= 0) cidx += (long long)(p.j[d] + g.off[d] - blo[d]) * bs[d];
  long long i = (long long)i0 + i1 * g.st[1] + i2 * g.st[2];
  double v = src[i];
  if (hsep && (f.hall || pml_at(f, g, c, qcoord(g, p, T_H, c, c)))) v = hsep[i];
  p.idx = i;
  if (use_fb && type == T_E && e_implicit(f, g, c, p))  // fused: E = chi1inv * D (not stored)
    v = usrc ? (dsrc[i] * usrc[i]) : dsrc[i];
  dst[cidx] = v;
}

int k_fill(double *p, double v, size_t n, void *stream) {
  if (n == 0) return 0;
  size_t blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  fill_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(p, v, n);
  return rc();
}

// ------------------------------------------------------------- energy
// fields::field_energy_in_box(c, where) (src/energy_and_flux.cpp:67-83) ->
// integrate(2, {Ec, Dc} or {Hc, Bc}) on c's own Yee grid (src/integrate.cpp:
// 46-129): per point fv = 0.25 * (((f + f) + f) + f) of each field (offsets 0
// on a component grid), term = (fv0 * fv1) * IVEC_LOOP_WEIGHT.  One launch per
// reference chunk box; every thread accumulates its terms with TwoSum
// compensation, the workgroup combines (s, c) pairs in LDS and writes one pair.
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

__global__ __launch_bounds__(256) void energy_kernel(const double *A, const double *Asep,
                                                     const double *Bv, DevGrid g, DevFields f,
                                                     int type, int c, EBox box, const double *wt,
                                                     double *partial) {
  __shared__ double ls[256], lc[256];
  const long long n0 = box.dn[0], n1 = box.dn[1], n2 = box.dn[2];
  const long long ntot = n0 * n1 * n2;
  double s = 0.0, comp = 0.0;
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < ntot;
       q += (long long)gridDim.x * 256) {
    const long long a0 = q % n0, r = q / n0, a1 = r % n1, a2 = r / n1;
    const long long ia[3] = {a0, a1, a2};
    Pt p;
    long long li = 0;
    double w[3];
    for (int d = 0; d < 3; d++) {
      const int ax = g.ax[d];
      w[d] = 1.0;
      p.j[d] = 0;
      if (ax < 0) continue;
      p.j[d] = box.dlo[ax] + (int)ia[ax];
      li += (long long)p.j[d] * g.st[ax];
      w[d] = wt[box.wofs[ax] + ia[ax]];
    }
    // IVEC_LOOP_WEIGHT order: W(yd[2]) * (W(yd[1]) * (dV * W(yd[0])))
    const double wgt = w[box.yd[2]] * (w[box.yd[1]] * (box.dV0 * w[box.yd[0]]));
    const double *src = A;
    if (Asep && (f.hall || pml_at(f, g, c, qcoord(g, p, type, c, c)))) src = Asep;  // H separate here
    const double x = src[li], y = Bv[li];
    const double xv = 0.25 * (((x + x) + x) + x), yv = 0.25 * (((y + y) + y) + y);
    const double t = (xv * yv) * wgt;
    double ns, e;
    two_sum(s, t, ns, e);
    s = ns;
    comp += e;
  }
  ls[threadIdx.x] = s;
  lc[threadIdx.x] = comp;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if ((int)threadIdx.x < k) {
      double ns, e;
      two_sum(ls[threadIdx.x], ls[threadIdx.x + k], ns, e);
      ls[threadIdx.x] = ns;
      lc[threadIdx.x] = lc[threadIdx.x] + lc[threadIdx.x + k] + e;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = ls[0];
    partial[2 * blockIdx.x + 1] = lc[0];
  }
}

int k_energy(const double *A, const double *Asep, const double *Bv, const DevGrid &g,
             const DevFields &f, int type, int c, const EBox &box, const double *wt,
             double *partial, int nblocks, void *stream) {
  energy_kernel<<<nblocks, 256, 0, (hipStream_t)stream>>>(A, Asep, Bv, g, f, type, c, box, wt,
                                                          partial);
  return rc();
}

// average_with_backup (src/energy_and_flux.cpp:136-144): f = 0.5 * (f + backup)
__global__ void average_kernel(double *f, const double *bk, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = 0.5 * (f[i] + bk[i]);
}

int k_average(double *f, const double *bk, long long n, void *stream) {
  if (n <= 0) return 0;
  average_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(f, bk, n);
  return rc();
}

// lazy allocation on the first update_eh (src/update_eh.cpp:204-216): H starts
// as a copy of B, and the W auxiliary field as a copy of the field it shadows
__global__ void copy_kernel(double *dst, const double *src, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

int k_copy(double *dst, const double *src, long long n, void *stream) {
  if (n <= 0) return 0;
  copy_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(dst, src, n);
  return rc();
}

// ------------------------------------------------------------- periodic ghost wrap
// step_boundaries over the periodic connections (src/boundaries.cpp:347-623 with phase 1): one
// launch, one thread per ghost point (x faces) or pair of ghost points (y / z faces) of every
// listed array; the thread table is wrap_points (mnl_wrap.hpp).  Sources are owned points, so
// no thread reads what another one writes.
__global__ __launch_bounds__(256) void wrap_kernel(WrapArgs w, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  int arr;
  long long dst[2], src[2];
  const int np = wrap_points(w, t, arr, dst, src);
  if (np == 0) return;
  double *p = w.a[arr].p;
  if (np == 2 && dst[1] == dst[0] + 1 && src[1] == src[0] + 1 &&
      (((unsigned long long)(p + dst[0]) | (unsigned long long)(p + src[0])) & 15ull) == 0) {
    *reinterpret_cast<double2 *>(p + dst[0]) = *reinterpret_cast<const double2 *>(p + src[0]);
    return;
  }
  for (int k = 0; k < np; k++) p[dst[k]] = p[src[k]];
}

int k_wrap(const WrapArgs &w, void *stream) {
  if (w.n <= 0 || w.n > WRAP_MAXA || w.fstart[3] <= 0) return w.n > WRAP_MAXA ? 2 : 0;
  for (int a = 0; a < 3; a++)
    if (w.per[a] && w.N[a] < 2) return 2;
  const long long total = w.fstart[3] * w.n;
  wrap_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, total);
  return rc();
}

// Complex fields: the same connections with the Bloch phase of
// fields::process_incoming_chunk_data (src/step.cpp:173-197) over pairs of arrays (part 0 =
// real, part 1 = imaginary).  Each thread classifies its points' phases as connect_the_chunks
// does (src/boundaries.cpp:402-404): exactly 1 is a copy, exactly -1 a negation (multiplying by
// (1, 0) would change the sign of a zero), anything else the complex product with two roundings
// per part (the file is built without contraction).  Same thread table and access shapes as
// wrap_kernel; sources are owned points of either part.  wrap_phase_apply: mnl_wrap.hpp.

__global__ __launch_bounds__(256) void wrap_phase_kernel(WrapPhaseArgs A, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  int arr;
  long long dst[2], src[2];
  const int np = wrap_points(A.w, t, arr, dst, src);
  if (np == 0) return;
  double *p = A.w.a[arr].p, *q = A.q[arr];
  const int sh = A.w.a[arr].sh;
  if (np == 2 && dst[1] == dst[0] + 1 && src[1] == src[0] + 1 &&
      (((unsigned long long)(p + dst[0]) | (unsigned long long)(p + src[0]) |
        (unsigned long long)(q + dst[0]) | (unsigned long long)(q + src[0])) & 15ull) == 0) {
    const double2 vr = *reinterpret_cast<const double2 *>(p + src[0]);
    const double2 vi = *reinterpret_cast<const double2 *>(q + src[0]);
    double2 re, im;
    wrap_phase_apply(A.ph[wrap_phase_index(A.w, sh, dst[0])], vr.x, vi.x, re.x, im.x);
    wrap_phase_apply(A.ph[wrap_phase_index(A.w, sh, dst[1])], vr.y, vi.y, re.y, im.y);
    *reinterpret_cast<double2 *>(p + dst[0]) = re;
    *reinterpret_cast<double2 *>(q + dst[0]) = im;
    return;
  }
  for (int k = 0; k < np; k++) {
    double re, im;
    wrap_phase_apply(A.ph[wrap_phase_index(A.w, sh, dst[k])], p[src[k]], q[src[k]], re, im);
    p[dst[k]] = re;
    q[dst[k]] = im;
  }
}

int k_wrap_phase(const WrapPhaseArgs &A, void *stream) {
  const WrapArgs &w = A.w;
  if (w.n <= 0 || w.n > WRAP_MAXA || w.fstart[3] <= 0) return w.n > WRAP_MAXA ? 2 : 0;
  for (int a = 0; a < 3; a++)
    if (w.per[a] && w.N[a] < 2) return 2;
  for (int k = 0; k < w.n; k++)
    if (!w.a[k].p || !A.q[k]) return 2;
  const long long total = w.fstart[3] * w.n;
  wrap_phase_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(A, total);
  return rc();
}

int k_to_box(double *dst, const double *src, const double *hsep, const DevGrid &g, int comp_type,
             int comp_dir, const DevFields &f, const Box *fusedF, const double *dsrc,
             const double *usrc, const int blo[3], const int bhi[3], const long long bs[3],
             void *stream) {
  (void)fusedF;
  int l[3] = {0, 0, 0}, n[3] = {1, 1, 1};
  for (int d = 0; d < 3; d++) {
    const int a = g.ax[d];
    if (a < 0) continue;
    const int lo = std::max(blo[d] - g.off[d], 0), hi = std::min(bhi[d] - g.off[d], g.N[a] - 1);
    if (hi < lo) return 0;
    l[a] = lo;
    n[a] = hi - lo + 1;
  }
  int bl[3] = {0, 0, 0};
  long long bst[3] = {0, 0, 0};
  for (int d = 0; d < 3; d++)
    if (g.ax[d] >= 0) bl[d] = blo[d], bst[d] = bs[d];
  dim3 grd((n[0] + MNL_BX - 1) / MNL_BX, (n[1] + MNL_BY - 1) / MNL_BY, n[2]);
  to_box_kernel<<<grd, dim3(MNL_BX, MNL_BY), 0, (hipStream_t)stream>>>(
      dst, src, hsep, g, f, comp_type, comp_dir, l[0], l[1], l[2], n[0], n[1], bst[0], bst[1],
      bst[2], bl[0], bl[1], bl[2], fusedF ? 1 : 0, dsrc, usrc);
  return rc();
}

int k_to_canonical(double *dst, const double *src, const double *hsep, const DevGrid &g,
                   int comp_type, int comp_dir, const DevFields &f, const Box *fusedF,
                   const double *dsrc, const double *usrc, void *stream) {
  long long cs[3];
  canon_strides(g, cs);
  int blo[3] = {0, 0, 0}, bhi[3] = {0, 0, 0};
  for (int d = 0; d < 3; d++)
    if (g.ax[d] >= 0) bhi[d] = g.nglob[d];
  return k_to_box(dst, src, hsep, g, comp_type, comp_dir, f, fusedF, dsrc, usrc, blo, bhi, cs,
                  stream);
}

}  // namespace mnl
