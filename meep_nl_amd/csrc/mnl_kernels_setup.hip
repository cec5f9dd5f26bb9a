// mnl_kernels_setup.hip -- gfx950 kernels launched once while a structure or a fields object
// is set up (mnl_setup.cpp, the fused-step planning, initialize_field): subpixel averaging of
// chi1inv, box fills, the nonzero box of a susceptibility, the chi1inv palette indices,
// canonical layout -> device layout, and their launchers.
#include "mnl_device.hpp"

namespace mnl {

// canonical (Z fastest, whole cell) <-> device layout (rank-local box)
__global__ void from_canonical_kernel(double *dst, const double *src, DevGrid g, long long cs0,
                                      long long cs1, long long cs2) {
  int i0 = blockIdx.x * MNL_BX + threadIdx.x;
  int i1 = blockIdx.y * MNL_BY + threadIdx.y;
  int i2 = blockIdx.z;
  if (i0 >= g.N[0] || i1 >= g.N[1]) return;
  int ii[3] = {i0, i1, i2};
  long long cidx = 0;
  long long cs[3] = {cs0, cs1, cs2};
  for (int d = 0; d < 3; d++)
    if (g.ax[d] >= 0) cidx += (long long)(ii[g.ax[d]] + g.off[d]) * cs[d];
  dst[(long long)i0 + i1 * g.st[1] + i2 * g.st[2]] = src[cidx];
}

__global__ void box_fill_kernel(double *dst, DevGrid g, int type, int c, double x0, double x1,
                                double y0, double y1, double z0, double z1, double value,
                                int invert, double a, int io0, int io1, int io2) {
  int i0 = blockIdx.x * MNL_BX + threadIdx.x;
  int i1 = blockIdx.y * MNL_BY + threadIdx.y;
  int i2 = blockIdx.z;
  if (i0 >= g.N[0] || i1 >= g.N[1]) return;
  int ii[3] = {i0, i1, i2};
  double lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
  int io[3] = {io0, io1, io2};
  for (int d = 0; d < 3; d++) {
    if (g.ax[d] < 0) continue;
    int jj = ii[g.ax[d]] + g.off[d];
    double pos = (io[d] + 2 * jj + shift_of(type, c, d)) * (0.5 * (1.0 / a));
    if (pos < lo[d] || pos > hi[d]) return;
  }
  dst[(long long)i0 + i1 * g.st[1] + i2 * g.st[2]] = invert ? 1.0 / value : value;
}

// ------------------------------------------------------ subpixel averaging
// structure_chunk::set_chi1inv with a material_function (src/anisotropic_averaging.cpp:
// 221-298) over a list of geometric objects of isotropic permittivity (later objects
// win): per point the rownum'th row of the effective tensor at dV(here) (diagonal
// entry) and at dV(here - shift1) (off-diagonal entries), material_function::
// eff_chi1inv_row / normal_vector (58-219), in the reference's operation order.
__device__ double geo_chi1p1(const AvgArgs &A, const double r[3]) {
  for (int o = A.nobj - 1; o >= 0; o--) {
    const GeoObj &g = A.objs[o];
    const double dx = r[0] - g.c[0], dy = r[1] - g.c[1], dz = r[2] - g.c[2];
    bool in;
    if (g.kind == 0) {
      in = fabs(dx) <= 0.5 * g.p[0] && fabs(dy) <= 0.5 * g.p[1] && fabs(dz) <= 0.5 * g.p[2];
    } else if (g.kind == 1) {
      in = dx * dx + dy * dy + dz * dz <= g.p[0] * g.p[0];
    } else {
      const int ax = (int)g.p[2];
      const double da = ax == 0 ? dx : ax == 1 ? dy : dz;
      const double u = ax == 0 ? dy : dx, v = ax == 2 ? dy : dz;
      in = fabs(da) <= 0.5 * g.p[1] && u * u + v * v <= g.p[0] * g.p[0];
    }
    if (in) return g.eps;
  }
  return A.default_eps;
}

__device__ void eff_chi1inv_row(const AvgArgs &A, const double vmin[3], const double vmax[3],
                                double row[3]) {
  const int rownum = A.c;
  double cen[3] = {0, 0, 0};
  for (int k = 0; k < A.ndir; k++) {
    const int d = A.dirs[k];
    cen[d] = (vmin[d] + vmax[d]) * 0.5;
  }
  double meps = 1, minveps = 1;
  double grad[3] = {0, 0, 0};
  if (A.maxeval) {
    // normal_vector: sphere quadrature of diameter R around the centre
    double R = 0.0;
    for (int k = 0; k < A.ndir; k++) R = fmax(R, vmax[A.dirs[k]] - vmin[A.dirs[k]]);
    const int nd = A.ndir, min_iters = 1 << nd;
    const double *q = A.quad + (nd - 1) * AVG_MAXQ * 4;
    double prev = 0;
    bool break_early = true, uniform = false;
    for (int i = 0; i < A.nq[nd - 1]; ++i) {
      const double w = q[4 * i + 3];
      double pt[3] = {0, 0, 0};
      if (nd == 1) {
        pt[2] = cen[2] + q[4 * i + 2] * R;
      } else {
        for (int k = 0; k < nd; k++) pt[k] = cen[k] + q[4 * i + k] * R;
      }
      const double val = geo_chi1p1(A, pt);
      if (i > 0 && i < min_iters) {
        if (val != prev) break_early = false;
        if (i == min_iters - 1 && break_early) {
          uniform = true;
          break;
        }
      }
      prev = val;
      for (int k = 0; k < nd; k++) {
        const int d = A.dirs[k];
        grad[d] += (pt[d] - cen[d]) * (w * val);
      }
    }
    double g2 = 0.0;
    for (int k = 0; k < nd; k++) g2 += grad[A.dirs[k]] * grad[A.dirs[k]];
    if (!uniform && !(sqrt(g2) < 1e-8)) {
      double dd[3] = {0, 0, 0};
      for (int k = 0; k < nd; k++) dd[A.dirs[k]] = vmax[A.dirs[k]] - vmin[A.dirs[k]];
      int ms = 10, iter = 0;
      double old_meps = 0, old_minveps = 0;
      bool trivial = false;
      for (;;) {
        const bool go = nd == 3 ? (fabs(meps - old_meps) > A.tol * fabs(old_meps)) &&
                                      (fabs(minveps - old_minveps) > A.tol * fabs(old_minveps))
                                : (fabs(meps - old_meps) > A.tol * old_meps) &&
                                      (fabs(minveps - old_minveps) > A.tol * old_minveps);
        if (!go) break;
        old_meps = meps;
        old_minveps = minveps;
        meps = minveps = 0;
        if (nd == 3) {
          for (int k = 0; k < ms && !trivial; k++)
            for (int j = 0; j < ms && !trivial; j++)
              for (int i = 0; i < ms; i++) {
                const double pt[3] = {vmin[0] + i * dd[0] / ms, vmin[1] + j * dd[1] / ms,
                                      vmin[2] + k * dd[2] / ms};
                const double ep = geo_chi1p1(A, pt);
                if (ep < 0) {
                  trivial = true;
                  break;
                }
                meps += ep;
                minveps += 1 / ep;
              }
          if (trivial) break;
          meps /= ms * ms * ms;
          minveps /= ms * ms * ms;
          ms *= 2;
          if (A.maxeval && (iter += ms * ms * ms) >= A.maxeval) break;
        } else if (nd == 2) {
          for (int j = 0; j < ms && !trivial; j++)
            for (int i = 0; i < ms; i++) {
              const double pt[3] = {vmin[0] + i * dd[0] / ms, vmin[1] + j * dd[1] / ms, 0.0};
              const double ep = geo_chi1p1(A, pt);
              if (ep < 0) {
                trivial = true;
                break;
              }
              meps += ep;
              minveps += 1 / ep;
            }
          if (trivial) break;
          meps /= ms * ms;
          minveps /= ms * ms;
          ms *= 2;
          if (A.maxeval && (iter += ms * ms) >= A.maxeval) break;
        } else {
          bool neg = false;
          for (int i = 0; i < ms; i++) {
            const double pt[3] = {0.0, 0.0, vmin[2] + i * dd[2] / ms};
            const double ep = geo_chi1p1(A, pt);
            if (ep < 0) {
              meps = geo_chi1p1(A, cen);
              minveps = 1 / meps;
              neg = true;
              break;
            }
            meps += ep;
            minveps += 1 / ep;
          }
          if (neg) break;
          meps /= ms;
          minveps /= ms;
          ms *= 2;
          if (A.maxeval && (iter += ms * ms) >= A.maxeval) break;
        }
      }
      if (!trivial) {
        double n[3] = {0, 0, 0};
        const double nabsinv = 1.0 / sqrt(g2);
        for (int k = 0; k < nd; k++) n[A.dirs[k]] = grad[A.dirs[k]] * nabsinv;
        for (int i = 0; i < 3; ++i) row[i] = n[rownum] * n[i] * (minveps - 1 / meps);
        row[rownum] += 1 / meps;
        return;
      }
    }
  }
  row[0] = row[1] = row[2] = 0.0;
  row[rownum] = 1 / geo_chi1p1(A, cen);
}

__global__ void avg_chi1inv_kernel(AvgArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.ntot) return;
  // canonical index -> point (z fastest, then y, then x)
  int idx[3] = {0, 0, 0};
  long long r = i;
  for (int d = 2; d >= 0; d--)
    if (A.has[d]) {
      idx[d] = (int)(r % (A.n[d] + 1));
      r /= A.n[d] + 1;
    }
  const double h = 0.5 * A.inva;  // grid_volume::dV: hinva = 0.5 * inva * diameter (1.0)
  double vmin[3] = {0, 0, 0}, vmax[3] = {0, 0, 0}, omin[3] = {0, 0, 0}, omax[3] = {0, 0, 0};
  for (int k = 0; k < A.ndir; k++) {
    const int d = A.dirs[k];
    const int here = A.io[d] + 2 * idx[d] + (d == A.c ? 1 : 0);
    const double hp = here * (0.5 * A.inva), hm = (here - (d == A.c ? 1 : 0)) * (0.5 * A.inva);
    vmax[d] = hp + h;
    vmin[d] = hp - h;
    omax[d] = hm + h;  // here - shift1 (E: shifted back half a pixel along c)
    omin[d] = hm - h;
  }
  double row[3];
  eff_chi1inv_row(A, vmin, vmax, row);
  if (A.out[A.c]) A.out[A.c][i] = row[A.c];
  bool off = false;
  for (int d = 0; d < 3; d++) off = off || (d != A.c && A.out[d]);
  if (!off) return;
  eff_chi1inv_row(A, omin, omax, row);
  for (int d = 0; d < 3; d++)
    if (d != A.c && A.out[d]) A.out[d][i] = row[d];
}

// chi1inv palette indices over box F: uidx[i] = idx0 | idx1 << 8 | idx2 << 16,
// tab[c*256 + idx] == u[c][i] exactly; *bad != 0 if some value is missing.
__global__ void build_uidx_kernel(unsigned *uidx, const double *u0, const double *u1,
                                  const double *u2, const double *tab, int n0, int n1, int n2,
                                  Box F, long long st1, long long st2, int *bad) {
  const int x = F.lo[0] + blockIdx.x * blockDim.x + threadIdx.x, y = F.lo[1] + blockIdx.y,
            z = F.lo[2] + blockIdx.z;
  if (x > F.hi[0]) return;
  const long long i = x + y * st1 + z * st2;
  const double *u[3] = {u0, u1, u2};
  const int n[3] = {n0, n1, n2};
  unsigned w = 0;
  for (int c = 0; c < 3; c++) {
    // exact match on the bit pattern (table sorted by bit pattern on the host)
    const unsigned long long v = (unsigned long long)__double_as_longlong(u[c][i]);
    const double *t = tab + 256 * c;
    int lo = 0, hi = n[c] - 1, hit = -1;
    while (lo <= hi) {
      const int mid = (lo + hi) >> 1;
      const unsigned long long tm = (unsigned long long)__double_as_longlong(t[mid]);
      if (tm == v) {
        hit = mid;
        break;
      }
      if (tm < v)
        lo = mid + 1;
      else
        hi = mid - 1;
    }
    if (hit < 0) {
      atomicOr(bad, 1);
      hit = 0;
    }
    w |= (unsigned)hit << (8 * c);
  }
  uidx[i] = w;
}

int k_build_uidx(unsigned *uidx, const double *const u[3], const double *tab, const int n[3],
                 const Box &F, long long st1, long long st2, int *bad, void *stream) {
  if (empty(F)) return 0;
  dim3 grd((F.hi[0] - F.lo[0] + 1 + 255) / 256, F.hi[1] - F.lo[1] + 1, F.hi[2] - F.lo[2] + 1);
  build_uidx_kernel<<<grd, 256, 0, (hipStream_t)stream>>>(uidx, u[0], u[1], u[2], tab, n[0], n[1],
                                                          n[2], F, st1, st2, bad);
  return rc();
}

int k_from_canonical(double *dst, const double *src, const DevGrid &g, int comp_type, int comp_dir,
                     int zlo_glob, void *stream) {
  (void)comp_type;
  (void)comp_dir;
  (void)zlo_glob;
  long long cs[3];
  canon_strides(g, cs);
  dim3 grd((g.N[0] + MNL_BX - 1) / MNL_BX, (g.N[1] + MNL_BY - 1) / MNL_BY, g.N[2]);
  from_canonical_kernel<<<grd, dim3(MNL_BX, MNL_BY), 0, (hipStream_t)stream>>>(dst, src, g, cs[0],
                                                                               cs[1], cs[2]);
  return rc();
}

// fields::initialize_field (src/initialize.cpp:135-161): every point of the
// rank's array (ghost planes included: LOOP_OVER_VOL covers each chunk's whole
// array) gets += v; then zero_metal (src/boundaries.cpp:304-339) zeroes the owned
// points on the metallic high wall of each unshifted direction.  alt != null (H
// after its lazy allocation): the H array holds the value only where H is
// separate (PML chunk along c, src/update_eh.cpp:204-209), elsewhere H == B.
__global__ void init_add_kernel(double *dst, double *alt, const double *src, DevGrid g,
                                DevFields f, int type, int c, long long cs0, long long cs1,
                                long long cs2) {
  int i0 = blockIdx.x * MNL_BX + threadIdx.x;
  int i1 = blockIdx.y * MNL_BY + threadIdx.y;
  int i2 = blockIdx.z;
  if (i0 >= g.N[0] || i1 >= g.N[1]) return;
  int ii[3] = {i0, i1, i2};
  Pt p;
  long long cidx = 0;
  const long long cs[3] = {cs0, cs1, cs2};
  bool wall = false;
  for (int d = 0; d < 3; d++) {
    p.j[d] = g.ax[d] >= 0 ? ii[g.ax[d]] : 0;
    if (g.ax[d] < 0) continue;
    cidx += (long long)(p.j[d] + g.off[d]) * cs[d];
    if (!shift_of(type, c, d) && g.wall[d] && p.j[d] + g.off[d] == g.nglob[d]) wall = true;
  }
  double *t = dst;
  bool sep = pml_at(f, g, c, qcoord(g, p, type, c, c));
  if (f.hall && alt && !sep) {  // H-side materials: H separate in this point's chunk?
    int rz = 0;
    for (int e = 0; e < 3; e++) rz = rz * 3 + (g.ax[e] >= 0 ? f.zone[e][qcoord(g, p, type, c, e)] : 1);
    sep = f.hsep_all || ((f.hsep_zone[rz] >> c) & 1);
  }
  if (alt && !sep) t = alt;
  const long long li = (long long)i0 + i1 * g.st[1] + i2 * g.st[2];
  const double v = wall ? 0.0 : t[li] + src[cidx];
  t[li] = v;
  if (f.hall && alt && !sep) dst[li] = v;  // the H copy of an aliasing chunk follows B
}

int k_init_add(double *dst, double *alt, const double *src, const DevGrid &g, const DevFields &f,
               int comp_type, int comp_dir, void *stream) {
  long long cs[3];
  canon_strides(g, cs);
  dim3 grd((g.N[0] + MNL_BX - 1) / MNL_BX, (g.N[1] + MNL_BY - 1) / MNL_BY, g.N[2]);
  init_add_kernel<<<grd, dim3(MNL_BX, MNL_BY), 0, (hipStream_t)stream>>>(
      dst, alt, src, g, f, comp_type, comp_dir, cs[0], cs[1], cs[2]);
  return rc();
}

__global__ void nonzero_box_kernel(const double *a0, const double *a1, const double *a2,
                                   DevGrid g, int *box) {
  int i0 = blockIdx.x * MNL_BX + threadIdx.x;
  int i1 = blockIdx.y * MNL_BY + threadIdx.y;
  int i2 = blockIdx.z;
  if (i0 >= g.N[0] || i1 >= g.N[1]) return;
  const long long i = (long long)i0 + i1 * g.st[1] + i2 * g.st[2];
  const bool nz = (a0 && a0[i] != 0.0) || (a1 && a1[i] != 0.0) || (a2 && a2[i] != 0.0);
  if (!nz) return;
  const int ii[3] = {i0, i1, i2};
  for (int d = 0; d < 3; d++) {  // per direction, like Pt::j
    const int j = g.ax[d] >= 0 ? ii[g.ax[d]] : 0;
    atomicMin(box + d, j);
    atomicMax(box + 3 + d, j);
  }
}

int k_nonzero_box(const double *const a[3], const DevGrid &g, int *box, void *stream) {
  dim3 grd((g.N[0] + MNL_BX - 1) / MNL_BX, (g.N[1] + MNL_BY - 1) / MNL_BY, g.N[2]);
  nonzero_box_kernel<<<grd, dim3(MNL_BX, MNL_BY), 0, (hipStream_t)stream>>>(a[0], a[1], a[2], g,
                                                                           box);
  return rc();
}

int k_avg_chi1inv(const AvgArgs &a, void *stream) {
  if (a.ntot <= 0) return 0;
  avg_chi1inv_kernel<<<(unsigned)((a.ntot + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
  return rc();
}

int k_box_fill(double *dst, const DevGrid &g, int comp_type, int comp_dir, const double *lo,
               const double *hi, double value, int invert, double a, const int *io, void *stream) {
  dim3 grd((g.N[0] + MNL_BX - 1) / MNL_BX, (g.N[1] + MNL_BY - 1) / MNL_BY, g.N[2]);
  box_fill_kernel<<<grd, dim3(MNL_BX, MNL_BY), 0, (hipStream_t)stream>>>(
      dst, g, comp_type, comp_dir, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], value, invert, a,
      io[0], io[1], io[2]);
  return rc();
}

}  // namespace mnl
