// mnl_kernels_dft.hip -- gfx950 kernels of the DFT monitors (mnl_dft.cpp): the sampler, the
// sampling plan, the accumulators, gather / scatter / scale of DFT data in list order, the
// near-to-far-field transform, the pair sums of the energy and force monitors and the LDOS
// sums over the source points, with their launchers.
#include "mnl_device.hpp"

namespace mnl {

// ----------------------------------------------------------------- DFT
// dft_chunk::update_dft (src/dft.cpp:265-300), split in two so that the DFT
// array is read and written once per KB updates instead of once per update:
//  * dft_sample_kernel (every DFT step): the field averaged from the Yee points
//    onto the cell centre exactly as the reference does,
//    (w*0.25)*(((f0 + f1) + f2) + f3) with the weight product precomputed on the
//    host, into slot u of a small per-point buffer (E read through the
//    implicit-E rule in fused mode);
//  * dft_accum_kernel (every KB updates, and at the end of every step batch):
//    dft += fr_u * phase_u for u = 0..n-1 in update order -- the reference's
//    sequential accumulation, same operations in the same order, in registers.
// The DFT array is blocked by wave, [slot/64][freq][slot%64] complex, so a
// wave's access to one frequency is one contiguous 1-KB span.
__global__ void dft_sample_kernel(const int *__restrict__ pj, const double *__restrict__ pw,
                                  const int *__restrict__ pch, const DftChunkDev *__restrict__ ch,
                                  double *__restrict__ fr_out, long long npts, DevGrid g,
                                  DevFields f) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts) return;
  if (pj[3 * p] < 0) return;  // another rank's point
  const DftChunkDev cd = ch[pch[p]];
  const int c = cd.c, d = c % 3;
  const bool mag = c / 3 == T_H || c / 3 == T_B, raw = c / 3 >= T_D;  // raw: D or B itself
  Pt P;
  P.idx = 0;
  for (int e = 0; e < 3; e++) {
    P.j[e] = pj[3 * p + e];
    P.idx += (long long)P.j[e] * g.sdir[e];
  }
  auto val = [&](const Pt &q) -> double {
    if (raw) return mag ? f.B[d][q.idx] : f.D[d][q.idx];
    if (mag) {
      const bool sep = f.H[d] && (f.hall || pml_at(f, g, d, qcoord(g, q, T_H, d, d)));
      return sep ? f.H[d][q.idx] : f.B[d][q.idx];
    }
    if (e_implicit(f, g, d, q)) {
      const double dv = f.D[d][q.idx];
      return f.inveps[d] ? dv * f.inveps[d][q.idx] : dv;
    }
    return f.E[d][q.idx];
  };
  auto nb = [&](const Pt &q, int e) {
    Pt r = q;
    r.j[e] += 1;
    r.idx += g.sdir[e];
    return r;
  };
  double fr;
  if (cd.avgmode == 2) {
    const Pt q1 = nb(P, cd.d1), q2 = nb(P, cd.d2), q3 = nb(q1, cd.d2);
    fr = pw[p] * (val(P) + val(q1) + val(q2) + val(q3));
  } else if (cd.avgmode == 1) {
    fr = pw[p] * (val(P) + val(nb(P, cd.d1)));
  } else {
    fr = pw[p] * val(P);
  }
  fr_out[p] = fr;
}

// Sampling plan (built once per fused-mode epoch): per point the linear index of the first
// of the 1-4 Yee values its centred average reads (the others are +d1, +d2, +d1+d2) and, per
// value, where it lives (0 stored E, 1 implicit E = D * chi1inv, 2 B (H == B), 3 separate H)
// -- the per-point table lookups of dft_sample_kernel (PML flags, ownership, fused box) done
// once, so that the per-step sample is one metadata load and independent value loads.
// sel: bits 0-1 component direction, 2-3 avgmode, 4 + 2v: kind of value v, 12-13 d1, 14-15
// d2; 0xFFFF: another rank's point.  A D component is kind 1 with chi1inv == 1.0 (x * 1.0 == x;
// its palette byte is `one`'s, the entry that is bitwise 1.0), a B component kind 2 always, so
// the sampler needs no further kind.  The chi1inv of implicit-E values: as the palette bytes of
// the four values (spal, with uidx / utab: 4 B per point instead of 32) and as doubles (su,
// the fallback); *bad is set when a palette value is not bitwise the chi1inv array's.
__global__ void dft_plan_kernel(const int *__restrict__ pj, const int *__restrict__ pch,
                                const DftChunkDev *__restrict__ ch, long long npts, DevGrid g,
                                DevFields f, const unsigned *__restrict__ uidx,
                                const double *__restrict__ utab, int *__restrict__ sidx,
                                unsigned short *__restrict__ ssel, unsigned *__restrict__ spal,
                                double4 *__restrict__ su, int *__restrict__ bad, Box cb,
                                int *__restrict__ sci, unsigned one) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts) return;
  if (pj[3 * p] < 0) {
    ssel[p] = 0xFFFF;
    sidx[p] = 0;
    spal[p] = 0;
    su[p] = make_double4(1.0, 1.0, 1.0, 1.0);
    if (sci) sci[p] = -1;
    return;
  }
  const DftChunkDev cd = ch[pch[p]];
  const int c = cd.c, d = c % 3;
  const bool mag = c / 3 == T_H || c / 3 == T_B, raw = c / 3 >= T_D;
  Pt P;
  P.idx = 0;
  for (int e = 0; e < 3; e++) {
    P.j[e] = pj[3 * p + e];
    P.idx += (long long)P.j[e] * g.sdir[e];
  }
  auto kind = [&](const Pt &q) -> unsigned {
    if (raw) return mag ? 2u : 1u;
    if (mag) return (f.H[d] && (f.hall || pml_at(f, g, d, qcoord(g, q, T_H, d, d)))) ? 3u : 2u;
    return e_implicit(f, g, d, q) ? 1u : 0u;
  };
  auto nb = [&](const Pt &q, int e) {
    Pt r = q;
    r.j[e] += 1;
    r.idx += g.sdir[e];
    return r;
  };
  Pt q[4] = {P, P, P, P};
  int nv = 1;
  if (cd.avgmode == 2) {
    q[1] = nb(P, cd.d1), q[2] = nb(P, cd.d2), q[3] = nb(q[1], cd.d2);
    nv = 4;
  } else if (cd.avgmode == 1) {
    q[1] = nb(P, cd.d1);
    nv = 2;
  }
  unsigned sel = (unsigned)d | ((unsigned)cd.avgmode << 2) |
                 ((unsigned)max(cd.d1, 0) << 12) | ((unsigned)max(cd.d2, 0) << 14);
  double uv[4] = {1.0, 1.0, 1.0, 1.0};  // chi1inv of implicit-E values (x * 1.0 == x otherwise)
  unsigned pal = 0;
  bool mism = false;
  for (int v = 0; v < nv; v++) {
    const unsigned k = kind(q[v]);
    sel |= k << (4 + 2 * v);
    if (k == 1 && raw) {
      if (uidx) pal |= ((one >> (8 * d)) & 255u) << (8 * v);
    } else if (k == 1 && f.inveps[d]) {
      uv[v] = f.inveps[d][q[v].idx];
      if (uidx) {
        const unsigned b = (uidx[q[v].idx] >> (8 * d)) & 255u;
        pal |= b << (8 * v);
        mism = mism || utab[d * 256 + b] != uv[v];
      }
    } else if (k == 1 && uidx) {  // chi1inv == 1: a palette entry equal to 1.0
      const unsigned b = (uidx[q[v].idx] >> (8 * d)) & 255u;
      pal |= b << (8 * v);
      mism = mism || utab[d * 256 + b] != 1.0;
    }
  }
  if (mism) atomicOr(bad, 1);
  if (sci) {  // compact-box index of the first value if every value lies in the box
    int c[3], n[3];
    bool in = true;
    for (int e = 0; e < 3; e++) {
      const int ax = g.ax[e] >= 0 ? g.ax[e] : e;
      c[ax] = P.j[e] - cb.lo[ax];
      const int top = c[ax] + ((nv > 1 && cd.d1 == e) || (nv > 2 && cd.d2 == e) ? 1 : 0);
      n[ax] = cb.hi[ax] - cb.lo[ax] + 1;
      in = in && g.ax[e] >= 0 && c[ax] >= 0 && top < n[ax];
    }
    sci[p] = in ? c[0] + n[0] * (c[1] + n[1] * c[2]) : -1;
  }
  ssel[p] = (unsigned short)sel;
  sidx[p] = (int)P.idx;
  spal[p] = pal;
  su[p] = make_double4(uv[0], uv[1], uv[2], uv[3]);
}

struct DftSrc {  // the current buffer set: E, D, B, H per direction
  const double *E[3], *D[3], *B[3], *H[3];
};

// implicit E = D * chi1inv with chi1inv from the plan (constant in time; 1.0 where none)
__device__ __forceinline__ double dft_val(const DftSrc &s, int d, unsigned k, int i, double u) {
  if (k == 0) return s.E[d][i];
  if (k == 1) return s.D[d][i] * u;
  return k == 2 ? s.B[d][i] : s.H[d][i];
}

// fields::update_dfts' sample of one update (src/dft.cpp:265-300): the reference's centred
// average (w * 0.25) * (((f0 + f1) + f2) + f3) through the plan, for every flux object due at
// this step in one launch (DftSampleJobs: the workgroups of job i are blk0[i] ..)
typedef const DftSampleJobs __attribute__((address_space(4))) KDJ;
__global__ void __launch_bounds__(256) dft_sample_jobs_kernel(DftSampleJobs J, DftSrc s,
                                                              const double *__restrict__ utab) {
  // XCD-aware block order: workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8), so
  // each XCD takes one contiguous eighth of the points instead; the 2 x 2 averages of
  // neighbouring rows then meet their shared lines in that XCD's L2
  const unsigned nb = gridDim.x, xcd = blockIdx.x % 8u, q = nb / 8u, r = nb % 8u;
  const long long lb = xcd * q + min(xcd, r) + blockIdx.x / 8u;
  // the job table through the kernarg pointer (wave-uniform index: scalar loads, no copy)
  KDJ *jt = (KDJ *)__builtin_amdgcn_kernarg_segment_ptr();
  int ji = 0;
  for (int i = 1; i < jt->n; i++)
    if (lb >= jt->j[i].blk0) ji = i;
  const auto &jb = jt->j[ji];
  const long long p = (lb - jb.blk0) * 256 + threadIdx.x;
  if (p >= jb.npts) return;
  // the point's plan entries, loaded together (one round trip), then the values: compact-box
  // entries first (all in flight together), field-array loads only for the values the box
  // does not hold
  const unsigned sel = jb.ssel[p];
  const long long i0 = jb.sidx[p];
  const double w = jb.pw[p];
  const int ci = jb.cmp ? jb.sci[p] : -1;
  const unsigned pal = jb.usepal ? jb.spal[p] : 0u;
  if (sel == 0xFFFFu) return;  // another rank's point
  const int d = sel & 3, mode = (sel >> 2) & 3, d1 = (sel >> 12) & 3, d2 = (sel >> 14) & 3;
  const long long s1 = d1 == 0 ? J.sd[0] : (d1 == 1 ? J.sd[1] : J.sd[2]);
  const long long s2 = d2 == 0 ? J.sd[0] : (d2 == 1 ? J.sd[1] : J.sd[2]);
  const int nv = mode == 2 ? 4 : (mode == 1 ? 2 : 1);
  // chi1inv only for implicit-E values (kind 1 in any slot)
  const bool any1 = ((sel >> 4) & 0x55u & ~((sel >> 5) & 0x55u)) != 0;
  double u[4] = {1.0, 1.0, 1.0, 1.0};
  if (any1) {
    if (jb.usepal) {
#pragma unroll
      for (int v = 0; v < 4; v++)
        if (((sel >> (4 + 2 * v)) & 3) == 1) u[v] = utab[d * 256 + ((pal >> (8 * v)) & 255u)];
    } else {
      const double4 uu = ((const double4 *)jb.su)[p];
      u[0] = uu.x, u[1] = uu.y, u[2] = uu.z, u[3] = uu.w;
    }
  }
  const int c1 = d1 == 0 ? jb.cs[0] : (d1 == 1 ? jb.cs[1] : jb.cs[2]);
  const int c2 = d2 == 0 ? jb.cs[0] : (d2 == 1 ? jb.cs[1] : jb.cs[2]);
  const long long li[4] = {i0, i0 + s1, i0 + s2, i0 + s1 + s2};
  const int cix[4] = {ci, ci + c1, ci + c2, ci + c1 + c2};
  double val[4];
  bool got[4];
#pragma unroll
  for (int v = 0; v < 4; v++) {  // two-step points from the compact box of this state (dense)
    const unsigned k = (sel >> (4 + 2 * v)) & 3;
    const bool use = v < nv && ci >= 0 && (k == 1 || k == 2);
    val[v] = use ? jb.cmp[(size_t)((k == 1 ? d : 3 + d) * jb.ncell) + cix[v]] : 0.0;
    got[v] = use;
  }
#pragma unroll
  for (int v = 0; v < 4; v++) {  // the others (and entries no two-step point wrote)
    const unsigned k = (sel >> (4 + 2 * v)) & 3;
    if (v >= nv) continue;
    if (got[v] && (unsigned long long)__double_as_longlong(val[v]) != DFT_CMP_EMPTY)
      val[v] = k == 1 ? val[v] * u[v] : val[v];
    else
      val[v] = dft_val(s, d, k, (int)li[v], u[v]);
  }
  double fr;
  if (mode == 2) {
    fr = w * (val[0] + val[1] + val[2] + val[3]);
  } else if (mode == 1) {
    fr = w * (val[0] + val[1]);
  } else {
    fr = w * val[0];
  }
  jb.fr[p] = fr;
}

int k_dft_plan(const int *pj, const int *pch, const DftChunkDev *ch, long long npts,
               const DevGrid &g, const DevFields &f, const unsigned *uidx, const double *utab,
               int *sidx, unsigned short *ssel, unsigned *spal, void *su, int *bad,
               const Box &cbox, int *sci, unsigned pal_one, void *stream) {
  if (npts <= 0) return 0;
  dft_plan_kernel<<<(unsigned)((npts + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      pj, pch, ch, npts, g, f, uidx, utab, sidx, ssel, spal, (double4 *)su, bad, cbox, sci,
      pal_one);
  return rc();
}

int k_dft_sample_jobs(const DftSampleJobs &J, const DevGrid &g, const DevFields &f,
                      const double *utab, void *stream) {
  if (J.n <= 0 || J.n > DFT_MAXJ || J.nblk <= 0) return 0;
  if (J.j[0].blk0 != 0) return 2;
  DftSampleJobs t = J;
  for (int d = 0; d < 3; d++) t.sd[d] = g.sdir[d];
  DftSrc s;
  for (int d = 0; d < 3; d++) s.E[d] = f.E[d], s.D[d] = f.D[d], s.B[d] = f.B[d], s.H[d] = f.H[d];
  dft_sample_jobs_kernel<<<(unsigned)J.nblk, 256, 0, (hipStream_t)stream>>>(t, s, utab);
  return rc();
}

// Accumulation: one thread per point; a tile of DFT_FT frequencies is loaded
// into registers at once (DFT_FT independent loads in flight), every buffered
// update is added in order, and the tile is stored back.  When the whole wave
// belongs to one chunk (the usual case: slots are sorted by component and
// position) the phases are wave-uniform and come through scalar loads.
// one tile of FT frequencies at i0: FT independent loads in flight, every
// buffered update added in order, FT stores
template <int FT>
__device__ __forceinline__ void dft_accum_tile(double2 *__restrict__ dp,
                                               const double2 *__restrict__ php,
                                               const double *frv, int n, long long rstride,
                                               int i0) {
  double2 v[FT];
#pragma unroll
  for (int w = 0; w < FT; w++) v[w] = dp[(i0 + w) * 64];
#pragma unroll
  for (int u = 0; u < DFT_KB; u++) {
    if (u < n) {
#pragma unroll
      for (int w = 0; w < FT; w++) {
        const double2 q = php[u * rstride + i0 + w];
        v[w].x = v[w].x + frv[u] * q.x;
        v[w].y = v[w].y + frv[u] * q.y;
      }
    }
  }
#pragma unroll
  for (int w = 0; w < FT; w++) dp[(i0 + w) * 64] = v[w];
}

// tiles of DFT_FT frequencies, then the remainder in tiles of 8, 4, 2, 1
__device__ __forceinline__ void dft_accum_point(double2 *__restrict__ dp,
                                                const double2 *__restrict__ php,
                                                const double *frv, int n, long long rstride,
                                                int nfreq) {
  int i0 = 0;
  for (; i0 + DFT_FT <= nfreq; i0 += DFT_FT) dft_accum_tile<DFT_FT>(dp, php, frv, n, rstride, i0);
  if (nfreq - i0 >= 8) dft_accum_tile<8>(dp, php, frv, n, rstride, i0), i0 += 8;
  if (nfreq - i0 >= 4) dft_accum_tile<4>(dp, php, frv, n, rstride, i0), i0 += 4;
  if (nfreq - i0 >= 2) dft_accum_tile<2>(dp, php, frv, n, rstride, i0), i0 += 2;
  if (nfreq - i0 >= 1) dft_accum_tile<1>(dp, php, frv, n, rstride, i0);
}

// one tile of FT frequencies at i0 with the phases of the block's chunk staged in LDS
// (sph[u][DFT_FT], tile-relative column woff + w): broadcast LDS reads instead of a dependent
// global / scalar load per phase
template <int FT>
__device__ __forceinline__ void dft_accum_tile_lds(double2 *__restrict__ dp, const double2 *sph,
                                                   const double *frv, int n, int i0, int woff) {
  double2 v[FT];
#pragma unroll
  for (int w = 0; w < FT; w++) v[w] = dp[(i0 + woff + w) * 64];
#pragma unroll
  for (int u = 0; u < DFT_KB; u++) {
    if (u < n) {
#pragma unroll
      for (int w = 0; w < FT; w++) {
        const double2 q = sph[u * DFT_FT + woff + w];
        v[w].x = v[w].x + frv[u] * q.x;
        v[w].y = v[w].y + frv[u] * q.y;
      }
    }
  }
#pragma unroll
  for (int w = 0; w < FT; w++) dp[(i0 + woff + w) * 64] = v[w];
}

__global__ void __launch_bounds__(256)
    dft_accum_kernel(const int *__restrict__ pj, const int *__restrict__ pch,
                     double2 *__restrict__ dft, const double *__restrict__ fr, int n,
                     const double2 *__restrict__ ph, long long rstride, int nfreq,
                     long long npts) {
  __shared__ double2 sph[DFT_KB * DFT_FT];
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = p < npts && pj[3 * p] >= 0;
  const int k = pch[p < npts ? p : npts - 1];
  const int kb = pch[(long long)blockIdx.x * blockDim.x];
  const bool uni = __syncthreads_and(k == kb);  // one chunk (one phase row) for the block
  double frv[DFT_KB];
#pragma unroll
  for (int u = 0; u < DFT_KB; u++) frv[u] = (live && u < n) ? fr[u * npts + p] : 0.0;
  double2 *__restrict__ dp = dft + (p >> 6) * nfreq * 64 + (p & 63);
  if (!uni) {
    if (live) dft_accum_point(dp, ph + (long long)k * nfreq, frv, n, rstride, nfreq);
    return;
  }
  const double2 *php = ph + (long long)kb * nfreq;
  for (int i0 = 0; i0 < nfreq; i0 += DFT_FT) {  // block-uniform loop
    const int ft = min(DFT_FT, nfreq - i0);
    __syncthreads();  // the previous tile's readers are done
    for (int e = threadIdx.x; e < n * DFT_FT; e += blockDim.x) {
      const int u = e / DFT_FT, w = e % DFT_FT;
      if (w < ft) sph[e] = php[u * rstride + i0 + w];
    }
    __syncthreads();
    if (!live) continue;
    if (ft == DFT_FT) {
      dft_accum_tile_lds<DFT_FT>(dp, sph, frv, n, i0, 0);
    } else {  // the last, partial tile in pieces of 8, 4, 2, 1
      int w0 = 0;
      if (ft - w0 >= 8) dft_accum_tile_lds<8>(dp, sph, frv, n, i0, w0), w0 += 8;
      if (ft - w0 >= 4) dft_accum_tile_lds<4>(dp, sph, frv, n, i0, w0), w0 += 4;
      if (ft - w0 >= 2) dft_accum_tile_lds<2>(dp, sph, frv, n, i0, w0), w0 += 2;
      if (ft - w0 >= 1) dft_accum_tile_lds<1>(dp, sph, frv, n, i0, w0);
    }
  }
}

int k_dft_sample(const int *pj, const double *pw, const int *pch, const DftChunkDev *ch, double *fr,
                 long long npts, const DevGrid &g, const DevFields &f, void *stream) {
  if (npts <= 0) return 0;
  dft_sample_kernel<<<(unsigned)((npts + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      pj, pw, pch, ch, fr, npts, g, f);
  return rc();
}

int k_dft_accum(const int *pj, const int *pch, double *dft, const double *fr, int n,
                const double *ph, long long rstride, int nfreq, long long npts, void *stream) {
  if (npts <= 0 || n <= 0) return 0;
  if (n > DFT_KB || nfreq < 1) return 2;
  dft_accum_kernel<<<(unsigned)((npts + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      pj, pch, (double2 *)dft, fr, n, (const double2 *)ph, rstride, nfreq, npts);
  return rc();
}

// Complex fields: the numcmp == 2 branch of dft_chunk::update_dft
// (src/dft.cpp:295-299), dft += phase * (f_re + i f_im) per update in update order, each
// product as std::complex forms it (two products and one sum per part, no contraction).  fr0 /
// fr1: the buffered sample rows of part 0 / part 1 (the same slots).  One thread per point;
// launched only for complex fields, so the real path's kernel and bits do not move.
__global__ void __launch_bounds__(256)
    dft_accum_cplx_kernel(const int *__restrict__ pj, const int *__restrict__ pch,
                          double2 *__restrict__ dft, const double *__restrict__ fr0,
                          const double *__restrict__ fr1, int n, const double2 *__restrict__ ph,
                          long long rstride, int nfreq, long long npts) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= npts || pj[3 * p] < 0) return;
  const double2 *__restrict__ php = ph + (long long)pch[p] * nfreq;
  double a[DFT_KB], b[DFT_KB];
#pragma unroll
  for (int u = 0; u < DFT_KB; u++) {
    a[u] = u < n ? fr0[u * npts + p] : 0.0;
    b[u] = u < n ? fr1[u * npts + p] : 0.0;
  }
  double2 *__restrict__ dp = dft + (p >> 6) * nfreq * 64 + (p & 63);
  for (int i = 0; i < nfreq; i++) {
    double2 v = dp[(long long)i * 64];
#pragma unroll
    for (int u = 0; u < DFT_KB; u++) {
      if (u < n) {
        const double2 q = php[u * rstride + i];
        v.x = v.x + (q.x * a[u] - q.y * b[u]);
        v.y = v.y + (q.x * b[u] + q.y * a[u]);
      }
    }
    dp[(long long)i * 64] = v;
  }
}

int k_dft_accum_cplx(const int *pj, const int *pch, double *dft, const double *fr0,
                     const double *fr1, int n, const double *ph, long long rstride, int nfreq,
                     long long npts, void *stream) {
  if (npts <= 0 || n <= 0) return 0;
  if (n > DFT_KB || nfreq < 1 || !fr0 || !fr1) return 2;
  dft_accum_cplx_kernel<<<(unsigned)((npts + 255) / 256), 256, 0, (hipStream_t)stream>>>(
      pj, pch, (double2 *)dft, fr0, fr1, n, (const double2 *)ph, rstride, nfreq, npts);
  return rc();
}

// ------------------------------------------------- DFT data in list order
// get / load / scale of the DFT values (save_dft_hdf5 / load_dft_hdf5 / dft_chunk::scale_dft,
// src/dft.cpp:401-496).  The array is [slot/64][freq][slot%64]; the public order is the
// reference's list order [list point][freq].  Gather and scatter walk the array in slot order:
// one wave per block of 64 slots and tile of DFT_DT frequencies, so that every access to the
// blocked array is one contiguous 1-KB span, and the 64 x DFT_DT tile is transposed through
// LDS so that the list side moves DFT_DT * 16 B = one whole 128-B line per point.  inv[slot] is
// the slot's index in the list, or -1 (another list, another rank's point, the padded tail).
constexpr int DFT_DT = 8;      // frequencies per tile
constexpr int DFT_DW = 4;      // waves (slot blocks) per workgroup
constexpr int DFT_DP = 64 + 1; // LDS row pitch in double2

__global__ void __launch_bounds__(64 * DFT_DW)
    dft_gather_kernel(const double2 *__restrict__ dft, const int *__restrict__ inv,
                      double2 *__restrict__ out, int nfreq, long long nblk) {
  __shared__ double2 tile[DFT_DW][DFT_DT][DFT_DP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long blk = (long long)blockIdx.x * DFT_DW + wv;
  const int i0 = blockIdx.y * DFT_DT, ft = min(DFT_DT, nfreq - i0);
  const bool on = blk < nblk;
  const int k = on ? inv[blk * 64 + lane] : -1;
  if (on) {
    const double2 *__restrict__ dp = dft + (blk * nfreq + i0) * 64 + lane;
#pragma unroll
    for (int w = 0; w < DFT_DT; w++)
      if (w < ft) tile[wv][w][lane] = dp[w * 64];
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < DFT_DT; it++) {  // 8 lanes per point: its DFT_DT frequencies in a row
    const int q = it * (64 / DFT_DT) + lane / DFT_DT, w = lane % DFT_DT;
    const int kq = __shfl(k, q);
    if (kq >= 0 && w < ft) out[(long long)kq * nfreq + i0 + w] = tile[wv][w][q];
  }
}

// the inverse: dft[slot] = sign * in[list point] for the slots of this list
__global__ void __launch_bounds__(64 * DFT_DW)
    dft_scatter_kernel(double2 *__restrict__ dft, const int *__restrict__ inv,
                       const double2 *__restrict__ in, double sign, int nfreq, long long nblk) {
  __shared__ double2 tile[DFT_DW][DFT_DT][DFT_DP];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long blk = (long long)blockIdx.x * DFT_DW + wv;
  const int i0 = blockIdx.y * DFT_DT, ft = min(DFT_DT, nfreq - i0);
  const bool on = blk < nblk;
  const int k = on ? inv[blk * 64 + lane] : -1;
#pragma unroll
  for (int it = 0; it < DFT_DT; it++) {
    const int q = it * (64 / DFT_DT) + lane / DFT_DT, w = lane % DFT_DT;
    const int kq = __shfl(k, q);
    if (kq >= 0 && w < ft) {
      const double2 v = in[(long long)kq * nfreq + i0 + w];
      tile[wv][w][q] = make_double2(sign * v.x, sign * v.y);
    }
  }
  __syncthreads();
  if (k >= 0) {
    double2 *__restrict__ dp = dft + (blk * nfreq + i0) * 64 + lane;
#pragma unroll
    for (int w = 0; w < DFT_DT; w++)
      if (w < ft) dp[w * 64] = tile[wv][w][lane];
  }
}

// dft[i] *= s with the two roundings per product of std::complex<double>::operator*= on finite
// values (no contraction: -ffp-contract=off)
__global__ void __launch_bounds__(256)
    dft_scale_kernel(double2 *__restrict__ dft, double c, double d, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double2 v = dft[i];
    const double ac = v.x * c, bd = v.y * d, ad = v.x * d, bc = v.y * c;
    dft[i] = make_double2(ac - bd, ad + bc);
  }
}

int k_dft_gather(const double *dft, const int *inv, double *out, int nfreq, long long nslots,
                 void *stream) {
  const long long nblk = (nslots + 63) / 64;
  if (nblk <= 0 || nfreq < 1) return 0;
  const long long gx = (nblk + DFT_DW - 1) / DFT_DW, gy = (nfreq + DFT_DT - 1) / DFT_DT;
  if (gx > 0x7fffffffLL || gy > 65535) return 2;
  dft_gather_kernel<<<dim3((unsigned)gx, (unsigned)gy), 64 * DFT_DW, 0, (hipStream_t)stream>>>(
      (const double2 *)dft, inv, (double2 *)out, nfreq, nblk);
  return rc();
}

int k_dft_scatter(double *dft, const int *inv, const double *in, double sign, int nfreq,
                  long long nslots, void *stream) {
  const long long nblk = (nslots + 63) / 64;
  if (nblk <= 0 || nfreq < 1) return 0;
  const long long gx = (nblk + DFT_DW - 1) / DFT_DW, gy = (nfreq + DFT_DT - 1) / DFT_DT;
  if (gx > 0x7fffffffLL || gy > 65535) return 2;
  dft_scatter_kernel<<<dim3((unsigned)gx, (unsigned)gy), 64 * DFT_DW, 0, (hipStream_t)stream>>>(
      (double2 *)dft, inv, (const double2 *)in, sign, nfreq, nblk);
  return rc();
}

int k_dft_scale(double *dft, double re, double im, long long ncomplex, void *stream) {
  if (ncomplex <= 0) return 0;
  const long long nb = std::min<long long>((ncomplex + 255) / 256, 1 << 16);
  dft_scale_kernel<<<(unsigned)nb, 256, 0, (hipStream_t)stream>>>((double2 *)dft, re, im, ncomplex);
  return rc();
}

// ------------------------------------------------- near-to-far-field transform
// dft_near2far::farfield_lowlevel (src/near2far.cpp:340-387) for a block of NP far points and
// a tile of FT frequencies over one workgroup's slot range.  Lanes are slots (the DFT array's
// [slot/64][freq][slot%64] layout: coalesced 16-byte reads); x - x0, r and rhat are formed once
// per (slot, far point) and every DFT value once per slot and frequency, so the sincos and the
// green3d arithmetic dominate.  Each lane keeps its 12 doubles per (far point, frequency) in
// registers over the whole slot range; one wave reduction and one LDS pass per workgroup at
// the end.  The sums of one (far point, frequency) never depend on the other members of the
// block or tile, so a far point's result is the same in every batch.
__device__ __forceinline__ double n2f_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

template <int FT, int NP>
__global__ __launch_bounds__(64 * N2F_WAVES) void n2f_farfield_kernel(N2FArgs a) {
  __shared__ double red[N2F_WAVES][NP * FT * 12];
  constexpr double pi = 3.141592653589793238462643383276;  // meep::pi
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = blockIdx.y * FT, p0 = blockIdx.z * NP;
  const double n = sqrt(a.eps * a.mu), Z = sqrt(a.mu / a.eps);
  double kk[FT], kinv[FT], ce[FT], cm[FT];
#pragma unroll
  for (int w = 0; w < FT; w++) {  // tail tiles repeat the last frequency (not written)
    const double k = 2 * pi * a.freq[min(f0 + w, a.nfreq - 1)] * n;
    kk[w] = k;
    kinv[w] = 1.0 / k;
    ce[w] = k * n / (4 * pi) / a.eps;
    cm[w] = k * n / (4 * pi) / a.mu;
  }
  double X[NP][3];
#pragma unroll
  for (int q = 0; q < NP; q++)  // tail blocks repeat the last far point (not written)
#pragma unroll
    for (int d = 0; d < 3; d++) X[q][d] = a.xyz[3 * (long long)min(p0 + q, a.npts - 1) + d];
  double acc[NP][FT][12];
#pragma unroll
  for (int q = 0; q < NP; q++)
#pragma unroll
    for (int w = 0; w < FT; w++)
#pragma unroll
      for (int j = 0; j < 12; j++) acc[q][w][j] = 0.0;
  const long long nblk = (a.nslots + 63) >> 6;
  const long long b0 = (long long)blockIdx.x * a.wg_blocks;
  const long long b1 = min(b0 + (long long)a.wg_blocks, nblk);
  const double2 *__restrict__ dft = reinterpret_cast<const double2 *>(a.dft);
  for (long long b = b0 + wave; b < b1; b += N2F_WAVES) {
    const long long s = b * 64 + lane;
    if (s >= a.nslots) continue;  // the padded tail of the last block
    // the run of this slot: c0 is uniform over long slot runs, so the two sides of the
    // electric / magnetic choice below are wave-uniform except where a wave straddles two runs
    int lo = 0, hi = a.nruns - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (a.runs[mid].first <= s)
        lo = mid;
      else
        hi = mid - 1;
    }
    const int c0 = a.runs[lo].c0;
    const bool elec = c0 < 3;
    const int dir = c0 % 3;
    const double px = dir == 0 ? 1.0 : 0.0, py = dir == 1 ? 1.0 : 0.0, pz = dir == 2 ? 1.0 : 0.0;
    const double zf = elec ? 1.0 / Z : -Z;
    const double x0 = a.x0[s], y0 = a.x0[a.npad + s], z0 = a.x0[2 * a.npad + s];
    double rh[NP][3], rcp[NP][3], rinv[NP], rr[NP], pdr[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) {
      const double dx = X[q][0] - x0, dy = X[q][1] - y0, dz = X[q][2] - z0;
      const double r = sqrt(dx * dx + dy * dy + dz * dz);
      rr[q] = r;
      rinv[q] = 1.0 / r;
      rh[q][0] = dx / r, rh[q][1] = dy / r, rh[q][2] = dz / r;
      pdr[q] = px * rh[q][0] + py * rh[q][1] + pz * rh[q][2];
      rcp[q][0] = rh[q][1] * pz - rh[q][2] * py;
      rcp[q][1] = rh[q][2] * px - rh[q][0] * pz;
      rcp[q][2] = rh[q][0] * py - rh[q][1] * px;
    }
#pragma unroll
    for (int w = 0; w < FT; w++) {
      const double2 f = dft[(b * a.nfreq + min(f0 + w, a.nfreq - 1)) * 64 + lane];
      const double cw = elec ? ce[w] : cm[w];
#pragma unroll
      for (int q = 0; q < NP; q++) {
        double sn, cs;
        sincos(kk[w] * rr[q] + pi * 0.5, &sn, &cs);
        const double amp = cw * rinv[q];
        const double pc = amp * cs, ps = amp * sn;
        const double er = f.x * pc - f.y * ps, ei = f.x * ps + f.y * pc;  // expfac
        const double inv = kinv[w] * rinv[q];  // 1 / (k r)
        const double i2 = -(inv * inv);        // 1 / (i k r)^2
        const double t1r = 1.0 + i2, t1i = inv;
        const double t2r = (-1.0 - 3.0 * i2) * pdr[q], t2i = (-3.0 * inv) * pdr[q];
        const double qr = (er - ei * inv) * zf, qi = (er * inv + ei) * zf;  // expfac * term3
        double mn[6], cr[6];
        const double pv[3] = {px, py, pz};
#pragma unroll
        for (int j = 0; j < 3; j++) {
          const double mr = t1r * pv[j] + t2r * rh[q][j], mi = t1i * pv[j] + t2i * rh[q][j];
          mn[2 * j] = er * mr - ei * mi;
          mn[2 * j + 1] = er * mi + ei * mr;
          cr[2 * j] = qr * rcp[q][j];
          cr[2 * j + 1] = qi * rcp[q][j];
        }
#pragma unroll
        for (int j = 0; j < 6; j++) {
          acc[q][w][j] += elec ? mn[j] : cr[j];
          acc[q][w][6 + j] += elec ? cr[j] : mn[j];
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NP; q++)
#pragma unroll
    for (int w = 0; w < FT; w++)
#pragma unroll
      for (int j = 0; j < 12; j++) {
        const double v = n2f_wave_sum(acc[q][w][j]);
        if (lane == 0) red[wave][(q * FT + w) * 12 + j] = v;
      }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < NP * FT * 12) {
    const int q = t / (FT * 12), w = (t / 12) % FT, j = t % 12;
    if (p0 + q < a.npts && f0 + w < a.nfreq) {
      double v = red[0][t];
#pragma unroll
      for (int k = 1; k < N2F_WAVES; k++) v += red[k][t];
      a.part[(((long long)blockIdx.x * a.npts + p0 + q) * a.nfreq + f0 + w) * 12 + j] = v;
    }
  }
}

// out[i] = the workgroups' partial sums of element i, added in workgroup order
__global__ void __launch_bounds__(256)
    n2f_reduce_kernel(const double *__restrict__ part, double *__restrict__ out, int nwg,
                      long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v = 0.0;
  for (int g = 0; g < nwg; g++) v += part[g * n + i];
  out[i] = v;
}

// ------------------------------------------------- pair sums (energy, force)
// dft_energy::electric / magnetic (src/dft.cpp:657-687) and stress_sum (src/stress.cpp:90-99):
// per frequency the sum over paired chunks and their points of x * real(a * conj(b)), read from
// the DFT array where it lives.  The two chunks of a pair hold the same points in the same slot
// order, so the host hands over runs (two slot bases, a count, x).  Lanes take consecutive pair
// points -- consecutive slots of both chunks, so a wave's read of one frequency is one or two
// contiguous 1-KB spans of 16-byte values per chunk -- and keep PS_FT frequencies in registers
// over the workgroup's fixed range of pair points; then one wave reduction in registers and
// one LDS pass over the PS_WAVES waves.  No atomics: part[wg][freq] is added in workgroup order
// by n2f_reduce_kernel, and the split into workgroups depends on the object alone, so a value
// is the same bits in every call and every stepping mode.
template <int FT>
__global__ void __launch_bounds__(64 * PS_WAVES)
    dft_pair_sum_kernel(const double2 *__restrict__ dft, const PairRun *__restrict__ runs,
                        int nruns, long long total, int wg_pts, int nfreq,
                        double *__restrict__ part) {
  __shared__ double red[PS_WAVES][FT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = blockIdx.y * FT;
  const long long g0 = (long long)blockIdx.x * wg_pts, g1 = min(g0 + (long long)wg_pts, total);
  double acc[FT];
#pragma unroll
  for (int w = 0; w < FT; w++) acc[w] = 0.0;
  for (long long g = g0 + threadIdx.x; g < g1; g += 64 * PS_WAVES) {
    // the run of this pair point, by bisection every time: walking on from the previous
    // point's run instead measured 2 to 2.6 times slower
    int lo = 0, hi = nruns - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (runs[mid].g0 <= g)
        lo = mid;
      else
        hi = mid - 1;
    }
    const PairRun r = runs[lo];
    const long long sa = r.a0 + (g - r.g0), sb = r.b0 + (g - r.g0);
    const double2 *__restrict__ pa = dft + (sa >> 6) * nfreq * 64 + (sa & 63);
    const double2 *__restrict__ pb = dft + (sb >> 6) * nfreq * 64 + (sb & 63);
    double2 a[FT], b[FT];
#pragma unroll
    for (int w = 0; w < FT; w++) {  // tail tiles repeat the last frequency (not written)
      const long long fo = (long long)min(f0 + w, nfreq - 1) * 64;
      a[w] = pa[fo];
      b[w] = pb[fo];
    }
#pragma unroll
    for (int w = 0; w < FT; w++) acc[w] += r.x * (a[w].x * b[w].x + a[w].y * b[w].y);
  }
#pragma unroll
  for (int w = 0; w < FT; w++) {
    const double v = n2f_wave_sum(acc[w]);
    if (lane == 0) red[wave][w] = v;
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < FT && f0 + t < nfreq) {
    double v = red[0][t];
#pragma unroll
    for (int k = 1; k < PS_WAVES; k++) v += red[k][t];
    part[(long long)blockIdx.x * nfreq + f0 + t] = v;
  }
}

int k_dft_pair_sum(const double *dft, const PairRun *runs, int nruns, long long total, int wg_pts,
                   int nwg, int nfreq, long long npad, double *part, void *stream) {
  if (total <= 0 || nwg <= 0) return 0;
  if (nfreq < 1 || nruns < 1 || wg_pts < 1 || npad < 64) return 2;
  if ((long long)nwg * wg_pts < total) return 2;  // every pair point belongs to a workgroup
  const dim3 grd((unsigned)nwg, (unsigned)((nfreq + PS_FT - 1) / PS_FT));
  if (grd.y > 65535) return 2;
  dft_pair_sum_kernel<PS_FT><<<grd, dim3(64 * PS_WAVES), 0, (hipStream_t)stream>>>(
      (const double2 *)dft, runs, nruns, total, wg_pts, nfreq, part);
  return rc();
}

// ------------------------------------------------- norm of the DFT arrays
// fields::dft_norm (src/dft.cpp:312-361): the sum of |dft|^2 over every frequency of this
// rank's slots.  A wave takes whole 64-slot blocks of the workgroup's fixed range (lanes are
// slots: a frequency is one contiguous 1-KB span), then one wave reduction and one LDS pass over
// the waves in order.  No atomics: part[wg] is added in workgroup order by n2f_reduce_kernel and
// the split depends on the object alone, so the value is the same bits in every call.
__global__ void __launch_bounds__(64 * NORM_WAVES)
    dft_norm_kernel(const double2 *__restrict__ dft, const int *__restrict__ pj, long long npts,
                    int nfreq, long long nblk, long long wg_blocks, double *__restrict__ part) {
  __shared__ double red[NORM_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long b0 = (long long)blockIdx.x * wg_blocks, b1 = min(b0 + wg_blocks, nblk);
  double acc = 0.0;
  for (long long b = b0 + wave; b < b1; b += NORM_WAVES) {
    const long long s = b * 64 + lane;
    if (s >= npts || pj[3 * s] < 0) continue;  // the padded tail, another rank's slot
    const double2 *__restrict__ dp = dft + b * nfreq * 64 + lane;
    for (int i = 0; i < nfreq; i++) {
      const double2 v = dp[(long long)i * 64];
      acc += v.x * v.x + v.y * v.y;
    }
  }
  const double v = n2f_wave_sum(acc);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int k = 1; k < NORM_WAVES; k++) t += red[k];
    part[blockIdx.x] = t;
  }
}

int k_dft_norm(const double *dft, const int *pj, long long npts, int nfreq, long long nblk,
               long long wg_blocks, int nwg, double *part, void *stream) {
  if (npts <= 0 || nfreq < 1 || nwg <= 0) return 0;
  if (wg_blocks < 1 || nblk != (npts + 63) / 64) return 2;
  if ((long long)nwg * wg_blocks < nblk) return 2;  // every block belongs to a workgroup
  dft_norm_kernel<<<(unsigned)nwg, 64 * NORM_WAVES, 0, (hipStream_t)stream>>>(
      (const double2 *)dft, pj, npts, nfreq, nblk, wg_blocks, part);
  return rc();
}

// ------------------------------------------------- field probe
// The flush of a probe (fields::get_field recorded every step): the
// samplers have put w[i] * v[i] of update u into fr[u][slot]; one thread per buffered update
// forms res = 0; res += w[i] * v[i] over the list's points in list order, skipping the points
// another rank owns, and stores it in the ring.  When more rows are buffered than the ring
// holds, only the newest `cap` rows are stored (each index written once).
__global__ void __launch_bounds__(64)
    probe_append_kernel(const double *__restrict__ fr, long long npts, int n,
                        const int *__restrict__ pslot, int nlist, double *__restrict__ series,
                        int cap, int start) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= n || u < n - cap) return;
  double res = 0.0;
  for (int i = 0; i < nlist; i++) {
    const int s = pslot[i];
    if (s >= 0) res += fr[(long long)u * npts + s];
  }
  series[(int)(((long long)start + u) % cap)] = res;
}

int k_probe_append(const double *fr, long long npts, int n, const int *pslot, int nlist,
                   double *series, int cap, int start, void *stream) {
  if (n <= 0) return 0;
  if (n > DFT_KB || nlist < 1 || nlist > 8 || npts < nlist || cap < 1 || start < 0 || start >= cap)
    return 2;
  probe_append_kernel<<<(unsigned)((n + 63) / 64), 64, 0, (hipStream_t)stream>>>(
      fr, npts, n, pslot, nlist, series, cap, start);
  return rc();
}

// ------------------------------------------------- LDOS
// dft_ldos::update's sums over the source points (src/dft_ldos.cpp:107-149) for the buffered
// updates: EJ_u = sum fr[u][s] * conj(A[s]) over the slots below nE, HJ_u over the others.  A
// thread takes pairs of adjacent slots -- the rows are npad (even) doubles long, so a pair is one
// aligned 16-byte load and a wave reads 1 KB in a row -- keeps the pair's amplitudes in registers
// and walks a tile of UT updates (grid y), so that A is read once per tile, not once per update.
// Four accumulators per update; one wave reduction in registers and one LDS pass over the waves
// in wave order.  No atomics: part[wg][u][4] is added in workgroup order by n2f_reduce_kernel,
// and a workgroup's range of pairs depends on the object alone, so the sums of one update are
// the same bits wherever its row stands in the buffer and in every stepping mode.  A slot of
// another rank or of the padded tail (pj < 0) is never added, not even as 0 * value.
template <int UT>
__global__ void __launch_bounds__(64 * LDOS_WAVES)
    ldos_reduce_kernel(const double *__restrict__ fr, const double2 *__restrict__ amp,
                       const int *__restrict__ pj, long long npad, long long nE, int n,
                       long long wg_pairs, double *__restrict__ part) {
  __shared__ double red[LDOS_WAVES][UT * 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int u0 = blockIdx.y * UT;
  const long long q0 = (long long)blockIdx.x * wg_pairs, q1 = min(q0 + wg_pairs, npad >> 1);
  double acc[UT][4];
#pragma unroll
  for (int w = 0; w < UT; w++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[w][j] = 0.0;
  for (long long q = q0 + threadIdx.x; q < q1; q += 64 * LDOS_WAVES) {
    const long long s = 2 * q;
    const bool l0 = pj[3 * s] >= 0, l1 = pj[3 * (s + 1)] >= 0;
    if (!l0 && !l1) continue;
    const double2 a0 = amp[s], a1 = amp[s + 1];
    const bool h0 = s >= nE, h1 = s + 1 >= nE;
    double2 f[UT];
#pragma unroll
    for (int w = 0; w < UT; w++)  // tail tiles repeat the last row (not written)
      f[w] = *reinterpret_cast<const double2 *>(fr + (long long)min(u0 + w, n - 1) * npad + s);
#pragma unroll
    for (int w = 0; w < UT; w++) {
      const double r0 = f[w].x * a0.x, i0 = f[w].x * -a0.y;  // double * conj(A)
      const double r1 = f[w].y * a1.x, i1 = f[w].y * -a1.y;
      // (selects, not products with 0: a slot that is not added contributes an exact + 0.0)
      acc[w][0] += (l0 && !h0) ? r0 : 0.0;
      acc[w][1] += (l0 && !h0) ? i0 : 0.0;
      acc[w][2] += (l0 && h0) ? r0 : 0.0;
      acc[w][3] += (l0 && h0) ? i0 : 0.0;
      acc[w][0] += (l1 && !h1) ? r1 : 0.0;
      acc[w][1] += (l1 && !h1) ? i1 : 0.0;
      acc[w][2] += (l1 && h1) ? r1 : 0.0;
      acc[w][3] += (l1 && h1) ? i1 : 0.0;
    }
  }
#pragma unroll
  for (int w = 0; w < UT; w++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const double v = n2f_wave_sum(acc[w][j]);
      if (lane == 0) red[wave][w * 4 + j] = v;
    }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < UT * 4 && u0 + t / 4 < n) {
    double v = red[0][t];
#pragma unroll
    for (int k = 1; k < LDOS_WAVES; k++) v += red[k][t];
    part[((long long)blockIdx.x * n + u0 + t / 4) * 4 + (t & 3)] = v;
  }
}

// Fdft[i] += Ephase * EJ + Hphase * HJ (src/dft_ldos.cpp:150-153) for the buffered updates in
// update order, one thread per frequency: each product as std::complex forms it (two products
// and one sum or difference per part, no contraction), the two products added, then the sum
// added to F -- the reference's operations in its order.  On the device so that a flush in the
// middle of a batch needs no host round trip.
__global__ void __launch_bounds__(64)
    ldos_accum_kernel(const double *__restrict__ ej, const double *__restrict__ ph,
                      long long rstride, int n, int nfreq, double2 *__restrict__ F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nfreq) return;
  double2 v = F[i];
  for (int u = 0; u < n; u++) {
    const double *__restrict__ r = ph + u * rstride;
    const double ex = r[2 * i], ey = r[2 * i + 1];
    const double hx = r[2 * (nfreq + i)], hy = r[2 * (nfreq + i) + 1];
    const double ejx = ej[4 * u], ejy = ej[4 * u + 1], hjx = ej[4 * u + 2], hjy = ej[4 * u + 3];
    const double er = ex * ejx - ey * ejy, ei = ex * ejy + ey * ejx;
    const double hr = hx * hjx - hy * hjy, hi = hx * hjy + hy * hjx;
    v.x = v.x + (er + hr);
    v.y = v.y + (ei + hi);
  }
  F[i] = v;
}

int k_ldos_reduce(const double *fr, const double *amp, const int *pj, long long npad, long long nE,
                  int n, long long wg_pairs, int nwg, double *part, void *stream) {
  if (npad <= 0 || n <= 0) return 0;
  if (!fr || !amp || !pj || !part || (npad & 1) || n > DFT_KB || nE < 0 || nE > npad ||
      wg_pairs < 1 || nwg < 1 || nwg > LDOS_MAX_WG)
    return 2;
  if ((long long)nwg * wg_pairs < (npad >> 1)) return 2;  // every pair belongs to a workgroup
  const dim3 grd((unsigned)nwg, (unsigned)((n + LDOS_UT - 1) / LDOS_UT));
  ldos_reduce_kernel<LDOS_UT><<<grd, dim3(64 * LDOS_WAVES), 0, (hipStream_t)stream>>>(
      fr, (const double2 *)amp, pj, npad, nE, n, wg_pairs, part);
  return rc();
}

int k_ldos_accum(const double *ej, const double *ph, long long rstride, int n, int nfreq, double *F,
                 void *stream) {
  if (n <= 0) return 0;
  if (!ej || !ph || !F || n > DFT_KB || nfreq < 1 || rstride < 4LL * nfreq) return 2;
  ldos_accum_kernel<<<(unsigned)((nfreq + 63) / 64), 64, 0, (hipStream_t)stream>>>(
      ej, ph, rstride, n, nfreq, (double2 *)F);
  return rc();
}

// ------------------------------------------------- mode coefficients
// fields::get_overlap (src/dft.cpp:1377-1427) for a tile of MT modes x FT frequencies over one
// workgroup's slot range: the terms of dft_chunk::process_dft_component (src/dft.cpp:977-1027),
// w * conj(mode[c_conjugate](x)) * dft_val and w * conj(mode[c_conjugate](x)) * mode[c](x), of
// the one sum the range's component adds to.  The mode is an analytic plane wave, so its value
// is amplitude * phase with the phase the product of three table entries (mnl_modes.hpp): the
// device only multiplies and adds.  Lanes are consecutive slots (a frequency is a contiguous
// span of 16-byte values); each lane keeps its 4 doubles per (mode, frequency) in registers over
// the range, then one wave reduction and one LDS pass in wave order.  No atomics: the ranges
// hold this rank's slots only (other ranks' slots and the padded tail belong to no range) and
// depend on the object alone, so a sum is the same bits in every call and every stepping mode.
// Complex products as std::complex forms them (the file is built without contraction).
__device__ __forceinline__ double2 mo_cmul(double2 a, double2 b) {
  return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}

template <int MT, int FT>
__global__ void __launch_bounds__(64 * MO_WAVES) mode_overlap_kernel(ModeArgs a) {
  __shared__ double red[MO_WAVES][MT * FT * 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f0 = blockIdx.y * FT, m0 = blockIdx.z * MT;
  const ModeRange r = a.rng[blockIdx.x];
  const double2 *__restrict__ dft = (const double2 *)a.dft;
  const double2 *__restrict__ wv = (const double2 *)a.wv;
  const double2 *__restrict__ pa = (const double2 *)a.pa;
  const double2 *__restrict__ pb = (const double2 *)a.pb;
  const double2 *__restrict__ pl = (const double2 *)a.pl;
  const double2 *__restrict__ ac = (const double2 *)a.ac;
  const double2 *__restrict__ as = (const double2 *)a.as;
  double acc[MT][FT][4];
#pragma unroll
  for (int q = 0; q < MT; q++)
#pragma unroll
    for (int w = 0; w < FT; w++)
#pragma unroll
      for (int e = 0; e < 4; e++) acc[q][w][e] = 0.0;
  for (int s = r.s0 + (int)threadIdx.x; s < r.s1; s += 64 * MO_WAVES) {
    const ModeSlot ms = a.slot[s];
    const double2 ww = wv[s];  // (w, stored weight)
    const bool stored_w = (ms.layer & 2) != 0;
    const int layer = ms.layer & 1;
    const double2 *__restrict__ dp = dft + (long long)(s >> 6) * a.nfreq * 64 + (s & 63);
    double2 d[FT];
#pragma unroll
    for (int w = 0; w < FT; w++) {  // tail tiles repeat the last frequency (not written)
      double2 v = dp[(long long)min(f0 + w, a.nfreq - 1) * 64];
      v.x = v.x / ww.y, v.y = v.y / ww.y;  // dft / stored_weight
      if (stored_w && (v.x != 0.0 || v.y != 0.0)) v.x = v.x / ww.x, v.y = v.y / ww.x;
      d[w] = v;
    }
#pragma unroll
    for (int q = 0; q < MT; q++) {  // tail tiles repeat the last mode (not written)
      const int m = min(m0 + q, a.nmodes - 1);
      const double2 ab = mo_cmul(pa[(long long)m * a.na + ms.ia], pb[(long long)m * a.nb + ms.ib]);
#pragma unroll
      for (int w = 0; w < FT; w++) {
        const long long mf = (long long)m * a.nfreq + min(f0 + w, a.nfreq - 1);
        const double2 ph = mo_cmul(ab, pl[mf * 2 + layer]);
        const double2 mc = mo_cmul(ac[mf * 4 + r.j], ph);  // mode[c_conjugate](x)
        const double2 mo = mo_cmul(as[mf * 4 + r.j], ph);  // mode[c](x)
        const double2 wc = make_double2(ww.x * mc.x, ww.x * -mc.y);  // w * conj(mode1val)
        const double2 t = mo_cmul(wc, d[w]), u = mo_cmul(wc, mo);
        acc[q][w][0] += t.x;
        acc[q][w][1] += t.y;
        acc[q][w][2] += u.x;
        acc[q][w][3] += u.y;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < MT; q++)
#pragma unroll
    for (int w = 0; w < FT; w++)
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const double v = n2f_wave_sum(acc[q][w][e]);
        if (lane == 0) red[wave][(q * FT + w) * 4 + e] = v;
      }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < MT * FT * 4) {
    const int q = t / (FT * 4), w = (t >> 2) % FT;
    if (m0 + q < a.nmodes && f0 + w < a.nfreq) {
      double v = red[0][t];
#pragma unroll
      for (int k = 1; k < MO_WAVES; k++) v += red[k][t];
      a.part[(((long long)blockIdx.x * a.nmodes + m0 + q) * a.nfreq + f0 + w) * 4 + (t & 3)] = v;
    }
  }
}

int k_mode_overlap(const ModeArgs &a, int nwg, long long nslots, void *stream) {
  if (nwg <= 0) return 0;
  if (!a.dft || !a.slot || !a.wv || !a.rng || !a.pa || !a.pb || !a.pl || !a.ac || !a.as ||
      !a.part || a.nmodes < 1 || a.nfreq < 1 || a.na < 1 || a.nb < 1 || nslots < 1 ||
      nslots >= (1LL << 31))
    return 2;
  static_assert(MO_MT * MO_FT * 4 <= 64 * MO_WAVES, "one thread per partial sum");
  const dim3 grd((unsigned)nwg, (unsigned)((a.nfreq + MO_FT - 1) / MO_FT),
                 (unsigned)((a.nmodes + MO_MT - 1) / MO_MT));
  if (grd.y > 65535 || grd.z > 65535) return 2;
  mode_overlap_kernel<MO_MT, MO_FT><<<grd, dim3(64 * MO_WAVES), 0, (hipStream_t)stream>>>(a);
  return rc();
}

int k_n2f_farfield(const N2FArgs &a, int nwg, void *stream) {
  if (a.npts <= 0 || nwg <= 0) return 0;
  if (a.nfreq < 1 || a.nruns < 1 || a.wg_blocks < 1) return 2;
  const dim3 grd((unsigned)nwg, (unsigned)((a.nfreq + N2F_FT - 1) / N2F_FT),
                 (unsigned)((a.npts + N2F_NP - 1) / N2F_NP));
  if (grd.y > 65535 || grd.z > 65535) return 2;
  n2f_farfield_kernel<N2F_FT, N2F_NP><<<grd, dim3(64 * N2F_WAVES), 0, (hipStream_t)stream>>>(a);
  return rc();
}

int k_n2f_reduce(const double *part, double *out, int nwg, long long n, void *stream) {
  if (n <= 0) return 0;
  n2f_reduce_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(part, out, nwg,
                                                                                   n);
  return rc();
}

}  // namespace mnl
