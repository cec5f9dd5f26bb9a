// mnl_device.hpp -- what more than one kernel file (.hip) uses: the mapping from a thread to a
// grid point and the point predicates, plus the launchers' small host helpers.  Included only
// by .hip files.  No load / store helper and no body of the fused step lives here: those stay
// in mnl_kernels.hip, whose hash keys the committed HBM-traffic profile.
#pragma once
#include <hip/hip_runtime.h>

#include "mnl_internal.hpp"

// Every kernel is written for 64-lane wavefronts (gfx950): the fused bodies map one 64-column
// row to a wave, nr_hard_kernel runs one attempt per lane with a 64-bit ballot, the DFT and
// far-field kernels block their arrays by 64 slots.
#if defined(__AMDGCN_WAVEFRONT_SIZE) && __AMDGCN_WAVEFRONT_SIZE != 64
#error "the mnl kernels need wave64 (build for gfx950)"
#endif

namespace mnl {

#define MNL_BX 64
#define MNL_BY 4

__device__ __forceinline__ int shift_of(int type, int c, int d) {
  // grid_volume::iyee_shift (src/meep/vec.hpp:1133-1141)
  return (type == T_E || type == T_D) ? (d == c) : (d != c);
}

struct Pt {
  int j[3];       // local index per direction (0 for absent)
  long long idx;  // linear index
};

// little_owned_corner0 .. big_corner (src/meep/vec.hpp:1102-1104), with the
// metallic wall plane left untouched (it is zeroed by zero_metal in the
// reference, src/boundaries.cpp:304-339, and never becomes nonzero).
__device__ __forceinline__ bool owned(const DevGrid &g, int type, int c, const Pt &p) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    if (g.ax[d] < 0) continue;
    if (shift_of(type, c, d)) {
      if (p.j[d] < g.owned_lo_sh[d] || p.j[d] > g.owned_hi_sh[d]) return false;
    } else {
      if (p.j[d] < g.owned_lo_un[d] || p.j[d] > g.owned_hi_un[d]) return false;
    }
  }
  return true;
}

// global half-coordinate (relative to the cell's little corner) of a point
__device__ __forceinline__ int qcoord(const DevGrid &g, const Pt &p, int type, int c, int d) {
  return 2 * (p.j[d] + g.off[d]) + shift_of(type, c, d);
}

__device__ __forceinline__ bool pml_at(const DevFields &f, const DevGrid &g, int d, int q) {
  return g.ax[d] >= 0 && f.pml.flag[d] != nullptr && f.pml.flag[d][q] != 0;
}

// Fused mode: E of comp c at p is not stored but equals chi1inv * D (DESIGN.md
// "Fused step"): p inside the fused domain G, E_c owned there and not in a
// PML chunk along c (where E carries W-form history and is stored).
__device__ __forceinline__ bool e_implicit(const DevFields &f, const DevGrid &g, int c,
                                           const Pt &p) {
  if (!f.fused) return false;
#pragma unroll
  for (int d = 0; d < 3; d++)
    if (p.j[d] < f.fG.lo[d] || p.j[d] > f.fG.hi[d]) return false;
  for (int k = 0; k < f.npol; k++) {  // stored inside a polarization's nonzero box
    const Box &b = f.pol[k].nz;
    if (p.j[0] >= b.lo[0] && p.j[0] <= b.hi[0] && p.j[1] >= b.lo[1] && p.j[1] <= b.hi[1] &&
        p.j[2] >= b.lo[2] && p.j[2] <= b.hi[2])
      return false;
  }
  return owned(g, T_E, c, p) && !pml_at(f, g, c, qcoord(g, p, T_E, c, c));
}

// ----------------------------------------------------------------- host helpers
static inline bool empty(const Box &b) {
  for (int k = 0; k < 3; k++)
    if (b.hi[k] < b.lo[k]) return true;
  return false;
}
static inline int rc() { return hipGetLastError() == hipSuccess ? 0 : -1; }

static inline void canon_strides(const DevGrid &g, long long cs[3]) {
  // canonical whole-cell layout: Z fastest, then Y, then X (src/vec.cpp:482-494)
  long long nz = g.ax[2] >= 0 ? g.nglob[2] + 1 : 1;
  long long ny = g.ax[1] >= 0 ? g.nglob[1] + 1 : 1;
  cs[2] = g.ax[2] >= 0 ? 1 : 0;
  cs[1] = g.ax[1] >= 0 ? nz : 0;
  cs[0] = g.ax[0] >= 0 ? nz * ny : 0;
}

}  // namespace mnl
