// mnl_dft.cpp -- DFT monitors (fields::add_dft_flux / add_dft_fields / update_dfts,
// src/dft.cpp:195-300, src/loop_in_chunks.cpp:257-500): the reference's chunk loop over a
// region, the device point lists, the per-batch phases, the sampling plan and the buffered
// accumulation.
#include "mnl_host.hpp"

namespace mnlh {


// complex slot of (device slot, frequency) in the wave-blocked DFT array

// compute_boundary_weights (src/loop_in_chunks.cpp:257-300), snap_empty_dimensions = false
void dft_boundary_weights(const mnl_structure &S, const double wmin[3], const double wmax[3],
                          const int is[3], const int ie[3], double s0[3], double e0[3],
                          double s1[3], double e1[3]) {
  for (int d = 0; d < 3; d++) {
    s0[d] = s1[d] = e0[d] = e1[d] = 1.0;
    if (!S.has[d]) continue;
    double w0 = 1. - wmin[d] * S.a + 0.5 * is[d];
    double w1 = 1. + wmax[d] * S.a - 0.5 * ie[d];
    if (ie[d] >= is[d] + 3 * 2) {
      s0[d] = w0 * w0 / 2;
      s1[d] = 1 - (1 - w0) * (1 - w0) / 2;
      e0[d] = w1 * w1 / 2;
      e1[d] = 1 - (1 - w1) * (1 - w1) / 2;
    } else if (ie[d] == is[d] + 2 * 2) {
      s0[d] = w0 * w0 / 2;
      s1[d] = 1 - (1 - w0) * (1 - w0) / 2 - (1 - w1) * (1 - w1) / 2;
      e0[d] = w1 * w1 / 2;
      e1[d] = s1[d];
    } else if (wmin[d] == wmax[d]) {
      s0[d] = w0;
      s1[d] = w1;
      e0[d] = w1;
      e1[d] = w0;
    } else if (ie[d] == is[d] + 1 * 2) {
      s0[d] = w0 * w0 / 2 - (1 - w1) * (1 - w1) / 2;
      e0[d] = w1 * w1 / 2 - (1 - w0) * (1 - w0) / 2;
      s1[d] = e0[d];
      e1[d] = s0[d];
    }
  }
}

// the reference's chunks in creation order: x zones outer, then y, then z
// (absolute little corner io and cell counts n per direction)
std::vector<std::array<int, 6>> reference_chunks(const mnl_structure &S) {
  std::vector<std::pair<int, int>> iv[3];
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) {
      iv[d].push_back({0, 0});
      continue;
    }
    for (auto &z : zone_intervals(S, d)) iv[d].push_back({S.io[d] + z.c0, (z.c1 - z.c0) / 2});
  }
  std::vector<std::array<int, 6>> out;
  for (auto &ix : iv[0])
    for (auto &iy : iv[1])
      for (auto &iz : iv[2]) out.push_back({ix.first, iy.first, iz.first, ix.second, iy.second, iz.second});
  return out;
}

// fields::add_dft for component c over [wmin, wmax]: the chunks loop_in_chunks
// creates, prepended to `list` (their points appended to the flux object's point
// arrays).  Centered grid, or with yee the component's own grid (loop_in_chunks(...,
// cgrid = c), src/loop_in_chunks.cpp:350-356: where shifted by yee_shift(Centered) -
// yee_shift(c), rounded to the dielectric grid, shifted back by iyee_c).  sqrt_w: the loop
// weight's square root is applied (sqrt_dV_and_interp_weights, src/dft.cpp:277-280); extra:
// dft_chunk::extra_weight, kept for the force sum.
void dft_add(mnl_fields *F, DftFluxH &o, int c, const double wmin[3], const double wmax[3],
             bool incl, cplx stored_weight, double dt_factor, std::vector<DftChunkH> &list,
             std::vector<double> &pw, bool yee = false, bool sqrt_w = false, double extra = 1.0) {
  const mnl_structure &S = F->S;
  const DevGrid &g = F->g;
  int is[3] = {0, 0, 0}, ie[3] = {0, 0, 0}, sh[3] = {1, 1, 1};
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    if (yee) sh[d] = S.shift(c, d);
    const int iyc = 1 - sh[d];                                          // iyee_c
    const double yc = 1 * (0.5 * (1.0 / S.a)) - sh[d] * (0.5 * (1.0 / S.a));  // yee_c
    is[d] = 1 + 2 * int(floor((wmin[d] + yc) * S.a - .5)) - iyc;  // vec2diel_floor, equal_shift 0
    ie[d] = 1 + 2 * int(ceil((wmax[d] + yc) * S.a - .5)) - iyc;
  }
  double s0[3], s1[3], e0[3], e1[3];
  dft_boundary_weights(S, wmin, wmax, is, ie, s0, e0, s1, e1);
  double dV0 = 1.0;
  for (int d = 0; d < 3; d++)
    if (S.has[d] && wmax[d] - wmin[d] > 0.0) dV0 *= 1.0 / S.a;
  if (!F->allocated[c]) return;
  int yd[3];  // yucky loop directions (3D: X,Y,Z; 2D: Z,X,Y; 1D: X,Y,Z)
  if (S.dim == 2)
    yd[0] = 2, yd[1] = 0, yd[2] = 1;
  else
    yd[0] = 0, yd[1] = 1, yd[2] = 2;
  std::vector<DftChunkH> made;
  LatticeShifts ls(S, F->periodic, wmin, wmax);  // src/loop_in_chunks.cpp:390-532
  do {
  // complex fields: the lattice shift's Bloch phase (src/loop_in_chunks.cpp:409-416), which
  // dft_chunk folds into scale (src/dft.cpp:98, 171); real fields: 1
  cplx shift_phase = 1.0;
  if (is_complex(F))
    for (int d = 0; d < 3; d++)
      if (S.has[d]) shift_phase *= pow((F->part0 ? F->part0 : F)->eikna[d], ls.cur[d]);
  for (auto &ch : reference_chunks(S)) {
    int isc[3], iec[3];
    double s0c[3], s1c[3], e0c[3], e1c[3];
    bool emp = false;
    for (int d = 0; d < 3; d++) {
      s0c[d] = s1c[d] = e0c[d] = e1c[d] = 1.0;
      if (!S.has[d]) {
        isc[d] = iec[d] = 0;
        continue;
      }
      // little_owned_corner(cgrid) = io + 2 - iyee_shift, big_owned_corner = big - iyee_shift
      const int uoc = S.io[d] + 2 - sh[d], coc = ch[d] + 2 - sh[d],
                cbo = ch[d] + 2 * ch[3 + d] - sh[d];
      const int iscoS = std::max(uoc, std::min(coc, cbo)), iecoS = std::max(coc, cbo);
      isc[d] = std::max(is[d] - ls.shifti[d], iscoS);
      iec[d] = std::min(ie[d] - ls.shifti[d], iecoS);
      if (isc[d] > iec[d]) emp = true;
    }
    if (emp) continue;
    for (int d = 0; d < 3; d++) {
      if (!S.has[d]) continue;
      const int iscS = isc[d] + ls.shifti[d], iecS = iec[d] + ls.shifti[d];
      if (iscS == is[d]) {
        s0c[d] = s0[d];
        s1c[d] = s1[d];
      } else if (iscS == is[d] + 2) {
        s0c[d] = s1[d];
      }
      if (iecS == ie[d]) {
        e0c[d] = e0[d];
        e1c[d] = e1[d];
      } else if (iecS == ie[d] - 2) {
        e0c[d] = e1[d];
      }
      if (iec[d] == isc[d]) {
        double w = std::min(s0c[d], e0c[d]);
        s0c[d] = e0c[d] = s1c[d] = e1c[d] = w;
      } else if (iec[d] == isc[d] + 2) {
        double w = std::min(s0c[d], e1c[d]);
        s0c[d] = w, e1c[d] = w;
        w = std::min(s1c[d], e0c[d]);
        s1c[d] = w, e0c[d] = w;
      } else if (iec[d] == isc[d] + 4) {
        double w = std::min(s1c[d], e1c[d]);
        s1c[d] = w, e1c[d] = w;
      }
    }
    DftChunkH dc;
    dc.c = c;
    dc.scale = stored_weight * (is_complex(F) ? shift_phase : cplx(1.0)) * dt_factor;
    int nun = 0;
    for (int d = 0; d < 3; d++)
      if (!yee && S.has[d] && !S.shift(c, d)) nun++;
    dc.avgmode = nun;
    for (int d = 0; d < 3; d++) {
      dc.is[d] = isc[d], dc.ie[d] = iec[d];
      dc.shifti[d] = ls.shifti[d];
      dc.s0[d] = s0c[d], dc.s1[d] = s1c[d], dc.e0[d] = e0c[d], dc.e1[d] = e1c[d];
    }
    dc.dV0 = dV0;
    dc.incl = incl;
    dc.stored = stored_weight;
    dc.sqrt_w = incl && sqrt_w;
    dc.extra = extra;
    long ln[3];
    for (int k = 0; k < 3; k++) ln[k] = S.has[yd[k]] ? (iec[yd[k]] - isc[yd[k]]) / 2 + 1 : 1;
    dc.N = size_t(ln[0] * ln[1] * ln[2]);
    dc.p0 = 0;  // set when the lists are laid out
    auto W1 = [&](int k, long i) -> double {
      const int d = yd[k];
      const long n = ln[k];
      if (i > 1 && i < n - 2) return 1.0;
      if (i == 0) return s0c[d];
      if (i == 1) return s1c[d];
      if (i == n - 1) return e0c[d];
      if (i == n - 2) return e1c[d];
      return 1.0;
    };
    const double fac = nun == 2 ? 0.25 : (nun == 1 ? 0.5 : 1.0);
    // points in IVEC_LOOP_COUNTER order; local indices of the Yee base point
    std::vector<int> pj;
    std::vector<double> w;
    for (long i1 = 0; i1 < ln[0]; i1++)
      for (long i2 = 0; i2 < ln[1]; i2++)
        for (long i3 = 0; i3 < ln[2]; i3++) {
          const long ii[3] = {i1, i2, i3};
          int p[3] = {0, 0, 0};  // centered point, absolute half-coords
          for (int k = 0; k < 3; k++)
            if (S.has[yd[k]]) p[yd[k]] = isc[yd[k]] + 2 * int(ii[k]);
          double wt = incl ? (W1(2, i3) * (W1(1, i2) * ((dV0 + 0.0 * i2) * W1(0, i1)))) : 1.0;
          if (dc.sqrt_w) wt = sqrt(wt);
          w.push_back(wt * fac);
          // this rank owns the centered point if its slab index is in the owned range
          int j[3] = {0, 0, 0};
          bool mine = true;
          for (int d = 0; d < 3; d++) {
            if (!S.has[d]) continue;
            if (yee) {  // the Yee point itself; owned along d by one rank (walls included)
              j[d] = (p[d] - S.io[d] - sh[d]) / 2 - g.off[d];
              const int nloc = g.N[g.ax[d]] - 1;  // this rank's cells along d
              if (sh[d] ? (j[d] < 0 || j[d] > nloc - 1) : (j[d] < 1 || j[d] > nloc)) mine = false;
              continue;
            }
            const int base = p[d] - (S.shift(c, d) ? 0 : 1);  // Yee point of c at/below p
            j[d] = (base - S.io[d] - S.shift(c, d)) / 2 - g.off[d];
            const int jc = (p[d] - S.io[d] - 1) / 2 - g.off[d];  // centered index
            if (jc < g.owned_lo_sh[d] || jc > g.owned_hi_sh[d]) mine = false;
          }
          for (int d = 0; d < 3; d++) pj.push_back(mine ? j[d] : -1);
          if (o.n2f)
            for (int d = 0; d < 3; d++) o.h_pp.push_back(p[d] + ls.shifti[d]);
        }
    dc.p0 = o.h_pj.size() / 3;
    o.h_pj.insert(o.h_pj.end(), pj.begin(), pj.end());
    pw.insert(pw.end(), w.begin(), w.end());
    made.push_back(dc);
  }
  } while (ls.next());
  for (auto &m : made) list.insert(list.begin(), m);
}

static size_t dft_nchunks(const DftFluxH &o) {
  size_t n = 0;
  for (int l = 0; l < o.nlists; l++) n += o.L[l].size();
  return n;
}

// updates per accumulation of a new monitor: DFT_KB, or MNL_DFT_BLOCK (1 .. DFT_KB), read when
// the monitor is added
int dft_block() {
  const char *e = getenv("MNL_DFT_BLOCK");
  return e ? std::max(1, std::min(DFT_KB, atoi(e))) : DFT_KB;
}

// decimation_factor of fields::add_dft (src/dft.cpp:190-213)
int dft_decimation(mnl_fields *F, const double *freqs, int nfreq, int decim) {
  if (decim != 0) return decim;
  double src_freq_max = 0;
  for (auto &st : F->srcs) {
    const double fw = st.kind == 0 ? sqrt(-2.0 * log(1e-7)) / (st.width * pi) : 0.0;
    if (fw == 0)
      decim = 1;
    else
      src_freq_max =
          std::max(src_freq_max, std::abs(st.kind == 0 ? st.freq : st.cfreq.real()) + 0.5 * fw);
  }
  double freq_max = 0;
  for (int i = 0; i < nfreq; ++i) freq_max = std::max(freq_max, std::abs(freqs[i]));
  bool nonlinear = false;  // structure_chunk::has_nonlinearities: nonzero chi2/chi3
  for (int c = 0; c < 3; c++) {
    for (double v : F->S.chi2[c]) nonlinear = nonlinear || v != 0.0;
    for (double v : F->S.chi3[c]) nonlinear = nonlinear || v != 0.0;
  }
  for (auto &b : F->S.boxes) nonlinear = nonlinear || ((b.kind == 1 || b.kind == 2) && b.value != 0.0);
  // (src/dft.cpp:207-210 overwrites the fwidth == 0 case above)
  if ((freq_max > 0) && (src_freq_max > 0) && !nonlinear)
    return std::max(1, int(std::floor(1 / (F->dt * (freq_max + src_freq_max)))));
  return 1;
}

// Device layout of a DFT object whose E list holds the points of `pwE` and whose
// H points (ho) follow: per-point chunk ids, wave-blocked DFT array, slots.
int dft_layout(mnl_fields *F, std::unique_ptr<DftFluxH> &o, DftFluxH &ho, std::vector<double> &pwE,
               std::vector<double> &pwH) {
  const int nfreq = o->nfreq;
  // lay out: E points (creation order), then H points; chunks keep their p0
  // (energy / force objects add every list's points to the object itself: ho is empty)
  const size_t nE = o->h_pj.size() / 3;
  if (!ho.h_pj.empty())
    for (auto &h : o->H) h.p0 += nE;
  o->h_pj.insert(o->h_pj.end(), ho.h_pj.begin(), ho.h_pj.end());
  pwE.insert(pwE.end(), pwH.begin(), pwH.end());
  o->npts = o->h_pj.size() / 3;
  // per-point chunk id: chunks numbered list by list (E list then H list)
  std::vector<int> pch(o->npts, 0);
  std::vector<DftChunkDev> chd;
  auto lay = [&](const std::vector<DftChunkH> &L) {
    for (auto &dc : L) {
      DftChunkDev cd;
      cd.c = dc.c;
      cd.avgmode = dc.avgmode;
      cd.d1 = cd.d2 = -1;  // grid_volume::yee2cent_offsets order (X, Y, Z)
      for (int dd = 0; dd < 3; dd++)
        if (F->S.has[dd] && !F->S.shift(dc.c, dd)) (cd.d1 < 0 ? cd.d1 : cd.d2) = dd;
      for (size_t k = 0; k < dc.N; k++) pch[dc.p0 + k] = (int)chd.size();
      chd.push_back(cd);
    }
  };
  for (int l = 0; l < o->nlists; l++) lay(o->L[l]);
  for (auto &cd : chd) F->dft_samples_d = F->dft_samples_d || cd.c / 3 == T_D;
  // per point and update: 3 indices + chunk id + weight, the averaged field
  // values, the sample written and read back, and 1/kb of a read-modify-write
  // of one complex value per frequency (DESIGN.md "DFT")
  for (int l = 0; l < o->nlists; l++)
    for (auto &dc : o->L[l])
      o->bytes += double(dc.N) * (12 + 4 + 8 + 8.0 * (1 << dc.avgmode) + 16 +
                                  (12 + 4 + 32.0 * nfreq) / o->kb);
  // Device slots: the points sorted by component and chunk, then z, y, x (x fastest like
  // the field arrays), so that a wave's field reads are as contiguous as the
  // plane's orientation allows and a workgroup of the accumulation almost always holds one
  // chunk (one phase row, staged in LDS once); other ranks' points last.  Only the storage
  // order changes -- every point keeps its own reference-order accumulation.
  std::vector<int> ord(o->npts);
  for (size_t p = 0; p < o->npts; p++) ord[p] = (int)p;
  auto key = [&](int p) {
    const int *j = &o->h_pj[3 * (size_t)p];
    return std::make_tuple(j[0] < 0, chd[pch[p]].c, pch[p], j[2], j[1], j[0], p);
  };
  std::sort(ord.begin(), ord.end(), [&](int a, int b) { return key(a) < key(b); });
  o->slot.assign(o->npts, 0);
  std::vector<int> spj(3 * o->npts), spch(o->npts);
  std::vector<double> spw(o->npts);
  for (size_t t = 0; t < o->npts; t++) {
    const int p = ord[t];
    o->slot[p] = (int)t;
    for (int e = 0; e < 3; e++) spj[3 * t + e] = o->h_pj[3 * (size_t)p + e];
    spch[t] = pch[p];
    spw[t] = pwE[p];
  }
  for (int k = 0; k < 3; k++) o->bbox.lo[k] = INT32_MAX, o->bbox.hi[k] = -1;
  for (size_t p = 0; p < o->npts; p++) {
    if (o->h_pj[3 * p] < 0) continue;
    for (int k = 0; k < 3; k++) {
      o->bbox.lo[k] = std::min(o->bbox.lo[k], o->h_pj[3 * p + k]);
      o->bbox.hi[k] = std::max(o->bbox.hi[k], o->h_pj[3 * p + k] + 1);
    }
  }
  // compact box (two-step pairs, 3-D): every bbox cell, 2 states x 6 arrays, <= 1 GiB
  o->cmp_cells = 0, o->cmp_mask = 0;
  if (F->S.dim == 3 && o->bbox.hi[0] >= 0) {
    double nc = 1;
    for (int k = 0; k < 3; k++) nc *= o->bbox.hi[k] - o->bbox.lo[k] + 1;
    if (nc * 96 <= double(1u << 30)) o->cmp_cells = (unsigned)nc;
    for (int l = 0; l < o->nlists; l++)  // E and D samples read D_d (bit d), H and B B_d (3 + d)
      for (auto &dc : o->L[l]) {
        const bool mag = ctype(dc.c) == T_H || ctype(dc.c) == T_B;
        o->cmp_mask |= 1u << (mag ? 3 + cdir(dc.c) : cdir(dc.c));
      }
  }
  if (o->npts) {
    if (dev_alloc(F, &o->d_pj, o->h_pj.size(), false) || dev_alloc(F, &o->d_pch, o->npts, false) ||
        dev_alloc(F, &o->d_pw, o->npts, false) || dev_alloc(F, &o->d_ch, chd.size(), false) ||
        dev_alloc(F, &o->d_dft, 2 * ((o->npts + 63) & ~size_t(63)) * (size_t)nfreq) ||
        dev_alloc(F, &o->d_fr, o->npts * (size_t)o->kb))
      return -1;
    HIPCHK(hipMemcpyAsync(o->d_pj, spj.data(), spj.size() * 4, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(o->d_pch, spch.data(), spch.size() * 4, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(o->d_pw, spw.data(), spw.size() * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(o->d_ch, chd.data(), chd.size() * sizeof(DftChunkDev), hipMemcpyHostToDevice,
                          F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
  }
  F->dfts.push_back(std::move(o));
  dft_sampled_rebuild(F);
  return int(F->dfts.size()) - 1;
}

int dft_add_flux(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                 int decimation) {
  if (F->src_dirty && build_source_lists(F)) return -1;
  if (nreg < 1 || nfreq < 1) return fail("add_dft_flux: no regions / frequencies");
  std::unique_ptr<DftFluxH> o(new DftFluxH);
  o->nfreq = nfreq;
  for (int i = 0; i < nfreq; i++) o->omega.push_back(2 * pi * freqs[i]);
  o->decim = dft_decimation(F, freqs, nfreq, decimation);
  for (int d = 0; d < 3; d++) o->wmin[d] = regions[d], o->wmax[d] = regions[3 + d];
  o->kb = dft_block();
  o->nreg = nreg, o->normal = int(regions[6]);
  const double dt_factor = F->dt / sqrt(2.0 * pi) * o->decim;
  std::vector<double> pwE, pwH;
  DftFluxH ho;  // H points collected separately, appended after the E points
  for (int r = 0; r < nreg; r++) {
    const double *R = regions + 8 * r;
    const int d = int(R[6]);
    const double wgt = R[7];
    int cE[2], cH[2];
    switch (d) {  // fields::add_dft_flux (src/dft.cpp:601-617)
      case 0: cE[0] = MNL_EY, cE[1] = MNL_EZ, cH[0] = MNL_HZ, cH[1] = MNL_HY; break;
      case 1: cE[0] = MNL_EZ, cE[1] = MNL_EX, cH[0] = MNL_HX, cH[1] = MNL_HZ; break;
      default: cE[0] = MNL_EX, cE[1] = MNL_EY, cH[0] = MNL_HY, cH[1] = MNL_HX; break;
    }
    for (int i = 0; i < 2; ++i) {
      dft_add(F, *o, cE[i], R, R + 3, true, cplx(wgt * double(1 - 2 * i)), dt_factor, o->E, pwE);
      dft_add(F, ho, cH[i], R, R + 3, false, cplx(1.0), dt_factor, o->H, pwH);
    }
  }
  return dft_layout(F, o, ho, pwE, pwH);
}

// fields::add_dft_fields (src/dft.cpp:889-903): per component (in order) add_dft
// without dV / interpolation weights, stored_weight 1, prepended to one list; on
// the centered grid or (yee) each component's own grid
int dft_add_fields(mnl_fields *F, int ncomp, const int *comps, const double wmin[3],
                   const double wmax[3], const double *freqs, int nfreq, int yee, int decimation) {
  if (F->src_dirty && build_source_lists(F)) return -1;
  if (ncomp < 1 || nfreq < 1) return fail("add_dft_fields: no components / frequencies");
  for (int k = 0; k < ncomp; k++)
    if (comps[k] < 0 || comps[k] >= MNL_NUM_COMPONENTS)
      return fail("add_dft_fields: not a field component");
  std::unique_ptr<DftFluxH> o(new DftFluxH);
  o->fields = true;
  o->kind = DFT_FIELDS, o->nlists = 1;
  o->nfreq = nfreq;
  for (int i = 0; i < nfreq; i++) o->omega.push_back(2 * pi * freqs[i]);
  o->decim = dft_decimation(F, freqs, nfreq, decimation);
  for (int d = 0; d < 3; d++) o->wmin[d] = wmin[d], o->wmax[d] = wmax[d];
  o->kb = dft_block();
  const double dt_factor = F->dt / sqrt(2.0 * pi) * o->decim;
  std::vector<double> pwE, pwH;
  DftFluxH ho;
  for (int k = 0; k < ncomp; k++)
    dft_add(F, *o, comps[k], wmin, wmax, false, cplx(1.0), dt_factor, o->E, pwE, yee != 0);
  return dft_layout(F, o, ho, pwE, pwH);
}

// ------------------------------------------------------------------ energy, force
static std::unique_ptr<DftFluxH> dft_new(mnl_fields *F, int kind, int nlists, const double *R,
                                         const double *freqs, int nfreq, int decimation) {
  std::unique_ptr<DftFluxH> o(new DftFluxH);
  o->kind = kind, o->nlists = nlists;
  o->nfreq = nfreq;
  for (int i = 0; i < nfreq; i++) o->omega.push_back(2 * pi * freqs[i]);
  o->decim = dft_decimation(F, freqs, nfreq, decimation);
  for (int d = 0; d < 3; d++) o->wmin[d] = R[d], o->wmax[d] = R[3 + d];
  o->kb = dft_block();
  return o;
}

// fields::add_dft_energy (src/dft.cpp:701-727): per region and field direction E_d with the
// dV and interpolation weights, D_d without, H_d with, B_d without, each prepended to its own
// list; centred grid, stored weight 1 (the regions' weights do not enter)
int dft_add_energy(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                   int decimation) {
  if (F->src_dirty && build_source_lists(F)) return -1;
  if (nreg < 1 || nfreq < 1) return fail("add_dft_energy: no regions / frequencies");
  auto o = dft_new(F, DFT_ENERGY, 4, regions, freqs, nfreq, decimation);
  const double dt_factor = F->dt / sqrt(2.0 * pi) * o->decim;
  std::vector<double> pw, none;
  DftFluxH ho;
  for (int r = 0; r < nreg; r++) {
    const double *R = regions + 8 * r;
    for (int d = 0; d < 3; d++) {  // LOOP_OVER_FIELD_DIRECTIONS
      dft_add(F, *o, MNL_EX + d, R, R + 3, true, cplx(1.0), dt_factor, o->L[0], pw);
      dft_add(F, *o, MNL_DX + d, R, R + 3, false, cplx(1.0), dt_factor, o->L[2], pw);
      dft_add(F, *o, MNL_HX + d, R, R + 3, true, cplx(1.0), dt_factor, o->L[1], pw);
      dft_add(F, *o, MNL_BX + d, R, R + 3, false, cplx(1.0), dt_factor, o->L[3], pw);
    }
  }
  return dft_layout(F, o, ho, pw, none);
}

// volume::normal_direction (src/vec.cpp): the one direction of the cell in which the region
// is empty, -1 when there is none or more than one
static int dft_normal_direction(const mnl_structure &S, const double *R) {
  if (S.dim == 1) {
    for (int d = 0; d < 3; d++)
      if (S.has[d]) return d;
    return -1;
  }
  int nd = -1, nzero = 0;
  for (int d = 0; d < 3; d++)
    if (S.has[d] && R[3 + d] - R[d] == 0.0) nd = d, nzero++;
  return nzero == 1 ? nd : -1;
}

// fields::add_dft_force (src/stress.cpp:153-191): the stress tensor's terms on a surface with
// normal nd for the force along fd.  fd != nd: offdiag1 gets E_fd, H_fd (weighted, stored
// weight = the region's), offdiag2 gets E_nd, H_nd (unweighted), centred grid.  fd == nd: diag
// gets E_d, H_d of every field direction with square-root weights and the extra weight
// weight * (+-0.5), on each component's Yee grid.
int dft_add_force(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                  int decimation) {
  if (F->src_dirty && build_source_lists(F)) return -1;
  if (nreg < 1 || nfreq < 1) return fail("add_dft_force: no regions / frequencies");
  auto o = dft_new(F, DFT_FORCE, 3, regions, freqs, nfreq, decimation);
  const double dt_factor = F->dt / sqrt(2.0 * pi) * o->decim;
  std::vector<double> pw, none;
  DftFluxH ho;
  for (int r = 0; r < nreg; r++) {
    const double *R = regions + 8 * r;
    const int nd = dft_normal_direction(F->S, R);
    if (nd < 0) return fail("cannot determine dft_force normal");
    const int fd = int(R[6]);
    const double wgt = R[7];
    if (!(R[6] >= 0 && R[6] <= 2)) return fail("NO_DIRECTION dft_force is invalid");
    for (int d = 0; d < 3; d++) {  // everywhere = the union of the regions
      o->wmin[d] = std::min(o->wmin[d], R[d]);
      o->wmax[d] = std::max(o->wmax[d], R[3 + d]);
    }
    if (fd != nd) {
      dft_add(F, *o, MNL_EX + fd, R, R + 3, true, cplx(wgt), dt_factor, o->L[0], pw);
      dft_add(F, *o, MNL_EX + nd, R, R + 3, false, cplx(1.0), dt_factor, o->L[1], pw);
      dft_add(F, *o, MNL_HX + fd, R, R + 3, true, cplx(wgt), dt_factor, o->L[0], pw);
      dft_add(F, *o, MNL_HX + nd, R, R + 3, false, cplx(1.0), dt_factor, o->L[1], pw);
    } else {
      for (int d = 0; d < 3; d++) {
        const double w1 = wgt * (d == fd ? +0.5 : -0.5);
        dft_add(F, *o, MNL_EX + d, R, R + 3, true, cplx(1.0), dt_factor, o->L[2], pw, true, true, w1);
        dft_add(F, *o, MNL_HX + d, R, R + 3, true, cplx(1.0), dt_factor, o->L[2], pw, true, true, w1);
      }
    }
  }
  return dft_layout(F, o, ho, pw, none);
}

// the runs of lists la and lb zipped (pair_runs, mnl_pair_runs.hpp)
static long long dft_pair_runs(const DftFluxH &o, int la, int lb, double x,
                               std::vector<PairRun> &runs, long long total) {
  std::vector<PairChunk> A, B;
  for (auto &dc : o.L[la]) A.push_back({dc.p0, dc.N, dc.extra});
  for (auto &dc : o.L[lb]) B.push_back({dc.p0, dc.N, dc.extra});
  return pair_runs(A, B, o.h_pj, o.slot, x, runs, total);
}

static int dft_pair_build(mnl_fields *F, DftFluxH &o, int s) {
  DftFluxH::PairSum &ps = o.ps[s];
  if (ps.built) return 0;
  std::vector<PairRun> runs;
  long long total = 0;
  if (o.kind == DFT_ENERGY) {
    total = dft_pair_runs(o, s, 2 + s, 0.5, runs, 0);  // (E, D) or (H, B)
  } else {
    total = dft_pair_runs(o, 0, 1, -1.0, runs, 0);      // stress_sum(offdiag1, offdiag2)
    total = dft_pair_runs(o, 2, 2, -1.0, runs, total);  // stress_sum(diag, diag)
  }
  ps.total = total, ps.nruns = (int)runs.size();
  // the split into workgroups depends on the object alone
  const long long per = std::max<long long>(PS_WG_PTS, (total + PS_MAX_WG - 1) / PS_MAX_WG);
  ps.wg_pts = (int)((per + 255) / 256 * 256);
  ps.nwg = (int)((total + ps.wg_pts - 1) / ps.wg_pts);
  if (!runs.empty()) {
    HIPCHK(hipMalloc(&ps.d_runs, runs.size() * sizeof(PairRun)));
    HIPCHK(hipMemcpyAsync(ps.d_runs, runs.data(), runs.size() * sizeof(PairRun),
                          hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));  // runs leaves scope
  }
  ps.built = true;
  return 0;
}

// one pair sum on the device, all-reduced like flux(): out[nfreq]
static int dft_pair_sum(mnl_fields *F, DftFluxH &o, int s, double *out) {
  const size_t nf = o.nfreq;
  for (size_t i = 0; i < nf; ++i) out[i] = 0;
  std::string why;
  bool ok = true;
  auto run = [&]() -> int {
    if (dft_flush(F, o)) return -1;  // the buffered updates first (same stream)
    if (dft_pair_build(F, o, s)) return -1;
    const DftFluxH::PairSum &ps = o.ps[s];
    if (!ps.total) return 0;
    const size_t need = (size_t)ps.nwg * nf;
    if (o.ps_part_cap < need) {
      HIPCHK(hipStreamSynchronize(F->stream));
      if (o.d_ps_part) (void)hipFree(o.d_ps_part);
      o.d_ps_part = nullptr, o.ps_part_cap = 0;
      HIPCHK(hipMalloc(&o.d_ps_part, need * 8));
      o.ps_part_cap = need;
    }
    if (!o.d_ps_out) HIPCHK(hipMalloc(&o.d_ps_out, nf * 8));
    if (k_dft_pair_sum(o.d_dft, ps.d_runs, ps.nruns, ps.total, ps.wg_pts, ps.nwg, o.nfreq,
                       (long long)((o.npts + 63) & ~size_t(63)), o.d_ps_part, F->stream))
      return fail("dft pair sum launch failed");
    if (k_n2f_reduce(o.d_ps_part, o.d_ps_out, ps.nwg, (long long)nf, F->stream))
      return fail("dft pair sum reduce launch failed");
    HIPCHK(hipMemcpyAsync(out, o.d_ps_out, nf * 8, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    return 0;
  };
  if (run()) ok = false, why = g_err;
  if (F->nranks > 1) {
    if (F->comm->agree_ok(ok, F->stream))  // every rank fails together
      return ok ? fail("dft pair sum: a rank failed") : (g_err = why, -1);
    for (size_t i0 = 0; i0 < nf; i0 += 64)  // sum_to_all
      if (timed_allreduce(F, out + i0, (int)std::min<size_t>(64, nf - i0)))
        return fail("dft pair sum allreduce failed");
  }
  if (!ok) return g_err = why, -1;
  return 0;
}

// dft_energy::electric / magnetic / total (src/dft.cpp:657-699): which 0, 1, 2
int dft_energy_values(mnl_fields *F, int h, int which, double *out) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (o.kind != DFT_ENERGY) return fail("dft_energy: the handle is not an energy object");
  if (which < 0 || which > 2)
    return fail("dft_energy: which must be 0 (electric), 1 (magnetic) or 2 (total)");
  if (which < 2) return dft_pair_sum(F, o, which, out);
  std::vector<double> m(o.nfreq);
  if (dft_pair_sum(F, o, 0, out) || dft_pair_sum(F, o, 1, m.data())) return -1;
  for (int i = 0; i < o.nfreq; i++) out[i] = out[i] + m[i];
  return 0;
}

// dft_force::force (src/stress.cpp:101-114)
int dft_force_values(mnl_fields *F, int h, double *out) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (o.kind != DFT_FORCE) return fail("dft_force: the handle is not a force object");
  return dft_pair_sum(F, o, 0, out);
}

// per point of list `which` in list order: x, y, z of the DFT point (IVEC_LOOP_LOC), the
// component, and the loop weight as update_dft applies it (after the square root; 1.0 for
// unweighted lists).  Recomputed from the chunks' loops, not stored.
int dft_points(mnl_fields *F, int h, int which, double *out, long long npoints) {
  if (dft_bad_handle(F, h)) return -1;
  const DftFluxH &o = *F->dfts[h];
  if (dft_bad_which(o, which)) return fail("dft_points: no such list");
  const mnl_structure &S = F->S;
  const int yd[3] = {S.dim == 2 ? 2 : 0, S.dim == 2 ? 0 : 1, S.dim == 2 ? 1 : 2};
  long long k = 0;
  for (auto &dc : o.L[which]) {
    int n[3];
    for (int q = 0; q < 3; q++) n[q] = S.has[yd[q]] ? (dc.ie[yd[q]] - dc.is[yd[q]]) / 2 + 1 : 1;
    for (int i1 = 0; i1 < n[0]; i1++)
      for (int i2 = 0; i2 < n[1]; i2++)
        for (int i3 = 0; i3 < n[2]; i3++, k++) {
          if (k >= npoints) return fail("dft_points: buffer too small");
          const int ii[3] = {i1, i2, i3};
          double wl[3];
          for (int q = 0; q < 3; q++) {
            const int d = yd[q];
            wl[q] = loop_w1(dc.s0[d], dc.s1[d], dc.e0[d], dc.e1[d], ii[q], n[q]);
            out[5 * k + d] =
                S.has[d] ? (dc.is[d] + dc.shifti[d] + 2 * ii[q]) * (0.5 * (1.0 / S.a)) : 0.0;
          }
          double w = dc.incl ? wl[2] * (wl[1] * ((dc.dV0 + 0.0 * i2) * wl[0])) : 1.0;
          if (dc.sqrt_w) w = sqrt(w);
          out[5 * k + 3] = dc.c;
          out[5 * k + 4] = w;
        }
  }
  return 0;
}

// ------------------------------------------------------------------ near2far
// fields::get_eps / get_mu (src/monitor.cpp:202-224): the number of components over the
// trace of the interpolated diagonal chi1inv at pos
double n2f_medium_at(const mnl_structure &S, int t, const double pos[3]) {
  double tr = 0;
  int nc = 0;
  for (int k = 0; k < 3; k++) {
    const int c = (t == T_E ? MNL_EX : MNL_HX) + k;
    if (!has_field(S, c)) continue;
    int locs[8][3];
    double w[8];
    interpolate(S, c, pos, locs, w);
    double v = 0;
    for (int i = 0; i < 8 && w[i]; i++) {
      int j[3] = {0, 0, 0};
      bool in = true;
      for (int d = 0; d < 3; d++) {
        if (!S.has[d]) continue;
        const int h = locs[i][d] - S.io[d] - S.shift(c, d);
        j[d] = h / 2;
        if (h < 0 || j[d] > S.n[d]) in = false;
      }
      if (in) v += w[i] * mat_diag_at(S, t, k, j);
    }
    tr += v;
    nc++;
  }
  return nc / tr;
}

static bool n2f_approxeq(double a, double b) { return fabs(a - b) < 0.5e-11 * (fabs(a) + fabs(b)); }

// fields::add_dft_near2far (src/near2far.cpp:558-642): per region the two tangential E and the
// two tangential H components on their own Yee grids with dV and interpolation weights, the
// stored weight signed as n x field; every chunk in one list, with its equivalent current c0
int dft_add_near2far(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                     int decimation, int nperiods) {
  if (F->src_dirty && build_source_lists(F)) return -1;
  if (nreg < 1 || nfreq < 1) return fail("add_dft_near2far: no regions / frequencies");
  const mnl_structure &S = F->S;
  if (S.dim != 3) return fail("add_dft_near2far: 3-D only (no green2d / greencyl in this build)");
  if (nperiods > 1)
    return fail("add_dft_near2far: periodic near2far (nperiods > 1) needs periodic boundaries, "
                "which this build does not have");
  std::unique_ptr<DftFluxH> o(new DftFluxH);
  o->fields = true;  // chunks in E only
  o->n2f = true;
  o->kind = DFT_N2F, o->nlists = 1;
  o->nfreq = nfreq;
  for (int i = 0; i < nfreq; i++) o->omega.push_back(2 * pi * freqs[i]), o->freq.push_back(freqs[i]);
  o->decim = dft_decimation(F, freqs, nfreq, decimation);
  for (int d = 0; d < 3; d++) o->wmin[d] = regions[d], o->wmax[d] = regions[3 + d];
  o->kb = dft_block();
  const double dt_factor = F->dt / sqrt(2.0 * pi) * o->decim;
  std::vector<double> pw, pwH;
  DftFluxH ho;
  double eps = 0, mu = 0;
  for (int r = 0; r < nreg; r++) {
    const double *R = regions + 8 * r;
    const int nd = int(R[6]);
    const double wgt = R[7];
    for (int d = 0; d < 3; d++) {  // everywhere = the union of the regions
      o->wmin[d] = std::min(o->wmin[d], R[d]);
      o->wmax[d] = std::max(o->wmax[d], R[3 + d]);
    }
    const double cen[3] = {0.5 * (R[0] + R[3]), 0.5 * (R[1] + R[4]), 0.5 * (R[2] + R[5])};
    const double weps = n2f_medium_at(S, T_E, cen), wmu = n2f_medium_at(S, T_H, cen);
    if (r > 0 && !(n2f_approxeq(eps, weps) && n2f_approxeq(mu, wmu)))
      return fail("dft_near2far requires surfaces in a homogeneous medium");
    eps = weps, mu = wmu;
    const int fd[2] = {(nd + 1) % 3, (nd + 2) % 3};  // cyclic: the sign s below is that of n x c
    for (int i = 0; i < 2; ++i)      // E or H
      for (int j = 0; j < 2; ++j) {  // first or second component
        const int c = (i == 0 ? MNL_EX : MNL_HX) + fd[j];
        const int c0 = (i == 0 ? MNL_HX : MNL_EX) + fd[1 - j];
        double s = j == 0 ? 1 : -1;
        if (i == 0) s = -s;
        const size_t before = o->E.size();
        dft_add(F, *o, c, R, R + 3, true, cplx(s * wgt), dt_factor, o->E, pw, true);
        for (size_t k = 0; k + before < o->E.size(); k++) o->E[k].c0 = c0;  // prepended
      }
  }
  o->eps = eps, o->mu = mu;
  o->h_pw = pw;
  const int h = dft_layout(F, o, ho, pw, pwH);
  if (h < 0) return -1;
  DftFluxH &q = *F->dfts[h];
  // Yee positions (IVEC_LOOP_LOC: half-pixel coordinate * 0.5 / a) and c0 in slot order
  const size_t npad = (q.npts + 63) & ~size_t(63);
  std::vector<double> x0(3 * npad, 0.0);
  std::vector<int> sc0(q.npts, -1);
  q.nmine = 0;
  for (auto &dc : q.E)
    for (size_t p = dc.p0; p < dc.p0 + dc.N; p++) {
      const size_t t = q.slot[p];
      sc0[t] = dc.c0;
      for (int d = 0; d < 3; d++) x0[d * npad + t] = q.h_pp[3 * p + d] * (0.5 * (1.0 / S.a));
      if (q.h_pj[3 * p] >= 0) q.nmine++;
    }
  std::vector<N2FRun> runs;
  for (size_t t = 0; t < q.nmine; t++) {
    if (runs.empty() || runs.back().c0 != sc0[t]) runs.push_back({(int)t, 0, sc0[t]});
    runs.back().count++;
  }
  q.nruns = (int)runs.size();
  // the split of the slots into workgroups depends on the object alone
  const long long nblk = ((long long)q.nmine + 63) / 64;
  q.n2f_wg_blocks = (int)std::max<long long>(N2F_WG_BLOCKS, (nblk + N2F_MAX_WG - 1) / N2F_MAX_WG);
  q.n2f_nwg = (int)((nblk + q.n2f_wg_blocks - 1) / q.n2f_wg_blocks);
  if (q.npts) {
    if (dev_alloc(F, &q.d_x0, x0.size(), false) || dev_alloc(F, &q.d_freq, (size_t)nfreq, false) ||
        dev_alloc(F, &q.d_runs, std::max<size_t>(runs.size(), 1), false))
      return -1;
    HIPCHK(hipMemcpyAsync(q.d_x0, x0.data(), x0.size() * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(q.d_freq, q.freq.data(), (size_t)nfreq * 8, hipMemcpyHostToDevice,
                          F->stream));
    if (!runs.empty())
      HIPCHK(hipMemcpyAsync(q.d_runs, runs.data(), runs.size() * sizeof(N2FRun),
                            hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
  }
  return h;
}

// per point of the list (the order of mnl_fields_dft_data): x, y, z, c0, weight
int n2f_points(mnl_fields *F, int h, double *out, long long npoints) {
  if (dft_bad_handle(F, h)) return -1;
  const DftFluxH &o = *F->dfts[h];
  if (!o.n2f) return fail("near2far_points: the handle is not a near2far object");
  long long k = 0;
  for (auto &dc : o.E)
    for (size_t p = dc.p0; p < dc.p0 + dc.N; p++, k++) {
      if (k >= npoints) return fail("near2far_points: buffer too small");
      for (int d = 0; d < 3; d++) out[5 * k + d] = o.h_pp[3 * p + d] * (0.5 * (1.0 / F->S.a));
      out[5 * k + 3] = dc.c0;
      out[5 * k + 4] = o.h_pw[p] * real(dc.stored);
    }
  return 0;
}

// dft_near2far::farfield (src/near2far.cpp:340-398) for npts points, summed over ranks:
// out[npts][nfreq][6] complex.  Far points go through the kernels in batches that fit the
// scratch buffer of partial sums; the batching does not change any point's result.
int n2f_farfields(mnl_fields *F, int h, long long npts, const double *xyz, double *out) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (!o.n2f) return fail("near2far_farfields: the handle is not a near2far object");
  if (npts < 0) return fail("near2far_farfields: negative point count");
  const size_t per = (size_t)o.nfreq * 12;  // doubles per far point
  for (size_t i = 0; i < (size_t)npts * per; i++) out[i] = 0.0;
  std::string why;
  bool ok = true;
  const double t_start = wall_now();
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  auto run = [&]() -> int {
    if (dft_flush(F, o)) return -1;  // the buffered updates first (same stream)
    if (!o.nmine || !npts) return 0;
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    // batch: partial sums of at most 256 MiB, and the grid's z limit
    const size_t cap = (size_t(256) << 20) / 8;
    long long nb = std::max<size_t>(1, cap / ((size_t)o.n2f_nwg * per));
    nb = std::min<long long>({nb, npts, 65535LL * N2F_NP});
    if (o.n2f_part_cap < (size_t)o.n2f_nwg * nb * per || o.n2f_pts_cap < (size_t)nb) {
      HIPCHK(hipStreamSynchronize(F->stream));
      if (o.d_n2f_part) (void)hipFree(o.d_n2f_part);
      if (o.d_n2f_xyz) (void)hipFree(o.d_n2f_xyz);
      if (o.d_n2f_out) (void)hipFree(o.d_n2f_out);
      o.d_n2f_part = o.d_n2f_xyz = o.d_n2f_out = nullptr;
      o.n2f_part_cap = o.n2f_pts_cap = 0;
      HIPCHK(hipMalloc(&o.d_n2f_part, (size_t)o.n2f_nwg * nb * per * 8));
      HIPCHK(hipMalloc(&o.d_n2f_xyz, (size_t)nb * 3 * 8));
      HIPCHK(hipMalloc(&o.d_n2f_out, (size_t)nb * per * 8));
      o.n2f_part_cap = (size_t)o.n2f_nwg * nb * per;
      o.n2f_pts_cap = (size_t)nb;
    }
    N2FArgs a{};
    a.dft = o.d_dft, a.x0 = o.d_x0, a.runs = o.d_runs, a.nruns = o.nruns;
    a.nslots = (long long)o.nmine, a.npad = (long long)((o.npts + 63) & ~size_t(63));
    a.nfreq = o.nfreq, a.freq = o.d_freq, a.eps = o.eps, a.mu = o.mu;
    a.xyz = o.d_n2f_xyz, a.wg_blocks = o.n2f_wg_blocks, a.part = o.d_n2f_part;
    for (long long p0 = 0; p0 < npts; p0 += nb) {
      const long long n = std::min(nb, npts - p0);
      a.npts = (int)n;
      HIPCHK(hipMemcpyAsync(o.d_n2f_xyz, xyz + 3 * p0, (size_t)n * 24, hipMemcpyHostToDevice,
                            F->stream));
      HIPCHK(hipEventRecord(ev[0], F->stream));
      if (k_n2f_farfield(a, o.n2f_nwg, F->stream))
        return fail("near2far farfield launch failed");
      HIPCHK(hipEventRecord(ev[1], F->stream));
      if (k_n2f_reduce(o.d_n2f_part, o.d_n2f_out, o.n2f_nwg, n * (long long)per, F->stream))
        return fail("near2far reduce launch failed");
      HIPCHK(hipEventRecord(ev[2], F->stream));
      HIPCHK(hipMemcpyAsync(out + p0 * per, o.d_n2f_out, (size_t)n * per * 8,
                            hipMemcpyDeviceToHost, F->stream));
      HIPCHK(hipStreamSynchronize(F->stream));  // xyz and out are reused by the next batch
      for (int k = 0; k < 2; k++) {  // kernel_stats 9 / 10
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
        F->n2f_ms[k] += ms;
        F->n2f_count[k]++;
      }
    }
    return 0;
  };
  if (run()) ok = false, why = g_err;
  for (auto &e : ev)
    if (e) (void)hipEventDestroy(e);
  F->sink_s[MNL_SINK_FARFIELDS] += wall_now() - t_start;  // GetFarfieldsTime
  if (F->nranks > 1) {
    if (F->comm->agree_ok(ok, F->stream))  // every rank fails together
      return ok ? fail("near2far_farfields: a rank failed") : (g_err = why, -1);
    const size_t tot = (size_t)npts * per;
    for (size_t i0 = 0; i0 < tot; i0 += 64)  // sum_to_all
      if (timed_allreduce(F, out + i0, (int)std::min<size_t>(64, tot - i0)))
        return fail("near2far_farfields allreduce failed");
  }
  if (!ok) return g_err = why, -1;
  return 0;
}

// phases of every DFT update in steps [t0+1, t0+ns] -> device (one row per update), after
// the rows of the updates still buffered from earlier calls (accumulated by the next flush:
// when kb updates are buffered or before the DFT array is read, not at the end of every call)
int dft_prepare(mnl_fields *F, long long t0, int ns) {
  for (auto &op : F->dfts) {  // (probes have no phases)
    DftFluxH &o = *op;
    const size_t nch = dft_nchunks(o);
    const size_t rowlen = 2 * nch * (size_t)o.nfreq;
    std::vector<double> ph;
    ph.reserve(((size_t)o.nbuf + ns) * rowlen);
    if (o.nbuf > 0) {
      if (o.ph_host.size() < (size_t)o.row * rowlen || o.row < o.nbuf)
        return fail("dft: buffered phase rows lost");
      ph.insert(ph.end(), o.ph_host.begin() + (size_t)(o.row - o.nbuf) * rowlen,
                o.ph_host.begin() + (size_t)o.row * rowlen);
    }
    o.row = o.nbuf;
    std::vector<cplx> pe(o.nfreq), phh(o.nfreq);
    for (int s = 0; s < ns; s++) {
      const long long t = t0 + s + 1;
      if (t % o.decim) continue;
      const double tE = t * F->dt, tH = tE - 0.5 * F->dt;  // fields::update_dfts
      // exp(i omega t) once per frequency and time (E / H), then times each chunk's scale:
      // the same operations as the reference's per-chunk polar(1, omega t) * scale
      for (int i = 0; i < o.nfreq; i++) {
        pe[i] = std::polar(1.0, o.omega[i] * tE);
        phh[i] = std::polar(1.0, o.omega[i] * tH);
      }
      // chunks with the same time and the same scale (bitwise) share one row of products
      std::vector<std::pair<std::pair<bool, cplx>, size_t>> done;
      auto same = [](const cplx &x, const cplx &y) {
        return memcmp(&x, &y, sizeof(cplx)) == 0;
      };
      auto add = [&](const std::vector<DftChunkH> &L) {
        for (auto &dc : L) {
          const bool isH = ctype(dc.c) == T_H || ctype(dc.c) == T_B;  // is_H_or_B: t - dt/2
          size_t from = SIZE_MAX;
          for (auto &d : done)
            if (d.first.first == isH && same(d.first.second, dc.scale)) from = d.second;
          const size_t at = ph.size();
          if (from != SIZE_MAX) {
            for (int i = 0; i < 2 * o.nfreq; i++) ph.push_back(ph[from + i]);
            continue;
          }
          done.push_back({{isH, dc.scale}, at});
          const std::vector<cplx> &pt = isH ? phh : pe;
          for (int i = 0; i < o.nfreq; i++) {
            const cplx p = pt[i] * dc.scale;
            ph.push_back(p.real());
            ph.push_back(p.imag());
          }
        }
      };
      for (int l = 0; l < o.nlists; l++) add(o.L[l]);
    }
    if (ph.empty()) {
      o.ph_host.clear();
      continue;
    }
    if (o.ph_cap < ph.size()) {
      HIPCHK(hipStreamSynchronize(F->stream));
      if (o.d_ph) hipFree(o.d_ph);
      HIPCHK(hipMalloc(&o.d_ph, ph.size() * 8));
      o.ph_cap = ph.size();
    }
    (void)nch;
    HIPCHK(hipMemcpyAsync(o.d_ph, ph.data(), ph.size() * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    o.ph_host.swap(ph);
  }
  return 0;
}

// accumulate the buffered updates of one flux object
int dft_flush(mnl_fields *F, DftFluxH &o) {
  if (!o.nbuf) return 0;
  if (o.kind == DFT_PROBE) return probe_flush(F, o);
  if (o.kind == DFT_LDOS) return ldos_flush(F, o);
  const size_t nch = dft_nchunks(o);
  const long long rstride = (long long)(nch * o.nfreq);
  // Complex fields: part 1's object only samples; its rows are
  // accumulated with part 0's, dft += phase * (f_re + i f_im) per update in update order
  // (dft_chunk::update_dft, src/dft.cpp:295-299), into part 0's array, which every reader reads.
  if (F->part0) return 0;
  if (mnl_fields *T = F->twin.get()) {
    size_t h = 0;
    while (h < F->dfts.size() && F->dfts[h].get() != &o) h++;
    if (h >= T->dfts.size()) return fail("dft: the parts of the complex fields differ");
    DftFluxH &o1 = *T->dfts[h];
    if (o1.nbuf != o.nbuf || o1.npts != o.npts)
      return fail("dft: the parts of the complex fields differ");
    if (k_dft_accum_cplx(o.d_pj, o.d_pch, o.d_dft, o.d_fr, o1.d_fr, o.nbuf,
                         o.d_ph + 2 * (size_t)(o.row - o.nbuf) * rstride, rstride, o.nfreq,
                         (long long)o.npts, F->stream))
      return fail("dft accumulate launch failed");
    o.nbuf = o1.nbuf = 0;
    return 0;
  }
  if (k_dft_accum(o.d_pj, o.d_pch, o.d_dft, o.d_fr, o.nbuf,
                  o.d_ph + 2 * (size_t)(o.row - o.nbuf) * rstride, rstride, o.nfreq,
                  (long long)o.npts, F->stream))
    return fail("dft accumulate launch failed");
  o.nbuf = 0;
  return 0;
}

// after step t (fields::update_dfts, src/dft.cpp:249-263)
// what a sampling plan depends on: implicit E (the fused mode and its geometry) and which H
// components are stored separately
long long dft_plan_key(const mnl_fields *F) {
  long long k = (long long)F->fused_epoch * 2 + (F->fused ? 1 : 0);
  for (int d = 0; d < 3; d++) k = k * 2 + (F->f.H[d] ? 1 : 0);
  return k * 2 + (F->f.hall ? 1 : 0);
}

// fields: the buffer set to sample (null: the current one; temporal blocking samples the middle
// step of a pair from the mid set)
// cstate >= 0: a pair's middle (0) or new (1) state, whose two-step points are also in the
// monitors' compact boxes
int dft_update(mnl_fields *F, long long t, const DevFields *fields, int cstate, DftFluxH *only) {
  const bool planned = F->nlocal < (size_t(1) << 31);  // int32 indices in the plan
  const DevFields &fs = fields ? *fields : F->f;
  auto skip = [&](const DftFluxH &o) { return only ? &o != only || !o.npts : !dft_samples_at(o, t); };
  // the samples of every flux object due: planned ones in merged launches of up to DFT_MAXJ
  DftSampleJobs J{};
  auto launch = [&]() -> int {
    if (J.n && k_dft_sample_jobs(J, F->g, fs, F->d_utab, F->stream))
      return fail("dft sample launch failed");
    J = DftSampleJobs{};
    return 0;
  };
  for (DftFluxH *op : F->sampled) {
    DftFluxH &o = *op;
    if (skip(o)) continue;
    double *fr = o.d_fr + (size_t)o.nbuf * o.npts;
    if (planned) {
      const long long key = dft_plan_key(F);
      if (o.plan_key != key) {
        if (!o.d_sidx) {
          HIPCHK(hipMalloc(&o.d_sidx, o.npts * 4));
          HIPCHK(hipMalloc(&o.d_ssel, o.npts * 2));
          HIPCHK(hipMalloc(&o.d_spal, o.npts * 4));
          HIPCHK(hipMalloc(&o.d_su, o.npts * 32));
          HIPCHK(hipMalloc(&o.d_bad, sizeof(int)));
        }
        if (o.cmp_cells && !o.d_sci) HIPCHK(hipMalloc(&o.d_sci, o.npts * 4));
        const bool pal = F->fused && F->d_uidx && F->d_utab && F->dft_pal;
        HIPCHK(hipMemsetAsync(o.d_bad, 0, sizeof(int), F->stream));
        if (k_dft_plan(o.d_pj, o.d_pch, o.d_ch, (long long)o.npts, F->g, F->f,
                       pal ? F->d_uidx : nullptr, pal ? F->d_utab : nullptr, o.d_sidx, o.d_ssel,
                       o.d_spal, o.d_su, o.d_bad, o.bbox, o.cmp_cells ? o.d_sci : nullptr,
                       F->pal_one, F->stream))
          return fail("dft plan launch failed");
        int bad = 1;
        if (pal) {  // once per plan: are the palette bytes exact for every implicit value?
          HIPCHK(hipMemcpyAsync(&bad, o.d_bad, sizeof(int), hipMemcpyDeviceToHost, F->stream));
          HIPCHK(hipStreamSynchronize(F->stream));
        }
        o.usepal = pal && bad == 0;
        o.plan_key = key;
      }
      if (J.n == DFT_MAXJ && launch()) return -1;
      DftSampleJob &jb = J.j[J.n++];
      jb.sidx = o.d_sidx, jb.ssel = o.d_ssel, jb.spal = o.d_spal, jb.su = o.d_su;
      jb.pw = o.d_pw, jb.fr = fr, jb.npts = (long long)o.npts, jb.blk0 = J.nblk;
      jb.usepal = o.usepal ? 1 : 0;
      if (cstate >= 0 && o.cmp_on && o.d_cmp && o.d_sci) {
        jb.sci = o.d_sci;
        jb.cmp = o.d_cmp + (size_t)cstate * 6 * o.cmp_cells;
        jb.ncell = o.cmp_cells;
        const int n0 = o.bbox.hi[0] - o.bbox.lo[0] + 1, n1 = o.bbox.hi[1] - o.bbox.lo[1] + 1;
        for (int e = 0; e < 3; e++) {
          const int ax = F->g.ax[e];
          jb.cs[e] = ax == 0 ? 1 : ax == 1 ? n0 : ax == 2 ? n0 * n1 : 0;
        }
      }
      J.nblk += ((long long)o.npts + 255) / 256;
    } else if (k_dft_sample(o.d_pj, o.d_pw, o.d_pch, o.d_ch, fr, (long long)o.npts, F->g, fs,
                            F->stream)) {
      return fail("dft sample launch failed");
    }
  }
  if (launch()) return -1;
  for (DftFluxH *op : F->sampled) {
    DftFluxH &o = *op;
    if (skip(o)) continue;
    o.nbuf++;
    o.row++;
    if (o.kind == DFT_LDOS) ldos_sampled(F, o);
    if (o.nbuf == o.kb && dft_flush(F, o)) return -1;
  }
  return 0;
}

bool dft_due(const mnl_fields *F, long long t) {
  for (DftFluxH *op : F->sampled)
    if (dft_samples_at(*op, t)) return true;
  return false;
}


int dft_flux_values(mnl_fields *F, int h, double *out) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (dft_flush(F, o)) return -1;  // the buffered updates first
  const size_t nf = o.nfreq;
  std::vector<double> v(2 * ((o.npts + 63) & ~size_t(63)) * nf);
  bool ok = true;
  if (!v.empty())
    ok = hipMemcpyAsync(v.data(), o.d_dft, v.size() * 8, hipMemcpyDeviceToHost, F->stream) ==
             hipSuccess &&
         hipStreamSynchronize(F->stream) == hipSuccess;
  if (F->nranks > 1 && F->comm->agree_ok(ok, F->stream))  // every rank fails together
    return fail(ok ? "flux: a rank failed" : "flux: device copy failed");
  if (!ok) return fail("flux: device copy failed");
  for (size_t i = 0; i < nf; ++i) out[i] = 0;
  for (size_t k = 0; k < o.E.size() && k < o.H.size(); k++)  // dft_flux::flux (src/dft.cpp:533-547)
    for (size_t p = 0; p < o.E[k].N; ++p) {
      const size_t pe = o.E[k].p0 + p, ph = o.H[k].p0 + p;
      if (o.h_pj[3 * pe] < 0 && o.h_pj[3 * pe + 1] < 0 && o.h_pj[3 * pe + 2] < 0) continue;
      for (size_t i = 0; i < nf; ++i) {
        const size_t ie = dft_at(o.slot[pe], i, nf), ih = dft_at(o.slot[ph], i, nf);
        const cplx e(v[2 * ie], v[2 * ie + 1]);
        const cplx hv(v[2 * ih], v[2 * ih + 1]);
        out[i] += real(e * conj(hv));
      }
    }
  if (F->nranks > 1)
    for (size_t i0 = 0; i0 < nf; i0 += 64)
      if (timed_allreduce(F, out + i0, (int)std::min<size_t>(64, nf - i0)))
        return fail("flux allreduce failed");
  return 0;
}

// fields::get_dft_array(dft_flux / dft_fields, c, num_freq) (src/dft.cpp:1240-1280):
// process_dft_component into a whole array (get_dft_component_dims corners; every
// chunk of c in list order; dft / stored_weight, divided by the loop weight when the
// chunk stored it; times the interpolation weights of the empty dimensions,
// src/dft.cpp:908-1040), summed over ranks (sum_to_all: one owner per point), then
// collapse_array (src/array_slice.cpp:554-601).  out: re/im interleaved.
int dft_array(mnl_fields *F, int h, int c, int num_freq, int *rank, long long dims[3], double *out,
              long long nout) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (o.kind == DFT_ENERGY || o.kind == DFT_FORCE)
    return fail("get_dft_array: not available for energy and force objects in this build");
  if (dft_flush(F, o)) return -1;  // the buffered updates first
  if (num_freq < 0 || num_freq > o.nfreq - 1)
    return fail(("process_dft_component: frequency index " + std::to_string(num_freq) +
                 " is outside the range of the frequency array of size " +
                 std::to_string(o.nfreq)).c_str());
  const mnl_structure &S = F->S;
  std::vector<const DftChunkH *> L;
  for (auto &dc : o.E)
    if (dc.c == c) L.push_back(&dc);
  for (auto &dc : o.H)
    if (dc.c == c) L.push_back(&dc);
  for (auto *dc : L)
    if (dc->shifti[0] || dc->shifti[1] || dc->shifti[2])
      return fail("get_dft_array: a region that reaches a periodic face (image chunks) is not "
                  "supported");
  int mn[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, mx[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (auto *dc : L)
    for (int d = 0; d < 3; d++) mn[d] = std::min(mn[d], dc->is[d]), mx[d] = std::max(mx[d], dc->ie[d]);
  int r = 0, ds[3] = {0, 0, 0};
  long long full[3] = {1, 1, 1};
  if (!L.empty())
    for (int d = 0; d < 3; d++) {
      if (!S.has[d]) continue;
      long long n = (mx[d] - mn[d]) / 2 + 1;
      if (n > 1) ds[r] = d, full[r++] = n;
    }
  int rr = 0;  // collapse_array: directions empty in `where` are summed out
  long long rd[3] = {1, 1, 1};
  for (int k = 0; k < r; k++)
    if (o.wmax[ds[k]] - o.wmin[ds[k]] != 0.0) rd[rr++] = full[k];
  *rank = rr;
  for (int k = 0; k < 3; k++) dims[k] = k < rr ? rd[k] : 1;
  if (!out) return 0;
  long long rs[3] = {0, 0, 0}, nred = 1;
  for (int k = r - 1; k >= 0; k--)
    if (o.wmax[ds[k]] - o.wmin[ds[k]] != 0.0) rs[k] = nred, nred *= full[k];
  if (r == 0) nred = 0;
  if (nout < nred) return fail("output buffer too small");
  for (long long k = 0; k < 2 * nred; k++) out[k] = 0.0;
  if (r == 0) return 0;
  const size_t nf = o.nfreq;
  std::vector<double> v(2 * ((o.npts + 63) & ~size_t(63)) * nf);
  bool ok = true;
  if (!v.empty())
    ok = hipMemcpyAsync(v.data(), o.d_dft, v.size() * 8, hipMemcpyDeviceToHost, F->stream) ==
             hipSuccess &&
         hipStreamSynchronize(F->stream) == hipSuccess;
  if (F->nranks > 1 && F->comm->agree_ok(ok, F->stream))  // every rank fails together
    return fail(ok ? "get_dft_array: a rank failed" : "get_dft_array: device copy failed");
  if (!ok) return fail("get_dft_array: device copy failed");
  long long ntot = 1;
  for (int k = 0; k < r; k++) ntot *= full[k];
  std::vector<double> arr(2 * ntot, 0.0);
  bool empty_dim[3];
  for (int d = 0; d < 3; d++) empty_dim[d] = S.has[d] && o.wmax[d] - o.wmin[d] == 0.0;
  const int yd[3] = {S.dim == 2 ? 2 : 0, S.dim == 2 ? 0 : 1, S.dim == 2 ? 1 : 2};
  for (auto *dc : L) {
    int n[3];
    for (int k = 0; k < 3; k++) n[k] = S.has[yd[k]] ? (dc->ie[yd[k]] - dc->is[yd[k]]) / 2 + 1 : 1;
    size_t pidx = 0;  // chunk_idx: points in LOOP_OVER_IVECS order
    for (int i1 = 0; i1 < n[0]; i1++)
      for (int i2 = 0; i2 < n[1]; i2++)
        for (int i3 = 0; i3 < n[2]; i3++, pidx++) {
          const size_t pt = dc->p0 + pidx;
          const int *pj = &o.h_pj[3 * pt];
          if (pj[0] < 0 && pj[1] < 0 && pj[2] < 0) continue;  // another rank's point
          const int ii[3] = {i1, i2, i3};
          int p[3] = {0, 0, 0};
          for (int k = 0; k < 3; k++)
            if (S.has[yd[k]]) p[yd[k]] = dc->is[yd[k]] + 2 * ii[k];
          double wl[3], wi[3];
          for (int k = 0; k < 3; k++) {
            const int d = yd[k];
            wl[k] = loop_w1(dc->s0[d], dc->s1[d], dc->e0[d], dc->e1[d], ii[k], n[k]);
            wi[k] = empty_dim[d] ? wl[k] : loop_w1(1.0, 1.0, 1.0, 1.0, ii[k], n[k]);
          }
          const double w = wl[2] * (wl[1] * ((dc->dV0 + 0.0 * i2) * wl[0]));
          const double interp_w = wi[2] * (wi[1] * (1.0 * wi[0]));
          const size_t q = dft_at(o.slot[pt], num_freq, nf);
          cplx dft_val = cplx(v[2 * q], v[2 * q + 1]) / dc->stored;
          if (dc->incl && dft_val != 0.0) dft_val /= w;
          long long oi = 0;
          for (int k = 0; k < r; k++) oi = oi * full[k] + (p[ds[k]] - mn[ds[k]]) / 2;
          const cplx val = interp_w * dft_val;
          arr[2 * oi] = val.real();
          arr[2 * oi + 1] = val.imag();
        }
  }
  if (F->nranks > 1)
    for (size_t q = 0; q < arr.size(); q += 1 << 20) {
      const int n = (int)std::min<size_t>(1 << 20, arr.size() - q);
      if (timed_allreduce(F, arr.data() + q, n)) return fail("get_dft_array allreduce failed");
    }
  for (long long q = 0; q < ntot; q++) {  // collapse_array, in full-index order
    long long t = q, ri = 0;
    for (int k = r - 1; k >= 0; k--) {
      ri += (t % full[k]) * rs[k];
      t /= full[k];
    }
    out[2 * ri] += arr[2 * q];
    out[2 * ri + 1] += arr[2 * q + 1];
  }
  return 0;
}

// ------------------------------------------------------------------ DFT data
// get / load / scale of the accumulated values in list order, replacing
// save_dft_hdf5 / load_dft_hdf5 (src/dft.cpp:444-496) and dft_chunk::scale_dft (401-405).
// a list of the object: flux, fields and near2far objects answer for E and H as before (an
// absent H list is empty), energy objects have 0..3 = E, H, D, B, force objects 0..2 =
// offdiag1, offdiag2, diag
bool dft_bad_which(const DftFluxH &o, int which) {
  return which < 0 || which >= std::max(2, o.nlists);
}
const char *dft_list_name(const DftFluxH &o, int which) {
  static const char *const en[4] = {"E", "H", "D", "B"};
  static const char *const fo[4] = {"offdiag1", "offdiag2", "diag", ""};
  return (o.kind == DFT_FORCE ? fo : en)[which & 3];
}

size_t dft_list_points(const DftFluxH &o, int which) {
  size_t n = 0;
  for (auto &dc : o.L[which]) n += dc.N;
  return n;
}

// the per-slot inverse map of one list (built and uploaded at its first use) and a device
// buffer for the list's values
static int dft_list_ready(mnl_fields *F, DftFluxH &o, int which) {
  const size_t npad = (o.npts + 63) & ~size_t(63);
  if (!o.d_inv[which] && npad) {
    std::vector<int> inv(npad, -1);
    int k = 0;
    for (auto &dc : o.L[which])
      for (size_t p = dc.p0; p < dc.p0 + dc.N; p++, k++)
        if (o.h_pj[3 * p] >= 0) inv[o.slot[p]] = k;
    HIPCHK(hipMalloc(&o.d_inv[which], npad * 4));
    HIPCHK(hipMemcpyAsync(o.d_inv[which], inv.data(), npad * 4, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));  // inv leaves scope
  }
  const size_t need = 2 * dft_list_points(o, which) * (size_t)o.nfreq;
  if (o.list_cap < need) {
    HIPCHK(hipStreamSynchronize(F->stream));
    if (o.d_list) (void)hipFree(o.d_list);
    o.d_list = nullptr, o.list_cap = 0;
    HIPCHK(hipMalloc(&o.d_list, need * 8));
    o.list_cap = need;
  }
  return 0;
}

// one kernel between two events -> kernel_stats 11 (gather), 12 (scatter), 13 (scale)
template <class Fn>
static int dft_io_timed(mnl_fields *F, int id, double bytes, Fn launch) {
  hipEvent_t ev[2] = {nullptr, nullptr};
  auto run = [&]() -> int {
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventRecord(ev[0], F->stream));
    if (launch()) return fail("dft data kernel launch failed");
    HIPCHK(hipEventRecord(ev[1], F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    F->dftio_ms[id] += ms;
    F->dftio_count[id]++;
    F->dftio_bytes[id] = bytes;
    return 0;
  };
  const int r = run();
  for (auto &e : ev)
    if (e) (void)hipEventDestroy(e);
  return r;
}

int dft_get(mnl_fields *F, int h, int which, double *out, long long n) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (dft_bad_which(o, which)) return fail("dft_get: which must be 0 (E) or 1 (H)");
  const size_t nl = dft_list_points(o, which) * (size_t)o.nfreq;  // complex values
  if (n < 0 || (size_t)n < nl) return fail("dft buffer too small");
  if (dft_flush(F, o)) return -1;  // the buffered updates first (same stream)
  for (size_t i = 2 * nl; i < 2 * (size_t)n; i++) out[i] = 0.0;
  if (!nl) return 0;
  if (dft_list_ready(F, o, which)) return -1;
  HIPCHK(hipMemsetAsync(o.d_list, 0, nl * 16, F->stream));  // other ranks' points read 0
  const size_t npad = (o.npts + 63) & ~size_t(63);
  if (dft_io_timed(F, 0, 16.0 * nl + 16.0 * o.nfreq * npad + 4.0 * npad, [&]() {
        return k_dft_gather(o.d_dft, o.d_inv[which], o.d_list, o.nfreq, (long long)npad, F->stream);
      }))
    return -1;
  HIPCHK(hipMemcpyAsync(out, o.d_list, nl * 16, hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

int dft_load(mnl_fields *F, int h, int which, const double *in, long long n, int sign) {
  if (dft_bad_handle(F, h)) return -1;
  if (sign != 1 && sign != -1) return fail("dft_load: sign must be 1 or -1");
  DftFluxH &o = *F->dfts[h];
  if (dft_bad_which(o, which)) return fail("dft_load: which must be 0 (E) or 1 (H)");
  const size_t nl = dft_list_points(o, which) * (size_t)o.nfreq;
  if (n < 0 || (size_t)n != nl) {
    char b[160];  // load_dft_hdf5 (src/dft.cpp:482-484), sizes in doubles as there
    snprintf(b, sizeof b, "incorrect dataset size (%lld vs. %lld) in load_dft %d:%s",
             (long long)(2 * n), (long long)(2 * nl), h, dft_list_name(o, which));
    return fail(b);
  }
  // the updates sampled before the load belong to the values it replaces: accumulate them
  // now (nbuf = 0, no phase row carried over), then overwrite this list
  if (dft_flush(F, o)) return -1;
  if (!nl) return 0;
  if (dft_list_ready(F, o, which)) return -1;
  HIPCHK(hipMemcpyAsync(o.d_list, in, nl * 16, hipMemcpyHostToDevice, F->stream));
  const size_t npad = (o.npts + 63) & ~size_t(63);
  return dft_io_timed(F, 1, 32.0 * nl + 4.0 * npad, [&]() {
    return k_dft_scatter(o.d_dft, o.d_inv[which], o.d_list, (double)sign, o.nfreq,
                         (long long)npad, F->stream);
  });
}

int dft_scale(mnl_fields *F, int h, double re, double im) {
  if (dft_bad_handle(F, h)) return -1;
  DftFluxH &o = *F->dfts[h];
  if (dft_flush(F, o)) return -1;  // everything accumulated so far is scaled
  const size_t nc = ((o.npts + 63) & ~size_t(63)) * (size_t)o.nfreq;
  if (!nc) return 0;
  return dft_io_timed(F, 2, 32.0 * nc, [&]() {
    return k_dft_scale(o.d_dft, re, im, (long long)nc, F->stream);
  });
}

}  // namespace mnlh
