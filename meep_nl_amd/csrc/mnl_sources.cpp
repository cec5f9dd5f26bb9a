// mnl_sources.cpp -- sources and point values: the reference's chunk loops, volume sources and
// their device lists, local indices, and get_field's interpolation.
#include "mnl_host.hpp"

namespace mnlh {

// ------------------------------------------------------------- loop_in_chunks
// One reference chunk's loop of fields::loop_in_chunks over [wmin, wmax] on
// component c's Yee grid (src/loop_in_chunks.cpp:325-520; no symmetry, Bloch
// phase 1): half-coordinate range [isc, iec] and the boundary weights.  Along a
// periodic direction the loop over lattice shifts (390-532) adds the chunks'
// images: shifti is the shift (half-coordinates) from a loop point to the point
// of `where` it stands for.
struct CLoop {
  int isc[3], iec[3], shifti[3];
  int chunk = 0;  // index of the reference chunk
  cplx ph = 1.0;  // the lattice shift's Bloch phase (src/loop_in_chunks.cpp:409-416)
  double s0[3], s1[3], e0[3], e1[3];
  double W(int d, long i) const {  // IVEC_LOOP_WEIGHT1x (src/meep/vec.hpp:372-378)
    const long n = (iec[d] - isc[d]) / 2 + 1;
    if (i > 1 && i < n - 2) return 1.0;
    return i == 0 ? s0[d] : (i == 1 ? s1[d] : i == n - 1 ? e0[d] : (i == n - 2 ? e1[d] : 1.0));
  }
};

static std::vector<CLoop> chunk_loops(const mnl_structure &S, const bool per[3], int c,
                                      const double wmin[3], const double wmax[3],
                                      const cplx *eikna = nullptr) {
  int is[3] = {0, 0, 0}, ie[3] = {0, 0, 0};
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    const int iyc = 1 - S.shift(c, d);    // iyee_shift(Centered) - iyee_shift(c)
    const double yc = iyc * (0.5 / S.a);  // wherec = where + yee_c
    is[d] = 1 + 2 * int(floor((wmin[d] + yc) * S.a - .5)) - iyc;  // vec2diel_floor - iyee_c
    ie[d] = 1 + 2 * int(ceil((wmax[d] + yc) * S.a - .5)) - iyc;
  }
  double s0[3], s1[3], e0[3], e1[3];
  dft_boundary_weights(S, wmin, wmax, is, ie, s0, e0, s1, e1);
  std::vector<CLoop> out;
  LatticeShifts ls(S, per, wmin, wmax);
  do {
  cplx ph = 1.0;
  if (eikna)  // complex fields: ph *= pow(eikna[d], ishift[d]) over the directions
    for (int d = 0; d < 3; d++)
      if (S.has[d]) ph *= pow(eikna[d], ls.cur[d]);
  int nchunk = 0;
  for (auto &ch : reference_chunks(S)) {
    CLoop L;
    L.chunk = nchunk++;
    L.ph = ph;
    bool emp = false;
    for (int d = 0; d < 3; d++) {
      L.s0[d] = L.s1[d] = L.e0[d] = L.e1[d] = 1.0;
      L.shifti[d] = ls.shifti[d];
      if (!S.has[d]) {
        L.isc[d] = L.iec[d] = 0;
        continue;
      }
      // little_owned_corner(c) = little + 2 - iyee_shift(c), big_owned_corner(c) =
      // big - iyee_shift(c) (src/meep/vec.hpp:1102-1107)
      const int sh = S.shift(c, d);
      const int uoc = S.io[d] + 2 - sh, coc = ch[d] + 2 - sh, cbo = ch[d] + 2 * ch[3 + d] - sh;
      const int iscoS = std::max(uoc, std::min(coc, cbo)), iecoS = std::max(coc, cbo);
      L.isc[d] = std::max(is[d] - ls.shifti[d], iscoS);
      L.iec[d] = std::min(ie[d] - ls.shifti[d], iecoS);
      if (L.isc[d] > L.iec[d]) emp = true;
    }
    if (emp) continue;
    for (int d = 0; d < 3; d++) {
      if (!S.has[d]) continue;
      const int iscS = L.isc[d] + ls.shifti[d], iecS = L.iec[d] + ls.shifti[d];
      if (iscS == is[d]) {
        L.s0[d] = s0[d];
        L.s1[d] = s1[d];
      } else if (iscS == is[d] + 2) {
        L.s0[d] = s1[d];
      }
      if (iecS == ie[d]) {
        L.e0[d] = e0[d];
        L.e1[d] = e1[d];
      } else if (iecS == ie[d] - 2) {
        L.e0[d] = e1[d];
      }
      if (L.iec[d] == L.isc[d]) {
        double w = std::min(L.s0[d], L.e0[d]);
        L.s0[d] = L.e0[d] = L.s1[d] = L.e1[d] = w;
      } else if (L.iec[d] == L.isc[d] + 2) {
        double w = std::min(L.s0[d], L.e1[d]);
        L.s0[d] = w, L.e1[d] = w;
        w = std::min(L.s1[d], L.e0[d]);
        L.s1[d] = w, L.e0[d] = w;
      } else if (L.iec[d] == L.isc[d] + 4) {
        double w = std::min(L.s1[d], L.e1[d]);
        L.s1[d] = w, L.e1[d] = w;
      }
    }
    out.push_back(L);
  }
  } while (ls.next());
  return out;
}

// ------------------------------------------------------------- sources
// fields::add_volume_source(c, src, where, A, amp) (src/sources.cpp:455-494):
// the source volume is clamped to the cell, delta-function directions scale
// the amplitude by a, and src_vol_chunkloop (243-312) gives every owned point
// of each reference chunk the amplitude IVEC_LOOP_WEIGHT * amp * A(loc -
// center).  The points of all chunks form one group (src_vol list order).
static int add_volume_source(mnl_fields *F, int c, int st, const double wmin0[3],
                             const double wmax0[3], cplx amp0, mnl_amp_func afunc, void *adata) {
  const mnl_structure &S = F->S;
  double wmin[3], wmax[3];
  for (int d = 0; d < 3; d++) {
    wmin[d] = S.has[d] ? wmin0[d] : 0.0;
    wmax[d] = S.has[d] ? wmax0[d] : 0.0;
    if (wmax[d] < wmin[d]) return fail("source volume: max < min");
    if (!S.has[d]) continue;
    const double w = S.n[d] * (1.0 / S.a);  // user_volume width
    const double wd = wmax[d] - wmin[d];
    if (wd > w + 1.0 / S.a) {
      const char *nm[3] = {"X", "Y", "Z"};
      return fail(std::string("Source width > cell width in ") + nm[d] + " direction!");
    } else if (wd > w) {  // less than a pixel too wide
      const double dw = wd - w;
      wmin[d] = wmin[d] - dw * 0.5;
      wmax[d] = wmin[d] + w;
    }
  }
  cplx amp = amp0;
  for (int d = 0; d < 3; d++)
    if (S.has[d] && wmax[d] - wmin[d] == 0.0) amp *= S.a;  // delta-function units
  double center[3];
  for (int d = 0; d < 3; d++) center[d] = (wmin[d] + wmax[d]) * 0.5;
  int yd[3];
  if (S.dim == 2)
    yd[0] = 2, yd[1] = 0, yd[2] = 1;
  else
    yd[0] = 0, yd[1] = 1, yd[2] = 2;
  SrcGroup grp;
  grp.comp = c;
  grp.st = st;
  for (const CLoop &L : chunk_loops(S, F->periodic, c, wmin, wmax,
                                    is_complex(F) ? (F->part0 ? F->part0 : F)->eikna : nullptr)) {
    long ln[3];
    for (int k = 0; k < 3; k++) ln[k] = S.has[yd[k]] ? (L.iec[yd[k]] - L.isc[yd[k]]) / 2 + 1 : 1;
    for (long i1 = 0; i1 < ln[0]; i1++)
      for (long i2 = 0; i2 < ln[1]; i2++)
        for (long i3 = 0; i3 < ln[2]; i3++) {
          const long ii[3] = {i1, i2, i3};
          int p[3] = {0, 0, 0};
          for (int k = 0; k < 3; k++)
            if (S.has[yd[k]]) p[yd[k]] = L.isc[yd[k]] + 2 * int(ii[k]);
          bool own = true;
          int jg[3] = {0, 0, 0};
          long long gi = 0;
          for (int d = 0; d < 3; d++)
            if (S.has[d]) {
              const int o = p[d] - S.io[d];
              if (!(o > 0 && o <= 2 * S.n[d])) own = false;
              jg[d] = (p[d] - S.io[d] - S.shift(c, d)) / 2;
              gi += jg[d] * S.cstride(d);
            }
          if (!own) continue;
          double w[3];
          for (int k = 0; k < 3; k++) w[k] = L.W(yd[k], ii[k]);
          const double wgt = w[2] * (w[1] * (1.0 * w[0]));
          cplx A = 1.0;
          if (afunc) {
            double rel[3];
            for (int d = 0; d < 3; d++)  // loc += shift (src/sources.cpp:270)
              rel[d] = S.has[d] ? (p[d] + L.shifti[d]) * (0.5 * (1.0 / S.a)) - center[d] : 0.0;
            double re = 0, im = 0;
            afunc(rel, adata, &re, &im);
            A = cplx(re, im);
          }
          grp.amp.push_back(wgt * (amp * std::conj(L.ph)) * A);  // src/sources.cpp:259
          grp.gidx.push_back(gi);
          grp.chunk.push_back(L.chunk);
          for (int d = 0; d < 3; d++) grp.jglob.push_back(jg[d]);
        }
  }
  if (grp.gidx.empty()) return 0;
  for (auto &o : F->groups)  // src_vol::combinable merge (src/fields.cpp:588-597)
    if (o.comp == grp.comp && o.st == grp.st && o.gidx == grp.gidx) {
      for (size_t i = 0; i < o.amp.size(); i++) o.amp[i] += grp.amp[i];
      F->src_dirty = true;
      return 0;
    }
  F->groups.push_back(std::move(grp));
  F->src_dirty = true;
  return 0;
}

// local linear index of a global point of component c, or -1 if not owned by this rank
long long local_index(const mnl_fields *F, int c, const int jg[3], bool include_wall) {
  const DevGrid &g = F->g;
  long long li = 0;
  for (int d = 0; d < 3; d++) {
    if (g.ax[d] < 0) continue;
    int j = jg[d] - g.off[d];
    int sh = F->S.shift(c, d);
    int lo = sh ? g.owned_lo_sh[d] : g.owned_lo_un[d];
    int hi = sh ? g.owned_hi_sh[d] : g.owned_hi_un[d];
    if (include_wall && !sh && jg[d] == g.nglob[d] && j >= 0 && j < g.N[g.ax[d]]) hi = j;
    if (j < lo || j > hi) return -1;
    li += (long long)j * g.st[g.ax[d]];
  }
  return li;
}

// local linear index of a global point anywhere in this rank's arrays (ghost
// planes included), or -1
static long long local_index_ghost(const mnl_fields *F, const int jg[3]) {
  const DevGrid &g = F->g;
  long long li = 0;
  for (int d = 0; d < 3; d++) {
    if (g.ax[d] < 0) continue;
    int j = jg[d] - g.off[d];
    if (j < 0 || j >= g.N[g.ax[d]]) return -1;
    li += (long long)j * g.st[g.ax[d]];
  }
  return li;
}

int build_source_lists(mnl_fields *F) {
  // whole-cell facts (the same on every rank): what keeps the step unfused
  F->any_srcB = F->any_isrc = F->any_dsrc_w = false;
  for (const SrcGroup &G : F->groups) {
    const bool mag = ctype(G.comp) == T_H, integ = F->srcs[G.st].is_integrated;
    if (mag && !integ) F->any_srcB = true;
    if (!mag && integ) F->any_isrc = true;
    if (!mag && !integ) {
      const int d = cdir(G.comp);
      if (F->S.has[d] && F->pml_any[d])
        for (size_t j = 0; j < G.gidx.size(); j++)
          if (F->h_flag[d][2 * G.jglob[3 * j + d] + 1]) F->any_dsrc_w = true;
    }
  }
  F->srcB_idx.clear(), F->srcD_idx.clear(), F->isrc_idx.clear();
  F->srcB_comp.clear(), F->srcD_comp.clear(), F->isrc_comp.clear();
  F->srcB_ref.clear(), F->srcD_ref.clear(), F->isrc_ref.clear();
  F->isrc_zone.clear();
  for (size_t gi = 0; gi < F->groups.size(); gi++) {
    const SrcGroup &G = F->groups[gi];
    const SrcTime &st = F->srcs[G.st];
    int c = G.comp;
    bool mag = ctype(c) == T_H;
    for (size_t j = 0; j < G.gidx.size(); j++) {
      const int *jg = &G.jglob[3 * j];
      int tgt = mag ? 3 * T_B + cdir(c) : 3 * T_D + cdir(c);
      long long li = local_index(F, tgt, jg, false);
      if (st.is_integrated && !mag) {
        // integrated dipoles are read (never written): keep the rank's ghost copies
        // too, so a slab seam sees what one GPU sees; the zone box restricts the
        // subtraction to readers in the owning reference chunk.  A dipole on the
        // high metallic wall plane stays: the chunk owns that point and its
        // f_minus_p there (D = 0 minus the dipole) is read by neighbours through
        // the Newton-Raphson / OFFDIAG sums (src/update_eh.cpp:136-146).
        li = local_index(F, tgt, jg, true);
        if (li < 0 && F->nranks > 1) {
          bool wall = false;  // high PEC wall of an unshifted direction: nobody owns it
          for (int d = 0; d < 3; d++)
            if (F->g.ax[d] >= 0 && !F->S.shift(tgt, d) && jg[d] == F->g.nglob[d]) wall = true;
          if (!wall) li = local_index_ghost(F, jg);
        }
        if (li < 0) continue;
        int zb = 0;
        for (int d = 0; d < 3; d++) {
          int z = 1;
          if (F->S.has[d]) z = F->h_zone[d][2 * jg[d] + F->S.shift(tgt, d)];
          zb = zb * 3 + z;
        }
        F->isrc_idx.push_back(li);
        F->isrc_comp.push_back(cdir(c));
        F->isrc_zone.push_back((unsigned char)zb);
        F->isrc_ref.push_back({(int)gi, (int)j});
        continue;
      }
      if (li < 0) continue;
      if (!st.is_integrated) {
        auto &I = mag ? F->srcB_idx : F->srcD_idx;
        auto &C = mag ? F->srcB_comp : F->srcD_comp;
        auto &R = mag ? F->srcB_ref : F->srcD_ref;
        I.push_back(li);
        C.push_back(cdir(c));
        R.push_back({(int)gi, (int)j});
      }
    }
  }
  // integrated dipoles for the E kernels: sorted by local index (stable, so the
  // entries of one point keep list order), with their position in the table
  F->isrc_dev = ISrcDev{};
  if (!F->isrc_idx.empty()) {
    const size_t n = F->isrc_idx.size();
    std::vector<int> ord(n);
    for (size_t k = 0; k < n; k++) ord[k] = (int)k;
    std::stable_sort(ord.begin(), ord.end(),
                     [&](int a, int b) { return F->isrc_idx[a] < F->isrc_idx[b]; });
    std::vector<long long> si(n);
    std::vector<int> sc(n), so(n);
    std::vector<unsigned char> sz(n);
    for (size_t k = 0; k < n; k++)
      si[k] = F->isrc_idx[ord[k]], sc[k] = F->isrc_comp[ord[k]], sz[k] = F->isrc_zone[ord[k]],
      so[k] = ord[k];
    long long *di;
    int *dc, *dor;
    unsigned char *dz;
    if (dev_alloc(F, &di, n, false) || dev_alloc(F, &dc, n, false) || dev_alloc(F, &dor, n, false) ||
        dev_alloc(F, &dz, n, false))
      return -1;
    HIPCHK(hipMemcpyAsync(di, si.data(), n * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(dc, sc.data(), n * 4, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(dor, so.data(), n * 4, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(dz, sz.data(), n, hipMemcpyHostToDevice, F->stream));
    F->isrc_dev.n = (int)n;
    F->isrc_dev.idx = di, F->isrc_dev.comp = dc, F->isrc_dev.orig = dor, F->isrc_dev.zone = dz;
    F->isrc_dev.imin = si.front(), F->isrc_dev.imax = si.back();
  }
  // layers: the k-th occurrence of a (component, point) goes to layer k, so a layer
  // is applied in parallel and the layers in list order (step_source order)
  for (int t = 0; t < 2; t++) {
    auto &I = t ? F->srcD_idx : F->srcB_idx;
    auto &C = t ? F->srcD_comp : F->srcB_comp;
    auto &R = t ? F->srcD_ref : F->srcB_ref;
    std::unordered_map<long long, int> seen;
    std::vector<int> lay(I.size());
    int nl = 0;
    for (size_t k = 0; k < I.size(); k++) {
      lay[k] = seen[I[k] * 3 + C[k]]++;
      nl = std::max(nl, lay[k] + 1);
    }
    std::vector<size_t> ord(I.size());
    for (size_t k = 0; k < ord.size(); k++) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return lay[a] < lay[b]; });
    std::vector<long long> I2;
    std::vector<int> C2;
    std::vector<std::pair<int, int>> R2;
    auto &A = F->src_amp[t];
    auto &Gd = F->src_gid[t];
    auto &L = F->src_layer[t];
    A.clear(), Gd.clear(), L.assign(nl + 1, 0);
    for (size_t k : ord) {
      I2.push_back(I[k]);
      C2.push_back(C[k]);
      R2.push_back(R[k]);
      cplx a = F->groups[R[k].first].amp[R[k].second];
      // part 1 of complex fields adds imag(a J) where part 0 adds real(a J) (src/step.cpp:
      // 300-315): the kernel's real((a_i, -a_r) J) = a_i J_r + a_r J_i
      if (F->part0) a = cplx(imag(a), -real(a));
      A.push_back(real(a));
      A.push_back(imag(a));
      Gd.push_back(R[k].first);
      L[lay[k] + 1]++;
    }
    for (int l = 0; l < nl; l++) L[l + 1] += L[l];
    I.swap(I2), C.swap(C2), R.swap(R2);
    if (I.empty()) continue;
    long long **dI = t ? &F->d_srcD_idx : &F->d_srcB_idx;
    int **dC = t ? &F->d_srcD_comp : &F->d_srcB_comp;
    if (dev_alloc(F, dI, I.size(), false) || dev_alloc(F, dC, C.size(), false) ||
        dev_alloc(F, &F->d_src_amp[t], A.size(), false) ||
        dev_alloc(F, &F->d_src_gid[t], Gd.size(), false))
      return -1;
    HIPCHK(hipMemcpyAsync(*dI, I.data(), I.size() * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(*dC, C.data(), C.size() * 4, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(F->d_src_amp[t], A.data(), A.size() * 8, hipMemcpyHostToDevice,
                          F->stream));
    HIPCHK(hipMemcpyAsync(F->d_src_gid[t], Gd.data(), Gd.size() * 4, hipMemcpyHostToDevice,
                          F->stream));
  }
  HIPCHK(hipStreamSynchronize(F->stream));
  F->src_dirty = false;
  // LDOS objects follow the sources: buffered rows flushed with the old lists, then new lists
  return F->ldoses.empty() ? 0 : ldos_sources_rebuilt(F);
}

// SrcDev of field type t (0 = B, 1 = D) reading the group currents at J
SrcDev src_dev(mnl_fields *F, int t, const double *J) {
  SrcDev s;
  s.n = (int)(t ? F->srcD_idx.size() : F->srcB_idx.size());
  s.idx = t ? F->d_srcD_idx : F->d_srcB_idx;
  s.comp = t ? F->d_srcD_comp : F->d_srcB_comp;
  s.amp = F->d_src_amp[t];
  s.gid = F->d_src_gid[t];
  s.J = J;
  s.dt = F->dt;
  s.nlayer = (int)F->src_layer[t].size() - 1;
  s.layer = F->src_layer[t].data();
  if (s.nlayer < 0) s.nlayer = 0;
  return s;
}

// (the interpolation helpers and the DFT monitors: mnl_dft.cpp)
void interpolate(const mnl_structure &S, int c, const double pc[3], int locs[8][3], double w[8]) {
  const double SMALL = 1e-13;
  double p[3] = {0, 0, 0}, midv[3] = {0, 0, 0}, dv[3] = {0, 0, 0};
  int middle[3] = {0, 0, 0};
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    double ys = S.shift(c, d) * (0.5 * (1.0 / S.a));
    p[d] = (pc[d] - ys) * S.a;
    middle[d] = ((int)floor(p[d])) * 2 + 1 + S.shift(c, d);
    midv[d] = middle[d] * (0.5 * (1.0 / S.a));
    dv[d] = (pc[d] - midv[d]) * (2 * S.a);
  }
  int already = 1;
  for (int i = 0; i < 8; i++) {
    for (int d = 0; d < 3; d++) locs[i][d] = S.has[d] ? my_round(midv[d] * 2 * S.a) : 0;
    w[i] = 1.0;
  }
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    for (int i = 0; i < already; i++) {
      for (int e = 0; e < 3; e++) locs[already + i][e] = locs[i][e];
      w[already + i] = w[i];
      locs[i][d] = middle[d] - 1;
      w[i] *= 0.5 * (1.0 - dv[d]);
      locs[already + i][d] = middle[d] + 1;
      w[already + i] *= 0.5 * (1.0 + dv[d]);
    }
    already *= 2;
  }
  for (int i = already; i < 8; i++) w[i] = 0.0;
  double total = 0.0;
  for (int i = 0; i < already; i++) total += w[i];
  for (int i = 0; i < already; i++) w[i] += (1.0 - total) * (1.0 / already);
  for (int i = 0; i < already; i++) {
    if (w[i] < 0.0 || w[i] < SMALL) w[i] = 0.0;
  }
  int l = already, off = 0;
  while (l) {
    if (fabs(w[off]) < 2e-15) {
      w[off] = w[off + l - 1];
      for (int e = 0; e < 3; e++) locs[off][e] = locs[off + l - 1][e];
      w[off + l - 1] = 0.0;
      for (int e = 0; e < 3; e++) locs[off + l - 1][e] = 0;
    } else
      off += 1;
    l -= 1;
  }
  bool all_same = true;
  for (int i = 0; i < 8 && w[i]; i++)
    if (w[i] != w[0]) all_same = false;
  if (all_same) {
    int nw = 0;
    for (int i = 0; i < 8 && w[i]; i++) nw++;
    for (int i = 0; i < 8 && w[i]; i++) w[i] = 1.0 / nw;
  }
}

// value of component c at absolute half-coords p (0 if not owned by this rank)
static int value_at(mnl_fields *F, int c, const int p[3], double *out) {
  const mnl_structure &S = F->S;
  *out = 0.0;
  int jg[3] = {0, 0, 0};
  for (int d = 0; d < 3; d++)
    if (S.has[d]) {
      int o = p[d] - S.io[d];
      if (!(o > 0 && o <= 2 * S.n[d])) return 0;  // not owned by the cell
      jg[d] = (p[d] - S.io[d] - S.shift(c, d)) / 2;
    }
  if (!F->allocated[c]) return 0;
  long long li = local_index(F, c, jg, true);
  if (li < 0) return 0;
  int t = ctype(c), d = cdir(c);
  const double *src = nullptr;
  switch (t) {
    case T_E: src = F->f.E[d]; break;
    case T_D: src = F->f.D[d]; break;
    case T_B: src = F->f.B[d]; break;
    case T_H: {
      src = F->f.B[d];
      if (F->hall) {  // H stored everywhere once the first H update has run
        if (F->h_first_done) src = F->f.H[d];
      } else if (F->f.H[d] && S.has[d]) {
        int q = 2 * jg[d];
        if (F->h_flag[d][q]) src = F->f.H[d];
      }
      break;
    }
  }
  if (!src) return 0;
  HIPCHK(hipStreamSynchronize(F->stream));
  if (in_fused_box(F, c, jg)) {  // E = chi1inv * D inside the fused region
    double dv = 0, uv = 1;
    HIPCHK(hipMemcpy(&dv, F->f.D[d] + li, sizeof(double), hipMemcpyDeviceToHost));
    if (F->f.inveps[d]) {
      HIPCHK(hipMemcpy(&uv, F->f.inveps[d] + li, sizeof(double), hipMemcpyDeviceToHost));
      *out = dv * uv;
    } else {
      *out = dv;
    }
    return 0;
  }
  HIPCHK(hipMemcpy(out, src + li, sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int get_field(mnl_fields *F, int c, const double pos[3], double *out, bool reduce) {
  int locs[8][3];
  double w[8];
  double pp[3] = {pos[0], pos[1], pos[2]};
  if (F->S.dim == 1) pp[0] = pp[1] = 0;
  if (F->S.dim == 2) pp[2] = 0;
  interpolate(F->S, c, pp, locs, w);
  cplx res = 0.0;
  bool ok = true;
  for (int i = 0; i < 8 && w[i] && ok; i++) {
    double v;
    if (value_at(F, c, locs[i], &v)) ok = false;
    else res += w[i] * cplx(v);
  }
  double r = real(res);
  if (reduce && F->nranks > 1) {
    const std::string why = g_err;
    if (F->comm->agree_ok(ok, F->stream)) return fail(ok ? "get_field: a rank failed" : why);
    if (timed_allreduce(F, &r, 1)) return fail("allreduce failed");
  }
  if (!ok) return -1;
  *out = r;
  return 0;
}

int add_source_any(mnl_fields *F, int comp, int kind, const double *p, int np, mnl_src_func func,
                   void *fdata, const double vmin[3], const double vmax[3], double amp_re,
                   double amp_im, int is_integrated, mnl_amp_func afunc, void *adata) {
  if (!F || check_comp(comp)) return -1;
  if (!(ctype(comp) == T_E || ctype(comp) == T_H)) return fail("sources must be E or H components");
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  SrcTime st;
  if (kind == MNL_SRC_GAUSSIAN) {
    if (np < 4) return fail("gaussian source needs 4 parameters");
    // gaussian_src_time(f, w, st, et) (src/sources.cpp:85-96)
    st.kind = 0;
    st.freq = p[0];
    st.width = p[1];
    st.peak_time = 0.5 * (p[2] + p[3]);
    st.cutoff = (p[3] - p[2]) * 0.5;
    while (exp(-st.cutoff * st.cutoff / (2 * st.width * st.width)) < 1e-100) st.cutoff *= 0.9;
    st.cutoff = float(st.cutoff);
  } else if (kind == MNL_SRC_CONTINUOUS) {
    if (np < 6) return fail("continuous source needs 6 parameters");
    st.kind = 1;
    st.cfreq = cplx(p[0], p[1]);
    st.cwidth = p[2];
    st.start_time = float(p[3]);
    st.end_time = float(p[4]);
    st.slowness = p[5];
  } else if (kind == MNL_SRC_CUSTOM) {  // custom_src_time(func, data, st, et)
    st.kind = 2;
    st.func = func;
    st.fdata = fdata;
    st.start_time = float(p[0]);
    st.end_time = float(p[1]);
  } else
    return fail("unknown source kind");
  st.is_integrated = is_integrated != 0;
  int idx = -1;
  for (size_t i = 0; i < F->srcs.size(); i++)
    if (F->srcs[i].same(st)) idx = (int)i;
  if (idx < 0) {
    if (F->srcs.empty()) F->src0_born = F->t;
    F->srcs.push_back(st);
    idx = (int)F->srcs.size() - 1;
  }
  if (require_component(F, comp)) return -1;
  double lo[3] = {vmin[0], vmin[1], vmin[2]}, hi[3] = {vmax[0], vmax[1], vmax[2]};
  if (F->S.dim == 1) lo[0] = lo[1] = hi[0] = hi[1] = 0;
  if (F->S.dim == 2) lo[2] = hi[2] = 0;
  return add_volume_source(F, comp, idx, lo, hi, cplx(amp_re, amp_im), afunc, adata);
}

}  // namespace mnlh
