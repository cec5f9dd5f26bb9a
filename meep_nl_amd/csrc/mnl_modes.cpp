// mnl_modes.cpp -- mode coefficients of diffraction orders: fields::get_eigenmode_coefficients
// with a DiffractedPlanewave (src/mpb.cpp:925-1004).  The mode is the
// analytic plane wave of mnl_modes.hpp; the overlap sums of fields::get_overlap
// (src/dft.cpp:1377-1437) over the flux object's DFT array stay on the device
// (k_mode_overlap, k_n2f_reduce), summed over the ranks like dft_flux_values; the coefficients
// are formed on the host.
#include "mnl_host.hpp"
#include "mnl_modes.hpp"

namespace mnlh {

// the components of fields::get_overlap's four sums (src/dft.cpp:1380-1412): sum j runs over the
// chunks of comp[j] and conjugates the mode's conj[j]
static void mode_sum_components(int nd, int comp[4], int conj[4]) {
  const int e0 = (nd + 1) % 3, e1 = (nd + 2) % 3;  // X: Ey Ez; Y: Ez Ex; Z: Ex Ey
  const int cE[2] = {MNL_EX + e0, MNL_EX + e1}, cH[2] = {MNL_HX + e1, MNL_HX + e0};
  comp[0] = cE[0], conj[0] = cH[0];
  comp[1] = cE[1], conj[1] = cH[1];
  comp[2] = cH[0], conj[2] = cE[0];
  comp[3] = cH[1], conj[3] = cE[1];
}

static DftFluxH *mode_object(mnl_fields *F, int h, int nmodes) {
  if (h >= LDOS_BASE || h < 0 || h >= (int)F->dfts.size() || F->dfts[h]->kind != DFT_FLUX ||
      F->dfts[h]->nreg < 1) {
    fail("mode_coefficients: the handle is not a flux object");
    return nullptr;
  }
  DftFluxH &o = *F->dfts[h];
  if (o.nreg != 1) {
    fail("mode_coefficients: a flux object with several regions is not supported (one region "
         "per mode monitor)");
    return nullptr;
  }
  if (F->S.dim == 1) {
    fail("mode_coefficients: 1-D cells are not supported");
    return nullptr;
  }
  if (nmodes < 1) {
    fail("mode_coefficients: no modes (nmodes < 1)");
    return nullptr;
  }
  if (o.normal < 0 || o.normal > 2 || !F->S.has[o.normal]) {
    fail("mode_coefficients: the flux region has no normal direction in this cell");
    return nullptr;
  }
  return &o;
}

// the per-slot index arrays and the workgroups' slot ranges, once per object
static int mode_index_build(mnl_fields *F, DftFluxH &o) {
  DftFluxH::ModeIdx &M = o.mo;
  if (M.built) return 0;
  const mnl_structure &S = F->S;
  const int nd = o.normal;
  M.da = M.db = -1;
  for (int d = 0; d < 3; d++)
    if (d != nd && S.has[d]) (M.da < 0 ? M.da : M.db) = d;
  if (M.da < 0) M.da = (nd + 1) % 3;  // (not reached: 1-D cells are refused)
  int comp[4], conj[4];
  mode_sum_components(nd, comp, conj);
  const int yd[3] = {S.dim == 2 ? 2 : 0, S.dim == 2 ? 0 : 1, S.dim == 2 ? 1 : 2};
  // pass 1: the distinct coordinates (image chunks' shifted ones included)
  std::vector<int> ca, cb, cl;
  for (int l = 0; l < 2; l++)
    for (auto &dc : o.L[l])
      for (int d = 0; d < 3; d++) {
        if (!S.has[d]) continue;
        std::vector<int> &v = d == nd ? cl : (d == M.da ? ca : cb);
        for (int c = dc.is[d]; c <= dc.ie[d]; c += 2) v.push_back(c + dc.shifti[d]);
      }
  for (auto *v : {&ca, &cb, &cl}) {
    std::sort(v->begin(), v->end());
    v->erase(std::unique(v->begin(), v->end()), v->end());
  }
  if (cl.size() > 2) return fail("mode_coefficients: the flux plane has more than two layers");
  M.ca = ca, M.cb = cb;
  M.nlayer = std::max<int>(1, (int)cl.size());
  for (size_t i = 0; i < cl.size(); i++) M.layer[i] = cl[i];
  if (M.ca.empty()) M.ca.push_back(0);
  if (M.db < 0 || M.cb.empty()) M.cb.assign(1, 0);
  auto index_of = [](const std::vector<int> &v, int c) {
    return (int)(std::lower_bound(v.begin(), v.end(), c) - v.begin());
  };
  // pass 2: per slot the table indices, the layer, the weights; which sum it adds to
  const size_t npts = o.npts;
  M.nslots = (long long)npts;
  if (npts >= (size_t(1) << 31)) return fail("mode_coefficients: too many DFT points");
  std::vector<ModeSlot> ms(npts, ModeSlot{0, 0, 0, 0});
  std::vector<double> wv(2 * npts, 1.0);
  std::vector<int> sj(npts, -1);  // -1: another rank's slot, or of no sum
  for (int l = 0; l < 2; l++)
    for (auto &dc : o.L[l]) {
      int j = -1;
      for (int q = 0; q < 4; q++)
        if (comp[q] == dc.c) j = q;
      int n[3];
      for (int q = 0; q < 3; q++) n[q] = S.has[yd[q]] ? (dc.ie[yd[q]] - dc.is[yd[q]]) / 2 + 1 : 1;
      size_t pidx = 0;
      for (int i1 = 0; i1 < n[0]; i1++)
        for (int i2 = 0; i2 < n[1]; i2++)
          for (int i3 = 0; i3 < n[2]; i3++, pidx++) {
            const size_t pt = dc.p0 + pidx;
            const size_t t = (size_t)o.slot[pt];
            const int ii[3] = {i1, i2, i3};
            double wl[3];
            int c[3] = {0, 0, 0};
            for (int q = 0; q < 3; q++) {
              const int d = yd[q];
              wl[q] = loop_w1(dc.s0[d], dc.s1[d], dc.e0[d], dc.e1[d], ii[q], n[q]);
              if (S.has[d]) c[d] = dc.is[d] + dc.shifti[d] + 2 * ii[q];
            }
            // IVEC_LOOP_WEIGHT(s0, s1, e0, e1, dV0 + dV1 * loop_i2) (src/dft.cpp:980)
            const double w = wl[2] * (wl[1] * ((dc.dV0 + 0.0 * i2) * wl[0]));
            ModeSlot &m = ms[t];
            m.ia = index_of(M.ca, c[M.da]);
            m.ib = M.db >= 0 ? index_of(M.cb, c[M.db]) : 0;
            m.layer = (M.nlayer > 1 && c[nd] == M.layer[1] ? 1 : 0) | (dc.incl ? 2 : 0);
            wv[2 * t] = w;
            wv[2 * t + 1] = real(dc.stored);  // (the stored weights of a flux object are real)
            if (o.h_pj[3 * pt] >= 0) sj[t] = j;
          }
    }
  // the ranges: this rank's slots of sum j are consecutive (dft_layout sorts by component); each
  // run is cut into ranges of a size that depends on its length alone
  std::vector<ModeRange> rng;
  for (int j = 0; j < 4; j++) {
    M.wg0[j] = (int)rng.size();
    size_t lo = npts, hi = 0, cnt = 0;
    for (size_t t = 0; t < npts; t++)
      if (sj[t] == j) lo = std::min(lo, t), hi = std::max(hi, t + 1), cnt++;
    if (!cnt) continue;
    if (hi - lo != cnt) return fail("mode_coefficients: the slots of one component are not consecutive");
    const long long per0 = std::max<long long>(MO_WG_SLOTS, ((long long)cnt + MO_MAX_WG - 1) / MO_MAX_WG);
    const long long per = (per0 + 63) / 64 * 64;
    for (long long s = (long long)lo; s < (long long)hi; s += per)
      rng.push_back(ModeRange{(int)s, (int)std::min<long long>(s + per, (long long)hi), j, 0});
  }
  M.wg0[4] = M.nwg = (int)rng.size();
  if (npts) {
    HIPCHK(hipMalloc(&M.d_slot, npts * sizeof(ModeSlot)));
    HIPCHK(hipMalloc(&M.d_wv, npts * 16));
    HIPCHK(hipMemcpyAsync(M.d_slot, ms.data(), npts * sizeof(ModeSlot), hipMemcpyHostToDevice,
                          F->stream));
    HIPCHK(hipMemcpyAsync(M.d_wv, wv.data(), npts * 16, hipMemcpyHostToDevice, F->stream));
    if (!rng.empty()) {
      HIPCHK(hipMalloc(&M.d_rng, rng.size() * sizeof(ModeRange)));
      HIPCHK(hipMemcpyAsync(M.d_rng, rng.data(), rng.size() * sizeof(ModeRange),
                            hipMemcpyHostToDevice, F->stream));
    }
    HIPCHK(hipStreamSynchronize(F->stream));  // the host vectors leave scope
  }
  M.built = true;
  return 0;
}

// does the medium at pos carry a susceptibility or a conductivity (at the points get_eps /
// get_mu interpolate from)?
static bool mode_medium_dispersive(const mnl_structure &S, const double pos[3]) {
  for (int t : {T_E, T_H})
    for (int k = 0; k < 3; k++) {
      const int c = (t == T_E ? MNL_EX : MNL_HX) + k;
      if (!has_field(S, c)) continue;
      int locs[8][3];
      double w[8];
      interpolate(S, c, pos, locs, w);
      for (int i = 0; i < 8 && w[i]; i++) {
        long long idx = 0;
        bool in = true;
        for (int d = 0; d < 3; d++) {
          if (!S.has[d]) continue;
          const int hh = locs[i][d] - S.io[d] - S.shift(c, d);
          if (hh < 0 || hh / 2 > S.n[d]) in = false;
          idx += (long long)(hh / 2) * S.cstride(d);
        }
        if (!in) continue;
        const auto &cond = S.cond[t == T_E ? 1 : 0][k];
        if (!cond.empty() && cond[idx] != 0.0) return true;
        for (const Lorentz &L : (t == T_E ? S.lor : S.hlor)) {
          if (!L.sigma[k].empty() && L.sigma[k][idx] != 0.0) return true;
          for (int d = 0; d < 3; d++)
            if (!L.off[k][d].empty() && L.off[k][d][idx] != 0.0) return true;
        }
      }
    }
  return false;
}

// the geometry of one call and its table
static int mode_build_table(mnl_fields *F, DftFluxH &o, const ModeCall &c, mnlmodes::Geometry &G,
                            mnlmodes::Table &T) {
  const mnl_structure &S = F->S;
  const DftFluxH::ModeIdx &M = o.mo;
  // src/mpb.cpp:352-354, 630-635: the out-of-plane k_z of a 2-D cell (fields::use_bloch refuses
  // a direction the cell lacks, so it is always 0 here) and of a 3-D cell one pixel thick
  if (S.dim == 3 && S.n[2] == 1 && F->periodic[2] && real(F->bloch_k[2]) != 0.0)
    return fail("mode_coefficients: a 3-D cell one pixel thick along z with a Bloch k_z (the "
                "reference's special case of a 2-D cell with k_z) is not supported");
  for (int d = 0; d < 3; d++) {
    G.has[d] = S.has[d];
    G.ncell[d] = S.has[d] ? S.n[d] : 1;
    G.periodic[d] = F->periodic[d];
    G.bloch[d] = real(F->bloch_k[d]);
    G.emin[d] = c.eig_vol ? c.eig_vol[d] : o.wmin[d];
    G.emax[d] = c.eig_vol ? c.eig_vol[3 + d] : o.wmax[d];
    G.kpoint[d] = c.kpoint ? c.kpoint[d] : 0.0;
    if (!S.has[d]) G.emin[d] = G.emax[d] = 0.0;
  }
  G.a = S.a;
  G.normal = o.normal;
  const double cen[3] = {0.5 * (G.emin[0] + G.emax[0]), 0.5 * (G.emin[1] + G.emax[1]),
                         0.5 * (G.emin[2] + G.emax[2])};
  if (mode_medium_dispersive(S, cen))
    return fail("mode_coefficients: the medium at the centre of the eigenmode volume has a "
                "susceptibility or a conductivity; the frequency-dependent epsilon / mu a "
                "DiffractedPlanewave needs there is not available in this build");
  G.eps = n2f_medium_at(S, T_E, cen), G.mu = n2f_medium_at(S, T_H, cen);
  G.da = M.da, G.db = M.db, G.ca = M.ca, G.cb = M.cb;
  G.nlayer = M.nlayer, G.layer[0] = M.layer[0], G.layer[1] = M.layer[1];
  std::vector<mnlmodes::Mode> modes(c.nmodes);
  for (int m = 0; m < c.nmodes; m++) {
    for (int d = 0; d < 3; d++) {
      modes[m].g[d] = c.g[3 * m + d];
      modes[m].axis[d] = c.axis ? c.axis[3 * m + d] : 0.0;
    }
    modes[m].s = cplx(c.sp[4 * m], c.sp[4 * m + 1]);
    modes[m].p = cplx(c.sp[4 * m + 2], c.sp[4 * m + 3]);
  }
  std::vector<double> freqs(o.nfreq);
  for (int i = 0; i < o.nfreq; i++) freqs[i] = o.omega[i] / (2 * pi);
  std::string err;
  if (mnlmodes::build(G, modes, freqs, T, err)) return fail(err);
  return 0;
}

int mode_table(mnl_fields *F, const ModeCall &c, long long dims[4], int *coords, double *k,
               double *vgrp, double *amp, double *pa, double *pb, double *pl) {
  DftFluxH *op = mode_object(F, c.h, c.nmodes);
  if (!op) return -1;
  DftFluxH &o = *op;
  if (mode_index_build(F, o)) return -1;
  mnlmodes::Geometry G;
  mnlmodes::Table T;
  if (mode_build_table(F, o, c, G, T)) return -1;
  dims[0] = T.na, dims[1] = T.nb, dims[2] = G.nlayer, dims[3] = G.da * 4 + (G.db < 0 ? 3 : G.db);
  if (coords) {
    int *q = coords;
    for (int v : G.ca) *q++ = v;
    for (int i = 0; i < T.nb; i++) *q++ = G.db >= 0 ? G.cb[i] : 0;
    *q++ = G.layer[0], *q++ = G.layer[1];
  }
  const size_t nmf = (size_t)T.nmodes * T.nfreq;
  auto put = [](double *dst, const std::vector<cplx> &v) {
    if (dst)
      for (size_t i = 0; i < v.size(); i++) dst[2 * i] = real(v[i]), dst[2 * i + 1] = imag(v[i]);
  };
  if (k)
    for (size_t i = 0; i < 3 * nmf; i++) k[i] = T.k[i];
  if (vgrp)
    for (size_t i = 0; i < nmf; i++) vgrp[i] = T.vgrp[i];
  put(amp, T.amp), put(pa, T.pa), put(pb, T.pb), put(pl, T.pl);
  return 0;
}

int mode_coefficients(mnl_fields *F, const ModeCall &c, double *coeffs, double *vgrp,
                      double *kpoints, double *cscale, double *overlaps) {
  DftFluxH *op = mode_object(F, c.h, c.nmodes);
  if (!op) return -1;
  DftFluxH &o = *op;
  DftFluxH::ModeIdx &M = o.mo;
  const int nm = c.nmodes, nf = o.nfreq;
  const size_t nmf = (size_t)nm * nf;
  std::vector<double> sums(16 * nmf, 0.0);  // [sum j][mode][freq][4]
  mnlmodes::Geometry G;
  mnlmodes::Table T;
  std::string why;
  bool ok = true;
  auto run = [&]() -> int {
    if (dft_flush(F, o)) return -1;  // the buffered updates first (same stream)
    if (mode_index_build(F, o)) return -1;
    if (mode_build_table(F, o, c, G, T)) return -1;
    if (!M.nwg) return 0;
    int comp[4], conj[4];
    mode_sum_components(o.normal, comp, conj);
    // one upload: pa, pb, pl, ac, as (complex)
    const size_t npa = (size_t)nm * T.na, npb = (size_t)nm * T.nb, npl = 2 * nmf, nam = 4 * nmf;
    std::vector<double> tab;
    tab.reserve(2 * (npa + npb + npl + 2 * nam));
    auto push = [&](const cplx &v) { tab.push_back(real(v)), tab.push_back(imag(v)); };
    for (const cplx &v : T.pa) push(v);
    for (const cplx &v : T.pb) push(v);
    for (const cplx &v : T.pl) push(v);
    for (size_t mf = 0; mf < nmf; mf++)
      for (int j = 0; j < 4; j++) push(T.amp[mf * 6 + conj[j]]);
    for (size_t mf = 0; mf < nmf; mf++)
      for (int j = 0; j < 4; j++) push(T.amp[mf * 6 + comp[j]]);
    const size_t npart = (size_t)M.nwg * nmf * 4, nout = 16 * nmf;
    if (M.tab_cap < tab.size() || M.part_cap < npart || M.out_cap < nout) {
      HIPCHK(hipStreamSynchronize(F->stream));
      for (double **p : {&M.d_tab, &M.d_part, &M.d_out}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
      }
      M.tab_cap = M.part_cap = M.out_cap = 0;
      HIPCHK(hipMalloc(&M.d_tab, tab.size() * 8));
      HIPCHK(hipMalloc(&M.d_part, npart * 8));
      HIPCHK(hipMalloc(&M.d_out, nout * 8));
      M.tab_cap = tab.size(), M.part_cap = npart, M.out_cap = nout;
    }
    HIPCHK(hipMemcpyAsync(M.d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemsetAsync(M.d_out, 0, nout * 8, F->stream));  // a sum without slots is 0
    ModeArgs a{};
    a.dft = o.d_dft, a.slot = M.d_slot, a.wv = M.d_wv, a.rng = M.d_rng;
    a.pa = M.d_tab, a.pb = a.pa + 2 * npa, a.pl = a.pb + 2 * npb, a.ac = a.pl + 2 * npl;
    a.as = a.ac + 2 * nam;
    a.nmodes = nm, a.nfreq = nf, a.na = T.na, a.nb = T.nb, a.part = M.d_part;
    if (k_mode_overlap(a, M.nwg, M.nslots, F->stream))
      return fail("mode overlap launch failed");
    for (int j = 0; j < 4; j++) {
      const int n = M.wg0[j + 1] - M.wg0[j];
      if (n > 0 && k_n2f_reduce(M.d_part + (size_t)M.wg0[j] * nmf * 4, M.d_out + (size_t)j * nmf * 4,
                                n, (long long)(nmf * 4), F->stream))
        return fail("mode overlap reduce launch failed");
    }
    HIPCHK(hipMemcpyAsync(sums.data(), M.d_out, nout * 8, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));  // (tab leaves scope)
    return 0;
  };
  if (run()) ok = false, why = g_err;
  if (F->nranks > 1) {
    if (F->comm->agree_ok(ok, F->stream))  // every rank fails together
      return ok ? fail("mode_coefficients: a rank failed") : (g_err = why, -1);
    for (size_t i0 = 0; i0 < sums.size(); i0 += 64)  // sum_to_all
      if (timed_allreduce(F, sums.data() + i0, (int)std::min<size_t>(64, sums.size() - i0)))
        return fail("mode_coefficients allreduce failed");
  }
  if (!ok) return g_err = why, -1;
  // src/mpb.cpp:957-999 per (mode, frequency)
  for (int m = 0; m < nm; m++)
    for (int f = 0; f < nf; f++) {
      const size_t mf = (size_t)m * nf + f;
      cplx S[4], MM[4];
      for (int j = 0; j < 4; j++) {
        const double *q = &sums[((size_t)j * nmf + mf) * 4];
        S[j] = cplx(q[0], q[1]), MM[j] = cplx(q[2], q[3]);
      }
      if (overlaps)
        for (int j = 0; j < 4; j++) {
          overlaps[(mf * 8 + j) * 2] = real(S[j]), overlaps[(mf * 8 + j) * 2 + 1] = imag(S[j]);
          overlaps[(mf * 8 + 4 + j) * 2] = real(MM[j]);
          overlaps[(mf * 8 + 4 + j) * 2 + 1] = imag(MM[j]);
        }
      if (T.evan[mf]) {  // mode not found, assume evanescent
        if (g_verbosity > 0 && F->rank == 0)
          printf("WARNING: diffraction order for g=(%d,%d,%d) is evanescent!\n", c.g[3 * m],
                 c.g[3 * m + 1], c.g[3 * m + 2]);
        for (int q = 0; q < 4; q++) coeffs[mf * 4 + q] = 0.0;
        if (vgrp) vgrp[mf] = 0.0;
        if (kpoints)
          for (int d = 0; d < 3; d++) kpoints[mf * 3 + d] = 0.0;
        if (cscale) cscale[mf] = 0.0;
        continue;
      }
      const double vg = T.vgrp[mf];
      if (vgrp) vgrp[mf] = vg;
      if (kpoints)
        for (int d = 0; d < 3; d++) kpoints[mf * 3 + d] = T.k[mf * 3 + d];
      const cplx mode_flux[2] = {S[0] - S[1], S[2] - S[3]};
      const cplx mode_mode[2] = {MM[0] - MM[1], MM[2] - MM[3]};
      const cplx cplus = 0.5 * (mode_flux[0] + mode_flux[1]);
      const cplx cminus = 0.5 * (mode_flux[0] - mode_flux[1]);
      cplx normfac = 0.5 * (mode_mode[0] + mode_mode[1]);
      if (normfac == 0.0) normfac = 1.0;
      const double csc = sqrt(1.0 / abs(normfac));
      if (cscale) cscale[mf] = csc;
      const cplx cp = cplus * csc, cm = cminus * csc;
      const int ip = vg > 0.0 ? 0 : 1;
      coeffs[mf * 4 + 2 * ip] = real(cp), coeffs[mf * 4 + 2 * ip + 1] = imag(cp);
      coeffs[mf * 4 + 2 * (1 - ip)] = real(cm), coeffs[mf * 4 + 2 * (1 - ip) + 1] = imag(cm);
    }
  return 0;
}

}  // namespace mnlh
