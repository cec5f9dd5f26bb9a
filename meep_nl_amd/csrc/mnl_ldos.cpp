// mnl_ldos.cpp -- LDOS spectra: dft_ldos (src/dft_ldos.cpp).
// An LDOS object is one more object the DFT samplers sample: two point lists, the points of
// every electric source volume (the raw Yee value of E there, weight 1) and of every magnetic one
// (H), in the order dft_ldos::update visits them.  A flush reduces every buffered row to
// EJ = sum E conj(A) and HJ = sum H conj(A) on the device (k_ldos_reduce, k_n2f_reduce) and adds
// Ephase EJ + Hphase HJ to the device Fdft (k_ldos_accum); Jdft is host data.
#include "mnl_host.hpp"

namespace mnlh {

static DftFluxH *ldos_at(mnl_fields *F, int h) {
  const long long i = (long long)h - LDOS_BASE;
  if (h < LDOS_BASE || i >= (long long)F->ldoses.size() || !F->ldoses[i]) {
    fail("bad ldos handle");
    return nullptr;
  }
  return F->ldoses[i].get();
}

static size_t ldos_rowlen(const DftFluxH &o) { return 4 * (size_t)o.nfreq + 2; }

// gv.dV(gv.icenter(), 1).computational_volume() (src/vec.cpp:175-179, 623-634, 1089-1101)
static double ldos_dV(const mnl_structure &S) {
  const double inva = 1.0 / S.a, hinva = 0.5 * inva * 1.0;
  double vol = 1.0;
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    const int n = S.n[d] - (S.n[d] & 1);  // round_down_to_even
    const double h = (S.io[d] + n) * (0.5 * inva);
    vol *= (h + hinva) - (h - hinva);
  }
  return vol;
}

static void ldos_free_lists(DftFluxH &o) {
  for (void **p : {(void **)&o.d_pj, (void **)&o.d_pch, (void **)&o.d_pw, (void **)&o.d_ch,
                   (void **)&o.d_fr, (void **)&o.d_sidx, (void **)&o.d_ssel, (void **)&o.d_spal,
                   &o.d_su, (void **)&o.d_bad, (void **)&o.ld->d_amp, (void **)&o.ld->d_part}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}

// The two lists from the current sources.  dft_ldos::update (src/dft_ldos.cpp:107-149): chunks in
// chunk order, each chunk's sources in list order (a source volume's points of one chunk are one
// src_vol there), each volume's points in index order; the electric sources of every chunk form
// the E list, the magnetic ones the H list.  Nothing is in flight and nothing buffered.
static int ldos_build(mnl_fields *F, DftFluxH &o) {
  const mnl_structure &S = F->S;
  const DevGrid &g = F->g;
  LdosH &L = *o.ld;
  ldos_free_lists(o);
  L.comp.clear(), L.ijk.clear(), L.amp.clear();
  o.h_pj.clear(), o.slot.clear(), o.E.clear(), o.H.clear();
  o.plan_key = -1;
  for (int k = 0; k < 3; k++) o.bbox.lo[k] = INT32_MAX, o.bbox.hi[k] = -1;
  size_t cnt[2] = {0, 0};
  for (int mag = 0; mag < 2; mag++) {
    std::vector<std::array<int, 3>> ord;  // (chunk, group, point), group-major as added
    for (size_t gi = 0; gi < F->groups.size(); gi++) {
      const SrcGroup &G = F->groups[gi];
      if ((ctype(G.comp) == T_H) != (mag == 1)) continue;
      for (size_t j = 0; j < G.gidx.size(); j++) ord.push_back({G.chunk[j], (int)gi, (int)j});
    }
    std::stable_sort(ord.begin(), ord.end(),
                     [](const std::array<int, 3> &a, const std::array<int, 3> &b) {
                       return a[0] < b[0];
                     });
    for (const auto &e : ord) {
      const SrcGroup &G = F->groups[e[1]];
      L.comp.push_back(3 * (mag ? T_H : T_E) + cdir(G.comp));
      for (int d = 0; d < 3; d++) L.ijk.push_back(G.jglob[3 * e[2] + d]);
      L.amp.push_back(G.amp[e[2]]);
    }
    cnt[mag] = ord.size();
  }
  L.nE = cnt[0], L.nH = cnt[1];
  double asum = 0.0;  // Jsum += abs(A) in list order; the whole list on every rank
  for (const cplx &A : L.amp) asum += std::abs(A);
  L.jsum_lists = asum * sqrt(ldos_dV(S));
  const size_t n = L.nE + L.nH, npad = (n + 1) & ~size_t(1);
  o.npts = npad;
  o.cmp_cells = 0;  // no compact box: the pair plan keeps the middle state of bbox in the mid set
  L.nwg = 0, L.wg_pairs = 0;
  if (!npad) return 0;
  std::vector<double> pw(npad, 1.0), amp(2 * npad, 0.0);
  std::vector<int> pch(npad, 0);
  o.h_pj.assign(3 * npad, -1);  // the padded tail: nobody's
  for (size_t p = 0; p < n; p++) {
    const int c = L.comp[p];
    const int *jg = &L.ijk[3 * p];
    // owned as the source lists own their points (build_source_lists): exactly one rank's
    const bool mine = F->allocated[c] && local_index(F, c, jg, false) >= 0;
    pch[p] = ctype(c) == T_H ? 3 + cdir(c) : cdir(c);
    amp[2 * p] = real(L.amp[p]), amp[2 * p + 1] = imag(L.amp[p]);
    o.slot.push_back((int)p);
    if (!mine) continue;
    for (int d = 0; d < 3; d++) {
      const int j = S.has[d] ? jg[d] - g.off[d] : 0;
      o.h_pj[3 * p + d] = j;
      o.bbox.lo[d] = std::min(o.bbox.lo[d], j);
      o.bbox.hi[d] = std::max(o.bbox.hi[d], j + 1);
    }
  }
  DftChunkDev cd[6];
  for (int k = 0; k < 6; k++) cd[k] = DftChunkDev{3 * (k < 3 ? T_E : T_H) + k % 3, 0, -1, -1};
  const long long pairs = (long long)(npad >> 1);
  L.wg_pairs = std::max<long long>(LDOS_WG_PAIRS, (pairs + LDOS_MAX_WG - 1) / LDOS_MAX_WG);
  L.nwg = (int)((pairs + L.wg_pairs - 1) / L.wg_pairs);
  HIPCHK(hipMalloc(&o.d_pj, o.h_pj.size() * 4));
  HIPCHK(hipMalloc(&o.d_pch, npad * 4));
  HIPCHK(hipMalloc(&o.d_pw, npad * 8));
  HIPCHK(hipMalloc(&o.d_ch, sizeof cd));
  HIPCHK(hipMalloc(&o.d_fr, npad * (size_t)o.kb * 8));
  HIPCHK(hipMalloc(&L.d_amp, npad * 16));
  HIPCHK(hipMalloc(&L.d_part, (size_t)L.nwg * o.kb * 4 * 8));
  HIPCHK(hipMemcpyAsync(o.d_pj, o.h_pj.data(), o.h_pj.size() * 4, hipMemcpyHostToDevice,
                        F->stream));
  HIPCHK(hipMemcpyAsync(o.d_pch, pch.data(), npad * 4, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemcpyAsync(o.d_pw, pw.data(), npad * 8, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemcpyAsync(o.d_ch, cd, sizeof cd, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemcpyAsync(L.d_amp, amp.data(), npad * 16, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemsetAsync(o.d_fr, 0, npad * (size_t)o.kb * 8, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));  // the host vectors leave scope
  return 0;
}

int ldos_add(mnl_fields *F, const double *freqs, int nfreq) {
  if (nfreq < 1) return fail("add_ldos: no frequencies");
  if (F->ldoses.size() >= size_t(1) << 20) return fail("add_ldos: too many LDOS objects");
  if (F->src_dirty && build_source_lists(F)) return -1;
  std::unique_ptr<DftFluxH> o(new DftFluxH);
  o->kind = DFT_LDOS, o->nlists = 2, o->fields = false;
  o->nfreq = nfreq, o->decim = 1;
  o->kb = dft_block();
  o->ld.reset(new LdosH);
  o->ld->freq.assign(freqs, freqs + nfreq);
  o->ld->Jdft.assign(nfreq, cplx(0.0));
  HIPCHK(hipMalloc(&o->ld->d_F, (size_t)nfreq * 16));
  HIPCHK(hipMalloc(&o->ld->d_ej, (size_t)o->kb * 4 * 8));
  HIPCHK(hipMemsetAsync(o->ld->d_F, 0, (size_t)nfreq * 16, F->stream));
  if (ldos_build(F, *o)) return -1;
  F->ldoses.push_back(std::move(o));
  dft_sampled_rebuild(F);
  return LDOS_BASE + int(F->ldoses.size()) - 1;
}

// the source lists were rebuilt (sources added, removed, changed): every object accumulates what
// it has buffered with the lists those rows were sampled with, then takes the new lists
int ldos_sources_rebuilt(mnl_fields *F) {
  bool any = false;
  for (auto &o : F->ldoses) {
    if (!o) continue;
    if (ldos_flush(F, *o)) return -1;
    any = true;
  }
  if (!any) return 0;
  HIPCHK(hipStreamSynchronize(F->stream));  // no sample or flush still in flight
  for (auto &o : F->ldoses)
    if (o && ldos_build(F, *o)) return -1;
  dft_sampled_rebuild(F);
  return 0;
}

// one row per update: Ephase[nfreq], Hphase[nfreq] (src/dft_ldos.cpp:151-152), then the current
// of the first source as dft_ldos::update reads it at step count t -- the last calc_sources of
// fields::step was at time() + dt of the step before (src/step.cpp:106), 0 before the first step
// and before the first step after the first src_time was created (its cache starts at 0)
// -- and whether there is a source at all (src/dft_ldos.cpp:156)
static void ldos_row(const mnl_fields *F, const DftFluxH &o, long long t, std::vector<double> &ph) {
  const double dt = F->dt, time = t * dt;
  const double scale = (dt / sqrt(2 * pi));
  for (int half = 0; half < 2; half++)
    for (int i = 0; i < o.nfreq; i++) {
      const double f = o.ld->freq[i];
      const cplx p = half == 0 ? std::polar(1.0, 2 * pi * f * time) * scale
                               : std::polar(1.0, 2 * pi * f * (time - dt / 2)) * scale;
      ph.push_back(p.real());
      ph.push_back(p.imag());
    }
  double J = 0.0;
  if (!F->srcs.empty() && t > F->src0_born) {
    SrcTime st = F->srcs[0];
    st.cur_time = NAN;
    st.update((t - 1) * dt + dt, dt);
    J = real(st.cur_current);
  }
  ph.push_back(J);
  ph.push_back(F->srcs.empty() ? 0.0 : 1.0);
}

// the buffered rows to the front, then the rows of the updates at the step counts ts
static int ldos_rows(mnl_fields *F, DftFluxH &o, const std::vector<long long> &ts) {
  const size_t rowlen = ldos_rowlen(o);
  std::vector<double> ph;
  ph.reserve(((size_t)o.nbuf + ts.size()) * rowlen);
  if (o.nbuf > 0) {
    if (o.ph_host.size() < (size_t)o.row * rowlen || o.row < o.nbuf)
      return fail("ldos: buffered phase rows lost");
    ph.insert(ph.end(), o.ph_host.begin() + (size_t)(o.row - o.nbuf) * rowlen,
              o.ph_host.begin() + (size_t)o.row * rowlen);
  }
  o.row = o.nbuf;
  for (long long t : ts) ldos_row(F, o, t, ph);
  if (ph.empty()) {
    o.ph_host.clear();
    return 0;
  }
  if (o.ph_cap < ph.size()) {
    HIPCHK(hipStreamSynchronize(F->stream));
    if (o.d_ph) hipFree(o.d_ph);
    o.d_ph = nullptr, o.ph_cap = 0;
    HIPCHK(hipMalloc(&o.d_ph, ph.size() * 8));
    o.ph_cap = ph.size();
  }
  HIPCHK(hipMemcpyAsync(o.d_ph, ph.data(), ph.size() * 8, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  o.ph_host.swap(ph);
  return 0;
}

// before a chunk of ns steps from step t0: the rows of the recording objects' updates
int ldos_prepare(mnl_fields *F, long long t0, int ns) {
  for (auto &op : F->ldoses) {
    if (!op) continue;
    DftFluxH &o = *op;
    if (!o.ld->rec) continue;  // (rows still buffered stay where they are)
    std::vector<long long> ts;
    for (int s = 0; s < ns; s++) ts.push_back(t0 + s + 1);
    if (ldos_rows(F, o, ts)) return -1;
  }
  return 0;
}

// an update was sampled: Jsum is that of the lists it used (recomputed by every update,
// src/dft_ldos.cpp:105-165)
void ldos_sampled(mnl_fields *, DftFluxH &o) { o.ld->jsum = o.ld->jsum_lists; }

// dft_ldos::update(fields&): one update of the current state
int ldos_update(mnl_fields *F, int h) {
  if (!ldos_at(F, h)) return -1;
  if (F->src_dirty && build_source_lists(F)) return -1;  // (may rebuild the object's lists)
  DftFluxH &o = *ldos_at(F, h);
  if (ldos_rows(F, o, {F->t})) return -1;
  if (!o.npts) {  // no source point anywhere: EJ = HJ = 0, Jsum = 0; the row still counts for J
    o.nbuf++, o.row++;
    ldos_sampled(F, o);
    return o.nbuf == o.kb ? ldos_flush(F, o) : 0;
  }
  return dft_update(F, F->t, nullptr, -1, &o);
}

int ldos_record(mnl_fields *F, int h, int on) {
  DftFluxH *o = ldos_at(F, h);
  if (!o) return -1;
  o->ld->rec = on != 0;
  return 0;
}

// accumulate the buffered rows: the device sums and Fdft, then Jdft on the host in update order
int ldos_flush(mnl_fields *F, DftFluxH &o) {
  if (!o.nbuf) return 0;
  LdosH &L = *o.ld;
  const int n = o.nbuf;
  const size_t rowlen = ldos_rowlen(o);
  if (o.ph_host.size() < (size_t)o.row * rowlen || o.row < n)
    return fail("ldos: buffered phase rows lost");
  if (o.npts) {
    if (k_ldos_reduce(o.d_fr, L.d_amp, o.d_pj, (long long)o.npts, (long long)L.nE, n, L.wg_pairs,
                      L.nwg, L.d_part, F->stream))
      return fail("ldos reduce launch failed");
    if (k_n2f_reduce(L.d_part, L.d_ej, L.nwg, (long long)n * 4, F->stream))
      return fail("ldos reduce launch failed");
    if (k_ldos_accum(L.d_ej, o.d_ph + (size_t)(o.row - n) * rowlen, (long long)rowlen, n, o.nfreq,
                     L.d_F, F->stream))
      return fail("ldos accumulate launch failed");
  }
  for (int u = 0; u < n; u++) {
    const double *r = &o.ph_host[(size_t)(o.row - n + u) * rowlen];
    if (r[4 * o.nfreq + 1] == 0.0) continue;  // no sources: Jdft is not touched
    const double J = r[4 * o.nfreq];
    for (int i = 0; i < o.nfreq; i++) L.Jdft[i] += cplx(r[2 * i], r[2 * i + 1]) * J;
  }
  o.nbuf = 0;
  return 0;
}

// dft_ldos::ldos / F / J / overall_scale (src/dft_ldos.cpp:60-95); any output may be null.  F is
// summed over the ranks and the formula applied to the sum (the reference applies it per rank
// and sums: the same up to rounding); J and Jsum are the same on every rank.
int ldos_data(mnl_fields *F, int h, double *ldos, double *Fout, double *Jout, double *scale) {
  DftFluxH *op = ldos_at(F, h);
  if (!op) return -1;
  DftFluxH &o = *op;
  LdosH &L = *o.ld;
  const int nf = o.nfreq;
  std::vector<double> Fv(2 * (size_t)nf, 0.0);
  std::string why;
  bool ok = true;
  auto run = [&]() -> int {
    if (ldos_flush(F, o)) return -1;  // the buffered rows first (same stream)
    HIPCHK(hipMemcpyAsync(Fv.data(), L.d_F, (size_t)nf * 16, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    return 0;
  };
  if (run()) ok = false, why = g_err;
  if (F->nranks > 1) {
    if (F->comm->agree_ok(ok, F->stream))  // every rank fails together
      return ok ? fail("ldos_data: a rank failed") : (g_err = why, -1);
    for (int q = 0; q < 2 * nf; q += 64)  // sum_to_all
      if (timed_allreduce(F, Fv.data() + q, std::min(64, 2 * nf - q)))
        return fail("ldos_data allreduce failed");
  }
  if (!ok) return g_err = why, -1;
  const double Jsum_all = L.jsum;
  const double s = 4.0 / pi * -0.5 / (Jsum_all * Jsum_all);
  for (int i = 0; i < nf; i++) {
    const cplx Fi(Fv[2 * i], Fv[2 * i + 1]), Ji = L.Jdft[i];
    const double abs2 = real(Ji) * real(Ji) + imag(Ji) * imag(Ji);
    if (ldos) ldos[i] = s * real(Fi * conj(Ji)) / abs2;
    if (Fout) Fout[2 * i] = Fv[2 * i], Fout[2 * i + 1] = Fv[2 * i + 1];
    if (Jout) Jout[2 * i] = real(Ji), Jout[2 * i + 1] = imag(Ji);
  }
  if (scale) *scale = s;
  return 0;
}

// the global list in list order, E list then H list
int ldos_points(mnl_fields *F, int h, long long cap, long long *n, int *comp, int *ijk,
                double *amp) {
  if (!ldos_at(F, h)) return -1;
  if (F->src_dirty && build_source_lists(F)) return -1;
  const LdosH &L = *ldos_at(F, h)->ld;
  const long long np = (long long)(L.nE + L.nH);
  *n = np;
  if (!comp && !ijk && !amp) return 0;
  if (cap < np) return fail("ldos_points: buffer too small");
  for (long long p = 0; p < np; p++) {
    if (comp) comp[p] = L.comp[p];
    if (ijk)
      for (int d = 0; d < 3; d++) ijk[3 * p + d] = L.ijk[3 * p + d];
    if (amp) amp[2 * p] = real(L.amp[p]), amp[2 * p + 1] = imag(L.amp[p]);
  }
  return 0;
}

// after the step counter was set (set_time, load): the buffered rows are dropped
void ldos_restart(mnl_fields *F) {
  for (auto &o : F->ldoses)
    if (o) o->nbuf = 0, o->row = 0;
}

int ldos_remove(mnl_fields *F, int h) {
  if (!ldos_at(F, h)) return -1;
  HIPCHK(hipStreamSynchronize(F->stream));  // no sample or flush still in flight
  F->ldoses[h - LDOS_BASE].reset();         // the entry stays: no other object's handle moves
  dft_sampled_rebuild(F);
  return 0;
}

int ldos_remove_all(mnl_fields *F) {
  if (F->ldoses.empty()) return 0;
  HIPCHK(hipStreamSynchronize(F->stream));
  F->ldoses.clear();
  dft_sampled_rebuild(F);
  return 0;
}

}  // namespace mnlh
