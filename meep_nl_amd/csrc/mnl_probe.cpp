// mnl_probe.cpp -- field probes and the norm of the DFT arrays.
// A probe is fields::get_field(c, pt) (src/monitor.cpp:127-160) recorded after every step on
// the device: one more object the DFT samplers sample (one list of up to 8 points with the
// get_field weights, no averaging, no frequencies), whose flush appends one value per buffered
// update to a device series instead of accumulating a DFT array.  dft_norm / dft_maxfreq /
// max_decimation are fields::dft_norm() and its companions (src/dft.cpp:312-399).
#include "mnl_host.hpp"

namespace mnlh {

// The set of sampled objects changed.  The pair plan holds raw pointers to the objects' compact
// boxes (tb_cmp) and its signature knows only their bounding boxes, not whose they are: drop
// the plan, so that the next batch of pairs builds a new one (a removed probe's box is freed
// with it, and a probe added again at the same point must get its own).
void dft_sampled_rebuild(mnl_fields *F) {
  F->tb_sig = 0;  // (tb_plan runs before every batch of pairs and compares signatures)
  F->tb_cmp.clear();
  F->sampled.clear();  // (may name an object that is gone already: not looked at)
  for (auto &o : F->dfts) F->sampled.push_back(o.get());
  for (auto &o : F->probes)
    if (o) F->sampled.push_back(o.get());
  for (auto &o : F->ldoses)
    if (o) F->sampled.push_back(o.get());
  for (DftFluxH *o : F->sampled) o->cmp_on = false;
}

// entries of a new probe's series: MNL_PROBE_CAP, or 2^16
static int probe_capacity() {
  const char *e = getenv("MNL_PROBE_CAP");
  return e ? std::max(1, atoi(e)) : 1 << 16;
}

static DftFluxH *probe_at(mnl_fields *F, int h) {
  const long long i = (long long)h - PROBE_BASE;
  if (h < PROBE_BASE || i >= (long long)F->probes.size() || !F->probes[i]) {
    fail("bad probe handle");
    return nullptr;
  }
  return F->probes[i].get();
}

// the interpolation points and weights of get_field (mnl_sources.cpp) as a DFT point list: a
// point this rank would read 0 for in value_at (outside the cell, not owned, component not
// allocated) is "another rank's" (-1)
int probe_add(mnl_fields *F, int c, const double pos[3]) {
  const mnl_structure &S = F->S;
  const DevGrid &g = F->g;
  if (F->probes.size() >= size_t(1) << 20) return fail("add_probe: too many probes");
  double pp[3] = {pos[0], pos[1], pos[2]};
  if (S.dim == 1) pp[0] = pp[1] = 0;
  if (S.dim == 2) pp[2] = 0;
  int locs[8][3];
  double w[8];
  interpolate(S, c, pp, locs, w);
  std::unique_ptr<DftFluxH> o(new DftFluxH);
  o->kind = DFT_PROBE, o->nlists = 1, o->fields = true;
  o->nfreq = 0, o->decim = 1;
  o->kb = dft_block();
  std::vector<double> pw;
  std::vector<int> pslot(8, -1);
  for (int k = 0; k < 3; k++) o->bbox.lo[k] = INT32_MAX, o->bbox.hi[k] = -1;
  int n = 0;
  for (int i = 0; i < 8 && w[i]; i++, n++) {
    int jg[3] = {0, 0, 0}, j[3] = {0, 0, 0};
    bool mine = F->allocated[c];
    for (int d = 0; d < 3; d++) {
      if (!S.has[d]) continue;
      const int q = locs[i][d] - S.io[d];
      if (!(q > 0 && q <= 2 * S.n[d])) mine = false;  // not owned by the cell
      jg[d] = (locs[i][d] - S.io[d] - S.shift(c, d)) / 2;
      j[d] = jg[d] - g.off[d];
    }
    mine = mine && local_index(F, c, jg, true) >= 0;
    for (int d = 0; d < 3; d++) o->h_pj.push_back(mine ? j[d] : -1);
    pw.push_back(w[i]);
    o->slot.push_back(i);
    if (!mine) continue;
    pslot[i] = i;
    for (int d = 0; d < 3; d++) {
      o->bbox.lo[d] = std::min(o->bbox.lo[d], j[d]);
      o->bbox.hi[d] = std::max(o->bbox.hi[d], j[d] + 1);
    }
  }
  DftChunkH dc{};
  dc.c = c, dc.scale = cplx(0.0), dc.avgmode = 0, dc.N = (size_t)n, dc.p0 = 0;
  dc.dV0 = 1.0, dc.incl = false, dc.stored = cplx(1.0);
  o->E.push_back(dc);
  o->npts = (size_t)n;
  // compact box of the pairs (3-D), as dft_layout gives every monitor one
  if (S.dim == 3 && o->bbox.hi[0] >= 0) {
    unsigned nc = 1;
    for (int k = 0; k < 3; k++) nc *= unsigned(o->bbox.hi[k] - o->bbox.lo[k] + 1);
    o->cmp_cells = nc;
    const bool mag = ctype(c) == T_H || ctype(c) == T_B;
    o->cmp_mask = 1u << (mag ? 3 + cdir(c) : cdir(c));
  }
  o->series_cap = probe_capacity();
  o->series_n = 0, o->series_t = F->t;
  const DftChunkDev cd{c, 0, -1, -1};
  const std::vector<int> pch(n, 0);
  HIPCHK(hipMalloc(&o->d_pj, o->h_pj.size() * 4));
  HIPCHK(hipMalloc(&o->d_pch, (size_t)n * 4));
  HIPCHK(hipMalloc(&o->d_pw, (size_t)n * 8));
  HIPCHK(hipMalloc(&o->d_ch, sizeof(DftChunkDev)));
  HIPCHK(hipMalloc(&o->d_fr, (size_t)n * o->kb * 8));
  HIPCHK(hipMalloc(&o->d_pslot, 8 * 4));
  HIPCHK(hipMalloc(&o->d_series, (size_t)o->series_cap * 8));
  HIPCHK(hipMemcpyAsync(o->d_pj, o->h_pj.data(), o->h_pj.size() * 4, hipMemcpyHostToDevice,
                        F->stream));
  HIPCHK(hipMemcpyAsync(o->d_pch, pch.data(), (size_t)n * 4, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemcpyAsync(o->d_pw, pw.data(), (size_t)n * 8, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemcpyAsync(o->d_ch, &cd, sizeof cd, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemcpyAsync(o->d_pslot, pslot.data(), 8 * 4, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipMemsetAsync(o->d_fr, 0, (size_t)n * o->kb * 8, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));  // the host vectors leave scope
  F->probes.push_back(std::move(o));
  dft_sampled_rebuild(F);
  return PROBE_BASE + int(F->probes.size()) - 1;
}

// the buffered rows -> the series: the value of step s at index s % series_cap
int probe_flush(mnl_fields *F, DftFluxH &o) {
  if (!o.nbuf) return 0;
  const int start = (int)((o.series_t + 1) % o.series_cap);
  if (k_probe_append(o.d_fr, (long long)o.npts, o.nbuf, o.d_pslot, (int)o.npts, o.d_series,
                     o.series_cap, start, F->stream))
    return fail("probe append launch failed");
  o.series_t += o.nbuf;
  o.series_n = std::min<long long>(o.series_n + o.nbuf, o.series_cap);
  o.nbuf = 0;
  return 0;
}

// count alone (values null: nothing is consumed), or the values since the last read, summed
// over the ranks as get_field's partial sums are, with the step of the first one
int probe_read(mnl_fields *F, int h, long long cap, long long *count, long long *t_first,
               double *values) {
  DftFluxH *op = probe_at(F, h);
  if (!op) return -1;
  DftFluxH &o = *op;
  std::string why;
  bool ok = true;
  long long n = 0;
  auto run = [&]() -> int {
    if (probe_flush(F, o)) return -1;  // the buffered rows first (same stream)
    n = o.series_n;
    *count = n;
    *t_first = o.series_t - n + 1;
    if (!values) return 0;
    if (cap < n) return fail("probe_read: buffer too small");
    const long long i0 = (*t_first % o.series_cap + o.series_cap) % o.series_cap;
    const long long n0 = std::min<long long>(n, o.series_cap - i0);  // up to the ring's end
    if (n0 > 0)
      HIPCHK(hipMemcpyAsync(values, o.d_series + i0, (size_t)n0 * 8, hipMemcpyDeviceToHost,
                            F->stream));
    if (n > n0)
      HIPCHK(hipMemcpyAsync(values + n0, o.d_series, (size_t)(n - n0) * 8, hipMemcpyDeviceToHost,
                            F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    o.series_n = 0;
    return 0;
  };
  if (run()) ok = false, why = g_err;
  if (F->nranks > 1) {
    if (F->comm->agree_ok(ok, F->stream))  // every rank fails together
      return ok ? fail("probe_read: a rank failed") : (g_err = why, -1);
    if (values)  // every rank has taken the same steps: n is the same everywhere
      for (long long q = 0; q < n; q += 1 << 20)
        if (timed_allreduce(F, values + q, (int)std::min<long long>(1 << 20, n - q)))
          return fail("probe_read allreduce failed");
  }
  if (!ok) return g_err = why, -1;
  return 0;
}

int probe_reset(mnl_fields *F, int h) {
  DftFluxH *o = probe_at(F, h);
  if (!o) return -1;
  if (probe_flush(F, *o)) return -1;
  o->series_n = 0;
  return 0;
}

// after the step counter was set (set_time, load): every probe empty at the new step
void probe_restart(mnl_fields *F) {
  for (auto &o : F->probes)
    if (o) o->nbuf = 0, o->series_n = 0, o->series_t = F->t;
}

int probe_remove(mnl_fields *F, int h) {
  if (!probe_at(F, h)) return -1;
  HIPCHK(hipStreamSynchronize(F->stream));  // no sample or append still in flight
  F->probes[h - PROBE_BASE].reset();        // the entry stays: no other probe's handle moves
  dft_sampled_rebuild(F);
  return 0;
}

int probe_remove_all(mnl_fields *F) {
  if (F->probes.empty()) return 0;
  HIPCHK(hipStreamSynchronize(F->stream));  // no sample or append still in flight
  F->probes.clear();
  dft_sampled_rebuild(F);
  return 0;
}

// fields::dft_norm (src/dft.cpp:312-361): sqrt of the sum of |dft|^2 over every frequency and
// point of every chunk of every DFT object, summed over the ranks.  Per object one launch over
// the array where it lives, split into workgroups by the object's size alone, the partial sums
// added in workgroup order; the objects' sums added in handle order on the host.
int dft_norm(mnl_fields *F, double *out) {
  *out = 0.0;
  std::string why;
  bool ok = true;
  double sum = 0.0;
  auto run = [&]() -> int {
    const size_t nobj = F->dfts.size();
    if (!nobj) return 0;
    if (F->norm_out_cap < nobj) {
      HIPCHK(hipStreamSynchronize(F->stream));
      if (F->d_norm_out) (void)hipFree(F->d_norm_out);
      F->d_norm_out = nullptr, F->norm_out_cap = 0;
      HIPCHK(hipMalloc(&F->d_norm_out, nobj * 8));
      F->norm_out_cap = nobj;
    }
    HIPCHK(hipMemsetAsync(F->d_norm_out, 0, nobj * 8, F->stream));
    for (size_t h = 0; h < nobj; h++) {
      DftFluxH &o = *F->dfts[h];
      if (dft_flush(F, o)) return -1;  // the buffered updates first (same stream)
      if (!o.npts || !o.nfreq) continue;
      const long long nblk = (long long)((o.npts + 63) / 64);
      if (!o.d_norm_part) {
        o.norm_wg_blocks = std::max<long long>(NORM_WG_BLOCKS, (nblk + NORM_MAX_WG - 1) / NORM_MAX_WG);
        o.norm_nwg = (int)((nblk + o.norm_wg_blocks - 1) / o.norm_wg_blocks);
        HIPCHK(hipMalloc(&o.d_norm_part, (size_t)o.norm_nwg * 8));
      }
      if (k_dft_norm(o.d_dft, o.d_pj, (long long)o.npts, o.nfreq, nblk, o.norm_wg_blocks,
                     o.norm_nwg, o.d_norm_part, F->stream))
        return fail("dft norm launch failed");
      if (k_n2f_reduce(o.d_norm_part, F->d_norm_out + h, o.norm_nwg, 1, F->stream))
        return fail("dft norm reduce launch failed");
    }
    std::vector<double> v(nobj);
    HIPCHK(hipMemcpyAsync(v.data(), F->d_norm_out, nobj * 8, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    for (double x : v) sum += x;
    return 0;
  };
  if (run()) ok = false, why = g_err;
  if (F->nranks > 1) {
    if (F->comm->agree_ok(ok, F->stream))  // every rank fails together
      return ok ? fail("dft_norm: a rank failed") : (g_err = why, -1);
    if (timed_allreduce(F, &sum, 1)) return fail("dft_norm allreduce failed");  // sum_to_all
  }
  if (!ok) return g_err = why, -1;
  *out = std::sqrt(sum);
  return 0;
}

// fields::dft_maxfreq (src/dft.cpp:380-399): every rank holds every object, no max_to_all
double dft_maxfreq(const mnl_fields *F) {
  double maxomega = 0;
  for (auto &o : F->dfts)
    for (double w : o->omega) maxomega = std::max(maxomega, std::abs(w));
  return maxomega / (2 * pi);
}

// fields::max_decimation (src/dft.cpp:365-377)
int dft_max_decimation(const mnl_fields *F) {
  int maxdec = 1;
  for (auto &o : F->dfts) maxdec = std::max(maxdec, o->decim);
  return maxdec;
}

}  // namespace mnlh
