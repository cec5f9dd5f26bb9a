// mnl_tune.cpp -- the tuner of the fused step's knobs (mnl_fields_tune).
#include "mnl_host.hpp"

namespace mnlh {

// Tuning of the fused step, measured rather than modelled:
// (1) the tile kernel's z-chunk length (fill of the last round of items vs. the halo planes
// of short chunks); (2) on one rank with polarization chunks, the CUs given to their general
// kernel running beside the tile kernel (a split that balances the two launches; too few
// or too many CUs and one of them runs alone at the end).  Every candidate is stepped for
// real: results do not depend on either knob (each point's update is the same arithmetic).
// Times are the fused launches' own (profiling events around them), not the host's
// per-batch work.
int tune(mnl_fields *F, int reps, int *zchunk, int *gen_cus) {
  // the first step runs unfused (lazy first updates); the second takes the fused decision
  for (int i = 0; i < 2 && !F->fused; i++)
    if (fields_step(F, 1)) return -1;
  if (!F->fused) return 0;
  const bool prof = F->profiling;  // restored with the timers after tuning
  double tms[TM_CAP];
  long long tcnt[TM_CAP];
  for (int k = 0; k < TM_CAP; k++) tms[k] = F->timer_ms[k], tcnt[k] = F->timer_count[k];
  F->profiling = true;
  const bool verbose = getenv("MNL_TUNE_VERBOSE") != nullptr;
  // per-step time of the fused launches: tile kernel (+ the pairs' phase and rim launches of
  // temporal blocking) and the polarization chunks' general kernel
  auto fused_ms = [&]() {
    return F->timer_ms[TM_BINT] + F->timer_ms[TM_TB] + F->timer_ms[TM_RIM];
  };
  auto timed = [&](double *tile_ms, double *gen_ms) -> int {  // two warm-up steps (a pair
    if (fields_step(F, 2)) return -1;                           // builds its plan), then an
    const int r = reps + (reps & 1);                            // even number timed
    const double b0 = fused_ms(), g0 = F->timer_ms[TM_GEN];
    if (fields_step(F, r)) return -1;
    *tile_ms = (fused_ms() - b0) / r;
    *gen_ms = (F->timer_ms[TM_GEN] - g0) / r;
    if (F->nranks > 1) {  // every rank keeps the same knobs: the slowest rank's times
      std::vector<double> v(2 * (size_t)F->nranks, 0.0);
      v[2 * F->rank] = *tile_ms, v[2 * F->rank + 1] = *gen_ms;
      if (F->comm->allreduce_sum(v.data(), (int)v.size(), F->stream)) return fail("tune allreduce failed");
      for (int q = 0; q < F->nranks; q++)
        *tile_ms = std::max(*tile_ms, v[2 * q]), *gen_ms = std::max(*gen_ms, v[2 * q + 1]);
    }
    return 0;
  };
  int rc = 0;
  const int split0 = F->tile_gen_cus;
  if (!F->fused_zchunk_env) {
    static const int cand[] = {0, 16, 20, 24, 32, 48};
    F->tile_gen_cus = 0;  // the two launches one after the other while the length is chosen
    int best = F->fused_zchunk;
    double best_ms = 0;
    for (int c : cand) {
      if (F->fused && set_fused(F, false)) { rc = -1; break; }
      F->fused_zchunk = c;
      double tm, gm;
      if (timed(&tm, &gm)) { rc = -1; break; }
      if (!F->fused) continue;  // this length does not fit the fused kernels; longer ones may
      if (verbose)
        fprintf(stderr, "tune rank %d: zchunk %d: %.4f ms/step (tile %.4f, general %.4f)\n",
                F->rank, c, tm + gm, tm, gm);
      if (best_ms == 0 || tm + gm < best_ms) best_ms = tm + gm, best = c;
    }
    F->tile_gen_cus = split0;
    if (!rc && F->fused && set_fused(F, false)) rc = -1;  // the next step rebuilds with `best`
    F->fused_zchunk = best;
    if (!rc && zchunk) *zchunk = best;
  }
  if (!rc && F->nranks == 1 && !F->tile_gen_cus_env) {
    F->tile_gen_cus = 0;
    double tm = 0, gm = 0;
    if (timed(&tm, &gm)) rc = -1;
    if (!rc && F->fused && gm > 0) {
      // start from the split that gives both launches the same time at their measured
      // one-after-the-other rates, in multiples of 8 CUs (one per XCD)
      const int cus = k_cu_count();
      const int s0 = 8 * (int)std::lround(cus * gm / (gm + tm) / 8.0);
      int best = 0;
      double best_ms = tm + gm;
      if (verbose)
        fprintf(stderr, "tune rank %d: general CUs 0: %.4f ms/step\n", F->rank, best_ms);
      for (int d : {-16, -8, 0, 8, 16}) {
        const int sc = s0 + d;
        if (sc < 8 || sc > cus - 8) continue;
        F->tile_gen_cus = sc;
        double t2, g2;
        if (timed(&t2, &g2)) { rc = -1; break; }
        if (verbose)
          fprintf(stderr, "tune rank %d: general CUs %d: %.4f ms/step\n", F->rank, sc, t2 + g2);
        if (t2 + g2 < best_ms) best_ms = t2 + g2, best = sc;
      }
      F->tile_gen_cus = best;
      if (!rc && gen_cus) *gen_cus = best;
    } else {
      F->tile_gen_cus = split0;
    }
  }
  // temporal blocking: planes per two-step item (automatic = the item count that fills whole
  // rounds), and whether pairs beat one-step stepping at all (small grids: the rim is a
  // large share of the cells)
  if (!rc && F->fused && F->tb_have && F->tb_enabled) {
    const int tz0 = F->tb_zchunk, ox0 = F->tb_ox;
    int best = tz0, best_ox = ox0;
    double best_ms = 0;
    // (16 / 24 / 40 added in round 5: 256^3 C2 runs 6 % faster at 16-24 planes than with the
    // automatic length, profiles/r05_ab_tb_zchunk_c2_256.json.  Round 6: the items hold up to
    // 124 columns, so a small grid has few of them per plane; 60-column items (half the lanes
    // idle, twice the items) and 12 / 20 planes are tried too, against the tail of a launch
    // with fewer items than a few rounds of CUs)
    // Round 6: the candidates' differences at 256^3 are within one box's drift over a sweep
    // (C2 picked 48 planes once, 6 % slower than 16-24), so the sweep runs forward and then
    // backward (a candidate's time is its better one), and the three best are timed again
    // with twice the steps before the choice
    std::vector<std::pair<int, int>> cands;  // (width setting, planes)
    for (int ox : {0, 60}) {
      if (F->tb_ox_set && ox != ox0) continue;
      for (int c : {0, 12, 16, 20, 24, 32, 40, 48, 64, 96, 128}) {
        if (F->tb_zchunk_env && c != tz0) continue;
        if (ox == 60 && c > 48) continue;  // the narrow items only help small grids
        cands.push_back({ox, c});
      }
    }
    std::vector<double> cms(cands.size(), 0.0);
    auto measure = [&](size_t i, int mult) -> int {
      F->tb_ox = cands[i].first;
      F->tb_zchunk = cands[i].second;
      double tm = 0, gm = 0;
      const int reps0 = reps;
      reps *= mult;
      const int r = timed(&tm, &gm);
      reps = reps0;
      if (r) return -1;
      if (verbose)
        fprintf(stderr, "tune rank %d: two-step planes %d, width %d: %.4f ms/step\n", F->rank,
                cands[i].second, cands[i].first ? cands[i].first : TB_OXW, tm + gm);
      if (cms[i] == 0 || tm + gm < cms[i]) cms[i] = tm + gm;
      return 0;
    };
    for (size_t i = 0; i < cands.size() && !rc; i++) rc = measure(i, 1);
    for (size_t i = cands.size(); i-- > 0 && !rc;) rc = measure(i, 1);
    if (!rc && cands.size() > 1) {
      std::vector<size_t> ord(cands.size());
      for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
      std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return cms[x] < cms[y]; });
      for (size_t k = 0; k < std::min<size_t>(3, ord.size()) && !rc; k++) rc = measure(ord[k], 2);
    }
    for (size_t i = 0; i < cands.size() && !rc; i++)
      if (best_ms == 0 || cms[i] < best_ms) best_ms = cms[i], best = cands[i].second, best_ox = cands[i].first;
    F->tb_zchunk = rc ? tz0 : best;
    F->tb_ox = rc ? ox0 : best_ox;
    if (!rc && !F->tb_env) {  // one-step stepping, timed twice as well (the better one)
      F->tb_enabled = false;
      double one = 0;
      for (int mult = 1; mult <= 2 && !rc; mult++) {
        double tm, gm;
        const int reps0 = reps;
        reps *= mult;
        if (timed(&tm, &gm)) rc = -1;
        reps = reps0;
        if (rc) break;
        if (verbose)
          fprintf(stderr, "tune rank %d: one-step: %.4f ms/step\n", F->rank, tm + gm);
        if (one == 0 || tm + gm < one) one = tm + gm;
      }
      F->tb_enabled = rc || one >= best_ms;
    }
  }
  F->profiling = prof;
  for (int k = 0; k < TM_CAP; k++) F->timer_ms[k] = tms[k], F->timer_count[k] = tcnt[k];
  return rc;
}

}  // namespace mnlh
