// mnl_pair_runs.hpp -- the run table of a pair sum (energy and force monitors, DESIGN.md
// section 30).  Plain C++ with no device or runtime types, so that it also builds into a
// stand-alone host program (tests/cpu/pair_runs_main.cpp).
#pragma once
#include <cstddef>
#include <vector>

namespace mnl {

struct PairRun {
  long long g0;    // pair points of the runs before this one
  int a0, b0, n;   // slots [a0, a0 + n) of the first list pair with [b0, b0 + n) of the second
  double x;        // the factor: 0.5 (energy) or the chunk's extra weight (force)
};

struct PairChunk {
  size_t p0, N;    // first point and points in the object's point arrays
  double extra;    // dft_chunk::extra_weight
};

// Lists A and B zipped chunk by chunk until the shorter one ends (the reference's
// for (cur1 && cur2) loops, src/dft.cpp:662-666, src/stress.cpp:91-98), this rank's points
// only (pj: 3 indices per point, -1: another rank's; slot: the device slot per point).  A run
// ends where either chunk's slots stop being consecutive; runs do not continue across chunks.
// x < 0: the first chunk's extra weight.  Appends to `runs`, returns the pair points so far.
inline long long pair_runs(const std::vector<PairChunk> &A, const std::vector<PairChunk> &B,
                           const std::vector<int> &pj, const std::vector<int> &slot, double x,
                           std::vector<PairRun> &runs, long long total) {
  for (size_t k = 0; k < A.size() && k < B.size(); k++) {
    const double xk = x < 0 ? A[k].extra : x;
    bool open = false;
    for (size_t i = 0; i < A[k].N && i < B[k].N; i++) {
      const size_t pa = A[k].p0 + i, pb = B[k].p0 + i;
      if (pj[3 * pa] < 0 || pj[3 * pb] < 0) continue;  // another rank's point
      const int sa = slot[pa], sb = slot[pb];
      if (open && runs.back().a0 + runs.back().n == sa && runs.back().b0 + runs.back().n == sb) {
        runs.back().n++;
      } else {
        runs.push_back({total, sa, sb, 1, xk});
        open = true;
      }
      total++;
    }
  }
  return total;
}

}  // namespace mnl
