// Stand-alone check of the pair-sum run table (meep_nl_amd/csrc/mnl_pair_runs.hpp), meant to be
// built with -fsanitize=address,undefined and run on its own
// (tests/test_dft_energy_force_cpu.py): lists of unequal length, chunks of unequal size,
// other ranks' points, broken slot sequences, and an exhaustive comparison of the runs with a
// point-by-point walk.  Exit status 0 and "ok" on success.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mnl_pair_runs.hpp"

using namespace mnl;

static int fails = 0;
#define CHECK(c)                                        \
  do {                                                  \
    if (!(c)) {                                         \
      printf("line %d: %s failed\n", __LINE__, #c);     \
      fails++;                                          \
    }                                                   \
  } while (0)

struct Lists {
  std::vector<PairChunk> A, B;
  std::vector<int> pj, slot;
};

// expand runs back into (slot a, slot b, x) triples
static std::vector<std::vector<double>> expand(const std::vector<PairRun> &runs) {
  std::vector<std::vector<double>> out;
  long long g = 0;
  for (auto &r : runs) {
    CHECK(r.g0 == g);
    CHECK(r.n >= 1);
    for (int i = 0; i < r.n; i++, g++) out.push_back({double(r.a0 + i), double(r.b0 + i), r.x});
  }
  return out;
}

static std::vector<std::vector<double>> walk(const Lists &l, double x) {
  std::vector<std::vector<double>> out;
  for (size_t k = 0; k < l.A.size() && k < l.B.size(); k++)
    for (size_t i = 0; i < l.A[k].N && i < l.B[k].N; i++) {
      const size_t pa = l.A[k].p0 + i, pb = l.B[k].p0 + i;
      if (l.pj[3 * pa] < 0 || l.pj[3 * pb] < 0) continue;
      out.push_back({double(l.slot[pa]), double(l.slot[pb]), x < 0 ? l.A[k].extra : x});
    }
  return out;
}

static unsigned rnd(unsigned &s) { return s = s * 1664525u + 1013904223u; }

int main() {
  {  // two chunks of 4 and 3 points against 4 and 3: consecutive slots give one run per chunk
    Lists l;
    l.A = {{0, 4, 0.5}, {4, 3, -0.5}};
    l.B = {{7, 4, 1.0}, {11, 3, 1.0}};
    for (int p = 0; p < 14; p++) {
      l.slot.push_back(p);
      for (int e = 0; e < 3; e++) l.pj.push_back(p);
    }
    std::vector<PairRun> runs;
    const long long n = pair_runs(l.A, l.B, l.pj, l.slot, -1.0, runs, 0);
    CHECK(n == 7);
    CHECK(runs.size() == 2);
    CHECK(runs[0].a0 == 0 && runs[0].b0 == 7 && runs[0].n == 4 && runs[0].x == 0.5);
    CHECK(runs[1].a0 == 4 && runs[1].b0 == 11 && runs[1].n == 3 && runs[1].x == -0.5);
    CHECK(runs[1].g0 == 4);
  }
  {  // empty lists, and a longer first list: the zip ends with the shorter one
    Lists l;
    std::vector<PairRun> runs;
    CHECK(pair_runs(l.A, l.B, l.pj, l.slot, 0.5, runs, 0) == 0 && runs.empty());
    l.A = {{0, 2, 1.0}, {2, 2, 1.0}};
    l.B = {{4, 2, 1.0}};
    for (int p = 0; p < 6; p++) {
      l.slot.push_back(5 - p);  // descending slots: one run per point
      for (int e = 0; e < 3; e++) l.pj.push_back(0);
    }
    CHECK(pair_runs(l.A, l.B, l.pj, l.slot, 0.5, runs, 0) == 2);
    CHECK(runs.size() == 2 && runs[0].n == 1 && runs[1].n == 1 && runs[1].x == 0.5);
  }
  unsigned seed = 12345;
  for (int it = 0; it < 2000; it++) {  // random lists against the point-by-point walk
    Lists l;
    const int na = rnd(seed) % 4, nb = rnd(seed) % 4;
    size_t p = 0;
    for (int k = 0; k < na; k++) {
      const size_t n = rnd(seed) % 9;
      l.A.push_back({p, n, double(rnd(seed) % 5) - 2.0});
      p += n;
    }
    for (int k = 0; k < nb; k++) {
      const size_t n = (k < na && rnd(seed) % 4) ? l.A[k].N : rnd(seed) % 9;
      l.B.push_back({p, n, 1.0});
      p += n;
    }
    int s = 0;
    for (size_t q = 0; q < p; q++) {
      s += 1 + (rnd(seed) % 8 == 0);  // mostly consecutive slots
      l.slot.push_back(s);
      const int mine = rnd(seed) % 6 ? 1 : -1;
      for (int e = 0; e < 3; e++) l.pj.push_back(mine);
    }
    const double x = it % 2 ? -1.0 : 0.5;
    std::vector<PairRun> runs;
    const long long start = it % 3;
    const long long n = pair_runs(l.A, l.B, l.pj, l.slot, x, runs, start);
    for (auto &r : runs) r.g0 -= start;
    const auto got = expand(runs), want = walk(l, x);
    CHECK(n - start == (long long)want.size());
    CHECK(got == want);
  }
  if (fails) return 1;
  printf("ok\n");
  return 0;
}
