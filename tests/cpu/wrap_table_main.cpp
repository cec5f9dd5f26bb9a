// Stand-alone check of the periodic wrap's thread table (meep_nl_amd/csrc/mnl_wrap.hpp), built
// with the address and undefined-behaviour sanitizers by tests/test_periodic_cpu.py.  For every
// grid shape, set of periodic axes and shift mask it runs the kernel's body on the host, thread
// by thread, into arrays with guard zones and checks that
//   - every ghost point is written exactly once and nothing else is written,
//   - every source is an owned point inside the array (no thread reads what another writes),
//   - the value is the owning point's: every periodic axis mapped at once (index mod period).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mnl_wrap.hpp"

using namespace mnl;

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      if (fails++ < 10) printf("line %d: %s\n", __LINE__, #c); \
    }                                                        \
  } while (0)

static long long lin(const WrapArgs &w, int i0, int i1, int i2) {
  return i0 * w.st[0] + i1 * w.st[1] + i2 * w.st[2];
}

static void run(int N0, int N1, int N2, int permask, int narr) {
  WrapArgs w{};
  w.N[0] = N0, w.N[1] = N1, w.N[2] = N2;
  const long long p0 = (N1 == 1 && N2 == 1) ? N0 : (N0 + 15) / 16 * 16;  // rows padded as the grid's
  w.st[0] = 1, w.st[1] = p0, w.st[2] = p0 * N1;
  for (int a = 0; a < 3; a++) w.per[a] = (permask >> a) & 1;
  const size_t nloc = (size_t)(p0 * N1 * N2);
  const size_t guard = 64;
  std::vector<std::vector<double>> buf(narr, std::vector<double>(nloc + 2 * guard, -7.0));
  w.n = narr;
  for (int k = 0; k < narr; k++) {
    w.a[k].p = buf[k].data() + guard;
    w.a[k].sh = (k * 3 + permask) & 7;  // every shift mask appears over the arrays
    for (int i2 = 0; i2 < N2; i2++)
      for (int i1 = 0; i1 < N1; i1++)
        for (int i0 = 0; i0 < N0; i0++)
          w.a[k].p[lin(w, i0, i1, i2)] = 1000.0 * k + i0 + 37.0 * i1 + 1511.0 * i2;
  }
  const long long per_arr = wrap_plan(w);
  CHECK(per_arr == w.fstart[3]);
  std::vector<std::vector<int>> written(narr, std::vector<int>(nloc, 0));
  std::vector<std::vector<double>> before = buf;
  const long long total = per_arr * narr;
  for (long long t = 0; t < total + 3; t++) {  // a few threads past the end, as a ragged grid has
    int arr = -1;
    long long dst[2], src[2];
    const int np = wrap_points(w, t, arr, dst, src);
    if (t >= total) {
      CHECK(np == 0);
      continue;
    }
    for (int k = 0; k < np; k++) {
      CHECK(arr >= 0 && arr < narr);
      CHECK(dst[k] >= 0 && (size_t)dst[k] < nloc && src[k] >= 0 && (size_t)src[k] < nloc);
      if (!(arr >= 0 && arr < narr && dst[k] >= 0 && (size_t)dst[k] < nloc && src[k] >= 0 &&
            (size_t)src[k] < nloc))
        continue;
      written[arr][dst[k]]++;
      // the source is read from the state before the launch: it must not be a destination
      w.a[arr].p[dst[k]] = before[arr][guard + src[k]];
    }
  }
  for (int k = 0; k < narr; k++) {
    const int sh = w.a[k].sh;
    for (int i2 = 0; i2 < N2; i2++)
      for (int i1 = 0; i1 < N1; i1++)
        for (int i0 = 0; i0 < N0; i0++) {
          const int j[3] = {i0, i1, i2};
          int s[3];
          bool ghost = false;
          for (int a = 0; a < 3; a++) {
            const bool g = w.per[a] && j[a] == (((sh >> a) & 1) ? w.N[a] - 1 : 0);
            // index mod period: a shifted component's plane n is plane 0, an unshifted
            // component's plane 0 is plane n
            s[a] = g ? (((sh >> a) & 1) ? 0 : w.N[a] - 1) : j[a];
            ghost = ghost || g;
          }
          const long long i = lin(w, i0, i1, i2);
          CHECK(written[k][i] == (ghost ? 1 : 0));
          const double want = 1000.0 * k + s[0] + 37.0 * s[1] + 1511.0 * s[2];
          CHECK(w.a[k].p[i] == want);
        }
    // sources are never destinations
    for (long long t = 0; t < per_arr; t++) {
      int arr;
      long long dst[2], src[2];
      const int np = wrap_points(w, t + k * per_arr, arr, dst, src);
      for (int q = 0; q < np; q++) CHECK(written[k][src[q]] == 0);
    }
    // padding and guard zones untouched
    for (size_t q = 0; q < guard; q++) CHECK(buf[k][q] == -7.0 && buf[k][guard + nloc + q] == -7.0);
  }
}

int main() {
  const int shapes[][3] = {{2, 2, 2}, {3, 2, 4}, {17, 5, 3}, {16, 4, 1}, {21, 19, 1},
                           {33, 7, 6}, {8, 3, 9}};
  for (auto &s : shapes)
    for (int pm = 1; pm < 8; pm++) {
      if (s[2] == 1 && (pm & 4)) continue;  // a 2-D grid has no third axis to wrap
      run(s[0], s[1], s[2], pm, 9);
    }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
