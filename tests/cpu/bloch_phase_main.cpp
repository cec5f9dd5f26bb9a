// Stand-alone check of the Bloch-phase wrap's host code (meep_nl_amd/csrc/mnl_bloch.hpp and the
// phase part of mnl_wrap.hpp), built with the address and undefined-behaviour sanitizers by
// tests/test_bloch_cpu.py.
//
//   bloch_phase_main                      self-test: for every grid shape, set of periodic axes
//                                         and shift mask the phased wrap's body runs on the host,
//                                         thread by thread, over pairs of arrays with guard
//                                         zones; every ghost point of both parts must be the
//                                         owning point times the table's phase (copy / negate /
//                                         product), written once, nothing else touched
//   bloch_phase_main table n0 n1 n2 a kr0 ki0 kr1 ki1 kr2 ki2
//                                         prints eikna of the three directions (n cells, a
//                                         pixels per unit length, k complex) and the 27 table
//                                         entries for device axes = directions, as hexadecimal
//                                         floats (exact), for the NumPy restatement to compare
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mnl_bloch.hpp"
#include "mnl_wrap.hpp"

using namespace mnl;
typedef std::complex<double> cplx;

static int fails = 0;
#define CHECK(c)                                             \
  do {                                                       \
    if (!(c)) {                                              \
      if (fails++ < 10) printf("line %d: %s\n", __LINE__, #c); \
    }                                                        \
  } while (0)

static bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }

static long long lin(const WrapArgs &w, int i0, int i1, int i2) {
  return i0 * w.st[0] + i1 * w.st[1] + i2 * w.st[2];
}

static void run(int N0, int N1, int N2, int permask, int narr, const cplx eikna[3]) {
  WrapPhaseArgs A{};
  WrapArgs &w = A.w;
  w.N[0] = N0, w.N[1] = N1, w.N[2] = N2;
  const long long p0 = (N1 == 1 && N2 == 1) ? N0 : (N0 + 15) / 16 * 16;
  w.st[0] = 1, w.st[1] = p0, w.st[2] = p0 * N1;
  for (int a = 0; a < 3; a++) w.per[a] = (permask >> a) & 1;
  const int dir_of_axis[3] = {0, 1, N2 > 1 ? 2 : -1};
  bloch_phase_table(eikna, dir_of_axis, A.ph);
  const size_t nloc = (size_t)(p0 * N1 * N2), guard = 64;
  std::vector<std::vector<double>> re(narr, std::vector<double>(nloc + 2 * guard, -7.0)), im = re;
  w.n = narr;
  for (int k = 0; k < narr; k++) {
    w.a[k].p = re[k].data() + guard;
    A.q[k] = im[k].data() + guard;
    w.a[k].sh = (k * 3 + permask) & 7;
    for (int i2 = 0; i2 < N2; i2++)
      for (int i1 = 0; i1 < N1; i1++)
        for (int i0 = 0; i0 < N0; i0++) {
          const double v = 1000.0 * k + i0 + 37.0 * i1 + 1511.0 * i2;
          // a zero among the values: a copy and a negation keep and flip its sign
          w.a[k].p[lin(w, i0, i1, i2)] = (i0 + i1 + i2) % 5 == 0 ? 0.0 : v + 0.25;
          A.q[k][lin(w, i0, i1, i2)] = (i0 + i1 + i2) % 7 == 0 ? -0.0 : -0.5 * v - 0.125;
        }
  }
  const long long per_arr = wrap_plan(w);
  const std::vector<std::vector<double>> re0 = re, im0 = im;
  std::vector<std::vector<int>> written(narr, std::vector<int>(nloc, 0));
  const long long total = per_arr * narr;
  for (long long t = 0; t < total + 3; t++) {
    int arr = -1;
    long long dst[2], src[2];
    const int np = wrap_points(w, t, arr, dst, src);
    if (t >= total) {
      CHECK(np == 0);
      continue;
    }
    for (int k = 0; k < np; k++) {
      const bool ok = arr >= 0 && arr < narr && dst[k] >= 0 && (size_t)dst[k] < nloc &&
                      src[k] >= 0 && (size_t)src[k] < nloc;
      CHECK(ok);
      if (!ok) continue;
      const int pi = wrap_phase_index(w, w.a[arr].sh, dst[k]);
      CHECK(pi > 0 && pi < 27);
      if (!(pi > 0 && pi < 27)) continue;
      written[arr][dst[k]]++;
      // sources are read from the state before the launch
      wrap_phase_apply(A.ph[pi], re0[arr][guard + src[k]], im0[arr][guard + src[k]],
                       w.a[arr].p[dst[k]], A.q[arr][dst[k]]);
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
          cplx ph = 1.0;  // locate_point_in_user_volume: directions in order
          for (int a = 0; a < 3; a++) {
            const int shifted = (sh >> a) & 1;
            const bool g = w.per[a] && j[a] == (shifted ? w.N[a] - 1 : 0);
            s[a] = g ? (shifted ? 0 : w.N[a] - 1) : j[a];
            if (g) ph *= shifted ? eikna[a] : conj(eikna[a]);
            ghost = ghost || g;
          }
          const long long i = lin(w, i0, i1, i2), o = lin(w, s[0], s[1], s[2]);
          CHECK(written[k][i] == (ghost ? 1 : 0));
          const double vr = re0[k][guard + o], vi = im0[k][guard + o];
          double wr = vr, wi = vi;
          if (ghost) {
            if (ph == 1.0) {
            } else if (ph == -1.0) {
              wr = -vr, wi = -vi;
            } else {
              const cplx t = ph * cplx(vr, vi);  // process_incoming_chunk_data
              wr = real(t), wi = imag(t);
            }
          }
          CHECK(same_bits(w.a[k].p[i], wr) && same_bits(A.q[k][i], wi));
        }
    for (size_t q = 0; q < guard; q++)
      CHECK(re[k][q] == -7.0 && re[k][guard + nloc + q] == -7.0 && im[k][q] == -7.0 &&
            im[k][guard + nloc + q] == -7.0);
  }
}

static int print_table(char **v) {
  const int n[3] = {atoi(v[0]), atoi(v[1]), atoi(v[2])};
  const double a = atof(v[3]);
  cplx eikna[3];
  for (int d = 0; d < 3; d++) {
    eikna[d] = bloch_eikna(cplx(strtod(v[4 + 2 * d], nullptr), strtod(v[5 + 2 * d], nullptr)), n[d], a);
    printf("eikna %d %a %a\n", d, real(eikna[d]), imag(eikna[d]));
  }
  const int dir_of_axis[3] = {0, 1, 2};
  double tab[27][2];
  bloch_phase_table(eikna, dir_of_axis, tab);
  for (int i = 0; i < 27; i++) printf("ph %d %a %a\n", i, tab[i][0], tab[i][1]);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 12 && !strcmp(argv[1], "table")) return print_table(argv + 2);
  const int shapes[][3] = {{2, 2, 2}, {3, 2, 4}, {17, 5, 3}, {16, 4, 1}, {21, 19, 1}, {33, 7, 6}};
  // k = 0; the zone edge (every phase +-1); a generic real k; a complex k
  const cplx ks[][3] = {{0.0, 0.0, 0.0},
                        {bloch_eikna(0.25, 16, 8.0), bloch_eikna(0.5, 8, 8.0), bloch_eikna(1.0, 4, 8.0)},
                        {bloch_eikna(0.1, 16, 8.0), bloch_eikna(0.2, 8, 8.0), bloch_eikna(-0.3, 4, 8.0)},
                        {bloch_eikna(cplx(0.1, 0.02), 16, 8.0), bloch_eikna(cplx(0.0, -0.01), 8, 8.0),
                         bloch_eikna(cplx(0.25, 0.01), 16, 8.0)}};
  for (int q = 0; q < 4; q++) {
    cplx e[3];
    for (int d = 0; d < 3; d++) e[d] = q == 0 ? cplx(1.0) : ks[q][d];
    if (q == 1)
      for (int d = 0; d < 3; d++) CHECK(real(e[d]) == -1.0 && imag(e[d]) == 0.0);
    for (auto &s : shapes)
      for (int pm = 1; pm < 8; pm++) {
        if (s[2] == 1 && (pm & 4)) continue;
        run(s[0], s[1], s[2], pm, 9, e);
      }
  }
  if (fails) {
    printf("%d checks failed\n", fails);
    return 1;
  }
  printf("ok\n");
  return 0;
}
