// Stand-alone driver of the mode table (meep_nl_amd/csrc/mnl_modes.hpp) for
// tests/test_mode_coeff_cpu.py: builds the table of a fixed list of cases and prints the inputs
// and the table, every double as a hex float.  Built with -fsanitize=address,undefined.
#include <cstdio>

#include "mnl_modes.hpp"

using namespace mnlmodes;

static void hx(double v) { printf(" %a", v); }
static void hc(const cplx &v) { printf(" %a %a", v.real(), v.imag()); }

static int run(const char *name, const Geometry &G, const std::vector<Mode> &modes,
               const std::vector<double> &freqs, bool expect_error = false) {
  Table T;
  std::string err;
  const int rc = build(G, modes, freqs, T, err);
  if (expect_error) {
    if (rc == 0) {
      fprintf(stderr, "%s: no error\n", name);
      return 1;
    }
    printf("error %s | %s\n", name, err.c_str());
    return 0;
  }
  if (rc) {
    fprintf(stderr, "%s: %s\n", name, err.c_str());
    return 1;
  }
  printf("case %s\n", name);
  printf("geom %d %d %d %d %d %d %d %d %d", (int)G.has[0], (int)G.has[1], (int)G.has[2], G.ncell[0],
         G.ncell[1], G.ncell[2], (int)G.periodic[0], (int)G.periodic[1], (int)G.periodic[2]);
  printf(" %d %d %d %d %d %d", G.normal, G.da, G.db, G.nlayer, G.layer[0], G.layer[1]);
  for (int d = 0; d < 3; d++) hx(G.bloch[d]);
  hx(G.a);
  for (int d = 0; d < 3; d++) hx(G.emin[d]);
  for (int d = 0; d < 3; d++) hx(G.emax[d]);
  for (int d = 0; d < 3; d++) hx(G.kpoint[d]);
  hx(G.eps), hx(G.mu);
  printf("\nca");
  for (int c : G.ca) printf(" %d", c);
  printf("\ncb");
  for (int c : G.cb) printf(" %d", c);
  printf("\nfreqs");
  for (double f : freqs) hx(f);
  printf("\n");
  const int nm = T.nmodes, nf = T.nfreq;
  for (int m = 0; m < nm; m++) {
    const Mode &M = modes[m];
    printf("mode %d %d %d %d", m, M.g[0], M.g[1], M.g[2]);
    for (int d = 0; d < 3; d++) hx(M.axis[d]);
    hc(M.s), hc(M.p);
    printf("\npa %d", m);
    for (int i = 0; i < T.na; i++) hc(T.pa[(size_t)m * T.na + i]);
    printf("\npb %d", m);
    for (int i = 0; i < T.nb; i++) hc(T.pb[(size_t)m * T.nb + i]);
    printf("\n");
    for (int f = 0; f < nf; f++) {
      const size_t mf = (size_t)m * nf + f;
      printf("k %d %d %d", m, f, T.evan[mf]);
      for (int d = 0; d < 3; d++) hx(T.k[mf * 3 + d]);
      hx(T.vgrp[mf]);
      printf("\namp %d %d", m, f);
      for (int q = 0; q < 6; q++) hc(T.amp[mf * 6 + q]);
      printf("\npl %d %d", m, f);
      hc(T.pl[mf * 2]), hc(T.pl[mf * 2 + 1]);
      printf("\n");
    }
  }
  return 0;
}

static std::vector<int> span(int lo, int hi) {
  std::vector<int> v;
  for (int c = lo; c <= hi; c += 2) v.push_back(c);
  return v;
}

int main() {
  int bad = 0;
  // a 2 x 2 x 3 cell at resolution 8, periodic in x and y; a full-period plane at z = 0.5625
  Geometry Z;
  for (int d = 0; d < 3; d++) Z.has[d] = true;
  Z.ncell[0] = 16, Z.ncell[1] = 16, Z.ncell[2] = 24;
  Z.periodic[0] = Z.periodic[1] = true;
  Z.a = 8, Z.normal = 2, Z.da = 0, Z.db = 1;
  Z.emin[0] = -1, Z.emax[0] = 1, Z.emin[1] = -1, Z.emax[1] = 1, Z.emin[2] = Z.emax[2] = 0.5625;
  Z.ca = span(-15, 15), Z.cb = span(-15, 15);
  Z.nlayer = 1, Z.layer[0] = 9;
  const Mode s00{{0, 0, 0}, {0, 0, 0}, 1.0, 0.0}, p00{{0, 0, 0}, {0, 0, 0}, 0.0, 1.0};
  bad += run("normal_incidence", Z, {s00, p00}, {0.5, 1.0});
  // order (1, 0): kx = 0.5; evanescent at 0.4, k2 == 0 at 0.5, propagating at 0.75
  const Mode s10{{1, 0, 0}, {0, 0, 0}, 1.0, 0.0}, m11{{-1, 1, 0}, {0.0, 1.0, 0.0}, cplx(0.3, -0.7), cplx(0.2, 0.4)};
  bad += run("evanescent_to_propagating", Z, {s10, m11}, {0.4, 0.75, 1.25});
  Geometry Zk = Z;
  Zk.kpoint[2] = 0.125;
  bad += run("k2_zero", Zk, {s10}, {0.5});
  // a Bloch k in x (periodic, spanned) but not in y (spanned, not periodic: the caller's kpoint)
  Geometry B = Z;
  B.periodic[1] = false;
  B.bloch[0] = 0.1, B.bloch[1] = 0.07, B.kpoint[1] = 0.05, B.kpoint[0] = 0.3;
  B.eps = 2.25;
  bad += run("bloch", B, {s00, m11}, {0.9, 1.1});
  // an eigenmode volume shorter than the period takes the caller's kpoint
  Geometry Bs = B;
  Bs.emin[0] = -0.5, Bs.emax[0] = 0.5;
  bad += run("bloch_short_volume", Bs, {s10}, {1.1});
  // coordinates of image chunks beyond the periodic faces, and two layers
  Geometry I = Z;
  I.bloch[0] = 0.1;
  I.ca = span(-19, 19);
  I.emin[2] = I.emax[2] = 0.59375;
  I.nlayer = 2, I.layer[0] = 9, I.layer[1] = 11;
  bad += run("image_coordinates", I, {m11}, {1.0});
  // the other normals
  Geometry X = Z;
  X.normal = 0, X.da = 1, X.db = 2;
  X.ncell[0] = 24, X.ncell[2] = 16, X.periodic[0] = false, X.periodic[2] = true;
  X.emin[0] = X.emax[0] = 0.5625, X.emin[2] = -1, X.emax[2] = 1;
  bad += run("normal_x", X, {s00, p00, m11, Mode{{0, 1, -1}, {0.3, 0.2, -0.5}, 0.5, cplx(0, 1)}},
             {0.8, 1.0});
  Geometry Y = Z;
  Y.normal = 1, Y.da = 0, Y.db = 2;
  Y.ncell[1] = 24, Y.ncell[2] = 16, Y.periodic[1] = false, Y.periodic[2] = true;
  Y.emin[1] = Y.emax[1] = -0.4375, Y.emin[2] = -1, Y.emax[2] = 1;
  Y.layer[0] = -7;
  Y.mu = 1.5;
  bad += run("normal_y", Y, {s00, p00, Mode{{1, 0, 1}, {0, 0, 0}, cplx(1, 1), 0.25}}, {0.9, 1.3});
  // a 2-D cell: the plane is a line along x, its normal y
  Geometry D;
  D.has[0] = D.has[1] = true;
  D.ncell[0] = 32, D.ncell[1] = 48;
  D.periodic[0] = true;
  D.bloch[0] = 0.1;
  D.a = 16, D.normal = 1, D.da = 0, D.db = -1;
  D.emin[0] = -1, D.emax[0] = 1, D.emin[1] = D.emax[1] = 0.53125;
  D.ca = span(-35, 35);
  D.nlayer = 1, D.layer[0] = 17;
  bad += run("two_d", D, {s00, p00, Mode{{1, 0, 0}, {0, 0, 0}, 0.6, 0.8}, Mode{{-1, 0, 0}, {0, 0, 0}, 0.0, 1.0}},
             {0.8, 1.2});
  // the axis along the wavevector is an error
  bad += run("axis_parallel", Z, {Mode{{0, 0, 0}, {0, 0, 2.0}, 1.0, 0.0}}, {1.0}, true);
  return bad ? 1 : 0;
}
