// mnl_modes.hpp -- the mode table of a DiffractedPlanewave: what
// fields::get_eigenmode builds when dp != NULL (src/mpb.cpp:342-347, 619-664), without MPB.  Per
// (mode, frequency) the wavevector, the group velocity and the six plane-wave amplitudes, and
// the phase exp(2 pi i k.(x - centre)) split into separable tables: the in-plane part of k does
// not depend on the frequency, and a monitor plane has at most two layers along its normal.
// Plain C++ (no HIP, no project header): shared by mnl_modes.cpp and tests/cpu/mode_table_main.cpp.
#pragma once
#include <cmath>
#include <complex>
#include <string>
#include <vector>

namespace mnlmodes {

using cplx = std::complex<double>;
constexpr double pi = 3.141592653589793238462643383276;  // meep::pi

// diffractedplanewave (src/meep.hpp): the order g, the axis (all 0: the first direction lying in
// the plane of the monitor, python/simulation.py:180) and the s / p amplitudes
struct Mode {
  int g[3];
  double axis[3];
  cplx s, p;
};

struct Geometry {
  bool has[3] = {false, false, false};  // the cell's directions
  int ncell[3] = {1, 1, 1};             // user_volume.num_direction
  bool periodic[3] = {false, false, false};  // both faces of the direction are Periodic
  double bloch[3] = {0, 0, 0};          // real(fields::k[dd])
  double a = 1;                         // resolution
  int normal = 2;                       // eig_vol.normal_direction()
  double emin[3] = {0, 0, 0}, emax[3] = {0, 0, 0};  // the eigenmode volume
  double kpoint[3] = {0, 0, 0};         // the caller's kpoint
  double eps = 1, mu = 1;               // get_eps / get_mu at the centre of the eigenmode volume
  // the distinct integer (half-pixel) coordinates of the monitor's points along the in-plane
  // directions da < db (db = -1: the plane is a line) and along the normal (1 or 2 layers);
  // a position is coordinate * (0.5 * (1 / a)) (IVEC_LOOP_LOC)
  int da = 0, db = -1;
  std::vector<int> ca, cb;
  int nlayer = 1, layer[2] = {0, 0};
};

struct Table {
  int nmodes = 0, nfreq = 0, na = 0, nb = 0;
  std::vector<double> k;     // [mode][freq][3]; 0 where evanescent
  std::vector<int> evan;     // [mode][freq]
  std::vector<double> vgrp;  // [mode][freq]
  std::vector<cplx> amp;     // [mode][freq][6]: Ex Ey Ez Hx Hy Hz
  std::vector<cplx> pa, pb;  // [mode][na], [mode][nb]: exp(2 pi i k_d (x_d - centre_d))
  std::vector<cplx> pl;      // [mode][freq][2]: the same along the normal, per layer
};

inline void cross(const double a[3], const double b[3], double out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
inline double norm3(const double a[3]) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// exp(2 pi i k (x - centre)) in one fixed order of operations
inline cplx phase(double k, double x, double cen) { return std::polar(1.0, (2 * pi) * (k * (x - cen))); }

// 0, or -1 with err set
inline int build(const Geometry &G, const std::vector<Mode> &modes, const std::vector<double> &freqs,
                 Table &T, std::string &err) {
  const int nm = (int)modes.size(), nf = (int)freqs.size(), n = G.normal;
  T.nmodes = nm, T.nfreq = nf, T.na = (int)G.ca.size(), T.nb = G.db >= 0 ? (int)G.cb.size() : 1;
  T.k.assign((size_t)nm * nf * 3, 0.0);
  T.evan.assign((size_t)nm * nf, 0);
  T.vgrp.assign((size_t)nm * nf, 0.0);
  T.amp.assign((size_t)nm * nf * 6, cplx(0.0));
  T.pa.assign((size_t)nm * T.na, cplx(1.0));
  T.pb.assign((size_t)nm * T.nb, cplx(1.0));
  T.pl.assign((size_t)nm * nf * 2, cplx(1.0));
  const double h = 0.5 * (1.0 / G.a);
  double cen[3], ext[3];
  for (int d = 0; d < 3; d++) cen[d] = 0.5 * (G.emin[d] + G.emax[d]), ext[d] = G.emax[d] - G.emin[d];
  // src/mpb.cpp:342-347: where the eigenmode volume spans the cell between periodic faces, the
  // starting component is the real part of the Bloch vector (vol2d / vol3d round the extent)
  double kp[3];
  for (int d = 0; d < 3; d++) {
    kp[d] = G.kpoint[d];
    if (!G.has[d] || d == n) continue;
    const int num = ext[d] == 0 ? 1 : (int)(ext[d] * G.a + 0.5);
    if (num == G.ncell[d] && G.periodic[d]) kp[d] = G.bloch[d];
  }
  for (int m = 0; m < nm; m++) {
    const Mode &M = modes[m];
    // src/mpb.cpp:621-629: (kparallel + G) in every direction of non-zero extent
    double kin[3], k2sum = 0;
    for (int d = 0; d < 3; d++) {
      kin[d] = kp[d];
      if (!G.has[d] || ext[d] == 0) continue;
      const double ktmp = kp[d] + M.g[d] / ext[d];
      kin[d] = ktmp;
      k2sum += ktmp * ktmp;
    }
    for (int i = 0; i < T.na; i++) T.pa[(size_t)m * T.na + i] = phase(kin[G.da], G.ca[i] * h, cen[G.da]);
    if (G.db >= 0)
      for (int i = 0; i < T.nb; i++)
        T.pb[(size_t)m * T.nb + i] = phase(kin[G.db], G.cb[i] * h, cen[G.db]);
    double ax[3] = {M.axis[0], M.axis[1], M.axis[2]};
    if (ax[0] == 0 && ax[1] == 0 && ax[2] == 0) ax[G.da] = 1.0;
    for (int f = 0; f < nf; f++) {
      const size_t mf = (size_t)m * nf + f;
      const double fr = freqs[f];
      // src/mpb.cpp:650-660
      const double nn = sqrt(G.eps * G.mu);
      const double k2 = fr * fr * nn * nn - k2sum;
      if (k2 < 0) {
        T.evan[mf] = 1;
        for (int q = 0; q < 6; q++) T.amp[mf * 6 + q] = 0.0;
        continue;
      }
      double k[3] = {kin[0], kin[1], kin[2]};
      if (k2 > 0) k[n] = sqrt(k2);
      double axk[3], shat[3], khat[3], phat[3];
      cross(ax, k, axk);
      const double la = norm3(ax), lk = norm3(k), lx = norm3(axk);
      if (!(lx > ldexp(1.0, -40) * la * lk)) {
        err = "mode_coefficients: the axis of DiffractedPlanewave is parallel to the wavevector "
              "(mode " + std::to_string(m) + ", frequency " + std::to_string(f) + ")";
        return -1;
      }
      for (int d = 0; d < 3; d++) shat[d] = axk[d] / lx, khat[d] = k[d] / lk;
      cross(shat, khat, phat);
      cplx E0[3], H0[3];
      for (int d = 0; d < 3; d++) E0[d] = M.s * shat[d] + M.p * phat[d];
      const double fm = fr * G.mu;
      H0[0] = (k[1] * E0[2] - k[2] * E0[1]) / fm;
      H0[1] = (k[2] * E0[0] - k[0] * E0[2]) / fm;
      H0[2] = (k[0] * E0[1] - k[1] * E0[0]) / fm;
      for (int d = 0; d < 3; d++) {
        T.k[mf * 3 + d] = k[d];
        T.amp[mf * 6 + d] = E0[d];
        T.amp[mf * 6 + 3 + d] = H0[d];
      }
      T.vgrp[mf] = k[n] / (fr * G.eps * G.mu);
      for (int l = 0; l < G.nlayer; l++) T.pl[mf * 2 + l] = phase(k[n], G.layer[l] * h, cen[n]);
    }
  }
  return 0;
}

}  // namespace mnlmodes
