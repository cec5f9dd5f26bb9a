// mnl_bloch.hpp -- the Bloch phases of the periodic ghost wrap with k != 0 (DESIGN.md section
// 33).  Plain C++ with no device or runtime types, shared by the host (mnl_host.cpp,
// mnl_step.cpp) and a stand-alone host program (tests/cpu/bloch_phase_main.cpp).
//
// fields::use_bloch (src/boundaries.cpp:88-99) keeps eikna[d] = exp(i k_d (2 pi / a) n_d) per
// periodic direction, with the zone edge real(k_d) n_d == a / 2 checked exactly (then
// -exp(-imag(k_d) (2 pi / a) n_d): exactly -1 for a real k).  A not-owned point is brought into
// the cell by locate_point_in_user_volume (src/boundaries.cpp:201-224): directions in loop
// order, the phase multiplied by conj(eikna[d]) for a point brought in from below (plane 0 of
// a component unshifted along d) and by eikna[d] from above (plane n of a shifted one).  The
// wrap maps a ghost point along all of its periodic axes at once (mnl_wrap.hpp), so its phase
// is one of at most 27 such products, indexed by {none, low, high} per device axis.
#pragma once
#include <complex>

namespace mnl {

constexpr double BLOCH_PI = 3.141592653589793238462643383276;  // meep::pi

// eikna of one direction: k in units of 2 pi / length, n cells, a pixels per unit length
inline std::complex<double> bloch_eikna(std::complex<double> k, int n, double a) {
  if (real(k) * n == 0.5 * a)  // check b.z. edge exactly
    return -exp(-imag(k) * ((2 * BLOCH_PI / a) * n));
  const std::complex<double> I(0.0, 1.0);
  return exp(I * k * ((2 * BLOCH_PI / a) * n));
}

enum { BLOCH_NONE = 0, BLOCH_LOW = 1, BLOCH_HIGH = 2 };

// index of a ghost point's phase: s[a] in {BLOCH_NONE, BLOCH_LOW, BLOCH_HIGH} per device axis
inline int bloch_index(int s0, int s1, int s2) { return s0 + 3 * (s1 + 3 * s2); }

// tab[bloch_index(...)] = (re, im).  dir_of_axis[a]: the direction X, Y, Z of device axis a
// (-1: absent); the product runs over the directions in loop order (X, Y, Z), which is the
// order of the device axes; eikna[d] of a direction that is not periodic is never used
// (its points are no ghosts: index BLOCH_NONE only).
inline void bloch_phase_table(const std::complex<double> eikna[3], const int dir_of_axis[3],
                              double tab[27][2]) {
  for (int s2 = 0; s2 < 3; s2++)
    for (int s1 = 0; s1 < 3; s1++)
      for (int s0 = 0; s0 < 3; s0++) {
        const int s[3] = {s0, s1, s2};
        std::complex<double> ph = 1.0;
        for (int d = 0; d < 3; d++)      // LOOP_OVER_DIRECTIONS
          for (int a = 0; a < 3; a++) {
            if (dir_of_axis[a] != d || s[a] == BLOCH_NONE) continue;
            if (s[a] == BLOCH_LOW)
              ph *= conj(eikna[d]);
            else
              ph *= eikna[d];
          }
        tab[bloch_index(s0, s1, s2)][0] = real(ph);
        tab[bloch_index(s0, s1, s2)][1] = imag(ph);
      }
}

}  // namespace mnl
