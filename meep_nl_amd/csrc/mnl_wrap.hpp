// mnl_wrap.hpp -- the thread table of the periodic ghost wrap.  Plain
// C++ with no device or runtime types, shared by the wrap kernel (mnl_kernels_io.hip), the
// host (mnl_step.cpp) and a stand-alone host program (tests/cpu/wrap_table_main.cpp).
//
// A direction with periodic boundaries (fields::use_bloch with k = 0) has, per component, one
// not-owned plane: plane 0 of a component unshifted along it (a copy of plane n) and plane n of
// a component shifted along it (a copy of plane 0); connect_the_chunks (src/boundaries.cpp:
// 347-623) connects each not-owned point to the owned point one lattice vector away.  A point
// that is not owned along several periodic axes maps along all of them at once, so its source
// is always an owned point and no thread reads what another thread of the launch writes.
#pragma once

#if defined(__HIPCC__)
#define MNL_HD __host__ __device__
#else
#define MNL_HD
#endif

namespace mnl {

constexpr int WRAP_MAXA = 40;  // arrays per launch (E, f_w, B, H, D and every P at most)

struct WrapArr {
  double *p;
  int sh;  // bit a: the component is shifted along device axis a
};

struct WrapArgs {
  int n;                  // arrays
  WrapArr a[WRAP_MAXA];
  int N[3];               // points per device axis
  long long st[3];        // strides per device axis (st[0] = 1)
  int per[3];             // device axis is periodic
  // threads of one array: the face of axis 0 (one thread per ghost point: one 8-byte element
  // per row), then the faces of axes 1 and 2 (one thread per pair of adjacent points of a row,
  // which move as one 16-byte access where neither is a ghost of axis 0)
  long long fstart[4];
};

// fills N / st / per dependent thread ranges; returns the threads of one array
MNL_HD inline long long wrap_plan(WrapArgs &w) {
  const long long half = (w.N[0] + 1) / 2;
  const long long cnt[3] = {w.per[0] ? (long long)w.N[1] * w.N[2] : 0,
                            w.per[1] ? half * w.N[2] : 0, w.per[2] ? half * w.N[1] : 0};
  w.fstart[0] = 0;
  for (int a = 0; a < 3; a++) w.fstart[a + 1] = w.fstart[a] + cnt[a];
  return w.fstart[3];
}

// the not-owned index of a component along a periodic axis, and the index it copies
MNL_HD inline int wrap_ghost(const WrapArgs &w, int sh, int a) { return ((sh >> a) & 1) ? w.N[a] - 1 : 0; }
MNL_HD inline int wrap_owner(const WrapArgs &w, int sh, int a) { return ((sh >> a) & 1) ? 0 : w.N[a] - 1; }

// Thread t of the launch: its array and up to two (destination, source) linear indices.
// Returns the number of points (0: nothing to do).
MNL_HD inline int wrap_points(const WrapArgs &w, long long t, int &arr, long long dst[2],
                              long long src[2]) {
  const long long per_arr = w.fstart[3];
  arr = (int)(t / per_arr);
  if (arr >= w.n) return 0;
  const long long r = t % per_arr;
  const int sh = w.a[arr].sh;
  int face = 0;
  while (face < 2 && r >= w.fstart[face + 1]) face++;
  const long long l = r - w.fstart[face];
  int i[3], nx = 1;
  if (face == 0) {
    i[0] = wrap_ghost(w, sh, 0);
    i[1] = (int)(l % w.N[1]);
    i[2] = (int)(l / w.N[1]);
  } else {
    const long long half = (w.N[0] + 1) / 2;
    i[0] = 2 * (int)(l % half);
    const int o = (int)(l / half);
    i[1] = face == 1 ? wrap_ghost(w, sh, 1) : o;
    i[2] = face == 1 ? o : wrap_ghost(w, sh, 2);
    nx = i[0] + 1 < w.N[0] ? 2 : 1;
  }
  int np = 0;
  for (int k = 0; k < nx; k++) {
    const int j[3] = {i[0] + k, i[1], i[2]};
    // a ghost of a lower periodic axis belongs to that axis' face
    bool lower = false;
    for (int a = 0; a < face; a++) lower = lower || (w.per[a] && j[a] == wrap_ghost(w, sh, a));
    if (lower) continue;
    long long d = 0, s = 0;
    for (int a = 0; a < 3; a++) {
      const bool gh = w.per[a] && j[a] == wrap_ghost(w, sh, a);
      d += j[a] * w.st[a];
      s += (gh ? wrap_owner(w, sh, a) : j[a]) * w.st[a];
    }
    dst[np] = d, src[np] = s;
    np++;
  }
  return np;
}

// Complex fields: the same threads over pairs of arrays (part 0, part 1)
// with the Bloch phase of every ghost point.  ph: the host's table (mnl_bloch.hpp), indexed by
// {none, low, high} per device axis.
struct WrapPhaseArgs {
  WrapArgs w;               // w.a[k].p: part 0
  double *q[WRAP_MAXA];     // part 1
  double ph[27][2];
};

// One ghost value: the phase classified as connect_the_chunks does (src/boundaries.cpp:402-404)
// -- exactly 1 is a copy, exactly -1 a negation, anything else the complex product of
// fields::process_incoming_chunk_data (src/step.cpp:188-193), two roundings per part (both
// compilers build this without contraction).
MNL_HD inline void wrap_phase_apply(const double ph[2], double vr, double vi, double &re,
                                    double &im) {
  const double pr = ph[0], pi = ph[1];
  if (pr == 1.0 && pi == 0.0) {
    re = vr, im = vi;
  } else if (pr == -1.0 && pi == 0.0) {
    re = -vr, im = -vi;
  } else {
    re = pr * vr - pi * vi;
    im = pr * vi + pi * vr;
  }
}

// the phase-table index of destination point dst of an array with shift mask sh: along every
// periodic axis on whose not-owned plane it lies, 1 (plane 0, brought in from below) or 2
// (plane n, from above)
MNL_HD inline int wrap_phase_index(const WrapArgs &w, int sh, long long dst) {
  const int j[3] = {(int)(dst % w.st[1]), (int)((dst % w.st[2]) / w.st[1]), (int)(dst / w.st[2])};
  int idx = 0, m = 1;
  for (int a = 0; a < 3; a++, m *= 3)
    if (w.per[a] && j[a] == wrap_ghost(w, sh, a)) idx += m * (((sh >> a) & 1) ? 2 : 1);
  return idx;
}

}  // namespace mnl
