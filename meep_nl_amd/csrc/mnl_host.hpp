// mnl_host.hpp -- the host side's shared internals: source times, the structure and fields
// objects, allocation, buffer sets, phase timing, and what each host source file (mnl_host.cpp
// lists them) offers the others.
// Internal to libmnl.so (not installed; the API is include/meep_nl_amd.h).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <set>
#include <unordered_set>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/meep_nl_amd.h"
#include "mnl_bloch.hpp"
#include "mnl_comm.hpp"
#include "mnl_internal.hpp"

using namespace mnl;
typedef std::complex<double> cplx;

namespace mnlh {
constexpr int TB_RES_CUS = 8;  // multi-rank: CUs left to the slab-face work (one per XCD)
constexpr int NAN_CH = 256;     // steps per chunk of a batch: the NaN flag is read after each

// phase timers (mnl_fields::timer_ms / timer_count, filled by PhaseTimer)
enum {
  TM_B = 0, TM_H, TM_D, TM_E, TM_SRC, TM_HALO, TM_BINT, TM_DINT, TM_GEN, TM_DFT, TM_DFTF,
  TM_TB,   // two-step kernel (temporal blocking), one launch per pair of steps
  TM_RIM,  // rim launches of the pairs (two per pair)
  TM_CHAIN,  // multi-rank pairs: a slab-face chain on the comm stream (two per pair)
  TM_WAIT,   // multi-rank pairs: the main stream waiting for the chain's E ghost (two per pair)
  TM_N
};
constexpr int TM_CAP = 16;  // length of timer_ms / timer_count
static_assert(TM_N <= TM_CAP, "a phase timer without a slot");

constexpr double pi = 3.141592653589793238462643383276;  // meep::pi
extern thread_local std::string g_err;

extern int g_verbosity;  // meep::verbosity (src/meep.hpp: default 1)

inline int fail(const std::string &m) {
  g_err = "meep: " + m;
  return -1;
}
#define HIPCHK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess)                                                         \
      return fail(std::string("HIP error ") + hipGetErrorString(e_) + " at " #x); \
  } while (0)

// on a declaration shared between the host files: not exported from libmnl.so
#define MNL_HIDDEN __attribute__((visibility("hidden")))

inline int cdir(int c) { return c % 3; }
inline int ctype(int c) { return c / 3; }

// ------------------------------------------------------------- source time
// gaussian_src_time / continuous_src_time (src/sources.cpp:85-141,
// src/meep.hpp:937-1056).
struct SrcTime {
  int kind = 0;
  bool is_integrated = false;
  double freq = 0, width = 0, peak_time = 0, cutoff = 0;
  cplx cfreq;
  double cwidth = 0, start_time = 0, end_time = 0, slowness = 3;
  double cur_time = NAN;
  cplx cur_dipole, cur_current;
  mnl_src_func func = nullptr;  // kind 2: custom_src_time (src/meep.hpp:1059-1092)
  void *fdata = nullptr;

  cplx dipole(double time) const {
    if (kind == 2) {
      const float rtime = float(time);
      if (!(rtime >= start_time && rtime <= end_time)) return 0.0;
      double re = 0, im = 0;
      func(time, fdata, &re, &im);
      return cplx(re, im);
    }
    if (kind == 0) {
      double tt = time - peak_time;
      if (float(fabs(tt)) > cutoff) return 0.0;
      cplx amp = 1.0 / cplx(0, -2 * pi * freq);
      return exp(-tt * tt / (2 * width * width)) * std::polar(1.0, -2 * pi * freq * tt) * amp;
    }
    float rtime = float(time);
    if (rtime < start_time || rtime > end_time) return 0.0;
    cplx amp = 1.0 / (cplx(0, -1.0) * (2 * pi) * cfreq);
    if (cwidth == 0.0) return exp(cplx(0, -1.0) * (2 * pi) * cfreq * time) * amp;
    double ts = (time - start_time) / cwidth - slowness;
    double te = (end_time - time) / cwidth - slowness;
    return exp(cplx(0, -1.0) * (2 * pi) * cfreq * time) * amp * (1.0 + tanh(ts)) *
           (1.0 + tanh(te)) * 0.25;
  }
  void update(double time, double dt) {  // src_time::update, src/meep.hpp:972-978
    if (time != cur_time) {
      cur_dipole = dipole(time);
      // custom_src_time::current: the dipole itself unless integrated
      cur_current = (kind == 2 && !is_integrated) ? dipole(time)
                                                 : (dipole(time + dt) - dipole(time)) / dt;
      cur_time = time;
    }
  }
  bool same(const SrcTime &o) const {
    return kind == o.kind && is_integrated == o.is_integrated && freq == o.freq &&
           width == o.width && peak_time == o.peak_time && cutoff == o.cutoff &&
           cfreq == o.cfreq && cwidth == o.cwidth && start_time == o.start_time &&
           end_time == o.end_time && slowness == o.slowness && func == o.func && fdata == o.fdata;
  }
};

struct SrcGroup {  // src_vol (src/meep_internals.hpp:49-82) over the whole cell
  int comp;        // E or H component
  int st;
  std::vector<long long> gidx;  // global canonical index of comp
  std::vector<int> chunk;       // the reference chunk that holds the point (its src_vol's chunk)
  std::vector<int> jglob;       // 3 global indices per point
  std::vector<cplx> amp;
};

struct Lorentz {
  double omega0, gamma;
  int drude;
  std::vector<double> sigma[3];  // canonical arrays (empty = 0)
  std::vector<double> off[3][3];  // off-diagonal sigma[c][d], d != c (empty = 0)
  bool aniso() const {
    for (int c = 0; c < 3; c++)
      for (int d = 0; d < 3; d++)
        if (!off[c][d].empty()) return true;
    return false;
  }
};

struct BoxSpec {
  int kind, index;
  double box[6];
  double value;
};

}  // namespace mnlh
using namespace mnlh;

// =============================================================== structure
struct mnl_structure {
  int dim;
  int n[3];
  int io[3];
  bool has[3];
  double a, courant, dt;
  double pml_thick[3][2] = {{0, 0}, {0, 0}, {0, 0}};
  double pml_R[3][2], pml_stretch[3][2];
  std::vector<double> chi1inv[3][3];  // [E comp][dir], canonical
  std::vector<double> chi2[3], chi3[3];
  std::vector<double> cond[2][3];     // conductivity of [B, D][dir], canonical (empty = 0)
  std::vector<Lorentz> lor;
  // H side: chi1inv of the H components (structure::set_mu ->
  // set_chi1inv(H_stuff), [H comp][dir], canonical) and the magnetic susceptibilities
  // (add_susceptibility(sigma, H_stuff, ...), diagonal sigma at the H components' points)
  std::vector<double> mu1inv[3][3];
  std::vector<Lorentz> hlor;
  std::vector<BoxSpec> boxes;
  size_t ntot;
  int nl_mode = 0;  // 0: the fork (NR chi2, inert chi3); 1: upstream Meep (Pade chi2/chi3)

  int shift(int c, int d) const {
    if (!has[d]) return 0;
    int t = ctype(c);
    if (t == T_E || t == T_D) return d == cdir(c);
    return d != cdir(c);
  }
  long long cstride(int d) const {
    if (!has[d]) return 0;
    long long nz = has[2] ? n[2] + 1 : 1, ny = has[1] ? n[1] + 1 : 1;
    return d == 2 ? 1 : (d == 1 ? nz : nz * ny);
  }
};

// ------------------------------------------------------------- DFT flux
// fields::add_dft_flux / add_dft / update_dfts / dft_flux::flux (src/dft.cpp:
// 51-300, 533-547, 578-640; loop_in_chunks src/loop_in_chunks.cpp:225-520),
// Cartesian, no symmetry, centered grid.  The point set, interpolation weights
// and list order are those of the reference's single-process chunk layout
// (PML regions broken off, structure.cpp:118-137), so every per-point DFT is
// bitwise the reference's; each rank accumulates the points it owns on the
// device, and flux() sums the pairs in list order on the host.
struct DftChunkH {
  int c;
  cplx scale;
  int avgmode;       // 0: point, 1: two Yee points, 2: four
  size_t N, p0;      // points, first point in the flux object's point arrays
  // the chunk's loop (for get_dft_array): corners, boundary weights, dV0,
  // include_dV_and_interp_weights, stored_weight
  int is[3], ie[3];
  double s0[3], s1[3], e0[3], e1[3], dV0;
  bool incl;
  cplx stored;
  int c0 = -1;       // near2far: the equivalent current's component (dft_chunk::vc)
  bool sqrt_w = false;  // sqrt_dV_and_interp_weights: the loop weight's square root is applied
  double extra = 1.0;   // dft_chunk::extra_weight (used by the force sum only)
  int shifti[3] = {0, 0, 0};  // periodic image chunk: the lattice shift from a loop point to
                              // the point of the region it stands for (dft_chunk::shift)
};
enum {
  DFT_FLUX = 0, DFT_FIELDS = 1, DFT_N2F = 2, DFT_ENERGY = 3, DFT_FORCE = 4, DFT_PROBE = 5,
  DFT_LDOS = 6
};
constexpr int DFT_MAXLISTS = 4;
// dft_ldos (src/dft_ldos.cpp): what an object of kind DFT_LDOS has beside
// the sampler's arrays.  The global point list (E list, then H list) follows the sources; slot =
// list index, padded to an even count.
struct LdosH {
  std::vector<double> freq;
  std::vector<cplx> Jdft;            // host data (the same on every rank)
  double jsum_lists = 0.0;           // (sum |A| over both lists) * sqrt(dV) of the current lists
  double jsum = 1.0;                 // Jsum of the last update (1.0 before the first)
  bool rec = false;                  // record(on): every step appends an update
  size_t nE = 0, nH = 0;             // points of the two lists
  std::vector<int> comp, ijk;        // per list point: the component sampled, 3 global indices
  std::vector<cplx> amp;             // ... and the source amplitude A
  double *d_amp = nullptr;           // A per slot (re, im)
  double *d_part = nullptr;          // [workgroup][update][4]
  double *d_ej = nullptr;            // [update][4]: EJ, HJ of the buffered updates
  double *d_F = nullptr;             // Fdft of this rank's points, [nfreq] complex
  int nwg = 0;                       // the fixed split of the pairs of slots into workgroups
  long long wg_pairs = 0;
  ~LdosH() {
    for (void *p : {(void *)d_amp, (void *)d_part, (void *)d_ej, (void *)d_F})
      if (p) (void)hipFree(p);
  }
};
struct DftFluxH {
  std::vector<double> omega;
  int nfreq = 0, decim = 1;
  bool fields = false;                // dft_fields (add_dft_fields): chunks in E only
  double wmin[3] = {0, 0, 0}, wmax[3] = {0, 0, 0};  // `where` (get_dft_array's collapse)
  // up to four chunk lists in list order (next_in_dft).  flux: E, H; fields / near2far: one
  // list; energy: E, H, D, B; force: offdiag1, offdiag2, diag
  int kind = DFT_FLUX;
  int nlists = 2;
  std::vector<DftChunkH> L[DFT_MAXLISTS];
  std::vector<DftChunkH> &E = L[0], &H = L[1];
  size_t npts = 0;                    // E points, then H points (energy / force: call order)
  std::vector<int> h_pj;              // 3 local indices per point (-1: not this rank's)
  Box bbox{};                         // this rank's points, +1 along every axis (dft_layout;
                                      // empty: lo > hi)
  int *d_pj = nullptr, *d_pch = nullptr;
  double *d_pw = nullptr;             // w * 0.25 / 0.5 / 1 per point
  DftChunkDev *d_ch = nullptr;        // per chunk (E list, then H list)
  double *d_dft = nullptr;            // [slot/64][freq][slot%64] complex (re, im)
  double *d_ph = nullptr;             // phases of one batch: [update][chunk][freq] complex
  size_t ph_cap = 0;
  int row = 0;                        // next phase row of this batch
  std::vector<double> ph_host;        // host copy of d_ph (the buffered rows move to the front)
  std::vector<int> slot;              // device slot of each point (reference order -> slot)
  double *d_fr = nullptr;             // [update][slot] sampled fields awaiting accumulation
  int nbuf = 0;                       // buffered updates (rows row-nbuf .. row-1)
  int kb = DFT_KB;                    // updates per accumulation
  double bytes = 0;                   // algorithmic bytes of one update (DESIGN.md "DFT")
  int *d_sidx = nullptr;              // sampling plan (k_dft_plan): first Yee index per point
  unsigned short *d_ssel = nullptr;   // ... and a selector per point
  unsigned *d_spal = nullptr;         // ... and the palette bytes of its implicit-E chi1inv
  void *d_su = nullptr;               // ... or those chi1inv values as doubles (fallback)
  int *d_bad = nullptr;               // palette check of the plan (k_dft_plan)
  bool usepal = false;                // the plan's palette bytes are exact
  // compact box (pairs of steps): bbox's D / B of the two-step points
  // for both steps of a pair, stored by the two-step kernel; per point its compact index
  double *d_cmp = nullptr;
  unsigned cmp_cells = 0;             // 0: the box is too large for a compact copy
  unsigned cmp_mask = 0;              // arrays the samples read (D0..D2, B0..B2)
  int *d_sci = nullptr;
  bool cmp_on = false;                // the current pair plan stores this monitor's box
  long long plan_key = -1;            // the mode the plan was built for (dft_plan_key)
  // near2far (dft_near2far): every chunk is in E; per point the absolute
  // half-pixel coordinates and the loop weight (reference order), on the device the Yee
  // positions [3][slots padded to 64] and the (first slot, count, c0) runs in slot order
  bool n2f = false;
  double eps = 1, mu = 1;             // the surrounding medium
  std::vector<double> freq;
  std::vector<int> h_pp;
  std::vector<double> h_pw;
  double *d_x0 = nullptr, *d_freq = nullptr;
  N2FRun *d_runs = nullptr;
  int nruns = 0;
  size_t nmine = 0;                   // this rank's slots (they sort first)
  int n2f_nwg = 0, n2f_wg_blocks = 0; // the fixed split of the slots into workgroups
  double *d_n2f_part = nullptr, *d_n2f_xyz = nullptr, *d_n2f_out = nullptr;  // farfields scratch
  size_t n2f_part_cap = 0, n2f_pts_cap = 0;
  // data in list order: per list the slot -> list index map (-1: not in
  // the list or not this rank's; built at first use) and a device buffer [list point][freq]
  int *d_inv[DFT_MAXLISTS] = {nullptr, nullptr, nullptr, nullptr};
  double *d_list = nullptr;
  size_t list_cap = 0;                // doubles
  // pair sums (energy / force): per sum the runs of paired slots, the
  // fixed split into workgroups, the partial sums [workgroup][freq] and the result
  struct PairSum {
    PairRun *d_runs = nullptr;
    int nruns = 0, nwg = 0, wg_pts = 0;
    long long total = 0;
    bool built = false;
  } ps[2];
  double *d_ps_part = nullptr, *d_ps_out = nullptr;
  size_t ps_part_cap = 0;
  // the fixed split of dft_norm's sum over the padded array into workgroups, its partial sums
  // [workgroup] and the result
  int norm_nwg = 0;
  long long norm_wg_blocks = 0;
  double *d_norm_part = nullptr;
  // field probe (kind DFT_PROBE): one list of up to 8 points with the
  // get_field weights, no frequencies.  Its flush turns each buffered row into one value of
  // the device series, a ring of series_cap values: the last series_n steps up to series_t
  // (the oldest dropped on overrun), the value of step s at index s % series_cap.  The probe
  // owns its device arrays (freed with it; those of the other kinds live as long as the fields).
  double *d_series = nullptr;
  int *d_pslot = nullptr;             // the points' slots in list order (-1: another rank's)
  int series_cap = 0;
  long long series_n = 0, series_t = 0;
  // LDOS (kind DFT_LDOS): two lists, no DFT array; the object owns its device arrays as a probe
  // does.  d_ph / ph_host hold one row per update: Ephase[nfreq], Hphase[nfreq] complex, then
  // the first source's current and whether there was a source at all
  std::unique_ptr<LdosH> ld;
  // flux objects: the regions given and the first one's normal (dft_flux::normal_direction)
  int nreg = 0, normal = -1;
  // mode coefficients (mnl_modes.cpp): the per-slot index arrays, the slot
  // ranges of the workgroups and the distinct coordinates the phase tables are built over;
  // built at the first call (a flux object's slot arrays are never rebuilt), with the per-call
  // tables, partial sums and results in buffers that grow
  struct ModeIdx {
    bool built = false;
    int da = 0, db = -1, nlayer = 1, layer[2] = {0, 0};
    std::vector<int> ca, cb;
    int nwg = 0, wg0[5] = {0, 0, 0, 0, 0};  // workgroups wg0[j] .. wg0[j+1]-1 add to sum j
    long long nslots = 0;
    ModeSlot *d_slot = nullptr;
    double *d_wv = nullptr;
    ModeRange *d_rng = nullptr;
    double *d_tab = nullptr, *d_part = nullptr, *d_out = nullptr;
    size_t tab_cap = 0, part_cap = 0, out_cap = 0;
  } mo;
  DftFluxH() = default;
  DftFluxH(const DftFluxH &) = delete;
  ~DftFluxH() {
    for (void *p : {(void *)d_inv[0], (void *)d_inv[1], (void *)d_inv[2], (void *)d_inv[3],
                    (void *)ps[0].d_runs, (void *)ps[1].d_runs, (void *)d_ps_part,
                    (void *)d_ps_out, (void *)d_list, (void *)d_n2f_part,
                    (void *)d_n2f_xyz, (void *)d_n2f_out, (void *)d_ph, (void *)d_sidx,
                    (void *)d_ssel, (void *)d_spal, d_su, (void *)d_bad, (void *)d_cmp,
                    (void *)d_sci, (void *)d_norm_part, (void *)d_series, (void *)d_pslot,
                    (void *)mo.d_slot, (void *)mo.d_wv, (void *)mo.d_rng, (void *)mo.d_tab,
                    (void *)mo.d_part, (void *)mo.d_out})
      if (p) (void)hipFree(p);
    if (kind == DFT_PROBE || kind == DFT_LDOS)
      for (void *p : {(void *)d_pj, (void *)d_pch, (void *)d_pw, (void *)d_ch, (void *)d_fr})
        if (p) (void)hipFree(p);
  }
};

// =============================================================== fields
struct mnl_fields {
  mnl_structure S;  // copy of the global structure description
  int device = 0;
  hipStream_t stream = nullptr;
  int rank = 0, nranks = 1;
  std::shared_ptr<Comm> comm;  // (part 1 of complex fields shares part 0's)
  int slab_dir = 2;  // direction decomposed across ranks
  // fields::use_bloch with k = 0: both boundaries of the direction are
  // Periodic -- no metal wall, plane n of the unshifted components owned, the not-owned planes
  // copies of the owner one lattice vector away (wrap)
  bool periodic[3] = {false, false, false};
  // complex fields (fields::use_real_fields undone).  Every step kernel is
  // linear with real coefficients in the supported media, so the real and the imaginary part
  // step as two real field sets: this object holds part 0 and owns `twin`, a second fields
  // object of the same structure that holds part 1, shares this one's stream and is stepped in
  // lockstep (step_batch_cplx).  The parts meet only at the ghost planes (wrap).  part0: the
  // twin's way back.  eikna: fields::eikna (src/boundaries.cpp:88-99), 1 where not periodic.
  std::unique_ptr<mnl_fields> twin;
  mnl_fields *part0 = nullptr;
  cplx eikna[3] = {1.0, 1.0, 1.0};
  cplx bloch_k[3] = {0.0, 0.0, 0.0};  // fields::k of the periodic directions (part 0 holds it)
  DevGrid g;
  DevFields f;
  size_t nlocal = 0;  // doubles per local array
  bool allocated[MNL_NUM_COMPONENTS] = {false};
  bool pml_any[3] = {false, false, false};
  std::vector<uint8_t> h_flag[3], h_zone[3];
  std::vector<double> h_sig[3], h_kap[3], h_siginv[3];
  std::vector<void *> dev_allocs;
  Box interior;
  // chi(2) Newton-Raphson runs only where chi2 != 0: the interior E update splits
  // into the bounding box of those points (NR kernel) and the rest (plain kernel)
  bool nr_split_done = false;
  bool nr_shell_free = false;  // the chi2 box lies inside the interior: plain shell E kernels
  Box nr_in{};
  std::vector<Box> nr_rest;
  Box nr_chi2{};  // bounding box of chi2 != 0 (device coordinates; empty: lo > hi)
  // fused mode with chi(2): the chi2 box grown by one point, whose E / P the fused
  // kernels leave to the NR E kernel (nr_fused_e); empty: no NR point anywhere
  Box nr_xbox{};
  std::vector<Box> shell;
  BoxList shell_list;
  // fused mode (DESIGN.md "Fused step")
  bool fused = false;        // currently stepping in fused mode
  Box fusedG;                // fused domain (local indices)
  Box fusedL;                // lean box (no PML, every component owned)
  BoxList fused_shell;       // everything else (multi-rank: the top plane)
  FusedArgs fgeo;            // tile / chunk bounds (filled by make_fused_boxes)
  std::vector<int> gitems;   // general-kernel items
  int *d_gitems = nullptr;
  size_t d_gitems_cap = 0;
  // one tile kernel over every chunk outside the polarization chunks (lean + PML bodies),
  // the general kernel over those chunks only; z chunks are cut at the lean box's z range
  // (short z-PML items)
  // Settled and no longer switchable (DESIGN.md sections 5, 24, 27): the OWNC item flag (AX = 1
  // loop 475 -> 324 instructions per plane), per-item uniform palette words (3.094 -> 2.970
  // ms/step), x-face rim strips paired two to a workgroup (2.55 -> 2.37 ms/step), one
  // persistent workgroup per CU, timing events without the system fence (0.4 % of a 512^3
  // step, 2.6 % of a 256^3 one).
  // diagnostic / A-B switches, read once when the fields are created (mnl_fields_create)
  bool no_palette = false;    // MNL_NO_PALETTE=1: per-cell chi1inv loads, no byte palette
  bool tile_gen_cus_env = false;        // MNL_TILE_GEN_CUS given (the tuner keeps it)
  bool fused_zchunk_env = false;        // MNL_FUSED_ZCHUNK given (the tuner keeps it)
  bool tb_env = false, tb_zchunk_env = false;  // MNL_TB / MNL_TB_ZCHUNK given (the same)
  bool nr_defer = true;       // MNL_NR_DEFER=0: every NR problem solved in place
  bool tile_stats = false, tb_stats = false;  // MNL_TILE_STATS / MNL_TB_STATS: print
  // MNL_ITEM_CLOCK=<file>: per-item start / end records of the persistent kernels, appended
  // to <file> after every batch (ItemClock; tools/item_clock.py)
  std::string clk_path;
  unsigned long long *d_clk = nullptr;
  unsigned *d_clk_n = nullptr;
  std::vector<int> titems;   // tile-kernel items (FusedArgs::titems)
  int *d_titems = nullptr;
  size_t d_titems_cap = 0;
  unsigned *d_tflag = nullptr;  // per tile item: uniform palette word or ~0u
  size_t tflag_n = 0;
  long long tile_cells = 0;     // own cells of the tile items
  double tile_cells_nu = -1;    // ... of those that read a palette index per cell
  std::vector<char> tile_z;     // per local z plane: stepped by the tile kernel
  long long gen_cells = 0;      // own cells of the general items
  FusedTab d_tab{};          // per-direction PML coefficient tables for the fused kernels
  // multi-rank fused stepping: chunk 0 on s_aux, halo exchange on s_comm,
  // overlapped with the interior kernels on `stream` (DESIGN.md "Multi-GPU")
  hipStream_t s_aux = nullptr, s_comm = nullptr;
  hipEvent_t ev_start = nullptr, ev_early = nullptr, ev_x1 = nullptr, ev_shell = nullptr,
             ev_x0 = nullptr;
  double *pp_B[3] = {nullptr, nullptr, nullptr}, *pp_D[3] = {nullptr, nullptr, nullptr};
  double *pp_E[3] = {nullptr, nullptr, nullptr}, *pp_H[3] = {nullptr, nullptr, nullptr};
  double *pp_UB[3] = {nullptr, nullptr, nullptr};
  int fused_zchunk = 0;
  bool fused_concurrent = false;  // last fused step ran the tile + general kernels concurrently
  int tile_gen_cus = 0;           // general kernel beside the tile kernel (CUs; 0: after it)
  unsigned long long *d_fused_ctr = nullptr;  // work-item counters of the fused kernels
  unsigned long long ctr_base[FUSED_NCTR] = {0};  // their values at the next launch
  int stagger = 0, nstagger = 0;  // dev_alloc offset step (bytes) for field arrays
  void *arena = nullptr;           // optional single allocation for field-sized arrays
  size_t arena_cap = 0, arena_used = 0, arena_gap = 0;
  int arena_req = 0;               // MNL_ARENA: field arrays to reserve (0: off)
  bool contig = false;             // MNL_CONTIG: physically contiguous field allocations
  int contig_fallbacks = 0;        // contiguous requests the driver could not satisfy
  bool palette_tried = false;
  bool dsrc_in_shell = false;  // a D source point lies outside the interior box
  bool any_srcB = false, any_isrc = false;  // anywhere in the cell (all ranks agree)
  bool any_dsrc_w = false;  // a D current source on a W-form (PML-along-E) point
  unsigned pal_one = 0;        // per direction (byte d) the palette entry that is bitwise 1.0
  unsigned *d_uidx = nullptr;  // chi1inv palette indices over fusedG (null: f64 chi1inv)
  double *d_utab = nullptr;    // 3 x 256 palette values
  unsigned long long uflag_sig = 0;  // geometry the flags were built for
  unsigned *d_gflag = nullptr;  // per general item (k_general_uniform)
  size_t gflag_n = 0;
  // cells of general items that still read a palette index per cell (the algorithmic
  // bytes of bench.py's roofline count 4 B of chi1inv for those only)
  double gen_cells_nu = -1;
  bool uflag_active = false;
  bool allow_fused = true;
  // the reference allocates H (as a copy of B) and the W auxiliary fields (as a
  // copy of E / H) on the first update_eh (src/update_eh.cpp:204-216); the first
  // step runs unfused and performs those copies at the same points of the step
  bool e_first_done = false, h_first_done = false;
  bool u_first_done[2] = {false, false};  // f_u of B / D: a copy of f on the first step_db
                                          // (src/step_db.cpp:71-75)
  bool first_step_mode = false;
  bool force_unfused_next = false;  // E / H set directly (initialize_field): E != chi1inv D
  // temporal blocking: pairs of steps as rim (one-step tile kernel) +
  // L2 (two-step kernel) + rim, over three buffer sets
  bool tb_enabled = true;           // MNL_TB=0 at creation: never
  int tb_zchunk = 0;                // MNL_SCHED_TB_ZCHUNK / MNL_TB_ZCHUNK: planes per two-step
                                    // item (0: automatic)
  int rim_zchunk = 0;               // MNL_SCHED_RIM_ZCHUNK: planes per rim item of a pair
                                    // (0: fused_zchunk)
  bool tb_pol_on = true;            // MNL_SCHED_TB_POL: grids with polarization chunks step in
                                    // pairs too (false: one step at a time there)
  bool tb_r1a = true;               // MNL_SCHED_R1_BESIDE: R1's non-strip items run on a side
                                    // stream beside the two-step kernel (false: all of R1 after it)
  int tb_rs0 = 0;                   // rim items before the narrow strips (one rank)
  bool tb_srcguard = true;          // MNL_SCHED_SRC_GUARD: a pair's step sources and NaN guard
                                    // in one launch (false: two launches per step)
  bool tb_pol = false;              // the pairs step polarization chunks (general kernel, one
                                    // step at a time beside the rim launches; one rank)
  bool tb_ox_set = false;           // tb_ox set by MNL_SCHED_TB_OX (the tuner keeps it)
  int tb_ox = 0;                    // MNL_SCHED_TB_OX: most own columns of a two-step item
                                    // (0: TB_OXW = 124, the 128 columns of lanes less two halo
                                    // columns per side)
  bool nr_early = true;             // MNL_SCHED_NR_EARLY / MNL_NR_EARLY: the NR box's E phase
                                    // runs beside the tile kernel (false: after both kernels)
  unsigned fused_epoch = 0;         // bumped on every entry into the fused mode
  unsigned long long tb_sig = 0;    // inputs of the current plan (0: none)
  bool tb_have = false;             // the current plan has two-step items
  bool tb_mid_fresh = false;        // middle set holds a copy of the state (ghost / wall entries)
  std::vector<int> tb_ritems, tb_rgeo;  // rim items (tile-kernel codes) and their own boxes
  std::vector<TB2Item> tb_items;        // two-step items
  int *d_tb_ritems = nullptr, *d_tb_rgeo = nullptr;
  unsigned *d_tb_rflag = nullptr, *d_tb_uflag = nullptr;
  TB2Item *d_tb_items = nullptr;
  size_t tb_rcap = 0, tb_gcap = 0, tb_icap = 0;
  bool tb_last = false;     // the last batch of >= 2 steps stepped in pairs (tb_usable)
  int tb_res = -1;          // MNL_SCHED_RES: CUs the pairs' persistent launches leave free (-1:
                            // TB_RES_CUS with several ranks, 0 with one; A/B of the reservation)
  int res_l = -1, res_r = -1;  // MNL_SCHED_RES_TB2 / MNL_SCHED_RES_RIM: the same for the two-step /
                               // the rim launches only
  bool tb_oom = false;      // the middle buffer set did not fit: temporal blocking off
  bool tb_oom_test = false; // MNL_TB_OOM=1: its allocation fails (tests)
  bool tb_narrow = true;    // MNL_SCHED_NARROW / MNL_TB_NARROW: the pairs' rim has narrow x-face
                            // strip items (A/B)
  bool dft_pal = true;      // MNL_SCHED_DFT_PAL: DFT sampling plans carry chi1inv as palette bytes
  bool dft_cmp = true;      // MNL_SCHED_DFT_CMP / MNL_DFT_CMP: pairs sample DFT monitors from the
                            // two-step kernel's compact boxes (false: from the field arrays)
  std::vector<TBCmp> tb_cmp;  // the compact DFT boxes of the current pair plan
  int tb_nnarrow = 0;       // narrow x-face strip items of the current plan
  int tb_rfree = 0;         // leading rim items that read no slab-face data (multi-rank)
  bool tb_chain_pending = false;  // the last multi-rank pair's s_comm chain not yet joined
  double *pp3_B[3] = {nullptr, nullptr, nullptr}, *pp3_D[3] = {nullptr, nullptr, nullptr};
  double *pp3_E[3] = {nullptr, nullptr, nullptr}, *pp3_H[3] = {nullptr, nullptr, nullptr};
  double *pp3_UB[3] = {nullptr, nullptr, nullptr};
  double tb_cells = 0, tb_border = 0, tb_cells_nu = 0;  // own / border points of the items,
                                                        // own points of the mixed-palette ones
  double rim_cells = 0, rim_lean = 0, rim_cells_nu = 0;  // rim items: own / lean / mixed cells
  int nan_every = 1;                // NaN guard cadence (src/step.cpp:138-139: every step)
  int since_nan = 0;                // steps since the last NaN guard (across calls)
  bool nan_due = false;             // a guard is due once the state is complete (pending rim)
  int nan_launched = 0;             // guards launched in this chunk (flag read at its end)
  long long nan_at = 0;             // time step of the state the next guard checks
  NanTerms nan_terms{};             // this batch's interpolation terms (nan_terms_build)
  int *d_nanflag = nullptr;         // [flag, step]
  CurlPlan planB, planD;
  bool nr = false;
  bool upnl = false;  // upstream chi2/chi3 update active (nl_mode 1 with nonzero chi)
  bool hall = false;  // H-side materials: H stored everywhere (DevFields::hall)
  std::vector<uint8_t> h_hsep_zone;  // host copy of DevFields::hsep_zone (27 zone boxes)
  // sources
  std::vector<SrcTime> srcs;
  long long src0_born = 0;  // step count at which the first src_time was created: its cached
                            // current is 0 until a step has run calc_sources on it
  std::vector<SrcGroup> groups;
  bool src_dirty = true;
  std::vector<long long> srcB_idx, srcD_idx, isrc_idx;  // local linear indices
  std::vector<int> srcB_comp, srcD_comp, isrc_comp;
  std::vector<unsigned char> isrc_zone;  // owning reference chunk (zone box) per isrc point
  ISrcDev isrc_dev{};                    // device copy (sorted), built with the lists
  std::vector<std::pair<int, int>> srcB_ref, srcD_ref, isrc_ref;  // (group, point)
  // current sources per field type ([0] B, [1] D), in layer order (SrcDev)
  std::vector<double> src_amp[2];
  std::vector<int> src_gid[2], src_layer[2];
  long long *d_srcB_idx = nullptr, *d_srcD_idx = nullptr;
  int *d_srcB_comp = nullptr, *d_srcD_comp = nullptr;
  double *d_src_amp[2] = {nullptr, nullptr};
  int *d_src_gid[2] = {nullptr, nullptr};
  double *d_vals = nullptr;
  size_t d_vals_cap = 0;
  long long t = 0;
  double dt;
  // timers / profiling
  bool profiling = false;
  // fields::times_spent by time_sink (src/meep.hpp:1610-1633 order), seconds
  double sink_s[MNL_NUM_TIME_SINKS] = {0};
  double last_out_wall = -1;  // "on time step" output (src/step.cpp:44-56)
  long long last_out_t = 0;
  double timer_ms[TM_CAP] = {0};
  long long timer_count[TM_CAP] = {0};
  double n2f_ms[2] = {0, 0};         // near2far: far-field kernel, reduce kernel (HIP events)
  long long n2f_count[2] = {0, 0};
  double dftio_ms[3] = {0, 0, 0};    // DFT data: gather, scatter, scale kernels (HIP events)
  long long dftio_count[3] = {0, 0, 0};
  double dftio_bytes[3] = {0, 0, 0}; // algorithmic bytes of the last launch
  std::vector<hipEvent_t> ev_pool;
  unsigned long long *d_nr_fallbacks = nullptr;
  NRHard *d_nr_hard = nullptr;      // deferred Newton-Raphson problems (NR runs only)
  unsigned *d_nr_hard_cnt = nullptr;
  double *d_scratch = nullptr;  // canonical-size staging buffer
  size_t scratch_cap = 0;
  std::vector<std::unique_ptr<DftFluxH>> dfts;  // DFT flux objects (add_dft_flux order)
  bool dft_samples_d = false;  // a monitor samples a D component (its low ghost: exchange 3)
  // field probes (mnl_probe.cpp): their own list, so that no DFT handle moves; a removed probe
  // leaves an empty entry.  sampled: what every step samples -- the DFT objects, then the probes
  std::vector<std::unique_ptr<DftFluxH>> probes;
  std::vector<DftFluxH *> sampled;
  // LDOS objects (mnl_ldos.cpp): their own list and handles, sampled after the probes while they
  // record or take an explicit update; a removed one leaves an empty entry
  std::vector<std::unique_ptr<DftFluxH>> ldoses;
  double *d_norm_out = nullptr;  // dft_norm's per-object sums
  size_t norm_out_cap = 0;

  ~mnl_fields() {
    if (device >= 0) hipSetDevice(device);
    for (void *p : dev_allocs) hipFree(p);
    for (auto e : ev_pool) hipEventDestroy(e);
    if (d_scratch) hipFree(d_scratch);
    if (d_norm_out) hipFree(d_norm_out);
    if (d_vals) hipFree(d_vals);
    if (d_gitems) hipFree(d_gitems);
    if (d_titems) hipFree(d_titems);
    if (d_tflag) hipFree(d_tflag);
    if (d_gflag) hipFree(d_gflag);
    for (void *p : {(void *)d_tb_ritems, (void *)d_tb_rgeo, (void *)d_tb_rflag, (void *)d_tb_uflag,
                    (void *)d_tb_items})
      if (p) hipFree(p);
    comm.reset();
    for (hipEvent_t e : {ev_start, ev_early, ev_x1, ev_shell, ev_x0})
      if (e) hipEventDestroy(e);
    if (s_aux) hipStreamDestroy(s_aux);
    if (s_comm) hipStreamDestroy(s_comm);
    if (stream && !part0) hipStreamDestroy(stream);  // part 1 runs on part 0's stream
  }
};

namespace mnlh {

// ---- buffer sets
// one buffer set of the fused step's per-point state (B, D, stored E, separate H, f_u of B):
// the current arrays, their ping-pong partners, the pairs' middle set.  A partner is null
// where the current array is null.
struct Set5 {
  double *B[3], *D[3], *E[3], *H[3], *UB[3];
};
inline Set5 set_cur(const mnl_fields *F) {
  Set5 s;
  for (int d = 0; d < 3; d++)
    s.B[d] = F->f.B[d], s.D[d] = F->f.D[d], s.E[d] = F->f.E[d], s.H[d] = F->f.H[d],
    s.UB[d] = F->f.UB[d];
  return s;
}
inline Set5 set_nxt(const mnl_fields *F) {
  Set5 s;
  for (int d = 0; d < 3; d++)
    s.B[d] = F->f.Bn[d], s.D[d] = F->f.Dn[d], s.E[d] = F->f.E[d] ? F->f.En[d] : nullptr,
    s.H[d] = F->f.H[d] ? F->f.Hn[d] : nullptr, s.UB[d] = F->f.UB[d] ? F->f.UBn[d] : nullptr;
  return s;
}
inline Set5 set_mid(const mnl_fields *F) {
  Set5 s;
  for (int d = 0; d < 3; d++)
    s.B[d] = F->pp3_B[d], s.D[d] = F->pp3_D[d], s.E[d] = F->f.E[d] ? F->pp3_E[d] : nullptr,
    s.H[d] = F->f.H[d] ? F->pp3_H[d] : nullptr, s.UB[d] = F->f.UB[d] ? F->pp3_UB[d] : nullptr;
  return s;
}
// fused-kernel arguments of one step from set `o` to set `n`
inline void args_sets(FusedArgs &a, const Set5 &o, const Set5 &n) {
  for (int d = 0; d < 3; d++) {
    a.Bo[d] = o.B[d], a.Do[d] = o.D[d], a.E[d] = o.E[d], a.Ho[d] = o.H[d], a.UBo[d] = o.UB[d];
    a.Bn[d] = n.B[d], a.Dn[d] = n.D[d], a.En[d] = n.E[d], a.Hn[d] = n.H[d], a.UBn[d] = n.UB[d];
  }
}
// `f` with set `o` as its current arrays (exchanges, shell kernels and DFT updates read a
// DevFields' pointers when enqueued) ...
inline DevFields fields_at(DevFields f, const Set5 &o) {
  for (int d = 0; d < 3; d++)
    f.B[d] = o.B[d], f.D[d] = o.D[d], f.E[d] = o.E[d], f.H[d] = o.H[d], f.UB[d] = o.UB[d];
  return f;
}
// ... and set `n` as their ping-pong partners
inline DevFields fields_at(DevFields f, const Set5 &o, const Set5 &n) {
  f = fields_at(f, o);
  for (int d = 0; d < 3; d++) {
    f.Bn[d] = n.B[d], f.Dn[d] = n.D[d], f.En[d] = o.E[d] ? n.E[d] : nullptr;
    f.Hn[d] = o.H[d] ? n.H[d] : nullptr, f.UBn[d] = o.UB[d] ? n.UB[d] : nullptr;
  }
  return f;
}
// the ping-pong swap after a fused step
inline void swap_cur_nxt(DevFields &f) {
  for (int d = 0; d < 3; d++) {
    std::swap(f.B[d], f.Bn[d]);
    std::swap(f.D[d], f.Dn[d]);
    std::swap(f.E[d], f.En[d]);
    std::swap(f.H[d], f.Hn[d]);
    std::swap(f.UB[d], f.UBn[d]);
  }
}

// ---- phase timing
// The timing events of a batch's phases; flush() adds their times to timer_ms / timer_count at
// the end of a chunk.  The events are read only after a stream synchronize, so they carry no
// system-scope fence when recorded -- with it every record wrote back / invalidated the caches
// between the kernels, 0.4 % of a 512^3 step and 2.6 % of a 256^3 one (round 6).
struct PhaseTimer {
  explicit PhaseTimer(mnl_fields *fields) : F(fields) {}
  int begin(int cat, hipStream_t st = nullptr);  // on the main stream (or st); -1: profiling off
  void end(int k, hipStream_t st = nullptr);
  // a phase that starts where phase k ended: its start is k's end event (one record fewer
  // between two back-to-back kernels)
  int next(int k, int cat);
  int flush();

 private:
  struct Span { hipEvent_t a, b; int cat; };
  bool reserve_events();  // the pool holds two events for the next span
  mnl_fields *F;
  std::vector<Span> spans;
};

// a host list on the device: the buffer grows as needed, the copy is enqueued on the main stream
template <class T>
int dev_upload(mnl_fields *F, T **d, size_t &cap, const std::vector<T> &h) {
  if (h.empty()) return 0;
  if (cap < h.size()) {
    if (*d) (void)hipFree(*d);
    *d = nullptr;
    HIPCHK(hipMalloc(d, h.size() * sizeof(T)));
    cap = h.size();
  }
  HIPCHK(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, F->stream));
  return 0;
}

// Field-sized arrays start at staggered offsets (a multiple of 128 B, different
// for every array) so that the many streams one fused step reads and writes at
// the same element index do not start on the same HBM channel / bank.
template <class T>
int dev_alloc(mnl_fields *F, T **p, size_t n, bool zero = true) {
  void *q = nullptr;
  const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
  if (F->arena_req > 0 && !F->arena && F->nlocal && bytes >= (size_t(64) << 20)) {
    const size_t cap = size_t(F->arena_req) * (F->nlocal * 8 + F->arena_gap + 4096);
    const hipError_t ea = F->contig ? hipExtMallocWithFlags(&F->arena, cap, hipDeviceMallocContiguous)
                                    : hipMalloc(&F->arena, cap);
    if (ea == hipSuccess) {
      F->arena_cap = cap;
      F->dev_allocs.push_back(F->arena);
    } else {
      F->arena_req = 0;
      (void)hipGetLastError();
    }
  }
  if (F->arena_cap && bytes >= (size_t(64) << 20)) {  // field-sized: bump-allocate in the arena
    const size_t at = (F->arena_used + 255) & ~size_t(255);
    if (at + bytes <= F->arena_cap) {
      F->arena_used = at + bytes + F->arena_gap;
      *p = (T *)((char *)F->arena + at);
      if (zero) {
        hipError_t e = hipMemsetAsync(*p, 0, bytes, F->stream);
        if (e != hipSuccess) return fail(std::string("hipMemset failed: ") + hipGetErrorString(e));
      }
      return 0;
    }
  }
  const bool big = bytes >= (size_t(64) << 20) && F->stagger > 0;
  const size_t off = big ? (size_t(F->stagger) * F->nstagger++) % (size_t(1) << 20) : 0;
  const size_t nb = bytes + (big ? (size_t(1) << 20) : 0);
  hipError_t e = hipErrorUnknown;
  if (F->contig && bytes >= (size_t(64) << 20)) {
    e = hipExtMallocWithFlags(&q, nb, hipDeviceMallocContiguous);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      F->contig_fallbacks++;
    }
  }
  if (e != hipSuccess) e = hipMalloc(&q, nb);
  if (e != hipSuccess) return fail(std::string("hipMalloc failed: ") + hipGetErrorString(e));
  if (zero) {
    e = hipMemsetAsync((char *)q + off, 0, bytes, F->stream);
    if (e != hipSuccess) return fail(std::string("hipMemset failed: ") + hipGetErrorString(e));
  }
  F->dev_allocs.push_back(q);
  *p = (T *)((char *)q + off);
  return 0;
}

inline bool any_periodic(const mnl_fields *F) {
  return F->periodic[0] || F->periodic[1] || F->periodic[2];
}
inline bool is_complex(const mnl_fields *F) { return F->twin || F->part0; }
// what complex fields do not do yet: `what` fails with the follow-up named
inline int refuse_complex(const mnl_fields *F, const char *what) {
  if (!is_complex(F)) return 0;
  return fail(std::string(what) + " is not supported on complex fields yet");
}
inline int check_comp(int c) {
  if (c < 0 || c >= MNL_NUM_COMPONENTS) return fail("invalid component");
  return 0;
}
inline bool all_eq(const std::vector<double> &v, double x) {
  for (double y : v)
    if (y != x) return false;
  return true;
}

// ---- mnl_setup.cpp: PML tables, grid, allocation, materials
struct ZoneIv {
  int c0, c1, zone;  // chunk covers half-coords [c0, c1] relative to io
};
std::vector<ZoneIv> zone_intervals(const mnl_structure &S, int d);
void slab_range(int ncell, int rank, int nranks, int *lo, int *hi);
bool has_field(const mnl_structure &S, int c);
int require_component(mnl_fields *F, int c);
int finalize_fields(mnl_fields *F);
int set_periodic(mnl_fields *F, int dir);
int initialize_field(mnl_fields *F, int c, const double *host);
MNL_HIDDEN int sphere_quadrature(int dim, double *xyzw);
MNL_HIDDEN int set_epsilon_geometry(mnl_structure *s, int device, int nobj, const double *objs,
                                    double default_eps, int use_averaging, double tol,
                                    int maxeval);

// ---- mnl_sources.cpp: sources, local indices, get_field
int build_source_lists(mnl_fields *F);
SrcDev src_dev(mnl_fields *F, int t, const double *J);
void interpolate(const mnl_structure &S, int c, const double pc[3], int locs[8][3], double w[8]);
long long local_index(const mnl_fields *F, int c, const int jg[3], bool include_wall);
int get_field(mnl_fields *F, int c, const double pos[3], double *out, bool reduce);
int add_source_any(mnl_fields *F, int comp, int kind, const double *p, int np, mnl_src_func func,
                   void *fdata, const double vmin[3], const double vmax[3], double amp_re,
                   double amp_im, int is_integrated, mnl_amp_func afunc, void *adata);

// ---- mnl_fused.cpp: planning of the fused step
void split_range(std::vector<int> &b, int lo, int hi_excl, int step, int align);
int tile_item_code(const mnl_fields *F, const FusedArgs &a, const Box &L, int x0, int x1, int y0,
                   int y1, int zs, int ze, bool *lean);
int strip_item_code(const mnl_fields *F, const FusedArgs &a, int x0, int x1, int y0, int y1, int zs,
                    int ze);
bool in_fused_box(const mnl_fields *F, int c, const int jg[3]);
bool fused_agreed(mnl_fields *F);
int set_fused(mnl_fields *F, bool on);
FusedArgs &fused_args(mnl_fields *F);

// ---- mnl_tb.cpp: pairs of steps (temporal blocking)
int tb_usable(mnl_fields *F, bool *ok);
int tb_pair(mnl_fields *F, const SrcDev &s0, const SrcDev &s1, PhaseTimer &pt, long long t_mid);
int tb_pair_multi(mnl_fields *F, const SrcDev &s0, const SrcDev &s1, PhaseTimer &pt,
                  long long t_mid);
int tb_chain_join(mnl_fields *F);

// ---- mnl_step.cpp: the step path and the NaN guard
constexpr int NR_HARD_CAP = 4096;  // deferred NR problems per E update (more: solved in place)
int exchange(mnl_fields *F, int kind, hipStream_t st = nullptr);
constexpr int WRAP_ALL = 5;  // wrap kind: every field and polarization array (readers, checkpoints)
int wrap(mnl_fields *F, int kind, hipStream_t st = nullptr);
int wrap_for_readers(mnl_fields *F);
int h_lazy_copy(mnl_fields *F);
int u_lazy_copy(mnl_fields *F, int which);
int e_lazy_copy(mnl_fields *F);
int update_h_any(mnl_fields *F, const BoxList &sl, bool pols);
int nr_split(mnl_fields *F);
int nr_defer_begin(mnl_fields *F, hipStream_t st = nullptr);
int nr_defer_end(mnl_fields *F, hipStream_t st = nullptr);
int fused_fail(const char *what, int kr);
int ensure_aux_stream(mnl_fields *F);
int shell_step(mnl_fields *F, hipStream_t st, bool fuseE, const SrcDev &sD,
               hipEvent_t h_in = nullptr);
int nan_launch(mnl_fields *F, hipStream_t st = nullptr, double *const *E = nullptr,
               double *const *D = nullptr);
void nan_count(mnl_fields *F, int k);
int fields_step(mnl_fields *F, int nsteps);

// ---- mnl_tune.cpp
int tune(mnl_fields *F, int reps, int *zchunk, int *gen_cus);

// ---- mnl_stats.cpp: kernel statistics and the byte model, tb_info, the mode word
MNL_HIDDEN int kernel_stats(const mnl_fields *F, int which, long long *launches, double *total_ms,
                            double *bytes_per_launch);
MNL_HIDDEN void traffic_model(const mnl_fields *F, double *bpc, double *cells);
MNL_HIDDEN void tb_info(const mnl_fields *F, double v[MNL_NUM_TBINFO]);
MNL_HIDDEN int fields_mode(const mnl_fields *F);

// ---- mnl_dft.cpp: loop_in_chunks helpers and DFT monitors
// loop_in_chunks' loop over lattice shifts (src/loop_in_chunks.cpp:390-412, 525-532): per
// periodic direction the shifts for which the cell's image meets [wmin, wmax], the first
// direction fastest; shifti in half-coordinates.  A shift whose image misses the region's
// grid points gives empty chunk loops, which the callers skip as the reference does.
struct LatticeShifts {
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, cur[3] = {0, 0, 0}, shifti[3] = {0, 0, 0};
  int iL[3] = {0, 0, 0};
  LatticeShifts(const mnl_structure &S, const bool per[3], const double wmin[3],
                const double wmax[3]) {
    for (int d = 0; d < 3; d++) {
      if (!S.has[d] || !per[d]) continue;
      const double L = S.n[d] * (1.0 / S.a);
      const double gmin = S.io[d] * (0.5 * (1.0 / S.a)), gmax = gmin + L;
      lo[d] = int(floor((wmin[d] - gmax) / L));
      hi[d] = int(ceil((wmax[d] - gmin) / L));
      iL[d] = 2 * S.n[d];
      cur[d] = lo[d];
      shifti[d] = iL[d] * cur[d];
    }
  }
  bool next() {  // false after the last shift
    for (int d = 0; d < 3; d++) {
      if (cur[d] + 1 <= hi[d]) {
        cur[d]++;
        shifti[d] = iL[d] * cur[d];
        return true;
      }
      cur[d] = lo[d];
      shifti[d] = iL[d] * cur[d];
    }
    return false;
  }
};
inline int my_round(double x) { return int(floor(fabs(x) + 0.5) * (x < 0 ? -1 : 1)); }
// handles of field probes start here; everything below is a DFT object's index
constexpr int PROBE_BASE = 1 << 30;
inline int dft_bad_handle(const mnl_fields *F, int h) {
  if (h >= PROBE_BASE)
    return fail("handle " + std::to_string(h) + " is a field probe, not a DFT object: it has "
                "no DFT data (read it with mnl_fields_probe_read)");
  return h < 0 || h >= (int)F->dfts.size() ? fail("bad dft handle") : 0;
}
inline size_t dft_at(size_t p, size_t i, size_t nf) { return ((p >> 6) * nf + i) * 64 + (p & 63); }
void dft_boundary_weights(const mnl_structure &S, const double wmin[3], const double wmax[3],
                          const int is[3], const int ie[3], double s0[3], double e0[3],
                          double s1[3], double e1[3]);
std::vector<std::array<int, 6>> reference_chunks(const mnl_structure &S);
int dft_decimation(mnl_fields *F, const double *freqs, int nfreq, int decim);
int dft_add_flux(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                 int decim);
int dft_add_fields(mnl_fields *F, int ncomp, const int *comps, const double wmin[3],
                   const double wmax[3], const double *freqs, int nfreq, int yee, int decimation);
int dft_block();
int dft_prepare(mnl_fields *F, long long t0, int ns);
int dft_flush(mnl_fields *F, DftFluxH &o);
long long dft_plan_key(const mnl_fields *F);
// cstate >= 0: a pair's middle (0) or new (1) state, whose two-step points are also in the
// monitors' compact boxes
// only: sample this object alone, whether it records or not (an explicit LDOS update)
int dft_update(mnl_fields *F, long long t, const DevFields *fields = nullptr, int cstate = -1,
               DftFluxH *only = nullptr);
bool dft_due(const mnl_fields *F, long long t);
// sampled by the step that reaches step count t: an LDOS object only while it records
inline bool dft_samples_at(const DftFluxH &o, long long t) {
  return o.npts && t % o.decim == 0 && (o.kind != DFT_LDOS || o.ld->rec);
}
int dft_flux_values(mnl_fields *F, int h, double *out);
int dft_add_energy(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                   int decimation);
int dft_add_force(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                  int decimation);
int dft_energy_values(mnl_fields *F, int h, int which, double *out);
int dft_force_values(mnl_fields *F, int h, double *out);
int dft_points(mnl_fields *F, int h, int which, double *out, long long npoints);
MNL_HIDDEN int dft_array(mnl_fields *F, int h, int c, int num_freq, int *rank, long long dims[3],
                         double *out, long long nout);
size_t dft_list_points(const DftFluxH &o, int which);
bool dft_bad_which(const DftFluxH &o, int which);
const char *dft_list_name(const DftFluxH &o, int which);
int dft_get(mnl_fields *F, int h, int which, double *out, long long n);
int dft_load(mnl_fields *F, int h, int which, const double *in, long long n, int sign);
int dft_scale(mnl_fields *F, int h, double re, double im);
// ---- mnl_probe.cpp: field probes, dft_norm
void dft_sampled_rebuild(mnl_fields *F);
int probe_flush(mnl_fields *F, DftFluxH &o);
int probe_add(mnl_fields *F, int c, const double pos[3]);
int probe_read(mnl_fields *F, int h, long long cap, long long *count, long long *t_first,
               double *values);
int probe_reset(mnl_fields *F, int h);
void probe_restart(mnl_fields *F);
int probe_remove(mnl_fields *F, int h);
int probe_remove_all(mnl_fields *F);
int dft_norm(mnl_fields *F, double *out);
double dft_maxfreq(const mnl_fields *F);
int dft_max_decimation(const mnl_fields *F);
// ---- mnl_ldos.cpp: LDOS spectra (dft_ldos)
constexpr int LDOS_BASE = 1 << 29;  // handles of LDOS objects: [LDOS_BASE, PROBE_BASE)
int ldos_add(mnl_fields *F, const double *freqs, int nfreq);
int ldos_update(mnl_fields *F, int h);
int ldos_record(mnl_fields *F, int h, int on);
int ldos_data(mnl_fields *F, int h, double *ldos, double *Fout, double *Jout, double *scale);
int ldos_points(mnl_fields *F, int h, long long cap, long long *n, int *comp, int *ijk,
                double *amp);
int ldos_remove(mnl_fields *F, int h);
int ldos_remove_all(mnl_fields *F);
int ldos_flush(mnl_fields *F, DftFluxH &o);
int ldos_prepare(mnl_fields *F, long long t0, int ns);  // phase rows of a chunk's updates
void ldos_sampled(mnl_fields *F, DftFluxH &o);          // an update was taken
int ldos_sources_rebuilt(mnl_fields *F);                // the source lists were rebuilt
void ldos_restart(mnl_fields *F);
int dft_save(mnl_fields *F, int h, const char *path);
int dft_load_file(mnl_fields *F, int h, const char *path, int sign);
int dft_add_near2far(mnl_fields *F, int nreg, const double *regions, const double *freqs, int nfreq,
                     int decimation, int nperiods);
int n2f_farfields(mnl_fields *F, int h, long long npts, const double *xyz, double *out);
int n2f_points(mnl_fields *F, int h, double *out, long long npoints);
double n2f_medium_at(const mnl_structure &S, int t, const double pos[3]);  // get_eps / get_mu
// ---- mnl_modes.cpp: mode coefficients of diffraction orders (get_eigenmode_coefficients with a
// DiffractedPlanewave)
struct ModeCall {  // the arguments of both entry points
  int h, nmodes;
  const int *g;
  const double *axis, *sp, *eig_vol, *kpoint;
};
int mode_coefficients(mnl_fields *F, const ModeCall &c, double *coeffs, double *vgrp,
                      double *kpoints, double *cscale, double *overlaps);
int mode_table(mnl_fields *F, const ModeCall &c, long long dims[4], int *coords, double *k,
               double *vgrp, double *amp, double *pa, double *pb, double *pl);

// ---- mnl_io.cpp: checkpoints, array slices, field energy
struct CkEntry {
  int kind, a, b;
  double *p;
  size_t n;
};
inline double wall_now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// loop_in_chunks' per-index weight of a dimension (s0 / s1 at the low end, e0 / e1 at the high)
inline double loop_w1(double s0, double s1, double e0, double e1, int i, int n) {
  return (i > 1 && i < n - 2) ? 1.0 : (i == 0 ? s0 : (i == 1 ? s1 : i == n - 1 ? e0 : (i == n - 2 ? e1 : 1.0)));
}
std::vector<CkEntry> ckpt_entries(mnl_fields *F);
int fields_dump(mnl_fields *F, const char *path);
int fields_load(mnl_fields *F, const char *path);
int structure_dump(const mnl_structure *S, const char *path);
int structure_load(mnl_structure *S, const char *path);
double mat_diag_at(const mnl_structure &S, int t, int k, const int j[3]);
int array_slice(mnl_fields *F, int c, const double vmin[3], const double vmax[3], int snap,
                int *rank, long long dims[3], double *out, long long nout);
int energy_in_box(mnl_fields *F, int which, const double wmin[3], const double wmax[3],
                  double *out);
int timed_allreduce(mnl_fields *F, double *v, int n);

}  // namespace mnlh
