// mnl_stats.cpp -- the diagnostic read-outs of the fields: the algorithmic-byte model behind the
// roofline numbers (kernel_stats, traffic_model; DESIGN.md "Roofline"), tb_info and the mode
// word.  The slots, ids and bits are the MNL_KSTAT_* / MNL_TBINFO_* / MNL_MODE_* enumerators of
// include/meep_nl_amd.h.  The byte formulas are pinned value for value by
// tests/test_gpu_stats_model.py: keep the order of their floating-point operations.
#include "mnl_host.hpp"

namespace mnlh {

// Algorithmic HBM bytes of the fused mode's launches over G (DESIGN.md "Fused step"): every
// point reads B, D and writes B, D (96 B) + chi1inv (4 B palette word or 3 doubles); PML state
// is counted per (point, component) where the reference keeps it: f_u of B / D, separate H,
// W-form E (read + write 16 B).
struct ByteModel {
  double lean;  // one step of the tile kernel
  double gen;   // one step of the general kernel (the polarization chunks)
  double tb;    // the two-step items' two steps (0 without a pair plan)
  double rim;   // one rim launch of a pair (0 without a pair plan)
};

static ByteModel byte_model(const mnl_fields *F) {
  ByteModel m{0, 0, 0, 0};
  if (!F->fused) return m;
  const DevGrid &g = F->g;
  const FusedArgs &a = F->fgeo;
  int nu = 0;
  for (int d = 0; d < 3; d++) nu += F->f.inveps[d] ? 1 : 0;
  const double ub = F->d_uidx ? 4.0 : 8.0 * nu;
  double extra = 0, extra_t = 0;
  // count of local indices j in [lo, hi] of axis e with an optional flag condition;
  // zsel (axis 2): 1 the tile kernel's planes, 2 the others
  int zsel = 1;
  auto cnt = [&](int e, int lo, int hi, int qshift, bool need_flag) -> double {
    double n = 0;
    for (int j = lo; j <= hi; j++) {
      if (e == 2 && (j < 0 || j >= (int)F->tile_z.size() ||
                             (F->tile_z[j] != 0) != (zsel == 1)))
        continue;
      if (need_flag) {
        if (!F->S.has[e] || F->h_flag[e].empty()) continue;
        if (!F->h_flag[e][2 * (j + g.off[e]) + qshift]) continue;
      }
      n += 1;
    }
    return n;
  };
  for (zsel = 1; zsel <= 2; zsel++) {
    for (int c = 0; c < 3; c++)
      for (int kind = 0; kind < 4; kind++) {
        // kind 0: f_u of B_c (flag along c+2, shifted); 1: H_c (along c, unshifted);
        // 2: f_u of D_c (along c+2, unshifted); 3: W-form E_c (along c, shifted)
        const bool btype = kind < 2;
        const int fe = (kind == 0 || kind == 2) ? (c + 2) % 3 : c;
        const int qs = (kind == 0 || kind == 3) ? 1 : 0;
        double n = 1;
        for (int e = 0; e < 3; e++) {
          const bool sh = btype ? (e != c) : (e == c);
          const int lo = sh ? a.osh_lo[e] : a.oun_lo[e], hi = sh ? a.osh_hi[e] : a.oun_hi[e];
          n *= cnt(e, lo, hi, qs, e == fe);
        }
        (zsel == 1 ? extra_t : extra) += 16.0 * n;
      }
  }
  // with per-item uniform palette words only the mixed items read chi1inv per cell
  const bool tuni = F->d_uidx && F->uflag_active && F->tile_cells_nu >= 0;
  m.lean = double(F->tile_cells) * 96.0 +
           (tuni ? F->tile_cells_nu : double(F->tile_cells)) * ub + extra_t;
  // polarization boxes: stored E (read + write), P and Pprev (read + write) and
  // sigma (read) per component and susceptibility
  for (int k = 0; k < F->f.npol; k++) {
    const Box &b = F->f.pol[k].nz;
    double n = 1;
    for (int e = 0; e < 3; e++) {
      const int lo = std::max(b.lo[e], F->fusedG.lo[e]), hi = std::min(b.hi[e], F->fusedG.hi[e]);
      n *= hi >= lo ? double(hi - lo + 1) : 0.0;
    }
    int nc = 0;
    for (int d = 0; d < 3; d++) nc += F->f.pol[k].P[d] ? 1 : 0;
    extra += n * nc * (40.0 + (k == 0 ? 16.0 : 0.0));
  }
  const bool guni = F->d_uidx && F->uflag_active && F->gen_cells_nu >= 0;
  m.gen = double(F->gen_cells) * 96.0 +
          (guni ? F->gen_cells_nu : double(F->gen_cells)) * ub + extra;
  if (F->tb_have) {
    // the two-step items' two steps: B, D read once and written once, the palette word where
    // the item is mixed, the border points' step n+1 B, D.  A rim launch: the tile kernel's
    // bytes with the rim's cells in place of the tile items'
    m.tb = F->tb_cells * 96.0 + (F->d_uidx ? F->tb_cells_nu : F->tb_cells) * ub +
           F->tb_border * 48.0;
    m.rim = m.lean - double(F->tile_cells) * 96.0 -
            (tuni ? F->tile_cells_nu : double(F->tile_cells)) * ub + F->rim_cells * 96.0 +
            (F->d_uidx ? F->rim_cells_nu : F->rim_cells) * ub;
  }
  return m;
}

// unfused interior curl of B (T_B) or D: read 3 source comps + read/write the updated comps
static double curl_bytes(const mnl_fields *F, int t) {
  const Box &b = F->interior;
  double pts = 1;
  for (int k = 0; k < 3; k++) pts *= double(b.hi[k] - b.lo[k] + 1);
  if (b.hi[0] < b.lo[0]) pts = 0;
  int ncomp = 0;
  const CurlPlan &p = t == T_B ? F->planB : F->planD;
  for (int d = 0; d < 3; d++) ncomp += p.present[d] ? 1 : 0;
  int nsrc = 0;
  for (int d = 0; d < 3; d++) nsrc += F->allocated[3 * (t == T_B ? T_E : T_H) + d] ? 1 : 0;
  return pts * 8.0 * (nsrc + 2 * ncomp);
}

int kernel_stats(const mnl_fields *F, int which, long long *launches, double *total_ms,
                 double *bytes_per_launch) {
  const ByteModel m = byte_model(F);
  const bool pairs = F->fused && F->tb_have;
  auto phase = [&](int cat, double bytes) {  // a phase timer's launches and time
    *launches = F->timer_count[cat];
    *total_ms = F->timer_ms[cat];
    *bytes_per_launch = bytes;
  };
  switch (which) {
    case MNL_KSTAT_TILE:  // concurrent tile + general: the timed span covers both kernels
      phase(TM_BINT, !F->fused               ? curl_bytes(F, T_B)
                     : F->fused_concurrent ? m.lean + m.gen
                                           : m.lean);
      break;
    case MNL_KSTAT_CURL_D:
      phase(TM_DINT, curl_bytes(F, T_D));
      break;
    case MNL_KSTAT_GENERAL:
      phase(TM_GEN, m.gen);
      break;
    case MNL_KSTAT_DFT: {
      double b = 0;
      for (auto &o : F->dfts) b += o->bytes;
      phase(TM_DFT, b);
      *total_ms += F->timer_ms[TM_DFTF];
      break;
    }
    case MNL_KSTAT_E_UPDATE:
      phase(TM_E, 0);
      break;
    case MNL_KSTAT_PAIRS:  // two phase launches per pair, the drains of the rim's last step
      phase(TM_TB, m.tb + 2.0 * m.rim);
      *total_ms += F->timer_ms[TM_RIM];
      if (pairs && F->tb_pol) {  // + the polarization chunks' two steps
        *total_ms += F->timer_ms[TM_GEN];
        *bytes_per_launch += 2.0 * m.gen;
      }
      break;
    case MNL_KSTAT_RIM:
      phase(TM_RIM, m.rim);
      break;
    case MNL_KSTAT_CHAIN:
      phase(TM_CHAIN, 0);
      break;
    case MNL_KSTAT_GHOST_WAIT:
      phase(TM_WAIT, 0);
      break;
    case MNL_KSTAT_N2F_FAR:
    case MNL_KSTAT_N2F_REDUCE:
      *launches = F->n2f_count[which - MNL_KSTAT_N2F_FAR];
      *total_ms = F->n2f_ms[which - MNL_KSTAT_N2F_FAR];
      *bytes_per_launch = 0;
      break;
    case MNL_KSTAT_DFT_GET:
    case MNL_KSTAT_DFT_LOAD:
    case MNL_KSTAT_DFT_SCALE:
      *launches = F->dftio_count[which - MNL_KSTAT_DFT_GET];
      *total_ms = F->dftio_ms[which - MNL_KSTAT_DFT_GET];
      *bytes_per_launch = F->dftio_bytes[which - MNL_KSTAT_DFT_GET];
      break;
    default:
      return fail("bad kernel id");
  }
  return 0;
}

// Minimal per-step HBM traffic per interior cell of the kernels in use (DESIGN.md "Roofline"):
// fused: B, D read+write, chi1inv read; unfused: curl B reads E(3)+B(3), writes B(3); curl D
// reads H=B(3)+D(3), writes D(3); E update reads D(3) (+chi1inv 3), writes E(3) (+P terms).
void traffic_model(const mnl_fields *F, double *bpc, double *cells) {
  double b;
  if (F->fused) {  // whole fused step over G per G point (PML state included)
    const ByteModel m = byte_model(F);
    double gc = 1;
    for (int e = 0; e < 3; e++) gc *= double(F->fusedG.hi[e] - F->fusedG.lo[e] + 1);
    b = (m.lean + m.gen) / gc;
  } else {
    double n = 0;
    for (int d = 0; d < 3; d++) n += F->allocated[d] ? 1 : 0;
    int nu = 0;
    for (int d = 0; d < 3; d++) nu += F->f.inveps[d] ? 1 : 0;
    b = 8.0 * (3 * n) * 2 + 8.0 * (2 * n) + 8.0 * nu;
    for (int k = 0; k < F->f.npol; k++)
      for (int d = 0; d < 3; d++)
        if (F->f.pol[k].P[d]) b += 8.0 * 5;
    for (int t = 0; t < 2; t++)  // cnd and cndinv read per conductive component
      for (int d = 0; d < 3; d++)
        if (F->f.cnd[t][d]) b += 8.0 * 2;
  }
  *bpc = b;
  double c = 1;
  for (int d = 0; d < 3; d++)
    if (F->S.has[d]) {
      if (d == F->slab_dir && F->nranks > 1)
        c *= double(F->g.owned_hi_sh[d] - F->g.owned_lo_sh[d] + 1);
      else
        c *= F->S.n[d];
    }
  *cells = c;
}

void tb_info(const mnl_fields *F, double v[MNL_NUM_TBINFO]) {
  v[MNL_TBINFO_ACTIVE] = F->fused && F->tb_have && F->tb_enabled && F->tb_last ? 1.0 : 0.0;
  v[MNL_TBINFO_TB_CELLS] = F->tb_cells;
  v[MNL_TBINFO_TB_BORDER] = F->tb_border;
  v[MNL_TBINFO_TB_CELLS_MIXED] = F->tb_cells_nu;
  v[MNL_TBINFO_RIM_CELLS] = F->rim_cells;
  v[MNL_TBINFO_RIM_CELLS_MIXED] = F->rim_cells_nu;
  v[MNL_TBINFO_TB_ITEMS] = double(F->tb_items.size());
  v[MNL_TBINFO_RIM_ITEMS] = double(F->tb_ritems.size());
  v[MNL_TBINFO_TB_PLANES] =
      F->tb_items.empty() ? 0.0 : double((F->tb_items[0].z >> 16) - (F->tb_items[0].z & 0xFFFF));
  v[MNL_TBINFO_NARROW_ITEMS] = double(F->tb_nnarrow);
  v[MNL_TBINFO_ENABLED] = F->tb_enabled ? 1.0 : 0.0;
  v[MNL_TBINFO_TB_ZCHUNK] = double(F->tb_zchunk);
  v[MNL_TBINFO_TB_WIDTH] = double(F->tb_ox ? F->tb_ox : TB_OXW);
  v[MNL_TBINFO_TB_POL] = F->tb_pol ? 1.0 : 0.0;
}

int fields_mode(const mnl_fields *F) {
  int m = std::min(F->contig_fallbacks, 255) << MNL_MODE_FALLBACKS_SHIFT;
  if (F->contig) m |= MNL_MODE_CONTIG;
  if (F->fused) m |= MNL_MODE_FUSED | MNL_MODE_TILE;
  if (F->fused && F->d_uidx) m |= MNL_MODE_PALETTE;
  if (F->fused && F->fused_concurrent) m |= MNL_MODE_CONCURRENT;
  return m;
}

}  // namespace mnlh
