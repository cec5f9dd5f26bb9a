// mnl_fused.cpp -- planning of the fused step (DESIGN.md "Fused step"): the tile / general item
// lists, whether a run can step fused, the PML tables and chi1inv palette of the fused kernels,
// entering and leaving the mode, and the kernels' arguments.
#include "mnl_host.hpp"

namespace mnlh {

// ------------------------------------------------------------- fused mode
// G = [0, N-2] per axis: every owned point except the top plane of a rank
// with an upper neighbour (its D needs the neighbour's new B first); that
// plane is the shell, stepped by the shell kernels around the halo exchange.
// L = interior box (no PML chunk along any direction) within [1, N-2]: tiles
// whose whole footprint lies in L run the lean body.
void split_range(std::vector<int> &b, int lo, int hi_excl, int step, int align) {
  // append starts covering [lo, hi_excl) in pieces of at most `step`, starts aligned
  int x = lo;
  while (x < hi_excl) {
    b.push_back(x);
    int nx = std::min(hi_excl, ((x + step) / align) * align);
    if (nx <= x) nx = std::min(hi_excl, x + step);
    x = nx;
  }
}

// directions whose PML tables are not the identity somewhere in [lo, hi] (per axis)
static int pml_dirs_in(const mnl_fields *F, const int lo[3], const int hi[3]) {
  const DevGrid &g = F->g;
  int m = 0;
  for (int d = 0; d < 3; d++) {
    if (F->h_flag[d].empty()) continue;
    for (int j = std::max(lo[d], 0); j <= std::min(hi[d], g.N[d] - 1) && !(m >> d & 1); j++)
      for (int sft = 0; sft < 2; sft++) {
        const size_t q = 2 * (size_t)(j + g.off[d]) + sft;
        if (q >= F->h_flag[d].size()) continue;
        const double kap = F->h_kap[d][q], sig = F->h_sig[d][q];
        if (F->h_flag[d][q] || kap - sig != 1.0 || kap + sig != 1.0 || F->h_siginv[d][q] != 1.0)
          m |= 1 << d;
      }
  }
  return m;
}

// Body code (bits 24-26) and OWNC flag (bit 29) of a tile item with own columns x0 .. x1,
// halo row y0 (own rows y0+1 .. y1) and planes [zs, ze): the lean body when its footprint
// lies in L, else the PML body of the directions whose tables are not the identity over the
// footprint; OWNC when a single-axis body's footprint is owned in y and z for every component.
int tile_item_code(const mnl_fields *F, const FusedArgs &a, const Box &L, int x0, int x1, int y0,
                   int y1, int zs, int ze, bool *lean) {
  const DevGrid &g = F->g;
  *lean = x0 - 1 >= L.lo[0] && x1 + 1 <= L.hi[0] && y0 >= L.lo[1] && y1 + 1 <= L.hi[1] &&
          zs - 1 >= L.lo[2] && ze <= L.hi[2];
  int body = 0;
  if (!*lean) {
    const int lo[3] = {x0 - 1, y0, zs - 1}, hi[3] = {x0 + FX, y0 + FR, ze};
    const int m = pml_dirs_in(F, lo, hi);
    body = m == 1 ? 1 : m == 2 ? 2 : m == 4 ? 3 : m == 0 ? 4 : m == 3 ? 6 : m == 5 ? 7 : 5;
  }
  int ownc = 0;
  if (body >= 1 && body <= 3) {
    const int ylo = std::max(a.osh_lo[1], a.oun_lo[1]), yhi = std::min(a.osh_hi[1], a.oun_hi[1]);
    const int zlo = std::max(a.osh_lo[2], a.oun_lo[2]), zhi = std::min(a.osh_hi[2], a.oun_hi[2]);
    ownc = (y0 >= ylo && y0 + FR <= yhi && zs - 1 >= zlo && ze <= zhi && y0 + FR <= g.N[1] - 1 &&
            ze <= g.N[2] - 1) ? 1 : 0;
  }
  return (body << 24) | (ownc << 29);
}

// Item code of a narrow x-face strip (strip_body: body 1 | OWNC | bit 30) with own columns
// x0 .. x1 (at most 16, x0 128-byte aligned), halo row y0, own rows y0+1 .. y1 (at most 63)
// and planes [zs, ze), or -1 when its footprint (columns x0-1 .. x1+1, rows y0 .. y1+1,
// planes zs-1 .. ze) meets PML along y or z or a point not owned in y or z.
int strip_item_code(const mnl_fields *F, const FusedArgs &a, int x0, int x1, int y0, int y1, int zs,
                    int ze) {
  const DevGrid &g = F->g;
  if (x1 - x0 + 1 > SW_N || (x0 & 15) || y1 - y0 > SR_N - 1 || y1 < y0 + 1 || ze <= zs)
    return -1;
  const int lo[3] = {x0 - 1, y0, zs - 1}, hi[3] = {x1 + 1, y1 + 1, ze};
  if (pml_dirs_in(F, lo, hi) != 1) return -1;
  const int ylo = std::max(a.osh_lo[1], a.oun_lo[1]), yhi = std::min(a.osh_hi[1], a.oun_hi[1]);
  const int zlo = std::max(a.osh_lo[2], a.oun_lo[2]), zhi = std::min(a.osh_hi[2], a.oun_hi[2]);
  if (!(y0 >= ylo && y1 + 1 <= yhi && zs - 1 >= zlo && ze <= zhi && y1 + 1 <= g.N[1] - 1 &&
        ze <= g.N[2] - 1))
    return -1;
  return (1 << 24) | (1 << 29) | (1 << 30);
}

// Fused geometry.  Tiles of the lean body's shape over all of G:
// columns in pieces of <= 64 from G.lo (128-byte aligned), rows in balanced pieces of
// <= 14, z chunks; every chunk whose footprint (planes zs-1 .. ze) misses the
// polarization boxes' z range is stepped by the tile kernel, one item per (tile, chunk),
// with the body its footprint needs (lean inside L, else the PML body of the directions
// whose tables are not the identity there).  The remaining (polarization) chunks keep the
// general kernel's items (wide tiles).  Multi-rank: chunk 0 = planes 0..1 (the B the
// lower neighbour needs), launched first.
static bool make_fused_boxes(mnl_fields *F) {
  const DevGrid &g = F->g;
  Box G, L;
  for (int k = 0; k < 3; k++) {
    G.lo[k] = 0;
    G.hi[k] = g.N[k] - 2;
    if (G.hi[k] < G.lo[k]) return false;
    L.lo[k] = std::max(F->interior.lo[k], 1);
    L.hi[k] = std::min(F->interior.hi[k], g.N[k] - 2);
  }
  if (F->interior.hi[0] < F->interior.lo[0])
    for (int k = 0; k < 3; k++) L.lo[k] = 1, L.hi[k] = 0;
  F->fusedG = G;
  F->fusedL = L;
  FusedArgs &a = F->fgeo;
  memset(&a, 0, sizeof(a));
  a.G = G;
  a.L = L;
  std::vector<int> xb, yb, zb, gyb;
  split_range(xb, G.lo[0], G.hi[0] + 1, FX, 16);
  {
    const int ny = G.hi[1] - G.lo[1] + 1, nt = (ny + FOWN - 1) / FOWN;
    for (int t = 0; t < nt; t++) yb.push_back(G.lo[1] + (int)((long long)ny * t / nt));
  }
  int pzl = INT32_MAX, pzh = -1;
  for (int k = 0; k < F->f.npol; k++)
    if (F->f.pol[k].nz.lo[2] <= F->f.pol[k].nz.hi[2]) {
      pzl = std::min(pzl, F->f.pol[k].nz.lo[2]);
      pzh = std::max(pzh, F->f.pol[k].nz.hi[2]);
    }
  // z segments: [lo, hi) with a flag "polarization chunk"
  // (cut at plane 2 on multi-rank runs so that chunk 0 = planes 0..1, and at the ends of
  // the polarization chunks [pzl-1, pzh+2), the planes whose tile footprint would meet
  // the polarization boxes)
  std::vector<std::pair<std::pair<int, int>, bool>> seg;
  {
    const int z0 = G.lo[2], zend = G.hi[2] + 1;
    const int p0 = pzh >= 0 ? std::max(z0, pzl - 1) : zend, p1 = pzh >= 0 ? std::min(zend, pzh + 2) : zend;
    std::vector<int> cut = {z0, zend};
    if (F->nranks > 1 && zend - z0 > 2) cut.push_back(z0 + 2);
    // the lean box's z range: chunks from L.lo+1 to L.hi can run the lean body (their
    // halo planes lie in L), the ones outside hold the z-PML planes (short PML items)
    if (L.lo[2] <= L.hi[2]) {
      if (L.lo[2] + 1 > z0 && L.lo[2] + 1 < zend) cut.push_back(L.lo[2] + 1);
      if (L.hi[2] > z0 && L.hi[2] < zend) cut.push_back(L.hi[2]);
    }
    if (p0 < p1) cut.push_back(p0), cut.push_back(p1);
    std::sort(cut.begin(), cut.end());
    cut.erase(std::unique(cut.begin(), cut.end()), cut.end());
    for (size_t i = 0; i + 1 < cut.size(); i++)
      seg.push_back({{cut[i], cut[i + 1]}, cut[i] >= p0 && cut[i + 1] <= p1 && p0 < p1});
  }
  // chunk length: MNL_FUSED_ZCHUNK, else the candidate whose item count fills whole
  // rounds of one workgroup per CU best (with the halo-plane overhead 1 / planes)
  const long long ntile = (long long)xb.size() * yb.size();
  int zc = F->fused_zchunk > 0 ? std::min(F->fused_zchunk, FUSED_MAXCH) : 24;
  if (F->fused_zchunk <= 0) {
    const long long cus = std::max(1, k_cu_count());
    double best = -1;
    for (int cand : {12, 14, 16, 18, 20, 22, 24, 28, 32}) {
      long long nch = 0, planes = 0;
      for (auto &sg : seg) {
        if (sg.second) continue;
        nch += (sg.first.second - sg.first.first + cand - 1) / cand;
        planes += sg.first.second - sg.first.first;
      }
      if (nch == 0) break;
      const long long items = ntile * nch;
      const double fill = double(items) / double(((items + cus - 1) / cus) * cus);
      const double per = double(planes) / double(nch);
      const double score = fill * per / (per + 1.0);
      if (score >= best - 1e-12) best = score, zc = cand;
    }
  }
  // polarization chunks (general kernel, wide tiles): short enough that their items
  // number at least two per CU
  int pzc = FUSED_MAXCH;
  {
    const long long per_chunk = (long long)xb.size() *
                                ((G.hi[1] - G.lo[1] + FUSED_GW_ROWS) / FUSED_GW_ROWS);
    long long pplanes = 0;
    for (auto &sg : seg)
      if (sg.second) pplanes += sg.first.second - sg.first.first;
    if (pplanes > 0) {
      const long long want = 2LL * std::max(1, k_cu_count());
      const long long nch = std::max(1LL, (want + per_chunk - 1) / per_chunk);
      pzc = (int)std::max(4LL, std::min<long long>(FUSED_MAXCH, (pplanes + nch - 1) / nch));
    }
  }
  std::vector<char> polch;
  auto split_bal = [&](int lo, int hi, int step, bool pol) {  // balanced pieces of <= step
    const int n = hi - lo, nt = (n + step - 1) / step;
    for (int t = 0; t < nt; t++) {
      zb.push_back(lo + (int)((long long)n * t / nt));
      polch.push_back(pol);
    }
  };
  for (auto &sg : seg) split_bal(sg.first.first, sg.first.second, sg.second ? pzc : zc, sg.second);
  split_range(gyb, G.lo[1], G.hi[1] + 1, FUSED_GW_ROWS, 1);
  if ((int)xb.size() > FUSED_MAXX || (int)yb.size() > FUSED_MAXY ||
      (int)gyb.size() > FUSED_MAXGY || (int)zb.size() > FUSED_MAXZ)
    return false;
  a.nx = (int)xb.size();
  a.ny = (int)yb.size();
  a.ngy = (int)gyb.size();
  a.nch = (int)zb.size();
  for (size_t i = 0; i < xb.size(); i++) a.xb[i] = xb[i];
  a.xb[xb.size()] = G.hi[0] + 1;
  for (size_t i = 0; i < yb.size(); i++) a.yb[i] = yb[i];
  a.yb[yb.size()] = G.hi[1] + 1;
  for (size_t i = 0; i < gyb.size(); i++) a.gyb[i] = gyb[i];
  a.gyb[gyb.size()] = G.hi[1] + 1;
  for (size_t i = 0; i < zb.size(); i++) a.zb[i] = zb[i];
  a.zb[zb.size()] = G.hi[2] + 1;
  for (int k = 0; k < 3; k++) {
    a.N[k] = g.N[k];
    a.off[k] = g.off[k];
    a.osh_lo[k] = g.owned_lo_sh[k];
    a.osh_hi[k] = std::min(g.owned_hi_sh[k], G.hi[k]);
    a.oun_lo[k] = g.owned_lo_un[k];
    a.oun_hi[k] = std::min(g.owned_hi_un[k], G.hi[k]);
  }
  // ---- tile items
  F->titems.clear();
  F->gitems.clear();
  F->tile_cells = F->gen_cells = 0;
  F->tile_z.assign(std::max(g.N[2], 1), 0);
  std::vector<int> early, heavy, lean, gen_e, gen_r;
  for (int ch = 0; ch < a.nch; ch++) {
    const int zs = a.zb[ch], ze = a.zb[ch + 1];
    if (polch[ch]) {
      for (int ty = 0; ty < a.ngy; ty++)
        for (int tx = 0; tx < a.nx; tx++) {
          const int y0 = a.gyb[ty] - 1;
          const int lo[3] = {a.xb[tx] - 1, y0, zs - 1};
          const int hi[3] = {a.xb[tx] + FX, y0 + FUSED_GW_ROWS + 1, ze + 1};
          const int m = pml_dirs_in(F, lo, hi);
          const int v = tx | (ty << 8) | (ch << 16) |
                        (((m & ~2) == 0 ? 2 : (m & ~4) == 0 ? 4 : 7) << 24);
          F->gen_cells += (long long)(a.xb[tx + 1] - a.xb[tx]) * (a.gyb[ty + 1] - a.gyb[ty]) *
                          (ze - zs);
          (ch == 0 ? gen_e : gen_r).push_back(v);
        }
      continue;
    }
    for (int z = zs; z < ze; z++) F->tile_z[z] = 1;
    for (int ty = 0; ty < a.ny; ty++)
      for (int tx = 0; tx < a.nx; tx++) {
        const int x0 = a.xb[tx], x1 = a.xb[tx + 1] - 1, y0 = a.yb[ty] - 1, y1 = a.yb[ty + 1] - 1;
        const long long cells = (long long)(x1 - x0 + 1) * (y1 - y0) * (ze - zs);
        F->tile_cells += cells;
        bool in_l;
        const int code = tile_item_code(F, a, L, x0, x1, y0, y1, zs, ze, &in_l);
        const int body = (code >> 24) & 7;
        const int v = tx | (ty << 8) | (ch << 16) | code;
        if (F->nranks > 1 && ch == 0)
          early.push_back(v);
        else
          (body ? heavy : lean).push_back(v);
      }
  }
  auto planes = [&](int v) { const int ch = (v >> 16) & 255; return a.zb[ch + 1] - a.zb[ch]; };
  auto longest_first = [&](std::vector<int> &v) {
    std::stable_sort(v.begin(), v.end(), [&](int x, int y) { return planes(x) > planes(y); });
  };
  longest_first(heavy);
  longest_first(lean);
  if (F->tile_stats) {  // per-body item / cell counts (diagnostics)
    long long ni[8] = {0}, nc[8] = {0};
    for (auto *v : {&early, &heavy, &lean})
      for (int it : *v) {
        const int b = (it >> 24) & 7, tx = it & 255, ty = (it >> 8) & 255, ch = (it >> 16) & 255;
        ni[b]++;
        nc[b] += (long long)(a.xb[tx + 1] - a.xb[tx]) * (a.yb[ty + 1] - a.yb[ty]) *
                 (a.zb[ch + 1] - a.zb[ch]);
      }
    fprintf(stderr, "tile: nx %d ny %d nch %d zc %d pzc %d gen %zu+%zu\n", a.nx, a.ny, a.nch, zc,
            pzc, gen_e.size(), gen_r.size());
    for (int b = 0; b < 8; b++) fprintf(stderr, "tile body %d: %lld items %lld cells\n", b, ni[b], nc[b]);
  }
  F->titems = early;
  F->titems.insert(F->titems.end(), heavy.begin(), heavy.end());
  F->titems.insert(F->titems.end(), lean.begin(), lean.end());
  a.ntit = (int)F->titems.size();
  a.ntit_e = (int)early.size();
  longest_first(gen_r);
  F->gitems = gen_e;
  F->gitems.insert(F->gitems.end(), gen_r.begin(), gen_r.end());
  a.ngen = (int)F->gitems.size();
  a.ngen_e = (int)gen_e.size();
  // ---- shell: the top plane of a rank with an upper neighbour
  BoxList &bl = F->fused_shell;
  memset(&bl, 0, sizeof(bl));
  if (F->nranks > 1 && F->rank + 1 < F->nranks) {
    Box b;
    for (int k = 0; k < 3; k++) b.lo[k] = 0, b.hi[k] = g.N[k] - 1;
    b.lo[2] = b.hi[2] = g.N[2] - 1;
    bl.b[0] = b;
    bl.start[0] = 0;
    bl.start[1] = (long long)g.N[0] * g.N[1];
    bl.n = 1;
  }
  // ... and the top plane of every periodic axis (one rank): plane n of the unshifted
  // components is owned there, and its D needs the wrapped B / H of plane 0 first.  The boxes
  // are disjoint: a later one leaves out the planes of the earlier ones.
  if (F->nranks == 1 && any_periodic(F)) {
    Box cur;
    for (int k = 0; k < 3; k++) cur.lo[k] = 0, cur.hi[k] = g.N[k] - 1;
    long long acc = 0;
    for (int k = 2; k >= 0; k--) {  // 3-D: device axis k is direction k
      if (!F->periodic[k]) continue;
      Box b = cur;
      b.lo[k] = b.hi[k] = g.N[k] - 1;
      bl.b[bl.n] = b;
      bl.start[bl.n] = acc;
      acc += (long long)(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1) * (b.hi[2] - b.lo[2] + 1);
      bl.n++;
      cur.hi[k] = g.N[k] - 2;
    }
    bl.start[bl.n] = acc;
  }
  return true;
}

// E of component c at global point jg is implicit (chi1inv * D) in fused mode
bool in_fused_box(const mnl_fields *F, int c, const int jg[3]) {
  if (!F->fused || ctype(c) != T_E) return false;
  const DevGrid &g = F->g;
  const int d = cdir(c);
  for (int e = 0; e < 3; e++) {
    if (g.ax[e] < 0) continue;
    const int j = jg[e] - g.off[e];
    if (j < F->fusedG.lo[g.ax[e]] || j > F->fusedG.hi[g.ax[e]]) return false;
    const bool sh = e == d;
    if (sh ? (j < g.owned_lo_sh[e] || j > g.owned_hi_sh[e])
           : (j < g.owned_lo_un[e] || j > g.owned_hi_un[e]))
      return false;
  }
  for (int k = 0; k < F->f.npol; k++) {  // E is stored inside the polarization boxes
    const Box &b = F->f.pol[k].nz;
    bool in = true;
    for (int e = 0; e < 3; e++) {
      const int j = g.ax[e] >= 0 ? jg[e] - g.off[e] : 0;
      in = in && j >= b.lo[e] && j <= b.hi[e];
    }
    if (in) return false;
  }
  const int q = 2 * jg[d] + 1;  // E_d is shifted along d
  return !(F->S.has[d] && F->h_flag[d][q]);
}

// chi(2) Newton-Raphson in the fused mode (one rank): the fused kernels store D everywhere
// and leave E and P of the chi2 box grown by one point (the NR neighbour reads of D - P,
// src/step_generic.cpp:740-743, stay inside it) to the NR E kernel; that box must lie in the
// interior (no PML, no wall plane) and inside the polarization box, where the fused
// kernels store E (elsewhere E is implicit and the NR kernel's stores would be lost)
static bool nr_fused_ok(mnl_fields *F) {
  if (F->nranks > 1 || F->f.npol == 0) return false;
  if (nr_split(F)) return false;
  Box &x = F->nr_xbox;
  const Box &c = F->nr_chi2;
  if (c.hi[0] < c.lo[0] || c.hi[1] < c.lo[1] || c.hi[2] < c.lo[2]) {  // no chi2 point
    for (int k = 0; k < 3; k++) x.lo[k] = 1, x.hi[k] = 0;
    return true;
  }
  Box p;
  for (int k = 0; k < 3; k++) p.lo[k] = INT32_MAX, p.hi[k] = -1;
  for (int q = 0; q < F->f.npol; q++)
    for (int k = 0; k < 3; k++) {
      p.lo[k] = std::min(p.lo[k], F->f.pol[q].nz.lo[k]);
      p.hi[k] = std::max(p.hi[k], F->f.pol[q].nz.hi[k]);
    }
  for (int k = 0; k < 3; k++) {
    x.lo[k] = c.lo[k] - 1, x.hi[k] = c.hi[k] + 1;
    if (x.lo[k] < F->interior.lo[k] || x.hi[k] > F->interior.hi[k]) return false;
    if (x.lo[k] < p.lo[k] || x.hi[k] > p.hi[k]) return false;
  }
  return true;
}

static bool fused_possible(mnl_fields *F) {
  if (!F->allow_fused || F->S.dim != 3 || F->upnl || F->f.aniso || F->hall) return false;
  // periodic directions: one rank; the chi(2) box's neighbour reads
  // would need the D / P ghosts inside the fused step
  if (any_periodic(F) && (F->nranks > 1 || F->nr)) return false;
  if (F->nr && !nr_fused_ok(F)) return false;
  for (int t = 0; t < 2; t++)
    for (int d = 0; d < 3; d++)
      if (F->f.cnd[t][d]) return false;
  if (F->any_srcB || F->any_isrc || F->any_dsrc_w) return false;
  // a D source inside a polarization box would need E recomputed after it
  // (local check; fused_agreed makes the decision collective)
  for (size_t k = 0; k < F->srcD_idx.size(); k++) {
    const long long idx = F->srcD_idx[k];
    const long long i2 = idx / F->g.st[2], r = idx % F->g.st[2];
    const int j[3] = {(int)(r % F->g.st[1]), (int)(r / F->g.st[1]), (int)i2};
    for (int q = 0; q < F->f.npol; q++) {
      const Box &b = F->f.pol[q].nz;
      bool in = true;
      for (int e = 0; e < 3; e++) in = in && j[e] >= b.lo[e] && j[e] <= b.hi[e];
      if (in) return false;
    }
  }
  for (int c = 0; c < MNL_NUM_COMPONENTS; c++)
    if (!F->allocated[c]) return false;
  for (int d = 0; d < 3; d++)  // separate H wherever PML lies along its direction
    if (F->pml_any[d] && (!F->f.H[d] || !F->f.WH[d] || !F->f.WE[d])) return false;
  const int nu = (F->f.inveps[0] ? 1 : 0) + (F->f.inveps[1] ? 1 : 0) + (F->f.inveps[2] ? 1 : 0);
  if (nu != 0 && nu != 3) return false;
  // the fused kernels address arrays with 32-bit byte offsets
  if (F->nlocal * 8 >= 0xFFFFFFF0ull) return false;
  // the tile / chunk geometry is built on entering the fused mode and uploaded by
  // set_fused; every change of its inputs (z-chunk, A/B switches) leaves the mode first,
  // so a batch that is already fused reuses it (no per-call host rebuild)
  if (F->fused) return true;
  if (!make_fused_boxes(F)) return false;
  return true;
}

// fused mode only if every rank can (the ranks' exchange sequences differ by mode)
bool fused_agreed(mnl_fields *F) {
  bool ok = fused_possible(F);
  if (F->nranks > 1) {
    double v = ok ? 1.0 : 0.0;
    if (F->comm->allreduce_sum(&v, 1, F->stream)) return false;
    ok = v == double(F->nranks);
  }
  return ok;
}

// per-direction PML tables of the fused kernels (identity where no PML)
static int upload_fused_tables(mnl_fields *F) {
  if (F->d_tab.flag[0]) return 0;
  for (int d = 0; d < 3; d++) {
    const size_t nq = 2 * (size_t)std::max(F->S.n[d], 0) + 2;
    std::vector<uint8_t> fl(nq, 0);
    std::vector<double> kms(nq, 1.0), kps(nq, 1.0), si(nq, 1.0);
    if (F->S.has[d] && !F->h_flag[d].empty())
      for (size_t q = 0; q < nq; q++) {
        fl[q] = F->h_flag[d][q];
        kms[q] = F->h_kap[d][q] - F->h_sig[d][q];
        kps[q] = F->h_kap[d][q] + F->h_sig[d][q];
        si[q] = F->h_siginv[d][q];
      }
    uint8_t *dfl;
    double *dkms, *dkps, *dsi;
    if (dev_alloc(F, &dfl, nq) || dev_alloc(F, &dkms, nq) || dev_alloc(F, &dkps, nq) ||
        dev_alloc(F, &dsi, nq))
      return -1;
    HIPCHK(hipMemcpyAsync(dfl, fl.data(), nq, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(dkms, kms.data(), nq * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(dkps, kps.data(), nq * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(dsi, si.data(), nq * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    F->d_tab.flag[d] = dfl;
    F->d_tab.kms[d] = dkms;
    F->d_tab.kps[d] = dkps;
    F->d_tab.siginv[d] = dsi;
  }
  return 0;
}

// chi1inv palette for the fused kernel (DESIGN.md "chi1inv palette"): at most
// 256 distinct values per component, candidates taken from the structure (1.0
// default, user chi1inv arrays, 1/eps of geometry boxes) and verified cell by
// cell on the device (bitwise), so a missing value just disables the palette.
static int build_palette(mnl_fields *F) {
  if (F->palette_tried) return 0;
  F->palette_tried = true;
  const mnl_structure &S = F->S;
  DevFields &f = F->f;
  if (!f.inveps[0] || !f.inveps[1] || !f.inveps[2]) return 0;
  if (F->no_palette) return 0;
  std::vector<double> tab(3 * 256, 0.0);
  int n[3];
  for (int c = 0; c < 3; c++) {
    std::set<uint64_t> cand;
    auto bits = [](double v) {
      uint64_t u;
      memcpy(&u, &v, 8);
      return u;
    };
    cand.insert(bits(1.0));
    const auto &diag = S.chi1inv[c][c];
    if (!diag.empty()) {
      std::unordered_set<uint64_t> us;
      for (double v : diag) {
        us.insert(bits(v));
        if (us.size() > 256) return 0;
      }
      cand.insert(us.begin(), us.end());
    }
    for (auto &b : S.boxes)
      if (b.kind == 0) cand.insert(bits(1.0 / b.value));
    if (cand.size() > 256) return 0;
    n[c] = (int)cand.size();
    int k = 0;
    for (uint64_t u : cand) memcpy(&tab[256 * c + k++], &u, 8);  // ascending bit patterns
  }
  F->pal_one = 0;  // the entry of 1.0 (always a candidate): what a DFT sample of raw D multiplies by
  for (int c = 0; c < 3; c++)
    for (int k = 0; k < n[c]; k++)
      if (tab[256 * c + k] == 1.0) F->pal_one |= (unsigned)k << (8 * c);
  unsigned *uidx = nullptr;
  double *utab;
  int *bad;
  if (dev_alloc(F, &uidx, F->nlocal) || dev_alloc(F, &utab, 3 * 256) || dev_alloc(F, &bad, 1))
    return -1;
  HIPCHK(hipMemcpyAsync(utab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, F->stream));
  const double *u[3] = {f.inveps[0], f.inveps[1], f.inveps[2]};
  if (k_build_uidx(uidx, u, utab, n, F->fusedG, F->g.st[1], F->g.st[2], bad, F->stream))
    return fail("palette index build failed");
  int hbad = 0;
  HIPCHK(hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  if (hbad) return 0;
  F->d_uidx = uidx;
  F->d_utab = utab;
  return 0;
}

int set_fused(mnl_fields *F, bool on) {
  DevFields &f = F->f;
  if (on == F->fused) return 0;
  if (on) {
    if (!F->d_fused_ctr) {  // FUSED_NCTR work-queue counters, 128 B apart
      if (dev_alloc(F, &F->d_fused_ctr, FUSED_NCTR * 16)) return -1;
    }
    if (upload_fused_tables(F)) return -1;
    if (dev_upload(F, &F->d_gitems, F->d_gitems_cap, F->gitems) ||
        dev_upload(F, &F->d_titems, F->d_titems_cap, F->titems))
      return -1;
    if (build_palette(F)) return -1;
    // ping-pong partners; the second buffer starts as a copy (ghost / wall entries
    // that no kernel writes)
    auto pair = [&](double **pp, double *cur, double **next) -> int {
      if (!cur) return 0;
      if (!*pp && dev_alloc(F, pp, F->nlocal, false)) return -1;
      HIPCHK(hipMemcpyAsync(*pp, cur, F->nlocal * 8, hipMemcpyDeviceToDevice, F->stream));
      *next = *pp;
      return 0;
    };
    for (int d = 0; d < 3; d++) {
      if (pair(&F->pp_B[d], f.B[d], &f.Bn[d]) || pair(&F->pp_D[d], f.D[d], &f.Dn[d]) ||
          pair(&F->pp_E[d], f.E[d], &f.En[d]) || pair(&F->pp_H[d], f.H[d], &f.Hn[d]) ||
          pair(&F->pp_UB[d], f.UB[d], &f.UBn[d]))
        return -1;
    }
    f.fG = F->fusedG;
    f.fused = 1;
    F->fused_epoch++;  // the temporal-blocking plan and its middle set are rebuilt
    F->tb_mid_fresh = false;
  } else {
    // materialise implicit E and the W aux fields over G (needs f.fused == 1),
    // then step in place again
    if (k_materialize_e(F->fusedG, F->g, f, F->stream)) return fail("materialize E failed");
    for (int d = 0; d < 3; d++) {
      F->pp_B[d] = f.Bn[d];  // the non-current buffers
      F->pp_D[d] = f.Dn[d];
      if (f.E[d]) F->pp_E[d] = f.En[d];
      if (f.H[d]) F->pp_H[d] = f.Hn[d];
      if (f.UB[d]) F->pp_UB[d] = f.UBn[d];
      f.Bn[d] = f.B[d];
      f.Dn[d] = f.D[d];
      f.En[d] = f.E[d];
      f.Hn[d] = f.H[d];
      f.UBn[d] = f.UB[d];
    }
    f.fused = 0;
  }
  F->fused = on;
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

// kernel arguments of one fused step (geometry from make_fused_boxes, pointers now)
FusedArgs &fused_args(mnl_fields *F) {
  FusedArgs &fa = F->fgeo;
  const DevFields &f = F->f;
  fa.nelem = (long long)F->nlocal;
  fa.C = F->S.courant;
  fa.st1 = F->g.st[1];
  fa.st2 = F->g.st[2];
  args_sets(fa, set_cur(F), set_nxt(F));
  for (int d = 0; d < 3; d++) fa.UD[d] = f.UD[d], fa.u[d] = f.inveps[d];
  fa.tab = F->d_tab;
  fa.npol = f.npol;
  for (int k = 0; k < MAX_POL; k++) fa.pol[k] = f.pol[k];
  for (int e = 0; e < 3; e++) fa.pbox.lo[e] = INT32_MAX, fa.pbox.hi[e] = -1;
  for (int k = 0; k < f.npol; k++)
    for (int e = 0; e < 3; e++) {
      fa.pbox.lo[e] = std::min(fa.pbox.lo[e], f.pol[k].nz.lo[e]);
      fa.pbox.hi[e] = std::max(fa.pbox.hi[e], f.pol[k].nz.hi[e]);
    }
  for (int e = 0; e < 3; e++) fa.xbox.lo[e] = 1, fa.xbox.hi[e] = 0;
  if (F->nr) fa.xbox = F->nr_xbox;
  fa.gitems = F->d_gitems;
  fa.titems = F->d_titems;
  fa.tflag = nullptr;
  fa.uidx = F->d_uidx;
  fa.utab = F->d_utab;
  fa.gflag = nullptr;
  if (F->d_uidx) {
    // flags of the current tile / chunk geometry (rebuilt if make_fused_boxes changed it)
    unsigned long long sig = 1469598103934665603ULL;
    auto mix = [&](long long v) { sig = (sig ^ (unsigned long long)v) * 1099511628211ULL; };
    for (int i = 0; i <= fa.nx; i++) mix(fa.xb[i]);
    for (int i = 0; i <= fa.ny; i++) mix(fa.yb[i]);
    for (int i = 0; i <= fa.nch; i++) mix(fa.zb[i]);
    for (int k = 0; k < 3; k++) mix(fa.L.lo[k]), mix(fa.L.hi[k]);
    for (int i = 0; i <= fa.ngy; i++) mix(fa.gyb[i]);
    for (int v : F->gitems) mix(v);
    for (int v : F->titems) mix(v);
    const size_t ng = F->gitems.size(), nt = F->titems.size();
    auto grow = [](unsigned *&p, size_t &cap, size_t want) {
      if (cap >= want) return true;
      if (p) hipFree(p);
      p = nullptr;
      const bool r = hipMalloc(&p, std::max<size_t>(want, 1) * sizeof(unsigned)) == hipSuccess;
      cap = r ? want : 0;
      return r;
    };
    bool ok = true;
    if (F->uflag_sig != sig) {
      ok = grow(F->d_gflag, F->gflag_n, ng) && grow(F->d_tflag, F->tflag_n, nt) &&
           k_general_uniform(fa, F->d_gflag, F->stream) == 0 &&
           k_tile_uniform(fa, F->d_tflag, F->stream) == 0;
      F->uflag_sig = ok ? sig : 0;
      if (ok) {  // per-item cell counts of the mixed items (traffic model)
        std::vector<unsigned> hg(ng), ht(nt);
        ok = (nt == 0 || hipMemcpyAsync(ht.data(), F->d_tflag, nt * 4, hipMemcpyDeviceToHost,
                                        F->stream) == hipSuccess) &&
             (ng == 0 || hipMemcpyAsync(hg.data(), F->d_gflag, ng * 4, hipMemcpyDeviceToHost,
                                        F->stream) == hipSuccess) &&
             hipStreamSynchronize(F->stream) == hipSuccess;
        double gn = 0;
        for (size_t i = 0; ok && i < ng; i++) {
          if (hg[i] != ~0u) continue;
          const int v = F->gitems[i], tx = v & 255, ty = (v >> 8) & 255, ch = (v >> 16) & 255;
          gn += double(fa.xb[tx + 1] - fa.xb[tx]) * (fa.gyb[ty + 1] - fa.gyb[ty]) *
                (fa.zb[ch + 1] - fa.zb[ch]);
        }
        double tn = 0;
        for (size_t i = 0; ok && i < nt; i++) {
          if (ht[i] != ~0u) continue;
          const int v = F->titems[i], tx = v & 255, ty = (v >> 8) & 255, ch = (v >> 16) & 255;
          tn += double(fa.xb[tx + 1] - fa.xb[tx]) * (fa.yb[ty + 1] - fa.yb[ty]) *
                (fa.zb[ch + 1] - fa.zb[ch]);
        }
        F->gen_cells_nu = gn;
        F->tile_cells_nu = tn;
        if (!ok) F->uflag_sig = 0;
      }
    }
    if (ok) {
      fa.gflag = ng ? F->d_gflag : nullptr;
      fa.tflag = nt ? F->d_tflag : nullptr;
    }
  }
  F->uflag_active = fa.gflag || fa.tflag;
  fa.ctr = F->d_fused_ctr;
  fa.clk = ItemClock{F->d_clk, F->d_clk_n, F->d_clk ? CLK_CAP : 0u, 0};
  return fa;
}

}  // namespace mnlh
