// mnl_tb.cpp -- temporal blocking: the plan of a pair of steps, its middle buffer set, and the
// pair's launch sequences on one rank and on a rank with neighbours.
#include "mnl_host.hpp"

namespace mnlh {

// ------------------------------------------------------------ temporal blocking
// (DESIGN.md section 24).  Two steps n -> n+2 of a one-rank fused run as three launches over
// three buffer sets (cur = state n, mid, nxt):
//   R1: the tile kernel over the rim items, cur -> mid (state n+1 on the rim);
//   source(n) into mid;
//   L:  the two-step kernel over the L2 items, cur -> nxt (state n+2), plus the state n+1 of
//       the L2 points on a face that borders the rim, into mid;
//   R2: the tile kernel over the rim items, mid -> nxt;  source(n+1) into nxt.
// L2 = the lean box shrunk by 2 minus boxes around the source points, so every value the
// two-step march computes is the lean body's (same expression, same operands): the pair is
// bitwise two one-step launches.  The rim is everything else of G: PML, walls, the ring of
// width >= 2 inside the lean box and the holes.

static bool box_meets(const Box &a, const Box &b) {
  for (int k = 0; k < 3; k++)
    if (a.hi[k] < b.lo[k] || b.hi[k] < a.lo[k]) return false;
  return true;
}

// Disjoint boxes of G: `two` covers L2 minus the holes, `rim` the rest.  Cells of the grid of
// all box bounds, merged into x runs, then along y, then along z.
static void tb_regions(const Box &G, const Box &L2, const std::vector<Box> &holes,
                       std::vector<Box> &two, std::vector<Box> &rim) {
  std::vector<int> cut[3];
  for (int k = 0; k < 3; k++) {
    std::vector<int> &c = cut[k];
    c = {G.lo[k], G.hi[k] + 1, L2.lo[k], L2.hi[k] + 1};
    for (const Box &h : holes) c.push_back(h.lo[k]), c.push_back(h.hi[k] + 1);
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    c.erase(std::remove_if(c.begin(), c.end(), [&](int v) { return v < G.lo[k] || v > G.hi[k] + 1; }),
            c.end());
  }
  auto is_two = [&](int x, int y, int z) {
    const int p[3] = {x, y, z};
    for (int k = 0; k < 3; k++)
      if (p[k] < L2.lo[k] || p[k] > L2.hi[k]) return false;
    for (const Box &h : holes) {
      bool in = true;
      for (int k = 0; k < 3; k++) in = in && p[k] >= h.lo[k] && p[k] <= h.hi[k];
      if (in) return false;
    }
    return true;
  };
  std::vector<Box> out[2];
  const int nx = (int)cut[0].size() - 1, ny = (int)cut[1].size() - 1, nz = (int)cut[2].size() - 1;
  for (int l = 0; l < nz; l++)
    for (int j = 0; j < ny; j++)
      for (int i = 0; i < nx;) {
        const bool c = is_two(cut[0][i], cut[1][j], cut[2][l]);
        int i2 = i;
        while (i2 + 1 < nx && is_two(cut[0][i2 + 1], cut[1][j], cut[2][l]) == c) i2++;
        Box b;
        b.lo[0] = cut[0][i], b.hi[0] = cut[0][i2 + 1] - 1;
        b.lo[1] = cut[1][j], b.hi[1] = cut[1][j + 1] - 1;
        b.lo[2] = cut[2][l], b.hi[2] = cut[2][l + 1] - 1;
        out[c ? 1 : 0].push_back(b);
        i = i2 + 1;
      }
  auto merge = [](std::vector<Box> &v, int ax) {
    for (bool changed = true; changed;) {
      changed = false;
      for (size_t a = 0; a < v.size() && !changed; a++)
        for (size_t b = 0; b < v.size(); b++) {
          if (a == b || v[b].lo[ax] != v[a].hi[ax] + 1) continue;
          bool ok = true;
          for (int k = 0; k < 3 && ok; k++)
            if (k != ax) ok = v[a].lo[k] == v[b].lo[k] && v[a].hi[k] == v[b].hi[k];
          if (!ok) continue;
          v[a].hi[ax] = v[b].hi[ax];
          v.erase(v.begin() + (long)b);
          changed = true;
          break;
        }
    }
  };
  for (auto *v : {&out[0], &out[1]}) merge(*v, 1), merge(*v, 2);
  rim.swap(out[0]);
  two.swap(out[1]);
}

// Build (or keep) the plan of the current fused geometry and source points.  No plan (tb_have
// false) when L2 is empty or an item would not fit the kernels' shapes.
static int tb_plan(mnl_fields *F) {
  unsigned long long sig = 1469598103934665603ULL;
  auto mix = [&](long long v) { sig = (sig ^ (unsigned long long)v) * 1099511628211ULL; };
  mix(F->fused_epoch), mix(F->tb_zchunk), mix(F->fused_zchunk), mix((long long)F->nlocal);
  mix(F->rim_zchunk), mix(F->tb_ox), mix(F->tb_pol_on);
  mix((long long)F->srcD_idx.size());
  for (long long v : F->srcD_idx) mix(v);
  // DFT monitors (one rank): the Yee points their samples average, +1 along every axis --
  // the two-step items store step n+1 there too (the middle-step sample reads the mid set)
  std::vector<Box> dbox;
  std::vector<DftFluxH *> cmon;  // monitors whose box the two-step kernel stores compactly
  for (DftFluxH *op : F->sampled) {  // (built once per monitor: this runs every batch)
    if (op->bbox.hi[0] < 0) continue;
    if (op->kind == DFT_LDOS && !op->ld->rec) continue;  // idle: no step samples it
    if (F->dft_cmp && op->cmp_cells && (int)cmon.size() < TB_MAXCMP)
      cmon.push_back(op);
    else
      dbox.push_back(op->bbox);
  }
  mix((long long)cmon.size());
  for (auto *o : cmon)
    for (int k = 0; k < 3; k++) mix(o->bbox.lo[k]), mix(o->bbox.hi[k]);
  // the NaN guard's points (it checks the middle state of every pair, src/step.cpp:138-139)
  if (F->nan_terms.n > 0) {
    Box nb;
    for (int i = 0; i < F->nan_terms.n; i++) {
      const long long li = F->nan_terms.idx[i];
      const int p[3] = {(int)(li % F->g.st[1]), (int)((li % F->g.st[2]) / F->g.st[1]),
                        (int)(li / F->g.st[2])};
      for (int k = 0; k < 3; k++) {
        nb.lo[k] = i ? std::min(nb.lo[k], p[k]) : p[k];
        nb.hi[k] = i ? std::max(nb.hi[k], p[k]) : p[k];
      }
    }
    dbox.push_back(nb);
  }
  mix((long long)dbox.size());
  for (const Box &b : dbox)
    for (int k = 0; k < 3; k++) mix(b.lo[k]), mix(b.hi[k]);
  if (sig == F->tb_sig) return 0;
  F->tb_sig = sig;
  F->tb_have = false;
  F->tb_ritems.clear(), F->tb_rgeo.clear(), F->tb_items.clear();
  // compact DFT boxes: allocated once, emptied (DFT_CMP_EMPTY) with every new plan
  F->tb_cmp.clear();
  for (DftFluxH *op : F->sampled) op->cmp_on = false;
  for (auto *o : cmon) {
    const size_t nd = (size_t)12 * o->cmp_cells;
    if (!o->d_cmp && hipMalloc(&o->d_cmp, nd * 8) != hipSuccess) {
      (void)hipGetLastError();
      o->d_cmp = nullptr;
      dbox.push_back(o->bbox);  // no memory for it: the middle state in mid, as before
      continue;
    }
    double empty;
    const unsigned long long e = DFT_CMP_EMPTY;
    memcpy(&empty, &e, 8);
    if (k_fill(o->d_cmp, empty, nd, F->stream)) return fail("fill launch failed");
    TBCmp c{};
    for (int k = 0; k < 3; k++) c.lo[k] = o->bbox.lo[k], c.n[k] = o->bbox.hi[k] - o->bbox.lo[k] + 1;
    c.p = o->d_cmp, c.mask = o->cmp_mask, c.ncell = o->cmp_cells;
    F->tb_cmp.push_back(c);
    o->cmp_on = true;
  }
  const Box &G = F->fusedG, &L = F->fusedL;
  const FusedArgs &a = F->fgeo;
  const DevGrid &g = F->g;
  if (F->S.dim != 3 || g.N[0] > 65535 || g.N[1] > 65535 || g.N[2] > 65535) return 0;
  Box L2;
  for (int k = 0; k < 3; k++) L2.lo[k] = L.lo[k] + 2, L2.hi[k] = L.hi[k] - 2;
  // x: the rim to the right of L2 starts on a 128-byte boundary (tile-kernel items); the rim
  // to the left ends on one when that costs no more columns than starting the two-step tiles
  // 4 columns past a 64-byte boundary (their lanes' line) -- a 16-column left rim runs as
  // narrow strips (strip_body), and the first two-step tile of a row starts its lanes on the
  // line below its own columns
  {
    const int a16 = G.lo[0] + (L2.lo[0] - G.lo[0] + 15) / 16 * 16;
    const int a4 = L2.lo[0] + ((4 - L2.lo[0]) % 8 + 8) % 8;
    L2.lo[0] = (F->tb_narrow && a16 <= a4) ? a16 : a4;
  }
  L2.hi[0] = (L2.hi[0] + 1) / 16 * 16 - 1;
  bool l2 = true;
  for (int k = 0; k < 3; k++) l2 = l2 && L2.hi[k] - L2.lo[k] >= 7;
  // one rank: no two-step region, no pairs.  Multi-rank: a rank without one (thin slab, PML)
  // still steps pairs as two rim launches (every rank runs the same exchange sequence)
  if (!l2 && F->nranks == 1) {
    if (F->tb_stats) fprintf(stderr, "tb: L2 empty\n");
    return 0;
  }
  if (!l2)
    for (int k = 0; k < 3; k++) L2.lo[k] = 1, L2.hi[k] = 0;
  // holes: no source point within distance 1 of a two-step own point (the march's D^{n+1}
  // would miss the current); a box of +-2 for margin, x widened to the alignments above and
  // to the L2 edge when that leaves fewer than 8 columns
  std::vector<Box> holes;
  for (long long idx : F->srcD_idx) {
    const long long i2 = idx / g.st[2], r = idx % g.st[2];
    const int s[3] = {(int)(r % g.st[1]), (int)(r / g.st[1]), (int)i2};
    Box h;
    for (int k = 0; k < 3; k++) h.lo[k] = s[k] - 2, h.hi[k] = s[k] + 2;
    if (!l2 || !box_meets(h, L2)) continue;
    h.lo[0] = std::max(h.lo[0], 0) / 16 * 16;
    while ((h.hi[0] + 1) % 8 != 4) h.hi[0]++;
    for (int k = 0; k < 3; k++) h.lo[k] = std::max(h.lo[k], L2.lo[k]), h.hi[k] = std::min(h.hi[k], L2.hi[k]);
    if (h.lo[0] - L2.lo[0] < 8) h.lo[0] = L2.lo[0];
    if (L2.hi[0] - h.hi[0] < 8) h.hi[0] = L2.hi[0];
    holes.push_back(h);
  }
  // polarization chunks (the planes [pzl - 1, pzh + 2) over the whole x-y extent of
  // G, make_fused_boxes): stepped by the general kernel, not by rim items; no two-step point
  // within distance 2 of them (their E is stored, not chi1inv D)
  Box P;
  bool have_p = false;
  if (F->f.npol > 0 && a.ngen > 0) {
    int pzl = INT32_MAX, pzh = -1;
    for (int k = 0; k < F->f.npol; k++)
      if (F->f.pol[k].nz.lo[2] <= F->f.pol[k].nz.hi[2]) {
        pzl = std::min(pzl, F->f.pol[k].nz.lo[2]);
        pzh = std::max(pzh, F->f.pol[k].nz.hi[2]);
      }
    if (pzh >= 0) {
      P = G;
      P.lo[2] = std::max(G.lo[2], pzl - 1), P.hi[2] = std::min(G.hi[2], pzh + 1);
      have_p = P.lo[2] <= P.hi[2];
    }
    if (have_p && l2) {
      Box h = L2;
      h.lo[2] = std::max(L2.lo[2], P.lo[2] - 2), h.hi[2] = std::min(L2.hi[2], P.hi[2] + 2);
      if (h.lo[2] <= h.hi[2]) holes.push_back(h);
    }
  }
  F->tb_pol = have_p;
  std::vector<Box> two, rim;
  if (l2) {
    tb_regions(G, L2, holes, two, rim);
  } else {
    rim.push_back(G);
  }
  if (have_p) {  // rim boxes minus P
    std::vector<Box> keep;
    for (const Box &b : rim) {
      if (!box_meets(b, P)) {
        keep.push_back(b);
        continue;
      }
      std::vector<Box> part, inside;
      tb_regions(b, b, {P}, part, inside);
      keep.insert(keep.end(), part.begin(), part.end());
    }
    rim.swap(keep);
  }
  if (two.empty() && F->nranks == 1) return 0;
  // ---- rim items: tile-kernel shapes (columns <= 64 from 128-byte boundaries, rows <= 14,
  // chunks <= zc cut at the lean box's z range), bodies as make_fused_boxes
  // planes per rim item: its own setting (tuned with pairs), else the one-step chunk length
  const int zc = F->rim_zchunk > 0 ? std::min(F->rim_zchunk, FUSED_MAXCH)
                 : F->fused_zchunk > 0 ? std::min(F->fused_zchunk, FUSED_MAXCH) : 24;
  struct RI {
    int code, g0, g1, g2, g3, planes;
    bool dep;  // multi-rank: reads the ghost plane 0 or the top plane N-1 (slab-face data)
  };
  const bool lower = F->rank > 0, upper = F->rank + 1 < F->nranks;
  const int N2 = g.N[2];
  std::vector<std::array<int, 3>> spts;  // D source points (local indices)
  for (long long idx : F->srcD_idx) {
    const long long i2 = idx / g.st[2], r = idx % g.st[2];
    spts.push_back({(int)(r % g.st[1]), (int)(r / g.st[1]), (int)i2});
  }
  std::vector<RI> heavy, lean;
  F->rim_cells = F->rim_lean = 0;
  F->tb_nnarrow = 0;
  // a column box (x fixed, rows / planes inclusive) of two-step points
  auto col_two = [&](int x, int ylo, int yhi, int zlo, int zhi) {
    if (!l2 || x < L2.lo[0] || x > L2.hi[0] || ylo < L2.lo[1] || yhi > L2.hi[1] || zlo < L2.lo[2] ||
        zhi > L2.hi[2])
      return false;
    Box c;
    c.lo[0] = c.hi[0] = x, c.lo[1] = ylo, c.hi[1] = yhi, c.lo[2] = zlo, c.hi[2] = zhi;
    for (const Box &h : holes)
      if (box_meets(c, h)) return false;
    return true;
  };
  for (const Box &b : rim) {
    if (b.lo[0] % 16) {  // cannot happen with the alignments above
      if (F->tb_stats) fprintf(stderr, "tb: rim box at x %d not 128-byte aligned\n", b.lo[0]);
      return 0;
    }
    std::vector<int> xs, zs;
    split_range(xs, b.lo[0], b.hi[0] + 1, FX, 16);
    xs.push_back(b.hi[0] + 1);
    // a 16-column x-face box whose x-1 column is outside the grid or two-step: narrow strips
    const bool narrow = F->tb_narrow && b.hi[0] - b.lo[0] + 1 == SW_N &&
                        (b.lo[0] == 0 || col_two(b.lo[0] - 1, b.lo[1], b.hi[1], b.lo[2], b.hi[2]));
    std::vector<int> zcut = {b.lo[2], b.hi[2] + 1};
    // cuts at the lean box's z range (lean bodies for the planes inside it), unless a piece
    // would be thinner than 4 planes (the ring between L and L2: a 1-2-plane item costs more
    // per cell as a lean item than inside its PML neighbour); slab-face cuts always
    for (int v : {L.lo[2] + 1, L.hi[2]})
      if (v - b.lo[2] >= 4 && b.hi[2] + 1 - v >= 4) zcut.push_back(v);
    for (int v : {lower ? 2 : -1, upper ? N2 - 2 : -1})
      if (v > b.lo[2] && v < b.hi[2] + 1) zcut.push_back(v);
    std::sort(zcut.begin(), zcut.end());
    zcut.erase(std::unique(zcut.begin(), zcut.end()), zcut.end());
    std::sort(zcut.begin(), zcut.end());
    for (size_t s = 0; s + 1 < zcut.size(); s++) {
      const int n = zcut[s + 1] - zcut[s], nt = (n + zc - 1) / zc;
      for (int t = 0; t < nt; t++) zs.push_back(zcut[s] + (int)((long long)n * t / nt));
    }
    zs.push_back(b.hi[2] + 1);
    if (narrow) {
      const int ny = b.hi[1] - b.lo[1] + 1, nty = (ny + (SR_N - 1) - 1) / (SR_N - 1);
      std::vector<RI> items;
      bool ok = true;
      for (size_t iz = 0; iz + 1 < zs.size() && ok; iz++)
        for (int ty = 0; ty < nty && ok; ty++) {
          const int x0 = b.lo[0], x1 = b.hi[0];
          const int yf = b.lo[1] + (int)((long long)ny * ty / nty);
          const int y1 = b.lo[1] + (int)((long long)ny * (ty + 1) / nty) - 1;
          const int z0 = zs[iz], z1 = zs[iz + 1];
          const int code = strip_item_code(F, a, x0, x1, yf - 1, y1, z0, z1);
          if (code < 0) {
            ok = false;
            break;
          }
          bool src_in = false;
          if (F->nranks > 1)
            for (const auto &sp : spts)
              src_in = src_in || (sp[0] >= x0 - 1 && sp[0] <= x1 + 1 && sp[1] >= yf - 1 &&
                                  sp[1] <= y1 + 1 && sp[2] >= z0 - 1 && sp[2] <= z1);
          items.push_back(RI{code, x0 | (x1 << 16), yf | (y1 << 16), z0 | (z1 << 16), -1, z1 - z0,
                             (lower && z0 <= 1) || (upper && z1 >= N2 - 1) || src_in});
        }
      if (ok) {
        for (const RI &it : items) {
          heavy.push_back(it);
          F->rim_cells += double(SW_N) * (((it.g1 >> 16) - (it.g1 & 0xFFFF)) + 1) * it.planes;
        }
        F->tb_nnarrow += (int)items.size();
        continue;
      }
    }
    const int ny = b.hi[1] - b.lo[1] + 1, nty = (ny + FOWN - 1) / FOWN;
    for (size_t iz = 0; iz + 1 < zs.size(); iz++)
      for (int ty = 0; ty < nty; ty++)
        for (size_t ix = 0; ix + 1 < xs.size(); ix++) {
          const int x0 = xs[ix], x1 = xs[ix + 1] - 1;
          const int yf = b.lo[1] + (int)((long long)ny * ty / nty);
          const int y1 = b.lo[1] + (int)((long long)ny * (ty + 1) / nty) - 1;
          const int z0 = zs[iz], z1 = zs[iz + 1];
          bool in_l;
          const int code = tile_item_code(F, a, L, x0, x1, yf - 1, y1, z0, z1, &in_l);
          const double cells = double(x1 - x0 + 1) * (y1 - yf + 1) * (z1 - z0);
          F->rim_cells += cells;
          if (in_l) F->rim_lean += cells;
          // multi-rank: the sources are applied after the top plane's step (slab-face
          // chain), so items holding a source point wait for it too
          bool src_in = false;  // in the footprint (E = chi1inv * D of a neighbour)
          if (F->nranks > 1)
            for (const auto &sp : spts)
              src_in = src_in || (sp[0] >= x0 - 1 && sp[0] <= x1 + 1 && sp[1] >= yf - 1 &&
                                  sp[1] <= y1 + 1 && sp[2] >= z0 - 1 && sp[2] <= z1);
          RI it{code, x0 | (x1 << 16), yf | (y1 << 16), z0 | (z1 << 16), -1, z1 - z0,
                (lower && z0 <= 1) || (upper && z1 >= N2 - 1) || src_in};
          (((code >> 24) & 7) ? heavy : lean).push_back(it);
        }
  }
  // x-face strips of at most 32 columns (the rim left and right of L2) with the same rows,
  // planes and body (AX = 1) share one workgroup in pairs (pml_body<PAIR>): a narrow item
  // costs about a whole tile's time per plane (one dependent round per plane; unpaired strips
  // measured 2.55 against 2.37 ms/step at 512^3, round 4)
  {
    std::vector<RI> keep;
    std::vector<size_t> open;  // unpaired strips, by (rows, planes, code)
    for (const RI &it : heavy) {
      const int w = (it.g0 >> 16) - (it.g0 & 0xFFFF) + 1;
      if (((it.code >> 24) & 7) != 1 || w > 32 || ((it.code >> 30) & 1)) {
        keep.push_back(it);
        continue;
      }
      bool done = false;
      for (size_t k = 0; k < open.size() && !done; k++) {
        RI &o = keep[open[k]];
        if (o.g1 == it.g1 && o.g2 == it.g2 && o.code == it.code && o.dep == it.dep) {
          o.g3 = it.g0;
          open.erase(open.begin() + (long)k);
          done = true;
        }
      }
      if (!done) {
        open.push_back(keep.size());
        keep.push_back(it);
      }
    }
    heavy.swap(keep);
  }
  // longest first; a narrow strip plane costs ~1.3 wide-tile planes (item clock, round 5)
  auto longest_first = [](std::vector<RI> &v) {
    auto cost = [](const RI &r) { return r.planes * (((r.code >> 30) & 1) ? 1.3 : 1.0); };
    std::stable_sort(v.begin(), v.end(), [&](const RI &x, const RI &y) { return cost(x) > cost(y); });
  };
  longest_first(heavy);
  longest_first(lean);
  // items that need no slab-face data first (multi-rank: they run before the face exchange)
  std::vector<RI> order;
  for (int dep = 0; dep < 2; dep++)
    for (auto *v : {&heavy, &lean})
      for (const RI &it : *v)
        if (it.dep == (dep == 1)) order.push_back(it);
  // one rank: the narrow strips (they read the two-step kernel's output) last, so that R1's
  // other items can run beside the two-step kernel (tb_pair, tb_r1a).  The second rim launch
  // takes the same list in the same order (its own longest-first order measured slower:
  // 512^3 +0.8 %, C2 256^3 +3.6 %)
  F->tb_rs0 = (int)order.size();
  if (F->nranks == 1) {
    auto strip = [](const RI &r) { return ((r.code >> 30) & 1) != 0; };
    std::stable_partition(order.begin(), order.end(), [&](const RI &r) { return !strip(r); });
    F->tb_rs0 = 0;
    for (const RI &it : order) F->tb_rs0 += strip(it) ? 0 : 1;
  }
  F->tb_rfree = 0;
  for (const RI &it : order) F->tb_rfree += it.dep ? 0 : 1;
  for (const RI &it : order) {
    F->tb_ritems.push_back(it.code);
    F->tb_rgeo.push_back(it.g0), F->tb_rgeo.push_back(it.g1), F->tb_rgeo.push_back(it.g2);
    F->tb_rgeo.push_back(it.g3);
  }
  // ---- two-step items: up to 124 x 12 own points (128 x 16 columns of lanes, two per lane),
  // z chunks of tz planes (automatic: the length whose item count fills whole rounds of one
  // workgroup per CU best, with the three halo planes of a chunk as overhead)
  // own columns of the two-step items: x0 .. x1 with lane 0's first column lx = x0 - 2 (x0 - 3
  // when x0 is odd: lane loads are 16-byte aligned), x1 <= lx + 125 and at most tb_ox columns
  // (0: TB_OXW = 124); widths of a box are whole pieces of that width plus the remainder
  const int oxw = F->tb_ox ? F->tb_ox : TB_OXW;
  auto lane0 = [](int x0) { return (x0 & 1) ? x0 - 3 : x0 - 2; };
  auto next_x1 = [&](int x0, int hi) {
    return std::min(std::min(lane0(x0) + TB_LX * TB_PX - 3, x0 + oxw - 1), hi);
  };
  auto box_items_x = [&](const Box &b) {
    int n = 0;
    for (int x = b.lo[0]; x <= b.hi[0]; x = next_x1(x, b.hi[0]) + 1) n++;
    return n;
  };
  int tz = F->tb_zchunk;
  if (tz <= 0) {
    const long long cus = std::max(1, k_cu_count());
    double best = -1;
    for (int cand : {32, 40, 48, 56, 64, 80, 96, 128}) {
      long long items = 0, chunks = 0, planes = 0;
      for (const Box &b : two) {
        const long long ntx = box_items_x(b);
        const long long nty = (b.hi[1] - b.lo[1] + TB_OY) / TB_OY;
        const long long nz = b.hi[2] - b.lo[2] + 1, nch = (nz + cand - 1) / cand;
        items += ntx * nty * nch;
        chunks += nch;
        planes += nz;
      }
      const double fill = double(items) / double(((items + cus - 1) / cus) * cus);
      const double per = double(planes) / double(std::max(chunks, 1LL));
      const double score = fill * per / (per + 3.0);
      if (score > best + 1e-12) best = score, tz = cand;
    }
  }
  F->tb_cells = F->tb_border = 0;
  // z pieces of a column of items: balanced chunks of <= tz planes.  (Long pieces over most
  // of a column with short ones queued last, to save most pieces' three halo planes, measured
  // no faster in-process: 2.2685 vs 2.2693 ms/step at 512^3, round 5 -- not kept.)
  auto zpieces = [&](int z0, int nz) {
    std::vector<std::pair<int, int>> v;  // [lo, hi] inclusive
    const int nch = (nz + tz - 1) / tz;
    for (int ch = 0; ch < nch; ch++)
      v.push_back({z0 + (int)((long long)nz * ch / nch), z0 + (int)((long long)nz * (ch + 1) / nch) - 1});
    return v;
  };
  std::vector<TB2Item> items;
  for (const Box &b : two) {
    const int ny = b.hi[1] - b.lo[1] + 1, nty = (ny + TB_OY - 1) / TB_OY;
    const int nz = b.hi[2] - b.lo[2] + 1;
    for (const auto &zp : zpieces(b.lo[2], nz))
      for (int ty = 0; ty < nty; ty++)
        for (int x0 = b.lo[0]; x0 <= b.hi[0];) {
          const int lx = lane0(x0);
          Box o;
          o.lo[0] = x0;
          o.hi[0] = next_x1(x0, b.hi[0]);
          x0 = o.hi[0] + 1;
          o.lo[1] = b.lo[1] + (int)((long long)ny * ty / nty);
          o.hi[1] = b.lo[1] + (int)((long long)ny * (ty + 1) / nty) - 1;
          o.lo[2] = zp.first;
          o.hi[2] = zp.second;
          // faces bordering the rim: the layer outside the face, widened by 1 along the other
          // axes (points of an edge / corner see diagonal neighbours), meets a rim box
          int faces = 0;
          double nb = 0;
          for (int f = 0; f < 6; f++) {
            const int ax = f / 2;
            Box s = o;
            for (int k = 0; k < 3; k++)
              if (k != ax) s.lo[k]--, s.hi[k]++;
            s.lo[ax] = s.hi[ax] = (f & 1) ? o.hi[ax] + 1 : o.lo[ax] - 1;
            bool m = false;
            for (const Box &r : rim) m = m || box_meets(s, r);
            if (m) {
              faces |= 1 << f;
              double fc = 1;
              for (int k = 0; k < 3; k++)
                if (k != ax) fc *= o.hi[k] - o.lo[k] + 1;
              nb += fc;
            }
          }
          TB2Item it;
          it.x = o.lo[0] | (o.hi[0] << 16);
          it.y = o.lo[1] | (o.hi[1] << 16);
          it.z = o.lo[2] | ((o.hi[2] + 1) << 16);
          it.faces = faces;
          it.bx = it.by = it.bz = -1, it.lx = lx;
          {
            // the first compact DFT box the own points meet goes to the kernel's compact
            // stores; other compact boxes the item meets take the middle-set stores below
            std::vector<Box> ibox = dbox;
            int cm = -1;
            for (size_t m = 0; m < F->tb_cmp.size(); m++) {
              const TBCmp &c = F->tb_cmp[m];
              bool meet = true;
              Box cb;
              for (int k = 0; k < 3; k++) {
                cb.lo[k] = c.lo[k], cb.hi[k] = c.lo[k] + c.n[k] - 1;
                meet = meet && std::max(o.lo[k], cb.lo[k]) <= std::min(o.hi[k], cb.hi[k]);
              }
              if (!meet) continue;
              if (cm < 0)
                cm = (int)m;
              else
                ibox.push_back(cb);
            }
            if (cm >= 0) it.faces |= (cm + 1) << 8;
            Box u;  // bounding box of the item's intersections with the DFT boxes
            bool any = false;
            for (const Box &db : ibox) {
              Box x;
              bool ok = true;
              for (int k = 0; k < 3; k++) {
                x.lo[k] = std::max(o.lo[k], db.lo[k]);
                x.hi[k] = std::min(o.hi[k], db.hi[k]);
                ok = ok && x.lo[k] <= x.hi[k];
              }
              if (!ok) continue;
              for (int k = 0; k < 3; k++) {
                u.lo[k] = any ? std::min(u.lo[k], x.lo[k]) : x.lo[k];
                u.hi[k] = any ? std::max(u.hi[k], x.hi[k]) : x.hi[k];
              }
              any = true;
            }
            if (any) {
              it.bx = u.lo[0] | (u.hi[0] << 16);
              it.by = u.lo[1] | (u.hi[1] << 16);
              it.bz = u.lo[2] | (u.hi[2] << 16);
              double nb2 = 1;
              for (int k = 0; k < 3; k++) nb2 *= u.hi[k] - u.lo[k] + 1;
              nb += nb2;
            }
          }
          items.push_back(it);
          F->tb_cells += double(o.hi[0] - o.lo[0] + 1) * (o.hi[1] - o.lo[1] + 1) *
                         (o.hi[2] - o.lo[2] + 1);
          F->tb_border += nb;  // an upper bound (edges counted twice)
        }
  }
  // the work queue takes the items in list order: longest first
  std::stable_sort(items.begin(), items.end(), [](const TB2Item &p, const TB2Item &q) {
    return (p.z >> 16) - (p.z & 0xFFFF) > (q.z >> 16) - (q.z & 0xFFFF);
  });
  F->tb_items = items;
  // ---- upload, palette-uniform flags, mixed-palette cell counts (traffic model)
  if (dev_upload(F, &F->d_tb_ritems, F->tb_rcap, F->tb_ritems) ||
      dev_upload(F, &F->d_tb_rgeo, F->tb_gcap, F->tb_rgeo) ||
      dev_upload(F, &F->d_tb_items, F->tb_icap, F->tb_items))
    return -1;
  const int nr = (int)F->tb_ritems.size(), ni = (int)F->tb_items.size();
  if (F->d_tb_rflag) (void)hipFree(F->d_tb_rflag);
  if (F->d_tb_uflag) (void)hipFree(F->d_tb_uflag);
  F->d_tb_rflag = F->d_tb_uflag = nullptr;
  F->rim_cells_nu = F->rim_cells;
  F->tb_cells_nu = F->tb_cells;
  if (F->d_uidx) {
    HIPCHK(hipMalloc(&F->d_tb_rflag, std::max(nr, 1) * sizeof(unsigned)));
    HIPCHK(hipMalloc(&F->d_tb_uflag, std::max(ni, 1) * sizeof(unsigned)));
    FusedArgs fa = fused_args(F);  // strides / palette of the current arrays
    if (k_tile_items_uniform(fa, F->d_tb_ritems, F->d_tb_rgeo, nr, F->d_tb_rflag, F->stream))
      return fail("rim palette flags failed");
    TB2Args t{};
    t.n = ni, t.items = F->d_tb_items, t.uidx = F->d_uidx;
    for (int k = 0; k < 3; k++) t.N[k] = g.N[k];
    t.st1 = g.st[1], t.st2 = g.st[2];
    if (k_tb2_uniform(t, F->d_tb_uflag, F->stream)) return fail("two-step palette flags failed");
    std::vector<unsigned> hr(nr), hi(ni);
    if (nr) HIPCHK(hipMemcpyAsync(hr.data(), F->d_tb_rflag, nr * 4, hipMemcpyDeviceToHost, F->stream));
    if (ni) HIPCHK(hipMemcpyAsync(hi.data(), F->d_tb_uflag, ni * 4, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    F->rim_cells_nu = F->tb_cells_nu = 0;
    for (int i = 0; i < nr; i++)
      if (hr[i] == ~0u) {
        const int *q = &F->tb_rgeo[4 * i];
        const int wx = (q[0] >> 16) - (q[0] & 0xFFFF) + 1 +
                       (q[3] >= 0 ? (q[3] >> 16) - (q[3] & 0xFFFF) + 1 : 0);
        F->rim_cells_nu += double(wx) * ((q[1] >> 16) - (q[1] & 0xFFFF) + 1) *
                           ((q[2] >> 16) - (q[2] & 0xFFFF));
      }
    for (int i = 0; i < ni; i++)
      if (hi[i] == ~0u) {
        const TB2Item &q = F->tb_items[i];
        F->tb_cells_nu += double((q.x >> 16) - (q.x & 0xFFFF) + 1) *
                          ((q.y >> 16) - (q.y & 0xFFFF) + 1) * ((q.z >> 16) - (q.z & 0xFFFF));
      }
  }
  HIPCHK(hipStreamSynchronize(F->stream));
  F->tb_have = ni > 0 || (F->nranks > 1 && nr > 0);
  if (F->tb_stats)
    fprintf(stderr, "tb: L2 [%d..%d]x[%d..%d]x[%d..%d], %zu holes, %zu two-step boxes, %zu rim "
            "boxes; %d two-step items (%d planes, %.0f cells, %.0f border), %d rim items "
            "(%.0f cells, %.0f lean, %d narrow strips)\n",
            L2.lo[0], L2.hi[0], L2.lo[1], L2.hi[1], L2.lo[2], L2.hi[2], holes.size(), two.size(),
            rim.size(), ni, tz, F->tb_cells, F->tb_border, nr, F->rim_cells, F->rim_lean,
            F->tb_nnarrow);
  return 0;
}

// The middle buffer set of the pairs (the arrays the fused step ping-pongs: B, D, stored E,
// separate H, f_u of B).  Allocated on the first pair; when device memory is short, whatever
// this call allocated is freed again and temporal blocking is switched off on this rank (the
// ranks agree in tb_usable), so a grid that fits with two sets keeps stepping one step at a
// time instead of failing.  MNL_TB_OOM=1 simulates the failure (tests).
static int tb_mid_alloc(mnl_fields *F) {
  DevFields &f = F->f;
  std::vector<double **> got;
  bool bad = false;
  auto one = [&](double **pp, double *cur) {
    if (!cur || *pp || bad) return;
    void *q = nullptr;
    if (F->tb_oom_test || hipMalloc(&q, F->nlocal * 8) != hipSuccess) {
      bad = true;
      (void)hipGetLastError();
      return;
    }
    *pp = (double *)q;
    got.push_back(pp);
  };
  for (int d = 0; d < 3; d++) {
    one(&F->pp3_B[d], f.B[d]);
    one(&F->pp3_D[d], f.D[d]);
    one(&F->pp3_E[d], f.E[d]);
    one(&F->pp3_H[d], f.H[d]);
    one(&F->pp3_UB[d], f.UB[d]);
  }
  if (!bad) {
    for (double **pp : got) F->dev_allocs.push_back(*pp);
    return 0;
  }
  for (double **pp : got) {
    (void)hipFree(*pp);
    *pp = nullptr;
  }
  (void)hipGetLastError();
  F->tb_enabled = false;
  F->tb_oom = true;
  if (g_verbosity > 0 && F->rank == 0)
    fprintf(stderr, "meep_nl_amd: not enough device memory for the temporal-blocking buffer set; "
                    "stepping one step at a time\n");
  return 1;
}

// Can the batch step in pairs?  Builds the plan when needed (-1: HIP error).
int tb_usable(mnl_fields *F, bool *ok) {
  *ok = false;
  // (no chi(2) NR box or upstream nonlinearity: the pairs have no E phase of their own.
  // Polarization chunks (the general items are exactly those chunks) step one step
  // at a time in the general kernel beside each rim launch, on one rank (round 6, DESIGN.md
  // section 27); L2 keeps a distance of 2 from them)
  const bool pol_ok = F->f.npol > 0 && F->fgeo.ngen > 0 && F->nranks == 1 && F->tb_pol_on;
  bool local = F->tb_enabled && F->fused &&
               ((F->fgeo.ngen == 0 && F->f.npol == 0) || pol_ok) && !F->nr && !F->upnl &&
               F->S.dim == 3 && F->slab_dir == 2 && !any_periodic(F);
  if (local && tb_plan(F)) return -1;
  if (local && F->tb_have && tb_mid_alloc(F)) local = false;
  if (F->tb_stats && !(local && F->tb_have))
    fprintf(stderr, "tb: no pairs (enabled %d fused %d ngen %d dim %d slab %d dfts %zu have %d)\n",
            (int)F->tb_enabled, (int)F->fused, F->fgeo.ngen, F->S.dim,
            F->slab_dir, F->dfts.size(), (int)F->tb_have);
  local = local && F->tb_have;
  if (F->nranks > 1) {  // every rank or none (their exchange sequences differ by mode)
    double v = local ? 1.0 : 0.0;
    if (F->comm->allreduce_sum(&v, 1, F->stream)) return fail("allreduce failed");
    local = v == double(F->nranks);
  }
  *ok = local;
  return 0;
}

// tile-kernel arguments of a rim launch: one step from set `o` to set `n`, the rim item list
static FusedArgs rim_args(mnl_fields *F, const FusedArgs &fa, const Set5 &o, const Set5 &n) {
  FusedArgs r = fa;
  args_sets(r, o, n);
  r.titems = F->d_tb_ritems;
  r.tgeo = F->d_tb_rgeo;
  r.tflag = F->d_uidx ? F->d_tb_rflag : nullptr;
  r.gbeg = 0, r.gend = (int)F->tb_ritems.size();
  r.clk.kind = 1;
  return r;
}

// general-kernel arguments of the polarization chunks in a pair: one step from `o` to `n`
// (P / P_prev and the f_u of D in place, as in one-step stepping)
static FusedArgs gen_args(const FusedArgs &fa, const Set5 &o, const Set5 &n) {
  FusedArgs r = fa;
  args_sets(r, o, n);
  r.wg_limit = 0;
  return r;
}

// two-step arguments: state n in `o`, border step n+1 into `m`, step n+2 into `n`
static TB2Args tb_args(mnl_fields *F, const Set5 &o, const Set5 &m, const Set5 &n) {
  const DevGrid &g = F->g;
  TB2Args t{};
  t.n = (int)F->tb_items.size();
  t.items = F->d_tb_items;
  t.uflag = F->d_uidx ? F->d_tb_uflag : nullptr;
  for (int d = 0; d < 3; d++) {
    t.Bo[d] = o.B[d], t.Do[d] = o.D[d];
    t.Bm[d] = m.B[d], t.Dm[d] = m.D[d];
    t.Bn[d] = n.B[d], t.Dn[d] = n.D[d];
    t.u[d] = F->f.inveps[d];
    t.N[d] = g.N[d];
  }
  t.uidx = F->d_uidx;
  t.utab = F->d_utab;
  t.st1 = g.st[1], t.st2 = g.st[2];
  t.nelem = (long long)F->nlocal;
  t.C = F->S.courant;
  t.ctr = F->d_fused_ctr;
  t.ctr_line = 3;
  t.clk = ItemClock{F->d_clk, F->d_clk_n, F->d_clk ? CLK_CAP : 0u, 2};
  t.ncmp = (int)F->tb_cmp.size();
  for (int i = 0; i < t.ncmp; i++) t.cmp[i] = F->tb_cmp[i];
  return t;
}

static int tb_src(mnl_fields *F, const SrcDev &s, double *const D[3]) {
  if (!s.n) return 0;
  DevFields fm = F->f;
  for (int d = 0; d < 3; d++) fm.Dn[d] = D[d];
  if (k_source(T_D, F->g, fm, s, 0, F->stream)) return fail("source launch failed");
  return 0;
}

// A pair's step tail on one rank: the step's D sources into D, then (when due) the NaN guard of
// the state E / D at time step `at` -- one launch (k_src_guard) for short source lists, else
// the two launches as before (tb_srcguard = 0: always two)
static int tb_tail(mnl_fields *F, const SrcDev &s, double *const D[3], double *const E[3], long long at) {
  nan_count(F, 1);
  F->nan_at = at;
  if (F->tb_srcguard && F->nan_due && F->nan_terms.n > 0 && s.n <= SRC_GUARD_MAXN &&
      s.nlayer <= SRC_GUARD_MAXL) {
    if (!F->d_nanflag && dev_alloc(F, &F->d_nanflag, 2)) return -1;
    DevFields fm = F->f;
    const double *Ec[3], *Dc[3], *U[3];
    for (int d = 0; d < 3; d++) fm.Dn[d] = D[d], Ec[d] = E[d], Dc[d] = D[d], U[d] = F->f.inveps[d];
    const int r = k_src_guard(fm, s, F->nan_terms, Ec, Dc, U, F->d_nanflag, (int)F->nan_at,
                              F->stream);
    if (r == 0) {
      F->nan_due = false;
      F->nan_launched++;
      return 0;
    }
    if (r != 2) return fail("source / guard launch failed");
  }
  if (tb_src(F, s, D)) return -1;
  return nan_launch(F, nullptr, E, D);
}

// the middle set starts as a copy of the state (entries no launch writes: walls, ghosts);
// its arrays exist (tb_mid_alloc ran in tb_usable)
static int tb_mid_init(mnl_fields *F) {
  if (F->tb_mid_fresh) return 0;
  DevFields &f = F->f;
  auto fresh = [&](double **pp, double *cur) -> int {
    if (!cur) return 0;
    if (!*pp) return fail("temporal blocking: middle buffer set missing");
    HIPCHK(hipMemcpyAsync(*pp, cur, F->nlocal * 8, hipMemcpyDeviceToDevice, F->stream));
    return 0;
  };
  for (int d = 0; d < 3; d++)
    if (fresh(&F->pp3_B[d], f.B[d]) || fresh(&F->pp3_D[d], f.D[d]) || fresh(&F->pp3_E[d], f.E[d]) ||
        fresh(&F->pp3_H[d], f.H[d]) || fresh(&F->pp3_UB[d], f.UB[d]))
      return -1;
  F->tb_mid_fresh = true;
  return 0;
}

// Steps n, n+1 (sources s0, s1) as three launches: L = the two-step
// kernel (cur -> nxt for the L2 points, their border values of step n+1 -> mid), R1 = the
// tile kernel over the rim items (cur -> mid), source(n) into mid, R2 = the rim items again
// (mid -> nxt), source(n+1) into nxt.  L runs first: the narrow x-face strips of R1 / R2 read
// the new B of their x-1 column (two-step points) from mid / nxt.  Every launch reads one set
// and writes disjoint points of others.
int tb_pair(mnl_fields *F, const SrcDev &s0, const SrcDev &s1, PhaseTimer &pt, long long t_mid) {
  if (tb_mid_init(F)) return -1;
  const FusedArgs &fa = fused_args(F);
  const Set5 cur = set_cur(F), mid = set_mid(F), nxt = set_nxt(F);
  TB2Args t = tb_args(F, cur, mid, nxt);
  const int nr = (int)F->tb_ritems.size();
  FusedArgs r1 = rim_args(F, fa, cur, mid), r2 = rim_args(F, fa, mid, nxt);
  {  // CUs left free by the two-step launch / the rim launches (A/B; the multi-rank default)
    const int rl = F->res_l >= 0 ? F->res_l : F->tb_res, rr = F->res_r >= 0 ? F->res_r : F->tb_res;
    if (rl > 0) t.wg_limit = std::max(1, k_cu_count() - rl);
    if (rr > 0) r1.wg_limit = r2.wg_limit = std::max(1, k_cu_count() - rr);
  }
  // R1's items other than the narrow strips read only cur and write rim points of mid: they
  // run on a side stream beside L, taking the CUs L's workgroups leave at the end of its queue
  // (the strips read L's border values of mid and follow L).  One timing span covers L and R1
  const int na = F->tb_r1a && !F->tb_pol ? std::min(F->tb_rs0, nr) : 0;
  if (na > 0 && ensure_aux_stream(F)) return -1;
  int k = pt.begin(TM_TB);
  int kr = 0;
  if (na > 0) {
    HIPCHK(hipEventRecord(F->ev_start, F->stream));
    HIPCHK(hipStreamWaitEvent(F->s_aux, F->ev_start, 0));
  }
  kr = k_tb2(t, F->stream, F->ctr_base);
  if (kr) return fused_fail("two-step kernel launch failed", kr);
  if (na > 0) {
    kr = k_tile_items(r1, r1.titems, r1.tgeo, r1.tflag, na, 5, F->s_aux, F->ctr_base);
    if (kr) return fused_fail("rim kernel launch failed", kr);
    HIPCHK(hipEventRecord(F->ev_early, F->s_aux));
    if (nr > na) {
      kr = k_tile_items(r1, r1.titems + na, r1.tgeo + 4 * na, r1.tflag ? r1.tflag + na : nullptr,
                        nr - na, 4, F->stream, F->ctr_base);
      if (kr) return fused_fail("rim kernel launch failed", kr);
    }
    HIPCHK(hipStreamWaitEvent(F->stream, F->ev_early, 0));
    pt.end(k);
  } else {
    pt.end(k);
    k = pt.begin(TM_RIM);
    kr = k_tile_items(r1, r1.titems, r1.tgeo, r1.tflag, nr, 4, F->stream, F->ctr_base);
    pt.end(k);
    if (kr) return fused_fail("rim kernel launch failed", kr);
  }
  if (F->tb_pol) {  // the polarization chunks' step n (before the sources of the step)
    k = pt.begin(TM_GEN);
    kr = k_fused(gen_args(fa, cur, mid), 1, F->stream, F->ctr_base);
    pt.end(k);
    if (kr) return fused_fail("fused general kernel launch failed", kr);
  }
  // the step's sources, then the guard of the middle step (its terms' points hold step n+1 in
  // mid: rim items, or the two-step items' store box)
  if (tb_tail(F, s0, mid.D, mid.E, t_mid)) return -1;
  if (dft_due(F, t_mid)) {  // fields::update_dfts after the pair's first step, from mid
    const DevFields fm = fields_at(F->f, mid);
    k = pt.begin(TM_DFT);
    const int r = dft_update(F, t_mid, &fm, 0);
    pt.end(k);
    if (r) return -1;
  }
  k = pt.begin(TM_RIM);
  kr = k_tile_items(r2, r2.titems, r2.tgeo, r2.tflag, nr, 4, F->stream, F->ctr_base);
  pt.end(k);
  if (kr) return fused_fail("rim kernel launch failed", kr);
  if (F->tb_pol) {
    k = pt.begin(TM_GEN);
    kr = k_fused(gen_args(fa, mid, nxt), 1, F->stream, F->ctr_base);
    pt.end(k);
    if (kr) return fused_fail("fused general kernel launch failed", kr);
  }
  if (tb_tail(F, s1, nxt.D, nxt.E, t_mid + 1)) return -1;
  swap_cur_nxt(F->f);
  return 0;
}

// Multi-rank pair (one rank of a z-slab decomposition; fused, no D source on the top
// plane).  L2 lies >= 2 planes from the slab faces, so only the rim meets them:
//   main: L (cur -> nxt, border -> mid) on all CUs but RES (the previous pair's slab-face
//         chain still runs on s_comm), then, once the E ghost of step n is in (ev_x0), R1
//         (rim, cur -> mid);
//   s_comm: B/H plane exchange of mid, the top plane's step n (shell kernels, old = cur,
//         new = mid), source(n), E plane exchange of mid (ev_x0);
//   main: R2 over the rim items that read no slab-face data and hold no source point
//         (beside that chain), then the others once it is done;
//   s_comm: the same chain for nxt -- beside the next pair's L.
// Every kernel reads and writes disjoint points of its sets.
static int tb_face_chain(mnl_fields *F, const Set5 &o, const Set5 &n, const SrcDev &src,
                         hipEvent_t after, PhaseTimer &pt) {
  DevFields &f = F->f;
  HIPCHK(hipStreamWaitEvent(F->s_comm, after, 0));
  const int kc = pt.begin(TM_CHAIN, F->s_comm);
  // exchanges and shell kernels read F->f's pointers when enqueued: point them at the sets
  const DevFields keep = f;
  f = fields_at(keep, o, n);
  int r = exchange(F, 1, F->s_comm) ? fail("H halo exchange failed") : 0;
  // the sources of the step (every D point: after the top plane's curl D, as the one-step
  // path applies them after all of D); with one on the top plane E follows the source there
  if (!r) r = shell_step(F, F->s_comm, !F->dsrc_in_shell, src);
  if (!r) {  // the E plane of the new set goes up
    for (int d = 0; d < 3; d++) f.E[d] = n.E[d];
    if (exchange(F, 0, F->s_comm)) r = fail("E halo exchange failed");
  }
  f = keep;
  if (r) return r;
  pt.end(kc, F->s_comm);
  HIPCHK(hipEventRecord(F->ev_x0, F->s_comm));
  return 0;
}

int tb_pair_multi(mnl_fields *F, const SrcDev &s0, const SrcDev &s1, PhaseTimer &pt,
                  long long t_mid) {
  if (tb_mid_init(F)) return -1;
  const FusedArgs &fa = fused_args(F);
  const Set5 cur = set_cur(F), mid = set_mid(F), nxt = set_nxt(F);
  TB2Args t = tb_args(F, cur, mid, nxt);
  const int cus = k_cu_count();
  const int res = F->tb_res >= 0 ? F->tb_res : TB_RES_CUS;
  t.wg_limit = res > 0 ? cus - res : 0;
  const int nr = (int)F->tb_ritems.size(), nf = F->tb_rfree;
  int k = pt.begin(TM_TB);
  int kr = k_tb2(t, F->stream, F->ctr_base);
  pt.end(k);
  if (kr) return fused_fail("two-step kernel launch failed", kr);
  // R1 once the E ghost (and top plane) of step n are in
  k = pt.begin(TM_WAIT);
  HIPCHK(hipStreamWaitEvent(F->stream, F->ev_x0, 0));
  pt.end(k);
  FusedArgs r1 = rim_args(F, fa, cur, mid);
  k = pt.begin(TM_RIM);
  kr = k_tile_items(r1, r1.titems, r1.tgeo, r1.tflag, nr, 4, F->stream, F->ctr_base);
  pt.end(k);
  if (kr) return fused_fail("rim kernel launch failed", kr);
  HIPCHK(hipEventRecord(F->ev_early, F->stream));
  if (tb_face_chain(F, cur, mid, s0, F->ev_early, pt)) return -1;
  nan_count(F, 1);  // the middle step's guard, after its top plane and sources (s_comm)
  F->nan_at = t_mid;
  if (nan_launch(F, F->s_comm, mid.E, mid.D)) return -1;
  // R2: the items without slab-face reads beside the chain, then the others
  FusedArgs r2 = rim_args(F, fa, mid, nxt);
  r2.wg_limit = res > 0 ? cus - res : 0;
  k = pt.begin(TM_RIM);
  kr = k_tile_items(r2, r2.titems, r2.tgeo, r2.tflag, nf, 4, F->stream, F->ctr_base);
  pt.end(k);
  if (!kr) {
    const int kw = pt.begin(TM_WAIT);
    HIPCHK(hipStreamWaitEvent(F->stream, F->ev_x0, 0));
    pt.end(kw);
    if (dft_due(F, t_mid)) {
      // fields::update_dfts after the pair's first step, from mid (round 6): the chain has
      // put mid's top plane, sources and E ghost in; the H component normal to the slabs gets
      // its low ghost now (exchange kind 3, as post_step does after a one-step step).  The
      // exchange reads F->f's pointers when enqueued: point them at mid meanwhile
      const DevFields keep = F->f, fm = fields_at(keep, mid);
      F->f = fm;
      k = pt.begin(TM_DFT);
      int r = exchange(F, 3) ? fail("DFT halo exchange failed") : 0;
      F->f = keep;
      if (!r) r = dft_update(F, t_mid, &fm, 0);
      pt.end(k);
      if (r) return -1;
    }
    k = pt.begin(TM_RIM);
    r2.wg_limit = 0;
    kr = k_tile_items(r2, r2.titems + nf, r2.tgeo + 4 * nf, r2.tflag ? r2.tflag + nf : nullptr,
                      nr - nf, 4, F->stream, F->ctr_base);
  }
  pt.end(k);
  if (kr) return fused_fail("rim kernel launch failed", kr);
  HIPCHK(hipEventRecord(F->ev_early, F->stream));
  if (tb_face_chain(F, mid, nxt, s1, F->ev_early, pt)) return -1;
  swap_cur_nxt(F->f);
  F->tb_chain_pending = true;  // a one-step step next waits for it (tb_chain_join)
  nan_count(F, 1);
  F->nan_at = t_mid + 1;
  return nan_launch(F, F->s_comm);  // after the chain: the top plane of the new state
}

// Before a one-step step after a multi-rank pair: the pair's last slab-face chain (top plane,
// sources, E ghost) ran on s_comm; the one-step kernels on the main stream read its results.
int tb_chain_join(mnl_fields *F) {
  if (!F->tb_chain_pending) return 0;
  F->tb_chain_pending = false;
  HIPCHK(hipStreamWaitEvent(F->stream, F->ev_x0, 0));
  return 0;
}

}  // namespace mnlh
