// mnl_step.cpp -- the step path (fields::step, src/step.cpp:35-140): halo exchange, the lazy
// first-step copies, the Newton-Raphson E phases, the multi-rank fused step, phase timing,
// step_batch and its parts, the NaN guard, fields_step.
#include "mnl_host.hpp"

namespace mnlh {

// ------------------------------------------------------------- halo exchange
// step_boundaries replacement for the slab decomposition (src/step.cpp:226-288):
// kind 0 (before curl B): E comps unshifted along the slab axis need the low
//   ghost plane (local 0) <- rank-1's top owned plane (local nloc).
// kind 1 (before curl D): B (and separate H) comps shifted along the slab axis
//   need the high ghost plane (local nloc) <- rank+1's first plane (local 0).
// kind 2 (before NR E update): D comps (and Lorentz P), both directions.
// kind 3 (before a DFT update): H comps unshifted along the slab axis need the
//   low ghost plane, which the centred-grid average reads (src/dft.cpp:281-287);
//   so do the D comps unshifted along it once a monitor samples D itself.
int exchange(mnl_fields *F, int kind, hipStream_t st) {
  if (!st) st = F->stream;
  const DevGrid &g = F->g;
  const int sd = F->slab_dir, ax = g.ax[sd];
  const size_t plane = (size_t)g.st[ax];
  const int nloc = g.N[ax] - 1;
  const int up = F->rank + 1 < F->nranks ? F->rank + 1 : -1;
  const int dn = F->rank > 0 ? F->rank - 1 : -1;
  struct Item {
    double *p;
    bool low_ghost;  // true: send top plane up, receive plane 0 from below
  };
  std::vector<Item> items;
  auto gather = [&](const mnl_fields *F) {  // (shadows F: one part's arrays)
  for (int c = 0; c < 3; c++) {
    if (kind == 0) {
      if (c != sd && F->f.E[c] && F->allocated[c]) items.push_back({F->f.E[c], true});
    } else if (kind == 1) {
      if (c != sd && F->f.Bn[c] && F->allocated[3 * T_H + c]) {
        items.push_back({F->f.Bn[c], false});
        if (F->f.H[c]) items.push_back({F->f.Hn[c], false});
      }
    } else if (kind == 4) {  // W of E (E, and f_w where allocated): the one ghost plane
      if (F->f.E[c] && F->allocated[c]) {
        items.push_back({F->f.E[c], c != sd});
        if (F->f.WE[c]) items.push_back({F->f.WE[c], c != sd});
      }
    } else if (kind == 3) {  // DFT: H comps unshifted along the slab axis, low ghost
      if (c == sd && F->allocated[3 * T_H + c]) {
        items.push_back({F->f.B[c], true});
        if (F->f.H[c]) items.push_back({F->f.H[c], true});
      }
      if (F->dft_samples_d && c != sd && F->f.D[c] && F->allocated[3 * T_D + c])
        items.push_back({F->f.D[c], true});
    } else {
      if (F->f.Dn[c] && F->allocated[3 * T_D + c]) items.push_back({F->f.Dn[c], c != sd});
      for (int k = 0; k < F->f.npol; k++)
        if (F->f.pol[k].P[c]) items.push_back({F->f.pol[k].P[c], c != sd});
    }
  }
  };
  // complex fields: both parts' arrays in one group, whichever part
  // the call names (they share the communicator and the slab geometry)
  if (is_complex(F)) {
    mnl_fields *P = F->part0 ? F->part0 : F;
    gather(P);
    gather(P->twin.get());
  } else {
    gather(F);
  }
  if (items.empty()) return 0;
  Comm &cm = *F->comm;
  if (cm.group_start()) return -1;
  for (auto &it : items) {
    if (it.low_ghost) {
      if (up >= 0 && cm.send(it.p + (size_t)nloc * plane, plane, up, st)) return -1;
      if (dn >= 0 && cm.recv(it.p, plane, dn, st)) return -1;
    } else {
      if (dn >= 0 && cm.send(it.p, plane, dn, st)) return -1;
      if (up >= 0 && cm.recv(it.p + (size_t)nloc * plane, plane, up, st)) return -1;
    }
  }
  return cm.group_end(st);
}

// step_boundaries over the periodic connections (fields::use_bloch with k = 0; src/boundaries.cpp:
// 347-623, phase 1): the same kinds and arrays as exchange, with the rank as its own neighbour
// along every periodic direction -- plane 0 of a component unshifted along it is a copy of plane
// n, plane n of a shifted one a copy of plane 0.  One launch per call (wrap_kernel); a point on
// the not-owned planes of several periodic directions maps along all of them at once.  Every
// component of a kind is listed, whichever way it is shifted, so that whole arrays read back
// with valid ghosts.  After exchange where both run: the slab ghost planes wrap too.
// kind WRAP_ALL: every field and polarization array (readers, checkpoints).
// The longest list: E, f_w, B, H, D with the ping-pong sets of B, H and D (24 arrays) and three
// per susceptibility, of which a structure takes MAX_POL -- one launch holds them all.
constexpr int WRAP_FIELD_ARRAYS = 3 * 8;  // per direction: E, f_w, Bn, Hn, B, H, D, Dn (the add() calls below)
static_assert(WRAP_FIELD_ARRAYS + 3 * MAX_POL <= WRAP_MAXA, "wrap(WRAP_ALL) must fit one launch");
static int wrap_list(mnl_fields *F, int kind, WrapArgs &w);
static int wrap_cplx(mnl_fields *F, int kind, hipStream_t st);

int wrap(mnl_fields *F, int kind, hipStream_t st) {
  if (!any_periodic(F)) return 0;
  if (is_complex(F)) return wrap_cplx(F->part0 ? F->part0 : F, kind, st);
  if (!st) st = F->stream;
  WrapArgs w{};
  if (wrap_list(F, kind, w)) return -1;
  if (w.n == 0) return 0;
  wrap_plan(w);
  if (k_wrap(w, st)) return fail("periodic wrap launch failed");
  return 0;
}

// Complex fields: one launch for both parts, every ghost point times
// its Bloch phase (fields::process_incoming_chunk_data, src/step.cpp:173-197).  Both parts
// list the same arrays in the same order: they have the same structure and step in the same
// mode.
static int wrap_cplx(mnl_fields *F, int kind, hipStream_t st) {
  mnl_fields *T = F->twin.get();
  if (!st) st = F->stream;
  WrapPhaseArgs A{};
  WrapArgs w1{};
  if (wrap_list(F, kind, A.w) || wrap_list(T, kind, w1)) return -1;
  if (A.w.n != w1.n) return fail("periodic wrap: the parts of the complex fields differ");
  if (A.w.n == 0) return 0;
  for (int i = 0; i < w1.n; i++) {
    if (A.w.a[i].sh != w1.a[i].sh) return fail("periodic wrap: the parts of the complex fields differ");
    A.q[i] = w1.a[i].p;
  }
  int dir_of_axis[3] = {-1, -1, -1};
  for (int d = 0; d < 3; d++)
    if (F->g.ax[d] >= 0) dir_of_axis[F->g.ax[d]] = d;
  bloch_phase_table(F->eikna, dir_of_axis, A.ph);
  wrap_plan(A.w);
  if (k_wrap_phase(A, st)) return fail("periodic wrap launch failed");
  return 0;
}

// the arrays of one wrap kind (no launch)
static int wrap_list(mnl_fields *F, int kind, WrapArgs &w) {
  const DevGrid &g = F->g;
  const DevFields &f = F->f;
  for (int k = 0; k < 3; k++) w.N[k] = g.N[k], w.st[k] = g.st[k];
  for (int d = 0; d < 3; d++)
    if (g.ax[d] >= 0 && F->periodic[d]) w.per[g.ax[d]] = 1;
  bool full = false;
  auto add = [&](double *p, int type, int c) {
    if (!p) return;
    for (int i = 0; i < w.n; i++)
      if (w.a[i].p == p) return;  // H aliasing B, unfused Bn == B
    if (w.n == WRAP_MAXA) {  // out of reach (the static_assert above); it guards w.a all the same
      full = true;
      return;
    }
    int sh = 0;
    for (int d = 0; d < 3; d++)
      if (g.ax[d] >= 0 && F->S.shift(3 * type + c, d)) sh |= 1 << g.ax[d];
    w.a[w.n++] = WrapArr{p, sh};
  };
  const bool all = kind == WRAP_ALL;
  for (int c = 0; c < 3; c++) {
    if ((kind == 0 || kind == 4 || all) && F->allocated[3 * T_E + c]) {
      add(f.E[c], T_E, c);
      if (kind != 0) add(f.WE[c], T_E, c);
    }
    if ((kind == 1 || all) && F->allocated[3 * T_H + c]) add(f.Bn[c], T_H, c), add(f.Hn[c], T_H, c);
    if ((kind == 3 || all) && F->allocated[3 * T_H + c]) add(f.B[c], T_H, c), add(f.H[c], T_H, c);
    if (((kind == 3 && F->dft_samples_d) || all) && F->allocated[3 * T_D + c]) add(f.D[c], T_D, c);
    if ((kind == 2 || all) && F->allocated[3 * T_D + c]) {
      add(f.Dn[c], T_D, c);
      for (int k = 0; k < f.npol; k++) add(f.pol[k].P[c], T_E, c);
    }
  }
  if (full) return fail("periodic wrap: too many arrays");
  return 0;
}

// Before whole arrays are read: every ghost plane valid.  In the fused mode the owner of a
// ghost E point may be implicit (chi1inv * D, not stored), so the mode is left first, which
// materialises E; the next batch enters it again.
int wrap_for_readers(mnl_fields *F) {
  if (!any_periodic(F)) return 0;
  if (is_complex(F)) {  // both parts leave the mode: the wrap lists the same arrays of each
    mnl_fields *P = F->part0 ? F->part0 : F;
    for (mnl_fields *p : {P, P->twin.get()})
      if (p->fused && set_fused(p, false)) return -1;
    return wrap(P, WRAP_ALL);
  }
  if (F->fused && set_fused(F, false)) return -1;
  return wrap(F, WRAP_ALL);
}

int fused_fail(const char *what, int kr) {
  return fail(std::string(what) + " (" + std::to_string(kr) + ", " +
              hipGetErrorString(hipGetLastError()) + ")");
}

// one rank: CUs of the polarization chunks' general kernel beside the tile
// kernel (0: after it on the same stream; the tuner's choice, or MNL_TILE_GEN_CUS)
static int tile_gen_split(const mnl_fields *F) {
  const int v = F->tile_gen_cus;
  const int cus = k_cu_count();
  return (v > 0 && v < cus) ? v : 0;
}

// streams / events of the overlapped multi-rank step; the E ghost plane is made
// valid once (kind 0) since each step ends with the exchange for the next one
static int multi_begin(mnl_fields *F) {
  // (not ensure_aux_stream: these events order work against the exchanges, whose data other
  // devices read, so they keep the system-scope release that the one-rank events drop)
  if (!F->s_comm) {
    HIPCHK(hipStreamCreateWithFlags(&F->s_comm, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&F->s_aux, hipStreamNonBlocking));
    for (hipEvent_t *e : {&F->ev_start, &F->ev_early, &F->ev_x1, &F->ev_shell, &F->ev_x0})
      HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  HIPCHK(hipEventRecord(F->ev_start, F->stream));
  HIPCHK(hipStreamWaitEvent(F->s_comm, F->ev_start, 0));
  if (exchange(F, 0, F->s_comm)) return fail("E halo exchange failed");
  HIPCHK(hipEventRecord(F->ev_x0, F->s_comm));
  return 0;
}

// One rank: the side stream of launches that run beside the main stream's, and the two events
// that order them, created at first use.  The events release at device scope: every reader
// is on this device.
int ensure_aux_stream(mnl_fields *F) {
  if (F->s_aux) return 0;
  HIPCHK(hipStreamCreateWithFlags(&F->s_aux, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&F->ev_start, hipEventDisableTiming | hipEventReleaseToDevice));
  HIPCHK(hipEventCreateWithFlags(&F->ev_early, hipEventDisableTiming | hipEventReleaseToDevice));
  return 0;
}

// The top plane's step of a rank with neighbours (the fused shell) on stream st: curl B with
// the H update fused in, curl D -- after `h_in` when given -- with the E update fused in when
// fuseE, the step's D sources, then the E update that was not fused.  The kernels read F->f's
// pointers when enqueued.
int shell_step(mnl_fields *F, hipStream_t st, bool fuseE, const SrcDev &sD, hipEvent_t h_in) {
  const DevGrid &g = F->g;
  const DevFields &f = F->f;
  const BoxList *sl = &F->fused_shell;
  if (k_curl(T_B, F->interior, sl, g, f, F->planB, F->S.courant, st, true))
    return fail("curl B launch failed");
  if (h_in) HIPCHK(hipStreamWaitEvent(st, h_in, 0));
  if (k_curl(T_D, F->interior, sl, g, f, F->planD, F->S.courant, st, fuseE))
    return fail("curl D launch failed");
  if (sD.n && k_source(T_D, g, f, sD, 0, st)) return fail("source launch failed");
  if (!fuseE) {
    ISrcDev is{};
    if (k_update_e(F->interior, sl, g, f, is, 0, true, st)) return fail("update E launch failed");
  }
  return 0;
}

// One fused step of a rank with neighbours.  Chunk 0 (planes 0..1: the B that
// the lower neighbour needs) runs first on s_aux; its B/H plane goes down while
// the interior runs on the main stream; the top plane (shell) follows once the
// upper neighbour's plane has arrived, and its E goes up for the next step.
static int step_fused_multi(mnl_fields *F, const SrcDev &sD, PhaseTimer &pt) {
  DevFields &f = F->f;
  FusedArgs &fa = fused_args(F);
  HIPCHK(hipEventRecord(F->ev_start, F->stream));
  HIPCHK(hipStreamWaitEvent(F->s_aux, F->ev_start, 0));
  HIPCHK(hipStreamWaitEvent(F->s_aux, F->ev_x0, 0));
  int kr = k_fused(fa, 5, F->s_aux, F->ctr_base);
  if (!kr) kr = k_fused(fa, 2, F->s_aux, F->ctr_base);
  if (kr) return fused_fail("fused early kernel launch failed", kr);
  HIPCHK(hipEventRecord(F->ev_early, F->s_aux));
  HIPCHK(hipStreamWaitEvent(F->s_comm, F->ev_early, 0));
  if (exchange(F, 1, F->s_comm)) return fail("H halo exchange failed");
  HIPCHK(hipEventRecord(F->ev_x1, F->s_comm));
  int k = pt.begin(TM_BINT);
  // the persistent main launch leaves TB_RES_CUS CUs to the chunk-0 launch on s_aux and
  // the slab-face work after it, so they cannot queue behind it for the whole step
  fa.wg_limit = k_cu_count() - TB_RES_CUS;
  kr = k_fused(fa, 6, F->stream, F->ctr_base);
  fa.wg_limit = 0;
  if (kr) return fused_fail("fused kernel launch failed", kr);
  pt.end(k);
  if (fa.ngen > fa.ngen_e) {
    k = pt.begin(TM_GEN);
    kr = k_fused(fa, 3, F->stream, F->ctr_base);
    if (kr) return fused_fail("fused general kernel launch failed", kr);
    pt.end(k);
  }
  // the top plane; its curl D reads the lower neighbour's H plane (ev_x1)
  if (shell_step(F, F->stream, !F->dsrc_in_shell && f.npol == 0, sD, F->ev_x1)) return -1;
  HIPCHK(hipEventRecord(F->ev_shell, F->stream));
  swap_cur_nxt(f);
  HIPCHK(hipStreamWaitEvent(F->s_comm, F->ev_shell, 0));
  if (exchange(F, 0, F->s_comm)) return fail("E halo exchange failed");
  HIPCHK(hipEventRecord(F->ev_x0, F->s_comm));
  return 0;
}

// first update_eh(H_stuff): H = copy of B and f_w = copy of H where they are
// separate (src/update_eh.cpp:204-216)
int h_lazy_copy(mnl_fields *F) {
  DevFields &f = F->f;
  for (int d = 0; d < 3; d++) {
    if (!f.H[d] || !f.Bn[d]) continue;
    if (k_copy(f.H[d], f.Bn[d], (long long)F->nlocal, F->stream)) return fail("copy launch failed");
    if (f.WH[d] && k_copy(f.WH[d], f.Bn[d], (long long)F->nlocal, F->stream))
      return fail("copy launch failed");
  }
  F->h_first_done = true;
  return 0;
}
// first step_db(B_stuff / D_stuff): f_u = copy of f where a PML lies along
// dsigu (src/step_db.cpp:71-75)
int u_lazy_copy(mnl_fields *F, int which) {
  DevFields &f = F->f;
  for (int d = 0; d < 3; d++) {
    double *u = which == 0 ? f.UB[d] : f.UD[d];
    const double *src = which == 0 ? f.B[d] : f.D[d];
    if (u && src && k_copy(u, src, (long long)F->nlocal, F->stream)) return fail("copy launch failed");
  }
  F->u_first_done[which] = true;
  return 0;
}
// first update_eh(E_stuff): f_w = copy of E (src/update_eh.cpp:212-216)
int e_lazy_copy(mnl_fields *F) {
  DevFields &f = F->f;
  for (int d = 0; d < 3; d++)
    if (f.WE[d] && f.E[d] &&
        k_copy(f.WE[d], f.E[d], (long long)F->nlocal, F->stream))
      return fail("copy launch failed");
  F->e_first_done = true;
  return 0;
}

// update_eh(H_stuff) [+ update_pols(H_stuff) when pols]: the PML W update over the shell boxes, or,
// with H-side materials, the H kernel over the whole rank-local box
int update_h_any(mnl_fields *F, const BoxList &sl, bool pols) {
  if (F->hall) {
    Box all;
    for (int k = 0; k < 3; k++) all.lo[k] = 0, all.hi[k] = F->g.N[k] - 1;
    if (k_update_hmat(all, F->g, F->f, pols ? 1 : 0, F->stream)) return fail("update H launch failed");
    return 0;
  }
  bool anyH = false;
  for (int d = 0; d < 3; d++) anyH = anyH || F->f.H[d];
  if (anyH && k_update_h(sl, F->g, F->f, F->stream)) return fail("update H launch failed");
  return 0;
}

// Interior E update with chi(2) Newton-Raphson: the NR kernel over the bounding
// box of chi2 != 0 inside the interior, the plain kernel over the rest (outside
// that box chi2 = 0, so every point takes E = chi1inv * (D - P) either way).
int nr_split(mnl_fields *F) {
  const DevGrid &g = F->g;
  if (!F->nr_split_done) {
    int *d = nullptr;
    HIPCHK(hipMalloc(&d, 6 * sizeof(int)));
    std::unique_ptr<void, void (*)(void *)> guard(d, [](void *p) { (void)hipFree(p); });
    int box[6] = {INT32_MAX, INT32_MAX, INT32_MAX, -1, -1, -1};
    HIPCHK(hipMemcpyAsync(d, box, sizeof box, hipMemcpyHostToDevice, F->stream));
    const double *c2[3] = {F->f.chi2[0], F->f.chi2[1], F->f.chi2[2]};
    if (k_nonzero_box(c2, g, d, F->stream)) return fail("chi2 box failed");
    HIPCHK(hipMemcpyAsync(box, d, sizeof box, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    const Box &I = F->interior;
    Box n;
    bool empty = false;
    F->nr_shell_free = true;  // chi2 != 0 nowhere outside the interior box
    for (int k = 0; k < 3; k++) F->nr_chi2.lo[k] = box[k], F->nr_chi2.hi[k] = box[3 + k];
    for (int k = 0; k < 3; k++) {  // 3-D: device axis k == direction k
      n.lo[k] = std::max(box[k], I.lo[k]);
      n.hi[k] = std::min(box[3 + k], I.hi[k]);
      empty = empty || n.hi[k] < n.lo[k];
      if (box[3 + k] >= box[k] && (box[k] < I.lo[k] || box[3 + k] > I.hi[k]))
        F->nr_shell_free = false;
    }
    F->nr_rest.clear();
    if (empty) {
      F->nr_in.lo[0] = 1, F->nr_in.hi[0] = 0;
      F->nr_rest.push_back(I);
    } else {
      F->nr_in = n;
      Box r = I;  // peel z, then y, then x slabs off the interior
      for (int k = 2; k >= 0; k--) {
        if (r.lo[k] < n.lo[k]) {
          Box b = r;
          b.hi[k] = n.lo[k] - 1;
          F->nr_rest.push_back(b);
        }
        if (r.hi[k] > n.hi[k]) {
          Box b = r;
          b.lo[k] = n.hi[k] + 1;
          F->nr_rest.push_back(b);
        }
        r.lo[k] = n.lo[k], r.hi[k] = n.hi[k];
      }
    }
    F->nr_split_done = true;
  }
  return 0;
}

static int nr_interior_e(mnl_fields *F, const ISrcDev &is) {
  const DevGrid &g = F->g;
  if (nr_split(F)) return -1;
  if (F->nr_in.hi[0] >= F->nr_in.lo[0] &&
      k_update_e(F->nr_in, nullptr, g, F->f, is, 0, false, F->stream))
    return fail("update E launch failed");
  DevFields plain = F->f;
  plain.nr_enabled = 0;
  for (const Box &b : F->nr_rest)
    if (k_update_e(b, nullptr, g, plain, is, 0, false, F->stream)) return fail("update E launch failed");
  return 0;
}

// Before an E update that may run the NR branch: enable deferral (MNL_NR_DEFER=0 solves
// every problem in place, sequentially) and clear the list; after it, the parallel pass.
int nr_defer_begin(mnl_fields *F, hipStream_t st) {
  if (!F->d_nr_hard) return 0;
  F->f.nr_hard = F->nr_defer ? F->d_nr_hard : nullptr;
  if (F->f.nr_hard)
    HIPCHK(hipMemsetAsync(F->d_nr_hard_cnt, 0, sizeof(unsigned), st ? st : F->stream));
  return 0;
}
int nr_defer_end(mnl_fields *F, hipStream_t st) {
  if (!F->f.nr_hard) return 0;
  if (k_nr_hard(F->f, st ? st : F->stream)) return fail("NR parallel-attempt kernel launch failed");
  return 0;
}

// Fused mode with chi(2) (nr_fused_ok): the fused kernels stored the new D (Dn) everywhere
// and E / P everywhere but the chi2 box grown by one point; here that box: E by the NR
// kernel (Newton-Raphson where chi2 != 0, chi1inv * (D - P) at the other points, the
// values the fused kernels would have stored), then update_P over it, as the unfused
// NR path orders them (src/step_generic.cpp:730-816, src/susceptibility.cpp:251-258)
static int nr_fused_e(mnl_fields *F, const ISrcDev &is, hipStream_t st = nullptr) {
  const Box &x = F->nr_xbox;
  if (x.hi[0] < x.lo[0]) return 0;
  if (!st) st = F->stream;
  if (nr_defer_begin(F, st)) return -1;
  if (k_update_e(x, nullptr, F->g, F->f, is, 0, false, st)) return fail("update E launch failed");
  if (nr_defer_end(F, st)) return -1;
  if (k_update_pols(x, nullptr, F->g, F->f, st)) return fail("pols launch failed");
  return 0;
}

// The NR box's E phase may run right after the polarization chunks' general kernel, on its
// stream beside the tile kernel (it reads the new D of the box and the old E, writes only the
// box's new E / P -- points the tile kernel neither reads nor writes), when no D source point
// lies in the box (sources are added to the new D after the fused kernels)
static bool nr_early_ok(const mnl_fields *F) {
  const Box &x = F->nr_xbox;
  if (!F->nr_early || x.hi[0] < x.lo[0]) return false;
  for (long long idx : F->srcD_idx) {
    const long long z = idx / F->g.st[2], r = idx % F->g.st[2];
    const long long y = r / F->g.st[1], xx = r % F->g.st[1];
    if (xx >= x.lo[0] && xx <= x.hi[0] && y >= x.lo[1] && y <= x.hi[1] && z >= x.lo[2] &&
        z <= x.hi[2])
      return false;
  }
  return true;
}

// diagnostics: append this batch's item records (rank-tagged binary, CLK_REC u64 each,
// preceded per batch by {magic, rank, count}) to clk_path and reset the counter
static int clk_dump(mnl_fields *F) {
  unsigned n = 0;
  HIPCHK(hipMemcpy(&n, F->d_clk_n, sizeof n, hipMemcpyDeviceToHost));
  n = std::min(n, CLK_CAP);
  std::vector<unsigned long long> h((size_t)n * CLK_REC);
  if (n) HIPCHK(hipMemcpy(h.data(), F->d_clk, h.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(F->d_clk_n, 0, sizeof(unsigned)));
  FILE *fp = fopen(F->clk_path.c_str(), "ab");
  if (!fp) return fail("MNL_ITEM_CLOCK: cannot open " + F->clk_path);
  const unsigned long long hd[CLK_REC] = {0x4b4c434d4e4dull, (unsigned long long)F->rank, n, 0, 0, 0, 0, 0};
  fwrite(hd, 8, CLK_REC, fp);
  if (n) fwrite(h.data(), 8, h.size(), fp);
  fclose(fp);
  return 0;
}

// ---- PhaseTimer
bool PhaseTimer::reserve_events() {
  while (F->ev_pool.size() < 2 * (spans.size() + 1)) {
    hipEvent_t e;
    if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return false;
    F->ev_pool.push_back(e);
  }
  return true;
}
int PhaseTimer::begin(int cat, hipStream_t st) {
  if (!F->profiling || !reserve_events()) return -1;
  const size_t i = spans.size();
  spans.push_back({F->ev_pool[2 * i], F->ev_pool[2 * i + 1], cat});
  hipEventRecord(spans[i].a, st ? st : F->stream);
  return (int)i;
}
void PhaseTimer::end(int k, hipStream_t st) {
  if (k >= 0) hipEventRecord(spans[k].b, st ? st : F->stream);
}
int PhaseTimer::next(int k, int cat) {
  if (!F->profiling || k < 0) return begin(cat);
  if (!reserve_events()) return -1;
  const size_t i = spans.size();
  spans.push_back({spans[k].b, F->ev_pool[2 * i + 1], cat});
  return (int)i;
}
int PhaseTimer::flush() {
  if (!F->profiling || spans.empty()) return 0;
  HIPCHK(hipStreamSynchronize(F->stream));
  if (F->s_comm) HIPCHK(hipStreamSynchronize(F->s_comm));
  for (auto &p : spans) {
    float ms = 0;
    hipEventElapsedTime(&ms, p.a, p.b);
    F->timer_ms[p.cat] += ms;
    F->timer_count[p.cat] += 1;
  }
  spans.clear();
  return 0;
}

// ---- one batch of steps
static int nan_terms_build(mnl_fields *F);  // the NaN guard (below)
static int nan_result(mnl_fields *F);

// does a D source point lie in the shell (outside the box the interior kernels own)?
static void dsrc_in_shell_scan(mnl_fields *F) {
  const Box &ib = F->fused ? F->fusedG : F->interior;
  F->dsrc_in_shell = false;
  for (long long idx : F->srcD_idx) {
    const long long i2 = idx / F->g.st[2], r = idx % F->g.st[2];
    const long long i1 = r / F->g.st[1], i0 = r % F->g.st[1];
    const long long ii[3] = {i0, i1, i2};
    bool in = true;
    for (int a = 0; a < 3; a++) in = in && ii[a] >= ib.lo[a] && ii[a] <= ib.hi[a];
    if (!in) F->dsrc_in_shell = true;
  }
}

// One step's row of the source table: the current of every group at time (B) and time + dt/2
// (D), complex, then the integrated dipoles real(amp * dipole(time + dt)) per point
struct SrcRow {
  size_t ng, nI, jofs, per;  // groups, dipole points, offset of the dipoles, doubles per step
  explicit SrcRow(const mnl_fields *F) : ng(F->groups.size()), nI(F->isrc_idx.size()) {
    jofs = (F->srcB_idx.size() || F->srcD_idx.size()) ? 4 * ng : 0;
    per = jofs + nI;
  }
};

// the source values of steps t0 .. t0 + ns - 1, computed on the host exactly as the reference,
// into d_vals
static int source_table(mnl_fields *F, long long t0, int ns, const SrcRow &row) {
  const size_t ng = row.ng, nI = row.nI, jofs = row.jofs, per = row.per;
  if (!per) return 0;
  const double dt = F->dt;
  std::vector<double> vals((size_t)ns * per);
  for (int s = 0; s < ns; s++) {
    long long tt = t0 + s;
    double time = tt * dt;
    double *vB = &vals[(size_t)s * per], *vD = vB + 2 * ng, *vI = vB + jofs;
    for (auto &st : F->srcs) st.update(time, dt);  // calc_sources(time())
    if (jofs)
      for (size_t g = 0; g < ng; g++) {
        const cplx J = F->srcs[F->groups[g].st].cur_current;
        vB[2 * g] = real(J), vB[2 * g + 1] = imag(J);
      }
    for (auto &st : F->srcs) st.update(time + 0.5 * dt, dt);
    if (jofs)
      for (size_t g = 0; g < ng; g++) {
        const cplx J = F->srcs[F->groups[g].st].cur_current;
        vD[2 * g] = real(J), vD[2 * g + 1] = imag(J);
      }
    for (auto &st : F->srcs) st.update(time + dt, dt);
    for (size_t k = 0; k < nI; k++) {
      const SrcGroup &G = F->groups[F->isrc_ref[k].first];
      const cplx A = G.amp[F->isrc_ref[k].second] * F->srcs[G.st].cur_dipole;
      vI[k] = F->part0 ? imag(A) : real(A);  // part 1 of complex fields: the imaginary part
    }
  }
  size_t bytes = vals.size() * sizeof(double);
  if (F->d_vals_cap < vals.size()) {
    HIPCHK(hipStreamSynchronize(F->stream));
    if (F->d_vals) hipFree(F->d_vals);
    HIPCHK(hipMalloc(&F->d_vals, bytes));
    F->d_vals_cap = vals.size();
  }
  HIPCHK(hipMemcpyAsync(F->d_vals, vals.data(), bytes, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));  // vals is a host temporary
  return 0;
}

// fields::update_dfts after t += 1 (src/step.cpp:125-127), s the chunk's step just taken; a
// rank's averages read its low ghost planes, which must hold this step's values first
static int post_step(mnl_fields *F, PhaseTimer &pt, int s, int cstate = -1) {
  const long long tn = F->t + s + 1;
  if (!dft_due(F, tn)) return 0;
  if (F->nranks > 1) {
    if (F->fused)
      HIPCHK(hipStreamWaitEvent(F->stream, F->ev_x0, 0));
    else if (exchange(F, 0))
      return fail("E halo exchange failed");
    if (exchange(F, 3)) return fail("DFT halo exchange failed");
  }
  if (wrap(F, 0) || wrap(F, 3)) return -1;  // periodic directions: the same ghosts
  const int k = pt.begin(TM_DFT);
  const int r = dft_update(F, tn, nullptr, cstate);
  pt.end(k);
  return r;
}

// the step's guard of the new state, after everything that writes it
static int step_guard(mnl_fields *F, int s) {
  nan_count(F, 1);
  F->nan_at = F->t + s + 1;
  return nan_launch(F);
}

// One rank's fused interior: the tile kernel and the polarization chunks' general kernel, in
// the timing span k (TM_BINT) that the caller opened and closes.  *nr_done: the NR box's E phase
// was launched here, beside the tile kernel.
static int fused_interior(mnl_fields *F, const ISrcDev &is, PhaseTimer &pt, int &k, bool *nr_done) {
  FusedArgs &fa = fused_args(F);
  int kr;
  if (const int ts = fa.ngen > 0 ? tile_gen_split(F) : 0) {
    // the polarization chunks' general items on `ts` CUs of a side
    // stream beside the tile kernel on the others (both read only the old buffers
    // and write the ping-pong partners: no ordering between them)
    if (ensure_aux_stream(F)) return -1;
    HIPCHK(hipEventRecord(F->ev_start, F->stream));
    HIPCHK(hipStreamWaitEvent(F->s_aux, F->ev_start, 0));
    fa.wg_limit = ts;
    kr = k_fused(fa, 1, F->s_aux, F->ctr_base);
    if (kr) return fused_fail("fused general kernel launch failed", kr);
    if (F->nr && F->nranks == 1 && nr_early_ok(F)) {
      const int ke = pt.begin(TM_E, F->s_aux);
      if (nr_fused_e(F, is, F->s_aux)) return -1;
      pt.end(ke, F->s_aux);
      *nr_done = true;
    }
    HIPCHK(hipEventRecord(F->ev_early, F->s_aux));
    fa.wg_limit = k_cu_count() - ts;
    kr = k_fused(fa, 4, F->stream, F->ctr_base);
    fa.wg_limit = 0;
    if (kr) return fused_fail("fused kernel launch failed", kr);
    HIPCHK(hipStreamWaitEvent(F->stream, F->ev_early, 0));
    F->fused_concurrent = true;
  } else {
    F->fused_concurrent = false;
    kr = k_fused(fa, 4, F->stream, F->ctr_base);
    if (kr) return fused_fail("fused kernel launch failed", kr);
    if (fa.ngen > 0) {
      pt.end(k);
      k = pt.next(k, TM_GEN);
      kr = k_fused(fa, 1, F->stream, F->ctr_base);
      if (kr) return fused_fail("fused general kernel launch failed", kr);
    }
  }
  return 0;
}

// One step (step s of the chunk), one launch sequence per phase of fields::step
// (src/step.cpp:35-140): unfused, or fused on one rank.
// Its three parts, between which the ghost planes are made valid: step_one runs them on one
// field set, step_one_cplx on the two parts of complex fields.
static int step_one_bh(mnl_fields *F, const SrcDev &sB, const ISrcDev &is, PhaseTimer &pt,
                       bool *nr_done);
static int step_one_de(mnl_fields *F, const SrcDev &sD, const ISrcDev &is, PhaseTimer &pt,
                       bool nr_done);

static int step_one(mnl_fields *F, int s, const SrcDev &sB, const SrcDev &sD, const ISrcDev &is,
                    PhaseTimer &pt) {
  // ---- B: halo of E (low ghost), curl, sources
  if (!F->u_first_done[0] && u_lazy_copy(F, 0)) return -1;
  if (F->nranks > 1) {
    int k = pt.begin(TM_HALO);
    if (exchange(F, 0)) return fail("E halo exchange failed");
    pt.end(k);
  }
  if (any_periodic(F)) {  // step_boundaries(E_stuff) of the step before, at its first reader
    int k = pt.begin(TM_HALO);
    if (wrap(F, 0)) return -1;
    pt.end(k);
  }
  bool nr_done = false;  // the NR box's E phase already launched (beside the tile kernel)
  if (step_one_bh(F, sB, is, pt, &nr_done)) return -1;
  if (F->nranks > 1) {
    int kk = pt.begin(TM_HALO);
    if (exchange(F, 1)) return fail("H halo exchange failed");
    pt.end(kk);
  }
  if (any_periodic(F)) {
    int kk = pt.begin(TM_HALO);
    if (wrap(F, 1)) return -1;
    pt.end(kk);
  }
  if (step_one_de(F, sD, is, pt, nr_done)) return -1;
  if (post_step(F, pt, s)) return -1;
  return step_guard(F, s);
}

// One step of complex fields (one rank, or unfused on several): each part of the step on part 0, then on part 1 (one
// stream), then the phased wrap of both, then the DFT samples of both.
static int step_one_cplx(mnl_fields *const P[2], int s, const SrcDev sB[2], const SrcDev sD[2],
                         const ISrcDev is[2], PhaseTimer &pt) {
  mnl_fields *F = P[0];
  for (int p = 0; p < 2; p++)
    if (!P[p]->u_first_done[0] && u_lazy_copy(P[p], 0)) return -1;
  // several ranks (unfused): one exchange lists both parts' planes, then the rank-local wrap
  if (F->nranks > 1 || any_periodic(F)) {
    int k = pt.begin(TM_HALO);
    if (F->nranks > 1 && exchange(F, 0)) return fail("E halo exchange failed");
    if (wrap(F, 0)) return -1;
    pt.end(k);
  }
  bool nr_done = false;
  for (int p = 0; p < 2; p++)
    if (step_one_bh(P[p], sB[p], is[p], pt, &nr_done)) return -1;
  if (F->nranks > 1 || any_periodic(F)) {
    int k = pt.begin(TM_HALO);
    if (F->nranks > 1 && exchange(F, 1)) return fail("H halo exchange failed");
    if (wrap(F, 1)) return -1;
    pt.end(k);
  }
  for (int p = 0; p < 2; p++)
    if (step_one_de(P[p], sD[p], is[p], pt, false)) return -1;
  // fields::update_dfts: both parts sample a row (part 1 first: part 0's update accumulates
  // the rows of both once its buffer is full, dft_flush)
  if (dft_due(F, F->t + s + 1)) {
    if (F->nranks > 1 && (exchange(F, 0) || exchange(F, 3))) return fail("DFT halo exchange failed");
    if (wrap(F, 0) || wrap(F, 3)) return -1;
    const int k = pt.begin(TM_DFT);
    const int r = dft_update(P[1], P[1]->t + s + 1) || dft_update(F, F->t + s + 1);
    pt.end(k);
    if (r) return -1;
  }
  for (int p = 0; p < 2; p++)
    if (step_guard(P[p], s)) return -1;
  return 0;
}

static int step_one_bh(mnl_fields *F, const SrcDev &sB, const ISrcDev &is, PhaseTimer &pt,
                       bool *nr_done_out) {
  DevFields &f = F->f;
  const DevGrid &g = F->g;
  const int nB = sB.n;
  const BoxList *sl = F->fused ? &F->fused_shell : &F->shell_list;
  int k = pt.begin(TM_BINT);
  bool &nr_done = *nr_done_out;
  if (F->fused) {
    if (fused_interior(F, is, pt, k, &nr_done)) return -1;
  } else if (k_curl(T_B, F->interior, nullptr, g, f, F->planB, F->S.courant, F->stream)) {
    return fail("curl B launch failed");
  }
  pt.end(k);
  // shell curl B; the PML H update rides along when no B source sits between
  // (timing events only around phases that launch something: an event record
  // between two kernels costs a few microseconds of GPU time)
  const bool fuseH = nB == 0 && !F->first_step_mode && !F->hall;
  const bool shell_work = sl->n > 0 && sl->start[sl->n] > 0;
  k = shell_work ? pt.begin(TM_B) : -1;
  if (k_curl(T_B, F->interior, sl, g, f, F->planB, F->S.courant, F->stream, fuseH))
    return fail("curl B launch failed");
  pt.end(k);
  if (nB && k_source(T_B, g, f, sB, 0, F->stream)) return fail("source launch failed");
  // ---- H
  if (!F->h_first_done && h_lazy_copy(F)) return -1;
  bool anyH = F->hall;
  for (int d = 0; d < 3; d++) anyH = anyH || f.H[d];
  k = (!fuseH && anyH && (shell_work || F->hall)) ? pt.begin(TM_H) : -1;
  if (!fuseH && update_h_any(F, *sl, true)) return -1;
  pt.end(k);
  return 0;
}

static int step_one_de(mnl_fields *F, const SrcDev &sD, const ISrcDev &is, PhaseTimer &pt,
                       bool nr_done) {
  DevFields &f = F->f;
  const DevGrid &g = F->g;
  const int nD = sD.n, nI = is.n;
  const BoxList *sl = F->fused ? &F->fused_shell : &F->shell_list;
  const bool shell_work = sl->n > 0 && sl->start[sl->n] > 0;
  // ---- D
  if (!F->u_first_done[1] && u_lazy_copy(F, 1)) return -1;
  int k = !F->fused ? pt.begin(TM_DINT) : -1;
  if (!F->fused && k_curl(T_D, F->interior, nullptr, g, f, F->planD, F->S.courant, F->stream))
    return fail("curl D launch failed");
  pt.end(k);
  // shell curl D; the shell E update rides along when it only reads its own D
  const bool fuseE = !F->nr && !F->upnl && f.npol == 0 && nI == 0 && !F->dsrc_in_shell &&
                     !F->first_step_mode;
  k = shell_work ? pt.begin(TM_D) : -1;
  if (k_curl(T_D, F->interior, sl, g, f, F->planD, F->S.courant, F->stream, fuseE))
    return fail("curl D launch failed");
  pt.end(k);
  if (nD && k_source(T_D, g, f, sD, 0, F->stream)) return fail("source launch failed");
  if ((F->nr || F->upnl) && F->nranks > 1) {
    if (exchange(F, 2)) return fail("D halo exchange failed");
  }
  if ((F->nr || F->upnl) && wrap(F, 2)) return -1;
  // ---- E (+ Lorentzian P)
  if (!F->e_first_done && e_lazy_copy(F)) return -1;
  if (F->fused && F->nr) {  // one rank: the fused kernels did all but the NR box
    if (!nr_done) {
      k = pt.begin(TM_E);
      if (nr_fused_e(F, is)) return -1;
      pt.end(k);
    }
  } else {
    // neighbour reads of D - P (NR, upstream chi) or of W (anisotropic sigma):
    // P after all of E
    bool fuse = !F->nr && !F->upnl && !f.aniso;
    k = (!F->fused || (!fuseE && shell_work) || (!fuse && f.npol) || f.aniso || f.wall_e)
            ? pt.begin(TM_E)
            : -1;
    if (nr_defer_begin(F)) return -1;
    if (!F->fused && F->nr && F->S.dim == 3) {
      if (nr_interior_e(F, is)) return -1;
    } else if (!F->fused && k_update_e(F->interior, nullptr, g, f, is, 0, fuse, F->stream)) {
      return fail("update E launch failed");
    }
    if (!fuseE) {
      // no chi2 outside the interior: the shell boxes never take the NR branch, so
      // they run the plain E kernel (same values, without the NR kernel's registers)
      DevFields plain = f;
      if (F->nr && F->nr_split_done && F->nr_shell_free) plain.nr_enabled = 0;
      if (k_update_e(F->interior, sl, g, plain, is, 0, fuse, F->stream))
        return fail("update E launch failed");
    }
    if (nr_defer_end(F)) return -1;
    if (f.aniso && !f.wall_e && k_aniso_wall(g, f, 0, F->stream))
      return fail("wall W launch failed");
    if (f.aniso && F->nranks > 1 && exchange(F, 4))  // WE_stuff ghosts (step.cpp:111-114)
      return fail("W halo exchange failed");
    if (f.aniso && wrap(F, 4)) return -1;
    if (!fuse && f.npol) {
      if (k_update_pols(F->interior, nullptr, g, f, F->stream) ||
          k_update_pols(F->interior, sl, g, f, F->stream))
        return fail("pols launch failed");
    }
    if ((f.aniso || f.wall_e) && k_aniso_wall(g, f, 1, F->stream))
      return fail("wall W launch failed");
    pt.end(k);
  }
  if (F->fused) swap_cur_nxt(f);
  return 0;
}

// step_batch for complex fields: both parts prepared, then stepped in lockstep one step at a
// time (no pairs of steps); each part has its own source table (part 1's amplitudes are -i times
// part 0's, so that it adds imag(A J) where part 0 adds real(A J), src/step.cpp:300-315) and
// its own NaN guard.
static int step_batch_cplx(mnl_fields *F, int nsteps) {
  mnl_fields *const P[2] = {F, F->twin.get()};
  for (mnl_fields *p : P) {
    if (p->src_dirty && build_source_lists(p)) return -1;
    p->tb_last = false;
  }
  // the same mode for both; several ranks step complex fields unfused
  const bool fuse = F->nranks == 1 && fused_agreed(P[0]) && fused_agreed(P[1]);
  for (mnl_fields *p : P) {
    if (set_fused(p, fuse)) return -1;
    dsrc_in_shell_scan(p);
    if (nan_terms_build(p)) return -1;
  }
  if (P[0]->fused != P[1]->fused)
    return fail("complex fields: the two parts did not enter the same stepping mode");
  const SrcRow row[2] = {SrcRow(P[0]), SrcRow(P[1])};
  PhaseTimer pt(F);
  for (int s0 = 0; s0 < nsteps; s0 += NAN_CH) {
    const int ns = std::min(NAN_CH, nsteps - s0);
    for (int p = 0; p < 2; p++) {
      if (!P[p]->dfts.empty() && dft_prepare(P[p], P[p]->t, ns)) return -1;
      if (source_table(P[p], P[p]->t, ns, row[p])) return -1;
    }
    for (int s = 0; s < ns; s++) {
      SrcDev sB[2], sD[2];
      ISrcDev is[2];
      for (int p = 0; p < 2; p++) {
        P[p]->f.nr_t = P[p]->t + s;
        const double *vs = P[p]->d_vals + (size_t)s * row[p].per;
        sB[p] = src_dev(P[p], 0, vs), sD[p] = src_dev(P[p], 1, vs + 2 * row[p].ng);
        is[p] = P[p]->isrc_dev;
        is[p].n = (int)row[p].nI;
        is[p].val = vs + row[p].jofs;
      }
      if (step_one_cplx(P, s, sB, sD, is, pt)) return -1;
    }
    for (mnl_fields *p : P) p->t += ns;
    if (pt.flush() != 0) return -1;
    for (mnl_fields *p : P)
      if (nan_result(p)) return -1;
  }
  for (mnl_fields *p : P)
    if (p->s_aux) HIPCHK(hipStreamSynchronize(p->s_aux));
  HIPCHK(hipStreamSynchronize(F->stream));
  HIPCHK(hipGetLastError());
  return 0;
}

static int step_batch(mnl_fields *F, int nsteps) {
  if (F->twin) return step_batch_cplx(F, nsteps);
  if (F->src_dirty && build_source_lists(F)) return -1;
  if (set_fused(F, fused_agreed(F))) return -1;
  dsrc_in_shell_scan(F);
  if (F->fused && F->nranks > 1 && multi_begin(F)) return -1;
  if (nan_terms_build(F)) return -1;  // NaN guard terms of this batch's mode / arrays
  bool tb_ok = false;  // step in pairs (temporal blocking; its plan stores the guard's points)
  if (nsteps >= 2 && tb_usable(F, &tb_ok)) return -1;
  if (nsteps >= 2) F->tb_last = tb_ok;
  const SrcRow row(F);
  const size_t ng = row.ng, per = row.per;
  PhaseTimer pt(F);
  for (int s0 = 0; s0 < nsteps; s0 += NAN_CH) {  // a chunk: one source table, one NaN flag read
    const int ns = std::min(NAN_CH, nsteps - s0);
    if (!F->dfts.empty() && dft_prepare(F, F->t, ns)) return -1;
    if (!F->ldoses.empty() && ldos_prepare(F, F->t, ns)) return -1;
    if (source_table(F, F->t, ns, row)) return -1;
    for (int s = 0; s < ns; s++) {
      F->f.nr_t = F->t + s;  // seeds of the NR random fallback (nr_voxel_seed)
      const double *vs = F->d_vals + (size_t)s * per;  // this step's row
      const SrcDev sB = src_dev(F, 0, vs), sD = src_dev(F, 1, vs + 2 * ng);
      ISrcDev is = F->isrc_dev;
      is.n = (int)row.nI;
      is.val = vs + row.jofs;  // kernels index val[step * n + orig] with step 0
      if (tb_ok && s + 1 < ns) {  // steps s and s + 1 as one pair
        const SrcDev sD1 = src_dev(F, 1, vs + per + 2 * ng);
        if (F->nranks > 1 ? tb_pair_multi(F, sD, sD1, pt, F->t + s + 1)
                          : tb_pair(F, sD, sD1, pt, F->t + s + 1))
          return -1;
        s++;
        if (post_step(F, pt, s, 1)) return -1;  // DFT of the pair's second step (the new state)
        continue;
      }
      if (tb_chain_join(F)) return -1;
      if (F->fused && F->nranks > 1) {
        if (step_fused_multi(F, sD, pt) || post_step(F, pt, s) || step_guard(F, s)) return -1;
      } else if (step_one(F, s, sB, sD, is, pt)) {
        return -1;
      }
    }
    // buffered DFT updates stay buffered across chunks and calls (a run that steps one step
    // per call accumulates once per kb updates, not once per call); readers flush first
    F->t += ns;
    if (pt.flush() != 0) return -1;
    if (nan_result(F)) return -1;  // stop within NAN_CH steps of a failing guard
  }
  if (F->s_comm) {
    HIPCHK(hipStreamSynchronize(F->s_comm));
    HIPCHK(hipStreamSynchronize(F->s_aux));
  }
  F->tb_chain_pending = false;
  HIPCHK(hipStreamSynchronize(F->stream));
  HIPCHK(hipGetLastError());
  if (F->d_clk && clk_dump(F)) return -1;
  return nan_result(F);
}

// NaN guard (src/step.cpp:138-139): abort when get_field(D_EnergyDensity, gv.center()) is
// not finite (src/monitor.cpp:96-113: 1/2 sum_d real(conj(E_d) D_d), each value interpolated
// as get_field does, src/monitor.cpp:127-160).  The terms (this rank's points of the 8-point
// stencils, which array, weight) are built once per batch on the host; nan_check_kernel sums
// them on the device after the step, and the host reads the flag once, at the end of the
// batch (no round trip per step).  Multi-rank: each rank checks its share and the ranks agree.
static int nan_terms_build(mnl_fields *F) {
  const mnl_structure &S = F->S;
  NanTerms &t = F->nan_terms;
  t.n = 0;
  double cen[3] = {0, 0, 0};
  for (int d = 0; d < 3; d++)
    if (S.has[d]) {
      int n = S.n[d] - (S.n[d] & 1);
      cen[d] = (S.io[d] + n) * (0.5 * (1.0 / S.a));
    }
  if (S.dim == 1) cen[0] = cen[1] = 0;
  if (S.dim == 2) cen[2] = 0;
  for (int d = 0; d < 3; d++) {
    if (!F->allocated[d] || !F->allocated[3 * T_D + d]) continue;
    for (int which = 0; which < 2; which++) {  // E_d terms, then D_d terms
      const int c = which == 0 ? d : 3 * T_D + d;
      int locs[8][3];
      double w[8];
      interpolate(S, c, cen, locs, w);
      for (int i = 0; i < 8 && w[i]; i++) {
        int jg[3] = {0, 0, 0};
        bool in = true;
        for (int e = 0; e < 3; e++)
          if (S.has[e]) {
            const int o = locs[i][e] - S.io[e];
            if (!(o > 0 && o <= 2 * S.n[e])) in = false;
            jg[e] = (locs[i][e] - S.io[e] - S.shift(c, e)) / 2;
          }
        if (!in) continue;
        const long long li = local_index(F, c, jg, true);
        if (li < 0) continue;
        if (t.n >= NAN_MAXT) return fail("NaN guard: too many terms");
        t.dir[t.n] = (unsigned char)d;
        t.kind[t.n] = which == 1 ? 2 : (in_fused_box(F, c, jg) ? 1 : 0);
        t.idx[t.n] = li;
        t.w[t.n] = w[i];
        t.n++;
      }
    }
  }
  return 0;
}

// launch the guard on the current state (or the given E / D arrays: the middle state of a
// pair) if one is due
int nan_launch(mnl_fields *F, hipStream_t st, double *const *Es, double *const *Ds) {
  if (!F->nan_due) return 0;
  F->nan_due = false;
  if (!st) st = F->stream;
  if (!F->d_nanflag && dev_alloc(F, &F->d_nanflag, 2)) return -1;  // zeroed; reset by nan_result
  const double *E[3], *D[3], *U[3];
  for (int d = 0; d < 3; d++)
    E[d] = Es ? Es[d] : F->f.E[d], D[d] = Ds ? Ds[d] : F->f.D[d], U[d] = F->f.inveps[d];
  if (k_nan_check(F->nan_terms, E, D, U, F->d_nanflag, (int)F->nan_at, st))
    return fail("NaN guard launch failed");
  F->nan_launched++;
  return 0;
}

// after k steps: count them, mark a guard due every nan_every steps (across calls)
void nan_count(mnl_fields *F, int k) {
  F->since_nan += k;
  if (F->since_nan >= F->nan_every) {
    F->since_nan = 0;
    F->nan_due = true;
  }
}

// end of a chunk of a batch: the reference's abort (src/step.cpp:138-139) if a guard saw NaN /
// Inf.  The message names the first failing step (the step after which the reference's check
// aborts); the time stays at the state the device holds -- the fields, the ping-pong buffers
// and the DFT accumulators have advanced past the failing step to the end of the chunk (at most
// NAN_CH steps), and t says so, so a caller that catches the error reads arrays labelled with
// their own time.  Multi-rank: every rank learns the earliest failing step of any rank.
static int nan_result(mnl_fields *F) {
  if (F->nan_launched == 0) return 0;  // the same on every rank (same step counts)
  if (F->s_comm) HIPCHK(hipStreamSynchronize(F->s_comm));
  HIPCHK(hipStreamSynchronize(F->stream));
  int h[2] = {0, 0};
  HIPCHK(hipMemcpy(h, F->d_nanflag, sizeof h, hipMemcpyDeviceToHost));
  if (h[0]) HIPCHK(hipMemset(F->d_nanflag, 0, sizeof h));
  F->nan_launched = 0;
  long long bad_t = h[0] ? (long long)h[1] : -1;
  if (F->nranks > 1) {
    std::vector<double> v(F->nranks, 0.0);
    v[F->rank] = double(bad_t);
    if (F->comm->allreduce_sum(v.data(), F->nranks, F->stream)) return fail("allreduce failed");
    bad_t = -1;
    for (double x : v)
      if (x >= 0 && (bad_t < 0 || (long long)x < bad_t)) bad_t = (long long)x;
  }
  if (bad_t < 0) return 0;
  return fail("simulation fields are NaN or Inf (at time step " + std::to_string(bad_t) +
              "; fields left at time step " + std::to_string(F->t) + ")");
}

static int fields_step_batches(mnl_fields *F, int nsteps);

// fields::step (src/step.cpp:40-140) over nsteps: the time spent goes to the
// reference's time sinks (per-phase kernel times when profiling is on, the
// rest to "time stepping"), and rank 0 prints "on time step ..." at most every
// MEEP_MIN_OUTPUT_TIME (4 s, src/meep.hpp:48) when verbosity > 0.
int fields_step(mnl_fields *F, int nsteps) {
  const double w0 = wall_now();
  double ms0[TM_N];
  for (int k = 0; k < TM_N; k++) ms0[k] = F->timer_ms[k];
  if (F->t == 0 || F->last_out_wall < 0) F->last_out_wall = w0, F->last_out_t = F->t;
  const int r = fields_step_batches(F, nsteps);
  const double wall = wall_now() - w0;
  auto dsec = [&](int k) { return (F->timer_ms[k] - ms0[k]) * 1e-3; };
  double parts[MNL_NUM_TIME_SINKS] = {0};
  if (F->profiling) {
    parts[MNL_SINK_UPDATE_B] = dsec(TM_B) + (F->fused ? 0.0 : dsec(TM_BINT));
    parts[MNL_SINK_UPDATE_H] = dsec(TM_H);
    parts[MNL_SINK_UPDATE_D] = dsec(TM_D) + dsec(TM_DINT);
    parts[MNL_SINK_UPDATE_E] = dsec(TM_E);
    parts[MNL_SINK_BOUNDARIES] = dsec(TM_HALO);
    parts[MNL_SINK_FOURIER] = dsec(TM_DFT) + dsec(TM_DFTF);
  }
  double rest = wall;
  for (int k = 0; k < MNL_NUM_TIME_SINKS; k++) F->sink_s[k] += parts[k], rest -= parts[k];
  F->sink_s[MNL_SINK_STEPPING] += std::max(rest, 0.0);
  return r;
}

static int fields_step_batches(mnl_fields *F, int nsteps) {
  while (nsteps > 0) {
    int m;
    mnl_fields *T = F->twin.get();  // complex fields: part 1 takes its first step with part 0
    if (T && T->force_unfused_next) F->force_unfused_next = true;
    if (!F->e_first_done || !F->h_first_done || !F->u_first_done[0] || !F->u_first_done[1] ||
        F->force_unfused_next) {
      const bool saved = F->allow_fused;
      F->allow_fused = false;
      F->first_step_mode = true;
      if (T) T->allow_fused = false, T->first_step_mode = true;
      const int r = step_batch(F, 1);
      F->allow_fused = saved;
      F->first_step_mode = false;
      if (T) T->allow_fused = saved, T->first_step_mode = false, T->force_unfused_next = false;
      if (r) return -1;
      F->force_unfused_next = false;
      m = 1;
    } else {
      m = nsteps;  // the NaN guard runs on the device inside the batch (nan_launch)
      if (step_batch(F, m)) return -1;
    }
    nsteps -= m;
    if (g_verbosity > 0 && F->rank == 0) {
      const double now = wall_now();
      if (now > F->last_out_wall + 4.0 && F->t > F->last_out_t) {
        printf("on time step %lld (time=%g), %g s/step\n", F->t, F->t * F->dt,
               (now - F->last_out_wall) / double(F->t - F->last_out_t));
        fflush(stdout);
        F->last_out_wall = now;
        F->last_out_t = F->t;
      }
    }
  }
  return 0;
}

}  // namespace mnlh