// mnl_host.cpp -- the C-ABI (include/meep_nl_amd.h) of the MI355X fields::step() path: argument
// checks, the device selection and a call into one of the files below (or a few lines on the
// structure / fields object itself); besides them the creation of fields with its environment
// reads and the table of scheduling options.
// The host side is built with g++ (not hipcc) on purpose: the per-step source amplitudes use
// std::complex / libm exactly as the reference does (src/sources.cpp:72-160,
// src/step.cpp:296-319), so the values handed to the GPU are bit-identical to the reference's.
// Its other files: mnl_setup.cpp (PML tables, grid, allocation, materials), mnl_sources.cpp
// (sources, get_field), mnl_fused.cpp (fused-tile planning), mnl_tb.cpp (pairs of steps),
// mnl_step.cpp (the step loop, NaN guard), mnl_tune.cpp (the tuner), mnl_dft.cpp, mnl_io.cpp,
// mnl_stats.cpp (kernel statistics, the byte model, tb_info, the mode word), mnl_comm.cpp.
#include "mnl_host.hpp"

namespace mnlh {
thread_local std::string g_err;
int g_verbosity = 1;

// share: the communicator of part 0 of complex fields, which part 1 (the fields created here)
// uses for its slab of the same rank: every collective of part 1 follows part 0's on the same
// host thread, in the same order on every rank
static mnl_fields *create_common(mnl_structure *s, int device, int rank, int nranks, const void *id,
                          LocalHub *hub = nullptr, std::shared_ptr<Comm> share = nullptr) {
  if (!s) {
    fail("null structure");
    return nullptr;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    fail("no HIP device available (the MI355X path has no CPU fallback)");
    return nullptr;
  }
  std::unique_ptr<mnl_fields> F(new mnl_fields());
  F->S = *s;
  F->dt = s->dt;
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  if (device >= ndev) {
    fail("device index out of range");
    return nullptr;
  }
  F->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&F->stream, hipStreamNonBlocking) != hipSuccess) {
    fail("cannot create HIP stream");
    return nullptr;
  }
  memset(&F->f, 0, sizeof(F->f));
  F->rank = rank;
  F->nranks = nranks;
  if (nranks > 1 && share) {
    F->comm = share;
  } else if (nranks > 1) {
    F->comm.reset(new Comm());
    if (hub ? F->comm->init_local(rank, nranks, hub) : F->comm->init(rank, nranks, id)) {
      fail(hub ? "local slab group init failed"
               : Comm::is_ipc_id(id) ? "IPC slab group init failed (shared-memory id)"
                                     : std::string("RCCL communicator init failed (") +
                                           comm_last_error() +
                                           "); MNL_COMM=ipc runs the same slabs over the "
                                           "IPC transport");
      return nullptr;
    }
  }
  if (const char *zc = getenv("MNL_FUSED_ZCHUNK")) {
    F->fused_zchunk = std::max(0, atoi(zc));
    F->fused_zchunk_env = true;  // the tuner keeps it
  }
  if (const char *tb = getenv("MNL_TB")) F->tb_enabled = atoi(tb) != 0, F->tb_env = true;
  if (const char *tz = getenv("MNL_TB_ZCHUNK"))
    F->tb_zchunk = std::max(0, atoi(tz)), F->tb_zchunk_env = true;
  if (const char *tn = getenv("MNL_TB_NARROW")) F->tb_narrow = atoi(tn) != 0;
  if (const char *to = getenv("MNL_TB_OOM")) F->tb_oom_test = atoi(to) != 0;
  if (const char *dc = getenv("MNL_DFT_CMP")) F->dft_cmp = atoi(dc) != 0;
  if (const char *ne = getenv("MNL_NR_EARLY")) F->nr_early = atoi(ne) != 0;
  if (const char *nf = getenv("MNL_NO_FUSED")) F->allow_fused = atoi(nf) == 0;
  if (const char *ne = getenv("MNL_NAN_EVERY")) F->nan_every = std::max(1, atoi(ne));
  if (const char *sg = getenv("MNL_STAGGER")) F->stagger = std::max(0, atoi(sg)) / 128 * 128;
  if (const char *ar = getenv("MNL_ARENA")) F->arena_req = std::max(0, atoi(ar));
  if (const char *cg = getenv("MNL_CONTIG")) F->contig = atoi(cg) != 0;
  if (const char *ag = getenv("MNL_ARENA_GAP")) F->arena_gap = std::max(0, atoi(ag)) / 128 * 128;
  auto env_is = [](const char *name, char v) {
    const char *e = getenv(name);
    return e && e[0] == v;
  };
  F->no_palette = env_is("MNL_NO_PALETTE", '1');
  if (const char *e = getenv("MNL_TILE_GEN_CUS")) {
    F->tile_gen_cus = std::max(0, atoi(e));
    F->tile_gen_cus_env = true;
  }
  F->nr_defer = !env_is("MNL_NR_DEFER", '0');
  F->tile_stats = getenv("MNL_TILE_STATS") != nullptr;
  F->tb_stats = getenv("MNL_TB_STATS") != nullptr;
  if (const char *ck = getenv("MNL_ITEM_CLOCK")) F->clk_path = ck;
  if (finalize_fields(F.get())) return nullptr;
  if (!F->clk_path.empty() && (dev_alloc(F.get(), &F->d_clk, (size_t)CLK_CAP * CLK_REC) ||
                               dev_alloc(F.get(), &F->d_clk_n, 1)))
    return nullptr;
  return F.release();
}

// mnl_fields_set_schedule's options (MNL_SCHED_* of include/meep_nl_amd.h), one row each: a
// switch stores value != 0 in `flag`; a count is stored in `count` when it is 0 or lies in
// lo .. hi, and fails with `err` otherwise.
struct SchedOpt {
  int id;
  const char *name;
  bool mnl_fields::*flag;
  int mnl_fields::*count;
  int lo, hi;
  const char *err;
  bool replan;  // the pair plan is rebuilt at the next batch
};
static const SchedOpt SCHED_OPTS[] = {
    {MNL_SCHED_NARROW, "narrow", &mnl_fields::tb_narrow, nullptr, 0, 0, nullptr, true},
    {MNL_SCHED_DFT_PAL, "dft_pal", &mnl_fields::dft_pal, nullptr, 0, 0, nullptr, true},
    {MNL_SCHED_RES, "res", nullptr, &mnl_fields::tb_res, -1, 1024, "bad reservation", false},
    {MNL_SCHED_RES_TB2, "res_tb2", nullptr, &mnl_fields::res_l, -1, 1024, "bad reservation", false},
    {MNL_SCHED_RES_RIM, "res_rim", nullptr, &mnl_fields::res_r, -1, 1024, "bad reservation", false},
    {MNL_SCHED_DFT_CMP, "dft_cmp", &mnl_fields::dft_cmp, nullptr, 0, 0, nullptr, true},
    {MNL_SCHED_RIM_ZCHUNK, "rim_zchunk", nullptr, &mnl_fields::rim_zchunk, 0, FUSED_MAXCH,
     "bad rim chunk", true},
    {MNL_SCHED_NR_EARLY, "nr_early", &mnl_fields::nr_early, nullptr, 0, 0, nullptr, true},
    {MNL_SCHED_TB_ZCHUNK, "tb_zchunk", nullptr, &mnl_fields::tb_zchunk, 0, 4096,
     "bad two-step chunk", true},
    {MNL_SCHED_TB_OX, "tb_ox", nullptr, &mnl_fields::tb_ox, 4, TB_OXW, "bad two-step width", true},
    {MNL_SCHED_TB_POL, "tb_pol", &mnl_fields::tb_pol_on, nullptr, 0, 0, nullptr, true},
    {MNL_SCHED_R1_BESIDE, "r1_beside", &mnl_fields::tb_r1a, nullptr, 0, 0, nullptr, true},
    {MNL_SCHED_SRC_GUARD, "src_guard", &mnl_fields::tb_srcguard, nullptr, 0, 0, nullptr, false},
};

// a source of complex fields goes to both parts with the same amplitude A: part 0 adds
// real(A J), part 1 imag(A J) (build_source_lists, source_table)
static int add_source_parts(mnl_fields *F, int comp, int kind, const double *p, int np,
                            mnl_src_func func, void *fdata, const double vmin[3],
                            const double vmax[3], double amp_re, double amp_im, int is_integrated,
                            mnl_amp_func afunc, void *adata) {
  if (add_source_any(F, comp, kind, p, np, func, fdata, vmin, vmax, amp_re, amp_im, is_integrated,
                     afunc, adata))
    return -1;
  if (F && F->twin)
    return add_source_any(F->twin.get(), comp, kind, p, np, func, fdata, vmin, vmax, amp_re, amp_im,
                          is_integrated, afunc, adata);
  return 0;
}

}  // namespace mnlh

// =============================================================== C ABI
extern "C" {

const char *mnl_last_error(void) { return g_err.c_str(); }
int mnl_version(void) { return 100; }

int mnl_device_count(int *count) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
  *count = n;
  return 0;
}

mnl_structure *mnl_structure_create(int dim, const int n[3], double a, double courant,
                                    const int io[3]) {
  if (dim < 1 || dim > 3) {
    fail("dim must be 1, 2 or 3");
    return nullptr;
  }
  if (!(a > 0) || !(courant > 0)) {
    fail("resolution and Courant must be positive");
    return nullptr;
  }
  mnl_structure *s = new mnl_structure();
  s->dim = dim;
  s->has[0] = dim >= 2;
  s->has[1] = dim >= 2;
  s->has[2] = dim != 2;
  for (int d = 0; d < 3; d++) {
    s->n[d] = s->has[d] ? n[d] : 0;
    s->io[d] = s->has[d] ? io[d] : 0;
    if (s->has[d] && s->n[d] < 2) {
      delete s;
      fail("need at least 2 cells along every present direction");
      return nullptr;
    }
    for (int k = 0; k < 2; k++) s->pml_R[d][k] = 1e-15, s->pml_stretch[d][k] = 1.0;
  }
  s->a = a;
  s->courant = courant;
  s->dt = courant / a;  // src/structure.cpp:110
  s->ntot = 1;
  for (int d = 0; d < 3; d++)
    if (s->has[d]) s->ntot *= size_t(s->n[d] + 1);
  return s;
}

void mnl_structure_destroy(mnl_structure *s) { delete s; }

int mnl_structure_add_pml(mnl_structure *s, int dir, int side, double thickness, double R,
                          double mean_stretch) {
  if (!s || dir < 0 || dir > 2 || side < 0 || side > 1) return fail("bad pml direction/side");
  if (thickness < 0) return fail("invalid boundary absorbers for this grid_volume");
  if (!s->has[dir]) return 0;
  s->pml_thick[dir][side] = thickness;
  s->pml_R[dir][side] = R;
  s->pml_stretch[dir][side] = mean_stretch;
  return 0;
}

int mnl_structure_set_chi1inv(mnl_structure *s, int comp, int dir, const double *host) {
  if (!s || comp < MNL_EX || comp > MNL_HZ || dir < 0 || dir > 2)
    return fail("chi1inv: E or H components only");
  auto &dst = comp <= MNL_EZ ? s->chi1inv[comp][dir] : s->mu1inv[comp - MNL_HX][dir];
  if (host)
    dst.assign(host, host + s->ntot);
  else
    dst.clear();
  return 0;
}
int mnl_structure_set_chi2(mnl_structure *s, int comp, const double *host) {
  if (!s || comp < MNL_EX || comp > MNL_EZ) return fail("chi2: E components only");
  s->chi2[comp].assign(host, host + s->ntot);
  return 0;
}
int mnl_structure_set_conductivity(mnl_structure *s, int comp, const double *host) {
  // structure_chunk::set_conductivity (src/structure.cpp:868-905): E/H name the
  // D/B array; an E value is multiplied by the current diagonal chi1inv
  if (!s || comp < 0 || comp >= MNL_NUM_COMPONENTS) return fail("invalid component for conductivity");
  const int t = ctype(comp), d = cdir(comp), tb = (t == T_D || t == T_E) ? 1 : 0;
  auto &dst = s->cond[tb][d];
  if (!host) {
    dst.clear();
    return 0;
  }
  dst.assign(host, host + s->ntot);
  if (t == T_E && !s->chi1inv[d][d].empty())
    for (size_t i = 0; i < s->ntot; i++) dst[i] = host[i] * s->chi1inv[d][d][i];
  return 0;
}

int mnl_structure_set_chi3(mnl_structure *s, int comp, const double *host) {
  if (!s || comp < MNL_EX || comp > MNL_EZ) return fail("chi3: E components only");
  s->chi3[comp].assign(host, host + s->ntot);  // inert in the fork
  return 0;
}
int mnl_structure_add_lorentzian(mnl_structure *s, double omega0, double gamma, int drude,
                                 const double *sx, const double *sy, const double *sz) {
  const double *sig[9] = {sx, nullptr, nullptr, nullptr, sy, nullptr, nullptr, nullptr, sz};
  return mnl_structure_add_lorentzian_tensor(s, omega0, gamma, drude, sig);
}

int mnl_structure_add_lorentzian_tensor(mnl_structure *s, double omega0, double gamma, int drude,
                                        const double *const sigma[9]) {
  if (!s || !sigma) return fail("null argument");
  if ((int)s->lor.size() >= MAX_POL) return fail("too many susceptibilities (max 4)");
  Lorentz L;
  L.omega0 = omega0;
  L.gamma = gamma;
  L.drude = drude;
  for (int c = 0; c < 3; c++)
    for (int d = 0; d < 3; d++) {
      const double *v = sigma[3 * c + d];
      if (!v) continue;
      auto &dst = d == c ? L.sigma[c] : L.off[c][d];
      dst.assign(v, v + s->ntot);
      if (all_eq(dst, 0.0)) dst.clear();
    }
  s->lor.push_back(std::move(L));
  return 0;
}
int mnl_structure_add_magnetic_lorentzian(mnl_structure *s, double omega0, double gamma,
                                          int drude, const double *sx, const double *sy,
                                          const double *sz) {
  if (!s) return fail("null argument");
  if ((int)s->hlor.size() >= MAX_HPOL) return fail("too many magnetic susceptibilities (max 2)");
  Lorentz L;
  L.omega0 = omega0;
  L.gamma = gamma;
  L.drude = drude;
  const double *sv[3] = {sx, sy, sz};
  for (int d = 0; d < 3; d++) {
    if (!sv[d]) continue;
    L.sigma[d].assign(sv[d], sv[d] + s->ntot);
    if (all_eq(L.sigma[d], 0.0)) L.sigma[d].clear();
  }
  s->hlor.push_back(std::move(L));
  return 0;
}
int mnl_structure_set_nonlinear_mode(mnl_structure *s, int mode) {
  if (!s || mode < 0 || mode > 1) return fail("nonlinear mode must be 0 (fork) or 1 (upstream)");
  s->nl_mode = mode;
  return 0;
}

int mnl_sphere_quadrature(int dim, double *xyzw) {
  if (dim < 1 || dim > 3) return fail("sphere quadrature: dim must be 1, 2 or 3");
  return sphere_quadrature(dim, xyzw);
}

int mnl_structure_set_epsilon_geometry(mnl_structure *s, int device, int nobj, const double *objs,
                                       double default_eps, int use_averaging, double tol,
                                       int maxeval) {
  if (!s || nobj < 0 || (nobj > 0 && !objs)) return fail("set_epsilon_geometry: bad arguments");
  return set_epsilon_geometry(s, device, nobj, objs, default_eps, use_averaging, tol, maxeval);
}

int mnl_structure_get_chi1inv(mnl_structure *s, int comp, int dir, double *host) {
  if (!s || comp < MNL_EX || comp > MNL_HZ || dir < 0 || dir > 2)
    return fail("chi1inv: E or H components only");
  const auto &v = comp <= MNL_EZ ? s->chi1inv[comp][dir] : s->mu1inv[comp - MNL_HX][dir];
  if (v.empty()) return 1;
  if (host) memcpy(host, v.data(), sizeof(double) * v.size());
  return 0;
}

int mnl_structure_set_box(mnl_structure *s, int kind, int index, const double box[6],
                          double value) {
  if (!s || kind < 0 || kind > 3) return fail("bad box kind");
  BoxSpec b;
  b.kind = kind;
  b.index = index;
  memcpy(b.box, box, sizeof(b.box));
  b.value = value;
  if (kind == 3) {  // make sure the susceptibility has a sigma array to fill
    if (index < 0 || index >= (int)s->lor.size()) return fail("box: no such susceptibility");
    for (int d = 0; d < 3; d++)
      if (s->lor[index].sigma[d].empty()) s->lor[index].sigma[d].assign(s->ntot, 0.0);
  }
  if (kind == 1) {
    for (int d = 0; d < 3; d++)
      if (s->chi2[d].empty()) s->chi2[d].assign(s->ntot, 0.0);
  }
  s->boxes.push_back(b);
  return 0;
}

mnl_fields *mnl_fields_create(mnl_structure *s, int device) {
  return create_common(s, device, 0, 1, nullptr);
}
mnl_fields *mnl_fields_create_dist(mnl_structure *s, int device, int rank, int nranks,
                                   const void *id) {
  if (nranks < 1 || rank < 0 || rank >= nranks) {
    fail("bad rank/nranks");
    return nullptr;
  }
  return create_common(s, device, rank, nranks, id);
}
void *mnl_local_hub_create(int nranks) {
  if (nranks < 1) {
    fail("bad nranks");
    return nullptr;
  }
  return local_hub_create(nranks);
}
void mnl_local_hub_destroy(void *hub) { local_hub_destroy((LocalHub *)hub); }
mnl_fields *mnl_fields_create_local(mnl_structure *s, int device, int rank, int nranks,
                                    void *hub) {
  if (!hub || nranks < 1 || rank < 0 || rank >= nranks) {
    fail("bad rank/nranks/hub");
    return nullptr;
  }
  return create_common(s, device, rank, nranks, nullptr, (LocalHub *)hub);
}
int mnl_slab_range(int ncell, int rank, int nranks, int *lo, int *hi) {
  if (nranks < 1 || rank < 0 || rank >= nranks || ncell < nranks) return fail("bad slab split");
  slab_range(ncell, rank, nranks, lo, hi);
  return 0;
}
int mnl_comm_unique_id(void *out128) { return Comm::unique_id(out128) ? fail("ncclGetUniqueId failed") : 0; }
int mnl_comm_ipc_id(void *out128, int nranks) {
  if (!out128) return fail("null id buffer");
  return Comm::ipc_id(out128, nranks) ? fail("cannot create the IPC shared-memory segment") : 0;
}
int mnl_comm_ipc_unlink(const void *id128) {
  return Comm::ipc_unlink(id128) ? fail("no such IPC shared-memory segment") : 0;
}
int mnl_comm_ipc_reduce(const void *id128, int rank, int nranks, double *host, int n, int ok) {
  if (!Comm::is_ipc_id(id128) || nranks < 1 || rank < 0 || rank >= nranks || n < 0)
    return fail("bad IPC id / rank / size");
  Comm cm;
  if (cm.init(rank, nranks, id128)) return fail("IPC slab group init failed (shared-memory id)");
  if (cm.agree_ok(ok != 0, nullptr)) return fail("a rank reported failure");
  if (cm.allreduce_sum(host, n, nullptr)) return fail("IPC allreduce failed");
  return 0;
}
const char *mnl_fields_transport(mnl_fields *f) {
  if (!f) return "";
  return f->comm ? f->comm->transport() : "single";
}
int mnl_comm_rccl_selftest(int device, int n) {
  if (n < 1) return fail("selftest needs n >= 1");
  if (hipSetDevice(device) != hipSuccess) return fail("hipSetDevice failed");
  const char *e = rccl_selftest(n);
  return e ? fail(e) : 0;
}

void mnl_fields_destroy(mnl_fields *f) { delete f; }

int mnl_fields_add_point_source(mnl_fields *F, int comp, int kind, const double *p, int np,
                                const double pos[3], double amp_re, double amp_im,
                                int is_integrated) {
  if (!pos) return fail("null position");
  return add_source_parts(F, comp, kind, p, np, nullptr, nullptr, pos, pos, amp_re, amp_im,
                        is_integrated, nullptr, nullptr);
}

int mnl_fields_add_volume_source(mnl_fields *F, int comp, int kind, const double *p, int np,
                                 const double vmin[3], const double vmax[3], double amp_re,
                                 double amp_im, int is_integrated, mnl_amp_func afunc,
                                 void *adata) {
  if (!vmin || !vmax) return fail("null volume");
  if (kind == MNL_SRC_CUSTOM) return fail("custom sources: use mnl_fields_add_custom_volume_source");
  return add_source_parts(F, comp, kind, p, np, nullptr, nullptr, vmin, vmax, amp_re, amp_im,
                        is_integrated, afunc, adata);
}

int mnl_fields_add_custom_volume_source(mnl_fields *F, int comp, mnl_src_func func, void *data,
                                        double start_time, double end_time, const double vmin[3],
                                        const double vmax[3], double amp_re, double amp_im,
                                        int is_integrated, mnl_amp_func afunc, void *adata) {
  if (!func) return fail("custom source needs a function");
  if (!vmin || !vmax) return fail("null volume");
  const double p[2] = {start_time, end_time};
  return add_source_parts(F, comp, MNL_SRC_CUSTOM, p, 2, func, data, vmin, vmax, amp_re, amp_im,
                        is_integrated, afunc, adata);
}

int mnl_fields_add_custom_point_source(mnl_fields *F, int comp, mnl_src_func func, void *data,
                                       double start_time, double end_time, const double pos[3],
                                       double amp_re, double amp_im, int is_integrated) {
  if (!func) return fail("custom source needs a function");
  const double p[2] = {start_time, end_time};
  if (!pos) return fail("null position");
  return add_source_parts(F, comp, MNL_SRC_CUSTOM, p, 2, func, data, pos, pos, amp_re, amp_im,
                        is_integrated, nullptr, nullptr);
}

int mnl_fields_require_component(mnl_fields *F, int comp) {
  if (!F || check_comp(comp)) return -1;
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (F->twin && require_component(F->twin.get(), comp)) return -1;
  return require_component(F, comp);
}

int mnl_fields_step(mnl_fields *F, int nsteps) {
  if (!F) return fail("null fields");
  if (nsteps <= 0) return 0;
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return fields_step(F, nsteps);
}

int mnl_fields_tune(mnl_fields *F, int reps, int *zchunk, int *gen_cus) {
  if (!F || reps < 1) return fail("bad argument");
  if (zchunk) *zchunk = -1;
  if (gen_cus) *gen_cus = -1;
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "tune")) return -1;
  return tune(F, reps, zchunk, gen_cus);
}

int mnl_fields_initialize_field(mnl_fields *F, int comp, const double *host, size_t n) {
  if (!F || check_comp(comp) || !host) return fail("bad argument");
  if (F->twin) return mnl_fields_initialize_field_complex(F, comp, host, nullptr, n);
  if (n < F->S.ntot) return fail("initialize_field: array smaller than the cell");
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  F->f.nr_t = F->t;  // its update_eh(E) solves at the current time step
  return initialize_field(F, comp, host);
}

int mnl_fields_energy_in_box(mnl_fields *F, int which, const double vmin[3], const double vmax[3],
                             double *out) {
  if (!F || !out || which < 0 || which > 2) return fail("bad argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  double lo[3], hi[3];
  const mnl_structure &S = F->S;
  for (int d = 0; d < 3; d++) {  // NULL: the whole cell (user_volume.surroundings())
    lo[d] = S.has[d] ? (vmin ? vmin[d] : S.io[d] * (0.5 / S.a)) : 0.0;
    hi[d] = S.has[d] ? (vmax ? vmax[d] : (S.io[d] + 2 * S.n[d]) * (0.5 / S.a)) : 0.0;
  }
  if (energy_in_box(F, which, lo, hi, out)) return -1;
  if (F->twin) {  // real(conj(E) D) = E0 D0 + E1 D1 (src/energy_and_flux.cpp:54-187): both parts
    double im = 0.0;
    if (energy_in_box(F->twin.get(), which, lo, hi, &im)) return -1;
    *out += im;
  }
  return 0;
}

int mnl_fields_set_nan_check(mnl_fields *F, int every) {
  if (!F || every < 1) return fail("NaN check cadence must be >= 1 step");
  F->nan_every = every;
  if (F->twin) F->twin->nan_every = every;
  return 0;
}

int mnl_fields_array_slice(mnl_fields *F, int comp, const double vmin[3], const double vmax[3],
                           int snap, int *rank, long long dims[3], double *out, long long nout) {
  if (!F || !vmin || !vmax || !rank || !dims) return fail("bad argument");
  if (comp != MNL_DIELECTRIC && comp != MNL_PERMEABILITY && check_comp(comp))
    return fail("bad argument");
  return array_slice(F, comp, vmin, vmax, snap, rank, dims, out, nout);
}

int mnl_fields_dump(mnl_fields *F, const char *filename) {
  if (!F || !filename) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "dump (checkpoints of complex fields are the follow-up)")) return -1;
  std::string p = filename;
  if (F->nranks > 1) p += ".rank" + std::to_string(F->rank);
  return fields_dump(F, p.c_str());
}

int mnl_fields_load(mnl_fields *F, const char *filename) {
  if (!F || !filename) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "load (checkpoints of complex fields are the follow-up)")) return -1;
  std::string p = filename;
  if (F->nranks > 1) p += ".rank" + std::to_string(F->rank);
  return fields_load(F, p.c_str());
}

int mnl_structure_dump(mnl_structure *s, const char *filename) {
  if (!s || !filename) return fail("null argument");
  return structure_dump(s, filename);
}

int mnl_structure_load(mnl_structure *s, const char *filename) {
  if (!s || !filename) return fail("null argument");
  return structure_load(s, filename);
}

int mnl_fields_time(mnl_fields *F, long long *t, double *dt) {
  if (!F) return fail("null fields");
  if (t) *t = F->t;
  if (dt) *dt = F->dt;
  return 0;
}

int mnl_fields_set_time(mnl_fields *F, long long t) {
  if (!F || t < 0) return fail("bad argument");
  F->t = t;
  if (F->twin) F->twin->t = t;
  probe_restart(F);
  ldos_restart(F);
  return 0;
}

int mnl_fields_zero_fields(mnl_fields *F) {
  // fields_chunk::zero_fields (src/fields.cpp:638-664): every field, f_u, f_w and f_cond
  // array to 0 and the polarizations re-initialised (P = P_prev = 0); the DFT
  // accumulators are kept.  Leaves fused mode first (its ping-pong partners are
  // rebuilt from the zeroed arrays when it is entered again).
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (F->twin && mnl_fields_zero_fields(F->twin.get())) return -1;
  if (F->fused && set_fused(F, false)) return -1;
  for (const CkEntry &e : ckpt_entries(F))
    if (e.kind != 11) HIPCHK(hipMemsetAsync(e.p, 0, e.n * sizeof(double), F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

int mnl_fields_remove_sources(mnl_fields *F) {
  // fields::remove_sources (src/fields.cpp:601-610): every source and its src_time
  if (!F) return fail("null fields");
  F->groups.clear();
  F->srcs.clear();
  F->src_dirty = true;
  if (F->twin) return mnl_fields_remove_sources(F->twin.get());
  return 0;
}

int mnl_fields_get_field(mnl_fields *F, int comp, const double pos[3], double *out) {
  if (!F || check_comp(comp)) return -1;
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return get_field(F, comp, pos, out, true);
}

size_t mnl_fields_ntot(mnl_fields *F) { return F ? F->S.ntot : 0; }

int mnl_fields_copy_component(mnl_fields *F, int comp, double *host, size_t n) {
  if (!F || check_comp(comp)) return -1;
  if (n < F->S.ntot) return fail("output buffer too small");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  memset(host, 0, F->S.ntot * sizeof(double));
  if (!has_field(F->S, comp) || !F->allocated[comp]) return 0;
  int t = ctype(comp), d = cdir(comp);
  const double *src = nullptr, *hsep = nullptr;
  switch (t) {
    case T_E: src = F->f.E[d]; break;
    case T_D: src = F->f.D[d]; break;
    case T_B: src = F->f.B[d]; break;
    case T_H:
      src = F->f.B[d];
      hsep = (F->hall && !F->h_first_done) ? nullptr : F->f.H[d];
      break;
  }
  if (!src) return 0;
  size_t nt = F->S.ntot;
  if (F->scratch_cap < nt) {
    if (F->d_scratch) hipFree(F->d_scratch);
    HIPCHK(hipMalloc(&F->d_scratch, nt * sizeof(double)));
    F->scratch_cap = nt;
  }
  HIPCHK(hipMemsetAsync(F->d_scratch, 0, nt * sizeof(double), F->stream));
  if (wrap_for_readers(F)) return -1;  // periodic: the not-owned planes read as their owners
  const bool fe = F->fused && t == T_E;
  if (k_to_canonical(F->d_scratch, src, hsep, F->g, t, d, F->f, fe ? &F->fusedG : nullptr,
                     fe ? F->f.D[d] : nullptr, fe ? F->f.inveps[d] : nullptr, F->stream))
    return fail("to_canonical launch failed");
  HIPCHK(hipMemcpyAsync(host, F->d_scratch, nt * sizeof(double), hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

int mnl_fields_time_spent(mnl_fields *F, double *out) {
  if (!F || !out) return fail("bad argument");
  for (int k = 0; k < MNL_NUM_TIME_SINKS; k++) out[k] = F->sink_s[k];
  return 0;
}

int mnl_fields_reset_timers(mnl_fields *F) {
  if (!F) return fail("null fields");
  for (int k = 0; k < MNL_NUM_TIME_SINKS; k++) F->sink_s[k] = 0;
  return 0;
}

int mnl_fields_allreduce(mnl_fields *F, double *v, int n) {
  if (!F || (n > 0 && !v) || n < 0) return fail("bad argument");
  if (F->nranks == 1 || n == 0) return 0;
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return timed_allreduce(F, v, n) ? fail("allreduce failed") : 0;
}

void mnl_set_verbosity(int level) { g_verbosity = level; }
int mnl_get_verbosity(void) { return g_verbosity; }

int mnl_fields_timers(mnl_fields *F, double out[6]) {
  if (!F) return fail("null fields");
  out[0] = F->timer_ms[TM_B] + F->timer_ms[TM_BINT];
  out[1] = F->timer_ms[TM_H];
  out[2] = F->timer_ms[TM_D] + F->timer_ms[TM_DINT];
  out[3] = F->timer_ms[TM_E];
  out[4] = F->timer_ms[TM_SRC];
  out[5] = F->timer_ms[TM_HALO];
  return 0;
}

int mnl_fields_nr_fallbacks(mnl_fields *F, long long *count) {
  if (!F) return fail("null fields");
  unsigned long long v = 0;
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  HIPCHK(hipMemcpy(&v, F->d_nr_fallbacks, sizeof(v), hipMemcpyDeviceToHost));
  *count = (long long)v;
  return 0;
}

int mnl_fields_use_complex_fields(mnl_fields *F) {
  // the inverse of fields::use_real_fields (src/fields.cpp:140-160): a second set of every
  // time-stepped array -- here a second fields object of the same structure (mnl_fields::twin)
  if (!F) return fail("null fields");
  if (F->twin) return 0;
  if (F->part0) return fail("use_complex_fields: bad fields object");
  if (F->S.dim == 1) return fail("use_complex_fields: 1-D cells are not supported");
  bool chi = false, offd = false, aniso = false;
  for (int c = 0; c < 3; c++) {
    chi = chi || !all_eq(F->S.chi2[c], 0.0) || !all_eq(F->S.chi3[c], 0.0);
    for (int d = 0; d < 3; d++) offd = offd || (d != c && !all_eq(F->S.chi1inv[c][d], 0.0));
  }
  for (const BoxSpec &b : F->S.boxes) chi = chi || (b.kind == 1 && b.value != 0.0);
  for (const Lorentz &L : F->S.lor) aniso = aniso || L.aniso();
  if (chi || F->nr || F->upnl)
    return fail("use_complex_fields: chi(2) / chi(3) media are not supported on complex fields "
                "(the Newton-Raphson solve on two parts is not built)");
  if (offd || aniso || F->f.aniso)
    return fail("use_complex_fields: off-diagonal chi1inv and anisotropic susceptibilities are "
                "not supported on complex fields");
  if (F->t != 0 || F->e_first_done || F->h_first_done || F->u_first_done[0] || F->u_first_done[1])
    return fail("use_complex_fields: only before the first step");
  if (!F->groups.empty() || !F->sampled.empty())
    return fail("use_complex_fields: only before sources and DFT monitors are added");
  if (any_periodic(F)) return fail("use_complex_fields: only before use_bloch");
  for (int c = 0; c < MNL_NUM_COMPONENTS; c++)
    if (F->allocated[c])
      return fail("use_complex_fields: only before initialize_field and before any component is "
                  "required");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (F->fused && set_fused(F, false)) return -1;
  // several ranks (every rank makes this call): part 1 takes the same slab and shares part 0's
  // communicator, so exchange lists both sets in one group
  std::unique_ptr<mnl_fields> T(
      create_common(&F->S, F->device, F->rank, F->nranks, nullptr, nullptr, F->comm));
  if (!T) return -1;
  // part 1 runs on part 0's stream: one sub-step of both parts is then in order before the
  // wrap that follows it
  HIPCHK(hipStreamSynchronize(T->stream));
  HIPCHK(hipStreamDestroy(T->stream));
  T->stream = F->stream;
  T->part0 = F;
  T->allow_fused = F->allow_fused;
  T->nan_every = F->nan_every;
  T->tb_enabled = false;
  F->twin = std::move(T);
  return 0;
}

int mnl_fields_is_real(mnl_fields *F, int *out) {
  if (!F || !out) return fail("null argument");
  *out = is_complex(F) ? 0 : 1;
  return 0;
}

int mnl_fields_get_field_complex(mnl_fields *F, int comp, const double pos[3], double out[2]) {
  // fields::get_field (src/monitor.cpp:115-160) without the real()
  if (!F || !pos || !out || check_comp(comp)) return -1;
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  out[1] = 0.0;
  if (get_field(F, comp, pos, &out[0], true)) return -1;
  return F->twin ? get_field(F->twin.get(), comp, pos, &out[1], true) : 0;
}

int mnl_fields_copy_component_part(mnl_fields *F, int part, int comp, double *host, size_t n) {
  if (!F || part < 0 || part > 1) return fail("bad argument");
  if (part == 1 && !F->twin) return fail("copy_component: real fields have no imaginary part");
  return mnl_fields_copy_component(part ? F->twin.get() : F, comp, host, n);
}

int mnl_fields_array_slice_part(mnl_fields *F, int part, int comp, const double vmin[3],
                                const double vmax[3], int snap, int *rank, long long dims[3],
                                double *out, long long nout) {
  if (!F || part < 0 || part > 1) return fail("bad argument");
  if (part == 1 && !F->twin) return fail("array_slice: real fields have no imaginary part");
  return mnl_fields_array_slice(part ? F->twin.get() : F, comp, vmin, vmax, snap, rank, dims, out,
                                nout);
}

int mnl_fields_initialize_field_complex(mnl_fields *F, int comp, const double *re,
                                        const double *im, size_t n) {
  // fields::initialize_field adds real(val) to part 0 and imag(val) to part 1
  // (src/initialize.cpp:155-160); im == NULL: 0.  Both parts take every step of the call (the
  // lazy copies, update_eh, the ghost planes), so that they stay in the same state.
  if (!F || check_comp(comp) || !re) return fail("bad argument");
  if (!F->twin) return fail("initialize_field_complex: the fields are real");
  if (n < F->S.ntot) return fail("initialize_field: array smaller than the cell");
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  mnl_fields *T = F->twin.get();
  if (require_component(F, comp) || require_component(T, comp)) return -1;
  for (mnl_fields *p : {F, T})
    if (p->fused && set_fused(p, false)) return -1;
  std::vector<double> zero;
  if (!im) zero.assign(F->S.ntot, 0.0), im = zero.data();
  F->f.nr_t = T->f.nr_t = F->t;
  if (initialize_field(F, comp, re) || initialize_field(T, comp, im)) return -1;
  return 0;
}

int mnl_fields_use_bloch(mnl_fields *F, int dir, double k_re, double k_im) {
  // fields::use_bloch (src/boundaries.cpp:88-103); real fields: k = 0 only
  if (!F) return fail("null fields");
  if (dir < 0 || dir > 2) return fail("use_bloch: direction must be 0 (X), 1 (Y) or 2 (Z)");
  if ((k_re != 0.0 || k_im != 0.0) && !F->twin)
    return fail("use_bloch: k != 0 needs complex fields (mnl_fields_use_complex_fields before "
                "use_bloch); real fields take only k = 0");
  if (F->S.dim == 1) return fail("use_bloch: periodic boundaries of 1-D cells are not supported");
  if (!F->S.has[dir]) return fail("use_bloch: the cell has no such direction");
  if (F->S.pml_thick[dir][0] > 0 || F->S.pml_thick[dir][1] > 0)
    return fail("use_bloch: a PML along a periodic direction is not supported");
  if (F->nranks > 1 && dir == F->slab_dir)
    return fail("use_bloch: the slab direction of fields on more than one rank cannot be "
                "periodic");
  if (F->periodic[dir] && !F->twin) return 0;
  {
    // The E / P kernels that read wall-plane neighbours of another reference chunk as 0
    // (on_wall: anisotropic sigma, and Newton-Raphson or upstream off-diagonal chi1inv with a
    // susceptibility) take plane n of a direction for a wall.  Such a neighbour exists only
    // where two other directions are split into PML chunks.
    int npml = 0;
    for (int d = 0; d < 3; d++) npml += F->S.has[d] && F->pml_any[d];
    if (npml >= 2 && (F->f.aniso || F->f.wall_e))
      return fail("use_bloch: anisotropic susceptibilities, and Newton-Raphson or off-diagonal "
                  "chi1inv with a susceptibility, are not supported in a periodic cell with PML "
                  "along two directions");
  }
  if (F->t != 0 || F->e_first_done || F->h_first_done || F->u_first_done[0] || F->u_first_done[1])
    return fail("use_bloch: only before the first step");
  if (!F->groups.empty() || !F->sampled.empty())
    return fail("use_bloch: only before sources and DFT monitors are added");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (F->fused && set_fused(F, false)) return -1;
  if (mnl_fields *T = F->twin.get()) {
    if (T->fused && set_fused(T, false)) return -1;
    F->eikna[dir] = bloch_eikna(cplx(k_re, k_im), F->S.n[dir], F->S.a);
    F->bloch_k[dir] = cplx(k_re, k_im);
    if (F->periodic[dir]) return 0;  // k set again
    if (set_periodic(T, dir)) return -1;
  }
  return set_periodic(F, dir);
}

int mnl_fields_boundary(mnl_fields *F, int dir, int side, int *kind) {
  if (!F || !kind || dir < 0 || dir > 2 || side < 0 || side > 1) return fail("bad argument");
  if (!F->S.has[dir]) return fail("boundary: the cell has no such direction");
  *kind = F->periodic[dir] ? MNL_BOUNDARY_PERIODIC : MNL_BOUNDARY_METALLIC;
  return 0;
}

int mnl_fields_set_fused(mnl_fields *F, int allow) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  F->allow_fused = allow != 0;
  if (F->twin && mnl_fields_set_fused(F->twin.get(), allow)) return -1;
  if (!F->allow_fused) return set_fused(F, false);
  return 0;
}

int mnl_fields_set_profiling(mnl_fields *F, int on) {
  if (!F) return fail("null fields");
  F->profiling = on != 0;  // (complex fields: part 0's timers time the launches of both parts)
  for (int k = 0; k < TM_CAP; k++) F->timer_ms[k] = 0, F->timer_count[k] = 0;
  return 0;
}

int mnl_fields_kernel_stats(mnl_fields *F, int which, long long *launches, double *total_ms,
                            double *bytes_per_launch) {
  if (!F) return fail("bad kernel id");
  return kernel_stats(F, which, launches, total_ms, bytes_per_launch);
}

int mnl_fields_set_temporal_blocking(mnl_fields *F, int on) {
  if (!F) return fail("null fields");
  F->tb_enabled = on != 0;  // (complex fields never step in pairs: part 1 keeps it off)
  return 0;
}

int mnl_fields_set_schedule(mnl_fields *F, int which, int value) {
  if (!F) return fail("null fields");
  if (F->twin && mnl_fields_set_schedule(F->twin.get(), which, value)) return -1;  // both parts
  for (const SchedOpt &o : SCHED_OPTS) {
    if (o.id != which) continue;
    if (o.count && value != 0 && (value < o.lo || value > o.hi)) return fail(o.err);
    if (o.count)
      F->*o.count = value;
    else
      F->*o.flag = value != 0;
    if (which == MNL_SCHED_DFT_PAL)  // the sampling plans are rebuilt at the next update
      for (DftFluxH *d : F->sampled) d->plan_key = -1;
    if (which == MNL_SCHED_TB_OX) F->tb_ox_set = value != 0;  // the tuner keeps a set width
    if (o.replan) F->tb_sig = 0;  // the pair plan is rebuilt at the next batch
    return 0;
  }
  return fail("bad schedule option");
}

int mnl_fields_tb_info(mnl_fields *F, double *out, int n) {
  if (!F || !out || n < 1) return fail("bad argument");
  double v[MNL_NUM_TBINFO];
  tb_info(F, v);
  for (int i = 0; i < n && i < MNL_NUM_TBINFO; i++) out[i] = v[i];
  return 0;
}

int mnl_fields_mode(mnl_fields *F, int *fused) {
  if (!F) return fail("null fields");
  *fused = fields_mode(F);
  return 0;
}

int mnl_fields_add_dft_fields(mnl_fields *F, int ncomp, const int *comps, const double vmin[3],
                              const double vmax[3], const double *freqs, int nfreq, int yee_grid,
                              int decimation, int *handle) {
  if (!F || !comps || !vmin || !vmax || !freqs || !handle) return fail("null argument");
  if (decimation < 0) return fail("decimation must be >= 0");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  const int h = dft_add_fields(F, ncomp, comps, vmin, vmax, freqs, nfreq, yee_grid, decimation);
  if (h < 0) return -1;
  // complex fields: part 1 gets the same object (the same handle), which samples its rows
  if (F->twin && dft_add_fields(F->twin.get(), ncomp, comps, vmin, vmax, freqs, nfreq, yee_grid,
                                decimation) != h)
    return fail("add_dft_fields: the parts of the complex fields differ");
  *handle = h;
  return 0;
}

int mnl_fields_dft_array(mnl_fields *F, int h, int comp, int num_freq, int *rank, long long dims[3],
                         double *out, long long nout) {
  if (!F || !rank || !dims) return fail("null argument");
  return dft_array(F, h, comp, num_freq, rank, dims, out, nout);
}

int mnl_fields_add_dft_flux(mnl_fields *F, int nreg, const double *regions, const double *freqs,
                            int nfreq, int decimation, int *handle) {
  if (!F || !regions || !freqs || !handle) return fail("null argument");
  if (decimation < 0) return fail("decimation must be >= 0");
  for (int r = 0; r < nreg; r++)
    if (regions[8 * r + 6] < 0 || regions[8 * r + 6] > 2) return fail("bad flux direction");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  const int h = dft_add_flux(F, nreg, regions, freqs, nfreq, decimation);
  if (h < 0) return -1;
  if (F->twin && dft_add_flux(F->twin.get(), nreg, regions, freqs, nfreq, decimation) != h)
    return fail("add_dft_flux: the parts of the complex fields differ");
  *handle = h;
  return 0;
}

int mnl_fields_dft_flux(mnl_fields *F, int h, double *out) {
  if (!F || !out) return fail("null argument");
  return dft_flux_values(F, h, out);
}

int mnl_fields_dft_size(mnl_fields *F, int h, long long *n) {
  if (!F || !n) return fail("null argument");
  if (dft_bad_handle(F, h)) return -1;
  const DftFluxH &o = *F->dfts[h];
  long long k = 0;
  for (auto &dc : o.E) k += (long long)dc.N;
  *n = k * o.nfreq;
  return 0;
}

int mnl_fields_dft_flush(mnl_fields *F) {
  if (!F) return fail("null fields");
  for (auto &o : F->dfts)
    if (dft_flush(F, *o)) return -1;
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

int mnl_fields_dft_data(mnl_fields *F, int h, int which, double *out, long long n) {
  if (!F || !out) return fail("null argument");
  if (dft_bad_handle(F, h)) return -1;
  if (dft_flush(F, *F->dfts[h])) return -1;  // the buffered updates first
  const DftFluxH &o = *F->dfts[h];
  const size_t nf = o.nfreq;
  std::vector<double> v(2 * ((o.npts + 63) & ~size_t(63)) * nf);
  if (!v.empty()) {
    HIPCHK(hipStreamSynchronize(F->stream));
    HIPCHK(hipMemcpy(v.data(), o.d_dft, v.size() * 8, hipMemcpyDeviceToHost));
  }
  long long k = 0;
  if (dft_bad_which(o, which)) return fail("dft_data: no such list");
  for (auto &dc : o.L[which])
    for (size_t p = 0; p < dc.N; p++)
      for (size_t i = 0; i < nf; i++) {
        if (k + 2 > 2 * n) return fail("dft buffer too small");
        out[k++] = v[2 * dft_at(o.slot[dc.p0 + p], i, nf)];
        out[k++] = v[2 * dft_at(o.slot[dc.p0 + p], i, nf) + 1];
      }
  return 0;
}

int mnl_fields_dft_get(mnl_fields *F, int h, int which, double *out, long long n) {
  if (!F || !out) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_get(F, h, which, out, n);
}

int mnl_fields_dft_load(mnl_fields *F, int h, int which, const double *in, long long n, int sign) {
  if (!F || (n > 0 && !in)) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_load(F, h, which, in, n, sign);
}

int mnl_fields_dft_scale(mnl_fields *F, int h, double re, double im) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_scale(F, h, re, im);
}

int mnl_fields_dft_save(mnl_fields *F, int h, const char *filename) {
  if (!F || !filename) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_save(F, h, filename);
}

int mnl_fields_dft_load_file(mnl_fields *F, int h, const char *filename, int sign) {
  if (!F || !filename) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_load_file(F, h, filename, sign);
}

int mnl_fields_add_probe(mnl_fields *F, int comp, const double pos[3], int *handle) {
  if (!F || !pos || !handle) return fail("null argument");
  if (check_comp(comp)) return -1;
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "add_probe")) return -1;
  const int h = probe_add(F, comp, pos);
  if (h < 0) return -1;
  *handle = h;
  return 0;
}

int mnl_fields_probe_read(mnl_fields *F, int h, long long cap, long long *count,
                          long long *t_first, double *values) {
  if (!F || !count || !t_first) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return probe_read(F, h, cap, count, t_first, values);
}

int mnl_fields_probe_reset(mnl_fields *F, int h) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return probe_reset(F, h);
}

int mnl_fields_remove_probe(mnl_fields *F, int h) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return probe_remove(F, h);
}

int mnl_fields_remove_probes(mnl_fields *F) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return probe_remove_all(F);
}

int mnl_fields_add_ldos(mnl_fields *F, const double *freqs, int nfreq, int *handle) {
  if (!F || !freqs || !handle) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "add_ldos")) return -1;
  const int h = ldos_add(F, freqs, nfreq);
  if (h < 0) return -1;
  *handle = h;
  return 0;
}

int mnl_fields_ldos_update(mnl_fields *F, int h) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return ldos_update(F, h);
}

int mnl_fields_ldos_record(mnl_fields *F, int h, int on) {
  if (!F) return fail("null fields");
  return ldos_record(F, h, on);
}

int mnl_fields_ldos_data(mnl_fields *F, int h, double *ldos, double *Fdft, double *Jdft,
                         double *overall_scale) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return ldos_data(F, h, ldos, Fdft, Jdft, overall_scale);
}

int mnl_fields_ldos_points(mnl_fields *F, int h, long long cap, long long *n, int *comp, int *ijk,
                           double *amp) {
  if (!F || !n) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return ldos_points(F, h, cap, n, comp, ijk, amp);
}

int mnl_fields_remove_ldos(mnl_fields *F, int h) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return ldos_remove(F, h);
}

int mnl_fields_mode_coefficients(mnl_fields *F, int h, int nmodes, const int *g, const double *axis,
                                 const double *sp, const double *eig_vol, const double *kpoint,
                                 double *coeffs, double *vgrp, double *kpoints, double *cscale,
                                 double *overlaps) {
  if (!F || !coeffs || (nmodes >= 1 && (!g || !sp))) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return mode_coefficients(F, ModeCall{h, nmodes, g, axis, sp, eig_vol, kpoint}, coeffs, vgrp,
                           kpoints, cscale, overlaps);
}

int mnl_fields_mode_table(mnl_fields *F, int h, int nmodes, const int *g, const double *axis,
                          const double *sp, const double *eig_vol, const double *kpoint,
                          long long *dims, int *coords, double *k, double *vgrp, double *amp,
                          double *pa, double *pb, double *pl) {
  if (!F || !dims || (nmodes >= 1 && (!g || !sp))) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return mode_table(F, ModeCall{h, nmodes, g, axis, sp, eig_vol, kpoint}, dims, coords, k, vgrp,
                    amp, pa, pb, pl);
}

int mnl_fields_remove_ldoses(mnl_fields *F) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return ldos_remove_all(F);
}

int mnl_fields_dft_norm(mnl_fields *F, double *norm) {
  if (!F || !norm) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "dft_norm")) return -1;
  return dft_norm(F, norm);
}

int mnl_fields_dft_maxfreq(mnl_fields *F, double *maxfreq) {
  if (!F || !maxfreq) return fail("null argument");
  *maxfreq = dft_maxfreq(F);
  return 0;
}

int mnl_fields_max_decimation(mnl_fields *F, int *decimation) {
  if (!F || !decimation) return fail("null argument");
  *decimation = dft_max_decimation(F);
  return 0;
}

int mnl_fields_dft_decimation(mnl_fields *F, int h, int *decimation) {
  if (!F || !decimation) return fail("null argument");
  if (dft_bad_handle(F, h)) return -1;
  *decimation = F->dfts[h]->decim;
  return 0;
}

int mnl_fields_add_dft_near2far(mnl_fields *F, int nreg, const double *regions, const double *freqs,
                                int nfreq, int decimation, int nperiods, int *handle) {
  if (!F || !regions || !freqs || !handle) return fail("null argument");
  if (decimation < 0) return fail("decimation must be >= 0");
  for (int r = 0; r < nreg; r++)
    if (regions[8 * r + 6] < 0 || regions[8 * r + 6] > 2)
      return fail("invalid normal direction in dft_near2far!");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "add_dft_near2far")) return -1;
  const int h = dft_add_near2far(F, nreg, regions, freqs, nfreq, decimation, nperiods);
  if (h < 0) return -1;
  *handle = h;
  return 0;
}

int mnl_fields_near2far_farfields(mnl_fields *F, int h, long long npts, const double *xyz,
                                  double *out) {
  if (!F || (npts > 0 && (!xyz || !out))) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return n2f_farfields(F, h, npts, xyz, out);
}

int mnl_fields_near2far_medium(mnl_fields *F, int h, double *eps, double *mu) {
  if (!F || !eps || !mu) return fail("null argument");
  if (dft_bad_handle(F, h)) return -1;
  if (!F->dfts[h]->n2f) return fail("near2far_medium: the handle is not a near2far object");
  *eps = F->dfts[h]->eps;
  *mu = F->dfts[h]->mu;
  return 0;
}

int mnl_fields_near2far_points(mnl_fields *F, int h, double *out, long long npoints) {
  if (!F || !out) return fail("null argument");
  return n2f_points(F, h, out, npoints);
}

int mnl_fields_add_dft_energy(mnl_fields *F, int nreg, const double *regions, const double *freqs,
                              int nfreq, int decimation, int *handle) {
  if (!F || !regions || !freqs || !handle) return fail("null argument");
  if (decimation < 0) return fail("decimation must be >= 0");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "add_dft_energy")) return -1;
  const int h = dft_add_energy(F, nreg, regions, freqs, nfreq, decimation);
  if (h < 0) return -1;
  *handle = h;
  return 0;
}

int mnl_fields_add_dft_force(mnl_fields *F, int nreg, const double *regions, const double *freqs,
                             int nfreq, int decimation, int *handle) {
  if (!F || !regions || !freqs || !handle) return fail("null argument");
  if (decimation < 0) return fail("decimation must be >= 0");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  if (refuse_complex(F, "add_dft_force")) return -1;
  const int h = dft_add_force(F, nreg, regions, freqs, nfreq, decimation);
  if (h < 0) return -1;
  *handle = h;
  return 0;
}

int mnl_fields_dft_energy(mnl_fields *F, int h, int which, double *out) {
  if (!F || !out) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_energy_values(F, h, which, out);
}

int mnl_fields_dft_force(mnl_fields *F, int h, double *out) {
  if (!F || !out) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  return dft_force_values(F, h, out);
}

int mnl_fields_dft_points(mnl_fields *F, int h, int which, double *out, long long n) {
  if (!F || (n > 0 && !out)) return fail("null argument");
  return dft_points(F, h, which, out, n);
}

int mnl_fields_dft_list_size(mnl_fields *F, int h, int which, long long *n) {
  if (!F || !n) return fail("null argument");
  if (dft_bad_handle(F, h)) return -1;
  const DftFluxH &o = *F->dfts[h];
  if (dft_bad_which(o, which)) return fail("dft_list_size: no such list");
  *n = (long long)dft_list_points(o, which) * o.nfreq;
  return 0;
}

int mnl_fields_traffic_model(mnl_fields *F, double *bpc, double *cells) {
  if (!F) return fail("null fields");
  traffic_model(F, bpc, cells);
  return 0;
}

}  // extern "C"
