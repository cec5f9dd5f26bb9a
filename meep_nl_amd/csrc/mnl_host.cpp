// mnl_host.cpp -- the C-ABI (include/meep_nl_amd.h) of the MI355X fields::step() path, with the
// structure description, quadrature, kernel statistics and traffic model that only it needs.
// The host side is built with g++ (not hipcc) on purpose: the per-step source amplitudes use
// std::complex / libm exactly as the reference does (src/sources.cpp:72-160,
// src/step.cpp:296-319), so the values handed to the GPU are bit-identical to the reference's.
// Its other files: mnl_setup.cpp (PML tables, grid, allocation, materials), mnl_sources.cpp
// (sources, get_field), mnl_fused.cpp (fused-tile planning), mnl_tb.cpp (pairs of steps),
// mnl_step.cpp (the step loop, NaN guard), mnl_tune.cpp (the tuner), mnl_dft.cpp, mnl_io.cpp.
#include "mnl_host.hpp"

namespace mnlh {
thread_local std::string g_err;
int g_verbosity = 1;

static mnl_fields *create_common(mnl_structure *s, int device, int rank, int nranks, const void *id,
                          LocalHub *hub = nullptr) {
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
  if (nranks > 1) {
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

}  // namespace

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

// ------------------------------------------------------------------ subpixel averaging
// Quadrature points and weights on the unit sphere for 1-D / 2-D / 3-D, the table
// the reference generates at build time (src/sphere-quad.cpp -> sphere-quad.h):
// 1-D {0,0,+-1}, 2-D 12 points on the circle, 3-D the 50-point degree-11 formula
// (McLaren; Stroud U3:11-1) with octahedral symmetry, each list reordered to
// maximise every point's distance from the earlier ones (squared distances
// compared in single precision, as the generator does).
namespace {
void sq_sort(int n, double *x, double *y, double *z, double *w) {
  for (int i = 1; i < n; ++i) {
    double best = 0, bestsum = 0;
    int jb = i;
    for (int j = i; j < n; ++j) {
      double mn = 1e20, sum = 0;
      for (int k = 0; k < i; ++k) {
        const double dx = x[k] - x[j], dy = y[k] - y[j], dz = z[k] - z[j];
        const double d2 = float(dx * dx + dy * dy + dz * dz);
        mn = mn < d2 ? mn : d2;
        sum += d2;
      }
      if (mn > best || (mn == best && sum > bestsum)) best = mn, bestsum = sum, jb = j;
    }
    std::swap(x[i], x[jb]);
    std::swap(y[i], y[jb]);
    std::swap(z[i], z[jb]);
    std::swap(w[i], w[jb]);
  }
}
// rotate (a, b, c) -> (c, a, b)
inline void rot3(double &a, double &b, double &c) {
  const double t = c;
  c = b;
  b = a;
  a = t;
}
void sphere_quad50(double *x, double *y, double *z, double *w) {
  int n = 0;
  auto put = [&](double a, double b, double c, double wt) {
    x[n] = a, y[n] = b, z[n] = c, w[n++] = wt;
  };
  double a = 1, b = 0, c = 0;  // 6 axis points
  for (int i = 0; i < 2; ++i) {
    a = -a;
    for (int j = 0; j < 3; ++j) rot3(a, b, c), put(a, b, c, 9216 / 725760.0);
  }
  a = b = sqrt(0.5), c = 0;  // 12 edge midpoints
  for (int i = 0; i < 2; ++i) {
    a = -a;
    for (int j = 0; j < 2; ++j) {
      b = -b;
      for (int k = 0; k < 3; ++k) rot3(a, b, c), put(a, b, c, 16384 / 725760.0);
    }
  }
  a = b = c = sqrt(1.0 / 3.0);  // 8 cube corners
  for (int i = 0; i < 2; ++i) {
    a = -a;
    for (int j = 0; j < 2; ++j) {
      b = -b;
      for (int k = 0; k < 2; ++k) c = -c, put(a, b, c, 15309 / 725760.0);
    }
  }
  a = b = sqrt(1.0 / 11.0), c = 3 * a;  // 24 points (1, 1, 3) / sqrt(11)
  for (int i = 0; i < 2; ++i) {
    a = -a;
    for (int j = 0; j < 2; ++j) {
      b = -b;
      for (int k = 0; k < 2; ++k) {
        c = -c;
        for (int l = 0; l < 3; ++l) rot3(a, b, c), put(a, b, c, 14641 / 725760.0);
      }
    }
  }
}
}  // namespace

// q[dim-1][i] = {x, y, z, weight}, nq = {2, 12, 50}
static void sphere_quad_table(double q[3][AVG_MAXQ][4], int nq[3]) {
  memset(q, 0, sizeof(double) * 3 * AVG_MAXQ * 4);
  nq[0] = 2, nq[1] = 12, nq[2] = 50;
  q[0][0][2] = 1, q[0][0][3] = 0.5;
  q[0][1][2] = -1, q[0][1][3] = 0.5;
  double x[AVG_MAXQ], y[AVG_MAXQ], z[AVG_MAXQ], w[AVG_MAXQ];
  const double pi = 3.141592653589793238462643383279502884197;
  for (int i = 0; i < 12; ++i) {
    x[i] = cos(2 * i * pi / 12);
    y[i] = sin(2 * i * pi / 12);
    z[i] = 0.0;
    w[i] = 1.0 / 12;
  }
  sq_sort(12, x, y, z, w);
  for (int i = 0; i < 12; ++i) q[1][i][0] = x[i], q[1][i][1] = y[i], q[1][i][2] = z[i], q[1][i][3] = w[i];
  sphere_quad50(x, y, z, w);
  sq_sort(50, x, y, z, w);
  for (int i = 0; i < 50; ++i) q[2][i][0] = x[i], q[2][i][1] = y[i], q[2][i][2] = z[i], q[2][i][3] = w[i];
}

int mnl_sphere_quadrature(int dim, double *xyzw) {
  if (dim < 1 || dim > 3) return fail("sphere quadrature: dim must be 1, 2 or 3");
  double q[3][AVG_MAXQ][4];
  int nq[3];
  sphere_quad_table(q, nq);
  if (xyzw) memcpy(xyzw, q[dim - 1], sizeof(double) * 4 * nq[dim - 1]);
  return nq[dim - 1];
}

// structure::set_epsilon(material_function &, use_anisotropic_averaging, tol, maxeval)
// (src/structure.cpp:397-401 -> structure_chunk::set_chi1inv, src/anisotropic_averaging.cpp:
// 221-298) for a material function made of geometric objects, evaluated on a GPU.  The
// per-point values do not depend on the chunking, so the whole cell is computed once;
// which rows each reference chunk keeps (its trivial test) is decided per chunk when the
// fields are created, as for arrays set with mnl_structure_set_chi1inv.
int mnl_structure_set_epsilon_geometry(mnl_structure *s, int device, int nobj, const double *objs,
                                       double default_eps, int use_averaging, double tol,
                                       int maxeval) {
  if (!s || nobj < 0 || (nobj > 0 && !objs)) return fail("set_epsilon_geometry: bad arguments");
  std::vector<GeoObj> h(nobj);
  for (int o = 0; o < nobj; o++) {
    const double *r = objs + MNL_GEO_STRIDE * o;
    GeoObj &g = h[o];
    g.kind = (int)r[0];
    if (g.kind < 0 || g.kind > 2 || r[0] != g.kind) return fail("set_epsilon_geometry: bad object kind");
    g.eps = r[1];
    for (int d = 0; d < 3; d++) g.c[d] = r[2 + d], g.p[d] = r[5 + d];
    if (g.kind == 2 && !(g.p[2] == 0 || g.p[2] == 1 || g.p[2] == 2))
      return fail("set_epsilon_geometry: cylinder axis must be 0, 1 or 2");
  }
  int prev_dev = -1;
  HIPCHK(hipGetDevice(&prev_dev));
  if (device >= 0) HIPCHK(hipSetDevice(device));
  struct RestoreDev {  // leave the caller's current device as it was
    int d;
    ~RestoreDev() {
      if (d >= 0) (void)hipSetDevice(d);
    }
  } restore{prev_dev};
  double q[3][AVG_MAXQ][4];
  AvgArgs A{};
  sphere_quad_table(q, A.nq);
  A.ndir = 0;
  for (int d = 0; d < 3; d++) {
    A.has[d] = s->has[d];
    A.n[d] = s->n[d];
    A.io[d] = s->io[d];
    if (s->has[d]) A.dirs[A.ndir++] = d;
  }
  A.inva = 1.0 / s->a;
  A.default_eps = default_eps;
  A.nobj = nobj;
  A.maxeval = use_averaging ? maxeval : 0;  // set_chi1inv: !use_anisotropic_averaging -> 0
  A.tol = tol;
  A.ntot = (long long)s->ntot;
  // E components with a field and the rows the chunk allocates (FOR_FT_COMPONENTS with
  // has_field): 1-D Ex only, with its x row; 2-D and 3-D Ex, Ey, Ez with all three
  const int ncomp = s->dim == 1 ? 1 : 3;
  GeoObj *dobj = nullptr;
  double *dq = nullptr, *dout = nullptr;
  auto cleanup = [&]() {
    if (dobj) hipFree(dobj);
    if (dq) hipFree(dq);
    if (dout) hipFree(dout);
  };
  auto chk = [&](hipError_t e, const char *what) {
    if (e == hipSuccess) return 0;
    cleanup();
    return fail(std::string("set_epsilon_geometry: ") + what + ": " + hipGetErrorString(e));
  };
  if (nobj > 0) {
    if (chk(hipMalloc(&dobj, sizeof(GeoObj) * nobj), "hipMalloc")) return -1;
    if (chk(hipMemcpy(dobj, h.data(), sizeof(GeoObj) * nobj, hipMemcpyHostToDevice), "copy")) return -1;
  }
  if (chk(hipMalloc(&dq, sizeof(q)), "hipMalloc")) return -1;
  if (chk(hipMemcpy(dq, q, sizeof(q), hipMemcpyHostToDevice), "copy")) return -1;
  const int nrow = s->dim == 1 ? 1 : 3;
  if (chk(hipMalloc(&dout, sizeof(double) * s->ntot * nrow), "hipMalloc")) return -1;
  A.objs = dobj;
  A.quad = dq;
  for (int c = 0; c < ncomp; c++) {
    A.c = c;
    for (int d = 0; d < 3; d++) A.out[d] = nullptr;
    for (int d = 0; d < nrow; d++) A.out[d] = dout + s->ntot * d;
    if (k_avg_chi1inv(A, nullptr)) {
      cleanup();
      return fail("set_epsilon_geometry: kernel launch failed");
    }
    if (chk(hipDeviceSynchronize(), "kernel")) return -1;
    for (int d = 0; d < nrow; d++) {
      auto &dst = s->chi1inv[c][d];
      dst.resize(s->ntot);
      if (chk(hipMemcpy(dst.data(), A.out[d], sizeof(double) * s->ntot, hipMemcpyDeviceToHost),
              "copy back"))
        return -1;
    }
    // the reference deletes trivial off-diagonal rows, and the diagonal when the whole
    // tensor is trivial (src/anisotropic_averaging.cpp:282-296); done here over the whole
    // cell, per chunk at field creation
    bool triv[3];
    for (int d = 0; d < nrow; d++) {
      const double tv = d == c ? 1.0 : 0.0;
      const auto &v = s->chi1inv[c][d];
      triv[d] = std::all_of(v.begin(), v.end(), [&](double x) { return x == tv; });
    }
    for (int d = nrow; d < 3; d++) triv[d] = true;
    for (int d = 0; d < nrow; d++)
      if (d != c && triv[d]) std::vector<double>().swap(s->chi1inv[c][d]);
    if (triv[0] && triv[1] && triv[2] && c < nrow) std::vector<double>().swap(s->chi1inv[c][c]);
  }
  cleanup();
  return 0;
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
  char id[128];
  if (Comm::unique_id(id)) return fail("ncclGetUniqueId failed");
  Comm cm;
  if (cm.init(0, 1, id)) return fail("RCCL communicator init failed");
  hipStream_t s;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return fail("stream");
  std::vector<double> h(n), back(n);
  for (int i = 0; i < n; i++) h[i] = 0.5 * i - 3.25;
  double *a = nullptr, *b = nullptr;
  int rc = 0;
  if (hipMalloc(&a, n * sizeof(double)) != hipSuccess ||
      hipMalloc(&b, n * sizeof(double)) != hipSuccess)
    rc = fail("hipMalloc failed");
  if (!rc && hipMemcpy(a, h.data(), n * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
    rc = fail("upload failed");
  if (!rc && (cm.group_start() || cm.send(a, n, 0, s) || cm.recv(b, n, 0, s) || cm.group_end(s)))
    rc = fail("grouped send/recv failed");
  if (!rc && (hipStreamSynchronize(s) != hipSuccess ||
              hipMemcpy(back.data(), b, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess))
    rc = fail("download failed");
  if (!rc && memcmp(back.data(), h.data(), n * sizeof(double)) != 0)
    rc = fail("send/recv data mismatch");
  std::vector<double> red(h);
  if (!rc && cm.allreduce_sum(red.data(), n, s)) rc = fail("allreduce failed");
  if (!rc && memcmp(red.data(), h.data(), n * sizeof(double)) != 0)
    rc = fail("allreduce data mismatch");
  if (a) (void)hipFree(a);
  if (b) (void)hipFree(b);
  (void)hipStreamDestroy(s);
  return rc;
}

void mnl_fields_destroy(mnl_fields *f) { delete f; }

int mnl_fields_add_point_source(mnl_fields *F, int comp, int kind, const double *p, int np,
                                const double pos[3], double amp_re, double amp_im,
                                int is_integrated) {
  if (!pos) return fail("null position");
  return add_source_any(F, comp, kind, p, np, nullptr, nullptr, pos, pos, amp_re, amp_im,
                        is_integrated, nullptr, nullptr);
}

int mnl_fields_add_volume_source(mnl_fields *F, int comp, int kind, const double *p, int np,
                                 const double vmin[3], const double vmax[3], double amp_re,
                                 double amp_im, int is_integrated, mnl_amp_func afunc,
                                 void *adata) {
  if (!vmin || !vmax) return fail("null volume");
  if (kind == MNL_SRC_CUSTOM) return fail("custom sources: use mnl_fields_add_custom_volume_source");
  return add_source_any(F, comp, kind, p, np, nullptr, nullptr, vmin, vmax, amp_re, amp_im,
                        is_integrated, afunc, adata);
}

int mnl_fields_add_custom_volume_source(mnl_fields *F, int comp, mnl_src_func func, void *data,
                                        double start_time, double end_time, const double vmin[3],
                                        const double vmax[3], double amp_re, double amp_im,
                                        int is_integrated, mnl_amp_func afunc, void *adata) {
  if (!func) return fail("custom source needs a function");
  if (!vmin || !vmax) return fail("null volume");
  const double p[2] = {start_time, end_time};
  return add_source_any(F, comp, MNL_SRC_CUSTOM, p, 2, func, data, vmin, vmax, amp_re, amp_im,
                        is_integrated, afunc, adata);
}

int mnl_fields_add_custom_point_source(mnl_fields *F, int comp, mnl_src_func func, void *data,
                                       double start_time, double end_time, const double pos[3],
                                       double amp_re, double amp_im, int is_integrated) {
  if (!func) return fail("custom source needs a function");
  const double p[2] = {start_time, end_time};
  if (!pos) return fail("null position");
  return add_source_any(F, comp, MNL_SRC_CUSTOM, p, 2, func, data, pos, pos, amp_re, amp_im,
                        is_integrated, nullptr, nullptr);
}

int mnl_fields_require_component(mnl_fields *F, int comp) {
  if (!F || check_comp(comp)) return -1;
  if (!has_field(F->S, comp)) return fail("component not present in this dimensionality");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
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
  return tune(F, reps, zchunk, gen_cus);
}

int mnl_fields_initialize_field(mnl_fields *F, int comp, const double *host, size_t n) {
  if (!F || check_comp(comp) || !host) return fail("bad argument");
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
  return energy_in_box(F, which, lo, hi, out);
}

int mnl_fields_set_nan_check(mnl_fields *F, int every) {
  if (!F || every < 1) return fail("NaN check cadence must be >= 1 step");
  F->nan_every = every;
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
  std::string p = filename;
  if (F->nranks > 1) p += ".rank" + std::to_string(F->rank);
  return fields_dump(F, p.c_str());
}

int mnl_fields_load(mnl_fields *F, const char *filename) {
  if (!F || !filename) return fail("null argument");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
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
  return 0;
}

int mnl_fields_zero_fields(mnl_fields *F) {
  // fields_chunk::zero_fields (src/fields.cpp:638-664): every field, f_u, f_w and f_cond
  // array to 0 and the polarizations re-initialised (P = P_prev = 0); the DFT
  // accumulators are kept.  Leaves fused mode first (its ping-pong partners are
  // rebuilt from the zeroed arrays when it is entered again).
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
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

int mnl_fields_set_fused(mnl_fields *F, int allow) {
  if (!F) return fail("null fields");
  if (hipSetDevice(F->device) != hipSuccess) return fail("hipSetDevice failed");
  F->allow_fused = allow != 0;
  if (!F->allow_fused) return set_fused(F, false);
  return 0;
}

int mnl_fields_set_profiling(mnl_fields *F, int on) {
  if (!F) return fail("null fields");
  F->profiling = on != 0;
  for (int k = 0; k < TM_CAP; k++) F->timer_ms[k] = 0, F->timer_count[k] = 0;
  return 0;
}

// Algorithmic HBM bytes of one fused step over G (DESIGN.md "Fused step"):
// every point reads B, D and writes B, D (96 B) + chi1inv (4 B palette word
// or 3 doubles); PML state is counted per (point, component) where the
// reference keeps it: f_u of B / D, separate H, W-form E (read + write 16 B).
// lean_bytes: the tile kernel's share, gen_bytes: the general kernel's (polarization chunks).
static void fused_bytes(const mnl_fields *F, double *lean_bytes, double *gen_bytes) {
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
  *lean_bytes = double(F->tile_cells) * 96.0 +
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
  *gen_bytes = double(F->gen_cells) * 96.0 +
               (guni ? F->gen_cells_nu : double(F->gen_cells)) * ub + extra;
}

int mnl_fields_kernel_stats(mnl_fields *F, int which, long long *launches, double *total_ms,
                            double *bytes_per_launch) {
  if (!F || which < 0 || which > 13) return fail("bad kernel id");
  if (which >= 11) {  // DFT data: the gather / scatter / scale kernels
    *launches = F->dftio_count[which - 11];
    *total_ms = F->dftio_ms[which - 11];
    *bytes_per_launch = F->dftio_bytes[which - 11];
    return 0;
  }
  if (which == 9 || which == 10) {  // near2far: the far-field kernel / the reduce kernel
    *launches = F->n2f_count[which - 9];
    *total_ms = F->n2f_ms[which - 9];
    *bytes_per_launch = 0;
    return 0;
  }
  if (which == 7 || which == 8) {  // multi-rank pairs: slab-face chains / E-ghost waits
    const int cat = which == 7 ? TM_CHAIN : TM_WAIT;
    *launches = F->timer_count[cat];
    *total_ms = F->timer_ms[cat];
    *bytes_per_launch = 0;
    return 0;
  }
  if (which == 5 || which == 6) {
    // temporal blocking.  5 = whole pairs of steps: launches = pairs, time = every launch of
    // the pairs (two phase launches each, the drains of the rim's last step), bytes per pair =
    // the two-step items' two steps (B, D read once and written once, the palette word where
    // the item is mixed, the border points' step n+1 B, D) + two rim steps.  6 = the rim
    // launches, one step each
    int nu = 0;
    for (int d = 0; d < 3; d++) nu += F->f.inveps[d] ? 1 : 0;
    const double ub = F->d_uidx ? 4.0 : 8.0 * nu;
    double tb_b = 0, rim_b = 0;
    if (F->fused && F->tb_have) {
      tb_b = F->tb_cells * 96.0 + (F->d_uidx ? F->tb_cells_nu : F->tb_cells) * ub +
             F->tb_border * 48.0;
      double lb, gb;
      fused_bytes(F, &lb, &gb);
      const bool tuni = F->d_uidx && F->uflag_active && F->tile_cells_nu >= 0;
      rim_b = lb - double(F->tile_cells) * 96.0 -
              (tuni ? F->tile_cells_nu : double(F->tile_cells)) * ub + F->rim_cells * 96.0 +
              (F->d_uidx ? F->rim_cells_nu : F->rim_cells) * ub;
    }
    if (which == 5) {
      *launches = F->timer_count[TM_TB];
      *total_ms = F->timer_ms[TM_TB] + F->timer_ms[TM_RIM];
      *bytes_per_launch = tb_b + 2.0 * rim_b;
      if (F->fused && F->tb_have && F->tb_pol) {  // + the polarization chunks' two steps
        double lb, gb;
        fused_bytes(F, &lb, &gb);
        *total_ms += F->timer_ms[TM_GEN];
        *bytes_per_launch += 2.0 * gb;
      }
    } else {
      *launches = F->timer_count[TM_RIM];
      *total_ms = F->timer_ms[TM_RIM];
      *bytes_per_launch = rim_b;
    }
    return 0;
  }
  if (which == 4) {  // E update (update_eh(E_stuff) incl. chi(2) Newton-Raphson, Lorentzian P)
    *launches = F->timer_count[TM_E];
    *total_ms = F->timer_ms[TM_E];
    *bytes_per_launch = 0;
    return 0;
  }
  if (which == 3) {  // DFT updates of one step (all flux objects)
    *launches = F->timer_count[TM_DFT];
    *total_ms = F->timer_ms[TM_DFT] + F->timer_ms[TM_DFTF];
    double b = 0;
    for (auto &o : F->dfts) b += o->bytes;
    *bytes_per_launch = b;
    return 0;
  }
  // 0: lean fused kernel (or interior curl B when unfused), 1: interior curl D
  // (unfused), 2: general fused kernel
  int cat = which == 0 ? TM_BINT : (which == 1 ? TM_DINT : TM_GEN);
  *launches = F->timer_count[cat];
  *total_ms = F->timer_ms[cat];
  if (F->fused && which != 1) {
    double lb, gb;
    fused_bytes(F, &lb, &gb);
    // concurrent lean + general: the timed span covers both kernels
    *bytes_per_launch = which == 0 ? (F->fused_concurrent ? lb + gb : lb) : gb;
    return 0;
  }
  if (which == 2) {
    *bytes_per_launch = 0;
    return 0;
  }
  const Box &b = F->interior;
  double pts = 1;
  for (int k = 0; k < 3; k++) pts *= double(b.hi[k] - b.lo[k] + 1);
  if (b.hi[0] < b.lo[0]) pts = 0;
  // interior curl: read 3 source comps + read/write the updated comps
  int ncomp = 0;
  const CurlPlan &p = which == 0 ? F->planB : F->planD;
  for (int d = 0; d < 3; d++) ncomp += p.present[d] ? 1 : 0;
  int nsrc = 0;
  for (int d = 0; d < 3; d++) nsrc += F->allocated[3 * (which == 0 ? T_E : T_H) + d] ? 1 : 0;
  *bytes_per_launch = pts * 8.0 * (nsrc + 2 * ncomp);
  return 0;
}

int mnl_fields_set_temporal_blocking(mnl_fields *F, int on) {
  if (!F) return fail("null fields");
  F->tb_enabled = on != 0;
  return 0;
}

int mnl_fields_set_schedule(mnl_fields *F, int which, int value) {
  if (!F) return fail("null fields");
  const bool v = value != 0;
  if (which == 0) {
    F->tb_narrow = v;
  } else if (which >= 2 && which <= 4) {  // CUs left free by the pair launches (single rank)
    if (value < -1 || value > 1024) return fail("bad reservation");
    (which == 2 ? F->tb_res : which == 3 ? F->res_l : F->res_r) = value;
    return 0;
  } else if (which == 5) {
    F->dft_cmp = v;
  } else if (which == 7) {
    F->nr_early = v;
  } else if (which == 11) {  // pairs with polarization chunks (0: one-step stepping there)
    F->tb_pol_on = v;
  } else if (which == 12) {  // R1's non-strip items beside the two-step kernel (one rank)
    F->tb_r1a = v;
  } else if (which == 16) {  // a pair's source + guard launches merged (one rank)
    F->tb_srcguard = v;
    return 0;
  } else if (which == 9) {  // most own columns of a two-step item (0: TB_OXW = 124)
    if (value != 0 && (value < 4 || value > TB_OXW)) return fail("bad two-step width");
    F->tb_ox = value;
    F->tb_ox_set = value != 0;  // the tuner keeps a width that was set
  } else if (which == 8) {  // planes per two-step item (0: automatic)
    if (value < 0 || value > 4096) return fail("bad two-step chunk");
    F->tb_zchunk = value;
  } else if (which == 6) {  // planes per rim item (0: the one-step chunk length)
    if (value < 0 || value > FUSED_MAXCH) return fail("bad rim chunk");
    F->rim_zchunk = value;
  } else if (which == 1) {
    F->dft_pal = v;
    for (auto &o : F->dfts) o->plan_key = -1;  // plans rebuilt at the next update
  } else {
    return fail("bad schedule option");
  }
  F->tb_sig = 0;  // the pair plan is rebuilt at the next batch
  return 0;
}

int mnl_fields_tb_info(mnl_fields *F, double *out, int n) {
  if (!F || !out || n < 1) return fail("bad argument");
  const double v[14] = {F->fused && F->tb_have && F->tb_enabled && F->tb_last ? 1.0 : 0.0,
                       F->tb_cells,
                       F->tb_border,
                       F->tb_cells_nu,
                       F->rim_cells,
                       F->rim_cells_nu,
                       double(F->tb_items.size()),
                       double(F->tb_ritems.size()),
                       F->tb_items.empty() ? 0.0 : double((F->tb_items[0].z >> 16) -
                                                          (F->tb_items[0].z & 0xFFFF)),
                       double(F->tb_nnarrow),
                       F->tb_enabled ? 1.0 : 0.0,
                       double(F->tb_zchunk),  // the setting (0: automatic)
                       double(F->tb_ox ? F->tb_ox : TB_OXW),  // most own columns of an item
                       F->tb_pol ? 1.0 : 0.0};  // polarization chunks stepped inside the pairs
  for (int i = 0; i < n && i < 14; i++) out[i] = v[i];
  return 0;
}

int mnl_fields_mode(mnl_fields *F, int *fused) {
  if (!F) return fail("null fields");
  *fused = (F->fused ? 1 : 0) | (F->fused && F->d_uidx ? 2 : 0) | (F->contig ? 4 : 0) |
           (F->fused ? 16 : 0) | (F->fused && F->fused_concurrent ? 32 : 0) |
           (std::min(F->contig_fallbacks, 255) << 8);
  return 0;
}

// fields::get_dft_array(dft_flux / dft_fields, c, num_freq) (src/dft.cpp:1240-1280):
// process_dft_component into a whole array (get_dft_component_dims corners; every
// chunk of c in list order; dft / stored_weight, divided by the loop weight when the
// chunk stored it; times the interpolation weights of the empty dimensions,
// src/dft.cpp:908-1040), summed over ranks (sum_to_all: one owner per point), then
// collapse_array (src/array_slice.cpp:554-601).  out: re/im interleaved.
static int dft_array_values(mnl_fields *F, int h, int c, int num_freq, int *rank,
                            long long dims[3], double *out, long long nout) {
  if (h < 0 || h >= (int)F->dfts.size()) return fail("bad dft handle");
  DftFluxH &o = *F->dfts[h];
  if (dft_flush(F, o)) return -1;  // the buffered updates first
  if (num_freq < 0 || num_freq > o.nfreq - 1)
    return fail(("process_dft_component: frequency index " + std::to_string(num_freq) +
                 " is outside the range of the frequency array of size " +
                 std::to_string(o.nfreq)).c_str());
  const mnl_structure &S = F->S;
  std::vector<const DftChunkH *> L;
  for (auto &dc : o.E)
    if (dc.c == c) L.push_back(&dc);
  for (auto &dc : o.H)
    if (dc.c == c) L.push_back(&dc);
  int mn[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, mx[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (auto *dc : L)
    for (int d = 0; d < 3; d++) mn[d] = std::min(mn[d], dc->is[d]), mx[d] = std::max(mx[d], dc->ie[d]);
  int r = 0, ds[3] = {0, 0, 0};
  long long full[3] = {1, 1, 1};
  if (!L.empty())
    for (int d = 0; d < 3; d++) {
      if (!S.has[d]) continue;
      long long n = (mx[d] - mn[d]) / 2 + 1;
      if (n > 1) ds[r] = d, full[r++] = n;
    }
  int rr = 0;  // collapse_array: directions empty in `where` are summed out
  long long rd[3] = {1, 1, 1};
  for (int k = 0; k < r; k++)
    if (o.wmax[ds[k]] - o.wmin[ds[k]] != 0.0) rd[rr++] = full[k];
  *rank = rr;
  for (int k = 0; k < 3; k++) dims[k] = k < rr ? rd[k] : 1;
  if (!out) return 0;
  long long rs[3] = {0, 0, 0}, nred = 1;
  for (int k = r - 1; k >= 0; k--)
    if (o.wmax[ds[k]] - o.wmin[ds[k]] != 0.0) rs[k] = nred, nred *= full[k];
  if (r == 0) nred = 0;
  if (nout < nred) return fail("output buffer too small");
  for (long long k = 0; k < 2 * nred; k++) out[k] = 0.0;
  if (r == 0) return 0;
  const size_t nf = o.nfreq;
  std::vector<double> v(2 * ((o.npts + 63) & ~size_t(63)) * nf);
  bool ok = true;
  if (!v.empty())
    ok = hipMemcpyAsync(v.data(), o.d_dft, v.size() * 8, hipMemcpyDeviceToHost, F->stream) ==
             hipSuccess &&
         hipStreamSynchronize(F->stream) == hipSuccess;
  if (F->nranks > 1 && F->comm->agree_ok(ok, F->stream))  // every rank fails together
    return fail(ok ? "get_dft_array: a rank failed" : "get_dft_array: device copy failed");
  if (!ok) return fail("get_dft_array: device copy failed");
  long long ntot = 1;
  for (int k = 0; k < r; k++) ntot *= full[k];
  std::vector<double> arr(2 * ntot, 0.0);
  bool empty_dim[3];
  for (int d = 0; d < 3; d++) empty_dim[d] = S.has[d] && o.wmax[d] - o.wmin[d] == 0.0;
  const int yd[3] = {S.dim == 2 ? 2 : 0, S.dim == 2 ? 0 : 1, S.dim == 2 ? 1 : 2};
  for (auto *dc : L) {
    int n[3];
    for (int k = 0; k < 3; k++) n[k] = S.has[yd[k]] ? (dc->ie[yd[k]] - dc->is[yd[k]]) / 2 + 1 : 1;
    size_t pidx = 0;  // chunk_idx: points in LOOP_OVER_IVECS order
    for (int i1 = 0; i1 < n[0]; i1++)
      for (int i2 = 0; i2 < n[1]; i2++)
        for (int i3 = 0; i3 < n[2]; i3++, pidx++) {
          const size_t pt = dc->p0 + pidx;
          const int *pj = &o.h_pj[3 * pt];
          if (pj[0] < 0 && pj[1] < 0 && pj[2] < 0) continue;  // another rank's point
          const int ii[3] = {i1, i2, i3};
          int p[3] = {0, 0, 0};
          for (int k = 0; k < 3; k++)
            if (S.has[yd[k]]) p[yd[k]] = dc->is[yd[k]] + 2 * ii[k];
          double wl[3], wi[3];
          for (int k = 0; k < 3; k++) {
            const int d = yd[k];
            wl[k] = loop_w1(dc->s0[d], dc->s1[d], dc->e0[d], dc->e1[d], ii[k], n[k]);
            wi[k] = empty_dim[d] ? wl[k] : loop_w1(1.0, 1.0, 1.0, 1.0, ii[k], n[k]);
          }
          const double w = wl[2] * (wl[1] * ((dc->dV0 + 0.0 * i2) * wl[0]));
          const double interp_w = wi[2] * (wi[1] * (1.0 * wi[0]));
          const size_t q = dft_at(o.slot[pt], num_freq, nf);
          cplx dft_val = cplx(v[2 * q], v[2 * q + 1]) / dc->stored;
          if (dc->incl && dft_val != 0.0) dft_val /= w;
          long long oi = 0;
          for (int k = 0; k < r; k++) oi = oi * full[k] + (p[ds[k]] - mn[ds[k]]) / 2;
          const cplx val = interp_w * dft_val;
          arr[2 * oi] = val.real();
          arr[2 * oi + 1] = val.imag();
        }
  }
  if (F->nranks > 1)
    for (size_t q = 0; q < arr.size(); q += 1 << 20) {
      const int n = (int)std::min<size_t>(1 << 20, arr.size() - q);
      if (timed_allreduce(F, arr.data() + q, n)) return fail("get_dft_array allreduce failed");
    }
  for (long long q = 0; q < ntot; q++) {  // collapse_array, in full-index order
    long long t = q, ri = 0;
    for (int k = r - 1; k >= 0; k--) {
      ri += (t % full[k]) * rs[k];
      t /= full[k];
    }
    out[2 * ri] += arr[2 * q];
    out[2 * ri + 1] += arr[2 * q + 1];
  }
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
  *handle = h;
  return 0;
}

int mnl_fields_dft_array(mnl_fields *F, int h, int comp, int num_freq, int *rank, long long dims[3],
                         double *out, long long nout) {
  if (!F || !rank || !dims) return fail("null argument");
  return dft_array_values(F, h, comp, num_freq, rank, dims, out, nout);
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
  *handle = h;
  return 0;
}

int mnl_fields_dft_flux(mnl_fields *F, int h, double *out) {
  if (!F || !out) return fail("null argument");
  return dft_flux_values(F, h, out);
}

int mnl_fields_dft_size(mnl_fields *F, int h, long long *n) {
  if (!F || !n) return fail("null argument");
  if (h < 0 || h >= (int)F->dfts.size()) return fail("bad dft handle");
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
  if (h < 0 || h >= (int)F->dfts.size()) return fail("bad dft handle");
  if (dft_flush(F, *F->dfts[h])) return -1;  // the buffered updates first
  const DftFluxH &o = *F->dfts[h];
  const size_t nf = o.nfreq;
  std::vector<double> v(2 * ((o.npts + 63) & ~size_t(63)) * nf);
  if (!v.empty()) {
    HIPCHK(hipStreamSynchronize(F->stream));
    HIPCHK(hipMemcpy(v.data(), o.d_dft, v.size() * 8, hipMemcpyDeviceToHost));
  }
  long long k = 0;
  for (auto &dc : which ? o.H : o.E)
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

int mnl_fields_dft_decimation(mnl_fields *F, int h, int *decimation) {
  if (!F || !decimation) return fail("null argument");
  if (h < 0 || h >= (int)F->dfts.size()) return fail("bad dft handle");
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
  if (h < 0 || h >= (int)F->dfts.size()) return fail("bad dft handle");
  if (!F->dfts[h]->n2f) return fail("near2far_medium: the handle is not a near2far object");
  *eps = F->dfts[h]->eps;
  *mu = F->dfts[h]->mu;
  return 0;
}

int mnl_fields_near2far_points(mnl_fields *F, int h, double *out, long long npoints) {
  if (!F || !out) return fail("null argument");
  return n2f_points(F, h, out, npoints);
}

int mnl_fields_traffic_model(mnl_fields *F, double *bpc, double *cells) {
  if (!F) return fail("null fields");
  // Minimal per-step HBM traffic per interior cell of the kernels in use
  // (DESIGN.md "Roofline"): fused: B, D read+write, chi1inv read;
  // unfused: curl B reads E(3)+B(3), writes B(3); curl D reads H=B(3)+D(3),
  // writes D(3); E update reads D(3) (+chi1inv 3), writes E(3) (+P terms).
  double n = 0;
  for (int d = 0; d < 3; d++) n += F->allocated[d] ? 1 : 0;
  int nu = 0;
  for (int d = 0; d < 3; d++) nu += F->f.inveps[d] ? 1 : 0;
  double b;
  if (F->fused) {  // whole fused step over G per G point (PML state included)
    double lb, gb, gc = 1;
    fused_bytes(F, &lb, &gb);
    for (int e = 0; e < 3; e++) gc *= double(F->fusedG.hi[e] - F->fusedG.lo[e] + 1);
    b = (lb + gb) / gc;
  } else {
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
  return 0;
}

}  // extern "C"
