// mnl_setup.cpp -- what a fields object is built from: PML chunk / zone tables, the rank's grid
// and boxes, curl plans, component allocation, conductivity and the H / E materials
// (finalize_fields), and initialize_field; and the structure's subpixel-averaged epsilon of
// geometric objects with its sphere quadrature (set_epsilon_geometry).
#include "mnl_host.hpp"

namespace mnlh {

// ------------------------------------------------------------- PML zones
// structure::use_pml + effort volumes (src/structure.cpp:509-523, 118-137)
// and structure_chunk::use_pml (src/structure.cpp:656-691) folded into
// per-direction tables over the global half-coordinate q = p - io.
static inline double pml_x(int i, double dx, double bloc, double a) {
  double here = i * 0.5 / a;
  return (0.5 / a * ((int)(dx * (2 * a) + 0.5) - (int)(fabs(bloc - here) * (2 * a) + 0.5)));
}

std::vector<ZoneIv> zone_intervals(const mnl_structure &S, int d) {
  std::vector<ZoneIv> iv;
  int n2 = 2 * S.n[d];
  int nlo = 0, nhi = 0;
  if (S.n[d] > 1 && S.pml_thick[d][0] > 0) nlo = int(S.pml_thick[d][0] * S.a + 1 + 0.5);
  if (S.n[d] > 1 && S.pml_thick[d][1] > 0) nhi = int(S.pml_thick[d][1] * S.a + 1 + 0.5);
  int lo_end = nlo ? 2 * nlo : 0, hi_start = nhi ? n2 - 2 * nhi : n2;
  if (nlo) iv.push_back({0, lo_end, 0});
  if (hi_start > lo_end) iv.push_back({lo_end, hi_start, 1});
  if (nhi) iv.push_back({hi_start, n2, 2});
  return iv;
}

static int build_pml_tables(mnl_fields *F) {
  const mnl_structure &S = F->S;
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    int nq = 2 * S.n[d] + 2;
    F->h_flag[d].assign(nq, 0);
    F->h_zone[d].assign(nq, 1);
    F->h_sig[d].assign(nq, 0.0);
    F->h_kap[d].assign(nq, 1.0);
    F->h_siginv[d].assign(nq, 1.0);
    auto ivs = zone_intervals(S, d);
    int nlo = 0, nhi = 0;
    for (auto &z : ivs) {
      if (z.zone == 0) nlo = 1;
      if (z.zone == 2) nhi = 1;
    }
    {  // PML chunks may touch (no interior chunk along d) but not overlap
      int lo_end = -1, hi_start = INT32_MAX;
      for (auto &z : ivs) {
        if (z.zone == 0) lo_end = z.c1;
        if (z.zone == 2) hi_start = z.c0;
      }
      if (nlo && nhi && lo_end > hi_start)
        return fail("PML layers overlap (2*int(thickness*a+1.5) > cells along a direction)");
    }
    for (auto &z : ivs) {
      // chunk-local profile, chunk io_c = io + c0, n_c = (c1-c0)/2
      int io_c = S.io[d] + z.c0, big_c = S.io[d] + z.c1;
      std::vector<double> sig, kap, siginv;
      bool flag = false;
      for (int side = 0; side < 2; side++) {
        double dx = S.pml_thick[d][side];
        if (dx <= 0.0 || S.n[d] <= 1) continue;
        double bloc = (side == 0 ? S.io[d] : S.io[d] + 2 * S.n[d]) * (0.5 * (1.0 / S.a));
        double prefac = (-log(S.pml_R[d][side])) / (4 * dx * (1. / 3.));
        double kappa_prefac = (S.pml_stretch[d][side] - 1) / (1. / 4.);
        bool found = false;
        for (int i = io_c; i <= big_c + 1; ++i)
          if (pml_x(i, dx, bloc, S.a) > 0) {
            found = true;
            break;
          }
        if (!found) continue;
        flag = true;
        int nc = big_c - io_c + 2;
        sig.assign(nc, 0.0);
        kap.assign(nc, 1.0);
        siginv.assign(nc, 1.0);
        for (int i = io_c; i <= big_c + 1; ++i) {
          int idx = i - io_c;
          double x = pml_x(i, dx, bloc, S.a);
          if (x > 0) {
            double u = x / dx;
            double sp = u * u;
            sig[idx] = 0.5 * F->dt * prefac * sp;
            kap[idx] = 1 + kappa_prefac * sp * (x / dx);
            siginv[idx] = 1 / (kap[idx] + sig[idx]);
          }
        }
      }
      // owned half-coords of this chunk: (c0, c1]
      for (int q = z.c0 + 1; q <= z.c1; q++) {
        F->h_zone[d][q] = (uint8_t)z.zone;
        if (flag) {
          F->h_flag[d][q] = 1;
          F->h_sig[d][q] = sig[q - z.c0];
          F->h_kap[d][q] = kap[q - z.c0];
          F->h_siginv[d][q] = siginv[q - z.c0];
        }
      }
      if (flag) F->pml_any[d] = true;
      // The cell's not-owned plane 0 lies in the first chunk's arrays.  Nothing steps it, but
      // whoever reads a component there (the centred DFT average beside a low wall, get_field)
      // must pick the chunk's separate H as at the chunk's owned points: the two differ once
      // initialize_field has added to B after the first H update copied it.
      if (flag && z.c0 == 0) F->h_flag[d][0] = 1;
    }
  }
  return 0;
}

// ------------------------------------------------------------- grid / boxes
// Equal split of the slab-axis cells over ranks (first `rem` ranks get one more).
void slab_range(int ncell, int rank, int nranks, int *lo, int *hi) {
  int base = ncell / nranks, rem = ncell % nranks;
  *lo = rank * base + std::min(rank, rem);
  *hi = *lo + base + (rank < rem ? 1 : 0);
}

static void setup_grid(mnl_fields *F) {
  const mnl_structure &S = F->S;
  DevGrid &g = F->g;
  memset(&g, 0, sizeof(g));
  g.dim = S.dim;
  int nax = 0;
  for (int d = 0; d < 3; d++) g.ax[d] = S.has[d] ? nax++ : -1;
  // slab direction = slowest present direction
  F->slab_dir = S.has[2] ? 2 : 1;
  int lo_cell = 0, hi_cell = S.n[F->slab_dir];
  slab_range(S.n[F->slab_dir], F->rank, F->nranks, &lo_cell, &hi_cell);
  int Nax[3] = {1, 1, 1};
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    g.nglob[d] = S.n[d];
    g.wall[d] = F->periodic[d] ? 0 : 1;
    if (d == F->slab_dir) {
      g.off[d] = lo_cell;
      Nax[g.ax[d]] = hi_cell - lo_cell + 1;
      int nloc = hi_cell - lo_cell;
      g.owned_lo_sh[d] = 0;
      g.owned_hi_sh[d] = nloc - 1;
      g.owned_lo_un[d] = 1;
      // global wall plane excluded (a periodic direction has none: plane n is owned)
      g.owned_hi_un[d] = (hi_cell == S.n[d] && !F->periodic[d]) ? nloc - 1 : nloc;
    } else {
      g.off[d] = 0;
      Nax[g.ax[d]] = S.n[d] + 1;
      g.owned_lo_sh[d] = 0;
      g.owned_hi_sh[d] = S.n[d] - 1;
      g.owned_lo_un[d] = 1;
      g.owned_hi_un[d] = F->periodic[d] ? S.n[d] : S.n[d] - 1;
    }
  }
  for (int k = 0; k < 3; k++) g.N[k] = Nax[k];
  long long p0 = (g.N[0] + 15) / 16 * 16;
  if (g.N[1] == 1 && g.N[2] == 1) p0 = g.N[0];
  g.st[0] = 1;
  g.st[1] = p0;
  g.st[2] = p0 * g.N[1];
  F->nlocal = size_t(p0) * g.N[1] * g.N[2];
  for (int d = 0; d < 3; d++) g.sdir[d] = g.ax[d] >= 0 ? g.st[g.ax[d]] : 0;
}

// fields::use_bloch(d, 0) (src/fields.cpp:75-90): the ownership ranges of the grid change, the
// array extents, the boxes (PML only) and everything allocated do not
int set_periodic(mnl_fields *F, int dir) {
  F->periodic[dir] = true;
  setup_grid(F);
  F->tb_sig = 0;
  return 0;
}

static void make_shell_list(mnl_fields *F) {
  BoxList &bl = F->shell_list;
  memset(&bl, 0, sizeof(bl));
  long long acc = 0;
  for (auto &b : F->shell) {
    bool emp = false;
    for (int k = 0; k < 3; k++) emp = emp || b.hi[k] < b.lo[k];
    if (emp) continue;
    bl.b[bl.n] = b;
    bl.start[bl.n] = acc;
    acc += (long long)(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1) * (b.hi[2] - b.lo[2] + 1);
    bl.n++;
  }
  bl.start[bl.n] = acc;
}

static void setup_boxes(mnl_fields *F) {
  const mnl_structure &S = F->S;
  DevGrid &g = F->g;
  int ilo[3] = {0, 0, 0}, ihi[3] = {0, 0, 0};  // per device axis, local
  bool none = false;
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) continue;
    int n = S.n[d];
    std::vector<char> good(n + 1);
    for (int j = 0; j <= n; j++) {
      int q0 = 2 * j, q1 = 2 * j + 1;
      bool ok = F->h_flag[d][q0] == 0 && F->h_flag[d][q1] == 0;
      if (F->nr) ok = ok && F->h_zone[d][q0] == 1 && F->h_zone[d][q1] == 1;
      good[j] = ok;
    }
    int lo = 0;
    while (lo <= n && !good[lo]) lo++;
    int hi = n;
    while (hi >= 0 && !good[hi]) hi--;
    for (int j = lo; j <= hi; j++)
      if (!good[j]) lo = hi + 1;  // non-contiguous: no interior
    if (lo > hi) none = true;
    int a = g.ax[d];
    int l = lo - g.off[d], h = hi - g.off[d];
    l = std::max(l, 0);
    h = std::min(h, g.N[a] - 1);
    if (l > h) none = true;
    ilo[a] = l;
    ihi[a] = h;
  }
  Box full;
  for (int k = 0; k < 3; k++) full.lo[k] = 0, full.hi[k] = g.N[k] - 1;
  F->shell.clear();
  if (none) {
    F->interior = full;
    F->interior.hi[0] = -1;  // empty
    F->shell.push_back(full);
    return;
  }
  Box in = full;
  for (int k = 0; k < 3; k++)
    if (g.N[k] > 1 || ihi[k] >= ilo[k]) in.lo[k] = ilo[k], in.hi[k] = ihi[k];
  F->interior = in;
  // onion shell decomposition, slowest axis first
  Box cur = full;
  for (int k = 2; k >= 0; k--) {
    if (in.lo[k] > cur.lo[k]) {
      Box b = cur;
      b.hi[k] = in.lo[k] - 1;
      F->shell.push_back(b);
    }
    if (in.hi[k] < cur.hi[k]) {
      Box b = cur;
      b.lo[k] = in.hi[k] + 1;
      F->shell.push_back(b);
    }
    cur.lo[k] = in.lo[k];
    cur.hi[k] = in.hi[k];
  }
}

// ------------------------------------------------------------- allocation
static bool is_like(int dim, int c1, int c2) {  // src/fields.cpp:473-491
  if (dim != 2) return true;
  auto tm = [](int c) {
    return c == MNL_HX || c == MNL_HY || c == MNL_BX || c == MNL_BY || c == MNL_EZ ||
           c == MNL_DZ;
  };
  return !(tm(c1) ^ tm(c2));
}
bool has_field(const mnl_structure &S, int c) {
  if (S.dim == 1) return c == MNL_EX || c == MNL_HY || c == MNL_DX || c == MNL_BY;
  return true;
}

static void make_plans(mnl_fields *F) {
  // src/fields.cpp:438-471: comp d of B/D gets term1 (comp (d+2)%3 along (d+1)%3)
  // if that direction exists and the partner is allocated, term2 likewise.
  const mnl_structure &S = F->S;
  for (int t = 0; t < 2; t++) {
    CurlPlan &p = t == 0 ? F->planB : F->planD;
    int ft = t == 0 ? T_B : T_D, src = t == 0 ? T_E : T_H;
    for (int d = 0; d < 3; d++) {
      p.present[d] = F->allocated[3 * ft + d];
      int terms = 0;
      int c1 = (d + 2) % 3, dir1 = (d + 1) % 3, c2 = (d + 1) % 3, dir2 = (d + 2) % 3;
      if (S.has[dir1] && F->allocated[3 * src + c1]) terms |= 1;
      if (S.has[dir2] && F->allocated[3 * src + c2]) terms |= 2;
      p.terms[d] = terms;
      if (!terms) p.present[d] = 0;
    }
  }
  for (int d = 0; d < 3; d++) {
    F->f.ecomp_present[d] = F->allocated[3 * T_E + d];
    F->f.hcomp_present[d] = F->allocated[3 * T_H + d];
  }
}

static int alloc_component(mnl_fields *F, int c) {
  int t = ctype(c), d = cdir(c);
  if (F->allocated[c]) return 0;
  double **slot = nullptr;
  switch (t) {
    case T_E: slot = &F->f.E[d]; break;
    case T_D: slot = &F->f.D[d]; break;
    case T_B: slot = &F->f.B[d]; break;
    case T_H: slot = nullptr; break;
  }
  if (slot && !*slot)
    if (dev_alloc(F, slot, F->nlocal)) return -1;
  if (t == T_D) F->f.Dn[d] = F->f.D[d];
  if (t == T_H) {
    if (!F->f.B[d] && dev_alloc(F, &F->f.B[d], F->nlocal)) return -1;
    F->f.Bn[d] = F->f.B[d];
    // H separate in chunks with PML along d (src/update_eh.cpp:204-209); with H-side
    // materials stored everywhere (a copy of B where the chunk aliases it)
    if (F->pml_any[d] || F->hall)
      if (dev_alloc(F, &F->f.H[d], F->nlocal)) return -1;
    if (F->pml_any[d])
      if (dev_alloc(F, &F->f.WH[d], F->nlocal)) return -1;
  }
  if (t == T_B) F->f.Bn[d] = F->f.B[d];
  if (t == T_E) F->f.En[d] = F->f.E[d];
  if (t == T_H) F->f.Hn[d] = F->f.H[d];
  if (t == T_E && F->pml_any[d] && !F->f.WE[d])
    if (dev_alloc(F, &F->f.WE[d], F->nlocal)) return -1;
  if (t == T_B || t == T_D) {
    int du = (d + 2) % 3;  // dsigu = cycle(d,2): f_u auxiliary (src/step_db.cpp:71-75)
    double **u = t == T_B ? &F->f.UB[d] : &F->f.UD[d];
    if (F->S.has[du] && F->pml_any[du] && !*u)
      if (dev_alloc(F, u, F->nlocal)) return -1;
    if (t == T_B) F->f.UBn[d] = F->f.UB[d];
  }
  F->allocated[c] = true;
  return 0;
}

int require_component(mnl_fields *F, int c) {  // src/fields.cpp:566-586
  for (int ca = 0; ca < MNL_NUM_COMPONENTS; ca++) {
    if (!has_field(F->S, ca) || !is_like(F->S.dim, c, ca)) continue;
    if (alloc_component(F, ca)) return -1;
  }
  // polarizations: P for every allocated E comp with nontrivial sigma
  for (int k = 0; k < F->f.npol; k++) {
    const Lorentz &L = F->S.lor[F->S.lor.size() - 1 - k];
    PolDev &pd = F->f.pol[k];
    for (int d = 0; d < 3; d++)
      if (F->allocated[d] && !L.sigma[d].empty() && pd.sigma[d] && !pd.P[d]) {
        if (dev_alloc(F, &pd.P[d], F->nlocal)) return -1;
        if (dev_alloc(F, &pd.Pp[d], F->nlocal)) return -1;
      }
  }
  // magnetic polarizations: P of every allocated H comp with nontrivial sigma; then
  // f_minus_p of B exists in every chunk (needs_P uses the global sigma flags,
  // src/update_eh.cpp:84-100), so H is separate everywhere (src/update_eh.cpp:204-209)
  for (int k = 0; k < F->f.nhpol; k++) {
    const Lorentz &L = F->S.hlor[F->S.hlor.size() - 1 - k];
    PolDev &pd = F->f.hpol[k];
    for (int d = 0; d < 3; d++)
      if (F->allocated[3 * T_H + d] && !L.sigma[d].empty() && pd.sigma[d] && !pd.P[d]) {
        if (dev_alloc(F, &pd.P[d], F->nlocal)) return -1;
        if (dev_alloc(F, &pd.Pp[d], F->nlocal)) return -1;
        F->f.hsep_all = 1;
      }
  }
  make_plans(F);
  return 0;
}

// upload a canonical host array into a device-layout buffer of this rank
static int upload_canonical(mnl_fields *F, double *dst, const std::vector<double> &host, int comp) {
  size_t nt = F->S.ntot;
  if (F->scratch_cap < nt) {
    if (F->d_scratch) hipFree(F->d_scratch);
    HIPCHK(hipMalloc(&F->d_scratch, nt * sizeof(double)));
    F->scratch_cap = nt;
  }
  HIPCHK(hipMemcpyAsync(F->d_scratch, host.data(), nt * sizeof(double), hipMemcpyHostToDevice,
                        F->stream));
  if (k_from_canonical(dst, F->d_scratch, F->g, ctype(comp), cdir(comp), 0, F->stream))
    return fail("from_canonical kernel launch failed");
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

// Is a chi1inv row entry nontrivial inside the reference chunk that covers
// zone box (zx,zy,zz)?  Chunk array points: [io_c+shift, big_c+shift]
// (src/anisotropic_averaging.cpp:246-296 trivial test over LOOP_OVER_VOL).
static bool nontrivial_in_zone(const mnl_structure &S, const std::vector<double> &arr, int comp,
                               const ZoneIv *zv[3], double trivial) {
  int lo[3], hi[3];
  for (int d = 0; d < 3; d++) {
    if (!S.has[d]) {
      lo[d] = hi[d] = 0;
      continue;
    }
    // points j with io+2j+sh in [io + c0 + sh, io + c1 + sh]  <=>  j in [c0/2, c1/2]
    lo[d] = zv[d]->c0 / 2;
    hi[d] = zv[d]->c1 / 2;
  }
  for (int x = lo[0]; x <= hi[0]; x++)
    for (int y = lo[1]; y <= hi[1]; y++)
      for (int z = lo[2]; z <= hi[2]; z++) {
        long long i = x * S.cstride(0) + y * S.cstride(1) + z * S.cstride(2);
        if (arr[i] != trivial) return true;
      }
  (void)comp;
  return false;
}

static std::vector<ZoneIv> zone_ivs_or_one(const mnl_structure &S, int d) {
  if (S.has[d]) return zone_intervals(S, d);
  return {{0, 0, 1}};
}

// Conductivity of the D and B components: cnd and cndinv = 1/(1 + cnd*dt*0.5)
// (structure_chunk::update_condinv, src/structure.cpp:693-707) where nonzero
// anywhere; f_cond where a PML lies along dsig = cycle(d, 1); per reference
// chunk, whether its conductivity array survives the trivial test
// (src/structure.cpp:898-901) -- that selects the f_cond branch of step_curl.
static int setup_conductivity(mnl_fields *F) {
  const mnl_structure &S = F->S;
  DevFields &f = F->f;
  std::vector<uint8_t> cz(27, 0);
  bool any = false;
  for (int t = 0; t < 2; t++)
    for (int d = 0; d < 3; d++) {
      const int comp = 3 * (t ? T_D : T_B) + d;
      const auto &cv = S.cond[t][d];
      if (!has_field(S, comp) || cv.empty() || all_eq(cv, 0.0)) continue;
      any = true;
      std::vector<double> inv(cv.size());
      for (size_t i = 0; i < cv.size(); i++) inv[i] = 1 / (1 + cv[i] * F->dt * 0.5);
      double *pc, *pi;
      if (dev_alloc(F, &pc, F->nlocal) || dev_alloc(F, &pi, F->nlocal)) return -1;
      if (upload_canonical(F, pc, cv, comp) || upload_canonical(F, pi, inv, comp)) return -1;
      f.cnd[t][d] = pc;
      f.cndinv[t][d] = pi;
      const int dsig = (d + 1) % 3;
      if (S.has[dsig] && F->pml_any[dsig] && dev_alloc(F, &f.fcnd[t][d], F->nlocal)) return -1;
      auto ivx = zone_ivs_or_one(S, 0), ivy = zone_ivs_or_one(S, 1), ivz = zone_ivs_or_one(S, 2);
      for (auto &zx : ivx)
        for (auto &zy : ivy)
          for (auto &zz : ivz) {
            const ZoneIv *zv[3] = {&zx, &zy, &zz};
            if (nontrivial_in_zone(S, cv, comp, zv, 0.0))
              cz[zx.zone * 9 + zy.zone * 3 + zz.zone] |= 1 << (3 * t + d);
          }
    }
  f.cnd_dt2 = F->dt * 0.5;
  if (!any) return 0;
  uint8_t *dcz;
  if (dev_alloc(F, &dcz, 27)) return -1;
  HIPCHK(hipMemcpyAsync(dcz, cz.data(), 27, hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  f.cnd_zone = dcz;
  return 0;
}

// H-side materials: chi1inv of the H components (set_mu) and
// magnetic Lorentzian susceptibilities.  The fork's update_eh(H_stuff) takes
// step_update_EDHB's diagonal branch whatever off-diagonal rows exist (its 3x3 branch
// needs chi3, which no H component has, src/step_generic.cpp:730-906), so only the
// diagonal enters the arithmetic; the rows still decide per reference chunk whether H is
// separate from B (chi1inv[H_c][c] kept: the diagonal given and some entry of the row
// nontrivial in the chunk, src/anisotropic_averaging.cpp:279-296, src/update_eh.cpp:204-209).
static int setup_h_materials(mnl_fields *F) {
  const mnl_structure &S = F->S;
  DevFields &f = F->f;
  bool mu_any = false, hl_any = false, off_any = false;
  for (int c = 0; c < 3; c++) {
    if (!has_field(S, 3 * T_H + c)) continue;
    for (int d = 0; d < 3; d++) {
      const auto &v = S.mu1inv[c][d];
      if (v.empty() || all_eq(v, d == c ? 1.0 : 0.0)) continue;
      mu_any = true;
      off_any = off_any || d != c;
    }
  }
  for (const Lorentz &L : S.hlor)
    for (int d = 0; d < 3; d++)
      hl_any = hl_any || (!L.sigma[d].empty() && has_field(S, 3 * T_H + d));
  F->hall = mu_any || hl_any;
  f.hall = F->hall ? 1 : 0;
  if (!F->hall) return 0;
  if (S.nl_mode == 1 && off_any)  // upstream Meep would average them in (OFFDIAG)
    return fail("off-diagonal mu is not supported in the upstream nonlinear mode");
  if ((int)S.hlor.size() > MAX_HPOL) return fail("too many magnetic susceptibilities (max 2)");
  for (int c = 0; c < 3; c++) {
    const auto &diag = S.mu1inv[c][c];
    if (!has_field(S, 3 * T_H + c) || diag.empty() || all_eq(diag, 1.0)) continue;
    double *p;
    if (dev_alloc(F, &p, F->nlocal)) return -1;
    if (upload_canonical(F, p, diag, 3 * T_H + c)) return -1;
    f.invmu[c] = p;
  }
  std::vector<uint8_t> hz(27, 0);
  auto ivx = zone_ivs_or_one(S, 0), ivy = zone_ivs_or_one(S, 1), ivz = zone_ivs_or_one(S, 2);
  for (auto &zx : ivx)
    for (auto &zy : ivy)
      for (auto &zz : ivz) {
        const ZoneIv *zv[3] = {&zx, &zy, &zz};
        for (int c = 0; c < 3; c++) {
          if (!has_field(S, 3 * T_H + c) || S.mu1inv[c][c].empty()) continue;
          bool nt = false;
          for (int d = 0; d < 3 && !nt; d++) {
            const auto &v = S.mu1inv[c][d];
            nt = !v.empty() && nontrivial_in_zone(S, v, 3 * T_H + c, zv, d == c ? 1.0 : 0.0);
          }
          if (nt) hz[zx.zone * 9 + zy.zone * 3 + zz.zone] |= 1 << c;
        }
      }
  uint8_t *dz;
  if (dev_alloc(F, &dz, 27)) return -1;
  HIPCHK(hipMemcpyAsync(dz, hz.data(), 27, hipMemcpyHostToDevice, F->stream));
  f.hsep_zone = dz;
  F->h_hsep_zone = hz;
  // magnetic pol list: reverse add order (as the E side)
  const int nh = (int)S.hlor.size();
  f.nhpol = nh;
  for (int k = 0; k < nh; k++) {
    const Lorentz &L = S.hlor[nh - 1 - k];
    PolDev &pd = f.hpol[k];
    const double omega2pi = 2 * pi * L.omega0, g2pi = L.gamma * 2 * pi;
    pd.omega0dtsqr = omega2pi * omega2pi * F->dt * F->dt;
    pd.gamma1inv = 1 / (1 + g2pi * F->dt / 2);
    pd.gamma1 = (1 - g2pi * F->dt / 2);
    pd.omega0dtsqr_denom = L.drude ? 0 : pd.omega0dtsqr;
    for (int d = 0; d < 3; d++) {
      if (L.sigma[d].empty() || !has_field(S, 3 * T_H + d)) continue;
      double *p;
      if (dev_alloc(F, &p, F->nlocal)) return -1;
      if (upload_canonical(F, p, L.sigma[d], 3 * T_H + d)) return -1;
      pd.sigma[d] = p;
    }
  }
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

static int setup_materials(mnl_fields *F) {
  const mnl_structure &S = F->S;
  DevFields &f = F->f;
  // Newton-Raphson needed? chi2 nontrivial and both off-diagonal rows present.
  F->nr = false;
  F->upnl = false;
  if (S.nl_mode == 1) {  // upstream Meep: Pade chi2/chi3 on every E point, no NR
    for (int c = 0; c < 3; c++)
      for (const auto *v : {&S.chi2[c], &S.chi3[c]})
        if (!v->empty() && !all_eq(*v, 0.0)) F->upnl = true;
    for (auto &b : S.boxes) F->upnl = F->upnl || ((b.kind == 1 || b.kind == 2) && b.value != 0.0);
    // off-diagonal chi1inv rows: the upstream OFFDIAG averages (step_generic.cpp:597-598)
    for (int c = 0; c < 3; c++)
      for (int k = 1; k <= 2; k++) {
        const auto &od = S.chi1inv[c][(c + k) % 3];
        if (!od.empty() && !all_eq(od, 0.0)) F->upnl = true;
      }
  }
  auto has_offd = [&](int c) {
    for (int k = 1; k <= 2; k++) {
      const auto &od = S.chi1inv[c][(c + k) % 3];
      if (!od.empty() && !all_eq(od, 0.0)) return true;
    }
    return false;
  };
  // chi2 nontrivial on component c: a host array or a chi2 box (rasterised below)
  bool box_chi2 = false;
  for (auto &b : S.boxes) box_chi2 = box_chi2 || (b.kind == 1 && b.value != 0.0);
  auto chi2_nt = [&](int c) { return box_chi2 || (!S.chi2[c].empty() && !all_eq(S.chi2[c], 0.0)); };
  for (int c = 0; c < 3 && !F->upnl; c++) {
    if (!chi2_nt(c)) continue;
    int d1 = (c + 1) % 3, d2 = (c + 2) % 3;
    if (!S.chi1inv[c][d1].empty() && !all_eq(S.chi1inv[c][d1], 0.0) &&
        !S.chi1inv[c][d2].empty() && !all_eq(S.chi1inv[c][d2], 0.0))
      F->nr = true;
  }
  bool box_eps = false;
  for (auto &b : S.boxes) box_eps = box_eps || b.kind == 0;
  for (int c = 0; c < 3; c++) {
    if (!has_field(S, c)) continue;
    const auto &diag = S.chi1inv[c][c];
    bool need = (!diag.empty() && !all_eq(diag, 1.0)) || F->nr || box_eps ||
                (F->upnl && has_offd(c));
    if (need) {
      double *p;
      if (dev_alloc(F, &p, F->nlocal)) return -1;
      if (!diag.empty()) {
        if (upload_canonical(F, p, diag, c)) return -1;
      } else if (k_fill(p, 1.0, F->nlocal, F->stream))
        return fail("fill failed");
      f.inveps[c] = p;
    }
    if (F->nr || F->upnl) {
      for (int k = 0; k < 2; k++) {
        int dd = (c + 1 + k) % 3;
        const auto &od = S.chi1inv[c][dd];
        if (od.empty() || (F->upnl && all_eq(od, 0.0))) continue;
        double *p;
        if (dev_alloc(F, &p, F->nlocal)) return -1;
        if (upload_canonical(F, p, od, c)) return -1;
        f.offd[c][k] = p;
      }
    }
    if (F->nr && chi2_nt(c)) {
      double *p;
      if (dev_alloc(F, &p, F->nlocal)) return -1;  // zeroed: boxes are filled in below
      if (!S.chi2[c].empty() && upload_canonical(F, p, S.chi2[c], c)) return -1;
      f.chi2[c] = p;
    }
    if (F->upnl) {  // both arrays on every E component (zeros where absent)
      const std::vector<double> *src[2] = {&S.chi2[c], &S.chi3[c]};
      for (int k = 0; k < 2; k++) {
        double *p;
        if (dev_alloc(F, &p, F->nlocal)) return -1;
        if (!src[k]->empty() && upload_canonical(F, p, *src[k], c)) return -1;
        (k == 0 ? f.chi2[c] : f.chi3[c]) = p;
      }
    }
  }
  // offdiag presence per reference chunk (zone box)
  std::vector<uint8_t> oz(27, 0);
  if (F->nr || F->upnl) {
    std::vector<ZoneIv> ivs[3];
    for (int d = 0; d < 3; d++) {
      if (S.has[d])
        ivs[d] = zone_intervals(S, d);
      else
        ivs[d] = {{0, 0, 1}};
    }
    for (auto &zx : ivs[0])
      for (auto &zy : ivs[1])
        for (auto &zz : ivs[2]) {
          const ZoneIv *zv[3] = {&zx, &zy, &zz};
          int zb = zx.zone * 9 + zy.zone * 3 + zz.zone;
          for (int c = 0; c < 3; c++)
            for (int k = 0; k < 2; k++) {
              int dd = (c + 1 + k) % 3;
              const auto &od = S.chi1inv[c][dd];
              if (!od.empty() && nontrivial_in_zone(S, od, c, zv, 0.0)) oz[zb] |= 1 << (3 * c + k);
            }
        }
  }
  uint8_t *doz;
  if (dev_alloc(F, &doz, 27)) return -1;
  HIPCHK(hipMemcpyAsync(doz, oz.data(), 27, hipMemcpyHostToDevice, F->stream));
  f.offd_zone = doz;
  if (setup_conductivity(F)) return -1;
  f.nr_enabled = F->nr ? 1 : 0;
  f.upnl = F->upnl ? 1 : 0;
  // Lorentzian susceptibilities: pol list = reverse add order
  // (src/anisotropic_averaging.cpp:368-369, src/fields.cpp:266-282)
  int nl = (int)S.lor.size();
  if (nl > MAX_POL) return fail("too many susceptibilities");
  f.npol = nl;
  bool box_sig = false;
  for (auto &b : S.boxes) box_sig = box_sig || b.kind == 3;
  for (int k = 0; k < nl; k++) {
    const Lorentz &L = S.lor[nl - 1 - k];
    PolDev &pd = f.pol[k];
    const double omega2pi = 2 * pi * L.omega0, g2pi = L.gamma * 2 * pi;
    pd.omega0dtsqr = omega2pi * omega2pi * F->dt * F->dt;
    pd.gamma1inv = 1 / (1 + g2pi * F->dt / 2);
    pd.gamma1 = (1 - g2pi * F->dt / 2);
    pd.omega0dtsqr_denom = L.drude ? 0 : pd.omega0dtsqr;
    for (int d = 0; d < 3; d++) {
      if (L.sigma[d].empty() || !has_field(S, d)) continue;
      double *p;
      if (dev_alloc(F, &p, F->nlocal)) return -1;
      if (upload_canonical(F, p, L.sigma[d], d)) return -1;
      pd.sigma[d] = p;
    }
    if (L.aniso()) {  // off-diagonal sigma + per-chunk array presence (zone boxes)
      f.aniso = 1;
      for (int c = 0; c < 3; c++)
        for (int d = 0; d < 3; d++) {
          if (L.off[c][d].empty() || !has_field(S, c)) continue;
          double *p;
          if (dev_alloc(F, &p, F->nlocal)) return -1;
          if (upload_canonical(F, p, L.off[c][d], c)) return -1;
          pd.soff[c][d] = p;
        }
      std::vector<uint16_t> zb(27, 0);
      auto ivx = zone_ivs_or_one(S, 0), ivy = zone_ivs_or_one(S, 1), ivz = zone_ivs_or_one(S, 2);
      for (auto &zx : ivx)
        for (auto &zy : ivy)
          for (auto &zz : ivz) {
            const ZoneIv *zv[3] = {&zx, &zy, &zz};
            uint16_t &m = zb[zx.zone * 9 + zy.zone * 3 + zz.zone];
            for (int c = 0; c < 3; c++) {
              bool row = !L.sigma[c].empty() && nontrivial_in_zone(S, L.sigma[c], c, zv, 0.0);
              for (int d = 0; d < 3; d++)
                if (d != c && !L.off[c][d].empty() && nontrivial_in_zone(S, L.off[c][d], c, zv, 0.0)) {
                  m |= 1 << (3 * c + d);
                  row = true;
                }
              if (row) m |= 1 << (4 * c);
            }
          }
      uint16_t *dz;
      if (dev_alloc(F, &dz, 27)) return -1;
      HIPCHK(hipMemcpyAsync(dz, zb.data(), 27 * sizeof(uint16_t), hipMemcpyHostToDevice, F->stream));
      HIPCHK(hipStreamSynchronize(F->stream));
      pd.zbits = dz;
    }
    (void)box_sig;
  }
  // geometry boxes (device rasterisation)
  for (auto &b : S.boxes) {
    double lo[3] = {b.box[0], b.box[2], b.box[4]}, hi[3] = {b.box[1], b.box[3], b.box[5]};
    for (int c = 0; c < 3; c++) {
      if (!has_field(S, c)) continue;
      double *dst = nullptr;
      int invert = 0;
      if (b.kind == 0) {
        dst = const_cast<double *>(f.inveps[c]);
        invert = 1;
      } else if (b.kind == 1)
        dst = const_cast<double *>(f.chi2[c]);
      else if (b.kind == 2)
        dst = const_cast<double *>(f.chi3[c]);  // upstream mode only (null otherwise)
      else if (b.kind == 3 && b.index < nl)
        dst = const_cast<double *>(f.pol[nl - 1 - b.index].sigma[c]);
      if (!dst) continue;
      if (k_box_fill(dst, F->g, T_E, c, lo, hi, b.value, invert, S.a, S.io, F->stream))
        return fail("box fill failed");
    }
  }
  // where each susceptibility can be nonzero (DESIGN.md "Dispersive E update")
  if (nl > 0) {
    int *dbox;
    if (dev_alloc(F, &dbox, 6 * nl, false)) return -1;
    std::vector<int> init(6 * nl);
    for (int k = 0; k < nl; k++)
      for (int e = 0; e < 3; e++) init[6 * k + e] = INT32_MAX, init[6 * k + 3 + e] = -1;
    HIPCHK(hipMemcpyAsync(dbox, init.data(), init.size() * 4, hipMemcpyHostToDevice, F->stream));
    for (int k = 0; k < nl; k++) {
      const double *sg[3] = {f.pol[k].sigma[0], f.pol[k].sigma[1], f.pol[k].sigma[2]};
      if (k_nonzero_box(sg, F->g, dbox + 6 * k, F->stream)) return fail("sigma box failed");
    }
    HIPCHK(hipMemcpyAsync(init.data(), dbox, init.size() * 4, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipStreamSynchronize(F->stream));
    for (int k = 0; k < nl; k++)
      for (int e = 0; e < 3; e++) {
        f.pol[k].nz.lo[e] = init[6 * k + e];
        f.pol[k].nz.hi[e] = init[6 * k + 3 + e];
      }
  }
  if (setup_h_materials(F)) return -1;
  // The E update reaches the high metallic wall planes the reference's chunks own
  // (zeroed only afterwards by step_boundaries): with D = 0 there, E is nonzero
  // only through neighbour reads (OFFDIAG, Newton-Raphson), and only a
  // polarization keeps what update_P reads of it.
  bool any_offd = false;
  for (int c = 0; c < 3; c++) any_offd = any_offd || f.offd[c][0] || f.offd[c][1];
  f.wall_e = ((F->upnl && any_offd) || F->nr) && f.npol > 0 ? 1 : 0;
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

static int upload_pml(mnl_fields *F) {
  for (int d = 0; d < 3; d++) {
    if (!F->S.has[d] || !F->pml_any[d]) continue;
    size_t nq = F->h_flag[d].size();
    uint8_t *fl, *zn;
    double *sg, *kp, *si;
    if (dev_alloc(F, &fl, nq) || dev_alloc(F, &zn, nq) || dev_alloc(F, &sg, nq) ||
        dev_alloc(F, &kp, nq) || dev_alloc(F, &si, nq))
      return -1;
    HIPCHK(hipMemcpyAsync(fl, F->h_flag[d].data(), nq, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(zn, F->h_zone[d].data(), nq, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(sg, F->h_sig[d].data(), nq * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(kp, F->h_kap[d].data(), nq * 8, hipMemcpyHostToDevice, F->stream));
    HIPCHK(hipMemcpyAsync(si, F->h_siginv[d].data(), nq * 8, hipMemcpyHostToDevice, F->stream));
    F->f.pml.flag[d] = fl;
    F->f.pml.sig[d] = sg;
    F->f.pml.kap[d] = kp;
    F->f.pml.siginv[d] = si;
    F->f.zone[d] = zn;
  }
  for (int d = 0; d < 3; d++) {  // zone tables are needed by the NR kernel everywhere
    if (!F->S.has[d] || F->f.zone[d]) continue;
    size_t nq = F->h_zone[d].size();
    uint8_t *zn;
    if (dev_alloc(F, &zn, nq)) return -1;
    HIPCHK(hipMemcpyAsync(zn, F->h_zone[d].data(), nq, hipMemcpyHostToDevice, F->stream));
    F->f.zone[d] = zn;
  }
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}

int finalize_fields(mnl_fields *F) {
  if (build_pml_tables(F)) return -1;
  setup_grid(F);
  if (upload_pml(F)) return -1;
  if (setup_materials(F)) return -1;
  setup_boxes(F);
  make_shell_list(F);
  if (dev_alloc(F, &F->d_nr_fallbacks, 1)) return -1;
  F->f.nr_fallbacks = F->d_nr_fallbacks;
  if (F->nr) {  // first attempts that fail are finished in parallel by nr_hard_kernel
    if (dev_alloc(F, &F->d_nr_hard, NR_HARD_CAP) || dev_alloc(F, &F->d_nr_hard_cnt, 1)) return -1;
    F->f.nr_hard_cnt = F->d_nr_hard_cnt;
    F->f.nr_hard_cap = NR_HARD_CAP;
  }
  make_plans(F);
  return 0;
}

// fields::initialize_field(c, func) (src/initialize.cpp:135-148) with the
// function's values given as a whole-cell host array (canonical layout, real
// part): add, step_boundaries(type(c)); for D / B also update_eh(E / H) and
// step_boundaries of that type.  Integrated-source dipoles are not subtracted
// in that E update (DESIGN.md "initialize_field").
int initialize_field(mnl_fields *F, int c, const double *host) {
  if (require_component(F, c)) return -1;
  if (F->fused && set_fused(F, false)) return -1;
  const int t = ctype(c), d = cdir(c);
  DevFields &f = F->f;
  size_t nt = F->S.ntot;
  if (F->scratch_cap < nt) {
    HIPCHK(hipStreamSynchronize(F->stream));
    if (F->d_scratch) hipFree(F->d_scratch);
    F->d_scratch = nullptr;
    HIPCHK(hipMalloc(&F->d_scratch, nt * sizeof(double)));
    F->scratch_cap = nt;
  }
  HIPCHK(hipMemcpyAsync(F->d_scratch, host, nt * sizeof(double), hipMemcpyHostToDevice, F->stream));
  double *dst = nullptr, *alt = nullptr;
  switch (t) {
    case T_E: dst = f.E[d]; break;
    case T_D: dst = f.D[d]; break;
    case T_B: dst = f.B[d]; break;
    case T_H:  // H == B until the first H update separates it (PML chunks only)
      dst = f.B[d];
      if (F->h_first_done && f.H[d]) dst = f.H[d], alt = f.B[d];
      break;
  }
  if (!dst) return fail("initialize_field: component not allocated");
  if (k_init_add(dst, alt, F->d_scratch, F->g, f, t, d, F->stream))
    return fail("initialize_field kernel launch failed");
  if (F->nranks > 1) {
    const int kind = t == T_E ? 0 : t == T_D ? 2 : 1;
    if (exchange(F, kind)) return fail("initialize_field halo exchange failed");
  }
  if (wrap(F, t == T_E ? 0 : t == T_D ? 2 : 3)) return -1;
  ISrcDev is{};
  if (t == T_D) {  // update_eh(E_stuff); step_boundaries(E_stuff)
    if (!F->e_first_done && e_lazy_copy(F)) return -1;
    if (nr_defer_begin(F)) return -1;
    if (k_update_e(F->interior, nullptr, F->g, f, is, 0, false, F->stream) ||
        k_update_e(F->interior, &F->shell_list, F->g, f, is, 0, false, F->stream))
      return fail("update E launch failed");
    if (nr_defer_end(F)) return -1;
    if (f.wall_e && k_aniso_wall(F->g, f, 1, F->stream)) return fail("wall E launch failed");
    if (F->nranks > 1 && exchange(F, 0)) return fail("E halo exchange failed");
    if (wrap(F, 0)) return -1;
  } else if (t == T_B) {  // update_eh(H_stuff); step_boundaries(H_stuff)
    if (!F->h_first_done && h_lazy_copy(F)) return -1;
    if (update_h_any(F, F->shell_list, false)) return -1;  // update_eh(H_stuff) only
    if (F->nranks > 1 && exchange(F, 1)) return fail("H halo exchange failed");
    if (wrap(F, 1)) return -1;
  } else {
    F->force_unfused_next = true;  // E (or H) differs from what D (B) implies
  }
  HIPCHK(hipStreamSynchronize(F->stream));
  return 0;
}


// ------------------------------------------------------------------ subpixel averaging
// Quadrature points and weights on the unit sphere for 1-D / 2-D / 3-D, the table
// the reference generates at build time (src/sphere-quad.cpp -> sphere-quad.h):
// 1-D {0,0,+-1}, 2-D 12 points on the circle, 3-D the 50-point degree-11 formula
// (McLaren; Stroud U3:11-1) with octahedral symmetry, each list reordered to
// maximise every point's distance from the earlier ones (squared distances
// compared in single precision, as the generator does).
static void sq_sort(int n, double *x, double *y, double *z, double *w) {
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
static inline void rot3(double &a, double &b, double &c) {
  const double t = c;
  c = b;
  b = a;
  a = t;
}
static void sphere_quad50(double *x, double *y, double *z, double *w) {
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

// the table of one dimensionality: its point count, and the points into xyzw if given
int sphere_quadrature(int dim, double *xyzw) {
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
int set_epsilon_geometry(mnl_structure *s, int device, int nobj, const double *objs,
                         double default_eps, int use_averaging, double tol, int maxeval) {
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

}  // namespace mnlh
