/* meep_nl_amd.h -- C-ABI of the MI355X-native fields::step() hot path.
 *
 * Drop-in boundary for the reference's time-stepping core (PMack10/meep_nl =
 * MIT Meep 1.30 + chi(2) Newton-Raphson fork).  Plain pointers and sizes only;
 * no torch / HIP types.  Each entry cites the reference interface it replaces.
 *
 * Conventions
 *   - components: MNL_EX..MNL_BZ (E, H, D, B x,y,z).  NOT the reference enum
 *     order (src/meep/vec.hpp:31-56 interleaves Er/Ep); bindings map by name.
 *   - grids: dim 1 = Z only (Meep D1), 2 = X,Y (Meep D2), 3 = X,Y,Z.
 *     n[d] cells, resolution a, little corner io[d] in half-pixels
 *     (grid_volume io, src/meep/vec.hpp:1014-1180; io = -n for center_origin).
 *   - host arrays use the reference's per-chunk layout for the whole cell:
 *     (n_d+1) points per present direction, Z fastest, X slowest
 *     (grid_volume::set_strides, src/vec.cpp:482-494).  Entry j of a
 *     component c sits at half-pixel io + 2 j + yee_shift(c).
 *   - every call returns 0 on success, nonzero on error; mnl_last_error()
 *     returns the message ("meep: ..." as meep::abort, src/mympi.cpp:244-262).
 *   - the product path has no CPU fallback: creating fields without a HIP
 *     device fails.
 */
#ifndef MEEP_NL_AMD_H
#define MEEP_NL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MNL_EX = 0, MNL_EY, MNL_EZ, MNL_HX, MNL_HY, MNL_HZ,
  MNL_DX, MNL_DY, MNL_DZ, MNL_BX, MNL_BY, MNL_BZ, MNL_NUM_COMPONENTS
};
/* derived components of array slices (the reference's Dielectric / Permeability,
 * src/meep/vec.hpp:52-53): epsilon / mu on the Centered grid from the diagonal chi1inv */
enum { MNL_DIELECTRIC = 12, MNL_PERMEABILITY = 13 };
enum { MNL_X = 0, MNL_Y = 1, MNL_Z = 2 };
enum { MNL_LOW = 0, MNL_HIGH = 1 };
enum { MNL_SRC_GAUSSIAN = 0, MNL_SRC_CONTINUOUS = 1, MNL_SRC_CUSTOM = 2 };
/* custom_src_time callback: writes the complex dipole f(t) (src/meep.hpp:1059-1092) */
typedef void (*mnl_src_func)(double t, void *data, double *re, double *im);
/* amplitude function A(r) of a volume source: writes A at the position rel
 * (relative to the volume centre; src/sources.cpp:262-271) */
typedef void (*mnl_amp_func)(const double rel[3], void *data, double *re, double *im);

typedef struct mnl_structure mnl_structure;
typedef struct mnl_fields mnl_fields;

/* Thread-local message of the last failing call (meep::abort text). */
const char *mnl_last_error(void);
/* ABI version (major*100+minor). */
int mnl_version(void);
/* Number of visible HIP devices (0 on a host without GPU). */
int mnl_device_count(int *count);

/* ---- structure (replaces meep::structure, src/meep.hpp:809-920) ---------- */

/* structure(grid_volume, eps, boundary_region, symmetry=identity, num_chunks,
 * Courant) -- src/structure.cpp:49-64; grid_volume from vol1d/vol2d/vol3d
 * (src/vec.cpp:904-931).  Vacuum, no PML until set below. */
mnl_structure *mnl_structure_create(int dim, const int n[3], double a, double courant,
                                    const int io[3]);
void mnl_structure_destroy(mnl_structure *s);

/* pml(thickness, d, side, Rasymptotic, mean_stretch) with the quadratic
 * profile -- src/structure.cpp:285-301, applied per chunk by
 * structure_chunk::use_pml (src/structure.cpp:661-691). */
int mnl_structure_add_pml(mnl_structure *s, int dir, int side, double thickness,
                          double R_asymptotic, double mean_stretch);

/* structure_chunk::set_chi1inv row (src/anisotropic_averaging.cpp:211-298)
 * for E component comp (epsilon) or H component comp (mu: structure::set_mu,
 * src/structure.cpp) and direction dir; host array in the layout above
 * (values at every point, ghosts included).  Off-diagonal entries are
 * accepted but only their presence/zeros enter the arithmetic, exactly as in
 * the fork (src/step_generic.cpp:631-633, 730-760; the H update always takes
 * the diagonal branch). NULL resets to trivial. */
int mnl_structure_set_chi1inv(mnl_structure *s, int comp, int dir, const double *host);
/* structure_chunk::set_chi2 / set_chi3 (src/structure.cpp:795-866).  chi3 is
 * inert in the fork (src/step_generic.cpp:829-886) and only recorded. */
int mnl_structure_set_chi2(mnl_structure *s, int comp, const double *host);
int mnl_structure_set_chi3(mnl_structure *s, int comp, const double *host);
/* structure::set_conductivity(c, C) (src/structure.cpp:425-437, chunk part
 * 868-905): conductivity of D or B component comp (an E / H component names
 * its D / B array; E values are multiplied by the diagonal chi1inv set so
 * far, as the reference does).  Enters step_curl's conductivity branches
 * (src/step_generic.cpp:89-229) with cndinv = 1/(1 + cnd dt/2)
 * (src/structure.cpp:693-707) and scales current sources by cndinv
 * (src/step.cpp:300-309).  NULL resets to zero. */
int mnl_structure_set_conductivity(mnl_structure *s, int comp, const double *host);
/* structure::add_susceptibility(sigma, E_stuff, lorentzian_susceptibility(
 * omega0, gamma, drude)) -- src/anisotropic_averaging.cpp:300-372, isotropic
 * (diagonal sigma per E component; NULL = 0). */
int mnl_structure_add_lorentzian(mnl_structure *s, double omega0, double gamma, int drude,
                                 const double *sigma_x, const double *sigma_y,
                                 const double *sigma_z);
/* add_susceptibility with a sigma tensor (src/anisotropic_averaging.cpp:
 * 300-372): sigma[3*c + d] = row of E component c, column d (NULL = 0), at
 * c's Yee points -- the reference samples the off-diagonal entries half a pixel
 * back along c (334-341), the caller does the same.  Off-diagonal entries
 * enter update_P's 2x2 / 3x3 branches (src/susceptibility.cpp:185-250) per
 * reference chunk. */
int mnl_structure_add_lorentzian_tensor(mnl_structure *s, double omega0, double gamma, int drude,
                                        const double *const sigma[9]);
/* structure::add_susceptibility(sigma, H_stuff, lorentzian_susceptibility(omega0,
 * gamma, drude)) (src/anisotropic_averaging.cpp:300-372): a magnetic Lorentzian / Drude
 * susceptibility, diagonal sigma per H component at its Yee points (NULL = 0), updated
 * by update_pols(H_stuff) after update_eh(H_stuff) (src/step.cpp:75-92).  At most 2. */
int mnl_structure_add_magnetic_lorentzian(mnl_structure *s, double omega0, double gamma,
                                          int drude, const double *sigma_x,
                                          const double *sigma_y, const double *sigma_z);
/* Nonlinear E update: 0 = the fork (chi2 through Newton-Raphson where the
 * 3x3 chi1inv is present, chi3 inert; default), 1 = upstream Meep (chi2/chi3
 * through the Pade approximant calc_nonlinear_u, src/step_generic.cpp:546-553,
 * on every E point including PML; diagonal chi1inv only).  Pinned by the
 * reference's python/tests/test_3rd_harm_1d.py golden harmonics. */
int mnl_structure_set_nonlinear_mode(mnl_structure *s, int mode);
/* Fill chi1inv/chi2/Lorentz-sigma of axis-aligned boxes on the device (fast
 * setup for large grids; same values as passing 1/eps(loc) arrays with
 * eps_averaging=False).  box = {xmin,xmax,ymin,ymax,zmin,zmax} in length
 * units; later boxes win.  kind: 0 = epsilon (value = eps), 1 = chi2,
 * 2 = chi3, 3 = Lorentz sigma of susceptibility #index. */
int mnl_structure_set_box(mnl_structure *s, int kind, int index, const double box[6],
                          double value);
/* structure::set_epsilon(material_function &eps, bool use_anisotropic_averaging,
 * double tol, int maxeval) (src/meep.hpp:841, src/structure.cpp:397-401) ->
 * structure_chunk::set_chi1inv (src/anisotropic_averaging.cpp:221-298) with the
 * default material_function::eff_chi1inv_row / normal_vector subpixel averaging
 * (58-219), for a material function given as geometric objects of isotropic
 * permittivity (later objects win, `default_eps` elsewhere), computed on HIP
 * device `device`.  objs: nobj records of MNL_GEO_STRIDE doubles
 * {kind, eps, cx, cy, cz, p0, p1, p2}: kind 0 = block (p = size, |r - c| <= p/2),
 * 1 = sphere (p0 = radius), 2 = cylinder (p0 = radius, p1 = height, p2 = axis
 * 0/1/2).  Coordinates of absent dimensions are 0.  use_averaging = 0 gives
 * 1/eps at each pixel centre (the reference's maxeval = 0 path).  Replaces every
 * chi1inv row of the E components (trivial rows dropped). */
#define MNL_GEO_STRIDE 8
int mnl_structure_set_epsilon_geometry(mnl_structure *s, int device, int nobj,
                                       const double *objs, double default_eps,
                                       int use_averaging, double tol, int maxeval);
/* Copy chi1inv[comp][dir] (whole cell, canonical layout) to host; returns 1
 * (nothing copied) when the row is trivial / absent. */
int mnl_structure_get_chi1inv(mnl_structure *s, int comp, int dir, double *host);
/* The unit-sphere quadrature of src/sphere-quad.cpp (the reference's generated
 * sphere-quad.h) for dim 1/2/3: writes {x, y, z, weight} per point if xyzw is
 * non-null, returns the number of points (2, 12, 50).  Host only. */
int mnl_sphere_quadrature(int dim, double *xyzw);

/* ---- fields (replaces meep::fields, src/meep.hpp:1731-2330) -------------- */

/* fields(structure*) + use_real_fields() (src/fields.cpp:32-89, 144-156) on
 * HIP device `device` (-1 = current).  Real fields only. */
mnl_fields *mnl_fields_create(mnl_structure *s, int device);
/* Distributed variant: one process per GPU, z-slab (3-D) / y-slab (2-D)
 * decomposition of the global grid described by `s` (every rank passes the
 * same global structure).  nccl_id: 128-byte RCCL unique id from rank 0
 * (mnl_comm_unique_id), shared by the caller (e.g. torch.distributed). */
mnl_fields *mnl_fields_create_dist(mnl_structure *s, int device, int rank, int nranks,
                                   const void *nccl_id);
int mnl_comm_unique_id(void *out128);
/* IPC transport id (one process per slab, several processes sharing one GPU --
 * RCCL refuses duplicate devices): creates a POSIX shared-memory control block
 * for `nranks` ranks and writes its 128-byte id; pass it to
 * mnl_fields_create_dist in place of the RCCL id.  Replaces the reference's
 * comms_manager (src/mympi.cpp:87-151) with a process-shared barrier plus
 * IPC-exported device staging buffers. */
int mnl_comm_ipc_id(void *out128, int nranks);
/* Remove the shared-memory name of an IPC id that will not be used (the first
 * init on rank 0 removes it otherwise; mapped segments stay valid). */
int mnl_comm_ipc_unlink(const void *id128);
/* Host-only collective over a fresh IPC group (no GPU call): every rank passes
 * the same id; on return host[0..n) holds the rank-order sum over ranks and the
 * return value is 0 on every rank, or -1 on every rank if any rank passed
 * ok = 0 (the status agreement the data collectives use before they start). */
int mnl_comm_ipc_reduce(const void *id128, int rank, int nranks, double *host, int n, int ok);
/* Transport of a fields object: "single", "rccl", "ipc" or "local". */
const char *mnl_fields_transport(mnl_fields *f);
/* One-rank RCCL self test on `device`: grouped ncclSend/ncclRecv to self of n
 * doubles plus an ncclAllReduce, through the same Comm wrappers the slab
 * exchange uses.  Returns 0 when the data arrived intact. */
int mnl_comm_rccl_selftest(int device, int n);
/* Cells [lo, hi) of the slab axis owned by `rank` (host-only helper). */
int mnl_slab_range(int ncell, int rank, int nranks, int *lo, int *hi);
/* Several slabs of one grid in ONE process on one device (one host thread per
 * slab calling mnl_fields_step concurrently): same decomposition and exchange
 * code as mnl_fields_create_dist, transport = device copies + host barriers.
 * Used to validate the multi-GPU path on a single MI355X. */
void *mnl_local_hub_create(int nranks);
void mnl_local_hub_destroy(void *hub);
mnl_fields *mnl_fields_create_local(mnl_structure *s, int device, int rank, int nranks,
                                    void *hub);
void mnl_fields_destroy(mnl_fields *f);

/* add_volume_source(c, src_time, volume(p,p), amp) for a point p
 * (src/sources.cpp:455-494, weights: src/loop_in_chunks.cpp:263-500).
 * kind GAUSSIAN: params = {freq, width, start_time, end_time} ->
 *   gaussian_src_time(f, w, st, et) (src/sources.cpp:85-96).
 * kind CONTINUOUS: params = {freq_re, freq_im, width, start, end, slowness}
 *   -> continuous_src_time (src/meep.hpp:1038-1056, src/sources.cpp:121-141).
 * is_integrated: dipole (E = eps^-1 (D - P_src)) vs current (D -= J dt)
 * (src/update_eh.cpp:136-146, src/step.cpp:296-319). */
int mnl_fields_add_point_source(mnl_fields *f, int comp, int kind, const double *params,
                                int nparams, const double pos[3], double amp_re, double amp_im,
                                int is_integrated);
/* add_point_source with custom_src_time(func, data, start, end) (src/meep.hpp:
 * 1059-1092; Python CustomSource, python/source.py:338-400): dipole(t) =
 * func(t) for float(t) in [float(start), float(end)], else 0; current = dipole
 * unless is_integrated (then the finite difference of the dipole).  func is
 * called on the host thread that steps the fields. */
int mnl_fields_add_custom_point_source(mnl_fields *f, int comp, mnl_src_func func, void *data,
                                       double start_time, double end_time, const double pos[3],
                                       double amp_re, double amp_im, int is_integrated);
/* fields::add_volume_source(c, src_time, volume(vmin, vmax), A, amp)
 * (src/sources.cpp:455-494, src_vol_chunkloop 243-312): every owned point of
 * component comp's grid in the volume gets the loop_in_chunks weight (linear
 * interpolation at the faces, per reference chunk) times amp times A(r - centre)
 * (afunc NULL: A = 1); zero-width directions scale amp by the resolution (J as
 * a delta function); a volume up to one pixel wider than the cell is clamped,
 * wider fails ("Source width > cell width").  kind / params as
 * mnl_fields_add_point_source (not CUSTOM).  Integrated (dipole) volume sources
 * have no point limit (sorted device arrays, binary search per reader). */
int mnl_fields_add_volume_source(mnl_fields *f, int comp, int kind, const double *params, int np,
                                 const double vmin[3], const double vmax[3], double amp_re,
                                 double amp_im, int is_integrated, mnl_amp_func afunc,
                                 void *adata);
int mnl_fields_add_custom_volume_source(mnl_fields *f, int comp, mnl_src_func func, void *data,
                                        double start_time, double end_time, const double vmin[3],
                                        const double vmax[3], double amp_re, double amp_im,
                                        int is_integrated, mnl_amp_func afunc, void *adata);
/* fields::require_component (src/fields.cpp:566-586). */
int mnl_fields_require_component(mnl_fields *f, int comp);
/* fields::step() x nsteps (src/step.cpp:35-140).  Collective for
 * distributed fields.  NaN/Inf check of the D energy density at the cell
 * centre (src/step.cpp:138-139) every `every` steps, counted across calls (default
 * 100): fails with "meep: simulation fields are NaN or Inf". */
int mnl_fields_step(mnl_fields *f, int nsteps);
/* No reference counterpart (tuning knobs of this implementation).  Times, over real steps:
 * (1) the tile kernel's z-chunk length (automatic, 16, 20, 24, 32, 48: 6 runs; skipped with
 * MNL_FUSED_ZCHUNK set), (2) on one rank, the CUs of the polarization chunks' general kernel
 * running beside the tile kernel (0, and with such chunks up to five splits around the balanced
 * one: up to 6 runs; skipped with MNL_TILE_GEN_CUS set), and keeps the fastest; with temporal
 * blocking also (3) the two-step items' planes and width: 124 columns
 * with automatic, 12, 16, 20, 24, 32, 40, 48, 64, 96, 128 planes and 60 columns with automatic,
 * 12, 16, 20, 24, 32, 40, 48 planes (19 candidates, swept forward and backward: 38 runs; the
 * three best again with 2 * reps timed steps), and (4) pairs vs one-step stepping (one run,
 * and one with 2 * reps timed steps).  A run is two warm-up steps and r timed ones, r = reps
 * rounded up to even.  Advances the fields by at most 2 + 51 * (2 + r) + 4 * (2 + 2 * reps)
 * steps (112 + 59 * reps for even reps), with results identical to plain stepping.  *zchunk = the length kept (0 = automatic), *gen_cus = the
 * CUs kept (0 = one launch after the other); -1 = not tuned (not in the fused mode:
 * at most 2 steps taken). */
int mnl_fields_tune(mnl_fields *f, int reps, int *zchunk, int *gen_cus);
int mnl_fields_set_nan_check(mnl_fields *f, int every);
/* Field energy over the box [vmin, vmax] (NULL, NULL: the whole cell,
 * user_volume.surroundings()), src/energy_and_flux.cpp:48-178:
 * which 0 = electric_energy_in_box (sum over E comps of 1/2 integral E.D),
 * 1 = magnetic_energy_in_box (1/2 integral H.B with the current B, H),
 * 2 = field_energy_in_box (electric + magnetic of B, H synchronized to E's
 * time: one extra B half step averaged in and restored).  Integration on each
 * component's Yee grid with loop_in_chunks weights; device reduction
 * (compensated), per reference chunk.  Collective. */
int mnl_fields_energy_in_box(mnl_fields *f, int which, const double vmin[3], const double vmax[3],
                             double *out);
/* fields::initialize_field(c, func) (src/initialize.cpp:135-161) with the
 * function evaluated by the caller: host = real part of func at every point of
 * component c in the whole-cell layout (n >= cell size).  Adds it to the
 * field, zeroes the metallic walls, exchanges ghosts; for D / B components also
 * updates E / H from them, as the reference does.  Collective. */
int mnl_fields_initialize_field(mnl_fields *f, int comp, const double *host, size_t n);
/* t (timesteps) and dt; time() = t*dt, round_time() = float(t*dt)
 * (src/meep.hpp:1891-1892). */
int mnl_fields_time(mnl_fields *f, long long *t, double *dt);
/* fields::t = t (the Python binding's fields.t assignment, python/simulation.py
 * restart_fields). */
int mnl_fields_set_time(mnl_fields *f, long long t);
/* fields::zero_fields (src/fields.cpp:638-664): all field / auxiliary arrays and the
 * polarizations to 0 (DFT accumulators kept). */
int mnl_fields_zero_fields(mnl_fields *f);
/* fields::remove_sources (src/fields.cpp:601-610). */
int mnl_fields_remove_sources(mnl_fields *f);
/* fields::get_field(c, vec) with 8-point interpolation
 * (src/monitor.cpp:127-160, src/vec.cpp:558-621).  Distributed: every rank
 * returns the global value (sum over ranks, as get_field(..., parallel=true)). */
int mnl_fields_get_field(mnl_fields *f, int comp, const double pos[3], double *out);
/* Copy the whole-cell array of a component (layout above, ghosts = 0 as in
 * the reference) into a caller-owned buffer of n doubles; H components read
 * B where H==B (src/fields.cpp:493-517).  Distributed: only rank-owned planes
 * are filled, the rest is 0 (sum over ranks gives the global array). */
int mnl_fields_copy_component(mnl_fields *f, int comp, double *host, size_t n);
/* fields::get_array_slice(volume, c) (src/array_slice.cpp:611-704, with
 * comp = MNL_DIELECTRIC / MNL_PERMEABILITY: src/array_slice.cpp:385-408, the
 * Dielectric / Permeability slices of Simulation.get_epsilon / get_mu;
 * get_array_slice_dimensions 447-507): the component on the Centered grid
 * points of the volume [vmin, vmax] (average of its Yee neighbours), empty
 * dimensions interpolated and collapsed (snap = 0) or snapped to the
 * nearest grid point (snap = 1, src/loop_in_chunks.cpp:275-287).  *rank / dims[3]: the
 * kept directions in X,Y,Z order; out (nout doubles, row-major) may be NULL to
 * query the size.  Collective for distributed fields (every rank gets the
 * whole slice). */
int mnl_fields_array_slice(mnl_fields *f, int comp, const double vmin[3], const double vmax[3],
                           int snap, int *rank, long long dims[3], double *out, long long nout);
/* Number of entries of the whole-cell array of comp. */
size_t mnl_fields_ntot(mnl_fields *f);
/* Per-sub-step GPU time in ms accumulated since creation (time_sink
 * FieldUpdateB/H/D/E, BoundarySteppingB/H, src/meep.hpp:1610-1633);
 * out[6]. */
int mnl_fields_timers(mnl_fields *f, double out[6]);
/* Time sinks in the reference's enum order (meep::time_sink,
 * src/meep.hpp:1610-1633; print_times labels src/time.cpp:28-51). */
enum {
  MNL_SINK_CONNECTING, MNL_SINK_STEPPING, MNL_SINK_BOUNDARIES, MNL_SINK_MPI_ALL,
  MNL_SINK_MPI_ONE, MNL_SINK_FIELD_OUTPUT, MNL_SINK_FOURIER, MNL_SINK_MPB,
  MNL_SINK_FARFIELDS, MNL_SINK_OTHER, MNL_SINK_UPDATE_B, MNL_SINK_UPDATE_H,
  MNL_SINK_UPDATE_D, MNL_SINK_UPDATE_E, MNL_SINK_BSTEP_B, MNL_SINK_BSTEP_WH,
  MNL_SINK_BSTEP_PH, MNL_SINK_BSTEP_H, MNL_SINK_BSTEP_D, MNL_SINK_BSTEP_WE,
  MNL_SINK_BSTEP_PE, MNL_SINK_BSTEP_E, MNL_NUM_TIME_SINKS
};
/* fields::get_time_spent_on for every sink of this rank, seconds (replaces
 * src/time.cpp:136-139 / timing_data_vector): wall time of mnl_fields_step
 * goes to "time stepping" except, with profiling on, the GPU time of the
 * unfused update kernels (B/H/D/E), halo exchanges ("copying boundaries")
 * and DFT updates ("Fourier transforming"); collectives of slices / energies
 * / fluxes / get_field to "all-all communication".  out[MNL_NUM_TIME_SINKS]. */
int mnl_fields_time_spent(mnl_fields *f, double *out);
/* fields::reset_timers (src/time.cpp:124-128). */
int mnl_fields_reset_timers(mnl_fields *f);
/* sum_to_all over the ranks of distributed fields (in place, n doubles);
 * a no-op on one rank.  Collective. */
int mnl_fields_allreduce(mnl_fields *f, double *v, int n);
/* meep::verbosity (default 1).  At > 0 rank 0 prints "on time step N
 * (time=T), S s/step" at most every 4 s of stepping (src/step.cpp:49-56). */
void mnl_set_verbosity(int level);
int mnl_get_verbosity(void);
/* Newton-Raphson attempts that fell back to random seeds (never in the
 * reference runs recorded in SURVEY.md; counted instead of printed). */
int mnl_fields_nr_fallbacks(mnl_fields *f, long long *count);
/* Algorithmic bytes per owned cell per step of this configuration
 * (DESIGN.md "Roofline") and owned cells of this rank. */
int mnl_fields_traffic_model(mnl_fields *f, double *bytes_per_cell_step, double *owned_cells);
/* fields::use_bloch(d, k) (src/fields.cpp:75-90) for k = 0: both boundaries of direction dir
 * (0 X, 1 Y, 2 Z) become Periodic.  No metal on those faces; each not-owned point is connected
 * to the owned point one lattice vector away with phase 1 (connect_the_chunks,
 * src/boundaries.cpp:347-623), and the ghost planes are copied on the device after the E and
 * the H updates.  The fields stay real.  Accepted only before sources,
 * DFT monitors and the first step.  Fails with a "meep: ..." message for k != 0 on real fields
 * (it needs complex fields: mnl_fields_use_complex_fields first), a PML on either side of the
 * direction, a 1-D cell, a direction the cell does not have, the slab direction of fields on more than one rank, and (PML along two
 * directions only) anisotropic susceptibilities or Newton-Raphson / off-diagonal chi1inv with a
 * susceptibility.  One rank steps periodic
 * 3-D runs in the fused mode like any other run (the top plane of each periodic direction as
 * shell boxes); pairs of steps, and the fused mode on several ranks, are declined. */
int mnl_fields_use_bloch(mnl_fields *f, int dir, double k_re, double k_im);
/* Complex fields: the inverse of fields::use_real_fields
 * (src/fields.cpp:140-160).  Fields are real when created (a project default: meep::fields are
 * complex until use_real_fields is called).  After this call the fields hold a second set of
 * every time-stepped array (part 1, the imaginary part), stepped by the same kernels;
 * mnl_fields_use_bloch then takes any complex k (in units of 2 pi, as fields::use_bloch,
 * src/boundaries.cpp:88-103), and the ghost planes are multiplied by the Bloch phase on the
 * device.  Sources add real(A J) to part 0 and imag(A J) to part 1 (src/step.cpp:300-315).
 * Accepted only before use_bloch, sources, monitors, initialize_field and the first step, in
 * 2-D and 3-D cells; on several ranks (every rank makes the call) the two parts' halo planes
 * travel in one exchange group and the steps run unfused.  Fails with a "meep: ..." message for chi(2) / chi(3) media,
 * off-diagonal chi1inv and anisotropic susceptibilities.  DFT flux and dft_fields objects
 * accumulate phase * (f_re + i f_im) per update (src/dft.cpp:295-299), an image chunk's Bloch
 * phase folded into its scale; near2far, energy and force objects, probes, dft_norm,
 * checkpoints (dump / load), the tuner and pairs of steps are refused or inactive. */
int mnl_fields_use_complex_fields(mnl_fields *f);
/* fields::is_real (src/meep.hpp): *out = 1 for real fields, 0 after use_complex_fields */
int mnl_fields_is_real(mnl_fields *f, int *out);
/* fields::get_field(c, loc) (src/monitor.cpp:115-160) as a complex number (out[0] real, out[1]
 * imaginary; 0 on real fields).  mnl_fields_get_field returns the real part. */
int mnl_fields_get_field_complex(mnl_fields *f, int comp, const double pos[3], double out[2]);
/* mnl_fields_copy_component / mnl_fields_array_slice of one part (0 real, 1 imaginary; part 1
 * fails on real fields): fields_chunk::f[c][cmp] (src/meep.hpp) */
int mnl_fields_copy_component_part(mnl_fields *f, int part, int comp, double *host, size_t n);
int mnl_fields_array_slice_part(mnl_fields *f, int part, int comp, const double vmin[3],
                                const double vmax[3], int snap, int *rank, long long dims[3],
                                double *out, long long nout);
/* fields::initialize_field with a complex function (src/initialize.cpp:135-160): re is added to
 * part 0 and im (NULL: 0) to part 1.  Complex fields only. */
int mnl_fields_initialize_field_complex(mnl_fields *f, int comp, const double *re,
                                        const double *im, size_t n);
/* boundary_condition of one side (0 low, 1 high) of a direction (src/meep.hpp: Periodic = 0,
 * Metallic = 1); fails for a direction the cell does not have. */
enum { MNL_BOUNDARY_PERIODIC = 0, MNL_BOUNDARY_METALLIC = 1 };
int mnl_fields_boundary(mnl_fields *f, int dir, int side, int *kind);
/* Allow (1, default) or forbid (0) the fused single-pass interior kernel
 * (used automatically for 3-D non-dispersive, non-NR configurations without
 * magnetic or integrated sources).  Results are identical either way. */
int mnl_fields_set_fused(mnl_fields *f, int allow);
/* How the last step ran and how the fields are allocated: *fused = an OR of these bits. */
enum {
  MNL_MODE_FUSED = 1,       /* the last step ran the fused interior kernel */
  MNL_MODE_PALETTE = 2,     /* it read chi1inv through the palette (DESIGN.md "chi1inv palette") */
  MNL_MODE_CONTIG = 4,      /* field arrays are requested physically contiguous (MNL_CONTIG) */
  MNL_MODE_TILE = 16,       /* it ran as the single tile kernel (lean + PML bodies, DESIGN.md
                               section 5), the only fused step there is: set whenever FUSED is */
  MNL_MODE_CONCURRENT = 32, /* the polarization chunks' general kernel ran beside the tile kernel
                               on a CU split: MNL_KSTAT_TILE then spans both launches */
  MNL_MODE_FALLBACKS_SHIFT = 8 /* bits 8-15: contiguity requests the driver could not satisfy
                                  (plain allocations instead), at most 255 */
};
int mnl_fields_mode(mnl_fields *f, int *fused);
/* Enable HIP-event timing around every sub-step kernel group (on the stream
 * the kernels run on) and reset the accumulated timers. */
int mnl_fields_set_profiling(mnl_fields *f, int on);
/* Accumulated launches / total ms of one kernel group since the last
 * mnl_fields_set_profiling, and its algorithmic bytes per launch (0 where the group is not
 * HBM-bound or has no model).  which = one of: */
enum {
  MNL_KSTAT_TILE = 0,       /* the tile kernel (fused mode) or curl B = step_db(B_stuff) */
  MNL_KSTAT_CURL_D = 1,     /* curl D = step_db(D_stuff) (unfused mode) */
  MNL_KSTAT_GENERAL = 2,    /* the general fused kernel (the polarization chunks) */
  MNL_KSTAT_DFT = 3,        /* the DFT updates of one step (all DFT objects) */
  MNL_KSTAT_E_UPDATE = 4,   /* update_eh(E_stuff): chi(2) Newton-Raphson, Lorentzian P; unfused */
  MNL_KSTAT_PAIRS = 5,      /* temporal blocking: launches = pairs of
                               steps, total_ms = every launch of the pairs, bytes per pair */
  MNL_KSTAT_RIM = 6,        /* the rim launches of the pairs, one step each */
  MNL_KSTAT_CHAIN = 7,      /* multi-rank pairs: the slab-face chains on the comm stream */
  MNL_KSTAT_GHOST_WAIT = 8, /* multi-rank pairs: the main stream waiting for a chain's E ghost */
  MNL_KSTAT_N2F_FAR = 9,    /* near2far: the far-field kernel (mnl_fields_near2far_farfields) */
  MNL_KSTAT_N2F_REDUCE = 10, /* near2far: the reduce kernel of the far-field transform */
  /* the kernels of the DFT data calls: always timed, bytes of the last launch */
  MNL_KSTAT_DFT_GET = 11,   /* the gather kernel of mnl_fields_dft_get */
  MNL_KSTAT_DFT_LOAD = 12,  /* the scatter kernel of mnl_fields_dft_load */
  MNL_KSTAT_DFT_SCALE = 13, /* the scale kernel of mnl_fields_dft_scale */
  MNL_NUM_KSTATS = 14
};
int mnl_fields_kernel_stats(mnl_fields *f, int which, long long *launches, double *total_ms,
                            double *bytes_per_launch);
/* Temporal blocking (no reference counterpart: how this build steps pairs of
 * fields::step(), src/step.cpp:35-140): the first n of these slots
 * of the current fused geometry go to out[0..n). */
enum {
  MNL_TBINFO_ACTIVE = 0,          /* 1: the last call of >= 2 steps stepped in pairs */
  MNL_TBINFO_TB_CELLS = 1,        /* own cells of the two-step items */
  MNL_TBINFO_TB_BORDER = 2,       /* their border points (upper bound) */
  MNL_TBINFO_TB_CELLS_MIXED = 3,  /* own cells of the mixed-palette two-step items */
  MNL_TBINFO_RIM_CELLS = 4,       /* rim cells */
  MNL_TBINFO_RIM_CELLS_MIXED = 5, /* cells of the mixed-palette rim items */
  MNL_TBINFO_TB_ITEMS = 6,        /* two-step items */
  MNL_TBINFO_RIM_ITEMS = 7,       /* rim items */
  MNL_TBINFO_TB_PLANES = 8,       /* planes of the first two-step item (the longest) */
  MNL_TBINFO_NARROW_ITEMS = 9,    /* narrow x-face strip items among the rim items */
  MNL_TBINFO_ENABLED = 10,        /* pairs allowed: set_temporal_blocking / MNL_TB / the tuner */
  MNL_TBINFO_TB_ZCHUNK = 11,      /* the two-step chunk setting (0: automatic) */
  MNL_TBINFO_TB_WIDTH = 12,       /* most own columns of a two-step item (124 unless set / tuned) */
  MNL_TBINFO_TB_POL = 13,         /* 1: polarization chunks stepped inside the pairs */
  MNL_NUM_TBINFO = 14
};
int mnl_fields_tb_info(mnl_fields *f, double *out, int n);
/* Allow (1, the default; MNL_TB=0 at creation turns it off) or forbid (0) stepping
 * pairs of steps with the two-step kernel.  Results are identical either way. */
int mnl_fields_set_temporal_blocking(mnl_fields *f, int on);
/* Scheduling options of the fused step (no reference counterpart; an option only changes how
 * the same per-point arithmetic is scheduled, results are identical).  For in-process A/B
 * measurements (tools/ab_inproc.py).  A switch takes value 0 / non-zero (all default to 1), the
 * others a count in the range given; every option but RES, RES_TB2, RES_RIM and SRC_GUARD has
 * the pair plan rebuilt at the next step.  10, 13, 14 and 15 are retired (variants measured
 * slower or no better and since removed): they fail like any unknown
 * number. */
enum {
  MNL_SCHED_NARROW = 0,     /* switch: the narrow x-face strip body of the pairs' rim
                               (MNL_TB_NARROW) */
  MNL_SCHED_DFT_PAL = 1,    /* switch: DFT sampling plans carry chi1inv as palette bytes (the
                               plans are rebuilt at the next update) */
  MNL_SCHED_RES = 2,        /* CUs the pair launches leave free (-1 the default .. 1024) */
  MNL_SCHED_RES_TB2 = 3,    /* the same for the two-step launch only */
  MNL_SCHED_RES_RIM = 4,    /* the same for the rim launches only */
  MNL_SCHED_DFT_CMP = 5,    /* switch: pairs sample DFT monitors from the two-step kernel's
                               compact boxes (MNL_DFT_CMP) */
  MNL_SCHED_RIM_ZCHUNK = 6, /* planes per rim item of a pair (0 = the one-step chunk .. 64) */
  MNL_SCHED_NR_EARLY = 7,   /* switch: the chi(2) NR box's E phase beside the tile kernel
                               (MNL_NR_EARLY) */
  MNL_SCHED_TB_ZCHUNK = 8,  /* planes per two-step item (0 = automatic .. 4096; MNL_TB_ZCHUNK) */
  MNL_SCHED_TB_OX = 9,      /* most own columns of a two-step item (4 .. 124; 0 = 124, the widest
                               the kernel's 128 columns of lanes hold); the tuner keeps a width
                               that was set */
  MNL_SCHED_TB_POL = 11,    /* switch: pairs of steps with polarization chunks */
  MNL_SCHED_R1_BESIDE = 12, /* switch: the first rim launch's items other than the narrow x-face
                               strips on a side stream beside the two-step kernel (one rank) */
  MNL_SCHED_SRC_GUARD = 16  /* switch: a pair's step sources and NaN guard in one launch (one
                               rank) */
};
int mnl_fields_set_schedule(mnl_fields *f, int which, int value);

/* ---- checkpoint (src/fields_dump.cpp, src/structure_dump.cpp) -----------
 * fields::dump / fields::load (src/fields_dump.cpp:108-145, 232-270): t and
 * every per-point state array of the rank (f, f_u, f_w, f_cond, and also the
 * polarizations and DFT accumulators), flat binary, not HDF5 (no HDF5 in this
 * build).  Distributed fields write one file per rank (filename.rank<r>).
 * load() needs fields built the same way (same structure, decomposition,
 * sources, flux objects) and resumes bit for bit.  structure dump/load
 * (structure::dump / load, src/structure_dump.cpp) save the host-side
 * material description; load before creating fields. */
int mnl_fields_dump(mnl_fields *f, const char *filename);
int mnl_fields_load(mnl_fields *f, const char *filename);
int mnl_structure_dump(mnl_structure *s, const char *filename);
int mnl_structure_load(mnl_structure *s, const char *filename);

/* ---- DFT flux (src/dft.cpp; meep.hpp dft_flux) --------------------------
 * fields::add_dft_flux (src/dft.cpp:578-640) for a volume_list: regions =
 * nreg x {min x,y,z, max x,y,z, direction (0..2), weight}, nfreq frequencies
 * (not angular), decimation 0 = the reference's automatic choice
 * (src/dft.cpp:195-216).  The DFT is accumulated on the device after every
 * decimated step (fields::update_dfts, src/dft.cpp:249-263); *handle gets the
 * flux object's index. */
int mnl_fields_add_dft_flux(mnl_fields *f, int nreg, const double *regions, const double *freqs,
                            int nfreq, int decimation, int *handle);
/* dft_flux::flux (src/dft.cpp:533-547), summed over ranks: out[nfreq]. */
int mnl_fields_dft_flux(mnl_fields *f, int handle, double *out);
/* Complex DFT values per list (which 0: E, 1: H), list order (next_in_dft),
 * point-major then frequency, re/im interleaved: *n = points * nfreq. */
int mnl_fields_dft_size(mnl_fields *f, int handle, long long *n);
/* out[2 * n]; points another rank owns read 0 (sum over ranks to assemble). */
int mnl_fields_dft_data(mnl_fields *f, int handle, int which, double *out, long long n);
/* the decimation factor the object was created with */
int mnl_fields_dft_decimation(mnl_fields *f, int handle, int *decimation);
/* ---- DFT data of any DFT object (flux, dft-fields, near2far handles) ------
 * The accumulated values of one chunk list (which 0: E, 1: H; dft-fields and near2far objects
 * keep every chunk in list 0) in list order, [point][freq] complex, n complex values.  A rank
 * holds the points it owns: get returns 0 for the others, load takes the full list and ignores
 * them, so the full list is the sum over the ranks and data of a run on one GPU loads into a
 * run on several.  Buffered updates are accumulated first.
 *
 * mnl_fields_dft_get: the array save_dft_hdf5 writes (src/dft.cpp:444-466; Python
 * get_dft_data / get_flux_data / get_near2far_data, python/simulation.py:3067-3071, 3297,
 * 3563), gathered on the device and copied for this list only; the same values as
 * mnl_fields_dft_data.  n >= mnl_fields_dft_size. */
int mnl_fields_dft_get(mnl_fields *f, int handle, int which, double *out, long long n);
/* load_dft_hdf5 (src/dft.cpp:468-496; Python load_flux_data / load_minus_flux_data /
 * load_near2far_data, python/simulation.py:3305-3355, 3575-3635): the list's values become
 * sign * in, sign = +-1 (-1: load followed by scale_dfts(-1) in one pass).  n must equal
 * mnl_fields_dft_size: "incorrect dataset size (%zd vs. %zd) in load_dft..." otherwise. */
int mnl_fields_dft_load(mnl_fields *f, int handle, int which, const double *in, long long n,
                        int sign);
/* dft_flux::scale_dfts / dft_fields::scale_dfts / dft_near2far::scale_dfts (src/dft.cpp:573-576,
 * 879; dft_chunk::scale_dft 401-405; Python scale_flux_fields / scale_near2far_fields,
 * python/simulation.py:5997, 6058): every value of every list times re + i im. */
int mnl_fields_dft_scale(mnl_fields *f, int handle, double re, double im);
/* dft_flux::save_hdf5 / load_hdf5, dft_near2far::save_hdf5 / load_hdf5 (Python save_flux /
 * load_flux / load_minus_flux, save_near2far / ...): a flat binary file (no HDF5 here) with a
 * magic, the number of lists, nfreq, the frequencies, the points per list and the lists in
 * list order.  Collective on several ranks: rank 0 writes the assembled lists, every rank
 * reads the file.  Loading checks the magic, nfreq and the sizes, not the frequencies. */
int mnl_fields_dft_save(mnl_fields *f, int handle, const char *filename);
int mnl_fields_dft_load_file(mnl_fields *f, int handle, const char *filename, int sign);
/* ---- Field probes: fields::get_field(c, pt) (src/monitor.cpp:127-160) after every step ------
 * A probe records, on the device and inside whatever stepping mode is active, the value
 * mnl_fields_get_field(comp, pos) would return after each step: the same interpolation points
 * and weights, the same per-point value rule, added in the same order (bitwise, except that a
 * -0.0 may read +0.0).  It is sampled with the DFT monitors, so steps are
 * never split by it.  *handle is a probe handle (not a DFT handle: the DFT data calls refuse it,
 * and adding a probe moves no DFT handle).  A probe of a component that has no array yet
 * records 0.  Probes are not part of mnl_fields_dump; after mnl_fields_load or
 * mnl_fields_set_time a probe is empty at the new step. */
int mnl_fields_add_probe(mnl_fields *f, int comp, const double pos[3], int *handle);
/* The values since the last read (or since the probe was added / reset), oldest first:
 * *count values, the first one that of step *t_first (the state after *t_first steps).  The
 * series holds the last 65536 steps (MNL_PROBE_CAP when the probe is added); older values are
 * dropped, which *t_first shows.  values == NULL: only *count and *t_first, nothing is
 * consumed; otherwise values[cap] with cap >= *count, and the series is emptied.  Buffered
 * samples are flushed first.  Distributed: collective, every rank gets the sum over the ranks
 * of their partial sums (fields::get_field(..., parallel = true)). */
int mnl_fields_probe_read(mnl_fields *f, int handle, long long cap, long long *count,
                          long long *t_first, double *values);
/* Empty a probe's series / remove one probe (the other probes keep their handles) / remove
 * every probe (their handles become invalid). */
int mnl_fields_probe_reset(mnl_fields *f, int handle);
int mnl_fields_remove_probe(mnl_fields *f, int handle);
int mnl_fields_remove_probes(mnl_fields *f);
/* ---- LDOS spectra: dft_ldos (src/dft_ldos.cpp) ------------------------------------------------
 * The power spectrum of the sources normalised to the local density of states.  An update sums
 * E conj(A) over the points of every electric source volume and H conj(A) over those of every
 * magnetic one (A: the source's amplitude at the point), Fourier-transforms the two sums and
 * the current of the first source; the sums run on the device inside whatever stepping mode is
 * active.  The point lists follow the sources: when sources are added,
 * removed or changed, what is buffered is accumulated with the old lists first.  Real fields
 * only.  LDOS objects are not DFT objects: they have their own handles and do not enter
 * mnl_fields_dft_norm / dft_maxfreq / max_decimation or mnl_fields_dump; after mnl_fields_load
 * or mnl_fields_set_time the updates still buffered are dropped.
 * mnl_fields_add_ldos replaces dft_ldos::dft_ldos(freq, Nfreq). */
int mnl_fields_add_ldos(mnl_fields *f, const double *freqs, int nfreq, int *handle);
/* Replaces dft_ldos::update(fields&): one update of the current state. */
int mnl_fields_ldos_update(mnl_fields *f, int handle);
/* on != 0: from now on every step appends the update of the state after it (what calling
 * mnl_fields_ldos_update after every single step does, without leaving the batch); on == 0:
 * no longer.  Updates are buffered and accumulated in blocks; every reader accumulates first. */
int mnl_fields_ldos_record(mnl_fields *f, int handle, int on);
/* Replaces dft_ldos::ldos() / F() / J() / overall_scale() (src/dft_ldos.cpp:60-95): ldos[nfreq],
 * F[2 nfreq] and J[2 nfreq] as (re, im), *overall_scale; any output may be NULL.  Before the
 * first update ldos is NaN, as the reference's.  Distributed: collective; F is summed over the
 * ranks and the formula applied to the sum. */
int mnl_fields_ldos_data(mnl_fields *f, int handle, double *ldos, double *F, double *J,
                         double *overall_scale);
/* Diagnostic (as mnl_fields_dft_points): the global point list in list order, the electric
 * sources' points, then the magnetic ones'.  *n points; with comp / ijk / amp given (each may be
 * NULL) and cap >= *n: the field component sampled, the point's 3 global indices on that
 * component's grid, the amplitude A as (re, im). */
int mnl_fields_ldos_points(mnl_fields *f, int handle, long long cap, long long *n, int *comp,
                           int *ijk, double *amp);
/* Remove one LDOS object (the others keep their handles) / every one; buffered updates are
 * dropped with it. */
int mnl_fields_remove_ldos(mnl_fields *f, int handle);
int mnl_fields_remove_ldoses(mnl_fields *f);
/* Replaces fields::get_eigenmode_coefficients(flux, eig_vol, ..., dp) (src/mpb.cpp:925-1004) for
 * DiffractedPlanewave modes (get_eigenmode with dp != NULL, src/mpb.cpp:342-347, 619-664: an
 * analytic plane wave, no eigensolver).  handle: a flux object with one region.  Per mode m:
 * g[3 m ..] the diffraction order, axis[3 m ..] (axis NULL or all 0: the first direction lying in
 * the plane of the monitor), sp[4 m ..] = s (re, im), p (re, im).  eig_vol: (min[3], max[3]) of
 * the eigenmode volume, NULL = the flux region; kpoint[3], NULL = 0.  Outputs per (mode,
 * frequency): coeffs[nmodes][nfreq][2] complex (forward, backward), vgrp, kpoints[..][3], cscale
 * (each may be NULL but coeffs), and overlaps[nmodes][nfreq][8] complex (may be NULL): the four
 * mode-flux sums of fields::get_overlap (src/dft.cpp:1377-1427: ExHy, EyHx, HyEx, HxEy for a z
 * normal) and the four mode-mode sums.  The sums are taken on the device from the DFT array
 * (buffered updates are accumulated first) in a fixed order and summed over the ranks
 * (collective).  Evanescent orders give 0 everywhere, as src/mpb.cpp:957-962. */
int mnl_fields_mode_coefficients(mnl_fields *f, int handle, int nmodes, const int *g,
                                 const double *axis, const double *sp, const double *eig_vol,
                                 const double *kpoint, double *coeffs, double *vgrp,
                                 double *kpoints, double *cscale, double *overlaps);
/* Diagnostic: the host table the call above hands to the device (arguments as there).
 * dims[4] = na, nb (entries of the two in-plane phase tables), the number of normal layers, and
 * 4 * da + db (the in-plane directions; db = 3: none).  Every other output may be NULL:
 * coords[na + nb + 2] the integer half-pixel coordinates of the table entries and of the two
 * layers; k[nmodes][nfreq][3]; vgrp[nmodes][nfreq]; amp[nmodes][nfreq][6] complex (Ex .. Hz);
 * pa[nmodes][na], pb[nmodes][nb], pl[nmodes][nfreq][2] complex: exp(2 pi i k_d (x_d - centre_d))
 * along the two in-plane directions and the normal. */
int mnl_fields_mode_table(mnl_fields *f, int handle, int nmodes, const int *g, const double *axis,
                          const double *sp, const double *eig_vol, const double *kpoint,
                          long long *dims, int *coords, double *k, double *vgrp, double *amp,
                          double *pa, double *pb, double *pl);
/* fields::dft_norm() (src/dft.cpp:312-361): the square root of the sum of |dft|^2 over every
 * frequency and point of every chunk list of every DFT object (flux, fields, near2far, energy,
 * force; not probes), reduced on the device in a fixed order and summed over the ranks
 * (collective).  Buffered updates are accumulated first. */
int mnl_fields_dft_norm(mnl_fields *f, double *norm);
/* fields::dft_maxfreq() (src/dft.cpp:380-399): the largest |omega| / 2 pi of any DFT object, 0
 * without any.  fields::max_decimation() (src/dft.cpp:365-377): the largest decimation factor
 * in use, at least 1.  Host only. */
int mnl_fields_dft_maxfreq(mnl_fields *f, double *maxfreq);
int mnl_fields_max_decimation(mnl_fields *f, int *decimation);
/* Accumulate every buffered DFT update now and wait for the device (no reference
 * counterpart: the reference adds each update to the DFT array in fields::update_dfts,
 * src/dft.cpp:249-263; this build samples every update and adds up to 32 of them per pass
 * over the array, in the same order, so the values are bitwise the same).  Every reader of
 * DFT values (flux, data, get_dft_array, dump) flushes by itself; buffered updates carry over
 * between step calls.  For timing: a timed region that includes the accumulation of its own
 * updates ends with this call. */
int mnl_fields_dft_flush(mnl_fields *f);
/* fields::add_dft_fields(components, ncomp, volume(vmin, vmax), freq, Nfreq,
 * use_centered_grid = !yee_grid, decimation_factor) (src/dft.cpp:889-903; Python
 * Simulation.add_dft_fields, python/simulation.py:2976-3036): any field components
 * (MNL_EX..MNL_BZ; D and B sample the D and B arrays themselves), accumulated on the device with the flux objects' kernels.
 * *handle is shared with the flux handles (mnl_fields_dft_data, _decimation). */
int mnl_fields_add_dft_fields(mnl_fields *f, int ncomp, const int *comps, const double vmin[3],
                              const double vmax[3], const double *freqs, int nfreq, int yee_grid,
                              int decimation, int *handle);
/* fields::get_dft_array(dft_fields or dft_flux, c, num_freq) (src/dft.cpp:1240-1280,
 * process_dft_component 908-1240, collapse_array src/array_slice.cpp:554-601): the
 * complex DFT of component comp at frequency index num_freq over the object's volume,
 * empty dimensions collapsed, summed over ranks.  *rank and dims[0..rank-1] (row-major,
 * X before Y before Z); out (2*nout doubles, re/im interleaved) may be NULL to query the
 * size.  rank 0 means the object holds no chunk of comp (no values). */
int mnl_fields_dft_array(mnl_fields *f, int handle, int comp, int num_freq, int *rank,
                         long long dims[3], double *out, long long nout);

/* ---- DFT energy and force monitors (src/dft.cpp:630-790, src/stress.cpp) ----
 * Objects of up to four chunk lists, accumulated like every other DFT object's; the handle is
 * shared with the other DFT handles.  `which` of mnl_fields_dft_data / _dft_get / _dft_load /
 * _dft_points / _dft_list_size and the order of the lists in a mnl_fields_dft_save file:
 * 0..3 = E, H, D, B for an energy object, 0..2 = offdiag1, offdiag2, diag for a force object.
 * mnl_fields_dft_array refuses both kinds.
 *
 * fields::add_dft_energy (src/dft.cpp:701-727; Python Simulation.add_energy,
 * python/simulation.py:3357-3400): regions as for mnl_fields_add_dft_flux; direction and
 * weight are ignored, as in the reference. */
int mnl_fields_add_dft_energy(mnl_fields *f, int nreg, const double *regions, const double *freqs,
                              int nfreq, int decimation, int *handle);
/* fields::add_dft_force (src/stress.cpp:153-191; Python Simulation.add_force,
 * python/simulation.py:3109-3150): regions as for mnl_fields_add_dft_flux with direction = the
 * force direction; the normal is that of the region ("cannot determine dft_force normal" for a
 * region that is not a surface of the cell's dimension). */
int mnl_fields_add_dft_force(mnl_fields *f, int nreg, const double *regions, const double *freqs,
                             int nfreq, int decimation, int *handle);
/* dft_energy::electric / magnetic / total (src/dft.cpp:657-699): which 0 electric, 1 magnetic,
 * 2 total = electric + magnetic per frequency.  Summed on the device (no atomics: two calls
 * return the same bits) and over ranks: out[nfreq]. */
int mnl_fields_dft_energy(mnl_fields *f, int handle, int which, double *out);
/* dft_force::force (src/stress.cpp:90-114), summed on the device and over ranks: out[nfreq]. */
int mnl_fields_dft_force(mnl_fields *f, int handle, double *out);
/* Per point of list `which` of any DFT object, in list order: x, y, z of the DFT point, the
 * component, and the loop weight as dft_chunk::update_dft applies it (src/dft.cpp:277-282:
 * after the square root; 1.0 for unweighted lists).  out[5 * n], n >= the list's points. */
int mnl_fields_dft_points(mnl_fields *f, int handle, int which, double *out, long long n);
/* Complex values of list `which` (points x nfreq); mnl_fields_dft_size is list 0's. */
int mnl_fields_dft_list_size(mnl_fields *f, int handle, int which, long long *n);
/* ---- near-to-far-field monitors (src/near2far.cpp; meep.hpp dft_near2far) ----
 * 3-D, non-periodic.  The DFT is accumulated like every other DFT object's
 * (mnl_fields_dft_data, _dft_size, _dft_decimation, _dft_flush, _dft_array and
 * dump / load work on the handle); the far-field transform runs on the device.
 *
 * fields::add_dft_near2far (src/near2far.cpp:558-642): regions as for
 * mnl_fields_add_dft_flux (direction = the surface normal).  nperiods > 1 fails:
 * periodic images need periodic boundaries. */
int mnl_fields_add_dft_near2far(mnl_fields *f, int nreg, const double *regions, const double *freqs,
                                int nfreq, int decimation, int nperiods, int *handle);
/* dft_near2far::farfield for npts points (src/near2far.cpp:340-398), summed over ranks:
 * out[npts][nfreq][6] complex (Ex,Ey,Ez,Hx,Hy,Hz; re/im interleaved) */
int mnl_fields_near2far_farfields(mnl_fields *f, int handle, long long npts, const double *xyz,
                                  double *out);
/* eps, mu of the surrounding medium */
int mnl_fields_near2far_medium(mnl_fields *f, int handle, double *eps, double *mu);
/* per point of the list (the order of mnl_fields_dft_data): x, y, z, c0 (MNL_EX..MNL_HZ),
 * weight (boundary weights * dV * sign * region weight); out[5 * points] */
int mnl_fields_near2far_points(mnl_fields *f, int handle, double *out, long long npoints);

#ifdef __cplusplus
}
#endif
#endif
