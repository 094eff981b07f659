/* mfs.h -- C ABI of libmfs_hip.so: the MI355X (gfx950) pressure / viscosity CG path.
 *
 * The reference (SSTDV-Project/python-fluid-simulation) has no FFI: its `solver/`
 * package is Python that launches numba-CUDA kernels and cupy expressions
 * directly.  This header is therefore the boundary a maintainer binds INSTEAD of
 * those launches: every entry point names the reference function it replaces
 * (file:line, relative to the reference repo root).  The Python classes in
 * python-fluid-simulation_amd/solver/ bind it with ctypes.
 *
 * Conventions
 *  - plain pointers + sizes only; every array pointer is a DEVICE pointer unless
 *    the parameter name ends in `_host`.  No allocation happens behind the ABI:
 *    workspaces are sized by a query and handed in by the caller.
 *  - arrays are C-order with the reference's axis order [x,y,z] (z contiguous):
 *    cell arrays (Nx,Ny,Nz); face arrays vx/wx (Nx+1,Ny,Nz), vy/wy (Nx,Ny+1,Nz),
 *    vz/wz (Nx,Ny,Nz+1); doubled grid sphi/lvol (2Nx+1,2Ny+1,2Nz+1), sv (...,3).
 *  - `*_dt` arguments are mfs_dtype codes describing the element type of the
 *    array group they follow.
 *  - every call is asynchronous on `stream` (a hipStream_t) unless documented
 *    otherwise; return value is an mfs_status.  Nothing throws.
 */
#ifndef MFS_H
#define MFS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFS_ABI_VERSION 3   /* bumped when an existing entry point changes or goes; additions (the 2D solvers) keep it */

typedef enum { MFS_F32 = 0, MFS_F64 = 1 } mfs_dtype;

typedef enum {
  MFS_OK = 0,
  MFS_NOT_CONVERGED = 1,  /* reference: raise ValueError("Failed to converge!"), PressureCGSolver3D.py:222-223 */
  MFS_E_INVALID = -1,     /* bad argument (null pointer, bad dtype, bad size, misuse) */
  MFS_E_HIP = -2,         /* a HIP runtime call failed; see mfs_last_error() */
  MFS_E_NODEVICE = -3,    /* no gfx950 device visible */
  MFS_E_TIMEOUT = -4,     /* slab loop: a peer GPU did not answer within MFS_P2P_TIMEOUT_MS; the solve was stopped */
  MFS_E_ZERODIV = -5,     /* CG: d.q == 0 -- the reference's `alpha = delta / dq` raises ZeroDivisionError
                             (PressureCGSolver3D.py:211, ViscosityCGSolver3D.py:594); returned by the next poll / solve */
  MFS_E_NONFINITE = -6    /* CG: d.q or r.r is NaN / inf (poisoned input).  The reference would iterate to max_iter on
                             `nan < tol**2` and then raise ValueError("Failed to converge!"); the device loop stops at once */
} mfs_status;

typedef void* mfs_stream; /* hipStream_t */

int mfs_abi_version(void);
/* thread-local text of the last failure on this thread ("" if none) */
const char* mfs_last_error(void);
/* name of the device the current HIP context runs on, e.g. "gfx950:..."; host call */
int mfs_device_name(char* buf_host, size_t cap);

/* ------------------------------------------------------------------------- */
/* Solid fractions                                                           */
/* ------------------------------------------------------------------------- */
/* replaces compute_solid_frac -- solver/SolidFraction3D.py:6-32.
 * Writes w*[0:N] on every axis; the upper faces w*[N] are left untouched.      */
int mfs_solid_frac3d(const int64_t gres[3], const void* sphi, int sphi_dt,
                     void* wx, void* wy, void* wz, int w_dt, mfs_stream stream);
/* replaces compute_solid_frac -- solver/SolidFraction2D.py:6-26 */
int mfs_solid_frac2d(const int64_t gres[2], const void* sphi, int sphi_dt,
                     void* wx, void* wy, int w_dt, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Pressure, 3D -- stateless kernels (the reference's module-level functions)  */
/* ------------------------------------------------------------------------- */
/* replaces initialize_solver -- solver/PressureCGSolver3D.py:6-50,155-159 */
int mfs_pressure_rhs3d(const int64_t gres[3], const double cell_size[3],
                       const void* vx, const void* vy, const void* vz, int v_dt,
                       const void* sv, int sv_dt, const void* lphi, int lphi_dt,
                       const void* wx, const void* wy, const void* wz, int w_dt,
                       void* b, int b_dt, mfs_stream stream);
/* replaces matvecmul -- solver/PressureCGSolver3D.py:52-130,161-165.
 * Ghost-fluid 7-point operator straight from lphi and the face weights; boundary
 * cells of `out` are not written.  v,out share `dt`.                            */
int mfs_pressure_apply3d(const int64_t gres[3], const void* v, void* out, int dt,
                         const void* wx, const void* wy, const void* wz, int w_dt,
                         const void* lphi, int lphi_dt, mfs_stream stream);
/* replaces apply_pressure -- solver/PressureCGSolver3D.py:132-153,167-171 (in place on vx,vy,vz) */
int mfs_pressure_update3d(const int64_t gres[3], const double cell_size[3],
                          void* vx, void* vy, void* vz, int v_dt, const void* pv, int pv_dt,
                          const void* wx, const void* wy, const void* wz, int w_dt,
                          const void* sv, int sv_dt, const void* lphi, int lphi_dt,
                          mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Pressure, 3D -- the CG engine (replaces the loop PressureCGSolver3D.py:198-223) */
/* ------------------------------------------------------------------------- */
typedef struct mfs_pcg3d mfs_pcg3d;

/* bytes of device workspace mfs_pcg3d_create needs for this grid / state dtype */
size_t mfs_pcg3d_workspace_bytes(const int64_t gres[3], int dt);
/* number of doubles in the residual-history buffer kept inside the workspace */
int64_t mfs_pcg3d_history_capacity(void);
/* host call. `workspace` must be 256-byte aligned device memory of at least
 * mfs_pcg3d_workspace_bytes(); it is zeroed asynchronously on `stream`.         */
int mfs_pcg3d_create(mfs_pcg3d** out_host, const int64_t gres[3], int dt,
                     void* workspace, size_t workspace_bytes, mfs_stream stream);
int mfs_pcg3d_destroy(mfs_pcg3d* h);
/* once per solve: fold lphi + face weights into the 4 coefficient arrays the
 * per-iteration stencil reads (diag, and fluid-masked lower-face weights).     */
int mfs_pcg3d_setup(mfs_pcg3d* h, const void* lphi, int lphi_dt,
                    const void* wx, const void* wy, const void* wz, int w_dt, mfs_stream stream);
/* out = A v on cell planes [x_begin, x_end) (clipped to the interior 1..Nx-2);
 * the per-iteration hot kernel.  Also leaves sum(v*out) partials in the handle. */
int mfs_pcg3d_apply(mfs_pcg3d* h, const void* v, void* out, int64_t x_begin, int64_t x_end,
                    mfs_stream stream);
/* CG vectors: caller-owned cell arrays of the handle's dtype (CGSolverBuffer.py:3-8 + solver.x) */
int mfs_pcg3d_bind(mfs_pcg3d* h, void* b, void* x, void* d, void* r, void* q);
/* x*=0; q=A x; d=r=b-q; delta0=sum r^2; done=(delta0<tol^2)   (PressureCGSolver3D.py:198-206) */
int mfs_pcg3d_begin(mfs_pcg3d* h, double tol, mfs_stream stream);
/* enqueue n CG iterations (lines 207-221); iterations after convergence are device-side no-ops */
int mfs_pcg3d_iterate(mfs_pcg3d* h, int64_t n, mfs_stream stream);
/* the two halves of ONE iteration of mfs_pcg3d_iterate's launch-per-phase loop (so a caller can bracket the stencil launch
 * with events): the stencil launch, then the x/r update and the direction update / its bookkeeping.  In the lean form
 * (mfs_pcg3d_set_lean) the bookkeeping of iteration j is done by the stencil launch of j + 1, or -- when a poll, history,
 * finish or another loop form comes first -- by a one-block launch those calls enqueue themselves. */
int mfs_pcg3d_native_apply(mfs_pcg3d* h, mfs_stream stream);
int mfs_pcg3d_native_finish(mfs_pcg3d* h, mfs_stream stream);
/* after mfs_pcg3d_iterate calls of one's own: settle what the fused loop forms still owe -- the deferred x update
 * (mfs_pcg3d_set_defer_x) and the direction vector parked in the engine's partner buffer -- so that x and d are the
 * reference's.  mfs_pcg3d_solve does this itself.  Host-synchronous; call once, when no more iterations follow. */
int mfs_pcg3d_finish(mfs_pcg3d* h, mfs_stream stream);
/* native fused loop: let `x += alpha d` ride in the NEXT iteration's stencil launch (which re-reads d from cache) so
 * that the x/r update kernel only streams r and q; same values; the last update is owed until mfs_pcg3d_finish /
 * the end of mfs_pcg3d_solve.  on < 0 = auto (default; env MFS_DEFER_X): only when the CG vectors exceed the
 * Infinity Cache.  A caller of mfs_pcg3d_iterate must therefore end with mfs_pcg3d_finish before reading x.   */
int mfs_pcg3d_set_defer_x(mfs_pcg3d* h, int on);
/* native fused loop without the deferred x update: mfs_pcg3d_iterate closes iteration j (convergence test :218, beta :220,
 * history) at the top of the stencil launch of iteration j + 1 -- every workgroup folds the r.r partials itself -- and
 * ends a batch with a one-block bookkeeping launch, instead of a reduction tail in the x/r update.  Same values, bit
 * for bit; shorter dependent chain per iteration (what bounds small grids).  on < 0 = auto (default; env MFS_LEAN). */
int mfs_pcg3d_set_lean(mfs_pcg3d* h, int on);
/* small grids (the reference notebook's 48x80x48 and the like): mfs_pcg3d_iterate runs a whole batch of iterations
 * (PressureCGSolver3D.py:207-221) as ONE launch of <= 64 resident workgroups that keep x, r, d, q in registers and
 * exchange the two dot products and the box faces through self-validating records in the workspace -- no kernel
 * boundary per reduction.  Same arithmetic per cell; the grouping of the dot products differs from the launch-per-phase
 * loops, so results agree with them to rounding.  on < 0 = auto (default; env MFS_RESIDENT): whenever the grid fits. */
int mfs_pcg3d_set_resident(mfs_pcg3d* h, int on);
/* synchronises `stream`, then reports the device-resident solver state. host call. */
int mfs_pcg3d_poll(mfs_pcg3d* h, mfs_stream stream, int64_t* iters_host, int* done_host,
                   double* delta_host, double* alpha_host, double* beta_host);
/* begin + iterate/poll until done or max_iter; MFS_OK or MFS_NOT_CONVERGED. host-synchronous.  check_every = iterations
 * enqueued between two looks at the convergence flag (the resident small-grid loop, which stops by itself inside a
 * batch, uses max(check_every, 128)). */
int mfs_pcg3d_solve(mfs_pcg3d* h, double tol, int64_t max_iter, int64_t check_every,
                    mfs_stream stream, int64_t* iters_host);
/* copies [delta0, dq1, delta1, dq2, delta2, ...] (first `cap` values) to the host; returns count or <0 */
int64_t mfs_pcg3d_history(mfs_pcg3d* h, double* out_host, int64_t cap, mfs_stream stream);

/* -- single phases of one iteration, for the slab-decomposed multi-GPU driver.
 * Order per iteration k:  [halo exchange of d] phase_apply(ranges...) ->
 * phase_reduce(0) -> [all-reduce scalars[DQ]] -> phase_update_xr ->
 * phase_reduce(1) -> [all-reduce scalars[RR]] -> phase_update_d
 * (or phase_update_r -> phase_reduce(1) -> [all-reduce RR || phase_update_x] -> phase_update_d). */
int mfs_pcg3d_phase_apply(mfs_pcg3d* h, int64_t x_begin, int64_t x_end, int first, mfs_stream stream);
/* two disjoint plane ranges in one launch (the driver's two edge planes) */
int mfs_pcg3d_phase_apply2(mfs_pcg3d* h, int64_t x_begin, int64_t x_end, int64_t x_begin2, int64_t x_end2,
                           int first, mfs_stream stream);
int mfs_pcg3d_phase_reduce(mfs_pcg3d* h, int which, mfs_stream stream);
int mfs_pcg3d_phase_update_xr(mfs_pcg3d* h, mfs_stream stream);
/* the same update as two kernels: `r -= a q` (+ r.r partials) and `x += a d`, so that the
 * driver can start the r.r all-reduce after the first and overlap it with the second */
int mfs_pcg3d_phase_update_r(mfs_pcg3d* h, mfs_stream stream);
int mfs_pcg3d_phase_update_x(mfs_pcg3d* h, mfs_stream stream);
int mfs_pcg3d_phase_update_d(mfs_pcg3d* h, mfs_stream stream);
/* begin, split around the one reduction it contains: begin_local -> [all-reduce RR] -> begin_finish */
int mfs_pcg3d_begin_local(mfs_pcg3d* h, double tol, mfs_stream stream);
int mfs_pcg3d_begin_finish(mfs_pcg3d* h, mfs_stream stream);
/* device pointer to the engine's double[MFS_PCG_NSCALARS] block and slot indices */
#define MFS_PCG_NSCALARS 16
#define MFS_PCG_S_DQ 0      /* sum d.q of the current iteration */
#define MFS_PCG_S_RR 1      /* sum r.r produced by the latest update (delta_new) */
#define MFS_PCG_S_DELTA 2   /* delta the current iteration started from */
#define MFS_PCG_S_TOL2 3
#define MFS_PCG_S_DONE 4
#define MFS_PCG_S_ITERS 5
#define MFS_PCG_S_ALPHA 6
#define MFS_PCG_S_BETA 7
#define MFS_PCG_S_LASTRR 8  /* r.r of the last completed iteration (what the reference keeps in self.delta) */
#define MFS_PCG_S_ERR 11    /* != 0: the device loop stopped itself: 1 / 2 a peer-to-peer wait of the slab loop timed out,
                               3 d.q == 0, 4 non-finite d.q or r.r */
#define MFS_PCG_S_LANE 13   /* diagnostics: 1 when the solve's listed launches mask dead vectors lane by lane (mfs_pcg3d_set_sparse) */
void* mfs_pcg3d_scalars(mfs_pcg3d* h);
/* performance knobs of the stencil kernel (results are identical for every setting):
 * variant 0 = direct loads, 1 = x-marching in registers, 2 = x-marching + LDS-staged
 * plane tiles (default); xchunk = cap on the planes of one march (0 = none);
 * blocks_per_cu = workgroups per CU the (tile, plane) work is cut into;
 * nontemporal > 0 marks the once-read coefficient streams, 0 never, < 0 = auto
 * (on when the six arrays of one apply exceed the Infinity Cache).                */
int mfs_pcg3d_tune(mfs_pcg3d* h, int variant, int xchunk, int blocks_per_cu, int nontemporal);
/* compressed coefficient access (default on): the per-iteration kernel reads the four
 * coefficient arrays only for z-vectors that are neither all-zero rows nor regular
 * interior rows (class byte per vector built by mfs_pcg3d_setup); results are bit-identical */
int mfs_pcg3d_set_compress(mfs_pcg3d* h, int on);
/* form of the native loop for the engine as bound: bit 0 = direction update fused into the stencil launch,
 * bit 1 = x update deferred into it too, bit 2 = Jacobi loop, bit 3 = resident small-grid loop (mfs_pcg3d_set_resident) */
int mfs_pcg3d_loop_info(mfs_pcg3d* h);
/* sparse lists of a single-domain solve (round 3; default on from 2^21 cells, env MFS_SPARSE / MFS_SPARSE_MIN): behind the
 * initial residual mfs_pcg3d_begin lists the 32-cell chunks holding a live z-vector (row not ZERO, or r, d != 0) and the
 * (tile, plane) pairs of the march holding one; the r update sweeps the listed chunks, the fused stencil launches visit the
 * listed pairs.  Dead vectors keep q = r = d = +0 and x unchanged, which is what the dense loop computes for them; the dot
 * products group differently (rounding).  The window / collective slab loops (mfs_pcg3d_slab_begin) build the same lists for
 * their owned planes and their interior launch, and so does the fused single-domain Jacobi loop (z = r / diag is 0 wherever r
 * is); begin_local / phase callers, the slab and the three-launch Jacobi loops stay dense.  Where more than
 * a quarter of the listed pairs' vectors are dead, the listed launches also mask those vectors' loads and stores lane by lane
 * (decided per solve on the device, picked up by the host with its first look at the scalar block: slot 13, diagnostics).
 * mfs_pcg3d_sparse_info (host-synchronous): out = {listed chunks, chunks, listed pairs, pairs}; zeros where a list is off. */
int mfs_pcg3d_set_sparse(mfs_pcg3d* h, int on);
int mfs_pcg3d_sparse_info(mfs_pcg3d* h, mfs_stream stream, int64_t out[4]);
/* OPT-IN Jacobi preconditioning of the native loop (default off; env MFS_JACOBI=1): delta = r.z with z = r / diag,
 * convergence test unchanged (r.r < tol^2).  Fused form (default where the fused direction update is available): the r
 * update stores z and closes the iteration, the next stencil launch forms d = z + beta d (2 launches per iteration);
 * otherwise z is formed inside the two vector phases (3 launches).  NOT the reference's algorithm -- the reference's CG
 * is unpreconditioned and its residual history cannot be matched with this on.  Runs in the single-GPU loop and in the
 * WINDOW slab loop (mfs_pcg3d_slab_*: z as the operand of the edge / interior direction updates, r.r and r.z all-reduced
 * in the tail of the r / z update); the phase API of the collective loop has no Jacobi form. */
int mfs_pcg3d_set_jacobi(mfs_pcg3d* h, int on);
/* fused direction update (default on, native loop only): `d = r + beta d` is formed inside the next
 * stencil launch instead of in a pass of its own; bit-identical; d ping-pongs with an engine buffer */
int mfs_pcg3d_set_fuse(mfs_pcg3d* h, int on);
/* planes of the operand stream the LDS march keeps in flight ahead of the plane it computes (1 or 2) */
int mfs_pcg3d_set_prefetch(mfs_pcg3d* h, int planes);

/* ------------------------------------------------------------------------- */
/* Pressure, 3D -- slab-decomposed CG over peer-to-peer windows (multi-GPU)     */
/* ------------------------------------------------------------------------- */
/* New design (the reference is single-GPU): one process per GPU, the grid cut into
 * x-slabs (mfs/dist.py).  A window is a block of uncached device memory per rank that
 * the other ranks of the node map through HIP IPC; inside the CG loop the edge planes of
 * the direction vector and the two dot products travel as plain xGMI stores issued by
 * the solver's own kernels (csrc/mfs_p2p.h, csrc/mfs_pcg_slab.h) -- no host round trip
 * and no collective call per iteration.  EXCEPTION to "nothing allocates behind the
 * ABI": the window is allocated here, because IPC-exportable uncached memory cannot be
 * carved from a caller's sub-allocator.                                             */
typedef struct mfs_p2p mfs_p2p;
/* size of the opaque IPC handle mfs_p2p_create writes (hipIpcMemHandle_t) */
size_t mfs_p2p_handle_bytes(void);
/* host call: allocate this rank's window for halo planes of `plane_bytes` (= Ny*Nz*sizeof
 * element) and write its IPC handle to handle_out_host (mfs_p2p_handle_bytes() bytes)  */
int mfs_p2p_create(mfs_p2p** out_host, int rank, int world, size_t plane_bytes, void* handle_out_host);
/* host call: map the peers' windows; handles_host = world handles in rank order (all-gathered by the caller) */
int mfs_p2p_connect(mfs_p2p* p, const void* handles_host);
/* COLLECTIVE, host-synchronous: every rank sends a patterned plane to its neighbours, takes part
 * in one all-reduce through the windows and verifies what it received.  ok_host = 1 only if
 * everything arrived intact within the time limit; detail_host (4 words, optional): ok, payload
 * vectors missing or wrong, all-reduce timed out, all-reduce sum as float bits                  */
int mfs_p2p_selftest(mfs_p2p* p, int round, mfs_stream stream, int* ok_host, unsigned* detail_host);
/* alloc_kind: 1 = hipDeviceMallocUncached, 2 = hipDeviceMallocFinegrained */
int mfs_p2p_info(mfs_p2p* p, int* alloc_kind_host, size_t* window_bytes_host);
/* host call; every rank must have finished using the windows (barrier first) */
int mfs_p2p_destroy(mfs_p2p* p);

/* let the engine run its slab loop over this window (null detaches) */
int mfs_pcg3d_attach_p2p(mfs_pcg3d* h, mfs_p2p* p);
/* the slab loop: begin / iterate / solve with the semantics of mfs_pcg3d_begin / _iterate /
 * _solve on the GLOBAL grid; COLLECTIVE -- every rank of the window calls them in step.
 * The engine's grid is this rank's slab incl. one ghost / boundary plane each side.
 * A peer that does not answer within MFS_P2P_TIMEOUT_MS (default 10000) stops the solve:
 * the next poll / solve returns MFS_E_TIMEOUT.                                          */
/* 1 if the slab loop can run on this engine (window attached, CG vectors bound and 16-byte aligned, Nz a multiple
 * of the 16-byte vector length, stencil variant 2, pressure operator); else the caller uses the collective loop */
/* Collective transport for the slab loop (round 3): the same launches as the window loop (edge d, fused interior march,
 * edge apply + d.q, r update + r.r) with NO in-kernel exchange -- the two edge planes travel by ncclSend / ncclRecv on the
 * solver's second stream beside the interior launch, each dot product is ONE ncclAllReduce on the device scalar block, all
 * enqueued from C (no host synchronisation, no Python inside a batch).  RCCL is resolved at run time from `lib_path` (the
 * librccl the process already maps).  mfs_rccl_unique_id on rank 0 -> every rank -> mfs_rccl_create (collective); then
 * mfs_pcg3d_attach_rccl with the rank's OWN one-rank window (mfs_p2p_create(&w, 0, 1, ...)); mfs_pcg3d_slab_begin / _iterate /
 * _solve run the loop.  The reference is single-GPU; this is the fallback where HIP-IPC windows fail. */
typedef struct mfs_rccl mfs_rccl;
int mfs_rccl_unique_id_bytes(void);
int mfs_rccl_unique_id(const char* lib_path, void* id_out);
int mfs_rccl_create(mfs_rccl** out_host, const char* lib_path, const void* id, int rank, int world);
int mfs_rccl_destroy(mfs_rccl* r);
int mfs_pcg3d_attach_rccl(mfs_pcg3d* h, mfs_p2p* own_window, mfs_rccl* comm);
int mfs_pcg3d_slab_supported(mfs_pcg3d* h);
/* slab loop tuning: send the edge planes from a second HIP stream so that the xGMI stores overlap the interior
 * stencil launch (costs two cross-stream event hops per iteration; default: on for planes >= 1 MiB of granules) */
int mfs_pcg3d_slab_set_aux(mfs_pcg3d* h, int on);
int mfs_pcg3d_slab_begin(mfs_pcg3d* h, double tol, mfs_stream stream);
int mfs_pcg3d_slab_iterate(mfs_pcg3d* h, int64_t n, mfs_stream stream);
int mfs_pcg3d_slab_solve(mfs_pcg3d* h, double tol, int64_t max_iter, int64_t check_every,
                         mfs_stream stream, int64_t* iters_host);

/* ------------------------------------------------------------------------- */
/* Viscosity, 3D -- stateless kernels (the reference's module-level functions) */
/* ------------------------------------------------------------------------- */
/* replaces extrapolate -- solver/ViscosityCGSolver3D.py:8-39,472-502 (in place on vx,vy,vz;
 * `workspace` holds the ping-pong copies and validity masks)                     */
size_t mfs_visc_extrapolate3d_workspace_bytes(const int64_t gres[3], int v_dt);
int mfs_visc_extrapolate3d(const int64_t gres[3], int num_iter, void* vx, void* vy, void* vz, int v_dt,
                           const void* sphi, int sphi_dt, void* workspace, size_t workspace_bytes,
                           mfs_stream stream);
/* the two pieces of extrapolate, for callers that act between sweeps (slab decomposition: the ghost planes of
 * values and validity travel after every sweep).  comp = 0/1/2 (vx/vy/vz); valid = one byte per face:
 * `valid = sphi(face) >= 0` (:479-481), then one Jacobi sweep old -> new (:8-39, the loop body of :483-502) */
int mfs_visc_valid3d(const int64_t gres[3], int comp, const void* sphi, int sphi_dt, unsigned char* valid,
                     mfs_stream stream);
int mfs_visc_extrapolate_sweep3d(const int64_t gres[3], int comp, const void* v_in, void* v_out, int v_dt,
                                 const unsigned char* valid_in, unsigned char* valid_out, mfs_stream stream);
/* replaces initialize_solver -- solver/ViscosityCGSolver3D.py:41-246,504-513.
 * `vol` is the doubled-grid fluid volume already divided by cell_vol/8 (self.vol, :568) */
int mfs_visc_rhs3d(const int64_t gres[3], double scale, double mu,
                   const void* vx, const void* vy, const void* vz, int v_dt,
                   const void* sphi, int sphi_dt, const void* vol, int vol_dt,
                   void* b_x, void* b_y, void* b_z, int b_dt, mfs_stream stream);
/* replaces matvecmul -- solver/ViscosityCGSolver3D.py:248-456,515-524 */
int mfs_visc_apply3d(const int64_t gres[3], double scale, double mu,
                     const void* vx, const void* vy, const void* vz, int v_dt,
                     void* out_x, void* out_y, void* out_z, int out_dt,
                     const void* sphi, int sphi_dt, const void* vol, int vol_dt, mfs_stream stream);
/* replaces apply_viscosity -- solver/ViscosityCGSolver3D.py:458-470,526-530 (in place on vx,vy,vz) */
int mfs_visc_writeback3d(const int64_t gres[3], void* vx, void* vy, void* vz, int v_dt,
                         const void* out_x, const void* out_y, const void* out_z, int out_dt,
                         const void* sphi, int sphi_dt, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Viscosity, 3D -- the CG engine (replaces the loop ViscosityCGSolver3D.py:575-612) */
/* ------------------------------------------------------------------------- */
/* The five CG vectors are FLAT arrays of mfs_vcg3d_dofs() elements laid out
 * [ x-faces (Nx+1,Ny,Nz) | y-faces (Nx,Ny+1,Nz) | z-faces (Nx,Ny,Nz+1) ]; the
 * reference's per-component arrays (x_x, x_y, x_z, ...) are views into them.       */
typedef struct mfs_vcg3d mfs_vcg3d;
size_t mfs_vcg3d_workspace_bytes(const int64_t gres[3], int dt);
int64_t mfs_vcg3d_dofs(const int64_t gres[3]);
int mfs_vcg3d_create(mfs_vcg3d** out_host, const int64_t gres[3], int dt,
                     void* workspace, size_t workspace_bytes, mfs_stream stream);
int mfs_vcg3d_destroy(mfs_vcg3d* h);
/* once per solve: de-interleave the doubled-grid `vol` into its 7 parity classes and
 * `sphi >= 0` at the 3 face classes into byte masks (unit stride for the iteration) */
int mfs_vcg3d_setup(mfs_vcg3d* h, double scale, double mu, const void* sphi, int sphi_dt,
                    const void* vol, int vol_dt, mfs_stream stream);
/* out = A v on flat vectors; the per-iteration kernel(s) */
int mfs_vcg3d_apply(mfs_vcg3d* h, const void* v, void* out, mfs_stream stream);
int mfs_vcg3d_bind(mfs_vcg3d* h, void* b, void* x, void* d, void* r, void* q);
/* q=A x (x = extrapolated velocity, NOT zeroed); d=r=b-q; delta0   (:575-587) */
int mfs_vcg3d_begin(mfs_vcg3d* h, double tol, mfs_stream stream);
/* n iterations of the loop :588-610: stencil launch, r update, direction + x update.  Opt-in form (mfs_vcg3d_set_fuse,
 * where the x-marching kernel serves the engine -- mfs_vcg3d_loop_info bit 0): 2 launches per iteration -- the stencil launch of iteration j also forms d_j = r + beta d_{j-1} (:609-610) and
 * performs x += alpha d_{j-1} (:595-597) for the faces it owns, the r update's last block closes the iteration (:604-608).
 * x then lags one update behind and d_j may sit in an engine buffer until mfs_vcg3d_finish / the end of mfs_vcg3d_solve. */
int mfs_vcg3d_iterate(mfs_vcg3d* h, int64_t n, mfs_stream stream);
/* settles what mfs_vcg3d_iterate's fused loop owes (last x update; d_iters = r + beta d unless converged, brought home to
 * the bound `d`): state as after the reference's loop :588-610.  Host-synchronous; begin again before iterating further. */
int mfs_vcg3d_finish(mfs_vcg3d* h, mfs_stream stream);
/* 1 / 0: fused direction + x update in mfs_vcg3d_iterate / solve (default 0 -- measured slower, DESIGN.md section 4;
 * env MFS_VISC_FUSE); results bit-identical */
int mfs_vcg3d_set_fuse(mfs_vcg3d* h, int on);
/* compressed class access of the x-marching kernel (default on; env MFS_VISC_COMPRESS): per z-vector and plane a class
 * (built by mfs_vcg3d_setup, stored in spare bits of the packed mask bytes) says whether every volume sample the
 * vector's step loads is 0 (air), 1 (bulk liquid) or anything else; only the last kind reads the seven class arrays
 * (lvol de-interleaved, ViscosityCGSolver3D.py:248-456 reads it at 7 of 8 doubled-grid parities).  Bit-identical. */
int mfs_vcg3d_set_compress(mfs_vcg3d* h, int on);
/* census of those classes after mfs_vcg3d_setup: counts_host[0] = z-vectors whose samples are all 0, [1] = all 1,
 * [2] = the rest (the only ones that read the class arrays).  Diagnostic, host-synchronous. */
int mfs_vcg3d_class_census(mfs_vcg3d* h, int64_t counts_host[3], mfs_stream stream);
/* sparse lists of a single-domain solve (round 3; default on from 2^21 unknowns, env MFS_VISC_SPARSE / MFS_VISC_SPARSE_MIN): the
 * r and d / x updates sweep the 32-unknown chunks holding a face whose row is not empty (or r, d != 0), and -- with the
 * compressed class access -- the march launches of mfs_vcg3d_iterate visit only the (tile, plane) pairs that are not all air
 * (their q = +0 was stored by the solve's initial q = A x; nothing else writes it).  Values as in the dense loop; the dot
 * products group differently.  The window slab loop and the single-domain Jacobi loop take the lists too; phase callers, the
 * opt-in fused loop and the slab Jacobi loop stay dense.
 * mfs_vcg3d_sparse_info (host-synchronous): out = {listed chunks, chunks, listed pairs, pairs} of the solve begun last. */
int mfs_vcg3d_set_sparse(mfs_vcg3d* h, int on);
int mfs_vcg3d_sparse_info(mfs_vcg3d* h, mfs_stream stream, int64_t out[4]);
/* bit 0: mfs_vcg3d_iterate will run the fused 2-launch loop for the engine as bound and set up; bit 1: the small-problem
 * loop -- the r update (:592-601), the r.r reduction, the test / bookkeeping (:604-608) and the x / direction updates
 * (:595-597, :609-610) in ONE launch whose resident workgroups exchange their partial sums (csrc/mfs_cg_core.h
 * k_update_rdx): 2 launches per iteration, results equal to the three-launch loop's up to the grouping of r.r */
int mfs_vcg3d_loop_info(mfs_vcg3d* h);
/* OPT-IN Jacobi preconditioning of the viscosity loop (default off; env MFS_VISC_JACOBI=1): z = r / diag with the operator's
 * own diagonal (vol_c + scale mu (...), :268 / :338 / :408; built once per solve), delta = r.z, convergence test unchanged
 * (r.r < tol^2).  NOT the reference's iteration (ViscosityCGSolver3D.py:575-612 is unpreconditioned): another residual
 * history, the same solution to the tolerance, far fewer iterations where partly filled cells make the diagonal span orders
 * of magnitude.  Single GPU (mfs_vcg3d_begin / iterate / solve) and the window slab loop (mfs_vcg3d_slab_begin / slab_iterate:
 * r.z all-reduced as a third episode); bit 2 of mfs_vcg3d_loop_info. */
int mfs_vcg3d_set_jacobi(mfs_vcg3d* h, int on);
/* 1 / 0: allow that small-problem loop (default 1; env MFS_RDX).  A launch that is not fully resident (shared GPU) times
 * out without having written anything; the next poll switches the engine to the three-launch loop for good. */
int mfs_vcg3d_set_merged(mfs_vcg3d* h, int on);
/* 1 / 0: allow the RESIDENT small-grid loop (default on where the grid qualifies; env MFS_VISC_RESIDENT): the loop
 * ViscosityCGSolver3D.py:588-610 as ONE launch per mfs_vcg3d_iterate batch -- x, r, d, q of every face in the registers of
 * up to 128 resident workgroups, d with its halo in LDS, dot products and halo faces exchanged as self-validating records
 * (csrc/mfs_vcg_resident.h).  Same arithmetic per element; the dot products group differently, so histories agree with the
 * launch-per-phase loop to rounding.  A launch that is not fully resident (shared GPU) times out at its first dot product
 * without having written anything; the next poll switches the engine to the launch-per-phase loop for good.
 * Bit 3 of mfs_vcg3d_loop_info. */
int mfs_vcg3d_set_resident(mfs_vcg3d* h, int on);
int mfs_vcg3d_poll(mfs_vcg3d* h, mfs_stream stream, int64_t* iters_host, int* done_host,
                   double* delta_host, double* alpha_host, double* beta_host);
int mfs_vcg3d_solve(mfs_vcg3d* h, double tol, int64_t max_iter, int64_t check_every,
                    mfs_stream stream, int64_t* iters_host);
int64_t mfs_vcg3d_history(mfs_vcg3d* h, double* out_host, int64_t cap, mfs_stream stream);
/* Which kernel the CG applies (matvecmul_{x,y,z}_kernel, ViscosityCGSolver3D.py:248-456, on the direction vector)
 * take for the engine as bound: 2 = x-marching 16-byte-vector kernel (csrc/mfs_vcg_march.h; needs Nz % 4 == 0 (fp32) /
 * Nz % 2 == 0 (fp64) and 16-byte aligned vectors), 0 = one-cell-per-lane direct-load kernel; both give bit-identical
 * results.  1 (the LDS-tiled kernel of MFS_VISC_TILED=1) is retired with that kernel: never returned.            */
int mfs_vcg3d_apply_kernel(mfs_vcg3d* h);
/* Slab decomposition along x (the build's extension; host driver mfs/dist.py:SlabVCG): one
 * iteration = halo exchange of d's edge planes (3 components), phase_apply, phase_reduce(0), all-reduce of
 * scalars[MFS_PCG_S_DQ], phase_update_xr, phase_reduce(1), all-reduce of scalars[MFS_PCG_S_RR], phase_update_d
 * -- the same phases and scalar block (device pointer: mfs_vcg3d_scalars) as mfs_pcg3d_phase_*.
 * set_slab(skip_top_x = 1) on every rank but the last: its last u plane is the right neighbour's.       */
int mfs_vcg3d_set_slab(mfs_vcg3d* h, int skip_top_x);
void* mfs_vcg3d_scalars(mfs_vcg3d* h);
int mfs_vcg3d_begin_local(mfs_vcg3d* h, double tol, mfs_stream stream);
int mfs_vcg3d_begin_finish(mfs_vcg3d* h, mfs_stream stream);
int mfs_vcg3d_phase_apply(mfs_vcg3d* h, mfs_stream stream);
int mfs_vcg3d_phase_reduce(mfs_vcg3d* h, int which, mfs_stream stream);
int mfs_vcg3d_phase_update_xr(mfs_vcg3d* h, mfs_stream stream);
int mfs_vcg3d_phase_update_d(mfs_vcg3d* h, mfs_stream stream);
/* The same loop with the halo planes and the two dot products moving through a peer-to-peer window (mfs_p2p_*, below /
 * above): attach a connected window created with plane_bytes = (Ny*Nz + (Ny+1)*Nz + Ny*(Nz+1)) * sizeof(element);
 * slab_begin / slab_iterate then enqueue whole iterations without any host-side exchange.  Poll as usual.   */
int mfs_vcg3d_attach_p2p(mfs_vcg3d* h, mfs_p2p* window);
int mfs_vcg3d_slab_begin(mfs_vcg3d* h, double tol, mfs_stream stream);
int mfs_vcg3d_slab_iterate(mfs_vcg3d* h, int64_t n, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Density solver, 3D -- reference solver/DensityCGSolver3D.py */
/* ------------------------------------------------------------------------- */
/* The CG loop of DensityCGSolver3D.solve (:318-345) runs on the pressure engine: call
 * mfs_pcg3d_setup_density instead of mfs_pcg3d_setup, then bind / solve as for pressure.
 * Its operator (matvecmul_kernel :118-207) is the pressure stencil with diag counting 1 per
 * fluid neighbour and the -z tap weighted by wz[x,y,z+1] (kept as written, :184).            */
int mfs_pcg3d_setup_density(mfs_pcg3d* h, const void* lphi, int lphi_dt,
                            const void* wx, const void* wy, const void* wz, int w_dt, mfs_stream stream);
/* replaces initialize_density -- :8-36,255-260: scatters particle mass pm[p] and the (scalar) particle
 * volume to the 8 surrounding cell centres with fp atomics; px is (P,3) row-major; gm, gvol share g_dt */
int mfs_density_splat3d(const int64_t gres[3], const double bound_min[3], const double cell_size[3],
                        const void* px, int px_dt, const void* pm, int pm_dt, double pvol, int64_t num_particles,
                        void* gm, void* gvol, int g_dt, mfs_stream stream);
/* replaces fix_volume -- :38-86,262-269 (in place on gvol; the reference's `lvol` argument is unused there) */
int mfs_density_fix_volume3d(const int64_t gres[3], const double cell_size[3], void* gvol, int g_dt,
                             const void* sphi, int sphi_dt, const void* lphi, int lphi_dt,
                             const void* wx, const void* wy, const void* wz, int w_dt, mfs_stream stream);
/* replaces initialize_solver -- :88-116,271-277 */
int mfs_density_rhs3d(const int64_t gres[3], double rho0, double dt, const double cell_size[3],
                      const void* gm, const void* gvol, int g_dt, const void* lphi, int lphi_dt,
                      const void* wx, const void* wy, const void* wz, int w_dt, void* b, int b_dt, mfs_stream stream);
/* replaces matvecmul -- :118-207,279-283 (stateless; boundary cells of `out` are not written) */
int mfs_density_apply3d(const int64_t gres[3], const void* v, void* out, int dt,
                        const void* wx, const void* wy, const void* wz, int w_dt,
                        const void* lphi, int lphi_dt, mfs_stream stream);
/* replaces compute_displacement -- :209-222,285-289: face displacements from the solved field pv */
int mfs_density_displacement3d(const int64_t gres[3], double dt, const double cell_size[3],
                               void* dx, void* dy, void* dz, int d_dt, const void* pv, int pv_dt,
                               const void* lphi, int lphi_dt, mfs_stream stream);
/* replaces apply_displacement -- :224-253,291-296: px[:, axis] += trilinear sample of the face array d
 * (shape dshape, samples at (index + grid_bias) * cell_size + bound_min)                              */
int mfs_density_advect3d(void* px, int px_dt, int64_t num_particles, const void* d, int d_dt,
                         const int64_t dshape[3], const double bound_min[3], const double cell_size[3],
                         const double grid_bias[3], int axis, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Density solver, 2D -- reference solver/DensityCGSolver2D.py                   */
/* ------------------------------------------------------------------------- */
/* The CG loop of DensityCGSolver2D.solve (:274-290) runs on the 2D pressure engine: mfs_pcg2d_setup_density (below,
 * beside mfs_pcg2d_setup), then bind / solve as for pressure.  Where the 2D kernels differ from their 3D twins it is
 * the reference that differs: the splat writes gm only, fix_volume reads lvol, the operator has no asymmetric tap. */
/* replaces initialize_density -- :8-33,197-202: scatters particle mass pm[p] to the 4 surrounding cell centres
 * (indices clamped to the grid) with fp atomics; px is (P,2) row-major.  ONLY gm is written: the reference's volume
 * scatter is commented out (:33); pvol and gvol are accepted and unused                                          */
int mfs_density_splat2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2],
                        const void* px, int px_dt, const void* pm, int pm_dt, double pvol, int64_t num_particles,
                        void* gm, void* gvol, int g_dt, mfs_stream stream);
/* replaces fix_volume -- :35-57,204-211: gvol = min(lvol summed over the cell's nine doubled-grid samples with
 * weights 1, 1/2, 1/4 -- or the cell volume for an internal fluid cell away from solids --, cell volume * open
 * fraction); interior cells only, boundary cells of gvol keep what they held                                    */
int mfs_density_fix_volume2d(const int64_t gres[2], const double cell_size[2], const void* lvol, int lvol_dt,
                             void* gvol, int g_dt, const void* sphi, int sphi_dt, const void* lphi, int lphi_dt,
                             const void* wx, const void* wy, int w_dt, mfs_stream stream);
/* replaces initialize_solver -- :59-83,213-219 */
int mfs_density_rhs2d(const int64_t gres[2], double rho0, double dt, const double cell_size[2],
                      const void* gm, const void* gvol, int g_dt, const void* lphi, int lphi_dt,
                      const void* wx, const void* wy, int w_dt, void* b, int b_dt, mfs_stream stream);
/* replaces matvecmul -- :85-139,221-225 (stateless; boundary cells of `out` are not written): the pressure 5-point
 * stencil with diag counting 1 per fluid neighbour and 1/theta per air neighbour                               */
int mfs_density_apply2d(const int64_t gres[2], const void* v, void* out, int dt,
                        const void* wx, const void* wy, int w_dt, const void* lphi, int lphi_dt, mfs_stream stream);
/* replaces compute_displacement -- :141-152,227-231: dx[x,y], dy[x,y] for 1 <= x <= Nx-1, 1 <= y <= Ny-1 (the last
 * cell included); every other entry of dx (Nx+1,Ny) and dy (Nx,Ny+1) is left alone                              */
int mfs_density_displacement2d(const int64_t gres[2], double dt, const double cell_size[2],
                               void* dx, void* dy, int d_dt, const void* pv, int pv_dt,
                               const void* lphi, int lphi_dt, mfs_stream stream);
/* replaces apply_displacement -- :171-195,233-238: px[:, axis] += bilinear sample of the face array d (shape dshape,
 * samples at (index + grid_bias) * cell_size + bound_min, indices clamped to dshape); four separate additions
 * into the stored value, so an fp32 px rounds after each                                                        */
int mfs_density_advect2d(void* px, int px_dt, int64_t num_particles, const void* d, int d_dt,
                         const int64_t dshape[2], const double bound_min[2], const double cell_size[2],
                         const double grid_bias[2], int axis, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Pressure, 2D (BASELINE config 1) -- reference solver/PressureCGSolver2D.py    */
/* ------------------------------------------------------------------------- */
/* replaces initialize_solver -- solver/PressureCGSolver2D.py:6-44,122-126 */
int mfs_pressure_rhs2d(const int64_t gres[2], const double cell_size[2],
                       const void* vx, const void* vy, int v_dt, const void* sv, int sv_dt,
                       const void* lphi, int lphi_dt, const void* wx, const void* wy, int w_dt,
                       void* b, int b_dt, mfs_stream stream);
/* replaces matvecmul -- solver/PressureCGSolver2D.py:46-100,128-132 */
int mfs_pressure_apply2d(const int64_t gres[2], const void* v, void* out, int dt,
                         const void* wx, const void* wy, int w_dt, const void* lphi, int lphi_dt,
                         mfs_stream stream);
/* replaces apply_pressure -- solver/PressureCGSolver2D.py:102-120,134-138 */
int mfs_pressure_update2d(const int64_t gres[2], const double cell_size[2], void* vx, void* vy, int v_dt,
                          const void* pv, int pv_dt, const void* wx, const void* wy, int w_dt,
                          const void* sv, int sv_dt, const void* lphi, int lphi_dt, mfs_stream stream);
/* the CG loop solver/PressureCGSolver2D.py:159-177 (no error on non-convergence in the reference:
 * mfs_pcg2d_solve returns MFS_NOT_CONVERGED and the caller carries on)                             */
typedef struct mfs_pcg2d mfs_pcg2d;
size_t mfs_pcg2d_workspace_bytes(const int64_t gres[2], int dt);
int mfs_pcg2d_create(mfs_pcg2d** out_host, const int64_t gres[2], int dt,
                     void* workspace, size_t workspace_bytes, mfs_stream stream);
int mfs_pcg2d_destroy(mfs_pcg2d* h);
int mfs_pcg2d_setup(mfs_pcg2d* h, const void* lphi, int lphi_dt, const void* wx, const void* wy, int w_dt);
/* the same engine on DensityCGSolver2D's operator (solver/DensityCGSolver2D.py:85-139, loop :274-290); a later
 * mfs_pcg2d_setup puts the engine back in pressure mode                                                      */
int mfs_pcg2d_setup_density(mfs_pcg2d* h, const void* lphi, int lphi_dt, const void* wx, const void* wy, int w_dt);
int mfs_pcg2d_bind(mfs_pcg2d* h, void* b, void* x, void* d, void* r, void* q);
/* out = A v (the loop's stencil launch on caller vectors, in the mode the last setup chose; bit-identical to
 * mfs_pressure_apply2d / mfs_density_apply2d, boundary cells of `out` untouched)                              */
int mfs_pcg2d_apply(mfs_pcg2d* h, const void* v, void* out, mfs_stream stream);
int mfs_pcg2d_solve(mfs_pcg2d* h, double tol, int64_t max_iter, int64_t check_every,
                    mfs_stream stream, int64_t* iters_host);
int mfs_pcg2d_poll(mfs_pcg2d* h, mfs_stream stream, int64_t* iters_host, int* done_host,
                   double* delta_host, double* alpha_host, double* beta_host);
int64_t mfs_pcg2d_history(mfs_pcg2d* h, double* out_host, int64_t cap, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Viscosity, 2D -- reference solver/ViscosityCGSolver2D.py                      */
/* ------------------------------------------------------------------------- */
/* Quirks of the 2D reference kept as they are: a face sample is solid where sphi <= 0 (3D: < 0); boundary faces
 * (x == 0, x >= shape[0]-1, y == 0, y >= shape[1]-1 of each component's own array) of b / out are never written;
 * `vol` is lvol / (cell_vol * 0.125) with cell_vol the cell area (:269).  `sv` is never read (not an argument).  */
/* replaces initialize_solver -- solver/ViscosityCGSolver2D.py:6-103,222-229 */
int mfs_visc_rhs2d(const int64_t gres[2], double scale, double mu, const void* vx, const void* vy, int v_dt,
                   const void* sphi, int sphi_dt, const void* vol, int vol_dt, void* b_x, void* b_y, int b_dt,
                   mfs_stream stream);
/* replaces matvecmul -- solver/ViscosityCGSolver2D.py:105-207,231-238 */
int mfs_visc_apply2d(const int64_t gres[2], double scale, double mu, const void* vx, const void* vy, int v_dt,
                     void* out_x, void* out_y, int out_dt, const void* sphi, int sphi_dt, const void* vol, int vol_dt,
                     mfs_stream stream);
/* replaces apply_viscosity -- solver/ViscosityCGSolver2D.py:209-220,240-244 (in place on vx, vy: faces of cells
 * 1 <= x <= Nx-1, 1 <= y <= Ny-1 whose sample is > 0)                                                        */
int mfs_visc_writeback2d(const int64_t gres[2], void* vx, void* vy, int v_dt, const void* out_x, const void* out_y,
                         int out_dt, const void* sphi, int sphi_dt, mfs_stream stream);
/* the CG loop solver/ViscosityCGSolver2D.py:266-315.  The five CG vectors are FLAT arrays of mfs_vcg2d_dofs()
 * elements laid out [ x-faces (Nx+1,Ny) | y-faces (Nx,Ny+1) ].  mfs_vcg2d_solve starts from x as bound (x = v,
 * not zeroed: r0 = b - A v) and returns MFS_NOT_CONVERGED after max_iter iterations (the reference raises
 * ValueError there, before apply_viscosity).                                                              */
typedef struct mfs_vcg2d mfs_vcg2d;
size_t mfs_vcg2d_workspace_bytes(const int64_t gres[2], int dt);
int64_t mfs_vcg2d_dofs(const int64_t gres[2]);
int mfs_vcg2d_create(mfs_vcg2d** out_host, const int64_t gres[2], int dt,
                     void* workspace, size_t workspace_bytes, mfs_stream stream);
int mfs_vcg2d_destroy(mfs_vcg2d* h);
/* once per solve: the sphi tests of every face -> class bits, the doubled-grid `vol` -> four fp64 parity planes */
int mfs_vcg2d_setup(mfs_vcg2d* h, double scale, double mu, const void* sphi, int sphi_dt,
                    const void* vol, int vol_dt, mfs_stream stream);
int mfs_vcg2d_bind(mfs_vcg2d* h, void* b, void* x, void* d, void* r, void* q);
/* out = A v on flat vectors (the loop's stencil launch; bit-identical to mfs_visc_apply2d, boundary faces untouched) */
int mfs_vcg2d_apply(mfs_vcg2d* h, const void* v, void* out, mfs_stream stream);
int mfs_vcg2d_solve(mfs_vcg2d* h, double tol, int64_t max_iter, int64_t check_every,
                    mfs_stream stream, int64_t* iters_host);
int mfs_vcg2d_poll(mfs_vcg2d* h, mfs_stream stream, int64_t* iters_host, int* done_host,
                   double* delta_host, double* alpha_host, double* beta_host);
int64_t mfs_vcg2d_history(mfs_vcg2d* h, double* out_host, int64_t cap, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Notebook grid kernels that bracket the two solves    */
/* ------------------------------------------------------------------------- */
/* replaces `extrapolate(gres, num_iter, vx, vy, vz, mx, my, mz)` -- 3D_viscous_fluid_sim.ipynb code cell 7
 * (call site ipynb:4652): validity = grid mass > 0.  Workspace as for mfs_visc_extrapolate3d.          */
int mfs_grid_extrapolate3d(const int64_t gres[3], int num_iter, void* vx, void* vy, void* vz, int v_dt,
                           const void* mx, const void* my, const void* mz, int m_dt,
                           void* workspace, size_t workspace_bytes, mfs_stream stream);
/* replaces the three kernels of `apply_boundary_condition(g, solid, dx)` -- code cell 5 (call site
 * ipynb:4655): writes the free-slip corrections dv_x, dv_y, dv_z (the caller adds them to the velocities) */
int mfs_grid_boundary_condition3d(const int64_t gres[3], const void* gvx, const void* gvy, const void* gvz, int v_dt,
                                  const void* gmx, const void* gmy, const void* gmz, int m_dt,
                                  const void* sphi, int sphi_dt, const void* sv, int sv_dt, double dx,
                                  void* dvx, void* dvy, void* dvz, int dv_dt, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Notebook particle <-> grid transfers                  */
/* ------------------------------------------------------------------------- */
/* Particle arrays: px, pv, pca are (P,3) row-major, pm is (P).  The reference kernels keep float32
 * locals whatever the array dtypes; `bound_min` and `grid_bias` are therefore used at float32 precision
 * and `cell_size` at float64 -- the notebook's container dtypes (code cell 9) -- so that base indices and
 * weights equal the reference's.  Scatters use fp atomics (order unspecified, as in the reference).     */
/* replaces p2g_particle -- 3D_viscous_fluid_sim.ipynb code cell 2: APIC scatter of mass and momentum of velocity
 * component `axis` to its face array (shape gres + e_axis; indices are clamped to gres - 1 as in the reference) */
int mfs_p2g_scatter3d(const int64_t gres[3], const double bound_min[3], const double cell_size[3],
                      const double grid_bias[3], int axis, const void* px, int px_dt, const void* pm, int pm_dt,
                      const void* pv, int pv_dt, const void* pca, int pca_dt, int64_t num_particles,
                      void* gm, void* gv, int g_dt, mfs_stream stream);
/* Tile-sorted forms of the three scatters (the build's own; same results up to the order of the fp atomics, which the
 * reference leaves unspecified too).  mfs_particle_tile_sort3d buckets the particles by the tile of 8^3 CELLS their cell
 * (floor((x - bound_min) / cell_size), clamped to gres) lies in: perm[num_particles] = particle indices tile by tile,
 * tile_start[mfs_particle_tiles3d(gres) + 1] = segment starts; work = 2 * tiles + num_particles int32 of scratch.  The
 * *_tiled entry points take that order and run one workgroup per tile with the tile's nodes in LDS (csrc/mfs_particles.hip);
 * they stay correct when particles have moved since the sort (contributions outside the staged nodes take the global
 * atomic), only slower.  p2g_particle / compute_fls_kernel / compute_fluid_volume_kernel: ipynb code cells 2, 4, 6. */
int64_t mfs_particle_tiles3d(const int64_t gres[3]);
int mfs_particle_tile_sort3d(const int64_t gres[3], const double bound_min[3], const double cell_size[3], const void* px,
                             int px_dt, int64_t num_particles, int32_t* perm, int32_t* tile_start, int32_t* work,
                             mfs_stream stream);
int mfs_p2g_scatter3d_tiled(const int64_t gres[3], const double bound_min[3], const double cell_size[3],
                            const double grid_bias[3], int axis, const void* px, int px_dt, const void* pm, int pm_dt,
                            const void* pv, int pv_dt, const void* pca, int pca_dt, int64_t num_particles,
                            const int32_t* perm, const int32_t* tile_start, void* gm, void* gv, int g_dt, mfs_stream stream);
int mfs_fluid_levelset3d_tiled(const int64_t gres[3], const double bound_min[3], const double cell_size[3], double radius,
                               const void* px, int px_dt, int64_t num_particles, const int32_t* perm,
                               const int32_t* tile_start, void* phi, int phi_dt, mfs_stream stream);
/* initialize_density_kernel (solver/DensityCGSolver3D.py:8-36) on the same tile order */
int mfs_density_splat3d_tiled(const int64_t gres[3], const double bound_min[3], const double cell_size[3], const void* px,
                              int px_dt, const void* pm, int pm_dt, double pvol, int64_t num_particles, const int32_t* perm,
                              const int32_t* tile_start, void* gm, void* gvol, int g_dt, mfs_stream stream);
int mfs_fluid_volume3d_tiled(const int64_t vres[3], const double bound_min[3], const double cell_size[3], const void* px,
                             int px_dt, double pvol, int64_t num_particles, const int32_t* perm, const int32_t* tile_start,
                             void* gvol, int g_dt, mfs_stream stream);
/* replaces p2g_grid -- code cell 2: gv /= gm wherever gm > 0 (count = elements of the face array) */
int mfs_p2g_normalize3d(int64_t count, const void* gm, void* gv, int g_dt, mfs_stream stream);
/* replaces g2p_particle -- code cell 3: pv[:, axis] and the affine row pca[:, :] from the face array gv */
int mfs_g2p_gather3d(const int64_t gres[3], const double bound_min[3], const double cell_size[3],
                     const double grid_bias[3], int axis, const void* px, int px_dt, void* pv, int pv_dt,
                     void* pca, int pca_dt, int64_t num_particles, const void* gv, int g_dt, mfs_stream stream);
/* replaces compute_fls_kernel -- code cell 4: phi = min(phi, |cell centre - x| - radius) over the 5^3 cells around
 * each particle (atomic min).  The caller pre-fills phi (the notebook: `ls.phi[:] = gdx * 3`).               */
int mfs_fluid_levelset3d(const int64_t gres[3], const double bound_min[3], const double cell_size[3], double radius,
                         const void* px, int px_dt, int64_t num_particles, void* phi, int phi_dt, mfs_stream stream);
/* replaces compute_fluid_volume_kernel + constrain_fluid_volume_kernel -- code cell 6: trilinear splat of the
 * particle volume onto the nodes of the array `gvol` (shape vres, spacing cell_size), then min(., cell volume).
 * The caller zeroes gvol first (the notebook: `fv.vol[:] = 0.0`).                                            */
int mfs_fluid_volume3d(const int64_t vres[3], const double bound_min[3], const double cell_size[3],
                       const void* px, int px_dt, double pvol, int64_t num_particles, void* gvol, int g_dt,
                       mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Rigid-body signed distances -- reference solver/sdf3D.py */
/* ------------------------------------------------------------------------- */
/* rb_d: num_bodies x 10 x 4 float64 (generate_rb :277-305): row 0 = [type code, parameters] (code // 2:
 * 0 sphere, 1 box, 2 cylinder; odd = flipped), rows 1-4 translation, rows 5-8 rotation, row 9 velocity.
 * position / vel are (P,3) row-major.                                                                   */
/* replaces evaluate_kernel -- solver/sdf3D.py:218-239 (the caller zeroes vel first, as evaluate() :266 does) */
int mfs_sdf_evaluate3d(const void* rb_d, int64_t num_bodies, const void* position, int pos_dt, int64_t num_positions,
                       void* sd, int sd_dt, void* vel, int vel_dt, mfs_stream stream);
/* evaluate_kernel on the nodes of a regular grid, for solids that move (no reference counterpart).  The position of
 * index i along an axis is get_grid_pos' (notebook code cell 9): (double)(float)bound_min + (double)((float)i +
 * (float)bias) * cell_size, multiply and add rounded separately.  sd: res[0] x res[1] x res[2] in C order, vel the same
 * with 3 components last; EVERY vel element is written: 0 where sd > 0 (or no bodies), else the winning body's row 9 --
 * plus w x (pos - T) when rb_w (num_bodies x 3 float64, rad/s; may be null = all zero) is given.  Extents up to 2^30. */
int mfs_sdf_evaluate_grid3d(const void* rb_d, int64_t num_bodies, const void* rb_w, const int64_t res[3],
                            const double bound_min[3], const double bias[3], const double cell_size[3], void* sd,
                            int sd_dt, void* vel, int vel_dt, mfs_stream stream);
/* replaces project_kernel -- solver/sdf3D.py:241-258 (in place on position) */
int mfs_sdf_project3d(const void* rb_d, int64_t num_bodies, void* position, int pos_dt, int64_t num_positions,
                      mfs_stream stream);

/* 2D -- reference solver/sdf2D.py.  rb_d: num_bodies x 8 x 3 float64 (generate_rb :221-252): row 0 = [type code,
 * parameters] (code // 2: 0 sphere, 1 box; odd = flipped), rows 1-3 translation, rows 4-6 rotation, row 7 velocity.
 * position / vel are (P,2) row-major.                                                                            */
/* replaces evaluate_kernel -- solver/sdf2D.py:146-169 (the caller zeroes vel first, as evaluate() :190 does) */
int mfs_sdf_evaluate2d(const void* rb_d, int64_t num_bodies, const void* position, int pos_dt, int64_t num_positions,
                       void* sd, int sd_dt, void* vel, int vel_dt, mfs_stream stream);
/* mfs_sdf_evaluate_grid3d one dimension down: sd res[0] x res[1], vel with 2 components last; rb_w: num_bodies float64
 * (may be null); the surface velocity is (v0 - w r1, v1 + w r0) with r = pos - T.                                  */
int mfs_sdf_evaluate_grid2d(const void* rb_d, int64_t num_bodies, const void* rb_w, const int64_t res[2],
                            const double bound_min[2], const double bias[2], const double cell_size[2], void* sd,
                            int sd_dt, void* vel, int vel_dt, mfs_stream stream);
/* replaces project_kernel -- solver/sdf2D.py:171-183 (in place on position) */
int mfs_sdf_project2d(const void* rb_d, int64_t num_bodies, void* position, int pos_dt, int64_t num_positions,
                      mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* The 2D time step: particle <-> grid transfers and grid kernels (csrc/mfs_notebook2d.hip) */
/* ------------------------------------------------------------------------- */
/* The reference has no 2D driver.  These are the 3D entry points above one dimension down: the same float32 locals
 * and the same order of operations with the z factor / z terms removed, so a 3D run whose particles lie on a
 * cell-centre plane and whose fields do not vary in z gives the bits of the 2D run on that plane.  Particle arrays:
 * px, pv, pca are (P,2) row-major, pm is (P).  Face arrays: x (Nx+1,Ny), y (Nx,Ny+1); doubled grid (2Nx+1,2Ny+1);
 * sv (2Nx+1,2Ny+1,2).  num_particles == 0 returns MFS_OK without a launch.  p2g's division is dimension-free:
 * mfs_p2g_normalize3d.                                                                                          */
/* mfs_p2g_scatter3d in 2D: APIC scatter of mass and momentum of component `axis` (0, 1) to its face array; four
 * corners, indices clamped to gres - 1                                                                          */
int mfs_p2g_scatter2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2],
                      const double grid_bias[2], int axis, const void* px, int px_dt, const void* pm, int pm_dt,
                      const void* pv, int pv_dt, const void* pca, int pca_dt, int64_t num_particles,
                      void* gm, void* gv, int g_dt, mfs_stream stream);
/* mfs_g2p_gather3d in 2D: pv[:, axis] and the affine row pca[:, 0:2] from the face array gv */
int mfs_g2p_gather2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2],
                     const double grid_bias[2], int axis, const void* px, int px_dt, void* pv, int pv_dt,
                     void* pca, int pca_dt, int64_t num_particles, const void* gv, int g_dt, mfs_stream stream);
/* mfs_fluid_levelset3d in 2D: phi = min(phi, |cell centre - x| - radius) over the 5^2 cells around each particle.
 * The caller pre-fills phi.                                                                                     */
int mfs_fluid_levelset2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2], double radius,
                         const void* px, int px_dt, int64_t num_particles, void* phi, int phi_dt, mfs_stream stream);
/* mfs_fluid_volume3d in 2D: bilinear splat of the particle volume (an area) onto the nodes of `gvol` (shape vres,
 * spacing cell_size), then min(., cell_size[0] * cell_size[1]).  The caller zeroes gvol first.                  */
int mfs_fluid_volume2d(const int64_t vres[2], const double bound_min[2], const double cell_size[2],
                       const void* px, int px_dt, double pvol, int64_t num_particles, void* gvol, int g_dt,
                       mfs_stream stream);
/* mfs_grid_extrapolate3d in 2D: num_iter Jacobi sweeps of the 4-neighbour average into interior faces with
 * mass <= 0; a face filled by one sweep is valid for the next; a sweep reads the previous sweep's values only
 * (ping-pong buffers in `workspace`, 256-byte aligned); array-boundary faces are untouched                      */
size_t mfs_grid_extrapolate2d_workspace_bytes(const int64_t gres[2], int v_dt);
int mfs_grid_extrapolate2d(const int64_t gres[2], int num_iter, void* vx, void* vy, int v_dt,
                           const void* mx, const void* my, int m_dt,
                           void* workspace, size_t workspace_bytes, mfs_stream stream);
/* mfs_grid_boundary_condition3d in 2D: the free-slip corrections dv_x, dv_y (the caller adds them); 0 on
 * array-boundary faces and where sphi / dx >= 1                                                                 */
int mfs_grid_boundary_condition2d(const int64_t gres[2], const void* gvx, const void* gvy, int v_dt,
                                  const void* gmx, const void* gmy, int m_dt,
                                  const void* sphi, int sphi_dt, const void* sv, int sv_dt, double dx,
                                  void* dvx, void* dvy, int dv_dt, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Surface extraction (csrc/mfs_surface.hip; DESIGN.md "Surface extraction")  */
/* ------------------------------------------------------------------------- */
/* What the notebook does with a CPU marching-cubes routine after scene set-up and after the run, on the device: an
 * indexed, welded, consistently oriented triangle mesh of {phi < level} by marching tetrahedra over the six Kuhn
 * tetrahedra of every lattice cube.  No atomics: the output is a function of the field alone.
 * phi: shape[0] x shape[1] x shape[2] in C order, every extent >= 2; a node is inside iff phi < level (NaN never is).
 * closed != 0: the lattice is the array plus one virtual layer of samples of value `outside` (> level) on every side;
 * nothing is copied.  The lattice may hold at most 2^31 - 1025 nodes.
 * Two passes.  _count classifies and leaves the totals in the first 16 bytes of `workspace` (DEVICE memory, 256-byte
 * aligned): int64 vertices, int64 triangles.  The caller reads them, allocates, and calls _fill with the SAME shape, phi,
 * level, closed, outside and workspace.  _fill reads the totals back itself (it drains `stream`), returns MFS_E_INVALID
 * without a launch when a capacity is smaller than its total or a total does not fit int32 (3 x triangles included),
 * and never writes past a capacity.  Totals of zero: MFS_OK, nothing written, the array pointers may be null.
 * vertices: cap_vertices x 3 float32, node p's vertices in C order of the lattice, its edges to p + (1,0,0) (0,1,0)
 * (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1) in that order, at origin + (p + t s) * spacing (fp64 arithmetic, rounded on
 * the store); faces: cap_faces x 3 int32, right-hand normal from inside to outside; normals: cap_vertices x 3 float32 or
 * null -- the normalised gradient of phi (central differences, one-sided at the lattice border) interpolated along
 * the edge.                                                                                                      */
size_t mfs_surface3d_workspace_bytes(const int64_t shape[3], int closed);
int mfs_surface3d_count(const int64_t shape[3], const void* phi, int phi_dt, double level, int closed, double outside,
                        void* workspace, size_t workspace_bytes, mfs_stream stream);
int mfs_surface3d_fill(const int64_t shape[3], const void* phi, int phi_dt, double level, int closed, double outside,
                       const double origin[3], const double spacing[3], void* workspace, size_t workspace_bytes,
                       void* vertices, int64_t cap_vertices, void* faces, int64_t cap_faces, void* normals,
                       mfs_stream stream);
/* The same one dimension down: every lattice square cut along its (1,1) diagonal, node p's edges to p + (1,0) (0,1)
 * (1,1); vertices cap_vertices x 2 float32; segments cap_segments x 2 int32, the inside on the left of (u, v).     */
size_t mfs_contour2d_workspace_bytes(const int64_t shape[2], int closed);
int mfs_contour2d_count(const int64_t shape[2], const void* phi, int phi_dt, double level, int closed, double outside,
                        void* workspace, size_t workspace_bytes, mfs_stream stream);
int mfs_contour2d_fill(const int64_t shape[2], const void* phi, int phi_dt, double level, int closed, double outside,
                       const double origin[2], const double spacing[2], void* workspace, size_t workspace_bytes,
                       void* vertices, int64_t cap_vertices, void* segments, int64_t cap_segments, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Triangle-mesh solids (csrc/mfs_meshsdf.hip; DESIGN.md "Triangle-mesh solids") */
/* ------------------------------------------------------------------------- */
/* No reference counterpart: the reference's scenes are spheres, boxes and cylinders.  Additions: the ABI version stays.
 * A lattice is shape[0] x shape[1] x shape[2] nodes in C order (every extent >= 2, fewer than 2^31 nodes), node (i,j,k)
 * at origin + (i,j,k) * spacing.  triangles: num_triangles x 9 float32, the three corners of each.
 * _distance3d: phi (float32) = the exact distance of every node to the nearest triangle, fp32 arithmetic, squared
 * distances compared and one square root at the end; zero-area triangles are skipped.  One workgroup owns a brick of
 * 4 x 8 x 8 nodes; cull != 0 drops, per brick, the triangles that provably cannot carry a minimum there -- bitwise the
 * same phi as cull == 0.  survivors: null, or mfs_meshsdf_bricks3d(shape) int32, the triangles each brick looped over.
 * _sign3d: phi must hold _distance3d's output (>= 0).  Nodes inside the closed surface get the sign bit, by the parity
 * of crossings of the ray along axis 0, ties broken half-open; odd_columns: shape[1] x shape[2] int32, 1 where a
 * column's total crossing count is odd (the surface is not closed there).  No atomics in either.                    */
int64_t mfs_meshsdf_bricks3d(const int64_t shape[3]);
int mfs_meshsdf_distance3d(const int64_t shape[3], const double origin[3], double spacing, const void* triangles,
                           int64_t num_triangles, int cull, void* phi, void* survivors, mfs_stream stream);
int mfs_meshsdf_sign3d(const int64_t shape[3], const double origin[3], double spacing, const void* triangles,
                       int64_t num_triangles, void* phi, void* odd_columns, mfs_stream stream);
/* Mesh bodies: num_bodies <= 16 rows of the packed (10,4) float64 layout of mfs_sdf_* (mesh_rb: translation rows 1-4,
 * rotation rows 5-8, velocity row 9; row 0 is not read), each with a float32 signed-distance volume in its own frame.
 * The *_host arrays are HOST memory, read before the launch: volumes_host[i] the DEVICE pointer of body i's volume,
 * extents_host 3 int64 per body, origins_host 3 doubles per body, spacings_host one double per body.  A volume is
 * sampled trilinearly at x_b = R^T (x - T); outside it: the sample at the clamped point plus the distance to its box.
 * _union_grid3d: the grid of mfs_sdf_evaluate_grid3d (same position rule).  For every node and every body in turn:
 * d < sd -> sd = d and vel = (d <= 0 ? row 9 + w x (x - T) : 0); rb_w: num_bodies x 3 float64 or null.  sd / vel hold
 * the level set the bodies are united with on entry; nodes no body wins are not written.
 * _project3d: in place; for every body in turn a position with sampled d < 0 moves by -d * R n, n the normalised gradient
 * of the sampled volume (central differences one spacing apart where it vanishes; still zero: left alone).          */
int mfs_mesh_union_grid3d(const void* mesh_rb, const void* rb_w, int64_t num_bodies, const void* const* volumes_host,
                          const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                          const int64_t res[3], const double bound_min[3], const double bias[3],
                          const double cell_size[3], void* sd, int sd_dt, void* vel, int vel_dt, mfs_stream stream);
int mfs_mesh_project3d(const void* mesh_rb, int64_t num_bodies, const void* const* volumes_host,
                       const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                       void* position, int pos_dt, int64_t num_positions, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Liquid skin (csrc/mfs_skin.hip; DESIGN.md "Liquid skin")                    */
/* ------------------------------------------------------------------------- */
/* No reference counterpart: the reference plots points.  Additions: the ABI version stays.
 * Zhu & Bridson's particle surface on a lattice (shape, origin, spacing as above: every extent >= 2, fewer than 2^31
 * nodes, scalar spacing h).  With d_i = x_i - x, w_i = max(1 - |d_i|^2 / R^2, 0)^3 and W = sum w_i, a node x gets
 * phi = | sum w_i d_i | / W - r where W > 0 and the background (float) (R - r) where W == 0; float32 out, fp32
 * arithmetic on coordinates taken relative to the node's brick in fp64 first.  0 < r < R <= 4 h.
 * One workgroup owns a brick of 4 x 8 x 8 nodes and gathers from bins: bin (c0, c1, c2) of the (nb0 + 2) x (nb1 + 2) x
 * (nb2 + 2) bins (nb = ceil(shape / (4, 8, 8)), C order) holds the particles of brick (c0 - 1, c1 - 1, c2 - 1)'s cell,
 * [origin + (c - 1) E h, origin + c E h) along each axis, E the brick's edge in nodes.
 * _bricks3d / _bins3d: their numbers (0 for a bad shape).
 * _keys3d: keys[p] (int32) = particle p's bin, or _bins3d(shape) when it lies outside every bin or is not finite.
 * particles: num_particles x 3, float32 or float64 (p_dt), fewer than 2^31.
 * _field3d: sorted_particles are the particles in ascending order of key; bin_starts: _bins3d(shape) + 1 int32, the
 * index of the first particle with key >= b (so the last entry counts the binned ones; the rest are never read).  The
 * caller's order inside a bin is the order of summation: a stable sort makes phi a function of the input alone.  No
 * atomics.  survivors: null, or _bricks3d(shape) int32, the particles each brick's nodes looped over.              */
int64_t mfs_skin_bricks3d(const int64_t shape[3]);
int64_t mfs_skin_bins3d(const int64_t shape[3]);
int mfs_skin_keys3d(const int64_t shape[3], const double origin[3], double spacing, const void* particles, int p_dt,
                    int64_t num_particles, void* keys, mfs_stream stream);
int mfs_skin_field3d(const int64_t shape[3], const double origin[3], double spacing, double radius, double influence,
                     const void* sorted_particles, int p_dt, int64_t num_particles, const void* bin_starts, void* phi,
                     void* survivors, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Liquid seeding (csrc/mfs_seed.hip; DESIGN.md "Seeding liquid from shapes")  */
/* ------------------------------------------------------------------------- */
/* No reference counterpart: the reference fills boxes on the host.  Additions: the ABI version stays.
 * Sites: shape[0] x shape[1] x shape[2] (each 1 .. 2^30), site (i,j,k) with the 64-bit index s = (i * n1 + j) * n2 + k.
 * Its particle sits at x_a = origin_a + ((i_a + 0.5) + jitter * u_a) * spacing in float64, every operation rounded on its
 * own, jitter in [0, 1], u_a = (h_a >> 8) * 2^-24 - 0.5 with, mix(x) being x ^= x >> 16, x *= 0x7feb352d, x ^= x >> 15,
 * x *= 0x846ca68b, x ^= x >> 16 on uint32: h = mix(seed_lo), h = mix(h ^ seed_hi), h = mix(h ^ s_lo), h = mix(h ^ s_hi),
 * h_a = mix(h + (a + 1) * 0x9E3779B9).
 * Shapes: num_include >= 1 and num_exclude >= 0, at most 16 together, includes first.  The *_host arrays are HOST memory,
 * read before the launch: volumes_host[i] the DEVICE pointer of shape i's volume, dtypes_host[i] its element type
 * (MFS_F32 / MFS_F64), extents_host 3 int64 per shape (each >= 2, fewer than 2^31 nodes), origins_host 3 doubles,
 * spacings_host one double, poses_host 12 doubles per shape: the rotation R row by row, then the translation T.  A
 * shape's value at x is its volume sampled trilinearly in float64 at R^T (x - T), as mfs_mesh_union_grid3d samples;
 * outside the volume: the sample at the clamped point plus the distance to its box.
 * A site is kept iff (min over includes) < 0 and (min over excludes) > clearance, both strict; a NaN sample keeps nothing.
 * One workgroup owns 256 consecutive sites; _blocks3d: their number (0 for a bad shape), at most 2^31 - 1 per call.
 * _count3d: counts (int32 per workgroup; may be null) = the sites it keeps; masks (4 uint64 per workgroup; may be null;
 * not both) = the ballots of its four waves, bit l of word w for site 256 b + 64 w + l.
 * _fill3d: offsets (int64 per workgroup) = the exclusive scan of counts.  The kept sites' positions (pos_dt; float32 is
 * the float64 value rounded once) go to rows offsets[b] + rank of `positions` (capacity x 3), rank counting the kept
 * sites of the workgroup in ascending s, and s itself to `sites` (int64, may be null).  Rows >= capacity are not stored.
 * No atomics: the output is in ascending s and two calls store the same bits.                                      */
int64_t mfs_seed_blocks3d(const int64_t shape[3]);
int mfs_seed_count3d(const int64_t shape[3], const double origin[3], double spacing, double jitter, uint64_t seed,
                     int64_t num_include, int64_t num_exclude, const void* const* volumes_host, const int* dtypes_host,
                     const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                     const double* poses_host, double clearance, void* counts, void* masks, mfs_stream stream);
int mfs_seed_fill3d(const int64_t shape[3], const double origin[3], double spacing, double jitter, uint64_t seed,
                    const void* masks, const void* offsets, void* positions, int pos_dt, void* sites, int64_t capacity,
                    mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Ray-marched images (csrc/mfs_render.hip; DESIGN.md "Rendering")             */
/* ------------------------------------------------------------------------- */
/* No reference counterpart: the reference hands its points to a notebook widget.  Additions: the ABI version stays.
 * Shapes: 1 to 16, described by the *_host arrays of mfs_seed_count3d (HOST memory, read before the launch).  Shape i at a
 * world point x is sampled at the body point R^T (x - T) exactly as there, but shows only inside its own box: with
 * u_a = (xb_a - origin_a) / spacing, the value is the trilinear sample if 0 <= u_a <= n_a - 1 on all axes and +inf
 * otherwise.  F(x) = min over the shapes, taken with a strict < from +inf: the id is the first shape that attains it and a
 * NaN sample is passed over.
 * camera: 14 HOST doubles, eye[3], f[3], r[3], u[3], half_w, half_h (an orthonormal frame; half the image plane's extents
 * at unit distance, or in world units when `ortho`).  Pixel (i, j), row i from the top: sx = ((j + 0.5) * (2 / W) - 1) *
 * half_w, sy = (1 - (i + 0.5) * (2 / H)) * half_h; perspective: o = eye, v = (f + sx r) + sy u, d = v / |v|; orthographic:
 * o = (eye + sx r) + sy u, d = f.  width, height in 1 .. 16384.
 * March: sample k of num_steps (1 .. 65536) is at t_k = near + k * step, x_k = o + t_k d.  The hit is the smallest k with
 * F(x_k) < 0; with a = F(x_{k-1}), b = F(x_k): depth = (t_k - step) + step * (a / (a - b)) if k > 0 and a is finite, else
 * t_k.  The normal is the hit shape's central difference over +-0.5 spacing along the world axes at o + depth d, sampled
 * as mfs_seed_count3d samples (clamp plus distance outside the box) and normalised; -d where its length is 0 or not finite.
 * All arithmetic on the ray is float64, every operation rounded on its own.
 * Outputs (DEVICE, height x width, C order): depth float64 (+inf at a miss), normal 3 x float32 (0 at a miss), shape_id
 * int32 (-1), steps int32 (the hit k; -1); evals (may be null) int32, the shape samples the pixel's lane evaluated in
 * its walk.
 * bricks_host[i]: DEVICE array of _brick_count3d(extents) float64 from _bricks3d, C order over ceil((n - 1) / 8) bricks
 * per axis: the minimum over the nodes 8 b .. min(8 b + 8, n - 1) of brick b, -inf if one of them is NaN.  With skip != 0
 * the march passes over samples of a shape that lie before the ray's entry into the shape's box, after its exit, or in
 * a brick whose minimum is > 0; the outputs, evals apart, are the same bits as with skip == 0 (bricks_host may then be
 * null), which evaluates every shape at every sample up to the hit.
 * _shade3d: rgb (DEVICE, height x width x 3 uint8) = floor(255 c + 0.5), c = albedo[id] * (0.25 + 0.75 * max(0, n . l)),
 * l = -d of the pixel's ray, or light_host (3 HOST doubles, the unit vector towards the light) when not null;
 * albedo_host: num_colors (1 .. 16) x 3 HOST doubles; background_host: 3 HOST ints in 0 .. 255, stored where id < 0 or
 * id >= num_colors.  near / step / num_steps play no part in it.                                                   */
int64_t mfs_render_brick_count3d(const int64_t extents[3]);
int mfs_render_bricks3d(const void* volume, int dtype, const int64_t extents[3], void* bricks, mfs_stream stream);
int mfs_render_march3d(const double* camera, int ortho, int64_t width, int64_t height, double near, double step,
                       int64_t num_steps, int64_t num_shapes, const void* const* volumes_host, const int* dtypes_host,
                       const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                       const double* poses_host, const void* const* bricks_host, int skip, void* depth, void* normal,
                       void* shape_id, void* steps, void* evals, mfs_stream stream);
int mfs_render_shade3d(const double* camera, int ortho, int64_t width, int64_t height, const void* normal,
                       const void* shape_id, int64_t num_colors, const double* albedo_host, const int* background_host,
                       const double* light_host, void* rgb, mfs_stream stream);

/* Paths: shadows, a refracting liquid, supersampling (tests/render_paths_numpy.py restates every operation).  Additions:
 * the ABI version stays.
 * _bricks_max3d: as _bricks3d, the MAXIMUM over each brick's nodes, +inf if one of them is NaN.
 * _paths3d: one ray per pixel of the width x height image (for s x s supersampling pass s times the extents and the
 * same camera: half_w and half_h do not change).  A segment march generalises the march above to any ray and a medium:
 * samples x_k = o + (t0 + k step) d, t0 = near for the camera's ray and 0 for every later segment; in air the rule is
 * the one above, over the shapes the segment includes; inside shape m (the medium) shape m counts negated and -inf outside
 * its box, so the hit with id m is the exit.  The normal is the hit shape's un-negated central difference, in float64.
 * materials_host: num_shapes x 8 HOST doubles: kind (0 opaque, 1 liquid), colour r g b in 0 .. 1, ior in (1, 4], absorb
 * r g b >= 0 per world unit (the last four are read of a liquid only).  light_host: 3 HOST doubles, the unit vector
 * towards a directional light; null: l = -d of the camera's ray.  background_host: 3 HOST ints in 0 .. 255, bg = value / 255.
 * A path runs at most four marches in fixed slots: 0 the camera's ray (num_steps samples); 1 inside the liquid
 * (inside_steps); 2 after the exit (num_steps); 3 the shadow ray of the surface finally shaded (shadow_steps, over the
 * opaque shapes only; run iff shadows != 0).  Slot 0 misses: bg.  A surface finally shaded (an opaque shape in slot 0, 1
 * or 2, or any shape met in slot 2, or another liquid met in slot 1) at x with normal n gives
 * albedo * (0.25 + 0.75 * (vis * max(0, n32 . l))), n32 = n rounded to float32 as _march3d stores it, vis = 0 if the
 * shadow march from x + bias n along l hits, else 1.  A liquid hit in slot 0: n faces the ray (negated if d . n > 0),
 * c = -d . n, r0 = ((ior - 1) / (ior + 1))^2, R = r0 + (1 - r0) (1 - c)^5 by multiplications; eta = 1 / ior,
 * k = 1 - eta^2 (1 - c^2), t = eta d + (eta c - sqrt(k)) n, normalised; slot 1 starts at x - bias n along t.  Its miss
 * leaves the liquid's colour behind, with L = inside_steps * step; a surface met leaves its shaded colour, with L = the
 * segment's depth; the exit (id = the medium, L = depth) refracts the same way with eta = ior and n facing the ray:
 * k < 0 is total internal reflection and leaves the liquid's colour, otherwise slot 2 starts at x - bias n; its miss
 * leaves bg.  colour = R bg + ((1 - R) exp(-(absorb L))) behind.
 * Outputs (DEVICE, C order): color height x width x 3 float64; steps and shape_id height x width x 4 int32 per slot
 * (-2: slot not run, -1: a miss); length height x width float64 (L; 0 without a liquid hit); evals (may be null) int32.
 * bricks_max_host[i]: read for liquid shapes only.  skip == 0 gives the same bits in every output but evals.
 * _resolve3d: rgb (DEVICE, height x width x 3 uint8) from color (DEVICE, (samples height) x (samples width) x 3 float64):
 * the samples^2 colours of a pixel summed in row-major order, divided by samples^2, floor(255 c + 0.5) held in 0 .. 255;
 * samples in 1 .. 4.                                                                                              */
int mfs_render_bricks_max3d(const void* volume, int dtype, const int64_t extents[3], void* bricks, mfs_stream stream);
int mfs_render_paths3d(const double* camera, int ortho, int64_t width, int64_t height, double near, double step,
                       int64_t num_steps, int64_t num_shapes, const void* const* volumes_host, const int* dtypes_host,
                       const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                       const double* poses_host, const void* const* bricks_host, const void* const* bricks_max_host,
                       int skip, const double* materials_host, const double* light_host, const int* background_host,
                       int shadows, double bias, int64_t shadow_steps, int64_t inside_steps, void* color, void* steps,
                       void* shape_id, void* length, void* evals, mfs_stream stream);
int mfs_render_resolve3d(const void* color, int64_t width, int64_t height, int samples, void* rgb, mfs_stream stream);

/* ------------------------------------------------------------------------- */
/* Particle data at points (csrc/mfs_attrib.hip; DESIGN.md "Particle data at points") */
/* ------------------------------------------------------------------------- */
/* No reference counterpart.  Additions: the ABI version stays.
 * Particles x_i (P x 3, float32 / float64) carry values a_i (P x C, C in 1 .. 4, float32 / float64, rounded to float32
 * on load); queries y_q (Q x 3, float32 / float64); an influence radius R > 0.  With d = x_i - y_q, t = 1 - |d|^2 / R^2
 * and w_qi = t^3 where t > 0, otherwise 0 (strict: a particle exactly R away adds nothing), W_q = sum_i w_qi and
 * A_q = sum_i w_qi a_i / W_q where W_q > 0; where W_q == 0 every channel is `fill`.  A particle whose position is not
 * finite adds nothing, a non-finite value of a contributing particle propagates, a query that is not finite is
 * uncovered (weight 0, values fill).  fp32 arithmetic on coordinates taken relative to the query's bin in fp64 first.
 * Bins: a lattice of shape (m0, m1, m2) cubic bins of edge exactly R with float64 origin o; the bin of a position is
 * c_a = floor((x_a - o_a) / R) in float64, its key (c0 m1 + c1) m2 + c2, and m0 m1 m2 (the sentinel) for a position
 * outside the lattice or not finite.  At most 2^31 - 2 bins.  A query in bin c takes contributions from the 27 bins
 * around c and from nothing else (a particle within R whose own bin index rounds one bin further away is lost: its
 * weight is below 1e-15).  A query with the sentinel key is not touched: the caller stores fill and weight 0.
 * _bins3d: m0 m1 m2, or 0 when an extent is < 1 or the product exceeds 2^31 - 2.
 * _keys3d: keys (DEVICE, count int32) of `positions`; box_host: null, or 6 HOST doubles lo[3], hi[3]: a position outside
 * the closed box gets the sentinel as well.
 * _gather3d: sorted_particles / sorted_values: the particles and their values in a STABLE sort by key (the caller's
 * order inside a bin is the order of summation: the result is a function of the input alone; no atomics);
 * bin_starts: bins + 1 int32, the index of the first sorted particle with key >= b.  sorted_queries: the queries in a
 * stable sort by key, query_rows (int64) the row of `values` / `weight` each came from.  items: num_items x 3 int32
 * (key, first, count): the sorted queries first .. first + count - 1, count <= 256, all of bin `key`; one workgroup
 * each.  values: DEVICE num_queries x channels float32; weight: num_queries float32; tested: null, or num_items int32,
 * the particles each item's lanes looped over.
 * _shade_albedo3d: _shade3d with one change: a pixel with shape_id == albedo_id takes pixel_albedo (DEVICE, height x
 * width x 3 float32, in 0 .. 1) in place of albedo_host[albedo_id]; where a component of it is NaN the pixel keeps the
 * palette's colour.                                                                                                */
int64_t mfs_attrib_bins3d(const int64_t shape[3]);
int mfs_attrib_keys3d(const int64_t shape[3], const double origin[3], double influence, const double* box_host,
                      const void* positions, int p_dt, int64_t count, void* keys, mfs_stream stream);
int mfs_attrib_gather3d(const int64_t shape[3], const double origin[3], double influence, int channels, double fill,
                        const void* sorted_particles, int p_dt, const void* sorted_values, int v_dt, int64_t num_particles,
                        const void* bin_starts, const void* sorted_queries, int q_dt, const void* query_rows,
                        int64_t num_queries, const void* items, int64_t num_items, void* values, void* weight, void* tested,
                        mfs_stream stream);
int mfs_render_shade_albedo3d(const double* camera, int ortho, int64_t width, int64_t height, const void* normal,
                              const void* shape_id, int64_t num_colors, const double* albedo_host,
                              const int* background_host, const double* light_host, const void* pixel_albedo,
                              int64_t albedo_id, void* rgb, mfs_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* MFS_H */
