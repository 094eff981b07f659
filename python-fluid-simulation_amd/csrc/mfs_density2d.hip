// mfs_density2d.hip -- the once-per-solve kernels of DensityCGSolver2D on gfx950.
//
// Reference: solver/DensityCGSolver2D.py.  The solver's CG loop (:274-290) runs on the 2D pressure engine
// (mfs_pressure2d.hip, mfs_pcg2d_setup_density); its operator is the template of mfs_apply2d.h.  Here: the particle
// splat (:8-33), fix_volume (:35-57), the right-hand side (:59-83), the stateless operator apply (the module-level
// matvecmul :221-225), compute_displacement (:141-152) and the particle gather apply_displacement (:171-195).
// One thread per cell / particle, fastest index on the contiguous axis, fp64 arithmetic in the reference's order
// whatever the storage dtype.  Where 2D differs from mfs_density.hip (3D), it is the reference that differs:
//  * the splat writes gm only (the gvol scatter is commented out, :33);
//  * fix_volume reads lvol at nine doubled-grid samples (:41-45) instead of the splatted volume;
//  * the -y tap of the operator uses wy[x,y] (no counterpart of the 3D wz[z+1] quirk).
#include <math.h>

#include "mfs_apply2d.h"

// No FMA contraction in this file's own kernels: base indices, float32-rounded grid positions and weights must round
// where the reference's separate multiply and add round.  (The operator template of mfs_apply2d.h states its own
// contraction inside its body, so it compiles the same here and in the engine.)
#pragma clang fp contract(off)

namespace mfs {

struct D2 { double v[2]; };

// bilinear stencil of a particle on a grid whose samples sit at (index + bias) * cell_size + bound_min:
// base index gi and the |gx - x| / cell_size weights, exactly as :19-23 / :182-186
__device__ __forceinline__ void particle_cell2(const void* px, int pdt, int64_t P, D2 bmin, D2 cs, D2 bias, long long gi[2],
                                               double w[2]) {
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const double x = ldx(px, pdt, 2 * P + d);
    gi[d] = (long long)floor((x - bmin.v[d]) / cs.v[d] - bias.v[d]);
    const double gx = ((double)gi[d] + bias.v[d]) * cs.v[d] + bmin.v[d];
    w[d] = fabs(gx - x) / cs.v[d];
  }
}

__device__ __forceinline__ double corner_weight2(int i, double w) { return (double)i + (i ? -1.0 : 1.0) * (1.0 - w); }

// initialize_density_kernel :8-33 -- scatter particle mass to the 4 surrounding cell centres (indices clamped to the grid)
__global__ void __launch_bounds__(256)
k_density_splat2d(Grid2 g, D2 bmin, D2 cs, const void* px, int pxdt, const void* pm, int pmdt, int64_t P, void* gm, int gdt) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const double m = ldx(pm, pmdt, p);
  long long gi[2];
  double w[2];
  particle_cell2(px, pxdt, p, bmin, cs, D2{{0.5, 0.5}}, gi, w);
  for (int ix = 0; ix < 2; ++ix)
    for (int iy = 0; iy < 2; ++iy) {
      const int cx = (int)max(0LL, min((long long)g.Nx - 1, gi[0] + ix));
      const int cy = (int)max(0LL, min((long long)g.Ny - 1, gi[1] + iy));
      const double weight = corner_weight2(ix, w[0]) * corner_weight2(iy, w[1]);
      atomic_addx(gm, gdt, g.c(cx, cy), weight * m);
    }
}

__device__ __forceinline__ double nonsolid_frac2(const Grid2& g, const void* wx, const void* wy, int wdt, int x, int y) {
  return (ldx(wx, wdt, g.fx(x, y)) + ldx(wx, wdt, g.fx(x + 1, y)) + ldx(wy, wdt, g.fy(x, y)) + ldx(wy, wdt, g.fy(x, y + 1))) *
         0.25;
}

// fix_volume_kernel :35-57 (interior cells; boundary cells of gvol keep what they held)
__global__ void __launch_bounds__(256)
k_density_fix_volume2d(Grid2 g, double cvol, double dx, const void* lvol, int vdt, void* gvol, int gdt, const void* sphi,
                       int sdt, const void* lphi, int ldt, const void* wx, const void* wy, int wdt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.Nx * g.Ny) return;
  const int y = (int)(i % g.Ny), x = (int)(i / g.Ny);
  if (x == 0 || x >= g.Nx - 1 || y == 0 || y >= g.Ny - 1) return;
  auto L = [&](int a, int b) { return ldx(lvol, vdt, g.dg(2 * x + a, 2 * y + b)); };
  double fluid_vol = L(1, 1) + (1.0 / 2.0) * (L(2, 1) + L(0, 1) + L(1, 2) + L(1, 0)) +
                     (1.0 / 4.0) * (L(2, 2) + L(0, 2) + L(2, 0) + L(0, 0));
  const bool near_solid = ldx(sphi, sdt, g.dg(2 * x + 1, 2 * y + 1)) < dx;
  const bool internal = ldx(lphi, ldt, i) < 0 && ldx(lphi, ldt, i + g.Ny) < 0 && ldx(lphi, ldt, i - g.Ny) < 0 &&
                        ldx(lphi, ldt, i + 1) < 0 && ldx(lphi, ldt, i - 1) < 0;
  if (internal && !near_solid) fluid_vol = cvol;
  stx(gvol, gdt, i, fmin(fluid_vol, cvol * nonsolid_frac2(g, wx, wy, wdt, x, y)));
}

// initialize_solver_kernel :59-83 -- b = (1 - clamp(density / rho0, 0.5, 1.5)) / dt in fluid cells
__global__ void __launch_bounds__(256)
k_density_rhs2d(Grid2 g, double rho0, double cvol, double dt, const void* gm, const void* gvol, int gdt, const void* lphi,
                int ldt, const void* wx, const void* wy, int wdt, void* b, int bdt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.Nx * g.Ny) return;
  const int y = (int)(i % g.Ny), x = (int)(i / g.Ny);
  if (x == 0 || x >= g.Nx - 1 || y == 0 || y >= g.Ny - 1) return;
  if (ldx(lphi, ldt, i) >= 0) { stx(b, bdt, i, 0.0); return; }
  const double solid_vol = (1 - nonsolid_frac2(g, wx, wy, wdt, x, y)) * cvol;
  const double solid_mass = rho0 * solid_vol;
  const double cell_mass = ldx(gm, gdt, i) + solid_mass;
  const double cell_vol = ldx(gvol, gdt, i) + solid_vol;
  double density_frac = cell_mass / fmax(cell_vol, 1e-10) / rho0;
  if (cell_mass < 1e-10) density_frac = 1;
  density_frac = fmax(0.5, fmin(1.5, density_frac));
  stx(b, bdt, i, (1 - density_frac) / dt);
}

// compute_displacement_kernel :141-152 -- cells 1 <= x <= Nx-1, 1 <= y <= Ny-1, the last cell included (`x > gres[0]-1`)
__global__ void __launch_bounds__(256)
k_density_displacement2d(Grid2 g, double dt, D2 cs, void* dx, void* dy, int ddt, const void* pv, int pdt, const void* lphi,
                         int ldt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (int64_t)g.Nx * g.Ny) return;
  const int y = (int)(i % g.Ny), x = (int)(i / g.Ny);
  if (x == 0 || y == 0) return;
  const double pc = ldx(lphi, ldt, i), p = ldx(pv, pdt, i);
  const double phix = fmin(1.0, fmax(0.01, edge_in_fraction(pc, ldx(lphi, ldt, i - g.Ny))));
  const double phiy = fmin(1.0, fmax(0.01, edge_in_fraction(pc, ldx(lphi, ldt, i - 1))));
  stx(dx, ddt, g.fx(x, y), (p - ldx(pv, pdt, i - g.Ny)) * dt * cs.v[0] / phix);
  stx(dy, ddt, g.fy(x, y), (p - ldx(pv, pdt, i - 1)) * dt * cs.v[1] / phiy);
}

// apply_displacement_kernel :171-195 -- px[P, axis] += bilinear sample of the face array `d` (shape s0,s1), indices
// clamped to that array's own shape
__global__ void __launch_bounds__(256)
k_density_advect2d(void* px, int pxdt, int64_t P, const void* d, int ddt, int s0, int s1, D2 bmin, D2 cs, D2 bias, int axis) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  long long gi[2];
  double w[2];
  particle_cell2(px, pxdt, p, bmin, cs, bias, gi, w);
  double pos = ldx(px, pxdt, 2 * p + axis);
  for (int ix = 0; ix < 2; ++ix)
    for (int iy = 0; iy < 2; ++iy) {
      const int cx = (int)max(0LL, min((long long)s0 - 1, gi[0] + ix));
      const int cy = (int)max(0LL, min((long long)s1 - 1, gi[1] + iy));
      const double weight = corner_weight2(ix, w[0]) * corner_weight2(iy, w[1]);
      const double add = weight * ldx(d, ddt, (int64_t)cx * s1 + cy);
      // the reference accumulates into the array element itself (:195): with an fp32 position array every
      // partial sum is rounded to fp32
      pos = pxdt == MFS_F32 ? (double)(float)(pos + add) : pos + add;
    }
  stx(px, pxdt, 2 * p + axis, pos);
}

}  // namespace mfs

using namespace mfs;

extern "C" {

int mfs_density_splat2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2], const void* px,
                        int px_dt, const void* pm, int pm_dt, double pvol, int64_t num_particles, void* gm, void* gvol,
                        int g_dt, mfs_stream stream) {
  (void)pvol; (void)gvol;   // accepted and unused: the reference's volume scatter is commented out (:33)
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(bound_min && cell_size && gm, "null argument");
  MFS_REQUIRE(num_particles >= 0 && (num_particles == 0 || (px && pm)), "particle arrays");
  MFS_REQUIRE(dtype_ok(px_dt) && dtype_ok(pm_dt) && dtype_ok(g_dt), "dtype");
  if (num_particles == 0) return MFS_OK;
  Grid2 g{(int)gres[0], (int)gres[1]};
  hipLaunchKernelGGL(k_density_splat2d, dim3(cdiv(num_particles, 256)), dim3(256), 0, (hipStream_t)stream, g,
                     D2{{bound_min[0], bound_min[1]}}, D2{{cell_size[0], cell_size[1]}}, px, px_dt, pm, pm_dt, num_particles,
                     gm, g_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_density_fix_volume2d(const int64_t gres[2], const double cell_size[2], const void* lvol, int lvol_dt, void* gvol,
                             int g_dt, const void* sphi, int sphi_dt, const void* lphi, int lphi_dt, const void* wx,
                             const void* wy, int w_dt, mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(cell_size && lvol && gvol && sphi && lphi && wx && wy, "null argument");
  MFS_REQUIRE(lvol != gvol, "lvol and gvol are aliased");
  MFS_REQUIRE(dtype_ok(lvol_dt) && dtype_ok(g_dt) && dtype_ok(sphi_dt) && dtype_ok(lphi_dt) && dtype_ok(w_dt), "dtype");
  Grid2 g{(int)gres[0], (int)gres[1]};
  const double cvol = cell_size[0] * cell_size[1];                 // cp.prod(cell_size) :209
  const double dx = std::min(cell_size[0], cell_size[1]);          // cp.min(cell_size) :210
  hipLaunchKernelGGL(k_density_fix_volume2d, dim3(cdiv(gres[0] * gres[1], 256)), dim3(256), 0, (hipStream_t)stream, g, cvol,
                     dx, lvol, lvol_dt, gvol, g_dt, sphi, sphi_dt, lphi, lphi_dt, wx, wy, w_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_density_rhs2d(const int64_t gres[2], double rho0, double dt, const double cell_size[2], const void* gm,
                      const void* gvol, int g_dt, const void* lphi, int lphi_dt, const void* wx, const void* wy, int w_dt,
                      void* b, int b_dt, mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(cell_size && gm && gvol && lphi && wx && wy && b, "null argument");
  MFS_REQUIRE(dtype_ok(g_dt) && dtype_ok(lphi_dt) && dtype_ok(w_dt) && dtype_ok(b_dt), "dtype");
  Grid2 g{(int)gres[0], (int)gres[1]};
  const double cvol = cell_size[0] * cell_size[1];
  hipLaunchKernelGGL(k_density_rhs2d, dim3(cdiv(gres[0] * gres[1], 256)), dim3(256), 0, (hipStream_t)stream, g, rho0, cvol,
                     dt, gm, gvol, g_dt, lphi, lphi_dt, wx, wy, w_dt, b, b_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_density_apply2d(const int64_t gres[2], const void* v, void* out, int dt, const void* wx, const void* wy, int w_dt,
                        const void* lphi, int lphi_dt, mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(v && out && wx && wy && lphi && v != out, "null / aliased array");
  MFS_REQUIRE(dtype_ok(dt) && dtype_ok(w_dt) && dtype_ok(lphi_dt), "dtype");
  Grid2 g{(int)gres[0], (int)gres[1]};
  hipLaunchKernelGGL(k_apply2d<true>, dim3(cdiv(gres[0] * gres[1], 256)), dim3(256), 0, (hipStream_t)stream, g, v, out, dt,
                     wx, wy, w_dt, lphi, lphi_dt, (double*)nullptr, (const double*)nullptr);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_density_displacement2d(const int64_t gres[2], double dt, const double cell_size[2], void* dx, void* dy, int d_dt,
                               const void* pv, int pv_dt, const void* lphi, int lphi_dt, mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(cell_size && dx && dy && pv && lphi, "null argument");
  MFS_REQUIRE(dx != dy, "dx and dy are aliased");
  MFS_REQUIRE(dtype_ok(d_dt) && dtype_ok(pv_dt) && dtype_ok(lphi_dt), "dtype");
  Grid2 g{(int)gres[0], (int)gres[1]};
  hipLaunchKernelGGL(k_density_displacement2d, dim3(cdiv(gres[0] * gres[1], 256)), dim3(256), 0, (hipStream_t)stream, g, dt,
                     D2{{cell_size[0], cell_size[1]}}, dx, dy, d_dt, pv, pv_dt, lphi, lphi_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_density_advect2d(void* px, int px_dt, int64_t num_particles, const void* d, int d_dt, const int64_t dshape[2],
                         const double bound_min[2], const double cell_size[2], const double grid_bias[2], int axis,
                         mfs_stream stream) {
  MFS_REQUIRE(d && dshape && bound_min && cell_size && grid_bias, "null argument");
  MFS_REQUIRE(num_particles >= 0 && (num_particles == 0 || px), "particle array");
  MFS_REQUIRE(axis >= 0 && axis < 2, "axis");
  MFS_REQUIRE(dtype_ok(px_dt) && dtype_ok(d_dt), "dtype");
  for (int a = 0; a < 2; ++a) MFS_REQUIRE(dshape[a] >= 1 && dshape[a] <= 65537, "array shape");
  if (num_particles == 0) return MFS_OK;
  hipLaunchKernelGGL(k_density_advect2d, dim3(cdiv(num_particles, 256)), dim3(256), 0, (hipStream_t)stream, px, px_dt,
                     num_particles, d, d_dt, (int)dshape[0], (int)dshape[1], D2{{bound_min[0], bound_min[1]}},
                     D2{{cell_size[0], cell_size[1]}}, D2{{grid_bias[0], grid_bias[1]}}, axis);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
