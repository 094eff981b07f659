// mfs_notebook2d.hip -- the 2D time step's particle <-> grid transfers and grid kernels on gfx950.
//
// The reference has no 2D driver: these are the kernels of 3D_viscous_fluid_sim.ipynb (code cells 2-7) one dimension
// down, i.e. mfs_particles.hip (p2g, g2p, level set, volume) and the notebook grid kernels of mfs_visc.hip (extrapolate,
// boundary condition) with the z factor / z terms REMOVED -- the same float32 locals, the same order of multiplies and
// adds over what is left, so that a 3D run whose particles sit on a cell-centre plane with nothing varying in z gives the
// bits of the 2D run on that plane (tests/test_notebook2d_oracle.py pins the numpy restatement that way).
// One thread per particle or per face, grid-stride, consecutive lanes on consecutive y (the contiguous axis).  The
// normalize of p2g is dimension-free: mfs_p2g_normalize3d serves both.
#include <math.h>

#include "mfs_common.h"

// No FMA contraction in this file: base indices, float32-rounded grid positions and weights must round where separate
// multiplies and adds round (as in mfs_particles.hip); the grid kernels then are their numpy restatement operation by
// operation as well.
#pragma clang fp contract(off)

namespace mfs {

struct QGrid {            // clamp extents (the `gres` argument) and the row length of the target array
  int N[2];
  int s1;
  __device__ __forceinline__ int64_t at(int x, int y) const { return (int64_t)x * s1 + y; }
};
struct QGeom {
  float bmin[2];          // bound_min at float32
  double cs[2];           // cell_size (float64: float32 / int64 in the containers)
  double off[2];          // sample position offset: the float32 grid bias, or 0.5 / 0 for the level set / volume
  int has_bias;           // 1: `... / cell_size - grid_bias` (p2g, g2p); 0: no bias term in the index
};

// x (float32), gi = floor(...), gx (float32): nb_cell of mfs_particles.hip on two axes
__device__ __forceinline__ void nb_cell2(const void* px, int pdt, int64_t P, const QGeom& g, float x[2], long long gi[2],
                                         float gx[2]) {
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    x[d] = (float)ldx(px, pdt, 2 * P + d);
    double t = (double)(x[d] - g.bmin[d]) / g.cs[d];               // float32 difference, float64 quotient
    if (g.has_bias) t -= g.off[d];
    gi[d] = (long long)floor(t);
    gx[d] = (float)(((double)gi[d] + g.off[d]) * g.cs[d] + (double)g.bmin[d]);
  }
}

// min of a field cell and a candidate, atomically: the two forms of mfs_particles.hip's atomic_min_t (one integer atomic on
// the IEEE bits after a plain read, or the compare-and-swap loop; the same bits either way)
__device__ __forceinline__ void atomic_min_q(void* p, int dt, int64_t i, double v, bool cas) {
  if (dt == MFS_F32) {
    const float fv = (float)v;
    if (!cas) {
      if (((const float*)p)[i] <= fv) return;
      if (fv >= 0.f) atomicMin((int*)p + i, __float_as_int(fv));
      else atomicMax((unsigned*)p + i, __float_as_uint(fv));
      return;
    }
    int* a = (int*)p + i;
    int old = *a, assumed;
    do {
      assumed = old;
      if (__int_as_float(assumed) <= fv) break;
      old = atomicCAS(a, assumed, __float_as_int(fv));
    } while (assumed != old);
  } else {
    if (!cas) {
      if (((const double*)p)[i] <= v) return;
      if (v >= 0.0) atomicMin((long long*)p + i, __double_as_longlong(v));
      else atomicMax((unsigned long long*)p + i, (unsigned long long)__double_as_longlong(v));
      return;
    }
    unsigned long long* a = (unsigned long long*)p + i;
    unsigned long long old = *a, assumed;
    do {
      assumed = old;
      if (__longlong_as_double((long long)assumed) <= v) break;
      old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(v));
    } while (assumed != old);
  }
}

__device__ __forceinline__ int clampq(long long v, int n) { return (int)max(0LL, min((long long)n - 1, v)); }

// p2g_particle one dimension down: four corners, affine term (disp + i * cell_size) . pc
__global__ void __launch_bounds__(256)
k_p2g_scatter2d(QGrid g, QGeom geo, int axis, const void* px, int pxdt, const void* pm, int pmdt, const void* pv, int pvdt,
                const void* pca, int pcdt, int64_t P, void* gm, void* gv, int gdt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    const double m = ldx(pm, pmdt, p);
    float x[2], gx[2], disp[2], w[2];
    long long gi[2];
    nb_cell2(px, pxdt, p, geo, x, gi, gx);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      disp[d] = gx[d] - x[d];
      w[d] = (float)((double)fabsf(disp[d]) / geo.cs[d]);
    }
    const float va = (float)ldx(pv, pvdt, 2 * p + axis);
    const double c0 = ldx(pca, pcdt, 2 * p), c1 = ldx(pca, pcdt, 2 * p + 1);
    for (int ix = 0; ix < 2; ++ix)
      for (int iy = 0; iy < 2; ++iy) {
        const int cx = clampq(gi[0] + ix, g.N[0]), cy = clampq(gi[1] + iy, g.N[1]);
        const double wx = ix + (ix ? -1.0 : 1.0) * (1 - (double)w[0]);
        const double wy = iy + (iy ? -1.0 : 1.0) * (1 - (double)w[1]);
        const double cv = ((double)disp[0] + ix * geo.cs[0]) * c0 + ((double)disp[1] + iy * geo.cs[1]) * c1;
        const double weight = wx * wy;
        const int64_t c = g.at(cx, cy);
        atomic_addx(gm, gdt, c, weight * m);
        atomic_addx(gv, gdt, c, weight * m * ((double)va + cv));
      }
  }
}

// g2p_particle one dimension down: every partial sum rounded to the particle arrays' dtype, as the reference's
// accumulation into the array element does
__global__ void __launch_bounds__(256)
k_g2p_gather2d(QGrid g, QGeom geo, int axis, const void* px, int pxdt, void* pv, int pvdt, void* pca, int pcdt, int64_t P,
               const void* gv, int gdt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  auto acc = [](double s, double t, int dt) { return dt == MFS_F32 ? (double)(float)(s + t) : s + t; };
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    float x[2], gx[2], w[2];
    long long gi[2];
    nb_cell2(px, pxdt, p, geo, x, gi, gx);
#pragma unroll
    for (int d = 0; d < 2; ++d) w[d] = (float)((double)fabsf(gx[d] - x[d]) / geo.cs[d]);
    double vel = 0.0, a0 = 0.0, a1 = 0.0;
    for (int ix = 0; ix < 2; ++ix)
      for (int iy = 0; iy < 2; ++iy) {
        const int cx = clampq(gi[0] + ix, g.N[0]), cy = clampq(gi[1] + iy, g.N[1]);
        const double wx = 1 - ix + (2 * ix - 1) * (double)w[0];
        const double wy = 1 - iy + (2 * iy - 1) * (double)w[1];
        const double gval = ldx(gv, gdt, g.at(cx, cy));
        vel = acc(vel, wx * wy * gval, pvdt);
        a0 = acc(a0, (2 * ix - 1) * wy * gval / geo.cs[0], pcdt);
        a1 = acc(a1, wx * (2 * iy - 1) * gval / geo.cs[1], pcdt);
      }
    stx(pv, pvdt, 2 * p + axis, vel);
    stx(pca, pcdt, 2 * p, a0);
    stx(pca, pcdt, 2 * p + 1, a1);
  }
}

// compute_fls_kernel one dimension down: phi = min(phi, |cell centre - x| - r) over the 5^2 cells around the particle
__global__ void __launch_bounds__(256)
k_fluid_levelset2d(QGrid g, QGeom geo, double r, const void* px, int pxdt, int64_t P, void* phi, int phidt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool cas = P > ((int64_t)8 << 20);      // as k_fluid_levelset of mfs_particles.hip
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    float x[2], gx[2];
    long long gi[2];
    nb_cell2(px, pxdt, p, geo, x, gi, gx);
    for (int dx = -2; dx <= 2; ++dx)
      for (int dy = -2; dy <= 2; ++dy) {
        const int ii[2] = {clampq(gi[0] + dx, g.N[0]), clampq(gi[1] + dy, g.N[1])};
        double n = 0.0;
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const float gip = (float)(((double)ii[d] + 0.5) * geo.cs[d] + (double)geo.bmin[d] - (double)x[d]);
          n += (double)(gip * gip);                              // float32 product, float64 sum
        }
        atomic_min_q(phi, phidt, g.at(ii[0], ii[1]), sqrt(n) - r, cas);
      }
  }
}

// compute_fluid_volume_kernel one dimension down: bilinear splat onto the nodes of the doubled grid
__global__ void __launch_bounds__(256)
k_fluid_volume_splat2d(QGrid g, QGeom geo, const void* px, int pxdt, double pvol, int64_t P, void* gvol, int gdt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
    float x[2], gx[2], w[2];
    long long gi[2];
    nb_cell2(px, pxdt, p, geo, x, gi, gx);
#pragma unroll
    for (int d = 0; d < 2; ++d) w[d] = (float)((double)fabsf(gx[d] - x[d]) / geo.cs[d]);
    for (int ix = 0; ix < 2; ++ix)
      for (int iy = 0; iy < 2; ++iy) {
        const int cx = clampq(gi[0] + ix, g.N[0]), cy = clampq(gi[1] + iy, g.N[1]);
        const double weight = (ix + (ix ? -1.0 : 1.0) * (1 - (double)w[0])) * (iy + (iy ? -1.0 : 1.0) * (1 - (double)w[1]));
        atomic_addx(gvol, gdt, g.at(cx, cy), weight * pvol);
      }
  }
}

// constrain_fluid_volume_kernel: min(., the node's cell area)
__global__ void __launch_bounds__(256) k_fluid_volume_constrain2d(int64_t n, void* gvol, int gdt, double cell_area) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
    stx(gvol, gdt, i, fmin(ldx(gvol, gdt, i), cell_area));
}

// ------------------------------------------------------------------ grid kernels ------------------------------------
// validity = grid mass > 0
__global__ void __launch_bounds__(256) k_grid_valid_mass2d(int64_t n, const void* m, int mdt, unsigned char* valid) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) valid[i] = ldx(m, mdt, i) > 0 ? 1 : 0;
}

// one Jacobi sweep of the 4-neighbour average into the invalid interior faces of one component's array (s0, s1).  Every
// face is written (copy-through or new value) into the OTHER buffer pair, so a sweep reads the previous sweep only.
__global__ void __launch_bounds__(256)
k_grid_extrap_sweep2d(int s0, int s1, const void* vin, void* vout, int vdt, const unsigned char* valid_in,
                      unsigned char* valid_out) {
  const int64_t n = (int64_t)s0 * s1, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int y = (int)(i % s1), x = (int)(i / s1);
    double nv = ldx(vin, vdt, i);
    unsigned char va = valid_in[i];
    const bool interior = !(x == 0 || x >= s0 - 1 || y == 0 || y >= s1 - 1);
    if (interior && !va) {
      double val = 0.0;
      int count = 0;
      const int64_t nb[4] = {i + s1, i - s1, i + 1, i - 1};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (valid_in[nb[k]]) { val += ldx(vin, vdt, nb[k]); ++count; }
      if (count > 0) { nv = val / count; va = 1; }
    }
    stx(vout, vdt, i, nv);
    valid_out[i] = va;
  }
}

struct V2 { const void* p[2]; };

// boundary_condition_{x,y} one dimension down.  AXIS 0: the x-face (x, y) of the array (Nx+1, Ny), doubled-grid node
// (2x, 2y+1), vy / my averaged over (x-ix, y+iy); AXIS 1: the y-face of (Nx, Ny+1), node (2x+1, 2y), vx / mx over
// (x+iz, y-iy) -- the 3D loops' order with the z tap dropped.  sv is (2Nx+1, 2Ny+1, 2).
template <int AXIS>
__global__ void __launch_bounds__(256)
k_grid_boundary_condition2d(int Nx, int Ny, V2 gv, int vdt, V2 gm, int mdt, const void* sphi, int sdt, const void* sv, int svdt,
                            double dx, void* dv, int dvdt) {
  const int s0 = Nx + (AXIS == 0), s1 = Ny + (AXIS == 1);
  constexpr int OTH = 1 - AXIS;
  const int o1 = Ny + (OTH == 1);                 // row length of the other component's array
  const int d1 = 2 * Ny + 1;                      // row length of the doubled grid
  const int64_t n = (int64_t)s0 * s1, stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32prod = vdt == MFS_F32 && mdt == MFS_F32;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const int y = (int)(i % s1), x = (int)(i / s1);
    if (x == 0 || x >= s0 - 1 || y == 0 || y >= s1 - 1) { stx(dv, dvdt, i, 0.0); continue; }
    const int Dx = 2 * x + (AXIS == 0 ? 0 : 1), Dy = 2 * y + (AXIS == 0 ? 1 : 0);
    const int64_t D = (int64_t)Dx * d1 + Dy;
    const double ndist = ldx(sphi, sdt, D) / dx;
    if (ndist >= 1) { stx(dv, dvdt, i, 0.0); continue; }
    double vel[2];
    vel[AXIS] = ldx(gv.p[AXIS], vdt, i);
    double msum = 0.0, vsum = 0.0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const int ox = AXIS == 0 ? -p : q, oy = AXIS == 0 ? q : -p;
        const int64_t f = (int64_t)(x + ox) * o1 + (y + oy);
        const double mm = ldx(gm.p[OTH], mdt, f), vv = ldx(gv.p[OTH], vdt, f);
        msum += mm;
        vsum += f32prod ? (double)((float)vv * (float)mm) : vv * mm;       // product in the arrays' own dtype
      }
    vel[OTH] = vsum / msum;
    const double rx = vel[0] - ldx(sv, svdt, 2 * D), ry = vel[1] - ldx(sv, svdt, 2 * D + 1);
    const double snx = ldx(sphi, sdt, D + d1) - ldx(sphi, sdt, D - d1);
    const double sny = ldx(sphi, sdt, D + 1) - ldx(sphi, sdt, D - 1);
    const double sn_inv = 1.0 / (snx * snx + sny * sny);
    const double s = snx * rx + sny * ry;
    const double proj = (s < 0 ? s : 0.0) * (AXIS == 0 ? snx : sny) * sn_inv;      // min(0, s): NaN -> 0
    stx(dv, dvdt, i, -proj * (1.0 - ndist));
  }
}

static int check_shape2(const int64_t s[2]) {
  MFS_REQUIRE(s != nullptr, "shape is null");
  for (int a = 0; a < 2; ++a) MFS_REQUIRE(s[a] >= 1 && s[a] <= 65537, "array extent out of range [1,65537]");
  return MFS_OK;
}

static QGeom make_geom2(const double bmin[2], const double cs[2], const double off[2], int has_bias) {
  QGeom g;
  for (int d = 0; d < 2; ++d) { g.bmin[d] = (float)bmin[d]; g.cs[d] = cs[d]; g.off[d] = (double)(float)off[d]; }
  g.has_bias = has_bias;
  return g;
}

// grid-stride launches: at most 2^16 blocks of 256
static int blocks_for(int64_t n) { return (int)std::min<int64_t>((n + 255) / 256, 65536); }

}  // namespace mfs

using namespace mfs;

extern "C" {

int mfs_p2g_scatter2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2],
                      const double grid_bias[2], int axis, const void* px, int px_dt, const void* pm, int pm_dt,
                      const void* pv, int pv_dt, const void* pca, int pca_dt, int64_t num_particles, void* gm, void* gv,
                      int g_dt, mfs_stream stream) {
  if (int e = check_shape2(gres)) return e;
  MFS_REQUIRE(bound_min && cell_size && grid_bias && gm && gv, "null argument");
  MFS_REQUIRE(axis >= 0 && axis < 2, "axis");
  MFS_REQUIRE(num_particles >= 0 && (num_particles == 0 || (px && pm && pv && pca)), "particle arrays");
  MFS_REQUIRE(dtype_ok(px_dt) && dtype_ok(pm_dt) && dtype_ok(pv_dt) && dtype_ok(pca_dt) && dtype_ok(g_dt), "dtype");
  if (num_particles == 0) return MFS_OK;
  QGrid g{{(int)gres[0], (int)gres[1]}, (int)gres[1] + (axis == 1)};
  hipLaunchKernelGGL(k_p2g_scatter2d, dim3(blocks_for(num_particles)), dim3(256), 0, (hipStream_t)stream, g,
                     make_geom2(bound_min, cell_size, grid_bias, 1), axis, px, px_dt, pm, pm_dt, pv, pv_dt, pca, pca_dt,
                     num_particles, gm, gv, g_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_g2p_gather2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2],
                     const double grid_bias[2], int axis, const void* px, int px_dt, void* pv, int pv_dt, void* pca,
                     int pca_dt, int64_t num_particles, const void* gv, int g_dt, mfs_stream stream) {
  if (int e = check_shape2(gres)) return e;
  MFS_REQUIRE(bound_min && cell_size && grid_bias && gv, "null argument");
  MFS_REQUIRE(axis >= 0 && axis < 2, "axis");
  MFS_REQUIRE(num_particles >= 0 && (num_particles == 0 || (px && pv && pca)), "particle arrays");
  MFS_REQUIRE(dtype_ok(px_dt) && dtype_ok(pv_dt) && dtype_ok(pca_dt) && dtype_ok(g_dt), "dtype");
  if (num_particles == 0) return MFS_OK;
  QGrid g{{(int)gres[0], (int)gres[1]}, (int)gres[1] + (axis == 1)};
  hipLaunchKernelGGL(k_g2p_gather2d, dim3(blocks_for(num_particles)), dim3(256), 0, (hipStream_t)stream, g,
                     make_geom2(bound_min, cell_size, grid_bias, 1), axis, px, px_dt, pv, pv_dt, pca, pca_dt, num_particles,
                     gv, g_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_fluid_levelset2d(const int64_t gres[2], const double bound_min[2], const double cell_size[2], double radius,
                         const void* px, int px_dt, int64_t num_particles, void* phi, int phi_dt, mfs_stream stream) {
  if (int e = check_shape2(gres)) return e;
  MFS_REQUIRE(bound_min && cell_size && phi, "null argument");
  MFS_REQUIRE(num_particles >= 0 && (num_particles == 0 || px), "particle array");
  MFS_REQUIRE(dtype_ok(px_dt) && dtype_ok(phi_dt), "dtype");
  if (num_particles == 0) return MFS_OK;
  QGrid g{{(int)gres[0], (int)gres[1]}, (int)gres[1]};
  const double half[2] = {0.5, 0.5};
  hipLaunchKernelGGL(k_fluid_levelset2d, dim3(blocks_for(num_particles)), dim3(256), 0, (hipStream_t)stream, g,
                     make_geom2(bound_min, cell_size, half, 0), radius, px, px_dt, num_particles, phi, phi_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_fluid_volume2d(const int64_t vres[2], const double bound_min[2], const double cell_size[2], const void* px,
                       int px_dt, double pvol, int64_t num_particles, void* gvol, int g_dt, mfs_stream stream) {
  if (int e = check_shape2(vres)) return e;
  MFS_REQUIRE(bound_min && cell_size && gvol, "null argument");
  MFS_REQUIRE(num_particles >= 0 && (num_particles == 0 || px), "particle array");
  MFS_REQUIRE(dtype_ok(px_dt) && dtype_ok(g_dt), "dtype");
  if (num_particles == 0) return MFS_OK;
  QGrid g{{(int)vres[0], (int)vres[1]}, (int)vres[1]};
  const double zero[2] = {0.0, 0.0};
  hipLaunchKernelGGL(k_fluid_volume_splat2d, dim3(blocks_for(num_particles)), dim3(256), 0, (hipStream_t)stream, g,
                     make_geom2(bound_min, cell_size, zero, 0), px, px_dt, pvol, num_particles, gvol, g_dt);
  const int64_t n = vres[0] * vres[1];
  hipLaunchKernelGGL(k_fluid_volume_constrain2d, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, n, gvol, g_dt,
                     cell_size[0] * cell_size[1]);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

size_t mfs_grid_extrapolate2d_workspace_bytes(const int64_t gres[2], int v_dt) {
  if (!gres || !dtype_ok(v_dt) || gres[0] < 1 || gres[1] < 1 || gres[0] > 65537 || gres[1] > 65537) return 0;
  size_t tot = 0;
  for (int c = 0; c < 2; ++c) {
    const size_t n = (size_t)(gres[0] + (c == 0)) * (size_t)(gres[1] + (c == 1));
    tot += align_up(n * dtype_size(v_dt), 256) + 2 * align_up(n, 256);
  }
  return tot;
}

int mfs_grid_extrapolate2d(const int64_t gres[2], int num_iter, void* vx, void* vy, int v_dt, const void* mx, const void* my,
                           int m_dt, void* workspace, size_t workspace_bytes, mfs_stream stream) {
  if (int e = check_shape2(gres)) return e;
  MFS_REQUIRE(vx && vy && mx && my && workspace, "null array");
  MFS_REQUIRE(vx != vy, "vx and vy are aliased");
  MFS_REQUIRE(dtype_ok(v_dt) && dtype_ok(m_dt), "dtype");
  MFS_REQUIRE(num_iter >= 0, "num_iter");
  MFS_REQUIRE(workspace_bytes >= mfs_grid_extrapolate2d_workspace_bytes(gres, v_dt), "workspace too small");
  MFS_REQUIRE(((uintptr_t)workspace % 256) == 0, "workspace must be 256-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  void* v[2] = {vx, vy};
  const void* m[2] = {mx, my};
  char* p = (char*)workspace;
  for (int c = 0; c < 2; ++c) {
    const int s0 = (int)gres[0] + (c == 0), s1 = (int)gres[1] + (c == 1);
    const int64_t n = (int64_t)s0 * s1;
    void* tmp = p; p += align_up((size_t)n * dtype_size(v_dt), 256);
    unsigned char* va = (unsigned char*)p; p += align_up((size_t)n, 256);
    unsigned char* vb = (unsigned char*)p; p += align_up((size_t)n, 256);
    if (num_iter == 0) continue;
    const int grid = blocks_for(n);
    hipLaunchKernelGGL(k_grid_valid_mass2d, dim3(grid), dim3(256), 0, st, n, m[c], m_dt, va);
    void *cur = v[c], *oth = tmp;
    unsigned char *mcur = va, *moth = vb;
    for (int it = 0; it < num_iter; ++it) {
      hipLaunchKernelGGL(k_grid_extrap_sweep2d, dim3(grid), dim3(256), 0, st, s0, s1, cur, oth, v_dt, mcur, moth);
      std::swap(cur, oth);
      std::swap(mcur, moth);
    }
    MFS_LAUNCH_CHECK();
    if (cur != v[c]) MFS_HIP_TRY(hipMemcpyAsync(v[c], cur, (size_t)n * dtype_size(v_dt), hipMemcpyDeviceToDevice, st));
  }
  return MFS_OK;
}

int mfs_grid_boundary_condition2d(const int64_t gres[2], const void* gvx, const void* gvy, int v_dt, const void* gmx,
                                  const void* gmy, int m_dt, const void* sphi, int sphi_dt, const void* sv, int sv_dt,
                                  double dx, void* dvx, void* dvy, int dv_dt, mfs_stream stream) {
  if (int e = check_shape2(gres)) return e;
  MFS_REQUIRE(gvx && gvy && gmx && gmy && sphi && sv && dvx && dvy, "null array");
  MFS_REQUIRE(dvx != dvy, "dvx and dvy are aliased");
  MFS_REQUIRE(dtype_ok(v_dt) && dtype_ok(m_dt) && dtype_ok(sphi_dt) && dtype_ok(sv_dt) && dtype_ok(dv_dt), "dtype");
  const int Nx = (int)gres[0], Ny = (int)gres[1];
  V2 gv{{gvx, gvy}}, gm{{gmx, gmy}};
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL((k_grid_boundary_condition2d<0>), dim3(blocks_for((int64_t)(Nx + 1) * Ny)), dim3(256), 0, st, Nx, Ny, gv,
                     v_dt, gm, m_dt, sphi, sphi_dt, sv, sv_dt, dx, dvx, dv_dt);
  hipLaunchKernelGGL((k_grid_boundary_condition2d<1>), dim3(blocks_for((int64_t)Nx * (Ny + 1))), dim3(256), 0, st, Nx, Ny, gv,
                     v_dt, gm, m_dt, sphi, sphi_dt, sv, sv_dt, dx, dvy, dv_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
