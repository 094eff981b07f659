// mfs_sdf2d.hip -- 2D rigid-body signed distance evaluation and particle projection on gfx950.
// Reference: solver/sdf2D.py -- evaluate_kernel (:146-169) and project_kernel (:171-183) with the sphere / box
// device functions (:50-143).
//
// A rigid body is an (8,3) float64 block of `rb_d` (generate_rb :221-252): row 0 = [type code, parameters],
// rows 1-3 = translation matrix, rows 4-6 = rotation matrix, row 7 = velocity.  type code // 2: 0 sphere (a disc),
// 1 box; odd = flipped (the fluid lives inside).  Kept as the source does it, not as its comments say:
//  * the sphere's centre is read from rb[1,2], rb[2,2] (:54-55) -- the translation column;
//  * sd starts at 100, max_disp at -100; the first body wins ties (`d < min_sd`); vel is written only where
//    min_sd <= 0, from the LAST row of the winning body (`rb_d[rb_index, -1, i]`, :169);
//  * box_project's test `rb[0,0] % 2 and ~(in_out)` (:122) -- `~` is the integer complement, true for every in_out
//    that can occur: a flipped box maps EVERY point into its frame, clamps it and maps it back;
//  * sphere_project's `dist <= 0.0001` branch (:71-74): a point at the centre of a flipped sphere goes to
//    (cx + radius, cy); at the centre of a solid one it stays.
#include <math.h>

#include "mfs_common.h"

// separate multiply / add roundings, like the reference's expressions under CPython (the goldens)
#pragma clang fp contract(off)

namespace mfs {

struct Rb2 {                     // one body, loaded into registers
  double p[3];                   // row 0
  double T[2];                   // translation T[i,2]
  double R[2][2];                // rotation
  double vel[2];                 // row 7
};

__device__ __forceinline__ Rb2 rb2_load(const double* __restrict__ rb_d, int i) {
  const double* b = rb_d + (int64_t)i * 24;
  Rb2 r;
  for (int k = 0; k < 3; ++k) r.p[k] = b[k];
  for (int k = 0; k < 2; ++k) r.T[k] = b[(1 + k) * 3 + 2];
  for (int a = 0; a < 2; ++a)
    for (int c = 0; c < 2; ++c) r.R[a][c] = b[(4 + a) * 3 + c];
  for (int k = 0; k < 2; ++k) r.vel[k] = b[7 * 3 + k];
  return r;
}

__device__ __forceinline__ bool rb2_flipped(const Rb2& r) { return fmod(r.p[0], 2.0) != 0.0; }

// pos_rb = inv_rigid(T, R) * position     (inv_rigid :29-38, matvecmul4 :19-27)
__device__ __forceinline__ void to_body2(const Rb2& r, const double pos[2], double out[2]) {
  for (int i = 0; i < 2; ++i) {
    double t2 = 0.0;
    for (int j = 0; j < 2; ++j) t2 -= r.R[j][i] * r.T[j];
    double tmp = 0.0;
    for (int j = 0; j < 2; ++j) tmp += r.R[j][i] * pos[j];
    tmp += t2;
    out[i] = tmp;
  }
}

// position = mat_TR(T, R) * pos_rb       (mat_TR :12-17)
__device__ __forceinline__ void to_world2(const Rb2& r, const double prb[2], double out[2]) {
  for (int i = 0; i < 2; ++i) {
    double tmp = 0.0;
    for (int j = 0; j < 2; ++j) tmp += r.R[i][j] * prb[j];
    tmp += r.T[i];
    out[i] = tmp;
  }
}

__device__ __forceinline__ double norm2(const double v[2]) { return sqrt(v[0] * v[0] + v[1] * v[1]); }

__device__ __forceinline__ double sphere_eval2(const Rb2& r, const double pos[2]) {
  const double d[2] = {pos[0] - r.T[0], pos[1] - r.T[1]};
  double sd = norm2(d) - r.p[1];
  if (rb2_flipped(r)) sd = -sd;
  return sd;
}

__device__ __forceinline__ void sphere_project2(const Rb2& r, double pos[2]) {
  const double d[2] = {pos[0] - r.T[0], pos[1] - r.T[1]};
  const double dist = norm2(d);
  if (dist <= 0.0001) {
    if (rb2_flipped(r)) { pos[0] = r.T[0] + r.p[1]; pos[1] = r.T[1]; }
    return;
  }
  double sd = dist - r.p[1];
  if (rb2_flipped(r)) sd = -sd;
  if (sd < 0)
    for (int i = 0; i < 2; ++i) pos[i] = d[i] / dist * r.p[1] + r.T[i];
}

__device__ __forceinline__ double box_eval2(const Rb2& r, const double pos[2]) {
  double prb[2];
  to_body2(r, pos, prb);
  double tmp = 0.0, max_disp = -100.0;
  for (int i = 0; i < 2; ++i) {
    const double disp = fabs(prb[i]) - r.p[1 + i] / 2;
    if (disp > 0) tmp += disp * disp;
    if (max_disp < disp) max_disp = disp;
  }
  double sd = sqrt(tmp);
  if (max_disp < 0) sd += max_disp;
  if (rb2_flipped(r)) sd = -sd;
  return sd;
}

__device__ __forceinline__ void box_project2(const Rb2& r, double pos[2]) {
  double prb[2];
  to_body2(r, pos, prb);
  int in_out = 0;
  for (int i = 0; i < 2; ++i)
    if (prb[i] > r.p[1 + i] / 2 || prb[i] < -r.p[1 + i] / 2) ++in_out;
  if (rb2_flipped(r)) {                      // `rb[0,0] % 2 and ~(in_out)`: always true for a flipped box (:122)
    for (int i = 0; i < 2; ++i) {
      const double h = r.p[1 + i] / 2;
      if (prb[i] < -h) prb[i] = -h;
      else if (prb[i] > h) prb[i] = h;
    }
    to_world2(r, prb, pos);
  } else if (in_out == 0) {                  // inside a solid box: out through the nearest face (:130-143)
    int index = 0;
    double dist_xyz = 100.0;
    for (int i = 0; i < 2; ++i) {
      const double h = r.p[1 + i] / 2;
      if (h - prb[i] < dist_xyz) { dist_xyz = h - prb[i]; index = i * 2; }
      if (prb[i] + h < dist_xyz) { dist_xyz = prb[i] + h; index = i * 2 + 1; }
    }
    prb[index / 2] += dist_xyz * ((index % 2) ? -1.0 : 1.0);
    to_world2(r, prb, pos);
  }
}

// evaluate_kernel :146-169
__global__ void __launch_bounds__(256)
k_sdf_evaluate2d(const double* __restrict__ rb_d, int nrb, const void* position, int pdt, int64_t P, void* sd, int sdt,
                 void* vel, int vdt) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const double pos[2] = {ldx(position, pdt, 2 * p), ldx(position, pdt, 2 * p + 1)};
  double min_sd = 100.0;
  int idx = 0;
  for (int i = 0; i < nrb; ++i) {
    const Rb2 r = rb2_load(rb_d, i);
    const int kind = (int)floor(r.p[0] / 2);
    double d = min_sd;                        // unknown kinds leave the minimum alone
    if (kind == 0) d = sphere_eval2(r, pos);
    else if (kind == 1) d = box_eval2(r, pos);
    if (d < min_sd) { min_sd = d; idx = i; }
  }
  stx(sd, sdt, p, min_sd);
  if (min_sd <= 0 && nrb > 0) {
    const Rb2 r = rb2_load(rb_d, idx);
    for (int k = 0; k < 2; ++k) stx(vel, vdt, 2 * p + k, r.vel[k]);
  }
}

// evaluate_kernel on the nodes of a regular grid (moving bodies: one solid level set per step): the position comes from
// the index by get_grid_pos' rule -- bound_min(f32) + (f32 index + f32 bias) * cell_size in float64, multiply and add
// rounded separately -- and EVERY vel element is written (0 outside the bodies).  rb_w (n), optional: angular velocities;
// the winning body's surface velocity is then v + w x (pos - T): (v0 - w r1, v1 + w r0), every operation rounded on its own.
struct GridArgs2 {
  int64_t n1, total;             // extent of the inner axis, number of points
  double bmin[2];                // bound_min, already rounded to float32
  float bias[2];
  double cs[2];
};

__global__ void __launch_bounds__(256)
k_sdf_evaluate_grid2d(const double* __restrict__ rb_d, int nrb, const double* __restrict__ rb_w, GridArgs2 a, void* sd,
                      int sdt, void* vel, int vdt) {
  const int64_t base = (int64_t)blockIdx.x * 256;       // wave-uniform: the 64-bit division is per block ...
  const int64_t p = base + threadIdx.x;
  if (p >= a.total) return;
  int64_t i0 = base / a.n1;
  uint32_t i1 = (uint32_t)(base - i0 * a.n1) + threadIdx.x;    // ... and per thread 32-bit (extents <= 2^30)
  const uint32_t q1 = i1 / (uint32_t)a.n1;
  i1 -= q1 * (uint32_t)a.n1;
  i0 += q1;
  const double pos[2] = {a.bmin[0] + (double)((float)i0 + a.bias[0]) * a.cs[0],
                         a.bmin[1] + (double)((float)i1 + a.bias[1]) * a.cs[1]};
  double min_sd = 100.0;
  int idx = 0;
  for (int i = 0; i < nrb; ++i) {
    const Rb2 r = rb2_load(rb_d, i);
    const int kind = (int)floor(r.p[0] / 2);
    double d = min_sd;                        // unknown kinds leave the minimum alone
    if (kind == 0) d = sphere_eval2(r, pos);
    else if (kind == 1) d = box_eval2(r, pos);
    if (d < min_sd) { min_sd = d; idx = i; }
  }
  stx(sd, sdt, p, min_sd);
  double v[2] = {0.0, 0.0};
  if (min_sd <= 0 && nrb > 0) {
    const Rb2 r = rb2_load(rb_d, idx);
    v[0] = r.vel[0];
    v[1] = r.vel[1];
    if (rb_w) {
      const double w = rb_w[idx];
      const double d[2] = {pos[0] - r.T[0], pos[1] - r.T[1]};
      v[0] = r.vel[0] - w * d[1];
      v[1] = r.vel[1] + w * d[0];
    }
  }
  for (int k = 0; k < 2; ++k) stx(vel, vdt, 2 * p + k, v[k]);
}

// project_kernel :171-183 -- every body in turn, each on the position the previous one left
__global__ void __launch_bounds__(256)
k_sdf_project2d(const double* __restrict__ rb_d, int nrb, void* position, int pdt, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double pos[2] = {ldx(position, pdt, 2 * p), ldx(position, pdt, 2 * p + 1)};
  for (int i = 0; i < nrb; ++i) {
    const Rb2 r = rb2_load(rb_d, i);
    const int kind = (int)floor(r.p[0] / 2);
    if (kind == 0) sphere_project2(r, pos);
    else if (kind == 1) box_project2(r, pos);
    if (pdt == MFS_F32)                       // the reference writes into the array row: float32 positions round per body
      for (int k = 0; k < 2; ++k) pos[k] = (double)(float)pos[k];
  }
  for (int k = 0; k < 2; ++k) stx(position, pdt, 2 * p + k, pos[k]);
}

}  // namespace mfs

using namespace mfs;

// evaluate_grid: per-thread index arithmetic is 32-bit within a row, the flat index 64-bit; one launch of 256-thread blocks
static const int64_t kGridMaxExtent2 = (int64_t)1 << 30;
static const int64_t kGridMaxPoints2 = (int64_t)0x7fffffff * 256;

extern "C" {

int mfs_sdf_evaluate2d(const void* rb_d, int64_t num_bodies, const void* position, int pos_dt, int64_t num_positions,
                       void* sd, int sd_dt, void* vel, int vel_dt, mfs_stream stream) {
  MFS_REQUIRE(num_bodies >= 0 && num_bodies <= 4096 && (num_bodies == 0 || rb_d), "rigid bodies");
  MFS_REQUIRE(num_positions >= 0 && (num_positions == 0 || (position && sd && vel)), "position / output arrays");
  MFS_REQUIRE(dtype_ok(pos_dt) && dtype_ok(sd_dt) && dtype_ok(vel_dt), "dtype");
  if (num_positions == 0) return MFS_OK;
  hipLaunchKernelGGL(k_sdf_evaluate2d, dim3(cdiv(num_positions, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const double*)rb_d, (int)num_bodies, position, pos_dt, num_positions, sd, sd_dt, vel, vel_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_sdf_evaluate_grid2d(const void* rb_d, int64_t num_bodies, const void* rb_w, const int64_t res[2],
                            const double bound_min[2], const double bias[2], const double cell_size[2], void* sd,
                            int sd_dt, void* vel, int vel_dt, mfs_stream stream) {
  MFS_REQUIRE(num_bodies >= 0 && num_bodies <= 4096 && (num_bodies == 0 || rb_d), "rigid bodies");
  MFS_REQUIRE(res && bound_min && bias && cell_size, "null grid description");
  MFS_REQUIRE(res[0] >= 0 && res[1] >= 0 && res[0] <= kGridMaxExtent2 && res[1] <= kGridMaxExtent2, "grid extents");
  MFS_REQUIRE(dtype_ok(sd_dt) && dtype_ok(vel_dt), "dtype");
  if (res[0] == 0 || res[1] == 0) return MFS_OK;
  MFS_REQUIRE(res[0] <= kGridMaxPoints2 / res[1], "grid too large for one launch");
  MFS_REQUIRE(sd && vel, "output arrays");
  GridArgs2 a;
  a.n1 = res[1];
  a.total = res[0] * res[1];
  for (int k = 0; k < 2; ++k) {
    a.bmin[k] = (double)(float)bound_min[k];
    a.bias[k] = (float)bias[k];
    a.cs[k] = cell_size[k];
  }
  hipLaunchKernelGGL(k_sdf_evaluate_grid2d, dim3(cdiv(a.total, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const double*)rb_d, (int)num_bodies, (const double*)rb_w, a, sd, sd_dt, vel, vel_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_sdf_project2d(const void* rb_d, int64_t num_bodies, void* position, int pos_dt, int64_t num_positions,
                      mfs_stream stream) {
  MFS_REQUIRE(num_bodies >= 0 && num_bodies <= 4096 && (num_bodies == 0 || rb_d), "rigid bodies");
  MFS_REQUIRE(num_positions >= 0 && (num_positions == 0 || position), "position array");
  MFS_REQUIRE(dtype_ok(pos_dt), "dtype");
  if (num_positions == 0 || num_bodies == 0) return MFS_OK;
  hipLaunchKernelGGL(k_sdf_project2d, dim3(cdiv(num_positions, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const double*)rb_d, (int)num_bodies, position, pos_dt, num_positions);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
