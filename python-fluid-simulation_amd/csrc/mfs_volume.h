// mfs_volume.h -- the one place a posed level-set volume is described, checked and sampled.
//
// A volume is n0 x n1 x n2 float32 / float64 nodes, node (0,0,0) at `origin` in the body frame, `spacing` apart; a pose
// (R, T) puts the body in the world.  Seeding, rendering and the mesh solids all read such volumes, at most kMaxVolumes per
// launch, described by value:
//   Volumes / Poses          the launch structs; fill_volumes() is their only writer and keeps every refusal
//   pose_to_body             x_b = R^T (x - T)
//   volume_sample            the trilinear sampler: ONE body, restated in numpy operation by operation
//                            (tests/seed_numpy.py, tests/meshsdf_numpy.py)
//   lattice_split            flat index of a lattice point -> (i0, i1, i2), 64-bit divisions per block only
//   GridArgs3 / check_lattice  the grid arguments of the evaluate / union kernels; the node-lattice check
// The first four are plain C++17 and compile without HIP (tests/c_abi/volume_sample_check.cpp runs them on the host); the
// host-side checks need mfs_common.h and exist under hipcc only.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/mfs.h"

#if defined(__HIPCC__)
#include "mfs_common.h"
#define MFS_HD __host__ __device__ __forceinline__
#else
#define MFS_HD inline
#endif
// Every expression of a function that opens with this rounds as written, whatever the including file's contraction.
#if defined(__clang__)
#define MFS_FP_AS_WRITTEN _Pragma("clang fp contract(off)")
#else
#define MFS_FP_AS_WRITTEN        // build with -ffp-contract=off
#endif

namespace mfs {

constexpr int kMaxVolumes = 16;

struct Volumes {                           // by value in the launch
  const void* vol[kMaxVolumes];
  int dt[kMaxVolumes];
  int n[kMaxVolumes][3];
  double org[kMaxVolumes][3];
  double h[kMaxVolumes];
};

struct Poses {                             // by value in the launch: the host-given poses of the same entries
  double R[kMaxVolumes][3][3];
  double T[kMaxVolumes][3];
};

// no launch struct grows: these are the sizes of the fields as the three files held them (the mesh kernels gained dt)
static_assert(sizeof(Volumes) == kMaxVolumes * (8 + 4 + 12 + 24 + 8), "Volumes: the fields, unpadded");
static_assert(sizeof(Poses) == kMaxVolumes * (72 + 24), "Poses: the fields, unpadded");

MFS_HD double volume_load(const void* p, int dt, int64_t i) {
  return dt == MFS_F32 ? (double)((const float*)p)[i] : ((const double*)p)[i];
}

// x_b = R^T (x - T)
MFS_HD void pose_to_body(const double R[3][3], const double T[3], const double x[3], double out[3]) {
  MFS_FP_AS_WRITTEN
  const double d[3] = {x[0] - T[0], x[1] - T[1], x[2] - T[2]};
  for (int i = 0; i < 3; ++i) out[i] = (R[0][i] * d[0] + R[1][i] * d[1]) + R[2][i] * d[2];
}

// Volume i at the body-frame point xb: the trilinear sample in float64; outside the volume: the sample at the clamped point
// plus the distance to the volume's box.  Every load is in bounds whatever xb.  Optional outputs (null: not wanted):
//   inside  0 <= u <= n - 1 on all three axes, u the node coordinate
//   cell    the clamped cell the loads came from
//   grad    the gradient of the returned function in the body frame -- along an axis where the point was clamped the
//           sample does not vary and only the distance term contributes
// F32: every volume of V is float32 (the mesh bodies') and dt is not read: the typed load's branch on a per-entry code
// cost k_mesh_union_grid a third of its time (profiles/shape_volume_refactor.txt).
template <bool F32 = false>
MFS_HD double volume_sample(const Volumes& V, int i, const double xb[3], bool* inside = nullptr, int* cell = nullptr,
                            double* grad = nullptr) {
  MFS_FP_AS_WRITTEN
  int64_t c[3];
  double f[3], e[3];
  bool in[3];
  for (int k = 0; k < 3; ++k) {
    const double t = (xb[k] - V.org[i][k]) / V.h[i];
    const double hi = (double)(V.n[i][k] - 1);
    in[k] = t >= 0.0 && t <= hi;
    const double tc = fmin(fmax(t, 0.0), hi);
    int ci = (int)floor(tc);
    if (ci > V.n[i][k] - 2) ci = V.n[i][k] - 2;
    if (ci < 0) ci = 0;                               // never taken for a finite point; keeps the loads in bounds regardless
    c[k] = ci;
    if (cell) cell[k] = ci;
    f[k] = tc - (double)ci;
    e[k] = (t - tc) * V.h[i];
  }
  if (inside) *inside = in[0] && in[1] && in[2];
  const int64_t s0 = (int64_t)V.n[i][1] * V.n[i][2], s1 = V.n[i][2];
  const int64_t p = c[0] * s0 + c[1] * s1 + c[2];
  const void* v = V.vol[i];
  const int dt = F32 ? (int)MFS_F32 : V.dt[i];
  const double v000 = volume_load(v, dt, p), v001 = volume_load(v, dt, p + 1), v010 = volume_load(v, dt, p + s1),
               v011 = volume_load(v, dt, p + s1 + 1);
  const double v100 = volume_load(v, dt, p + s0), v101 = volume_load(v, dt, p + s0 + 1),
               v110 = volume_load(v, dt, p + s0 + s1), v111 = volume_load(v, dt, p + s0 + s1 + 1);
  const double g0 = 1.0 - f[0], g1 = 1.0 - f[1], g2 = 1.0 - f[2];
  const double c00 = v000 * g2 + v001 * f[2], c01 = v010 * g2 + v011 * f[2];
  const double c10 = v100 * g2 + v101 * f[2], c11 = v110 * g2 + v111 * f[2];
  const double c0 = c00 * g1 + c01 * f[1], c1 = c10 * g1 + c11 * f[1];
  const double dist = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
  if (grad) {
    const double a00 = v000 * g1 + v010 * f[1], a01 = v001 * g1 + v011 * f[1];   // along axis 1, for d/dx2
    const double a10 = v100 * g1 + v110 * f[1], a11 = v101 * g1 + v111 * f[1];
    grad[0] = in[0] ? (c1 - c0) / V.h[i] : 0.0;
    grad[1] = in[1] ? ((c01 - c00) * g0 + (c11 - c10) * f[0]) / V.h[i] : 0.0;
    grad[2] = in[2] ? ((a01 - a00) * g0 + (a11 - a10) * f[0]) / V.h[i] : 0.0;
    if (dist > 0.0)
      for (int k = 0; k < 3; ++k) grad[k] += e[k] / dist;
  }
  return (c0 * g0 + c1 * f[0]) + dist;
}

// Point base + tid of a lattice with inner extents n1, n2 (flat index (i0 * n1 + i1) * n2 + i2), `base` the first point of
// the workgroup and so wave-uniform: the 64-bit divisions are per block, the per-lane ones 32-bit.  Needs extents <= 2^30
// and tid < 2^30.
struct LatticeIndex {
  int64_t i0;
  uint32_t i1, i2;
};

MFS_HD LatticeIndex lattice_split(int64_t base, int tid, int64_t n1, int64_t n2) {
  const int64_t row = base / n2;
  uint32_t i2 = (uint32_t)(base - row * n2) + (uint32_t)tid;
  const uint32_t q2 = i2 / (uint32_t)n2;
  i2 -= q2 * (uint32_t)n2;
  const int64_t i0 = row / n1;
  uint32_t i1 = (uint32_t)(row - i0 * n1) + q2;
  const uint32_t q1 = i1 / (uint32_t)n1;
  i1 -= q1 * (uint32_t)n1;
  return {i0 + q1, i1, i2};
}

// The regular grid of k_sdf_evaluate_grid and k_mesh_union_grid: point (i0, i1, i2) lies at
// bmin + (double)((float)i + bias) * cs per axis, the multiply and the add rounded separately.
struct GridArgs3 {
  int64_t n1, n2, total;         // extents of the two inner axes, number of points
  double bmin[3];                // bound_min, already rounded to float32
  float bias[3];
  double cs[3];
};

#if defined(__HIPCC__)
// ---------------------------------------------------------------------------------------------- host-side checks ----

// extents >= 2 and fewer than 2^31 nodes: 32-bit node indices
static inline bool volume_extents_ok(const int64_t* e) {
  return e[0] >= 2 && e[1] >= 2 && e[2] >= 2 && e[0] < ((int64_t)1 << 31) / e[1] / e[2];
}

// a lattice of nodes, as the mesh-to-SDF build and the skin write one
static inline int check_lattice(const int64_t shape[3], const double origin[3], double spacing) {
  MFS_REQUIRE(shape && origin, "null lattice description");
  MFS_REQUIRE(shape[0] >= 2 && shape[1] >= 2 && shape[2] >= 2, "lattice extents must be >= 2");
  MFS_REQUIRE(shape[0] < ((int64_t)1 << 31) / shape[1] / shape[2], "lattice node count must stay below 2^31");
  MFS_REQUIRE(spacing > 0 && isfinite(spacing), "spacing must be positive");
  for (int k = 0; k < 3; ++k) MFS_REQUIRE(isfinite(origin[k]), "origin must be finite");
  return MFS_OK;
}

// Entries 0 .. m - 1 of V (and of P, when given) from the host arrays of the C entry points, m <= kMaxVolumes the caller's
// to check: extents_host 3 per entry, origins_host 3, spacings_host 1, poses_host 12 (R row-major, then T).
// dtypes_host null: every volume is float32.  poses_host is read iff P is given.
static inline int fill_volumes(Volumes* V, Poses* P, int m, const void* const* volumes_host, const int* dtypes_host,
                               const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                               const double* poses_host) {
  memset(V, 0, sizeof(*V));
  if (P) memset(P, 0, sizeof(*P));
  for (int i = 0; i < m; ++i) {
    MFS_REQUIRE(volumes_host[i], "null shape volume");
    const int dt = dtypes_host ? dtypes_host[i] : (int)MFS_F32;
    MFS_REQUIRE(dtype_ok(dt), "dtype");
    MFS_REQUIRE(spacings_host[i] > 0 && isfinite(spacings_host[i]), "shape volume spacing must be positive");
    const int64_t* e = extents_host + 3 * i;
    MFS_REQUIRE(volume_extents_ok(e), "shape volume extents must be >= 2, fewer than 2^31 nodes");
    V->vol[i] = volumes_host[i];
    V->dt[i] = dt;
    V->h[i] = spacings_host[i];
    for (int k = 0; k < 3; ++k) {
      MFS_REQUIRE(isfinite(origins_host[3 * i + k]), "shape volume origin must be finite");
      V->n[i][k] = (int)e[k];
      V->org[i][k] = origins_host[3 * i + k];
    }
    if (!P) continue;
    for (int k = 0; k < 3; ++k) {
      MFS_REQUIRE(isfinite(poses_host[12 * i + 9 + k]), "shape translation must be finite");
      P->T[i][k] = poses_host[12 * i + 9 + k];
      for (int c = 0; c < 3; ++c) {
        MFS_REQUIRE(isfinite(poses_host[12 * i + 3 * k + c]), "shape rotation must be finite");
        P->R[i][k][c] = poses_host[12 * i + 3 * k + c];
      }
    }
  }
  return MFS_OK;
}

// The grid of a C entry point -> GridArgs3; an empty grid gives total == 0 and no launch.  256: the kernels' block.
static inline int fill_grid_args(GridArgs3* a, const int64_t res[3], const double bound_min[3], const double bias[3],
                                 const double cell_size[3]) {
  MFS_REQUIRE(res && bound_min && bias && cell_size, "null grid description");
  const int64_t lim = (int64_t)1 << 30;
  MFS_REQUIRE(res[0] >= 0 && res[1] >= 0 && res[2] >= 0 && res[0] <= lim && res[1] <= lim && res[2] <= lim, "grid extents");
  const int64_t rows = res[0] * res[1];
  MFS_REQUIRE(rows == 0 || res[2] == 0 || rows <= (int64_t)0x7fffffff * 256 / res[2], "grid too large for one launch");
  a->n1 = res[1];
  a->n2 = res[2];
  a->total = rows * res[2];
  for (int k = 0; k < 3; ++k) {
    a->bmin[k] = (double)(float)bound_min[k];
    a->bias[k] = (float)bias[k];
    a->cs[k] = cell_size[k];
  }
  return MFS_OK;
}
#endif  // __HIPCC__

}  // namespace mfs
