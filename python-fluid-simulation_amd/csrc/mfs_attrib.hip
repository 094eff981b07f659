// mfs_attrib.hip -- particle data evaluated at arbitrary points on gfx950 (no reference counterpart):
// A(y) = sum w_i a_i / sum w_i with the skin's weight w_i = max(1 - |x_i - y|^2 / R^2, 0)^3, for C = 1 .. 4 channels.
//   k_attrib_keys     the bin of every position (particles and queries alike): cubic bins of edge exactly R
//   k_attrib_gather   one workgroup per work item -- a bin and up to 256 of its queries -- gathers from the 27 bins
//                     around it; no atomics, fp32 on coordinates taken relative to the bin's low corner in fp64
// Particles and queries arrive sorted by bin (a stable sort by k_attrib_keys' key: the order inside a bin is the
// caller's order), the particles with the first one of every bin in `starts`.
#include <math.h>

#include "mfs_common.h"

namespace mfs {

constexpr int kAttribBlock = 256;          // threads per workgroup = queries per work item = particles per LDS batch
constexpr int kAttribMaxChannels = 4;

struct AttribLattice {
  int m[3];        // bins along each axis; the sentinel key is m[0] m[1] m[2]
  double org[3];
  double R;        // bin edge = influence radius
};

// key[p]: the C-order index of p's bin, c_a = floor((x_a - org_a) / R) in fp64; the number of bins when p lies outside
// the lattice, is not finite, or (has_box) lies outside the closed box [lo, hi].
__global__ void __launch_bounds__(kAttribBlock)
k_attrib_keys(AttribLattice L, int has_box, double lo0, double lo1, double lo2, double hi0, double hi1, double hi2,
              const void* __restrict__ pos, int dt, int64_t N, int* __restrict__ key) {
  const int64_t p = (int64_t)blockIdx.x * kAttribBlock + threadIdx.x;
  if (p >= N) return;
  const double lo[3] = {lo0, lo1, lo2}, hi[3] = {hi0, hi1, hi2};
  int c[3];
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double x = ldx(pos, dt, 3 * p + k);
    const double t = floor((x - L.org[k]) / L.R);
    bool in = t >= 0.0 && t <= (double)(L.m[k] - 1);            // false for NaN
    if (has_box) in = in && x >= lo[k] && x <= hi[k];
    ok = ok && in;
    c[k] = in ? (int)t : 0;
  }
  key[p] = ok ? (c[0] * L.m[1] + c[1]) * L.m[2] + c[2] : L.m[0] * L.m[1] * L.m[2];
}

template <int C> struct AttribRecord;
template <> struct AttribRecord<1> { float4 a; };                   // x y z a0
template <int C> struct AttribRecord { float4 a, b; };              // x y z a0 | a1 a2 a3 -

// One workgroup per work item (key, first, count): the queries first .. first + count - 1 of the sorted queries, all in
// bin `key`, one per lane.  The 27 bins around it are 9 runs of the sorted particles (three bins along axis 2 are
// neighbours in the sort; a bin beyond the lattice holds nothing); the runs are walked in ascending key order as one
// sequence in batches of 256, a lane per particle.  A lane stages its particle -- position minus the bin's low corner,
// subtracted in fp64 and rounded to fp32, and the C values rounded to fp32 -- in LDS; then ALL lanes loop over the batch:
// the trip count is uniform and every LDS read is a 16-byte broadcast of one address.  The loop body has no branch: a
// particle beyond R has t = 0, adds a weight of exactly 0, and its value is replaced by 0 (a select), so that only a
// contributing particle's non-finite value reaches the sums.  A work item whose 27 bins are empty stores `fill` and
// leaves before the loop.  rows: the original row of every sorted query.  tested (may be null): per item, the
// particles its lanes looped over.
template <int C>
__global__ void __launch_bounds__(kAttribBlock)
k_attrib_gather(AttribLattice L, float inv_R2, float fill, const void* __restrict__ ps, int pdt,
                const void* __restrict__ vs, int vdt, int P, const int* __restrict__ starts,
                const void* __restrict__ qs, int qdt, const int64_t* __restrict__ rows, int Q,
                const int* __restrict__ items, float* __restrict__ out, float* __restrict__ weight,
                int* __restrict__ tested) {
  __shared__ AttribRecord<C> s_p[kAttribBlock];
  const int tid = threadIdx.x;
  const int64_t item = blockIdx.x;
  const int key = items[3 * item], qfirst = items[3 * item + 1], qcount = items[3 * item + 2];
  const int m1 = L.m[1], m2 = L.m[2];
  if (key < 0 || key >= L.m[0] * m1 * m2) return;              // uniform; never true for a work list built from keys
  const int c2 = key % m2, c1 = (key / m2) % m1, c0 = key / (m2 * m1);
  const bool live = tid < qcount && qfirst >= 0 && qfirst + tid < Q;
  const int64_t row = live ? rows[qfirst + tid] : 0;

  int first[9], count[9], total = 0;
  const int z_lo = max(c2 - 1, 0), z_hi = min(c2 + 1, m2 - 1);
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    const int b0 = c0 + a / 3 - 1, b1 = c1 + a % 3 - 1;
    first[a] = 0;
    count[a] = 0;
    if (b0 >= 0 && b0 < L.m[0] && b1 >= 0 && b1 < m1) {
      const int base = (b0 * m1 + b1) * m2;
      first[a] = starts[base + z_lo];
      count[a] = starts[base + z_hi + 1] - first[a];
    }
    total += count[a];
  }
  if (tested && tid == 0) tested[item] = total;
  if (total == 0) {                                            // uniform over the workgroup
    if (live) {
#pragma unroll
      for (int k = 0; k < C; ++k) out[C * row + k] = fill;
      weight[row] = 0.f;
    }
    return;
  }

  // everything below is relative to the bin's low corner, subtracted in fp64: scene offsets cost no fp32 digits
  const double corner[3] = {L.org[0] + (double)c0 * L.R, L.org[1] + (double)c1 * L.R, L.org[2] + (double)c2 * L.R};
  float y0 = 0.f, y1 = 0.f, y2 = 0.f;
  if (live) {
    const int64_t q = qfirst + tid;
    y0 = (float)(ldx(qs, qdt, 3 * q) - corner[0]);
    y1 = (float)(ldx(qs, qdt, 3 * q + 1) - corner[1]);
    y2 = (float)(ldx(qs, qdt, 3 * q + 2) - corner[2]);
  }

  float W = 0.f, s[C];
#pragma unroll
  for (int k = 0; k < C; ++k) s[k] = 0.f;
  for (int b = 0; b < total; b += kAttribBlock) {
    int src = -1, rem = b + tid;                               // particle b + tid of the nine runs laid end to end
#pragma unroll
    for (int a = 0; a < 9; ++a) {
      if (rem >= 0 && rem < count[a]) src = first[a] + rem;
      rem -= count[a];
    }
    if (src >= 0 && src < P) {
      AttribRecord<C> rec;
      float v[kAttribMaxChannels] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < C; ++k) v[k] = (float)ldx(vs, vdt, (int64_t)C * src + k);
      rec.a.x = (float)(ldx(ps, pdt, 3 * (int64_t)src) - corner[0]);
      rec.a.y = (float)(ldx(ps, pdt, 3 * (int64_t)src + 1) - corner[1]);
      rec.a.z = (float)(ldx(ps, pdt, 3 * (int64_t)src + 2) - corner[2]);
      rec.a.w = v[0];
      if constexpr (C > 1) rec.b = make_float4(v[1], v[2], v[3], 0.f);
      s_p[tid] = rec;
    }
    __syncthreads();
    const int n = min(kAttribBlock, total - b);
    for (int j = 0; j < n; ++j) {
      const AttribRecord<C> p = s_p[j];
      const float d0 = p.a.x - y0, d1 = p.a.y - y1, d2 = p.a.z - y2;
      const float t = fmaxf(1.f - (d0 * d0 + d1 * d1 + d2 * d2) * inv_R2, 0.f);
      const float w = t * t * t;
      const bool on = w > 0.f;
      W += w;
      s[0] = fmaf(w, on ? p.a.w : 0.f, s[0]);
      if constexpr (C > 1) s[1] = fmaf(w, on ? p.b.x : 0.f, s[1]);
      if constexpr (C > 2) s[2] = fmaf(w, on ? p.b.y : 0.f, s[2]);
      if constexpr (C > 3) s[3] = fmaf(w, on ? p.b.z : 0.f, s[3]);
    }
    __syncthreads();                                           // s_p is rewritten by the next batch
  }
  if (live) {
    const bool covered = W > 0.f;
#pragma unroll
    for (int k = 0; k < C; ++k) out[C * row + k] = covered ? s[k] / W : fill;
    weight[row] = W;
  }
}

static int fill_attrib_lattice(AttribLattice* L, const int64_t shape[3], const double origin[3], double influence) {
  MFS_REQUIRE(shape && origin, "null shape / origin");
  MFS_REQUIRE(influence > 0 && isfinite(influence), "influence radius must be positive and finite");
  for (int k = 0; k < 3; ++k) {
    MFS_REQUIRE(shape[k] >= 1 && shape[k] <= ((int64_t)1 << 31) - 2, "bins per axis must be in 1 .. 2^31 - 2");
    MFS_REQUIRE(isfinite(origin[k]), "origin must be finite");
  }
  MFS_REQUIRE(shape[0] * shape[1] <= (((int64_t)1 << 31) - 2) / shape[2], "more than 2^31 - 2 bins");
  for (int k = 0; k < 3; ++k) {
    L->m[k] = (int)shape[k];
    L->org[k] = origin[k];
  }
  L->R = influence;
  return MFS_OK;
}

}  // namespace mfs

using namespace mfs;

extern "C" {

int64_t mfs_attrib_bins3d(const int64_t shape[3]) {
  if (!shape) return 0;
  const int64_t limit = ((int64_t)1 << 31) - 2;
  for (int k = 0; k < 3; ++k)
    if (shape[k] < 1 || shape[k] > limit) return 0;
  if (shape[0] * shape[1] > limit / shape[2]) return 0;
  return shape[0] * shape[1] * shape[2];
}

int mfs_attrib_keys3d(const int64_t shape[3], const double origin[3], double influence, const double* box_host,
                      const void* positions, int p_dt, int64_t count, void* keys, mfs_stream stream) {
  AttribLattice L;
  if (int st = fill_attrib_lattice(&L, shape, origin, influence)) return st;
  MFS_REQUIRE(dtype_ok(p_dt), "dtype");
  MFS_REQUIRE(count >= 0 && count < ((int64_t)1 << 31), "count must stay below 2^31");
  double box[6] = {0, 0, 0, 0, 0, 0};
  if (box_host)
    for (int k = 0; k < 6; ++k) {
      MFS_REQUIRE(isfinite(box_host[k]), "box must be finite");
      box[k] = box_host[k];
    }
  if (count == 0) return MFS_OK;
  MFS_REQUIRE(positions && keys, "null positions / keys");
  hipLaunchKernelGGL(k_attrib_keys, dim3(cdiv(count, kAttribBlock)), dim3(kAttribBlock), 0, (hipStream_t)stream, L,
                     box_host ? 1 : 0, box[0], box[1], box[2], box[3], box[4], box[5], positions, p_dt, count, (int*)keys);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_attrib_gather3d(const int64_t shape[3], const double origin[3], double influence, int channels, double fill,
                        const void* sorted_particles, int p_dt, const void* sorted_values, int v_dt, int64_t num_particles,
                        const void* bin_starts, const void* sorted_queries, int q_dt, const void* query_rows,
                        int64_t num_queries, const void* items, int64_t num_items, void* values, void* weight, void* tested,
                        mfs_stream stream) {
  AttribLattice L;
  if (int st = fill_attrib_lattice(&L, shape, origin, influence)) return st;
  MFS_REQUIRE(channels >= 1 && channels <= kAttribMaxChannels, "channels must be in 1 .. 4");
  MFS_REQUIRE(dtype_ok(p_dt) && dtype_ok(v_dt) && dtype_ok(q_dt), "dtype");
  MFS_REQUIRE(num_particles >= 0 && num_particles < ((int64_t)1 << 31), "particle count must stay below 2^31");
  MFS_REQUIRE(num_queries >= 0 && num_queries < ((int64_t)1 << 31), "query count must stay below 2^31");
  MFS_REQUIRE(num_items >= 0 && num_items <= num_queries, "at most one work item per query");
  if (num_items == 0) return MFS_OK;
  MFS_REQUIRE(num_particles == 0 || (sorted_particles && sorted_values), "null particles / values");
  MFS_REQUIRE(bin_starts && sorted_queries && query_rows && items && values && weight,
              "null bin_starts / queries / rows / items / values / weight");
  const float inv_R2 = (float)(1.0 / (influence * influence));
  const dim3 grid((unsigned)num_items), block(kAttribBlock);
#define MFS_ATTRIB_LAUNCH(C)                                                                                            \
  hipLaunchKernelGGL(k_attrib_gather<C>, grid, block, 0, (hipStream_t)stream, L, inv_R2, (float)fill, sorted_particles,  \
                     p_dt, sorted_values, v_dt, (int)num_particles, (const int*)bin_starts, sorted_queries, q_dt,        \
                     (const int64_t*)query_rows, (int)num_queries, (const int*)items, (float*)values, (float*)weight,    \
                     (int*)tested)
  switch (channels) {
    case 1: MFS_ATTRIB_LAUNCH(1); break;
    case 2: MFS_ATTRIB_LAUNCH(2); break;
    case 3: MFS_ATTRIB_LAUNCH(3); break;
    default: MFS_ATTRIB_LAUNCH(4); break;
  }
#undef MFS_ATTRIB_LAUNCH
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
