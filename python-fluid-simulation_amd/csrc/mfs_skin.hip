// mfs_skin.hip -- the liquid's skin on gfx950 (no reference counterpart): Zhu & Bridson's particle
// surface, phi(x) = | sum w_i (x_i - x) | / sum w_i - r with w = max(1 - |x_i - x|^2 / R^2, 0)^3, on a lattice.
//   k_skin_keys    the bin of every particle: the brick of 4 x 8 x 8 nodes it lies in, one ring of bricks around the lattice
//   k_skin_field   one workgroup per brick gathers from the 27 bins around it; no atomics, fp32 on brick-relative coordinates
// The particles arrive sorted by bin (a stable sort by k_skin_keys' key: the order inside a bin is the caller's order),
// with the first particle of every bin in `starts`.
#include <math.h>

#include "mfs_common.h"
#include "mfs_volume.h"

namespace mfs {

constexpr int kSkinBlock = 256;            // threads per workgroup = nodes per brick = particles per LDS batch
constexpr int kS0 = 4, kS1 = 8, kS2 = 8;   // brick of nodes owned by one workgroup (i2 fastest): a wave is one i0 plane
constexpr int kSkinReach = 4;              // influence <= kSkinReach * spacing: the shortest brick edge, so one ring of bins

struct SkinLattice {
  int n[3];        // nodes
  int nb[3];       // bricks; bins are nb + 2 along every axis, bin (c0, c1, c2) the brick (c0 - 1, c1 - 1, c2 - 1)
  double org[3];
  double h;
};

__device__ __forceinline__ int brick_edge(int k) { return k == 0 ? kS0 : (k == 1 ? kS1 : kS2); }

// key[p]: the C-order index of p's bin, or the number of bins when p lies outside the ring (farther than a brick edge,
// so farther than the influence radius, from every node) or is not finite.  Bin c along an axis covers
// [org + (c - 1) E h, org + c E h), E the brick edge in nodes: a node of brick b has all its contributors in bins b .. b + 2.
__global__ void __launch_bounds__(kSkinBlock)
k_skin_keys(SkinLattice L, const void* __restrict__ px, int pdt, int64_t P, int* __restrict__ key) {
  const int64_t p = (int64_t)blockIdx.x * kSkinBlock + threadIdx.x;
  if (p >= P) return;
  int c[3];
  bool ok = true;
  for (int k = 0; k < 3; ++k) {
    const double t = floor((ldx(px, pdt, 3 * p + k) - L.org[k]) / (brick_edge(k) * L.h));
    const bool in = t >= -1.0 && t <= (double)L.nb[k];          // false for NaN
    ok = ok && in;
    c[k] = in ? (int)t + 1 : 0;
  }
  const int m1 = L.nb[1] + 2, m2 = L.nb[2] + 2;
  key[p] = ok ? (c[0] * m1 + c[1]) * m2 + c[2] : (L.nb[0] + 2) * m1 * m2;
}

// One workgroup per brick.  The 27 bins around it are 9 runs of the sorted particles (three bins along axis 2 are
// neighbours in the sort); the runs are walked as one sequence in batches of 256, a lane per candidate.  A candidate
// survives when its distance to the brick's box of nodes is within R (plus slack for the fp32 rounding of that
// distance: a survivor beyond R adds a weight of exactly 0).  Survivors are compacted into LDS in lane order by
// ballots, then ALL lanes loop over them: the trip count is uniform and every LDS read is one 16-byte broadcast.
// A brick whose 27 bins are empty stores the background and leaves before the loop.
// survivors (may be null): per brick, the number of particles that reached the inner loop.
__global__ void __launch_bounds__(kSkinBlock)
k_skin_field(SkinLattice L, float r, float R, float inv_R2, float background, const void* __restrict__ ps, int pdt,
             const int* __restrict__ starts, float* __restrict__ phi, int* __restrict__ survivors) {
  __shared__ float4 s_p[kSkinBlock];
  __shared__ int s_wave[kSkinBlock / kWave];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const int k2 = tid % kS2, k1 = (tid / kS2) % kS1, k0 = tid / (kS2 * kS1);
  const int i0 = blockIdx.z * kS0 + k0, i1 = blockIdx.y * kS1 + k1, i2 = blockIdx.x * kS2 + k2;
  const bool live = i0 < L.n[0] && i1 < L.n[1] && i2 < L.n[2];
  const int64_t node = ((int64_t)i0 * L.n[1] + i1) * L.n[2] + i2;
  const int64_t brick = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;

  int first[9], count[9], total = 0;
  const int m1 = L.nb[1] + 2, m2 = L.nb[2] + 2;
#pragma unroll
  for (int a = 0; a < 9; ++a) {
    const int bin = ((blockIdx.z + a / 3) * m1 + blockIdx.y + a % 3) * m2 + blockIdx.x;
    first[a] = starts[bin];
    count[a] = starts[bin + 3] - first[a];
    total += count[a];
  }
  if (total == 0) {                                        // uniform over the workgroup
    if (live) phi[node] = background;
    if (survivors && tid == 0) survivors[brick] = 0;
    return;
  }

  // everything below is relative to the brick's first node, subtracted in fp64: scene offsets cost no fp32 digits
  const double borg[3] = {L.org[0] + (double)(blockIdx.z * kS0) * L.h, L.org[1] + (double)(blockIdx.y * kS1) * L.h,
                          L.org[2] + (double)(blockIdx.x * kS2) * L.h};
  const float x0 = (float)(k0 * L.h), x1 = (float)(k1 * L.h), x2 = (float)(k2 * L.h);
  const float e0 = (float)((kS0 - 1) * L.h), e1 = (float)((kS1 - 1) * L.h), e2 = (float)((kS2 - 1) * L.h);
  const float reach2 = R * R * 1.0001f;

  float W = 0.f, s0 = 0.f, s1 = 0.f, s2 = 0.f;
  int kept_total = 0;
  for (int c0 = 0; c0 < total; c0 += kSkinBlock) {
    int src = -1, rem = c0 + tid;                          // candidate c0 + tid of the nine runs laid end to end
#pragma unroll
    for (int a = 0; a < 9; ++a) {
      if (rem >= 0 && rem < count[a]) src = first[a] + rem;
      rem -= count[a];
    }
    float4 q = {0.f, 0.f, 0.f, 0.f};
    bool keep = false;
    if (src >= 0) {
      q.x = (float)(ldx(ps, pdt, 3 * (int64_t)src) - borg[0]);
      q.y = (float)(ldx(ps, pdt, 3 * (int64_t)src + 1) - borg[1]);
      q.z = (float)(ldx(ps, pdt, 3 * (int64_t)src + 2) - borg[2]);
      const float g0 = fmaxf(fmaxf(-q.x, q.x - e0), 0.f), g1 = fmaxf(fmaxf(-q.y, q.y - e1), 0.f);
      const float g2 = fmaxf(fmaxf(-q.z, q.z - e2), 0.f);
      keep = g0 * g0 + g1 * g1 + g2 * g2 <= reach2;
    }
    const unsigned long long mask = __ballot(keep);
    if (lane == 0) s_wave[wid] = __popcll(mask);
    __syncthreads();
    int off = 0, kept = 0;
#pragma unroll
    for (int w = 0; w < kSkinBlock / kWave; ++w) {
      const int c = s_wave[w];
      if (w < wid) off += c;
      kept += c;
    }
    if (keep) s_p[off + __popcll(mask & ((1ull << lane) - 1ull))] = q;
    __syncthreads();
    kept_total += kept;
    for (int j = 0; j < kept; ++j) {
      const float4 p = s_p[j];
      const float d0 = p.x - x0, d1 = p.y - x1, d2 = p.z - x2;
      const float t = fmaxf(1.f - (d0 * d0 + d1 * d1 + d2 * d2) * inv_R2, 0.f);
      const float w = t * t * t;
      W += w;
      s0 += w * d0;
      s1 += w * d1;
      s2 += w * d2;
    }
    __syncthreads();                                       // s_p and s_wave are rewritten by the next batch
  }
  if (live) {
    float v = background;
    if (W > 0.f) {                                         // divide first: the squares of w d underflow at the rim
      const float a0 = s0 / W, a1 = s1 / W, a2 = s2 / W;
      v = sqrtf(a0 * a0 + a1 * a1 + a2 * a2) - r;
    }
    phi[node] = v;
  }
  if (survivors && tid == 0) survivors[brick] = kept_total;
}

static int fill_skin_lattice(SkinLattice* L, const int64_t shape[3], const double origin[3], double spacing) {
  if (int st = check_lattice(shape, origin, spacing)) return st;
  for (int k = 0; k < 3; ++k) {
    L->n[k] = (int)shape[k];
    L->org[k] = origin[k];
  }
  L->nb[0] = cdiv(shape[0], kS0);
  L->nb[1] = cdiv(shape[1], kS1);
  L->nb[2] = cdiv(shape[2], kS2);
  L->h = spacing;
  MFS_REQUIRE((int64_t)(L->nb[0] + 2) * (L->nb[1] + 2) < ((int64_t)1 << 31) / (L->nb[2] + 2), "too many bins");
  MFS_REQUIRE(L->nb[0] <= 65535 && L->nb[1] <= 65535, "lattice too long for one launch");
  return MFS_OK;
}

}  // namespace mfs

using namespace mfs;

extern "C" {

int64_t mfs_skin_bricks3d(const int64_t shape[3]) {
  if (!shape || shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return 0;
  return (int64_t)cdiv(shape[0], kS0) * cdiv(shape[1], kS1) * cdiv(shape[2], kS2);
}

int64_t mfs_skin_bins3d(const int64_t shape[3]) {
  if (!shape || shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return 0;
  return (int64_t)(cdiv(shape[0], kS0) + 2) * (cdiv(shape[1], kS1) + 2) * (cdiv(shape[2], kS2) + 2);
}

int mfs_skin_keys3d(const int64_t shape[3], const double origin[3], double spacing, const void* particles, int p_dt,
                    int64_t num_particles, void* keys, mfs_stream stream) {
  SkinLattice L;
  if (int st = fill_skin_lattice(&L, shape, origin, spacing)) return st;
  MFS_REQUIRE(dtype_ok(p_dt), "dtype");
  MFS_REQUIRE(num_particles >= 0 && num_particles < ((int64_t)1 << 31), "particle count must stay below 2^31");
  if (num_particles == 0) return MFS_OK;
  MFS_REQUIRE(particles && keys, "null particles / keys");
  hipLaunchKernelGGL(k_skin_keys, dim3(cdiv(num_particles, kSkinBlock)), dim3(kSkinBlock), 0, (hipStream_t)stream, L,
                     particles, p_dt, num_particles, (int*)keys);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_skin_field3d(const int64_t shape[3], const double origin[3], double spacing, double radius, double influence,
                     const void* sorted_particles, int p_dt, int64_t num_particles, const void* bin_starts, void* phi,
                     void* survivors, mfs_stream stream) {
  SkinLattice L;
  if (int st = fill_skin_lattice(&L, shape, origin, spacing)) return st;
  MFS_REQUIRE(radius > 0 && isfinite(radius) && isfinite(influence) && influence > radius, "0 < radius < influence");
  MFS_REQUIRE(influence <= kSkinReach * spacing, "influence must not exceed 4 * spacing (one ring of neighbour bricks)");
  MFS_REQUIRE(dtype_ok(p_dt), "dtype");
  MFS_REQUIRE(num_particles >= 0 && num_particles < ((int64_t)1 << 31), "particle count must stay below 2^31");
  MFS_REQUIRE(num_particles == 0 || sorted_particles, "null particles");
  MFS_REQUIRE(bin_starts && phi, "null bin_starts / phi");
  const dim3 grid(L.nb[2], L.nb[1], L.nb[0]);
  hipLaunchKernelGGL(k_skin_field, grid, dim3(kSkinBlock), 0, (hipStream_t)stream, L, (float)radius, (float)influence,
                     (float)(1.0 / (influence * influence)), (float)(influence - radius), sorted_particles, p_dt,
                     (const int*)bin_starts, (float*)phi, (int*)survivors);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
