// mfs_seed.hip -- liquid seeded from level-set volumes on gfx950 (no reference counterpart):
//   k_seed_count   one lane per site of the particle lattice: hash -> jittered position -> sample every shape -> keep or not;
//                  the workgroup stores its four ballot masks and its count
//   k_seed_fill    ranks the kept lanes by popcounts of those masks and stores position (and site index) at offset + rank
// Between the two: an exclusive scan of the counts (the caller's).  No atomics: kept sites come out in ascending site
// index, and two calls store the same bits.
#include <math.h>

#include "mfs_common.h"
#include "mfs_volume.h"

namespace mfs {

constexpr int kSeedBlock = 256;            // threads per workgroup = consecutive site indices owned by it
constexpr int kSeedWaves = kSeedBlock / kWave;

struct SeedLattice {
  int64_t n1, n2, total;     // extents of the two inner axes, number of sites
  double org[3];
  double h;
  double jitter;
  uint32_t seed_lo, seed_hi;
};

// Every expression below rounds as written: the position is restated in numpy bit for bit (tests/seed_numpy.py), as is the
// sampler (mfs_volume.h).
#pragma clang fp contract(off)

__device__ __forceinline__ uint32_t seed_mix(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// x_a = origin_a + ((i_a + 0.5) + jitter * u_a) * h, u_a in [-0.5, 0.5) a pure function of (seed, s, a)
__device__ __forceinline__ void seed_position(const SeedLattice& L, int64_t s, const LatticeIndex& at, double x[3]) {
  const double idx[3] = {(double)at.i0, (double)at.i1, (double)at.i2};
  uint32_t hs = seed_mix(L.seed_lo);
  hs = seed_mix(hs ^ L.seed_hi);
  hs = seed_mix(hs ^ (uint32_t)((uint64_t)s & 0xffffffffu));
  hs = seed_mix(hs ^ (uint32_t)((uint64_t)s >> 32));
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const uint32_t ha = seed_mix(hs + (uint32_t)(a + 1) * 0x9E3779B9u);
    const double u = (double)(ha >> 8) * 0x1p-24 - 0.5;
    const double ju = L.jitter * u;
    const double c = (idx[a] + 0.5) + ju;
    const double ch = c * L.h;
    x[a] = L.org[a] + ch;
  }
}

// shape i at the world point x: its volume sampled at the body-frame point R^T (x - T)
__device__ __forceinline__ double seed_sample(const Volumes& V, const Poses& P, int i, const double x[3]) {
  double xb[3];
  pose_to_body(P.R[i], P.T[i], x, xb);
  return volume_sample(V, i, xb);
}

// minimum that keeps a NaN once it has seen one (numpy's np.minimum): a NaN sample then fails both comparisons below
__device__ __forceinline__ double seed_min(double m, double d) { return (d < m || d != d) ? d : m; }

// kept iff min over includes < 0 and min over excludes > clearance, both strict.  The excludes are sampled only where the
// includes keep the site: the decision is the same, and most of a lattice is outside the liquid.
// counts (may be null): per workgroup, the number kept; masks (may be null): per workgroup, the four waves' ballots.
__global__ void __launch_bounds__(kSeedBlock)
k_seed_count(SeedLattice L, Volumes V, Poses P, int n_inc, int n_exc, double clearance, int* __restrict__ counts,
             unsigned long long* __restrict__ masks) {
  __shared__ int s_wave[kSeedWaves];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * kSeedBlock;
  const int64_t s = base + tid;
  bool keep = false;
  if (s < L.total) {
    double x[3];
    seed_position(L, s, lattice_split(base, tid, L.n1, L.n2), x);
    double inc = INFINITY;
    for (int i = 0; i < n_inc; ++i) inc = seed_min(inc, seed_sample(V, P, i, x));
    if (inc < 0.0) {
      double exc = INFINITY;
      for (int i = n_inc; i < n_inc + n_exc; ++i) exc = seed_min(exc, seed_sample(V, P, i, x));
      keep = exc > clearance;
    }
  }
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) {
    s_wave[wid] = __popcll(mask);
    if (masks) masks[(int64_t)blockIdx.x * kSeedWaves + wid] = mask;
  }
  __syncthreads();
  if (tid == 0 && counts) {
    int total = 0;
#pragma unroll
    for (int w = 0; w < kSeedWaves; ++w) total += s_wave[w];
    counts[blockIdx.x] = total;
  }
}

// offsets[b]: the number kept in the workgroups before b.  A kept lane's rank inside its workgroup: the waves before its
// own in order, then the lanes below it.  Nothing is sampled again; the position comes from the hash as in the count pass.
// sites (may be null): the kept sites' indices.  capacity: rows of px / sites; a rank beyond it is not stored.
__global__ void __launch_bounds__(kSeedBlock)
k_seed_fill(SeedLattice L, const unsigned long long* __restrict__ masks, const int64_t* __restrict__ offsets, void* px,
            int pdt, int64_t* __restrict__ sites, int64_t capacity) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const int64_t base = (int64_t)blockIdx.x * kSeedBlock;
  const int64_t s = base + tid;
  int before = 0;
  unsigned long long mine = 0ull;
#pragma unroll
  for (int w = 0; w < kSeedWaves; ++w) {
    const unsigned long long m = masks[(int64_t)blockIdx.x * kSeedWaves + w];
    if (w < wid) before += __popcll(m);
    if (w == wid) mine = m;
  }
  if (!((mine >> lane) & 1ull) || s >= L.total) return;
  const int64_t row = offsets[blockIdx.x] + before + __popcll(mine & ((1ull << lane) - 1ull));
  if (row < 0 || row >= capacity) return;
  double x[3];
  seed_position(L, s, lattice_split(base, tid, L.n1, L.n2), x);
  for (int a = 0; a < 3; ++a) stx(px, pdt, 3 * row + a, x[a]);
  if (sites) sites[row] = s;
}

static int fill_seed_lattice(SeedLattice* L, const int64_t shape[3], const double origin[3], double spacing, double jitter,
                             uint64_t seed) {
  MFS_REQUIRE(shape && origin, "null lattice description");
  const int64_t lim = (int64_t)1 << 30;
  MFS_REQUIRE(shape[0] >= 1 && shape[1] >= 1 && shape[2] >= 1 && shape[0] <= lim && shape[1] <= lim && shape[2] <= lim,
              "site lattice extents must be in 1 .. 2^30");
  MFS_REQUIRE(spacing > 0 && isfinite(spacing), "spacing must be positive");
  MFS_REQUIRE(jitter >= 0 && jitter <= 1, "jitter must be in [0, 1]");
  MFS_REQUIRE(shape[0] * shape[1] <= ((int64_t)0x7fffffff * kSeedBlock) / shape[2],
              "site lattice needs more than 2^31 - 1 workgroups");
  for (int k = 0; k < 3; ++k) {
    MFS_REQUIRE(isfinite(origin[k]), "origin must be finite");
    L->org[k] = origin[k];
  }
  L->n1 = shape[1];
  L->n2 = shape[2];
  L->total = shape[0] * shape[1] * shape[2];
  L->h = spacing;
  L->jitter = jitter;
  L->seed_lo = (uint32_t)(seed & 0xffffffffu);
  L->seed_hi = (uint32_t)(seed >> 32);
  return MFS_OK;
}

}  // namespace mfs

using namespace mfs;

extern "C" {

int64_t mfs_seed_blocks3d(const int64_t shape[3]) {
  const int64_t lim = (int64_t)1 << 30;
  if (!shape || shape[0] < 1 || shape[1] < 1 || shape[2] < 1 || shape[0] > lim || shape[1] > lim || shape[2] > lim) return 0;
  const int64_t rows = shape[0] * shape[1];
  if (rows > ((int64_t)1 << 62) / shape[2]) return 0;
  return (rows * shape[2] + kSeedBlock - 1) / kSeedBlock;
}

int mfs_seed_count3d(const int64_t shape[3], const double origin[3], double spacing, double jitter, uint64_t seed,
                     int64_t num_include, int64_t num_exclude, const void* const* volumes_host, const int* dtypes_host,
                     const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                     const double* poses_host, double clearance, void* counts, void* masks, mfs_stream stream) {
  SeedLattice L;
  if (int st = fill_seed_lattice(&L, shape, origin, spacing, jitter, seed)) return st;
  MFS_REQUIRE(num_include >= 0 && num_exclude >= 0 && num_include <= kMaxVolumes &&
              num_exclude <= kMaxVolumes - num_include, "at most 16 shapes per call");
  MFS_REQUIRE(num_include >= 1, "at least one include shape");
  MFS_REQUIRE(volumes_host && dtypes_host && extents_host && origins_host && spacings_host && poses_host,
              "null shape description");
  MFS_REQUIRE(!(clearance != clearance), "clearance is NaN");
  MFS_REQUIRE(counts || masks, "null counts and masks");
  const int m = (int)(num_include + num_exclude);
  Volumes V;
  Poses P;
  if (int st = fill_volumes(&V, &P, m, volumes_host, dtypes_host, extents_host, origins_host, spacings_host, poses_host))
    return st;
  const int64_t blocks = (L.total + kSeedBlock - 1) / kSeedBlock;
  hipLaunchKernelGGL(k_seed_count, dim3((unsigned)blocks), dim3(kSeedBlock), 0, (hipStream_t)stream, L, V, P,
                     (int)num_include, (int)num_exclude, clearance, (int*)counts, (unsigned long long*)masks);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_seed_fill3d(const int64_t shape[3], const double origin[3], double spacing, double jitter, uint64_t seed,
                    const void* masks, const void* offsets, void* positions, int pos_dt, void* sites, int64_t capacity,
                    mfs_stream stream) {
  SeedLattice L;
  if (int st = fill_seed_lattice(&L, shape, origin, spacing, jitter, seed)) return st;
  MFS_REQUIRE(dtype_ok(pos_dt), "dtype");
  MFS_REQUIRE(capacity >= 0 && capacity <= L.total, "capacity");
  if (capacity == 0) return MFS_OK;
  MFS_REQUIRE(masks && offsets && positions, "null masks / offsets / positions");
  const int64_t blocks = (L.total + kSeedBlock - 1) / kSeedBlock;
  hipLaunchKernelGGL(k_seed_fill, dim3((unsigned)blocks), dim3(kSeedBlock), 0, (hipStream_t)stream, L,
                     (const unsigned long long*)masks, (const int64_t*)offsets, positions, pos_dt, (int64_t*)sites, capacity);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
