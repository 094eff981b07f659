// mfs_meshsdf.hip -- triangle-mesh solids on gfx950 (no reference counterpart):
//   k_mesh_distance   exact unsigned distance of every lattice node to a triangle soup, fp32, culled per brick of nodes
//   k_mesh_sign       inside / outside by the parity of ray crossings along array axis 0, one thread per (i1, i2) column
//   k_mesh_union_grid min of a grid's solid level set with the sampled volumes of posed mesh bodies (+ surface velocity)
//   k_mesh_project    particles inside a mesh body out along the gradient of its sampled volume
// Triangles travel as F x 9 float32 (three corners); a volume as n0 x n1 x n2 float32, node (0,0,0) at `origin`.
#include <math.h>

#include "mfs_common.h"
#include "mfs_volume.h"

namespace mfs {

constexpr int kMeshBlock = 256;        // threads per workgroup = triangles per LDS batch
constexpr int kB0 = 4, kB1 = 8, kB2 = 8;   // brick of nodes owned by one workgroup of k_mesh_distance (i2 fastest)
constexpr int kC1 = 16, kC2 = 16;      // tile of columns owned by one workgroup of k_mesh_sign (i2 fastest)

struct Lattice {
  int n[3];
  double org[3];
  double h;
};

// squared distance from p to triangle (a, b, c): Ericson's closest point, region by region.  The caller has dropped
// zero-area triangles (their longest edge belongs to a neighbour in a closed mesh), so va + vb + vc > 0 in the face region.
__device__ __forceinline__ float tri_dist2(const float p[3], const float* __restrict__ t) {
  const float ab[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]};
  const float ac[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
  const float ap[3] = {p[0] - t[0], p[1] - t[1], p[2] - t[2]};
  const float d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2];
  const float d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
  float q[3];                                   // closest point - p
  if (d1 <= 0.f && d2 <= 0.f) {
    for (int k = 0; k < 3; ++k) q[k] = ap[k];
  } else {
    const float bp[3] = {p[0] - t[3], p[1] - t[4], p[2] - t[5]};
    const float d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2];
    const float d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    const float cp[3] = {p[0] - t[6], p[1] - t[7], p[2] - t[8]};
    const float d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2];
    const float d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d3 >= 0.f && d4 <= d3) {
      for (int k = 0; k < 3; ++k) q[k] = bp[k];
    } else if (d6 >= 0.f && d5 <= d6) {
      for (int k = 0; k < 3; ++k) q[k] = cp[k];
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
      const float v = d1 / (d1 - d3);
      for (int k = 0; k < 3; ++k) q[k] = ap[k] - v * ab[k];
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
      const float w = d2 / (d2 - d6);
      for (int k = 0; k < 3; ++k) q[k] = ap[k] - w * ac[k];
    } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
      const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
      for (int k = 0; k < 3; ++k) q[k] = bp[k] - w * (t[6 + k] - t[3 + k]);
    } else {
      const float denom = 1.f / (va + vb + vc);
      const float v = vb * denom, w = vc * denom;
      for (int k = 0; k < 3; ++k) q[k] = ap[k] - (v * ab[k] + w * ac[k]);
    }
  }
  return q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
}

__device__ __forceinline__ bool tri_zero_area(const float* t) {
#pragma clang fp contract(off)      // (a, b, b) must give exactly 0: a contracted a1 b2 - a2 b1 leaves the product's rounding error
  const float ab[3] = {t[3] - t[0], t[4] - t[1], t[5] - t[2]};
  const float ac[3] = {t[6] - t[0], t[7] - t[1], t[8] - t[2]};
  const float n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
  return !(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] > 0.f);
}

// Compaction of one batch: lane `tid` holds a triangle in `t` and whether it is kept; the kept ones land in s_tri in lane
// order (wave ballots, then the four wave totals in order -- no atomics).  Returns the number kept; ends with a barrier.
__device__ __forceinline__ int compact_batch(const float t[9], bool keep, float (*s_tri)[9], int* s_wave) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
  const unsigned long long mask = __ballot(keep);
  const int below = __popcll(mask & ((1ull << lane) - 1ull));
  if (lane == 0) s_wave[wid] = __popcll(mask);
  __syncthreads();
  int off = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kMeshBlock / kWave; ++w) {
    const int c = s_wave[w];
    if (w < wid) off += c;
    total += c;
  }
  if (keep)
    for (int k = 0; k < 9; ++k) s_tri[off + below][k] = t[k];
  __syncthreads();
  return total;
}

// One workgroup per brick of kB0 x kB1 x kB2 nodes.  Sweep 1: Dc, the distance from the brick centre c to the nearest of
// the triangles' corners and centroids -- points of the mesh, so an upper bound on c's distance, at a few flops a triangle
// (lane per triangle, block minimum); every node x of the brick then has dist(x) <= Dc + hd, hd the half diagonal.  Sweep 2:
// a triangle inside the sphere (s, r) has every point at least |s - c| - r - hd from every node, so it cannot carry a
// node's minimum when |s - c| > Dc + 2 hd + r; it is dropped (plus a rounding slack).  Survivors of each batch are
// compacted into LDS and all lanes loop over them: uniform control flow, broadcast LDS reads.
// survivors (may be null): per brick, the number of triangles that reached the inner loop.
__global__ void __launch_bounds__(kMeshBlock)
k_mesh_distance(Lattice L, const float* __restrict__ tri, int F, int cull, float* __restrict__ phi,
                int* __restrict__ survivors) {
  __shared__ float s_tri[kMeshBlock][9];
  __shared__ int s_wave[kMeshBlock / kWave];
  __shared__ float s_min[kMeshBlock / kWave];
  const int tid = threadIdx.x;
  const int b0 = blockIdx.z * kB0, b1 = blockIdx.y * kB1, b2 = blockIdx.x * kB2;
  const int i2 = b2 + (tid % kB2), i1 = b1 + (tid / kB2) % kB1, i0 = b0 + tid / (kB2 * kB1);
  const bool live = i0 < L.n[0] && i1 < L.n[1] && i2 < L.n[2];
  const float h = (float)L.h;
  const float p[3] = {(float)(L.org[0] + i0 * L.h), (float)(L.org[1] + i1 * L.h), (float)(L.org[2] + i2 * L.h)};
  const float c[3] = {(float)(L.org[0] + (b0 + 0.5 * (kB0 - 1)) * L.h), (float)(L.org[1] + (b1 + 0.5 * (kB1 - 1)) * L.h),
                      (float)(L.org[2] + (b2 + 0.5 * (kB2 - 1)) * L.h)};
  const float hd = 0.5f * h * sqrtf((float)((kB0 - 1) * (kB0 - 1) + (kB1 - 1) * (kB1 - 1) + (kB2 - 1) * (kB2 - 1)));

  float reach = INFINITY;                            // triangles whose sphere lies beyond it from c are dropped
  if (cull) {
    float m = INFINITY;
    for (int f = tid; f < F; f += kMeshBlock) {
      float t[9];
      for (int k = 0; k < 9; ++k) t[k] = tri[(int64_t)f * 9 + k];
      const float q[4][3] = {{t[0], t[1], t[2]}, {t[3], t[4], t[5]}, {t[6], t[7], t[8]},
                             {(t[0] + t[3] + t[6]) * (1.f / 3.f), (t[1] + t[4] + t[7]) * (1.f / 3.f), (t[2] + t[5] + t[8]) * (1.f / 3.f)}};
      if (tri_zero_area(t)) continue;               // sweep 2 skips it: it may not lower the bound either
      for (int v = 0; v < 4; ++v) {
        const float e[3] = {q[v][0] - c[0], q[v][1] - c[1], q[v][2] - c[2]};
        m = fminf(m, e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
      }
    }
    for (int s = kWave / 2; s > 0; s >>= 1) m = fminf(m, __shfl_xor(m, s));
    if ((tid & (kWave - 1)) == 0) s_min[tid / kWave] = m;
    __syncthreads();
    m = fminf(fminf(s_min[0], s_min[1]), fminf(s_min[2], s_min[3]));
    const float U = sqrtf(m) + hd;                   // upper bound on any node's distance (inf for an empty mesh)
    reach = U + hd;
    reach += 1e-3f * reach + 1e-30f;                 // slack: fp32 rounding of Dc, of |s - c| and of r is ~1e-6 relative
  }

  float best = INFINITY;
  int kept_total = 0;
  for (int f0 = 0; f0 < F; f0 += kMeshBlock) {
    const int f = f0 + tid;
    float t[9];
    bool keep = false;
    if (f < F) {
      for (int k = 0; k < 9; ++k) t[k] = tri[(int64_t)f * 9 + k];
      keep = !tri_zero_area(t);
      if (keep && cull) {
        const float s[3] = {(t[0] + t[3] + t[6]) * (1.f / 3.f), (t[1] + t[4] + t[7]) * (1.f / 3.f), (t[2] + t[5] + t[8]) * (1.f / 3.f)};
        float r2 = 0.f;
        for (int v = 0; v < 3; ++v) {
          const float e[3] = {t[3 * v] - s[0], t[3 * v + 1] - s[1], t[3 * v + 2] - s[2]};
          r2 = fmaxf(r2, e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        }
        const float r = sqrtf(r2) * 1.001f;
        const float e[3] = {s[0] - c[0], s[1] - c[1], s[2] - c[2]};
        keep = !(sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) > reach + r);
      }
    }
    const int kept = compact_batch(t, keep, s_tri, s_wave);
    kept_total += kept;
    for (int j = 0; j < kept; ++j) best = fminf(best, tri_dist2(p, s_tri[j]));
    __syncthreads();                                 // s_tri is rewritten by the next batch
  }
  if (live) phi[((int64_t)i0 * L.n[1] + i1) * L.n[2] + i2] = sqrtf(best);
  if (survivors && tid == 0) survivors[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = kept_total;
}

// From here on every expression rounds as written: the sign pass needs the two triangles of an edge to evaluate the SAME
// bits, and the union / projection kernels are restated in numpy operation by operation (tests/meshsdf_numpy.py; their
// sampler is mfs_volume.h's).  The
// distance kernel above keeps the compiler's default contraction: cull on / off run the same code, so they still agree
// bit for bit.
#pragma clang fp contract(off)

// sign of the 2x2 determinant | p  q | of two points seen from the column, with the ties of a vanishing determinant
// broken as by an infinitesimal shift of the column (Bridson's `orientation`): antisymmetric in (p, q) mathematically.
__device__ __forceinline__ int orient2(double p1, double p2, double q1, double q2) {
  const double det = p2 * q1 - p1 * q2;
  if (det > 0) return 1;
  if (det < 0) return -1;
  if (q2 > p2) return 1;
  if (q2 < p2) return -1;
  if (p1 > q1) return 1;
  if (p1 < q1) return -1;
  return 0;
}

// The same edge seen from either of its two triangles: the corners are put in lexicographic order of their float32
// coordinates before the determinant is formed, and the result negated when that swapped them, so both triangles get
// bit-identical products and exactly opposite signs.  Also returns the determinant in *det (with the triangle's sense).
__device__ __forceinline__ int edge_sign(const float* P, const float* Q, double y, double z, double* det) {
  const bool swap = (Q[1] < P[1]) || (Q[1] == P[1] && (Q[2] < P[2] || (Q[2] == P[2] && Q[0] < P[0])));
  const float* A = swap ? Q : P;
  const float* B = swap ? P : Q;
  const double a1 = (double)A[1] - y, a2 = (double)A[2] - z, b1 = (double)B[1] - y, b2 = (double)B[2] - z;
  const double d = a2 * b1 - a1 * b2;
  const int s = orient2(a1, a2, b1, b2);
  *det = swap ? -d : d;
  return swap ? -s : s;
}

// One thread per (i1, i2) column, a workgroup per kC1 x kC2 tile.  Triangles are staged through LDS in batches; those
// whose projected box misses the tile are dropped at staging (closed-interval test: conservative).  A crossing toggles
// the sign bit of phi (>= 0 on entry, the unsigned distance) at the first node at or above it -- the column belongs to
// this thread alone, so there are no atomics -- and a running parity over the column then sets the final signs.
// odd[i1 * n2 + i2] = 1 when the column's total crossing count is odd (the mesh is not closed).
__global__ void __launch_bounds__(kMeshBlock)
k_mesh_sign(Lattice L, const float* __restrict__ tri, int F, float* __restrict__ phi, int* __restrict__ odd) {
  __shared__ float s_tri[kMeshBlock][9];
  __shared__ int s_wave[kMeshBlock / kWave];
  const int tid = threadIdx.x;
  const int b1 = blockIdx.y * kC1, b2 = blockIdx.x * kC2;
  const int i1 = b1 + tid / kC2, i2 = b2 + tid % kC2;
  const bool live = i1 < L.n[1] && i2 < L.n[2];
  const double y = L.org[1] + i1 * L.h, z = L.org[2] + i2 * L.h;
  const double ylo = L.org[1] + b1 * L.h, yhi = L.org[1] + (b1 + kC1 - 1) * L.h;
  const double zlo = L.org[2] + b2 * L.h, zhi = L.org[2] + (b2 + kC2 - 1) * L.h;
  const int64_t plane = (int64_t)L.n[1] * L.n[2], col = (int64_t)i1 * L.n[2] + i2;
  unsigned* bits = reinterpret_cast<unsigned*>(phi);
  int total = 0;
  for (int f0 = 0; f0 < F; f0 += kMeshBlock) {
    const int f = f0 + tid;
    float t[9];
    bool keep = false;
    if (f < F) {
      for (int k = 0; k < 9; ++k) t[k] = tri[(int64_t)f * 9 + k];
      const float y0 = fminf(t[1], fminf(t[4], t[7])), y1 = fmaxf(t[1], fmaxf(t[4], t[7]));
      const float z0 = fminf(t[2], fminf(t[5], t[8])), z1 = fmaxf(t[2], fmaxf(t[5], t[8]));
      keep = (double)y1 >= ylo && (double)y0 <= yhi && (double)z1 >= zlo && (double)z0 <= zhi;
    }
    const int kept = compact_batch(t, keep, s_tri, s_wave);
    if (live) {
      for (int j = 0; j < kept; ++j) {
        const float* A = s_tri[j];
        const float* B = A + 3;
        const float* C = A + 6;
        double ea, eb, ec;                               // determinants opposite A, B, C
        const int sa = edge_sign(B, C, y, z, &ea);
        if (sa == 0) continue;
        const int sb = edge_sign(C, A, y, z, &eb);
        if (sb != sa) continue;
        const int sc = edge_sign(A, B, y, z, &ec);
        if (sc != sa) continue;
        const double sum = ea + eb + ec;                 // twice the projected area
        if (sum == 0.0) continue;
        const double x = (ea / sum) * (double)A[0] + (eb / sum) * (double)B[0] + (ec / sum) * (double)C[0];
        const double fi = ceil((x - L.org[0]) / L.h);
        ++total;
        if (fi < (double)L.n[0]) {
          const int i0 = fi < 0.0 ? 0 : (int)fi;
          bits[i0 * plane + col] ^= 0x80000000u;
        }
      }
    }
    __syncthreads();
  }
  if (live) {
    unsigned parity = 0u;
    for (int i0 = 0; i0 < L.n[0]; ++i0) {
      const unsigned v = bits[i0 * plane + col];
      parity ^= v & 0x80000000u;
      bits[i0 * plane + col] = (v & 0x7fffffffu) | parity;
    }
    odd[col] = total & 1;
  }
}

// ------------------------------------------------------------------------------------------- posed mesh bodies ----
// The bodies' volumes travel as mfs_volume.h's Volumes, float32 all (dt = MFS_F32); their poses are read from the device
// body table.
struct MeshPose {
  double T[3];
  double R[3][3];
  double vel[3];
};

__device__ __forceinline__ MeshPose pose_load(const double* __restrict__ rb, int i) {
  const double* b = rb + (int64_t)i * 40;
  MeshPose r;
  for (int k = 0; k < 3; ++k) r.T[k] = b[(1 + k) * 4 + 3];
  for (int a = 0; a < 3; ++a)
    for (int c = 0; c < 3; ++c) r.R[a][c] = b[(5 + a) * 4 + c];
  for (int k = 0; k < 3; ++k) r.vel[k] = b[9 * 4 + k];
  return r;
}

// sd / vel hold a solid level set already (k_sdf_evaluate_grid's, or any); every mesh body in turn: d < sd -> sd = d and
// vel = (d <= 0 ? v + w x (x - T) : 0), k_sdf_evaluate_grid's rule.  The running minimum is kept in float64 across the
// bodies and stored once; nodes no body wins are not written.
__global__ void __launch_bounds__(256)
k_mesh_union_grid(const double* __restrict__ rb, const double* __restrict__ rb_w, int m, Volumes V, GridArgs3 a,
                  void* sd, int sdt, void* vel, int vdt) {
  const int64_t base = (int64_t)blockIdx.x * 256;
  const int64_t p = base + threadIdx.x;
  if (p >= a.total) return;
  const LatticeIndex at = lattice_split(base, threadIdx.x, a.n1, a.n2);
  const double pos[3] = {a.bmin[0] + (double)((float)at.i0 + a.bias[0]) * a.cs[0],
                         a.bmin[1] + (double)((float)at.i1 + a.bias[1]) * a.cs[1],
                         a.bmin[2] + (double)((float)at.i2 + a.bias[2]) * a.cs[2]};
  double cur = ldx(sd, sdt, p);
  double v[3] = {0.0, 0.0, 0.0};
  bool won = false;
  for (int i = 0; i < m; ++i) {
    const MeshPose r = pose_load(rb, i);
    double xb[3];
    pose_to_body(r.R, r.T, pos, xb);
    const double d = volume_sample<true>(V, i, xb);
    if (d < cur) {
      cur = d;
      won = true;
      for (int k = 0; k < 3; ++k) v[k] = 0.0;
      if (d <= 0) {
        for (int k = 0; k < 3; ++k) v[k] = r.vel[k];
        if (rb_w) {
          const double w[3] = {rb_w[3 * i], rb_w[3 * i + 1], rb_w[3 * i + 2]};
          const double x[3] = {pos[0] - r.T[0], pos[1] - r.T[1], pos[2] - r.T[2]};
          v[0] = r.vel[0] + (w[1] * x[2] - w[2] * x[1]);
          v[1] = r.vel[1] + (w[2] * x[0] - w[0] * x[2]);
          v[2] = r.vel[2] + (w[0] * x[1] - w[1] * x[0]);
        }
      }
    }
  }
  if (won) {
    stx(sd, sdt, p, cur);
    for (int k = 0; k < 3; ++k) stx(vel, vdt, 3 * p + k, v[k]);
  }
}

// every mesh body in turn, each on the position the previous one left (float32 positions round per body, as
// k_sdf_project): sampled d < 0 -> x -= d * R n, n the normalised gradient of the sampled volume.  A vanishing gradient
// falls back to central differences of samples one spacing apart; still zero: the particle stays.  d >= 0: no store.
__global__ void __launch_bounds__(256)
k_mesh_project(const double* __restrict__ rb, int m, Volumes V, void* position, int pdt, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  double pos[3] = {ldx(position, pdt, 3 * p), ldx(position, pdt, 3 * p + 1), ldx(position, pdt, 3 * p + 2)};
  bool moved = false;
  for (int i = 0; i < m; ++i) {
    const MeshPose r = pose_load(rb, i);
    double xb[3], g[3];
    pose_to_body(r.R, r.T, pos, xb);
    const double d = volume_sample<true>(V, i, xb, nullptr, nullptr, g);
    if (!(d < 0)) continue;
    double nn = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    if (!(nn > 0)) {
      for (int k = 0; k < 3; ++k) {
        double xp[3] = {xb[0], xb[1], xb[2]}, xm[3] = {xb[0], xb[1], xb[2]};
        xp[k] += V.h[i];
        xm[k] -= V.h[i];
        g[k] = volume_sample<true>(V, i, xp) - volume_sample<true>(V, i, xm);
      }
      nn = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
      if (!(nn > 0)) continue;
    }
    const double n[3] = {g[0] / nn, g[1] / nn, g[2] / nn};
    for (int k = 0; k < 3; ++k) {
      const double nw = (r.R[k][0] * n[0] + r.R[k][1] * n[1]) + r.R[k][2] * n[2];
      pos[k] = pos[k] - d * nw;
      if (pdt == MFS_F32) pos[k] = (double)(float)pos[k];
    }
    moved = true;
  }
  if (moved)
    for (int k = 0; k < 3; ++k) stx(position, pdt, 3 * p + k, pos[k]);
}

static int fill_lattice(Lattice* L, const int64_t shape[3], const double origin[3], double spacing) {
  if (int st = check_lattice(shape, origin, spacing)) return st;
  for (int k = 0; k < 3; ++k) {
    L->n[k] = (int)shape[k];
    L->org[k] = origin[k];
  }
  L->h = spacing;
  return MFS_OK;
}

// the bodies' volumes of a C entry point: float32, no host poses
static int fill_mesh_volumes(Volumes* V, int64_t m, const void* const* volumes_host, const int64_t* extents_host,
                             const double* origins_host, const double* spacings_host) {
  MFS_REQUIRE(m >= 0 && m <= kMaxVolumes, "at most 16 mesh bodies per call");
  MFS_REQUIRE(m == 0 || (volumes_host && extents_host && origins_host && spacings_host), "null mesh volume description");
  return fill_volumes(V, nullptr, (int)m, volumes_host, nullptr, extents_host, origins_host, spacings_host, nullptr);
}

}  // namespace mfs

using namespace mfs;

extern "C" {

int64_t mfs_meshsdf_bricks3d(const int64_t shape[3]) {
  if (!shape || shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return 0;
  return (int64_t)cdiv(shape[0], kB0) * cdiv(shape[1], kB1) * cdiv(shape[2], kB2);
}

int mfs_meshsdf_distance3d(const int64_t shape[3], const double origin[3], double spacing, const void* triangles,
                           int64_t num_triangles, int cull, void* phi, void* survivors, mfs_stream stream) {
  Lattice L;
  if (int st = fill_lattice(&L, shape, origin, spacing)) return st;
  MFS_REQUIRE(num_triangles >= 1 && num_triangles <= 0x7fffffff / 9 && triangles, "triangles");
  MFS_REQUIRE(phi, "null phi");
  const dim3 grid(cdiv(L.n[2], kB2), cdiv(L.n[1], kB1), cdiv(L.n[0], kB0));
  MFS_REQUIRE(grid.y <= 65535 && grid.z <= 65535, "lattice too long for one launch");
  hipLaunchKernelGGL(k_mesh_distance, grid, dim3(kMeshBlock), 0, (hipStream_t)stream, L, (const float*)triangles,
                     (int)num_triangles, cull, (float*)phi, (int*)survivors);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_meshsdf_sign3d(const int64_t shape[3], const double origin[3], double spacing, const void* triangles,
                       int64_t num_triangles, void* phi, void* odd_columns, mfs_stream stream) {
  Lattice L;
  if (int st = fill_lattice(&L, shape, origin, spacing)) return st;
  MFS_REQUIRE(num_triangles >= 1 && num_triangles <= 0x7fffffff / 9 && triangles, "triangles");
  MFS_REQUIRE(phi && odd_columns, "null phi / odd_columns");
  const dim3 grid(cdiv(L.n[2], kC2), cdiv(L.n[1], kC1));
  MFS_REQUIRE(grid.y <= 65535, "lattice too long for one launch");
  hipLaunchKernelGGL(k_mesh_sign, grid, dim3(kMeshBlock), 0, (hipStream_t)stream, L, (const float*)triangles,
                     (int)num_triangles, (float*)phi, (int*)odd_columns);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_mesh_union_grid3d(const void* mesh_rb, const void* rb_w, int64_t num_bodies, const void* const* volumes_host,
                          const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                          const int64_t res[3], const double bound_min[3], const double bias[3],
                          const double cell_size[3], void* sd, int sd_dt, void* vel, int vel_dt, mfs_stream stream) {
  Volumes V;
  if (int st = fill_mesh_volumes(&V, num_bodies, volumes_host, extents_host, origins_host, spacings_host)) return st;
  MFS_REQUIRE(num_bodies == 0 || mesh_rb, "null mesh_rb");
  GridArgs3 a;
  if (int st = fill_grid_args(&a, res, bound_min, bias, cell_size)) return st;
  MFS_REQUIRE(dtype_ok(sd_dt) && dtype_ok(vel_dt), "dtype");
  if (a.total == 0 || num_bodies == 0) return MFS_OK;
  MFS_REQUIRE(sd && vel, "null output arrays");
  hipLaunchKernelGGL(k_mesh_union_grid, dim3(cdiv(a.total, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const double*)mesh_rb, (const double*)rb_w, (int)num_bodies, V, a, sd, sd_dt, vel, vel_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_mesh_project3d(const void* mesh_rb, int64_t num_bodies, const void* const* volumes_host,
                       const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                       void* position, int pos_dt, int64_t num_positions, mfs_stream stream) {
  Volumes V;
  if (int st = fill_mesh_volumes(&V, num_bodies, volumes_host, extents_host, origins_host, spacings_host)) return st;
  MFS_REQUIRE(num_bodies == 0 || mesh_rb, "null mesh_rb");
  MFS_REQUIRE(num_positions >= 0 && (num_positions == 0 || position), "null position array");
  MFS_REQUIRE(dtype_ok(pos_dt), "dtype");
  if (num_positions == 0 || num_bodies == 0) return MFS_OK;
  MFS_REQUIRE(num_positions <= (int64_t)0x7fffffff * 256, "too many positions for one launch");
  hipLaunchKernelGGL(k_mesh_project, dim3(cdiv(num_positions, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const double*)mesh_rb, (int)num_bodies, V, position, pos_dt, num_positions);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
