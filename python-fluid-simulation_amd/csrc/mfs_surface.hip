// mfs_surface.hip -- surface extraction on the device: marching tetrahedra over the Kuhn cut of every lattice cube
// (mfs_surface3d_*) and marching triangles over the (1,1) cut of every lattice square (mfs_contour2d_*).  DESIGN.md
// "Surface extraction" states the contract; this file is classify / scan / emit with no atomics, so the output is a
// function of the field alone (two calls are bitwise identical):
//   count   one thread per node of the (extended) lattice, lanes along the last axis: the inside bits of the node's cube
//           corners -> cbits[node]; from them the node's owned-edge mask (its vertex count) and its cube's triangle count;
//           per-tile sums of both
//   scan    one block per quantity: exclusive scan of the tile sums, totals -> the head of the workspace
//   verts   per tile an ordered block scan of the vertex counts -> first[node]; positions (and normals) of the owned edges
//   faces   per tile an ordered block scan of the triangle counts; each triangle looks its three vertex indices up from
//           first[] and the owner's edge mask
// `closed` adds one virtual layer of `outside` samples around the array: sample() answers for it, nothing is padded.
// All arithmetic is fp64 (fp32 samples widened on load); only the stores of positions and normals round to fp32.
#include "mfs_common.h"

namespace mfs {
namespace {

constexpr int kSurfBlock = 256;
constexpr int kSurfPer = 4;                           // nodes per thread
constexpr int kSurfTile = kSurfBlock * kSurfPer;      // nodes per block

// ------------------------------------------------------------------ block helpers ----
// exclusive prefix of v over the block in thread order, block total in `total`; all threads must call
__device__ __forceinline__ int block_excl_scan(int v, int& total) {
  __shared__ int s_w[kSurfBlock / kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int u = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += u;
  }
  __syncthreads();                                    // s_w of the previous call has been read
  if (lane == kWave - 1) s_w[wave] = inc;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kSurfBlock / kWave; ++w) { const int c = s_w[w]; before += w < wave ? c : 0; tot += c; }
  total = tot;
  return before + inc - v;
}

// block totals of two counters, in thread 0
__device__ __forceinline__ void block_sum2(int& a, int& b) {
  __shared__ int s_a[kSurfBlock / kWave], s_b[kSurfBlock / kWave];
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) { a += __shfl_down(a, o, kWave); b += __shfl_down(b, o, kWave); }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) { s_a[wave] = a; s_b[wave] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = 0; b = 0;
    for (int w = 0; w < kSurfBlock / kWave; ++w) { a += s_a[w]; b += s_b[w]; }
  }
}

// exclusive scan of the tile sums in place (one block per array: blockIdx.x picks vertices or faces); the carry is 64-bit so
// that a total past int32 is reported, not wrapped -- the prefixes of a total that fits are exact in their low 32 bits
__global__ void __launch_bounds__(1024)
k_surf_scan(int* __restrict__ bsum_v, int* __restrict__ bsum_f, int nb, long long* __restrict__ totals) {
  int* bsum = blockIdx.x == 0 ? bsum_v : bsum_f;
  __shared__ long long s_pre[1024];
  __shared__ long long s_carry;
  const int t = threadIdx.x;
  if (t == 0) s_carry = 0;
  __syncthreads();
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const long long v = b0 + t < nb ? bsum[b0 + t] : 0;
    s_pre[t] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const long long u = t >= o ? s_pre[t - o] : 0;
      __syncthreads();
      s_pre[t] += u;
      __syncthreads();
    }
    const long long carry = s_carry;
    if (b0 + t < nb) bsum[b0 + t] = (int)(carry + s_pre[t] - v);
    __syncthreads();
    if (t == 1023) s_carry = carry + s_pre[1023];
    __syncthreads();
  }
  if (t == 0) totals[blockIdx.x] = s_carry;
}

// ------------------------------------------------------------------------- 3D ----
struct Surf3 {
  int n0, n1, n2;        // the array
  int e0, e1, e2;        // the lattice: the array, plus one virtual layer a side when closed
  int ext;               // 0 / 1
  int nodes;             // e0 * e1 * e2
  double level, outside;
  double org[3], sp[3];
};

// corner / offset code: x = 4, y = 2, z = 1.  Slot order of the contract: (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1)
// (1,1,1) = codes 4 2 1 6 5 3 7; slot_of(code) is the inverse, one nibble a code
__device__ __forceinline__ int slot_of3(int code) { return (0x63405120u >> (4 * code)) & 7; }
__device__ __forceinline__ int code_of3(int slot) { return (0x7356124u >> (4 * slot)) & 7; }

template <typename T>
__device__ __forceinline__ double sample3(const Surf3& s, const T* __restrict__ phi, int i, int j, int k) {
  const int a = i - s.ext, b = j - s.ext, c = k - s.ext;
  if ((unsigned)a < (unsigned)s.n0 && (unsigned)b < (unsigned)s.n1 && (unsigned)c < (unsigned)s.n2)
    return (double)phi[(a * s.n1 + b) * s.n2 + c];
  return s.outside;
}

__device__ __forceinline__ void split3(const Surf3& s, int g, int& i, int& j, int& k) {
  const unsigned q = (unsigned)g / (unsigned)s.e2;
  k = g - (int)q * s.e2;
  i = (int)(q / (unsigned)s.e1);
  j = (int)q - i * s.e1;
}

// which of +x, +y, +z steps stay inside the lattice (code bits)
__device__ __forceinline__ int exist3(const Surf3& s, int i, int j, int k) {
  return (i + 1 < s.e0 ? 4 : 0) | (j + 1 < s.e1 ? 2 : 0) | (k + 1 < s.e2 ? 1 : 0);
}

// the node's owned edges whose ends differ: bit = slot
__device__ __forceinline__ int edge_mask3(int cb, int exm) {
  const int in0 = cb & 1;
  int m = 0;
#pragma unroll
  for (int sl = 0; sl < 7; ++sl) {
    const int code = code_of3(sl);
    if ((code & ~exm) == 0 && ((cb >> code) & 1) != in0) m |= 1 << sl;
  }
  return m;
}

// the six Kuhn tetrahedra: chain 0, a, a|b, 7 for the ordered axis pairs (a, b); NEG: the permutation is odd
__device__ __forceinline__ void tet3(int t, int& a, int& ab, bool& neg) {
  // (x,y,z)+ (x,z,y)- (y,x,z)- (y,z,x)+ (z,x,y)+ (z,y,x)-
  const int A = (0x112244 >> (4 * t)) & 7;        // t = 0..5 -> 4 4 2 2 1 1
  const int B = (0x241412 >> (4 * t)) & 7;        //            2 1 4 1 4 2
  a = A; ab = A | B;
  neg = (0x26 >> t) & 1;                          // t = 1, 2, 5
}

__device__ __forceinline__ int tet_inside(int cb, int a, int ab) {
  return (cb & 1) | (((cb >> a) & 1) << 1) | (((cb >> ab) & 1) << 2) | (((cb >> 7) & 1) << 3);
}

__device__ __forceinline__ int tri_count3(int cb) {
  int n = 0;
#pragma unroll
  for (int t = 0; t < 6; ++t) {
    int a, ab; bool neg;
    tet3(t, a, ab, neg);
    const int p = __popc(tet_inside(cb, a, ab));
    n += p == 2 ? 2 : (p & 1);
  }
  return n;
}

template <typename T>
__global__ void __launch_bounds__(kSurfBlock)
k_surf3_count(Surf3 s, const T* __restrict__ phi, unsigned char* __restrict__ cbits, int* __restrict__ bsum_v,
              int* __restrict__ bsum_f) {
  int nv = 0, nf = 0;
#pragma unroll 1
  for (int r = 0; r < kSurfPer; ++r) {
    const int g = blockIdx.x * kSurfTile + r * kSurfBlock + (int)threadIdx.x;
    if (g < s.nodes) {
      int i, j, k;
      split3(s, g, i, j, k);
      const int exm = exist3(s, i, j, k);
      int cb = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c)
        if ((c & ~exm) == 0 && sample3(s, phi, i + (c >> 2), j + ((c >> 1) & 1), k + (c & 1)) < s.level) cb |= 1 << c;
      cbits[g] = (unsigned char)cb;
      nv += __popc(edge_mask3(cb, exm));
      if (exm == 7 && cb != 0 && cb != 255) nf += tri_count3(cb);
    }
  }
  block_sum2(nv, nf);
  if (threadIdx.x == 0) { bsum_v[blockIdx.x] = nv; bsum_f[blockIdx.x] = nf; }
}

// node gradient: central differences where both neighbours are in the lattice, one-sided at its border
template <typename T>
__device__ __forceinline__ void grad3(const Surf3& s, const T* __restrict__ phi, int i, int j, int k, double g[3]) {
  const int p[3] = {i, j, k}, e[3] = {s.e0, s.e1, s.e2};
  const double c = sample3(s, phi, i, j, k);
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const bool lo = p[d] > 0, hi = p[d] + 1 < e[d];
    const double vl = lo ? sample3(s, phi, i - (d == 0), j - (d == 1), k - (d == 2)) : c;
    const double vh = hi ? sample3(s, phi, i + (d == 0), j + (d == 1), k + (d == 2)) : c;
    const int w = (int)lo + (int)hi;
    g[d] = w ? (vh - vl) / ((double)w * s.sp[d]) : 0.0;
  }
}

template <typename T, bool NORMALS>
__global__ void __launch_bounds__(kSurfBlock)
k_surf3_verts(Surf3 s, const T* __restrict__ phi, const unsigned char* __restrict__ cbits, const int* __restrict__ bsum_v,
              int* __restrict__ first, float* __restrict__ verts, float* __restrict__ normals, int cap_v) {
  int run = bsum_v[blockIdx.x];
#pragma unroll 1
  for (int r = 0; r < kSurfPer; ++r) {
    const int g = blockIdx.x * kSurfTile + r * kSurfBlock + (int)threadIdx.x;
    int i = 0, j = 0, k = 0, em = 0;
    if (g < s.nodes) {
      split3(s, g, i, j, k);
      em = edge_mask3(cbits[g], exist3(s, i, j, k));
    }
    int total;
    int idx = run + block_excl_scan(__popc(em), total);
    run += total;
    if (g < s.nodes) first[g] = idx;
    if (em == 0) continue;
    const double pa = sample3(s, phi, i, j, k);
    double ga[3];
    if (NORMALS) grad3(s, phi, i, j, k, ga);
    const int p[3] = {i - s.ext, j - s.ext, k - s.ext};
    for (int sl = 0; sl < 7; ++sl) {
      if (!((em >> sl) & 1)) continue;
      const int code = code_of3(sl);
      const int d[3] = {code >> 2, (code >> 1) & 1, code & 1};
      const double pb = sample3(s, phi, i + d[0], j + d[1], k + d[2]);
      const double t = (s.level - pa) / (pb - pa);
      if (idx < cap_v) {
#pragma unroll
        for (int c = 0; c < 3; ++c) verts[(size_t)3 * idx + c] = (float)(s.org[c] + ((double)p[c] + t * (double)d[c]) * s.sp[c]);
        if (NORMALS) {
          double gb[3], n[3];
          grad3(s, phi, i + d[0], j + d[1], k + d[2], gb);
#pragma unroll
          for (int c = 0; c < 3; ++c) n[c] = (1.0 - t) * ga[c] + t * gb[c];
          const double len = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
#pragma unroll
          for (int c = 0; c < 3; ++c) normals[(size_t)3 * idx + c] = (float)(len > 0.0 ? n[c] / len : 0.0);
        }
      }
      ++idx;
    }
  }
}

__global__ void __launch_bounds__(kSurfBlock)
k_surf3_faces(Surf3 s, const unsigned char* __restrict__ cbits, const int* __restrict__ bsum_f, const int* __restrict__ first,
              int* __restrict__ faces, int cap_f) {
  int run = bsum_f[blockIdx.x];
  const int st0 = s.e1 * s.e2, st1 = s.e2;
#pragma unroll 1
  for (int r = 0; r < kSurfPer; ++r) {
    const int g = blockIdx.x * kSurfTile + r * kSurfBlock + (int)threadIdx.x;
    int i = 0, j = 0, k = 0, cb = 0, nf = 0;
    if (g < s.nodes) {
      split3(s, g, i, j, k);
      cb = cbits[g];
      if (exist3(s, i, j, k) == 7 && cb != 0 && cb != 255) nf = tri_count3(cb);
    }
    int total;
    int f = run + block_excl_scan(nf, total);
    run += total;
    if (nf == 0) continue;
    // vertex on the cube edge between corners ca and cc (ca a subset of cc): owner ca, slot of cc ^ ca
    auto vid = [&](int ca, int cc) {
      const int di = ca >> 2, dj = (ca >> 1) & 1, dk = ca & 1;
      const int o = g + di * st0 + dj * st1 + dk;
      const int em = edge_mask3(cbits[o], exist3(s, i + di, j + dj, k + dk));
      const int sl = slot_of3(cc ^ ca);
      return first[o] + __popc(em & ((1 << sl) - 1));
    };
    auto emit = [&](int a, int b, int c, bool flip) {
      if (f < cap_f) { faces[3 * f] = a; faces[3 * f + 1] = flip ? c : b; faces[3 * f + 2] = flip ? b : c; }
      ++f;
    };
    for (int t = 0; t < 6; ++t) {
      int a, ab; bool neg;
      tet3(t, a, ab, neg);
      const int ch[4] = {0, a, ab, 7};
      const int m = tet_inside(cb, a, ab);
      const int n = __popc(m);
      if (n == 0 || n == 4) continue;
      if (n == 2) {
        // inside pair A < B, outside pair C < D; cycle AC AD BD BC, split by AC-BD.  As written it is outward for the even
        // arrangements (A,B,C,D) of an even tetrahedron; {0,2} and {1,3} inside are the odd ones
        const int A = __ffs(m) - 1, B = 31 - __clz(m), om = ~m & 15, Cc = __ffs(om) - 1, D = 31 - __clz(om);
        const bool flip = (m == 5 || m == 10) != neg;
        auto e = [&](int u, int v) { return u < v ? vid(ch[u], ch[v]) : vid(ch[v], ch[u]); };
        const int ac = e(A, Cc), ad = e(A, D), bd = e(B, D), bc = e(B, Cc);
        emit(ac, ad, bd, flip);
        emit(ac, bd, bc, flip);
      } else {
        // the lone vertex i and the others j < k < l: (ij, ik, il) points away from i in an even tetrahedron when i is
        // even; a lone OUTSIDE vertex (three inside) wants the normal towards it
        const int lone = n == 1 ? m : (~m & 15);
        const int iv = __ffs(lone) - 1;
        int o[3], c = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) if (q != iv) o[c++] = q;
        const bool flip = ((iv & 1) != 0) != neg != (n == 3);
        auto e = [&](int v) { return iv < v ? vid(ch[iv], ch[v]) : vid(ch[v], ch[iv]); };
        emit(e(o[0]), e(o[1]), e(o[2]), flip);
      }
    }
  }
}

// ------------------------------------------------------------------------- 2D ----
struct Surf2 {
  int n0, n1, e0, e1, ext, nodes;
  double level, outside;
  double org[2], sp[2];
};

// corner / offset code: x = 2, y = 1; slots (1,0) (0,1) (1,1) = codes 2 1 3
__device__ __forceinline__ int slot_of2(int code) { return code == 2 ? 0 : (code == 1 ? 1 : 2); }
__device__ __forceinline__ int code_of2(int slot) { return slot == 0 ? 2 : (slot == 1 ? 1 : 3); }

template <typename T>
__device__ __forceinline__ double sample2(const Surf2& s, const T* __restrict__ phi, int i, int j) {
  const int a = i - s.ext, b = j - s.ext;
  if ((unsigned)a < (unsigned)s.n0 && (unsigned)b < (unsigned)s.n1) return (double)phi[a * s.n1 + b];
  return s.outside;
}
__device__ __forceinline__ int exist2(const Surf2& s, int i, int j) { return (i + 1 < s.e0 ? 2 : 0) | (j + 1 < s.e1 ? 1 : 0); }
__device__ __forceinline__ int edge_mask2(int cb, int exm) {
  const int in0 = cb & 1;
  int m = 0;
#pragma unroll
  for (int sl = 0; sl < 3; ++sl) {
    const int code = code_of2(sl);
    if ((code & ~exm) == 0 && ((cb >> code) & 1) != in0) m |= 1 << sl;
  }
  return m;
}
// the two triangles of a square: chain 0, a, 3 with a = 2 (counter-clockwise) and a = 1 (clockwise)
__device__ __forceinline__ int tri_inside(int cb, int a) { return (cb & 1) | (((cb >> a) & 1) << 1) | (((cb >> 3) & 1) << 2); }
__device__ __forceinline__ int seg_count2(int cb) {
  const int m0 = tri_inside(cb, 2), m1 = tri_inside(cb, 1);
  return (int)(m0 != 0 && m0 != 7) + (int)(m1 != 0 && m1 != 7);
}

template <typename T>
__global__ void __launch_bounds__(kSurfBlock)
k_cont2_count(Surf2 s, const T* __restrict__ phi, unsigned char* __restrict__ cbits, int* __restrict__ bsum_v,
              int* __restrict__ bsum_f) {
  int nv = 0, nf = 0;
#pragma unroll 1
  for (int r = 0; r < kSurfPer; ++r) {
    const int g = blockIdx.x * kSurfTile + r * kSurfBlock + (int)threadIdx.x;
    if (g < s.nodes) {
      const int i = (int)((unsigned)g / (unsigned)s.e1), j = g - i * s.e1;
      const int exm = exist2(s, i, j);
      int cb = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if ((c & ~exm) == 0 && sample2(s, phi, i + (c >> 1), j + (c & 1)) < s.level) cb |= 1 << c;
      cbits[g] = (unsigned char)cb;
      nv += __popc(edge_mask2(cb, exm));
      if (exm == 3) nf += seg_count2(cb);
    }
  }
  block_sum2(nv, nf);
  if (threadIdx.x == 0) { bsum_v[blockIdx.x] = nv; bsum_f[blockIdx.x] = nf; }
}

template <typename T>
__global__ void __launch_bounds__(kSurfBlock)
k_cont2_verts(Surf2 s, const T* __restrict__ phi, const unsigned char* __restrict__ cbits, const int* __restrict__ bsum_v,
              int* __restrict__ first, float* __restrict__ verts, int cap_v) {
  int run = bsum_v[blockIdx.x];
#pragma unroll 1
  for (int r = 0; r < kSurfPer; ++r) {
    const int g = blockIdx.x * kSurfTile + r * kSurfBlock + (int)threadIdx.x;
    int i = 0, j = 0, em = 0;
    if (g < s.nodes) {
      i = (int)((unsigned)g / (unsigned)s.e1);
      j = g - i * s.e1;
      em = edge_mask2(cbits[g], exist2(s, i, j));
    }
    int total;
    int idx = run + block_excl_scan(__popc(em), total);
    run += total;
    if (g < s.nodes) first[g] = idx;
    if (em == 0) continue;
    const double pa = sample2(s, phi, i, j);
    const int p[2] = {i - s.ext, j - s.ext};
    for (int sl = 0; sl < 3; ++sl) {
      if (!((em >> sl) & 1)) continue;
      const int code = code_of2(sl);
      const int d[2] = {code >> 1, code & 1};
      const double pb = sample2(s, phi, i + d[0], j + d[1]);
      const double t = (s.level - pa) / (pb - pa);
      if (idx < cap_v) {
#pragma unroll
        for (int c = 0; c < 2; ++c) verts[(size_t)2 * idx + c] = (float)(s.org[c] + ((double)p[c] + t * (double)d[c]) * s.sp[c]);
      }
      ++idx;
    }
  }
}

__global__ void __launch_bounds__(kSurfBlock)
k_cont2_segs(Surf2 s, const unsigned char* __restrict__ cbits, const int* __restrict__ bsum_f, const int* __restrict__ first,
             int* __restrict__ segs, int cap_f) {
  int run = bsum_f[blockIdx.x];
#pragma unroll 1
  for (int r = 0; r < kSurfPer; ++r) {
    const int g = blockIdx.x * kSurfTile + r * kSurfBlock + (int)threadIdx.x;
    int i = 0, j = 0, cb = 0, nf = 0;
    if (g < s.nodes) {
      i = (int)((unsigned)g / (unsigned)s.e1);
      j = g - i * s.e1;
      cb = cbits[g];
      if (exist2(s, i, j) == 3) nf = seg_count2(cb);
    }
    int total;
    int f = run + block_excl_scan(nf, total);
    run += total;
    if (nf == 0) continue;
    auto vid = [&](int ca, int cc) {
      const int di = ca >> 1, dj = ca & 1;
      const int o = g + di * s.e1 + dj;
      const int em = edge_mask2(cbits[o], exist2(s, i + di, j + dj));
      return first[o] + __popc(em & ((1 << slot_of2(cc ^ ca)) - 1));
    };
    for (int t = 0; t < 2; ++t) {
      const int a = t == 0 ? 2 : 1;
      const bool neg = t == 1;
      const int ch[3] = {0, a, 3};
      const int m = tri_inside(cb, a);
      if (m == 0 || m == 7) continue;
      const int n = __popc(m);
      // the lone vertex i, the others j < k: (ij -> ik) keeps i on its left in a counter-clockwise triangle unless i = 1
      const int iv = __ffs(n == 1 ? m : (~m & 7)) - 1;
      const int oj = iv == 0 ? 1 : 0, ok = iv == 2 ? 1 : 2;
      const bool flip = (iv == 1) != neg != (n == 2);
      auto e = [&](int v) { return iv < v ? vid(ch[iv], ch[v]) : vid(ch[v], ch[iv]); };
      const int u = e(oj), v = e(ok);
      if (f < cap_f) { segs[2 * f] = flip ? v : u; segs[2 * f + 1] = flip ? u : v; }
      ++f;
    }
  }
}

// ------------------------------------------------------------------- host side ----
struct SurfWs {
  long long* totals;      // [0] vertices, [1] faces / segments
  int *bsum_v, *bsum_f, *first;
  unsigned char* cbits;
  int nb;
  size_t bytes;
};

// lattice extents -> node count, or -1 when it does not fit int32
int64_t lattice_nodes(const int64_t* shape, int dim, int closed) {
  if (shape == nullptr) return -1;
  int64_t n = 1;
  for (int d = 0; d < dim; ++d) {
    if (shape[d] < 2 || shape[d] > INT32_MAX - 2) return -1;
    const int64_t e = shape[d] + (closed ? 2 : 0);
    if (n > INT32_MAX / e) return -1;
    n *= e;
  }
  if (n > INT32_MAX - kSurfTile) return -1;      // the last tile's node indices stay below 2^31
  return n;
}

SurfWs carve(void* ws, int64_t nodes) {
  SurfWs w;
  w.nb = (int)((nodes + kSurfTile - 1) / kSurfTile);
  char* p = (char*)ws;
  size_t off = 0;
  auto take = [&](size_t b) { char* q = p ? p + off : nullptr; off += align_up(b, 256); return q; };
  w.totals = (long long*)take(2 * sizeof(long long));
  w.bsum_v = (int*)take((size_t)w.nb * sizeof(int));
  w.bsum_f = (int*)take((size_t)w.nb * sizeof(int));
  w.first = (int*)take((size_t)nodes * sizeof(int));
  w.cbits = (unsigned char*)take((size_t)nodes);
  w.bytes = off;
  return w;
}

int check_common(const int64_t* shape, int dim, const void* phi, int phi_dt, double level, int closed, double outside,
                 void* workspace, size_t workspace_bytes, int64_t& nodes) {
  nodes = lattice_nodes(shape, dim, closed);
  MFS_REQUIRE(nodes > 0, "shape: every extent >= 2 and the lattice at most 2^31 - 1025 nodes");
  MFS_REQUIRE(phi != nullptr && workspace != nullptr, "phi or workspace is null");
  MFS_REQUIRE(dtype_ok(phi_dt), "bad phi dtype");
  MFS_REQUIRE(level == level && level - level == 0.0, "level must be finite");
  MFS_REQUIRE(!closed || outside > level, "closed needs outside > level");
  MFS_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  MFS_REQUIRE(workspace_bytes >= carve(nullptr, nodes).bytes, "workspace too small");
  return MFS_OK;
}

// the totals the count pass left, checked against the caller's capacities (one 16-byte copy; the stream is drained)
int read_totals(const SurfWs& w, int64_t cap_v, int64_t cap_f, long long tot[2], hipStream_t st) {
  MFS_HIP_TRY(hipMemcpyAsync(tot, w.totals, 2 * sizeof(long long), hipMemcpyDeviceToHost, st));
  MFS_HIP_TRY(hipStreamSynchronize(st));
  MFS_REQUIRE(tot[0] >= 0 && tot[1] >= 0 && tot[0] <= INT32_MAX && tot[1] <= INT32_MAX / 3, "vertex or index count does not fit int32");
  MFS_REQUIRE(cap_v >= tot[0] && cap_f >= tot[1], "capacities are smaller than the counted totals");
  return MFS_OK;
}

}  // namespace
}  // namespace mfs

using namespace mfs;

extern "C" {

size_t mfs_surface3d_workspace_bytes(const int64_t shape[3], int closed) {
  const int64_t nodes = lattice_nodes(shape, 3, closed);
  return nodes > 0 ? carve(nullptr, nodes).bytes : 0;
}

static Surf3 make3(const int64_t shape[3], double level, int closed, double outside, int64_t nodes) {
  Surf3 s;
  s.n0 = (int)shape[0]; s.n1 = (int)shape[1]; s.n2 = (int)shape[2];
  s.ext = closed ? 1 : 0;
  s.e0 = s.n0 + 2 * s.ext; s.e1 = s.n1 + 2 * s.ext; s.e2 = s.n2 + 2 * s.ext;
  s.nodes = (int)nodes;
  s.level = level;
  s.outside = closed ? outside : 0.0;
  for (int c = 0; c < 3; ++c) { s.org[c] = 0.0; s.sp[c] = 1.0; }
  return s;
}

int mfs_surface3d_count(const int64_t shape[3], const void* phi, int phi_dt, double level, int closed, double outside,
                        void* workspace, size_t workspace_bytes, mfs_stream stream) {
  int64_t nodes;
  if (int rc = check_common(shape, 3, phi, phi_dt, level, closed, outside, workspace, workspace_bytes, nodes)) return rc;
  const SurfWs w = carve(workspace, nodes);
  const Surf3 s = make3(shape, level, closed, outside, nodes);
  hipStream_t st = (hipStream_t)stream;
  if (phi_dt == MFS_F32)
    hipLaunchKernelGGL(k_surf3_count<float>, dim3(w.nb), dim3(kSurfBlock), 0, st, s, (const float*)phi, w.cbits, w.bsum_v, w.bsum_f);
  else
    hipLaunchKernelGGL(k_surf3_count<double>, dim3(w.nb), dim3(kSurfBlock), 0, st, s, (const double*)phi, w.cbits, w.bsum_v, w.bsum_f);
  hipLaunchKernelGGL(k_surf_scan, dim3(2), dim3(1024), 0, st, w.bsum_v, w.bsum_f, w.nb, w.totals);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_surface3d_fill(const int64_t shape[3], const void* phi, int phi_dt, double level, int closed, double outside,
                       const double origin[3], const double spacing[3], void* workspace, size_t workspace_bytes,
                       void* vertices, int64_t cap_vertices, void* faces, int64_t cap_faces, void* normals,
                       mfs_stream stream) {
  int64_t nodes;
  if (int rc = check_common(shape, 3, phi, phi_dt, level, closed, outside, workspace, workspace_bytes, nodes)) return rc;
  MFS_REQUIRE(origin != nullptr && spacing != nullptr, "origin or spacing is null");
  MFS_REQUIRE(spacing[0] > 0 && spacing[1] > 0 && spacing[2] > 0, "spacing must be positive");
  MFS_REQUIRE(cap_vertices >= 0 && cap_faces >= 0 && cap_vertices <= INT32_MAX && cap_faces <= INT32_MAX / 3, "capacity out of range");
  const SurfWs w = carve(workspace, nodes);
  hipStream_t st = (hipStream_t)stream;
  long long tot[2];
  if (int rc = read_totals(w, cap_vertices, cap_faces, tot, st)) return rc;
  if (tot[0] == 0 && tot[1] == 0) return MFS_OK;
  MFS_REQUIRE(vertices != nullptr && (faces != nullptr || tot[1] == 0), "vertices or faces is null");
  Surf3 s = make3(shape, level, closed, outside, nodes);
  for (int c = 0; c < 3; ++c) { s.org[c] = origin[c]; s.sp[c] = spacing[c]; }
  const int cv = (int)cap_vertices, cf = (int)cap_faces;
  float *v = (float*)vertices, *nr = (float*)normals;
  const dim3 grid(w.nb), block(kSurfBlock);
  if (phi_dt == MFS_F32) {
    if (nr) hipLaunchKernelGGL((k_surf3_verts<float, true>), grid, block, 0, st, s, (const float*)phi, w.cbits, w.bsum_v, w.first, v, nr, cv);
    else hipLaunchKernelGGL((k_surf3_verts<float, false>), grid, block, 0, st, s, (const float*)phi, w.cbits, w.bsum_v, w.first, v, nr, cv);
  } else {
    if (nr) hipLaunchKernelGGL((k_surf3_verts<double, true>), grid, block, 0, st, s, (const double*)phi, w.cbits, w.bsum_v, w.first, v, nr, cv);
    else hipLaunchKernelGGL((k_surf3_verts<double, false>), grid, block, 0, st, s, (const double*)phi, w.cbits, w.bsum_v, w.first, v, nr, cv);
  }
  if (tot[1] > 0) hipLaunchKernelGGL(k_surf3_faces, grid, block, 0, st, s, w.cbits, w.bsum_f, w.first, (int*)faces, cf);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

size_t mfs_contour2d_workspace_bytes(const int64_t shape[2], int closed) {
  const int64_t nodes = lattice_nodes(shape, 2, closed);
  return nodes > 0 ? carve(nullptr, nodes).bytes : 0;
}

static Surf2 make2(const int64_t shape[2], double level, int closed, double outside, int64_t nodes) {
  Surf2 s;
  s.n0 = (int)shape[0]; s.n1 = (int)shape[1];
  s.ext = closed ? 1 : 0;
  s.e0 = s.n0 + 2 * s.ext; s.e1 = s.n1 + 2 * s.ext;
  s.nodes = (int)nodes;
  s.level = level;
  s.outside = closed ? outside : 0.0;
  for (int c = 0; c < 2; ++c) { s.org[c] = 0.0; s.sp[c] = 1.0; }
  return s;
}

int mfs_contour2d_count(const int64_t shape[2], const void* phi, int phi_dt, double level, int closed, double outside,
                        void* workspace, size_t workspace_bytes, mfs_stream stream) {
  int64_t nodes;
  if (int rc = check_common(shape, 2, phi, phi_dt, level, closed, outside, workspace, workspace_bytes, nodes)) return rc;
  const SurfWs w = carve(workspace, nodes);
  const Surf2 s = make2(shape, level, closed, outside, nodes);
  hipStream_t st = (hipStream_t)stream;
  if (phi_dt == MFS_F32)
    hipLaunchKernelGGL(k_cont2_count<float>, dim3(w.nb), dim3(kSurfBlock), 0, st, s, (const float*)phi, w.cbits, w.bsum_v, w.bsum_f);
  else
    hipLaunchKernelGGL(k_cont2_count<double>, dim3(w.nb), dim3(kSurfBlock), 0, st, s, (const double*)phi, w.cbits, w.bsum_v, w.bsum_f);
  hipLaunchKernelGGL(k_surf_scan, dim3(2), dim3(1024), 0, st, w.bsum_v, w.bsum_f, w.nb, w.totals);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_contour2d_fill(const int64_t shape[2], const void* phi, int phi_dt, double level, int closed, double outside,
                       const double origin[2], const double spacing[2], void* workspace, size_t workspace_bytes,
                       void* vertices, int64_t cap_vertices, void* segments, int64_t cap_segments, mfs_stream stream) {
  int64_t nodes;
  if (int rc = check_common(shape, 2, phi, phi_dt, level, closed, outside, workspace, workspace_bytes, nodes)) return rc;
  MFS_REQUIRE(origin != nullptr && spacing != nullptr, "origin or spacing is null");
  MFS_REQUIRE(spacing[0] > 0 && spacing[1] > 0, "spacing must be positive");
  MFS_REQUIRE(cap_vertices >= 0 && cap_segments >= 0 && cap_vertices <= INT32_MAX && cap_segments <= INT32_MAX / 2, "capacity out of range");
  const SurfWs w = carve(workspace, nodes);
  hipStream_t st = (hipStream_t)stream;
  long long tot[2];
  if (int rc = read_totals(w, cap_vertices, cap_segments, tot, st)) return rc;
  if (tot[0] == 0 && tot[1] == 0) return MFS_OK;
  MFS_REQUIRE(vertices != nullptr && (segments != nullptr || tot[1] == 0), "vertices or segments is null");
  Surf2 s = make2(shape, level, closed, outside, nodes);
  for (int c = 0; c < 2; ++c) { s.org[c] = origin[c]; s.sp[c] = spacing[c]; }
  const dim3 grid(w.nb), block(kSurfBlock);
  if (phi_dt == MFS_F32)
    hipLaunchKernelGGL(k_cont2_verts<float>, grid, block, 0, st, s, (const float*)phi, w.cbits, w.bsum_v, w.first, (float*)vertices, (int)cap_vertices);
  else
    hipLaunchKernelGGL(k_cont2_verts<double>, grid, block, 0, st, s, (const double*)phi, w.cbits, w.bsum_v, w.first, (float*)vertices, (int)cap_vertices);
  if (tot[1] > 0) hipLaunchKernelGGL(k_cont2_segs, grid, block, 0, st, s, w.cbits, w.bsum_f, w.first, (int*)segments, (int)cap_segments);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
