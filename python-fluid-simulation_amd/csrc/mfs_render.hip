// mfs_render.hip -- ray-marched images of level-set volumes on gfx950 (no reference counterpart):
//   k_render_bricks  one workgroup per brick of 8 x 8 x 8 cells (9^3 nodes, clipped at the volume's end): its minimum,
//                    -inf when it holds a NaN (or its maximum, +inf); wave reduction, no atomics
//   k_render_march   one lane per pixel, one wave per 8 x 8 pixel tile: walks the samples t_k = near + k * step of its ray,
//                    stops at the first with min over the shapes < 0, refines by one secant step, takes the normal
//   k_render_shade   Lambert from the normals and shape ids, one lane per pixel
//   k_render_shade_albedo  the same with a per-pixel albedo for one shape (the liquid coloured by particle data)
//   k_render_paths   one lane per sub-pixel ray: up to four such marches in a loop over the path's state -- the camera's
//                    ray, inside a refracting liquid, after the exit, the shadow ray -- and the path's colour
//   k_render_resolve the box filter of the sub-pixel colours and the byte conversion
// Every shape is a sampled signed field under a rigid pose, as in mfs_seed.hip; the arithmetic on the ray is float64 with
// contraction off and is restated in numpy operation by operation (tests/render_numpy.py, tests/render_paths_numpy.py).
#include <math.h>

#include "mfs_common.h"
#include "mfs_volume.h"

namespace mfs {

constexpr int kRenderBlock = 256;          // threads per workgroup: four waves, each an 8 x 8 pixel tile of a 16 x 16 block
constexpr int kRenderTile = 16;            // pixels per workgroup edge
constexpr int kBrick = 8;                  // cells per brick edge
constexpr int kBrickNodes = (kBrick + 1) * (kBrick + 1) * (kBrick + 1);
// Node units by which a box is widened and a brick narrowed before a skip is computed from it.  The skips work on the line
// u0 + t du in a shape's node coordinates, the samples on x_k = o + t_k d taken to the body frame: the two differ by a few
// roundings of coordinates below 2^40 nodes, far less than this.
constexpr double kSkipMargin = 1e-3;

struct RenderCamera {
  double eye[3], f[3], r[3], u[3];
  double half_w, half_h;
  double near, step;
  int ortho, W, H, K;
};

struct RenderBricks {                      // by value in the launch, alongside the shapes' Volumes and Poses
  const double* brick[kMaxVolumes];        // minima per brick; null without skips
  int nb[kMaxVolumes][3];                  // bricks along each axis: ceil((n - 1) / 8)
};
static_assert(sizeof(RenderBricks) == kMaxVolumes * (8 + 12), "RenderBricks: the fields, unpadded");

struct RenderPalette {
  double albedo[kMaxVolumes][3];
  double light[3];
  int background[3];
  int n, has_light;
};

#pragma clang fp contract(off)

// shape i at the world point x: its volume sampled at R^T (x - T) (mfs_volume.h); inside and cell as volume_sample's
__device__ __forceinline__ double render_sample(const Volumes& V, const Poses& P, int i, const double x[3], bool* inside,
                                                int cell[3]) {
  double xb[3];
  pose_to_body(P.R[i], P.T[i], x, xb);
  return volume_sample(V, i, xb, inside, cell, nullptr);
}

// the render rule: a shape shows inside its own box only
__device__ __forceinline__ double render_value(const Volumes& V, const Poses& P, int i, const double x[3]) {
  bool inside;
  int cell[3];
  const double v = render_sample(V, P, i, x, &inside, cell);
  return inside ? v : INFINITY;
}

// F(x) = min over the shapes, taken with a strict < from +inf: the first shape that attains it; a NaN is passed over
__device__ __forceinline__ double render_scene(const Volumes& V, const Poses& P, int n, const double x[3]) {
  double best = INFINITY;
  for (int i = 0; i < n; ++i) {
    const double v = render_value(V, P, i, x);
    if (v < best) best = v;
  }
  return best;
}

// pixel (i, j), row i from the top -> origin and unit direction of its ray
__device__ __forceinline__ void render_ray(const RenderCamera& C, int i, int j, double o[3], double d[3]) {
  const double sx = (((double)j + 0.5) * (2.0 / (double)C.W) - 1.0) * C.half_w;
  const double sy = (1.0 - ((double)i + 0.5) * (2.0 / (double)C.H)) * C.half_h;
  if (C.ortho) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = (C.eye[a] + sx * C.r[a]) + sy * C.u[a];
      d[a] = C.f[a];
    }
  } else {
    double v[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = C.eye[a];
      v[a] = (C.f[a] + sx * C.r[a]) + sy * C.u[a];
    }
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = v[a] / len;
  }
}

// ---- the skips.  Nothing below enters a result: it only decides which samples of which shape are not evaluated, and every
// decision errs towards evaluating (DESIGN.md 4.16 has the argument).

// the ray in shape i's node coordinates: u(t) = u0 + t du
__device__ __forceinline__ void render_ray_nodes(const Volumes& V, const Poses& P, int i, const double o[3],
                                                 const double d[3], double u0[3], double du[3]) {
  const double e[3] = {o[0] - P.T[i][0], o[1] - P.T[i][1], o[2] - P.T[i][2]};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    u0[k] = (((P.R[i][0][k] * e[0] + P.R[i][1][k] * e[1]) + P.R[i][2][k] * e[2]) - V.org[i][k]) / V.h[i];
    du[k] = ((P.R[i][0][k] * d[0] + P.R[i][1][k] * d[1]) + P.R[i][2][k] * d[2]) / V.h[i];
  }
}

// the parameter interval [tin, tout] over which the line lies in the box [lo, hi]; false if it is empty
__device__ __forceinline__ bool render_slab(const double u0[3], const double du[3], const double lo[3], const double hi[3],
                                            double* tin, double* tout) {
  double a = -INFINITY, b = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (du[k] == 0.0) {
      if (!(u0[k] >= lo[k] && u0[k] <= hi[k])) return false;
    } else {
      const double t1 = (lo[k] - u0[k]) / du[k], t2 = (hi[k] - u0[k]) / du[k];
      a = fmax(a, fmin(t1, t2));
      b = fmin(b, fmax(t1, t2));
    }
  }
  *tin = a;
  *tout = b;
  return a <= b;
}

// The samples of one march: t_k = t0 + k * step, k < K.  The camera's rays start at t0 = near, every later segment of a
// path at its own origin with t0 = 0.
struct RenderSeg {
  double t0, step;
  int K;
};

// floor((t - t0) / step) + shift as a sample index, held in [lo, K]
__device__ __forceinline__ int render_index(const RenderSeg& C, double t, double shift, int lo) {
  double q = floor((t - C.t0) / C.step) + shift;
  if (!(q > (double)lo)) return lo;                   // also a NaN
  if (q > (double)C.K) return C.K;
  return (int)q;
}

// The smallest sample index >= kmin of shape i that has to be evaluated, when all that is known is the shape's box: the
// samples before the ray enters the box widened by the margin are outside the box itself, and so are all of them if the
// ray misses the widened box or has left it before sample kmin.  One sample is given away at the entry.
__device__ __forceinline__ int render_next_outside(const RenderSeg& C, const Volumes& V, const Poses& P, int i,
                                                   const double o[3], const double d[3], int kmin) {
  double u0[3], du[3], lo[3], hi[3], tin, tout;
  render_ray_nodes(V, P, i, o, d, u0, du);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lo[k] = -kSkipMargin;
    hi[k] = (double)(V.n[i][k] - 1) + kSkipMargin;
  }
  if (!render_slab(u0, du, lo, hi, &tin, &tout)) return C.K;
  if (tout < C.t0 + (double)kmin * C.step) return C.K;
  return render_index(C, tin, -1.0, kmin);
}

// Sample k of shape i lies in the brick of `cell`, whose minimum is > 0: the samples up to the ray's exit from the brick
// narrowed by the margin fall into cells of that brick, where a trilinear sample, a combination of the cell's nodes with
// weights in [0, 1], cannot be negative.  (Inside the shape, where its value counts negated, the same holds of a brick
// whose maximum is < 0: the sample cannot be positive.)  Returns the first index after them (k + 1 if sample k itself is not in the
// narrowed brick); one sample is given away at the exit.
__device__ __forceinline__ int render_next_brick(const RenderSeg& C, const Volumes& V, const Poses& P, int i,
                                                 const double o[3], const double d[3], int k, const int cell[3]) {
  double u0[3], du[3], lo[3], hi[3], tin, tout;
  render_ray_nodes(V, P, i, o, d, u0, du);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int b = cell[a] / kBrick;
    const int end = min(kBrick * b + kBrick, V.n[i][a] - 1);
    lo[a] = (double)(kBrick * b) + kSkipMargin;
    hi[a] = (double)end - kSkipMargin;
  }
  if (!render_slab(u0, du, lo, hi, &tin, &tout)) return k + 1;
  if (!(tin <= C.t0 + (double)k * C.step)) return k + 1;
  return render_index(C, tout, 0.0, k + 1);
}

__global__ void __launch_bounds__(kRenderBlock)
k_render_march(RenderCamera C, Volumes V, Poses P, RenderBricks B, int n, int skip, double* __restrict__ depth,
               float* __restrict__ normal, int* __restrict__ shape_id, int* __restrict__ steps, int* __restrict__ evals) {
  // per lane and shape: the next sample index at which the shape has to be evaluated.  Each lane reads and writes its own
  // column only: no barrier.
  __shared__ int s_next[kMaxVolumes][kRenderBlock];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int j = (int)blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7);
  const int i = (int)blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
  if (i >= C.H || j >= C.W) return;
  double o[3], d[3];
  render_ray(C, i, j, o, d);
  const RenderSeg G = {C.near, C.step, C.K};

  int k = C.K;
  for (int s = 0; s < n; ++s) {
    const int nx = skip ? render_next_outside(G, V, P, s, o, d, 0) : 0;
    s_next[s][tid] = nx;
    k = min(k, nx);
  }
  int count = 0, id = -1;
  double b = INFINITY;
  bool hit = false;
  while (k < C.K) {                                   // k grows by at least 1 per pass: at most K passes
    const double t = C.near + (double)k * C.step;
    const double x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    double best = INFINITY;
    int arg = -1, knext = C.K;
    for (int s = 0; s < n; ++s) {
      int nx = s_next[s][tid];
      if (nx <= k) {
        bool inside;
        int cell[3];
        double v = render_sample(V, P, s, x, &inside, cell);
        ++count;
        nx = k + 1;
        if (!inside) {
          v = INFINITY;
          if (skip) nx = render_next_outside(G, V, P, s, o, d, k + 1);
        } else if (skip && !(v < 0.0)) {
          const int* nb = B.nb[s];
          const double m = B.brick[s][((int64_t)(cell[0] / kBrick) * nb[1] + cell[1] / kBrick) * nb[2] + cell[2] / kBrick];
          if (m > 0.0) nx = render_next_brick(G, V, P, s, o, d, k, cell);
        }
        s_next[s][tid] = nx;
        if (v < best) {
          best = v;
          arg = s;
        }
      }
      knext = min(knext, nx);
    }
    if (best < 0.0) {
      hit = true;
      b = best;
      id = arg;
      break;
    }
    k = knext;
  }

  const int64_t p = (int64_t)i * C.W + j;
  if (evals) evals[p] = count;
  if (!hit) {
    depth[p] = INFINITY;
    normal[3 * p] = normal[3 * p + 1] = normal[3 * p + 2] = 0.0f;
    shape_id[p] = -1;
    steps[p] = -1;
    return;
  }
  // the secant needs the true F(x_{k-1}): a skip may have passed over that sample, so it is evaluated here, in full
  const double tk = C.near + (double)k * C.step;
  double dep = tk;
  if (k > 0) {
    const double tp = C.near + (double)(k - 1) * C.step;
    const double xp[3] = {o[0] + tp * d[0], o[1] + tp * d[1], o[2] + tp * d[2]};
    const double a = render_scene(V, P, n, xp);
    if (a < INFINITY && a > -INFINITY) dep = (tk - C.step) + C.step * (a / (a - b));
  }
  const double xh[3] = {o[0] + dep * d[0], o[1] + dep * d[1], o[2] + dep * d[2]};
  const double hh = 0.5 * V.h[id];
  double g[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double xa[3] = {xh[0], xh[1], xh[2]}, xb[3] = {xh[0], xh[1], xh[2]};
    xa[a] = xh[a] + hh;
    xb[a] = xh[a] - hh;
    bool inside;
    int cell[3];
    const double va = render_sample(V, P, id, xa, &inside, cell);
    const double vb = render_sample(V, P, id, xb, &inside, cell);
    g[a] = va - vb;
  }
  const double len = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  const bool ok = len > 0.0 && len < INFINITY;
  depth[p] = dep;
#pragma unroll
  for (int a = 0; a < 3; ++a) normal[3 * p + a] = ok ? (float)(g[a] / len) : (float)(-d[a]);
  shape_id[p] = id;
  steps[p] = k;
}

// ---- paths: shadows, one refracting liquid interface pair, supersampling (tests/render_paths_numpy.py restates all of it)

struct RenderBrickPtrs {                   // the brick counts follow from the extents: (n - 2) / 8 + 1
  const double* lo[kMaxVolumes];           // minima per brick; null without skips
  const double* hi[kMaxVolumes];           // maxima per brick, of the liquid shapes only; null elsewhere
};

struct RenderLook {
  double albedo[kMaxVolumes][3];
  double absorb[kMaxVolumes][3];           // per world unit, of a liquid
  double ior[kMaxVolumes];                 // 0: opaque
  double light[3], background[3];
  double bias;
  int has_light, shadows, K_shadow, K_inside;
  unsigned opaque;                         // bit s: shape s is opaque
  int pad_;
};
static_assert(sizeof(RenderCamera) + sizeof(Volumes) + sizeof(Poses) + sizeof(RenderBrickPtrs) + sizeof(RenderLook) + 64 <= 4096,
              "k_render_paths: the launch arguments must fit the 4 KiB kernel argument segment");

// One lane per sub-pixel ray, one wave per 8 x 8 tile.  A path is at most four marches in fixed slots -- 0 primary, 1 inside
// the liquid, 2 after the exit, 3 the shadow ray of the surface finally shaded -- run by ONE march in a loop over the
// path's state (o, d, segment, medium, mask).  medium = m: shape m counts negated, -inf outside its box; a shape whose
// bit is clear in mask is never sampled.
__global__ void __launch_bounds__(kRenderBlock)
k_render_paths(RenderCamera C, Volumes V, Poses P, RenderBrickPtrs B, RenderLook L, int n, int skip,
               double* __restrict__ color, int* __restrict__ steps, int* __restrict__ shape_id, double* __restrict__ length,
               int* __restrict__ evals) {
  __shared__ int s_next[kMaxVolumes][kRenderBlock];   // as k_render_march's: each lane its own column, no barrier
  // The Fresnel term and the length inside the liquid wait here, not in registers, while the later marches run: with
  // them the kernel fits 256 VGPRs, two waves per SIMD as k_render_march.  Each lane its own column again.
  __shared__ double s_keep[2][kRenderBlock];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int j = (int)blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7);
  const int i = (int)blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3);
  if (i >= C.H || j >= C.W) return;
  s_keep[0][tid] = s_keep[1][tid] = 0.0;
  const int64_t p = (int64_t)i * C.W + j;
  double o[3], d[3];
  render_ray(C, i, j, o, d);
#pragma unroll
  for (int q = 0; q < 4; ++q) steps[4 * p + q] = shape_id[4 * p + q] = -2;

  int K = C.K;                                        // of the segment in hand
  unsigned mask = n >= 32 ? ~0u : (1u << n) - 1u;
  int medium = -1, slot = 0, liq = -1, sid = -1, count = 0;
  bool lit = true, own = false;                       // own: the liquid's own colour lies behind it, not the background
  double lam = 0.0;

  for (;;) {                                          // at most four passes: the slot only grows
    const RenderSeg G = {slot == 0 ? C.near : 0.0, C.step, K};
    int k = G.K;
    for (int s = 0; s < n; ++s) {
      int nx = G.K;
      if ((mask >> s) & 1u) nx = (skip && s != medium) ? render_next_outside(G, V, P, s, o, d, 0) : 0;
      s_next[s][tid] = nx;
      k = min(k, nx);
    }
    int id = -1;
    double b = INFINITY;
    bool hit = false;
    while (k < G.K) {                                 // k grows by at least 1 per pass: at most K passes
      const double t = G.t0 + (double)k * G.step;
      const double x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
      double best = INFINITY;
      int arg = -1, knext = G.K;
      for (int s = 0; s < n; ++s) {
        int nx = s_next[s][tid];
        if (nx <= k) {                                // never an excluded shape: its entry is K
          bool inside;
          int cell[3];
          double v = render_sample(V, P, s, x, &inside, cell);
          ++count;
          nx = k + 1;
          const int* e = V.n[s];
          const int64_t brick = ((int64_t)(cell[0] / kBrick) * ((e[1] - 2) / kBrick + 1) + cell[1] / kBrick) *
                                    ((e[2] - 2) / kBrick + 1) + cell[2] / kBrick;
          if (s == medium) {
            v = inside ? -v : -INFINITY;
            // all nodes < 0: every product of a weight in [0, 1] with a node is <= -0, so is their sum, and the negated
            // sample is >= +0 -- `v < 0` is false for either zero
            if (skip && inside && !(v < 0.0) && B.hi[s][brick] < 0.0) nx = render_next_brick(G, V, P, s, o, d, k, cell);
          } else if (!inside) {
            v = INFINITY;
            if (skip) nx = render_next_outside(G, V, P, s, o, d, k + 1);
          } else if (skip && !(v < 0.0)) {
            if (B.lo[s][brick] > 0.0) nx = render_next_brick(G, V, P, s, o, d, k, cell);
          }
          s_next[s][tid] = nx;
          if (v < best) {
            best = v;
            arg = s;
          }
        }
        knext = min(knext, nx);
      }
      if (best < 0.0) {
        hit = true;
        b = best;
        id = arg;
        break;
      }
      k = knext;
    }
    steps[4 * p + slot] = hit ? k : -1;
    shape_id[4 * p + slot] = hit ? id : -1;
    if (slot == 3) {
      if (hit) lit = false;
      break;
    }
    if (!hit) {                                       // slots 0 and 2: the background stays behind
      if (slot == 1) {
        s_keep[1][tid] = (double)G.K * G.step;
        own = true;
      }
      break;
    }
    // the secant needs the segment's true F(x_{k-1}): a skip may have passed over that sample
    const double tk = G.t0 + (double)k * G.step;
    double dep = tk;
    if (k > 0) {
      const double tp = G.t0 + (double)(k - 1) * G.step;
      const double xp[3] = {o[0] + tp * d[0], o[1] + tp * d[1], o[2] + tp * d[2]};
      double a = INFINITY;
      for (int s = 0; s < n; ++s) {
        if (!((mask >> s) & 1u)) continue;
        bool inside;
        int cell[3];
        double v = render_sample(V, P, s, xp, &inside, cell);
        if (s == medium) v = inside ? -v : -INFINITY;
        else if (!inside) v = INFINITY;
        if (v < a) a = v;
      }
      // leaving the medium's box is no crossing of a field: the hit stays at t_k
      if (a < INFINITY && a > -INFINITY && !(id == medium && !(b > -INFINITY))) dep = (tk - G.step) + G.step * (a / (a - b));
    }
    const double xh[3] = {o[0] + dep * d[0], o[1] + dep * d[1], o[2] + dep * d[2]};
    const double hh = 0.5 * V.h[id];
    double g[3], nn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      double xa[3] = {xh[0], xh[1], xh[2]}, xb[3] = {xh[0], xh[1], xh[2]};
      xa[a] = xh[a] + hh;
      xb[a] = xh[a] - hh;
      bool inside;
      int cell[3];
      const double va = render_sample(V, P, id, xa, &inside, cell);
      const double vb = render_sample(V, P, id, xb, &inside, cell);
      g[a] = va - vb;
    }
    const double gl = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
    const bool ok = gl > 0.0 && gl < INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a) nn[a] = ok ? g[a] / gl : -d[a];

    if ((slot == 0 && L.ior[id] > 0.0) || (slot == 1 && id == medium)) {   // an interface of the liquid: refract
      if (slot == 0) liq = id;
      else s_keep[1][tid] = dep;
      const double eta = slot == 0 ? 1.0 / L.ior[liq] : L.ior[liq];
      double dn = (d[0] * nn[0] + d[1] * nn[1]) + d[2] * nn[2];
      if (dn > 0.0) {                                 // the normal faces the arriving ray
        dn = -dn;
#pragma unroll
        for (int a = 0; a < 3; ++a) nn[a] = -nn[a];
      }
      const double c = -dn;
      if (slot == 0) {
        const double q = (L.ior[liq] - 1.0) / (L.ior[liq] + 1.0), r0 = q * q, m1 = 1.0 - c, m2 = m1 * m1;
        s_keep[0][tid] = r0 + (1.0 - r0) * ((m2 * m2) * m1);
      }
      const double kk = 1.0 - (eta * eta) * (1.0 - c * c);
      if (kk < 0.0) {                                 // total internal reflection: the liquid's own colour
        own = true;
        break;
      }
      const double w = eta * c - sqrt(kk);
      double tv[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) tv[a] = eta * d[a] + w * nn[a];
      const double tl = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        o[a] = xh[a] - L.bias * nn[a];
        d[a] = tv[a] / tl;
      }
      medium = slot == 0 ? id : -1;
      K = slot == 0 ? L.K_inside : C.K;
      slot += 1;
      continue;
    }
    // the surface finally shaded: Lambert from the normal as k_render_march stores it, rounded to float32
    if (slot == 1) s_keep[1][tid] = dep;
    sid = id;
    double l[3] = {L.light[0], L.light[1], L.light[2]};
    if (!L.has_light) {                               // the headlight: -d of the camera's ray, taken again, not carried
      double o0[3], d0[3];
      render_ray(C, i, j, o0, d0);
#pragma unroll
      for (int a = 0; a < 3; ++a) l[a] = -d0[a];
    }
    lam = fmax(0.0, ((double)(float)nn[0] * l[0] + (double)(float)nn[1] * l[1]) + (double)(float)nn[2] * l[2]);
    if (!L.shadows) break;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = xh[a] + L.bias * nn[a];
      d[a] = l[a];
    }
    medium = -1;
    mask = L.opaque;
    K = L.K_shadow;
    slot = 3;
  }

  const double R = s_keep[0][tid], len = s_keep[1][tid];
  const double w = 0.25 + 0.75 * ((lit ? 1.0 : 0.0) * lam);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double behind = sid >= 0 ? L.albedo[sid][a] * w : own ? L.albedo[liq][a] : L.background[a];
    color[3 * p + a] = liq >= 0 ? R * L.background[a] + ((1.0 - R) * exp(-(L.absorb[liq][a] * len))) * behind : behind;
  }
  length[p] = liq >= 0 ? len : 0.0;
  if (evals) evals[p] = count;
}

// the box filter of s x s sub-pixel colours, summed in row-major order, and floor(255 c + 0.5)
__global__ void __launch_bounds__(kRenderBlock)
k_render_resolve(const double* __restrict__ color, int W, int H, int s, unsigned char* __restrict__ rgb) {
  const int64_t p = (int64_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  const int i = (int)(p / W), j = (int)(p % W);
  double sum[3] = {0.0, 0.0, 0.0};
  for (int a = 0; a < s; ++a)
    for (int b = 0; b < s; ++b) {
      const int64_t q = ((int64_t)(i * s + a) * ((int64_t)W * s) + (j * s + b)) * 3;
      if (a == 0 && b == 0) {
        sum[0] = color[q], sum[1] = color[q + 1], sum[2] = color[q + 2];
      } else {
        sum[0] = sum[0] + color[q], sum[1] = sum[1] + color[q + 1], sum[2] = sum[2] + color[q + 2];
      }
    }
  const double area = (double)(s * s);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    double q = floor(255.0 * (sum[a] / area) + 0.5);
    q = fmin(fmax(q, 0.0), 255.0);                    // fmax drops a NaN
    rgb[3 * p + a] = (unsigned char)(int)q;
  }
}

// wave minimum in every lane (the tree of wave_sum); all 64 lanes active, no NaN among the operands
__device__ __forceinline__ double wave_min(double v) {
  v = fmin(v, dpp_f64<0xB1>(v));
  v = fmin(v, dpp_f64<0x4E>(v));
  v = fmin(v, dpp_f64<0x124>(v));
  v = fmin(v, dpp_f64<0x128>(v));
  return fmin(fmin(readlane_f64(v, 0), readlane_f64(v, 16)), fmin(readlane_f64(v, 32), readlane_f64(v, 48)));
}

__global__ void __launch_bounds__(kRenderBlock)
k_render_bricks(const void* __restrict__ vol, int dt, int n0, int n1, int n2, int nb1, int nb2, int maxima,
                double* __restrict__ out) {
  __shared__ double s_part[kRenderBlock / kWave];
  const int tid = threadIdx.x;
  const int b2 = (int)(blockIdx.x % (unsigned)nb2), b1 = (int)((blockIdx.x / (unsigned)nb2) % (unsigned)nb1),
            b0 = (int)(blockIdx.x / (unsigned)nb2 / (unsigned)nb1);
  double m = INFINITY;
  for (int q = tid; q < kBrickNodes; q += kRenderBlock) {
    const int i0 = kBrick * b0 + q / 81, i1 = kBrick * b1 + (q / 9) % 9, i2 = kBrick * b2 + q % 9;
    if (i0 < n0 && i1 < n1 && i2 < n2) {
      double v = ldx(vol, dt, ((int64_t)i0 * n1 + i1) * n2 + i2);
      if (maxima) v = -v;                             // max = -min(-v), exactly
      if (v != v) v = -INFINITY;
      m = fmin(m, v);
    }
  }
  m = wave_min(m);
  if ((tid & (kWave - 1)) == 0) s_part[tid / kWave] = m;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kRenderBlock / kWave; ++w) m = fmin(m, s_part[w]);
    out[blockIdx.x] = maxima ? -m : m;
  }
}

// albedo_id * (0.25 + 0.75 * max(0, n . l)), l = -d (a headlight) or the given direction; floor(255 c + 0.5)
__global__ void __launch_bounds__(kRenderBlock)
k_render_shade(RenderCamera C, RenderPalette P, const float* __restrict__ normal, const int* __restrict__ shape_id,
               unsigned char* __restrict__ rgb) {
  const int64_t p = (int64_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (p >= (int64_t)C.W * C.H) return;
  const int id = shape_id[p];
  if (id < 0 || id >= P.n) {
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb[3 * p + a] = (unsigned char)P.background[a];
    return;
  }
  double l[3] = {P.light[0], P.light[1], P.light[2]};
  if (!P.has_light) {
    double o[3], d[3];
    render_ray(C, (int)(p / C.W), (int)(p % C.W), o, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) l[a] = -d[a];
  }
  const double nl = ((double)normal[3 * p] * l[0] + (double)normal[3 * p + 1] * l[1]) + (double)normal[3 * p + 2] * l[2];
  const double lam = fmax(0.0, nl);
  const double w = 0.25 + 0.75 * lam;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = P.albedo[id][a] * w;
    double q = floor(255.0 * c + 0.5);
    q = fmin(fmax(q, 0.0), 255.0);                    // fmax drops a NaN
    rgb[3 * p + a] = (unsigned char)(int)q;
  }
}

// k_render_shade with one change: a pixel of shape albedo_id takes its albedo from pixel_albedo (H x W x 3 float32) in
// place of the palette's; a pixel whose albedo has a NaN component keeps the palette's
__global__ void __launch_bounds__(kRenderBlock)
k_render_shade_albedo(RenderCamera C, RenderPalette P, const float* __restrict__ normal, const int* __restrict__ shape_id,
                      const float* __restrict__ pixel_albedo, int albedo_id, unsigned char* __restrict__ rgb) {
  const int64_t p = (int64_t)blockIdx.x * kRenderBlock + threadIdx.x;
  if (p >= (int64_t)C.W * C.H) return;
  const int id = shape_id[p];
  if (id < 0 || id >= P.n) {
#pragma unroll
    for (int a = 0; a < 3; ++a) rgb[3 * p + a] = (unsigned char)P.background[a];
    return;
  }
  double l[3] = {P.light[0], P.light[1], P.light[2]};
  if (!P.has_light) {
    double o[3], d[3];
    render_ray(C, (int)(p / C.W), (int)(p % C.W), o, d);
#pragma unroll
    for (int a = 0; a < 3; ++a) l[a] = -d[a];
  }
  const double nl = ((double)normal[3 * p] * l[0] + (double)normal[3 * p + 1] * l[1]) + (double)normal[3 * p + 2] * l[2];
  const double lam = fmax(0.0, nl);
  const double w = 0.25 + 0.75 * lam;
  double alb[3] = {P.albedo[id][0], P.albedo[id][1], P.albedo[id][2]};
  if (id == albedo_id) {
    const float a0 = pixel_albedo[3 * p], a1 = pixel_albedo[3 * p + 1], a2 = pixel_albedo[3 * p + 2];
    if (a0 == a0 && a1 == a1 && a2 == a2) {
      alb[0] = (double)a0;
      alb[1] = (double)a1;
      alb[2] = (double)a2;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double c = alb[a] * w;
    double q = floor(255.0 * c + 0.5);
    q = fmin(fmax(q, 0.0), 255.0);                    // fmax drops a NaN
    rgb[3 * p + a] = (unsigned char)(int)q;
  }
}

static int fill_render_camera(RenderCamera* C, const double* camera, int ortho, int64_t width, int64_t height, double near,
                              double step, int64_t num_steps) {
  MFS_REQUIRE(camera, "null camera");
  MFS_REQUIRE(width >= 1 && width <= 16384 && height >= 1 && height <= 16384, "image extents must be in 1 .. 16384");
  MFS_REQUIRE(num_steps >= 1 && num_steps <= 65536, "number of steps must be in 1 .. 65536");
  MFS_REQUIRE(step > 0 && isfinite(step) && isfinite(near), "near must be finite and step positive");
  for (int k = 0; k < 14; ++k) MFS_REQUIRE(isfinite(camera[k]), "camera must be finite");
  MFS_REQUIRE(camera[12] > 0 && camera[13] > 0, "camera half extents must be positive");
  const double* f = camera + 3;
  MFS_REQUIRE((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2] > 0.25, "degenerate view direction");
  for (int k = 0; k < 3; ++k) {
    C->eye[k] = camera[k];
    C->f[k] = camera[3 + k];
    C->r[k] = camera[6 + k];
    C->u[k] = camera[9 + k];
  }
  C->half_w = camera[12];
  C->half_h = camera[13];
  C->near = near;
  C->step = step;
  C->ortho = ortho ? 1 : 0;
  C->W = (int)width;
  C->H = (int)height;
  C->K = (int)num_steps;
  return MFS_OK;
}

}  // namespace mfs

using namespace mfs;

extern "C" {

int64_t mfs_render_brick_count3d(const int64_t extents[3]) {
  if (!extents || !volume_extents_ok(extents)) return 0;
  return ((extents[0] - 2) / kBrick + 1) * ((extents[1] - 2) / kBrick + 1) * ((extents[2] - 2) / kBrick + 1);
}

int mfs_render_bricks3d(const void* volume, int dtype, const int64_t extents[3], void* bricks, mfs_stream stream) {
  MFS_REQUIRE(volume && extents && bricks, "null volume / extents / bricks");
  MFS_REQUIRE(dtype_ok(dtype), "dtype");
  MFS_REQUIRE(volume_extents_ok(extents), "volume extents must be >= 2, fewer than 2^31 nodes");
  const int nb1 = (int)((extents[1] - 2) / kBrick + 1), nb2 = (int)((extents[2] - 2) / kBrick + 1);
  const int64_t blocks = mfs_render_brick_count3d(extents);
  hipLaunchKernelGGL(k_render_bricks, dim3((unsigned)blocks), dim3(kRenderBlock), 0, (hipStream_t)stream, volume, dtype,
                     (int)extents[0], (int)extents[1], (int)extents[2], nb1, nb2, 0, (double*)bricks);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_render_bricks_max3d(const void* volume, int dtype, const int64_t extents[3], void* bricks, mfs_stream stream) {
  MFS_REQUIRE(volume && extents && bricks, "null volume / extents / bricks");
  MFS_REQUIRE(dtype_ok(dtype), "dtype");
  MFS_REQUIRE(volume_extents_ok(extents), "volume extents must be >= 2, fewer than 2^31 nodes");
  const int nb1 = (int)((extents[1] - 2) / kBrick + 1), nb2 = (int)((extents[2] - 2) / kBrick + 1);
  const int64_t blocks = mfs_render_brick_count3d(extents);
  hipLaunchKernelGGL(k_render_bricks, dim3((unsigned)blocks), dim3(kRenderBlock), 0, (hipStream_t)stream, volume, dtype,
                     (int)extents[0], (int)extents[1], (int)extents[2], nb1, nb2, 1, (double*)bricks);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_render_paths3d(const double* camera, int ortho, int64_t width, int64_t height, double near, double step,
                       int64_t num_steps, int64_t num_shapes, const void* const* volumes_host, const int* dtypes_host,
                       const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                       const double* poses_host, const void* const* bricks_host, const void* const* bricks_max_host,
                       int skip, const double* materials_host, const double* light_host, const int* background_host,
                       int shadows, double bias, int64_t shadow_steps, int64_t inside_steps, void* color, void* steps,
                       void* shape_id, void* length, void* evals, mfs_stream stream) {
  RenderCamera C;
  if (int st = fill_render_camera(&C, camera, ortho, width, height, near, step, num_steps)) return st;
  MFS_REQUIRE(num_shapes >= 1 && num_shapes <= kMaxVolumes, "1 to 16 shapes per scene");
  MFS_REQUIRE(volumes_host && dtypes_host && extents_host && origins_host && spacings_host && poses_host,
              "null shape description");
  MFS_REQUIRE(!skip || (bricks_host && bricks_max_host), "null brick grids");
  MFS_REQUIRE(materials_host && background_host, "null materials / background");
  MFS_REQUIRE(color && steps && shape_id && length, "null output");
  MFS_REQUIRE(shadow_steps >= 1 && shadow_steps <= 65536 && inside_steps >= 1 && inside_steps <= 65536,
              "shadow and inside steps must be in 1 .. 65536");
  MFS_REQUIRE(isfinite(bias) && bias >= 0, "bias must be finite and >= 0");
  const int m = (int)num_shapes;
  Volumes V;
  Poses P;
  if (int st = fill_volumes(&V, &P, m, volumes_host, dtypes_host, extents_host, origins_host, spacings_host, poses_host))
    return st;
  RenderBrickPtrs B;
  RenderLook L;
  memset(&B, 0, sizeof(B));
  memset(&L, 0, sizeof(L));
  for (int i = 0; i < m; ++i) {
    const double* mat = materials_host + 8 * i;      // kind (0 opaque, 1 liquid), r g b in 0 .. 1, ior, absorb r g b
    MFS_REQUIRE(mat[0] == 0.0 || mat[0] == 1.0, "material kind must be 0 (opaque) or 1 (liquid)");
    const bool liquid = mat[0] == 1.0;
    for (int k = 0; k < 3; ++k) {
      MFS_REQUIRE(isfinite(mat[1 + k]), "albedo must be finite");
      L.albedo[i][k] = mat[1 + k];
      MFS_REQUIRE(!liquid || (isfinite(mat[5 + k]) && mat[5 + k] >= 0), "absorb must be finite and >= 0");
      L.absorb[i][k] = liquid ? mat[5 + k] : 0.0;
    }
    MFS_REQUIRE(!liquid || (mat[4] > 1.0 && mat[4] <= 4.0), "ior must be in (1, 4]");
    L.ior[i] = liquid ? mat[4] : 0.0;
    if (!liquid) L.opaque |= 1u << i;
    MFS_REQUIRE(!skip || (bricks_host[i] && (!liquid || bricks_max_host[i])), "null brick grid");
    B.lo[i] = skip ? (const double*)bricks_host[i] : nullptr;
    B.hi[i] = skip && liquid ? (const double*)bricks_max_host[i] : nullptr;
  }
  for (int k = 0; k < 3; ++k) {
    MFS_REQUIRE(background_host[k] >= 0 && background_host[k] <= 255, "background must be in 0 .. 255");
    L.background[k] = (double)background_host[k] / 255.0;
    if (light_host) {
      MFS_REQUIRE(isfinite(light_host[k]), "light must be finite");
      L.light[k] = light_host[k];
    }
  }
  L.has_light = light_host ? 1 : 0;
  L.shadows = shadows ? 1 : 0;
  L.bias = bias;
  L.K_shadow = (int)shadow_steps;
  L.K_inside = (int)inside_steps;
  const dim3 grid((unsigned)((C.W + kRenderTile - 1) / kRenderTile), (unsigned)((C.H + kRenderTile - 1) / kRenderTile));
  hipLaunchKernelGGL(k_render_paths, grid, dim3(kRenderBlock), 0, (hipStream_t)stream, C, V, P, B, L, m, skip ? 1 : 0,
                     (double*)color, (int*)steps, (int*)shape_id, (double*)length, (int*)evals);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_render_resolve3d(const void* color, int64_t width, int64_t height, int samples, void* rgb, mfs_stream stream) {
  MFS_REQUIRE(color && rgb, "null color / rgb");
  MFS_REQUIRE(samples >= 1 && samples <= 4, "samples must be in 1 .. 4");
  MFS_REQUIRE(width >= 1 && height >= 1 && width * samples <= 16384 && height * samples <= 16384,
              "image extents times samples must be in 1 .. 16384");
  const int64_t pixels = width * height;
  hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((pixels + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0,
                     (hipStream_t)stream, (const double*)color, (int)width, (int)height, samples, (unsigned char*)rgb);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_render_march3d(const double* camera, int ortho, int64_t width, int64_t height, double near, double step,
                       int64_t num_steps, int64_t num_shapes, const void* const* volumes_host, const int* dtypes_host,
                       const int64_t* extents_host, const double* origins_host, const double* spacings_host,
                       const double* poses_host, const void* const* bricks_host, int skip, void* depth, void* normal,
                       void* shape_id, void* steps, void* evals, mfs_stream stream) {
  RenderCamera C;
  if (int st = fill_render_camera(&C, camera, ortho, width, height, near, step, num_steps)) return st;
  MFS_REQUIRE(num_shapes >= 1 && num_shapes <= kMaxVolumes, "1 to 16 shapes per scene");
  MFS_REQUIRE(volumes_host && dtypes_host && extents_host && origins_host && spacings_host && poses_host,
              "null shape description");
  MFS_REQUIRE(!skip || bricks_host, "null brick grids");
  MFS_REQUIRE(depth && normal && shape_id && steps, "null output");
  const int m = (int)num_shapes;
  Volumes V;
  Poses P;
  if (int st = fill_volumes(&V, &P, m, volumes_host, dtypes_host, extents_host, origins_host, spacings_host, poses_host))
    return st;
  RenderBricks B;
  memset(&B, 0, sizeof(B));
  for (int i = 0; i < m; ++i) {
    MFS_REQUIRE(!skip || bricks_host[i], "null brick grid");
    B.brick[i] = skip ? (const double*)bricks_host[i] : nullptr;
    for (int k = 0; k < 3; ++k) B.nb[i][k] = (V.n[i][k] - 2) / kBrick + 1;
  }
  const dim3 grid((unsigned)((C.W + kRenderTile - 1) / kRenderTile), (unsigned)((C.H + kRenderTile - 1) / kRenderTile));
  hipLaunchKernelGGL(k_render_march, grid, dim3(kRenderBlock), 0, (hipStream_t)stream, C, V, P, B, m, skip ? 1 : 0,
                     (double*)depth, (float*)normal, (int*)shape_id, (int*)steps, (int*)evals);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_render_shade3d(const double* camera, int ortho, int64_t width, int64_t height, const void* normal,
                       const void* shape_id, int64_t num_colors, const double* albedo_host, const int* background_host,
                       const double* light_host, void* rgb, mfs_stream stream) {
  RenderCamera C;
  if (int st = fill_render_camera(&C, camera, ortho, width, height, 0.0, 1.0, 1)) return st;
  MFS_REQUIRE(normal && shape_id && rgb, "null normal / shape_id / rgb");
  MFS_REQUIRE(num_colors >= 1 && num_colors <= kMaxVolumes, "1 to 16 colours");
  MFS_REQUIRE(albedo_host && background_host, "null albedo / background");
  RenderPalette P;
  memset(&P, 0, sizeof(P));
  P.n = (int)num_colors;
  for (int k = 0; k < 3 * P.n; ++k) {
    MFS_REQUIRE(isfinite(albedo_host[k]), "albedo must be finite");
    P.albedo[k / 3][k % 3] = albedo_host[k];
  }
  for (int k = 0; k < 3; ++k) {
    MFS_REQUIRE(background_host[k] >= 0 && background_host[k] <= 255, "background must be in 0 .. 255");
    P.background[k] = background_host[k];
    if (light_host) {
      MFS_REQUIRE(isfinite(light_host[k]), "light must be finite");
      P.light[k] = light_host[k];
    }
  }
  P.has_light = light_host ? 1 : 0;
  const int64_t pixels = (int64_t)C.W * C.H;
  hipLaunchKernelGGL(k_render_shade, dim3((unsigned)((pixels + kRenderBlock - 1) / kRenderBlock)), dim3(kRenderBlock), 0,
                     (hipStream_t)stream, C, P, (const float*)normal, (const int*)shape_id, (unsigned char*)rgb);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_render_shade_albedo3d(const double* camera, int ortho, int64_t width, int64_t height, const void* normal,
                              const void* shape_id, int64_t num_colors, const double* albedo_host,
                              const int* background_host, const double* light_host, const void* pixel_albedo,
                              int64_t albedo_id, void* rgb, mfs_stream stream) {
  RenderCamera C;
  if (int st = fill_render_camera(&C, camera, ortho, width, height, 0.0, 1.0, 1)) return st;
  MFS_REQUIRE(normal && shape_id && rgb && pixel_albedo, "null normal / shape_id / rgb / pixel_albedo");
  MFS_REQUIRE(num_colors >= 1 && num_colors <= kMaxVolumes, "1 to 16 colours");
  MFS_REQUIRE(albedo_id >= 0 && albedo_id < num_colors, "albedo_id must name one of the colours");
  MFS_REQUIRE(albedo_host && background_host, "null albedo / background");
  RenderPalette P;
  memset(&P, 0, sizeof(P));
  P.n = (int)num_colors;
  for (int k = 0; k < 3 * P.n; ++k) {
    MFS_REQUIRE(isfinite(albedo_host[k]), "albedo must be finite");
    P.albedo[k / 3][k % 3] = albedo_host[k];
  }
  for (int k = 0; k < 3; ++k) {
    MFS_REQUIRE(background_host[k] >= 0 && background_host[k] <= 255, "background must be in 0 .. 255");
    P.background[k] = background_host[k];
    if (light_host) {
      MFS_REQUIRE(isfinite(light_host[k]), "light must be finite");
      P.light[k] = light_host[k];
    }
  }
  P.has_light = light_host ? 1 : 0;
  const int64_t pixels = (int64_t)C.W * C.H;
  hipLaunchKernelGGL(k_render_shade_albedo, dim3((unsigned)((pixels + kRenderBlock - 1) / kRenderBlock)),
                     dim3(kRenderBlock), 0, (hipStream_t)stream, C, P, (const float*)normal, (const int*)shape_id,
                     (const float*)pixel_albedo, (int)albedo_id, (unsigned char*)rgb);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

}  // extern "C"
