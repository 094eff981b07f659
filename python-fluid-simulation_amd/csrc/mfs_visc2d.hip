// mfs_visc2d.hip -- ViscosityCGSolver2D on gfx950.
//
// Reference: solver/ViscosityCGSolver2D.py.  Two layers:
//  * direct kernels (rhs, apply, writeback): one thread per face, the reference's statements in its order, on arrays
//    of either dtype.  They serve the module functions and are the bit-level yardstick of the engine;
//  * the engine mfs_vcg2d_*: the CG loop on the shared device-resident core (mfs_cg_core.h) over flat
//    [x-faces | y-faces] vectors.  Its operator apply is the hot path: one thread per cell computes q_x and q_y of that
//    cell, the sphi tests are folded into per-face class bits at setup, and `vol` is de-interleaved into four fp64
//    parity planes (cell centres, nodes, x-face centres, y-face centres) that share one row stride with the class
//    words and the y-face arrays.
//
// Quirks kept from the reference (not fixed): a face sample is solid where sphi <= 0 (3D: < 0); coupling terms apply
// where the neighbour sample is > 0, RHS terms where it is <= 0; boundary faces of b / q (x == 0, x >= shape[0]-1,
// y == 0, y >= shape[1]-1 of each component's own array) are never written.
//
// No FMA contraction in this file: the engine apply and the direct kernel must round identically (bit-equal q), and
// both must round where the reference's separate multiplies and adds round.
#pragma clang fp contract(off)

#include "mfs_cg_core.h"

namespace mfs {

struct V2 {
  int Nx, Ny;
  __device__ int64_t fx(int x, int y) const { return (int64_t)x * Ny + y; }          // (Nx+1, Ny)
  __device__ int64_t fy(int x, int y) const { return (int64_t)x * (Ny + 1) + y; }    // (Nx, Ny+1)
  __device__ int64_t dg(int i, int j) const { return (int64_t)i * (2 * Ny + 1) + j; }
  __host__ __device__ int64_t nfx() const { return (int64_t)(Nx + 1) * Ny; }
  __host__ __device__ int64_t nfy() const { return (int64_t)Nx * (Ny + 1); }
};

// ----------------------------------------------------------------------------------------------- direct kernels ---
// solver/ViscosityCGSolver2D.py:6-103 (x kernel :6-55, y kernel :57-103); threads [0, nfx) are x-faces, the rest y-faces
__global__ void __launch_bounds__(256)
k_visc_rhs2d(V2 g, double scale, double mu, const void* vx, const void* vy, int vdt, const void* sphi, int sdt,
             const void* vol, int wdt, void* bx, void* by, int bdt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nfx = g.nfx();
  if (t >= nfx + g.nfy()) return;
  auto S = [&](int i, int j) { return ldx(sphi, sdt, g.dg(i, j)); };
  auto W = [&](int i, int j) { return ldx(vol, wdt, g.dg(i, j)); };
  auto VX = [&](int x, int y) { return ldx(vx, vdt, g.fx(x, y)); };
  auto VY = [&](int x, int y) { return ldx(vy, vdt, g.fy(x, y)); };
  if (t < nfx) {
    const int x = (int)(t / g.Ny), y = (int)(t % g.Ny);
    if (x == 0 || x >= g.Nx || y == 0 || y >= g.Ny - 1) return;
    if (S(2 * x, 2 * y + 1) <= 0) { stx(bx, bdt, t, 0.0); return; }
    const double vc = W(2 * x, 2 * y + 1), vr = W(2 * x + 1, 2 * y + 1), vl = W(2 * x - 1, 2 * y + 1);
    const double vt = W(2 * x, 2 * y + 2), vb = W(2 * x, 2 * y);
    double b = VX(x, y) * vc;
    if (S(2 * x + 2, 2 * y + 1) <= 0) b += 2 * scale * mu * vr * VX(x + 1, y);
    if (S(2 * x - 2, 2 * y + 1) <= 0) b += 2 * scale * mu * vl * VX(x - 1, y);
    if (S(2 * x, 2 * y + 3) <= 0) b += scale * mu * vt * VX(x, y + 1);
    if (S(2 * x, 2 * y - 1) <= 0) b += scale * mu * vb * VX(x, y - 1);
    if (S(2 * x + 1, 2 * y + 2) <= 0) b += scale * mu * vt * VY(x, y + 1);
    if (S(2 * x - 1, 2 * y + 2) <= 0) b -= scale * mu * vt * VY(x - 1, y + 1);
    if (S(2 * x + 1, 2 * y) <= 0) b -= scale * mu * vb * VY(x, y);
    if (S(2 * x - 1, 2 * y) <= 0) b += scale * mu * vb * VY(x - 1, y);
    stx(bx, bdt, t, b);
  } else {
    const int64_t u = t - nfx;
    const int x = (int)(u / (g.Ny + 1)), y = (int)(u % (g.Ny + 1));
    if (x == 0 || x >= g.Nx - 1 || y == 0 || y >= g.Ny) return;
    if (S(2 * x + 1, 2 * y) <= 0) { stx(by, bdt, u, 0.0); return; }
    const double vc = W(2 * x + 1, 2 * y), vr = W(2 * x + 2, 2 * y), vl = W(2 * x, 2 * y);
    const double vt = W(2 * x + 1, 2 * y + 1), vb = W(2 * x + 1, 2 * y - 1);
    double b = VY(x, y) * vc;
    if (S(2 * x + 3, 2 * y) <= 0) b += scale * mu * vr * VY(x + 1, y);
    if (S(2 * x - 1, 2 * y) <= 0) b += scale * mu * vl * VY(x - 1, y);
    if (S(2 * x + 1, 2 * y + 2) <= 0) b += 2 * scale * mu * vt * VY(x, y + 1);
    if (S(2 * x + 1, 2 * y - 2) <= 0) b += 2 * scale * mu * vb * VY(x, y - 1);
    if (S(2 * x + 2, 2 * y + 1) <= 0) b += scale * mu * vr * VX(x + 1, y);
    if (S(2 * x + 2, 2 * y - 1) <= 0) b -= scale * mu * vr * VX(x + 1, y - 1);
    if (S(2 * x, 2 * y + 1) <= 0) b -= scale * mu * vl * VX(x, y);
    if (S(2 * x, 2 * y - 1) <= 0) b += scale * mu * vl * VX(x, y - 1);
    stx(by, bdt, u, b);
  }
}

// solver/ViscosityCGSolver2D.py:105-207 (x kernel :105-156, y kernel :158-207)
__global__ void __launch_bounds__(256)
k_visc_apply2d(V2 g, double scale, double mu, const void* vx, const void* vy, int vdt, void* ox, void* oy, int odt,
               const void* sphi, int sdt, const void* vol, int wdt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nfx = g.nfx();
  if (t >= nfx + g.nfy()) return;
  auto S = [&](int i, int j) { return ldx(sphi, sdt, g.dg(i, j)); };
  auto W = [&](int i, int j) { return ldx(vol, wdt, g.dg(i, j)); };
  auto VX = [&](int x, int y) { return ldx(vx, vdt, g.fx(x, y)); };
  auto VY = [&](int x, int y) { return ldx(vy, vdt, g.fy(x, y)); };
  if (t < nfx) {
    const int x = (int)(t / g.Ny), y = (int)(t % g.Ny);
    if (x == 0 || x >= g.Nx || y == 0 || y >= g.Ny - 1) return;
    if (S(2 * x, 2 * y + 1) <= 0) { stx(ox, odt, t, 0.0); return; }
    const double vc = W(2 * x, 2 * y + 1), vr = W(2 * x + 1, 2 * y + 1), vl = W(2 * x - 1, 2 * y + 1);
    const double vt = W(2 * x, 2 * y + 2), vb = W(2 * x, 2 * y);
    const double diag = vc + scale * mu * (2 * vr + 2 * vl + vt + vb);
    double val = diag * VX(x, y);
    if (S(2 * x + 2, 2 * y + 1) > 0) val -= 2 * scale * mu * vr * VX(x + 1, y);
    if (S(2 * x - 2, 2 * y + 1) > 0) val -= 2 * scale * mu * vl * VX(x - 1, y);
    if (S(2 * x, 2 * y + 3) > 0) val -= scale * mu * vt * VX(x, y + 1);
    if (S(2 * x, 2 * y - 1) > 0) val -= scale * mu * vb * VX(x, y - 1);
    if (S(2 * x + 1, 2 * y + 2) > 0) val -= scale * mu * vt * VY(x, y + 1);
    if (S(2 * x - 1, 2 * y + 2) > 0) val += scale * mu * vt * VY(x - 1, y + 1);
    if (S(2 * x + 1, 2 * y) > 0) val += scale * mu * vb * VY(x, y);
    if (S(2 * x - 1, 2 * y) > 0) val -= scale * mu * vb * VY(x - 1, y);
    stx(ox, odt, t, val);
  } else {
    const int64_t u = t - nfx;
    const int x = (int)(u / (g.Ny + 1)), y = (int)(u % (g.Ny + 1));
    if (x == 0 || x >= g.Nx - 1 || y == 0 || y >= g.Ny) return;
    if (S(2 * x + 1, 2 * y) <= 0) { stx(oy, odt, u, 0.0); return; }
    const double vc = W(2 * x + 1, 2 * y), vr = W(2 * x + 2, 2 * y), vl = W(2 * x, 2 * y);
    const double vt = W(2 * x + 1, 2 * y + 1), vb = W(2 * x + 1, 2 * y - 1);
    const double diag = vc + scale * mu * (vr + vl + 2 * vt + 2 * vb);
    double val = diag * VY(x, y);
    if (S(2 * x + 3, 2 * y) > 0) val -= scale * mu * vr * VY(x + 1, y);
    if (S(2 * x - 1, 2 * y) > 0) val -= scale * mu * vl * VY(x - 1, y);
    if (S(2 * x + 1, 2 * y + 2) > 0) val -= 2 * scale * mu * vt * VY(x, y + 1);
    if (S(2 * x + 1, 2 * y - 2) > 0) val -= 2 * scale * mu * vb * VY(x, y - 1);
    if (S(2 * x + 2, 2 * y + 1) > 0) val -= scale * mu * vr * VX(x + 1, y);
    if (S(2 * x + 2, 2 * y - 1) > 0) val += scale * mu * vr * VX(x + 1, y - 1);
    if (S(2 * x, 2 * y + 1) > 0) val += scale * mu * vl * VX(x, y);
    if (S(2 * x, 2 * y - 1) > 0) val -= scale * mu * vl * VX(x, y - 1);
    stx(oy, odt, u, val);
  }
}

// solver/ViscosityCGSolver2D.py:209-220: cells 1 <= x <= Nx-1, 1 <= y <= Ny-1 copy their non-solid faces
__global__ void __launch_bounds__(256)
k_visc_writeback2d(V2 g, void* vx, void* vy, int vdt, const void* ox, const void* oy, int odt, const void* sphi,
                   int sdt) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)g.Nx * g.Ny) return;
  const int x = (int)(t / g.Ny), y = (int)(t % g.Ny);
  if (x == 0 || y == 0) return;
  if (ldx(sphi, sdt, g.dg(2 * x, 2 * y + 1)) > 0) stx(vx, vdt, g.fx(x, y), ldx(ox, odt, g.fx(x, y)));
  if (ldx(sphi, sdt, g.dg(2 * x + 1, 2 * y)) > 0) stx(vy, vdt, g.fy(x, y), ldx(oy, odt, g.fy(x, y)));
}

// ------------------------------------------------------------------------------------------------------ engine ---
// Per cell (x, y), 0 <= x <= Nx, 0 <= y <= Ny, index c = x (Ny+1) + y (= the y-face index of (x, y)): one class word.
// Bits 0-7 the x-face's eight coupling tests (:124-147, neighbour sample > 0), bit 8 solid (:113, sample <= 0),
// bit 9 the face has an equation (interior); bits 16-25 the same for the y-face (:175-198, :164).
enum : uint32_t { kSolid = 1u << 8, kActive = 1u << 9, kYShift = 16 };

// solver/ViscosityCGSolver2D.py:113-147, :164-198 as bits; vol -> four fp64 parity planes (row stride Ny+1):
// VC = vol[2x+1, 2y+1], VN = vol[2x, 2y], VFX = vol[2x, 2y+1], VFY = vol[2x+1, 2y] (0 where the sample does not exist)
__global__ void __launch_bounds__(256)
k_vcg2d_setup(V2 g, const void* sphi, int sdt, const void* vol, int wdt, uint32_t* cls, double* vc, double* vn,
              double* vfx, double* vfy) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= (int64_t)(g.Nx + 1) * (g.Ny + 1)) return;
  const int x = (int)(c / (g.Ny + 1)), y = (int)(c % (g.Ny + 1));
  auto W = [&](int i, int j) { return ldx(vol, wdt, g.dg(i, j)); };
  auto P = [&](int i, int j) { return ldx(sphi, sdt, g.dg(i, j)) > 0; };
  vc[c] = (x < g.Nx && y < g.Ny) ? W(2 * x + 1, 2 * y + 1) : 0.0;
  vn[c] = W(2 * x, 2 * y);
  vfx[c] = y < g.Ny ? W(2 * x, 2 * y + 1) : 0.0;
  vfy[c] = x < g.Nx ? W(2 * x + 1, 2 * y) : 0.0;
  uint32_t w = 0;
  if (x >= 1 && x <= g.Nx - 1 && y >= 1 && y <= g.Ny - 2) {
    w |= kActive;
    if (ldx(sphi, sdt, g.dg(2 * x, 2 * y + 1)) <= 0) w |= kSolid;
    w |= (uint32_t)P(2 * x + 2, 2 * y + 1) << 0 | (uint32_t)P(2 * x - 2, 2 * y + 1) << 1 |
         (uint32_t)P(2 * x, 2 * y + 3) << 2 | (uint32_t)P(2 * x, 2 * y - 1) << 3 |
         (uint32_t)P(2 * x + 1, 2 * y + 2) << 4 | (uint32_t)P(2 * x - 1, 2 * y + 2) << 5 |
         (uint32_t)P(2 * x + 1, 2 * y) << 6 | (uint32_t)P(2 * x - 1, 2 * y) << 7;
  }
  if (x >= 1 && x <= g.Nx - 2 && y >= 1 && y <= g.Ny - 1) {
    uint32_t v = kActive;
    if (ldx(sphi, sdt, g.dg(2 * x + 1, 2 * y)) <= 0) v |= kSolid;
    v |= (uint32_t)P(2 * x + 3, 2 * y) << 0 | (uint32_t)P(2 * x - 1, 2 * y) << 1 |
         (uint32_t)P(2 * x + 1, 2 * y + 2) << 2 | (uint32_t)P(2 * x + 1, 2 * y - 2) << 3 |
         (uint32_t)P(2 * x + 2, 2 * y + 1) << 4 | (uint32_t)P(2 * x + 2, 2 * y - 1) << 5 |
         (uint32_t)P(2 * x, 2 * y + 1) << 6 | (uint32_t)P(2 * x, 2 * y - 1) << 7;
    w |= v << kYShift;
  }
  cls[c] = w;
}

// q = A v on the flat vectors (the loop's stencil launch); per-block partials of v.q.  One thread per cell (grid-stride
// over the cells): the x-face and the y-face of cell (x, y) share VC[c] and VN[c] and most of their neighbour reads.
// Faces without an equation are not written.  The statements are those of k_visc_apply2d with `2 * scale * mu` and
// `scale * mu` evaluated once on the host (the reference's left-to-right products, so the same bits).  The eight
// neighbour values of a face are loaded unconditionally (every address is inside the arrays for a face with an
// equation) and the class bits select the terms, so the loads of a face are in flight together instead of one
// branch at a time.
template <typename T>
__global__ void __launch_bounds__(256)
k_vcg2d_apply(int Nx, int Ny, const T* __restrict__ v, T* __restrict__ q, const uint32_t* __restrict__ cls,
              const double* __restrict__ VC, const double* __restrict__ VN, const double* __restrict__ VFX,
              const double* __restrict__ VFY, double sm, double s2m, double* __restrict__ partial,
              const double* __restrict__ done_flag) {
  if (done_flag && *done_flag != 0.0) return;
  const int64_t ncell = (int64_t)(Nx + 1) * (Ny + 1), nfx = (int64_t)(Nx + 1) * Ny;
  const int64_t R = Ny + 1;                       // row stride of the planes, class words and y-faces
  const T* __restrict__ vx = v;
  const T* __restrict__ vy = v + nfx;
  T* __restrict__ qx = q;
  T* __restrict__ qy = q + nfx;
  double acc = 0.0;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < ncell; c += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t w = cls[c];
    if (!(w & (kActive | (kActive << kYShift)))) continue;
    const int x = (int)(c / R), y = (int)(c - (int64_t)x * R);
    const int64_t ix = (int64_t)x * Ny + y;      // x-face (x, y); the y-face (x, y) is c
    const double vcc = VC[c], vnn = VN[c];
    if (w & kActive) {                                                         // :105-156
      double val = 0.0;
      const double v0 = (double)vx[ix];
      if (!(w & kSolid)) {
        const double vr = vcc, vl = VC[c - R], vt = VN[c + 1], vb = vnn, vc = VFX[c];
        const double n0 = (double)vx[ix + Ny], n1 = (double)vx[ix - Ny], n2 = (double)vx[ix + 1],
                     n3 = (double)vx[ix - 1], n4 = (double)vy[c + 1], n5 = (double)vy[c - R + 1],
                     n6 = (double)vy[c], n7 = (double)vy[c - R];
        const double diag = vc + sm * (2 * vr + 2 * vl + vt + vb);
        val = diag * v0;
        val = (w & 1u) ? val - s2m * vr * n0 : val;
        val = (w & 2u) ? val - s2m * vl * n1 : val;
        val = (w & 4u) ? val - sm * vt * n2 : val;
        val = (w & 8u) ? val - sm * vb * n3 : val;
        val = (w & 16u) ? val - sm * vt * n4 : val;
        val = (w & 32u) ? val + sm * vt * n5 : val;
        val = (w & 64u) ? val + sm * vb * n6 : val;
        val = (w & 128u) ? val - sm * vb * n7 : val;
      }
      const T st = (T)val;
      qx[ix] = st;
      acc += v0 * (double)st;
    }
    const uint32_t u = w >> kYShift;
    if (u & kActive) {                                                         // :158-207
      double val = 0.0;
      const double v0 = (double)vy[c];
      if (!(u & kSolid)) {
        const double vr = VN[c + R], vl = vnn, vt = vcc, vb = VC[c - 1], vc = VFY[c];
        const double n0 = (double)vy[c + R], n1 = (double)vy[c - R], n2 = (double)vy[c + 1], n3 = (double)vy[c - 1],
                     n4 = (double)vx[ix + Ny], n5 = (double)vx[ix + Ny - 1], n6 = (double)vx[ix],
                     n7 = (double)vx[ix - 1];
        const double diag = vc + sm * (vr + vl + 2 * vt + 2 * vb);
        val = diag * v0;
        val = (u & 1u) ? val - sm * vr * n0 : val;
        val = (u & 2u) ? val - sm * vl * n1 : val;
        val = (u & 4u) ? val - s2m * vt * n2 : val;
        val = (u & 8u) ? val - s2m * vb * n3 : val;
        val = (u & 16u) ? val - sm * vr * n4 : val;
        val = (u & 32u) ? val + sm * vr * n5 : val;
        val = (u & 64u) ? val + sm * vl * n6 : val;
        val = (u & 128u) ? val - sm * vl * n7 : val;
      }
      const T st = (T)val;
      qy[c] = st;
      acc += v0 * (double)st;
    }
  }
  if (partial) {
    const double tot = block_sum<256>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
  }
}

}  // namespace mfs

using namespace mfs;

struct mfs_vcg2d {
  V2 g;
  int dt;
  CgCore c;
  int64_t ncell;
  uint32_t* cls;
  double *vc, *vn, *vfx, *vfy;
  double sm, s2m;
  bool set_up;
  int grid;
};

static size_t vcg2d_tables_bytes(const int64_t gres[2]) {
  const size_t nc = (size_t)(gres[0] + 1) * (size_t)(gres[1] + 1);
  return 4 * align_up(nc * 8, 256) + align_up(nc * 4, 256);
}

static int vcg2d_apply(mfs_vcg2d* h, const void* v, void* out, bool use_done, hipStream_t st) {
  const double* done = use_done ? h->c.scal + S_DONE : nullptr;
  if (h->dt == MFS_F32)
    hipLaunchKernelGGL((k_vcg2d_apply<float>), dim3(h->grid), dim3(256), 0, st, h->g.Nx, h->g.Ny, (const float*)v,
                       (float*)out, h->cls, h->vc, h->vn, h->vfx, h->vfy, h->sm, h->s2m, h->c.part_dq, done);
  else
    hipLaunchKernelGGL((k_vcg2d_apply<double>), dim3(h->grid), dim3(256), 0, st, h->g.Nx, h->g.Ny, (const double*)v,
                       (double*)out, h->cls, h->vc, h->vn, h->vfx, h->vfy, h->sm, h->s2m, h->c.part_dq, done);
  MFS_LAUNCH_CHECK();
  h->c.n_part_dq = h->grid;
  return MFS_OK;
}

extern "C" {

int mfs_visc_rhs2d(const int64_t gres[2], double scale, double mu, const void* vx, const void* vy, int v_dt,
                   const void* sphi, int sphi_dt, const void* vol, int vol_dt, void* b_x, void* b_y, int b_dt,
                   mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(vx && vy && sphi && vol && b_x && b_y, "null array");
  MFS_REQUIRE(b_x != b_y && b_x != vx && b_x != vy && b_y != vx && b_y != vy, "aliased array");
  MFS_REQUIRE(dtype_ok(v_dt) && dtype_ok(sphi_dt) && dtype_ok(vol_dt) && dtype_ok(b_dt), "dtype");
  V2 g{(int)gres[0], (int)gres[1]};
  const int64_t n = g.nfx() + g.nfy();
  hipLaunchKernelGGL(k_visc_rhs2d, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g, scale, mu, vx, vy, v_dt,
                     sphi, sphi_dt, vol, vol_dt, b_x, b_y, b_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_visc_apply2d(const int64_t gres[2], double scale, double mu, const void* vx, const void* vy, int v_dt,
                     void* out_x, void* out_y, int out_dt, const void* sphi, int sphi_dt, const void* vol, int vol_dt,
                     mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(vx && vy && out_x && out_y && sphi && vol, "null array");
  MFS_REQUIRE(out_x != out_y && out_x != vx && out_x != vy && out_y != vx && out_y != vy, "aliased array");
  MFS_REQUIRE(dtype_ok(v_dt) && dtype_ok(out_dt) && dtype_ok(sphi_dt) && dtype_ok(vol_dt), "dtype");
  V2 g{(int)gres[0], (int)gres[1]};
  const int64_t n = g.nfx() + g.nfy();
  hipLaunchKernelGGL(k_visc_apply2d, dim3(cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, g, scale, mu, vx, vy,
                     v_dt, out_x, out_y, out_dt, sphi, sphi_dt, vol, vol_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int mfs_visc_writeback2d(const int64_t gres[2], void* vx, void* vy, int v_dt, const void* out_x, const void* out_y,
                         int out_dt, const void* sphi, int sphi_dt, mfs_stream stream) {
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(vx && vy && out_x && out_y && sphi, "null array");
  MFS_REQUIRE(vx != vy && vx != out_x && vx != out_y && vy != out_x && vy != out_y, "aliased array");
  MFS_REQUIRE(dtype_ok(v_dt) && dtype_ok(out_dt) && dtype_ok(sphi_dt), "dtype");
  V2 g{(int)gres[0], (int)gres[1]};
  hipLaunchKernelGGL(k_visc_writeback2d, dim3(cdiv(gres[0] * gres[1], 256)), dim3(256), 0, (hipStream_t)stream, g, vx,
                     vy, v_dt, out_x, out_y, out_dt, sphi, sphi_dt);
  MFS_LAUNCH_CHECK();
  return MFS_OK;
}

int64_t mfs_vcg2d_dofs(const int64_t gres[2]) {
  if (!gres || gres[0] < 1 || gres[1] < 1) return 0;
  return (gres[0] + 1) * gres[1] + gres[0] * (gres[1] + 1);
}

size_t mfs_vcg2d_workspace_bytes(const int64_t gres[2], int dt) {
  if (!gres || !dtype_ok(dt) || gres[0] < 1 || gres[1] < 1 || gres[0] > 65536 || gres[1] > 65536) return 0;
  return core_ws_bytes() + vcg2d_tables_bytes(gres) + 256;
}

int mfs_vcg2d_create(mfs_vcg2d** out, const int64_t gres[2], int dt, void* workspace, size_t workspace_bytes,
                     mfs_stream stream) {
  MFS_REQUIRE(out && workspace, "null argument");
  if (int e = check_gres2(gres)) return e;
  MFS_REQUIRE(dtype_ok(dt), "dtype");
  MFS_REQUIRE(((uintptr_t)workspace % 256) == 0, "workspace must be 256-byte aligned");
  MFS_REQUIRE(workspace_bytes >= mfs_vcg2d_workspace_bytes(gres, dt), "workspace too small");
  mfs_vcg2d* h = new mfs_vcg2d();
  h->g = V2{(int)gres[0], (int)gres[1]};
  h->dt = dt;
  h->ncell = (gres[0] + 1) * (gres[1] + 1);
  if (int e = core_init(h->c, dt, mfs_vcg2d_dofs(gres))) { delete h; return e; }
  char* p = core_carve(h->c, (char*)workspace);
  const size_t plane = align_up((size_t)h->ncell * 8, 256);
  h->vc = (double*)p; p += plane;
  h->vn = (double*)p; p += plane;
  h->vfx = (double*)p; p += plane;
  h->vfy = (double*)p; p += plane;
  h->cls = (uint32_t*)p;
  h->sm = h->s2m = 0.0;
  h->set_up = false;
  h->grid = std::max(1, std::min<int>(h->c.grid_vec, cdiv(h->ncell, 256)));
  if (hipMemsetAsync(workspace, 0, core_ws_bytes(), (hipStream_t)stream) != hipSuccess) {
    set_error("hipMemsetAsync(workspace) failed");
    core_free(h->c);
    delete h;
    return MFS_E_HIP;
  }
  *out = h;
  return MFS_OK;
}

int mfs_vcg2d_destroy(mfs_vcg2d* h) {
  if (!h) return MFS_OK;
  core_free(h->c);
  delete h;
  return MFS_OK;
}

int mfs_vcg2d_setup(mfs_vcg2d* h, double scale, double mu, const void* sphi, int sphi_dt, const void* vol, int vol_dt,
                    mfs_stream stream) {
  MFS_REQUIRE(h && sphi && vol, "null argument");
  MFS_REQUIRE(dtype_ok(sphi_dt) && dtype_ok(vol_dt), "dtype");
  h->sm = scale * mu;              // `scale * mu * ...` (:126-147)
  h->s2m = 2 * scale * mu;         // `2 * scale * mu * ...` (:125-128, :175-178)
  hipLaunchKernelGGL(k_vcg2d_setup, dim3(cdiv(h->ncell, 256)), dim3(256), 0, (hipStream_t)stream, h->g, sphi, sphi_dt,
                     vol, vol_dt, h->cls, h->vc, h->vn, h->vfx, h->vfy);
  MFS_LAUNCH_CHECK();
  h->set_up = true;
  return MFS_OK;
}

int mfs_vcg2d_bind(mfs_vcg2d* h, void* b, void* x, void* d, void* r, void* q) {
  MFS_REQUIRE(h, "null handle");
  return core_bind(h->c, b, x, d, r, q);
}

int mfs_vcg2d_apply(mfs_vcg2d* h, const void* v, void* out, mfs_stream stream) {
  MFS_REQUIRE(h && v && out && v != out, "null / aliased argument");
  MFS_REQUIRE(h->set_up, "engine not set up");
  return vcg2d_apply(h, v, out, false, (hipStream_t)stream);
}

int mfs_vcg2d_poll(mfs_vcg2d* h, mfs_stream stream, int64_t* iters, int* done, double* delta, double* alpha,
                   double* beta) {
  MFS_REQUIRE(h, "null handle");
  return core_poll(h->c, (hipStream_t)stream, iters, done, delta, alpha, beta);
}

// solver/ViscosityCGSolver2D.py:266-315: x = v on entry (not zeroed), r0 = b - A v, then the loop.  Returns
// MFS_NOT_CONVERGED after max_iter iterations (the reference raises ValueError there, :314-315: the caller does).
int mfs_vcg2d_solve(mfs_vcg2d* h, double tol, int64_t max_iter, int64_t check_every, mfs_stream stream,
                    int64_t* iters_host) {
  MFS_REQUIRE(h && h->c.x && h->set_up, "engine not bound / set up");
  MFS_REQUIRE(max_iter >= 0 && check_every >= 1, "max_iter / check_every");
  hipStream_t st = (hipStream_t)stream;
  return core_solve(h->c, tol, false, max_iter, check_every, st, iters_host,
                    [=](const void* v, void* out, bool use_done) { return vcg2d_apply(h, v, out, use_done, st); });
}

int64_t mfs_vcg2d_history(mfs_vcg2d* h, double* out_host, int64_t cap, mfs_stream stream) {
  if (!h) { set_error("mfs_vcg2d_history: null handle"); return MFS_E_INVALID; }
  return core_history(h->c, out_host, cap, (hipStream_t)stream);
}

}  // extern "C"
