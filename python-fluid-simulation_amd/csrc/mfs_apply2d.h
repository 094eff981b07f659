// mfs_apply2d.h -- the 5-point ghost-fluid stencil launch of the 2D CG engine (mfs_pressure2d.hip), shared by the two
// operators that run on it and by their stateless entry points:
//   DENS = false   PressureCGSolver2D.matvecmul_kernel (solver/PressureCGSolver2D.py:46-100): diag += w per fluid
//                  neighbour, w / theta per air neighbour
//   DENS = true    DensityCGSolver2D.matvecmul_kernel (solver/DensityCGSolver2D.py:85-139): diag += 1 per fluid
//                  neighbour, 1 / theta per air neighbour (no face weight in diag); the off-diagonal keeps w
// One template, so the engine's launch and the stateless launch of an operator are the same instructions per cell
// (bit-identical results), and the pressure instantiation is the arithmetic it was before the density operator existed.
#pragma once
#include "mfs_common.h"

namespace mfs {

struct Grid2 {
  int Nx, Ny;
  __device__ int64_t c(int x, int y) const { return (int64_t)x * Ny + y; }
  __device__ int64_t fx(int x, int y) const { return (int64_t)x * Ny + y; }
  __device__ int64_t fy(int x, int y) const { return (int64_t)x * (Ny + 1) + y; }
  __device__ int64_t dg(int i, int j) const { return (int64_t)i * (2 * Ny + 1) + j; }
};

// out = A v on interior cells (grid-stride; consecutive threads on consecutive y: coalesced); with `partial` also
// leaves per-block partials of v.out
template <bool DENS>
__global__ void __launch_bounds__(256)
k_apply2d(Grid2 g, const void* v, void* out, int dt, const void* wx, const void* wy, int wdt, const void* lphi, int ldt,
          double* partial, const double* done_flag) {
  // contraction stated here (the compiler's default for device code), so that the operator rounds the same in every
  // file that instantiates it, whatever contraction pragma that file sets before or after including this header
#pragma clang fp contract(fast)
  if (done_flag && *done_flag != 0.0) return;
  const int64_t n = (int64_t)g.Nx * g.Ny;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int y = (int)(i % g.Ny), x = (int)(i / g.Ny);
    if (x == 0 || x >= g.Nx - 1 || y == 0 || y >= g.Ny - 1) {
      // never written, yet the reference's d.q sums the whole arrays: a shared buffer's stale q counts here
      if (partial) acc += ldx(v, dt, i) * ldx(out, dt, i);
      continue;
    }
    const double phi = ldx(lphi, ldt, i);
    if (!(phi < 0)) { stx(out, dt, i, 0.0); continue; }
    double val = 0.0, diag = 0.0;
    auto tap = [&](int64_t nb, double w) {
#pragma clang fp contract(fast)
      const double nphi = ldx(lphi, ldt, nb);
      const double dw = DENS ? 1.0 : w;
      if (nphi < 0) { val -= w * ldx(v, dt, nb); diag += dw; }
      else          { diag += dw / fmin(1.0, fmax(0.01, phi / (phi - nphi))); }
    };
    tap(i + g.Ny, ldx(wx, wdt, g.fx(x + 1, y)));
    tap(i - g.Ny, ldx(wx, wdt, g.fx(x, y)));
    tap(i + 1, ldx(wy, wdt, g.fy(x, y + 1)));
    tap(i - 1, ldx(wy, wdt, g.fy(x, y)));
    const double vc = ldx(v, dt, i);
    val += diag * vc;
    stx(out, dt, i, val);
    acc += vc * (dt == MFS_F32 ? (double)(float)val : val);
  }
  if (partial) {
    const double tot = block_sum<256>(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
  }
}

}  // namespace mfs
