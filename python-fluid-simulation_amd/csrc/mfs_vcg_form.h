// mfs_vcg_form.h -- which kernel a stencil launch of the viscosity engine takes, and which loop mfs_vcg3d_iterate runs.
//
// Plain C++17, no HIP.  vmarch_form() is the ONE place where the engine's knobs, the grid, the operands' alignment and the
// caller's fused request become a kernel kind and, for the x-marching kernel (mfs_vcg_march.h), its template arguments, LDS
// bytes and main grid; vmarch_reachable() is the table of the tuples that can come out of it -- vcg_launch_march
// (mfs_visc.hip) instantiates exactly those.  vloop_form() is the one place where the loop is chosen.
// tests/c_abi/vcg_form_check.cpp holds all of it against the decision code it replaced.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>

namespace mfs {

constexpr size_t kVmMaxLds = 152 * 1024;          // the ring of plane buffers must fit the CU's LDS
constexpr size_t kVmTwoPerCuLds = 80 * 1024;      // up to here two workgroups share a CU; beyond it, one

// LDS of the march: a ring of `ring` plane slots, each the three components' images [Nz halo | tile | Nz halo] of a tile of
// `block` z-vectors of `vec` elements.  The kernel's vm_su / vm_lds_bytes (mfs_vcg_march.h) are these.
constexpr int vmarch_su(int vec, int block, int Nz) { return 2 * Nz + block * vec; }
constexpr size_t vmarch_lds_bytes(size_t elt, int vec, int block, int ring, int Nz) {
  return (size_t)ring * 3 * vmarch_su(vec, block, Nz) * elt;
}

// Geometry of the march on rows of Nz elements: threads per workgroup (= z-vectors per tile) and ring slots; block 0: rows
// too long.  256 x 4 wherever two such workgroups share a CU; 512 x 4 where only one 256-vector workgroup would fit anyway
// (fp64 from Nz ~ 150, fp32 from Nz ~ 300); 512 x 3 (a second barrier per plane) where even that ring exceeds the LDS.
// knob (MFS_VISC_MARCH_BLOCK, read at engine creation): 256 / 512 / 5123 force a geometry, anything else is automatic.
// ODDITY: a forced geometry that does not fit falls back to the automatic choice.
struct VMarchGeom { int block, ring; };
constexpr VMarchGeom vmarch_geom(size_t elt, int Nz, int knob) {
  const int vec = (int)(16 / elt), nzv2 = 2 * (Nz / vec);
  const bool f2564 = nzv2 <= 256 && vmarch_lds_bytes(elt, vec, 256, 4, Nz) <= kVmMaxLds;
  const bool f5124 = nzv2 <= 512 && vmarch_lds_bytes(elt, vec, 512, 4, Nz) <= kVmMaxLds;
  const bool f5123 = nzv2 <= 512 && vmarch_lds_bytes(elt, vec, 512, 3, Nz) <= kVmMaxLds;
  if (knob == 256 && f2564) return {256, 4};
  if (knob == 512 && f5124) return {512, 4};
  if (knob == 5123 && f5123) return {512, 3};
  if (f2564 && vmarch_lds_bytes(elt, vec, 256, 4, Nz) <= kVmTwoPerCuLds) return {256, 4};
  if (f5124) return {512, 4};
  if (f2564) return {256, 4};
  if (f5123) return {512, 3};
  return {0, 0};
}

struct VMarchInputs {
  size_t elt;                     // sizeof(T): 4 or 8 (whole 16-byte vectors: 4 or 2 elements)
  int Nx, Ny, Nz;
  int march, block_knob, march_bpc, compress, march_nt;      // the engine's knobs as stored
  int tw_block;                   // tile size the compressed class access' classes were built for (0: not built / none)
  bool aligned;                   // operand and result both 16-byte aligned
  bool masked;                    // tap masks wanted (initial q = A x, stand-alone apply)
  bool fused;                     // the caller asks for the fused form (direction and x update ride in the launch)
  int cus;
};

enum VApplyKind {
  kVApplyNone,       // a grid side < 2: nothing to compute
  kVApplyRows,       // degenerate grids: whichever boundary slabs exist, one k_vcg_apply_row launch each
  kVApplyAll,        // k_vcg_apply_all: the box and the three boundary slabs in one launch
  kVApplyMarch       // k_vcg_apply_march
};

struct VMarchForm {
  VApplyKind kind;
  // the grid has rows of whole vectors (classes exist), and its march geometry (block 0: none): set whatever `kind` is, for
  // vcg_build_classes / class_census / sparse_info
  bool rows_ok;
  int block, ring;
  size_t lds;                     // dynamic LDS bytes of the launch
  int bpc;                        // workgroups per CU
  int tiles;                      // tiles per plane
  int64_t total;                  // (tile, plane) pairs
  int gmain;                      // main grid (the boundary slabs' blocks come on top)
  // template arguments of the march (kind == kVApplyMarch)
  int nt;                         // 0 | 5
  bool comp, fuse;
  bool comp_wanted;               // the launch takes the compressed form once the classes are built for its tile size
};

// Nontemporal class loads / q stores once operand, result and classes (13 arrays) exceed the Infinity Cache; knob
// (MFS_VISC_MARCH_NT) 0 / 1 overrides, < 0 auto
constexpr bool vmarch_nt(int knob, size_t elt, int Nx, int Ny, int Nz) {
  return knob < 0 ? (13.0 * (double)Nx * Ny * Nz * (double)elt > 200e6) : (knob != 0);
}

inline void vmarch_form(const VMarchInputs& in, VMarchForm* out) {
  VMarchForm f{};
  const int vec = (int)(16 / in.elt);
  const int Nx = in.Nx, Ny = in.Ny, Nz = in.Nz;
  f.rows_ok = Nx >= 3 && Ny >= 3 && Nz % vec == 0 && Nz >= 2 * vec;
  if (f.rows_ok) {
    const VMarchGeom g = vmarch_geom(in.elt, Nz, in.block_knob);
    f.block = g.block; f.ring = g.ring;
  }
  if (f.block > 0) {
    const int ipp = (Ny - 2) * (Nz / vec);
    f.tiles = (ipp + f.block - 1) / f.block;
    f.total = (int64_t)f.tiles * (Nx - 2);
    f.lds = vmarch_lds_bytes(in.elt, vec, f.block, f.ring, Nz);
    f.bpc = f.lds > kVmTwoPerCuLds ? 1 : in.march_bpc;
    const int64_t cap = (int64_t)in.cus * f.bpc;
    f.gmain = (int)(f.total < cap ? (f.total < 1 ? 1 : f.total) : (cap < 1 ? 1 : cap));
  }
  // the march serves unmasked operands on rows of whole, 16-byte aligned vectors with 32-bit in-plane offsets
  const bool march = !in.masked && in.march != 0 && f.block > 0 && in.aligned &&
                     (int64_t)(Ny + 1) * (Nz + 4) <= (int64_t)0x7fffffff / 2;
  if (Nx < 2 || Ny < 2 || Nz < 2) f.kind = kVApplyNone;
  else if (march) f.kind = kVApplyMarch;
  else f.kind = (Nx >= 3 && Ny >= 3 && Nz >= 3) ? kVApplyAll : kVApplyRows;
  if (f.kind == kVApplyMarch) {
    f.nt = vmarch_nt(in.march_nt, in.elt, Nx, Ny, Nz) ? 5 : 0;
    // ODDITY: the 3-slot ring has no fused form: a fuse request there gets the plain march (and vloop_form the plain loop)
    f.fuse = in.fused && f.ring != 3;
    // ODDITY: the compressed form is taken only when the classes were built for the tile size the launch uses; the fused
    // form has no compressed class access
    f.comp_wanted = !f.fuse && in.compress != 0;
    f.comp = f.comp_wanted && in.tw_block > 0 && in.tw_block == f.block;
  }
  *out = f;
}

// The tuples (NT, FUSE, BLOCK, RING, COMP) vmarch_form can produce, the same for both dtypes: 12 unfused (NT x COMP x
// {256 x 4, 512 x 4, 512 x 3}) and 4 fused (NT x {256 x 4, 512 x 4})
constexpr bool vmarch_reachable(int nt, bool fuse, int block, int ring, bool comp) {
  if (nt != 0 && nt != 5) return false;
  if (!((block == 256 && ring == 4) || (block == 512 && (ring == 4 || ring == 3)))) return false;
  if (fuse) return ring == 4 && !comp;
  return true;
}

// each tuple packed into one integer, the reachable ones in ascending order: vcg_launch_march instantiates one kernel per
// entry and dtype and picks by code
struct VMarchTuple { int nt; bool fuse; int block, ring; bool comp; };
constexpr int kVMarchCodes = 1 << 5;
constexpr int vmarch_code(int nt, bool fuse, int block, int ring, bool comp) {
  return (int)(nt != 0) | (int)fuse << 1 | (int)(block == 512) << 2 | (int)(ring == 3) << 3 | (int)comp << 4;
}
constexpr VMarchTuple vmarch_decode(int c) {
  return VMarchTuple{(c & 1) ? 5 : 0, (c >> 1 & 1) != 0, (c >> 2 & 1) ? 512 : 256, (c >> 3 & 1) ? 3 : 4, (c >> 4 & 1) != 0};
}
constexpr bool vmarch_reachable(const VMarchTuple& t) { return vmarch_reachable(t.nt, t.fuse, t.block, t.ring, t.comp); }
constexpr int vmarch_count() {
  int n = 0;
  for (int c = 0; c < kVMarchCodes; ++c) n += vmarch_reachable(vmarch_decode(c));
  return n;
}
static_assert(vmarch_count() == 16, "the reachable set: 16 march forms per dtype");

constexpr std::array<int, vmarch_count()> vmarch_codes() {
  std::array<int, vmarch_count()> a{};
  int n = 0;
  for (int c = 0; c < kVMarchCodes; ++c)
    if (vmarch_reachable(vmarch_decode(c))) a[n++] = c;
  return a;
}

// ---------------------------------------------------------------- loop form -----
enum VLoopKind {
  kVLoopJacobiZ,       // opt-in Jacobi loop, z stored (aligned vectors, beyond the caches or MFS_VISC_JACOBI_Z = 1)
  kVLoopJacobi,        // opt-in Jacobi loop, partial sums folded by the consumers (aligned vectors)
  kVLoopJacobiScalar,  // opt-in Jacobi loop on misaligned vectors
  kVLoopFused,         // opt-in: direction and x update inside the march, 2 launches per iteration
  kVLoopResident,      // small grids: one resident launch per batch (mfs_vcg_resident.h)
  kVLoopMerged,        // small problems: both vector phases in one launch (k_update_rdx)
  kVLoopPlain          // stencil launch, r (+ x) update, direction update
};

struct VLoopInputs {
  bool bound, is_setup;           // x bound; mfs_vcg3d_setup called
  bool d_bound;                   // d bound
  bool vec_ok;                    // all five CG vectors 16-byte aligned (core_vec_ok)
  bool rdx_ok;                    // the merged vector-phase launch can serve the engine (core_rdx_ok)
  bool jacobi, fuse, split_x;     // knobs as stored
  int jacobi_z;                   // MFS_VISC_JACOBI_Z as read at creation: -1 auto, 0 / 1
  bool resident;                  // the resident loop is allowed (knob != 0)
  bool res_fits;                  // ... a plan exists, its tables are carved and the device has its workgroups' CUs
  bool p2p, skip_top_x;           // window attached; slab decomposition
  bool fuse_march;                // vmarch_form gives the fused march for d -> q as bound (looked at only when fuse is set)
  int64_t n;                      // unknowns
  size_t elt;
};

struct VLoopForm {
  VLoopKind kind;
  bool split_x;                   // kVLoopPlain: the x update rides in the direction update
  bool lists_begin, lists_slab;   // mfs_vcg3d_begin / mfs_vcg3d_slab_begin build the solve's sparse lists (vcg_build_live)
  int info;                       // mfs_vcg3d_loop_info: 1 fused | 2 merged | 4 Jacobi | 8 resident | 0 plain
};

inline VLoopForm vloop_form(const VLoopInputs& in) {
  VLoopForm f{};
  // the fused loop serves the reference's iteration with the x update split off, on aligned vectors, where the march has
  // a fused form for the engine as bound
  const bool fused = in.fuse && !in.jacobi && in.split_x && in.d_bound && in.vec_ok && in.fuse_march;
  // the resident loop: the reference's plain loop (no Jacobi, no fuse request, no slab form) on a grid that fits
  const bool resident = in.resident && in.res_fits && !in.jacobi && !in.fuse && !in.p2p && !in.skip_top_x && in.bound;
  if (in.jacobi) {
    // z stored pays beyond the caches; launch-bound sizes keep the form whose consumers fold the partial sums themselves
    const bool zform = in.jacobi_z < 0 ? (5.0 * (double)in.n * (double)in.elt > 100e6) : (in.jacobi_z != 0);
    f.kind = !in.vec_ok ? kVLoopJacobiScalar : zform ? kVLoopJacobiZ : kVLoopJacobi;
  } else if (fused) f.kind = kVLoopFused;
  else if (resident) f.kind = kVLoopResident;
  else if (in.rdx_ok && !in.p2p) f.kind = kVLoopMerged;
  else f.kind = kVLoopPlain;
  f.split_x = in.split_x;
  // single-domain, launch-per-phase loops and the Jacobi loop sweep live chunks only.
  // ODDITY: begin and slab_begin skip the lists whenever the fuse knob is set, even when the fused loop cannot serve the
  // engine and the plain loop then runs dense.
  f.lists_begin = !in.p2p && !in.skip_top_x && (in.jacobi || !in.fuse);
  f.lists_slab = !in.jacobi && !in.fuse;
  // ODDITY: loop_info on an engine not yet bound or set up says only whether the Jacobi knob is on (4 or 0)
  if (!in.bound || !in.is_setup) f.info = in.jacobi ? 4 : 0;
  else f.info = f.kind == kVLoopResident ? 8 : f.kind == kVLoopFused ? 1 : f.kind == kVLoopMerged ? 2 : in.jacobi ? 4 : 0;
  return f;
}

}  // namespace mfs
