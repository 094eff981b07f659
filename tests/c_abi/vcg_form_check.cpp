// vcg_form_check.cpp -- vmarch_form / vmarch_reachable / vloop_form (csrc/mfs_vcg_form.h) against the decision code they replaced.
//
// The old_* functions below are vcg_march_geom, vcg_march_ok, vcg_march_launch_blk / _nt, vcg_build_classes, vcg_march_launch,
// vcg_march_fused, vcg_apply_TM, vcg_apply, vcg_fuse_ok, vcg_resident_ok and the conditions of mfs_vcg3d_iterate, _loop_info,
// _begin, _slab_begin, _poll and _solve of mfs_visc.hip as they stood before the resolver, transcribed: same variables, same
// branches in the same order, every launch replaced by a `return` of the tuple it named, getenv by a field of the engine.
// The four knobs removed with the resolver (mask_cg, tiled, march_vec, merge_slabs) sit at their defaults 0, 0, 0, 1.
// It is the specification: do not tidy it.  Stand-alone (built by tests/test_vcg_form.py with the host compiler and
// -fsanitize=address,undefined); prints "ok ..." and exits 0, or says what differs and exits 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "mfs_vcg_form.h"

using namespace mfs;

namespace {

constexpr int MFS_F32 = 0, MFS_F64 = 1;
template <typename T> struct VecOf;
template <> struct VecOf<float> { static constexpr int N = 4; };
template <> struct VecOf<double> { static constexpr int N = 2; };
constexpr int MFS_VMARCH_MIN_WAVES = 2;

// ------------------------------------------------------------------ the specification: do not tidy it ----
struct OldCore { bool x, d; uintptr_t dp, qp; int cus; bool vec_ok, rdx_ok; size_t elt; };
struct OldPlan { bool ok; int W; };
struct OldCompact { int tw_block, seg_g; };
struct OldEngine {
  struct { int N[3]; } g;
  int dt;
  long long n;
  OldCore c;
  OldCompact cp;
  bool is_setup;
  int mask_cg, tiled, merge_slabs, march_vec;      // removed knobs: 0, 0, 1, 0
  int split_x, skip_top_x, march, march_bpc;
  bool p2p;
  int jacobi, resident;
  OldPlan res;
  bool res_ar;
  bool classes_ready;
  int compress, march_nt, fuse;
  int env_march_block;      // getenv("MFS_VISC_MARCH_BLOCK"), 0 when unset
  int env_jacobi_z;         // getenv("MFS_VISC_JACOBI_Z"), -1 when unset
  int built_G;              // G of the cost-balanced cut vcg_build_classes computed (-1: none)
};

template <int VEC, int BLOCK>
int old_vm_su(int Nz) { return 2 * Nz + BLOCK * VEC; }
template <typename T, int VEC, int BLOCK, int RING>
size_t old_vm_lds_bytes(int Nz) { return (size_t)RING * 3 * old_vm_su<VEC, BLOCK>(Nz) * sizeof(T); }

constexpr size_t old_kVmMaxLds = 152 * 1024;
constexpr int old_kVmMaxSegs = 4096;

template <typename T, int VEC>
int old_vcg_march_geom(const OldEngine* h) {
  const int Nz = h->g.N[2], nzv2 = 2 * (Nz / VEC);
  const int knob = h->env_march_block;
  const bool f2564 = nzv2 <= 256 && old_vm_lds_bytes<T, VEC, 256, 4>(Nz) <= old_kVmMaxLds;
  const bool f5124 = nzv2 <= 512 && old_vm_lds_bytes<T, VEC, 512, 4>(Nz) <= old_kVmMaxLds;
  const bool f5123 = nzv2 <= 512 && old_vm_lds_bytes<T, VEC, 512, 3>(Nz) <= old_kVmMaxLds;
  if (knob == 256 && f2564) return 2564;
  if (knob == 512 && f5124) return 5124;
  if (knob == 5123 && f5123) return 5123;
  if (f2564 && old_vm_lds_bytes<T, VEC, 256, 4>(Nz) <= 80 * 1024) return 2564;
  if (f5124) return 5124;
  if (f2564) return 2564;
  if (f5123) return 5123;
  return 0;
}

template <typename T, int VEC = VecOf<T>::N>
bool old_vcg_march_ok(const OldEngine* h, uintptr_t v, uintptr_t out) {
  const int Nx = h->g.N[0], Ny = h->g.N[1], Nz = h->g.N[2];
  if (!h->march || Nx < 3 || Ny < 3 || Nz % VEC != 0 || Nz < 2 * VEC) return false;
  if (old_vcg_march_geom<T, VEC>(h) == 0) return false;
  if ((v % 16) != 0 || (out % 16) != 0) return false;
  if ((int64_t)(Ny + 1) * (Nz + 4) > (int64_t)0x7fffffff / 2) return false;
  return true;
}

struct Tuple {
  int kind;                       // 0 nothing | 1 per-row launches | 2 k_vcg_apply_all | 3 k_vcg_apply_march
  int nt; bool fuse; int block, ring; bool comp;
  size_t lds; int bpc, gmain;
};

template <typename T, int VEC, int WAVES, int NT, bool FUSE = false, int BLOCK = 256, int RING = 4, bool COMP = false>
Tuple old_vcg_march_launch_blk(OldEngine* h) {
  const int Nx = h->g.N[0], Ny = h->g.N[1], Nz = h->g.N[2];
  const int ipp = (Ny - 2) * (Nz / VEC), tiles = (ipp + BLOCK - 1) / BLOCK;
  const int64_t total = (int64_t)tiles * (Nx - 2);
  const size_t lds = old_vm_lds_bytes<T, VEC, BLOCK, RING>(Nz);
  const int bpc = lds > 80 * 1024 ? 1 : h->march_bpc;
  const int gmain = (int)std::max<int64_t>(1, std::min<int64_t>(total, (int64_t)h->c.cus * bpc));
  return Tuple{3, NT, FUSE, BLOCK, RING, COMP, lds, bpc, gmain};
}

template <typename T, int VEC, int WAVES, int NT, bool FUSE = false, bool COMP = false>
Tuple old_vcg_march_launch_nt(OldEngine* h) {
  if constexpr (VEC == VecOf<T>::N && WAVES == MFS_VMARCH_MIN_WAVES) {
    const int geom = old_vcg_march_geom<T, VEC>(h);
    if (geom == 5124) return old_vcg_march_launch_blk<T, VEC, WAVES, NT, FUSE, 512, 4, COMP>(h);
    if constexpr (!FUSE) {
      if (geom == 5123) return old_vcg_march_launch_blk<T, VEC, WAVES, NT, FUSE, 512, 3, COMP>(h);
    }
  }
  return old_vcg_march_launch_blk<T, VEC, WAVES, NT, FUSE, 256, 4, COMP>(h);
}

void old_vcg_build_classes(OldEngine* h) {
  const int Nx = h->g.N[0], Ny = h->g.N[1], Nz = h->g.N[2];
  h->classes_ready = true;
  h->cp.tw_block = 0;
  h->cp.seg_g = 0;
  h->built_G = -1;
  if (Nx >= 3 && Ny >= 3) {
    const int vec = h->dt == MFS_F32 ? 4 : 2;
    if (Nz % vec == 0 && Nz >= 2 * vec) {
      const int geom = h->dt == MFS_F32 ? old_vcg_march_geom<float, 4>(h) : old_vcg_march_geom<double, 2>(h);
      h->cp.tw_block = geom / 10;
      if (h->cp.tw_block > 0) {
        const int ipp = (Ny - 2) * (Nz / vec), tiles = (ipp + h->cp.tw_block - 1) / h->cp.tw_block;
        const size_t ldsb = h->dt == MFS_F32 ? (size_t)(geom % 10) * 3 * (2 * Nz + h->cp.tw_block * 4) * 4
                                             : (size_t)(geom % 10) * 3 * (2 * Nz + h->cp.tw_block * 2) * 8;
        const int bpc = ldsb > 80 * 1024 ? 1 : h->march_bpc;
        const int64_t total = (int64_t)tiles * (Nx - 2);
        const int G = (int)std::max<int64_t>(1, std::min<int64_t>(total, (int64_t)h->c.cus * bpc));
        h->built_G = G;
        h->cp.seg_g = 0;
        if (G <= old_kVmMaxSegs && total < 0x7fffffff) h->cp.seg_g = G;
      }
    }
  }
}

template <typename T, int VEC, int WAVES>
Tuple old_vcg_march_launch(OldEngine* h) {
  const int knob = h->march_nt;
  const bool nt = knob < 0 ? (13.0 * (double)h->g.N[0] * h->g.N[1] * h->g.N[2] * sizeof(T) > 200e6) : (knob != 0);
  if constexpr (VEC == VecOf<T>::N && WAVES == MFS_VMARCH_MIN_WAVES) {
    if (h->compress && !h->classes_ready) old_vcg_build_classes(h);
    if (h->compress && h->cp.tw_block > 0 && h->cp.tw_block == old_vcg_march_geom<T, VEC>(h) / 10)
      return nt ? old_vcg_march_launch_nt<T, VEC, WAVES, 5, false, true>(h)
                : old_vcg_march_launch_nt<T, VEC, WAVES, 0, false, true>(h);
  }
  return nt ? old_vcg_march_launch_nt<T, VEC, WAVES, 5>(h)
            : old_vcg_march_launch_nt<T, VEC, WAVES, 0>(h);
}

template <typename T>
Tuple old_vcg_march_fused(OldEngine* h) {
  constexpr int VEC = VecOf<T>::N;
  const int knob = h->march_nt;
  const bool nt = knob < 0 ? (13.0 * (double)h->g.N[0] * h->g.N[1] * h->g.N[2] * sizeof(T) > 200e6) : (knob != 0);
  return nt ? old_vcg_march_launch_nt<T, VEC, MFS_VMARCH_MIN_WAVES, 5, true>(h)
            : old_vcg_march_launch_nt<T, VEC, MFS_VMARCH_MIN_WAVES, 0, true>(h);
}

template <typename T, bool MASK>
Tuple old_vcg_apply_TM(OldEngine* h, uintptr_t v, uintptr_t out) {
  const int Nx = h->g.N[0], Ny = h->g.N[1], Nz = h->g.N[2];
  if constexpr (sizeof(T) == 4) if (!MASK && !h->tiled && h->march_vec == 2 && old_vcg_march_ok<T, 2>(h, v, out))
    return old_vcg_march_launch<T, 2, 3>(h);
  if (!MASK && !h->tiled && old_vcg_march_ok<T>(h, v, out))
    return old_vcg_march_launch<T, VecOf<T>::N, MFS_VMARCH_MIN_WAVES>(h);
  if (Nx >= 3 && Ny >= 3 && Nz >= 3) {
    if (!MASK && h->tiled) {
      return Tuple{-1, 0, false, 0, 0, false, 0, 0, 0};        // k_vcg_apply_tiled: removed, unreachable at tiled = 0
    } else if (h->merge_slabs != 0) {
      return Tuple{2, 0, false, 0, 0, false, 0, 0, 0};         // k_vcg_apply_all
    } else {
      return Tuple{-1, 0, false, 0, 0, false, 0, 0, 0};        // k_vcg_apply_fused + k_vcg_apply_slabs: removed
    }
  }
  return Tuple{1, 0, false, 0, 0, false, 0, 0, 0};             // degenerate grids: k_vcg_apply_row launches
}

Tuple old_vcg_apply(OldEngine* h, uintptr_t v, uintptr_t out, bool masked) {
  if (h->g.N[0] < 2 || h->g.N[1] < 2 || h->g.N[2] < 2) return Tuple{0, 0, false, 0, 0, false, 0, 0, 0};
  if (h->dt == MFS_F32)
    return masked ? old_vcg_apply_TM<float, true>(h, v, out) : old_vcg_apply_TM<float, false>(h, v, out);
  return masked ? old_vcg_apply_TM<double, true>(h, v, out) : old_vcg_apply_TM<double, false>(h, v, out);
}

int old_apply_kernel(const OldEngine* h) {
  if (h->tiled) return 1;
  const uintptr_t d = h->c.d ? h->c.dp : 0, q = h->c.d ? h->c.qp : 0;
  const bool ok = h->dt == MFS_F32 ? old_vcg_march_ok<float>(h, d, q) : old_vcg_march_ok<double>(h, d, q);
  return ok ? 2 : 0;
}

bool old_core_vec_ok(const OldCore& c) { return c.vec_ok; }
bool old_core_rdx_ok(const OldCore& c) { return c.rdx_ok; }

bool old_vcg_fuse_ok(const OldEngine* h) {
  if ((h->dt == MFS_F32 ? old_vcg_march_geom<float, 4>(h) : old_vcg_march_geom<double, 2>(h)) % 10 == 3) return false;
  if (!h->fuse || h->jacobi || !h->split_x || h->mask_cg || h->tiled || h->march_vec == 2 || !h->c.d || !old_core_vec_ok(h->c)) return false;
  return h->dt == MFS_F32 ? old_vcg_march_ok<float>(h, h->c.dp, h->c.qp) : old_vcg_march_ok<double>(h, h->c.dp, h->c.qp);
}

bool old_vcg_resident_ok(const OldEngine* h) {
  return h->resident != 0 && h->res.ok && h->res_ar && !h->jacobi && !h->fuse && !h->mask_cg && !h->p2p && !h->skip_top_x &&
         h->c.x && h->c.cus >= h->res.W;
}

// mfs_vcg3d_iterate: which loop body runs (the VLoopKind it corresponds to), and for the plain one whether split_x
struct OldLoop { int kind; bool split_x; };
OldLoop old_iterate(const OldEngine* h) {
  if (h->jacobi) {
    const bool vec = old_core_vec_ok(h->c);
    const int zk = h->env_jacobi_z;
    const bool zform = zk < 0 ? (5.0 * (double)h->n * h->c.elt > 100e6) : (zk != 0);
    if (vec && zform) return {kVLoopJacobiZ, false};
    else if (vec) return {kVLoopJacobi, false};
    else return {kVLoopJacobiScalar, false};
  }
  if (old_vcg_fuse_ok(h)) return {kVLoopFused, false};
  if (old_vcg_resident_ok(h)) return {kVLoopResident, false};
  const bool rdx = old_core_rdx_ok(h->c) && !h->p2p;
  if (rdx) return {kVLoopMerged, false};
  if (h->split_x) return {kVLoopPlain, true};
  else return {kVLoopPlain, false};
}

int old_loop_info(const OldEngine* h) {
  if (!h->c.x || !h->is_setup) return h->jacobi ? 4 : 0;
  if (old_vcg_resident_ok(h)) return 8;
  return (old_vcg_fuse_ok(h) ? 1 : 0) | ((!h->jacobi && !old_vcg_fuse_ok(h) && old_core_rdx_ok(h->c) && !h->p2p) ? 2 : 0) | (h->jacobi ? 4 : 0);
}

// mfs_vcg3d_begin: does it reach vcg_build_live?
bool old_begin_lists(const OldEngine* h) {
  if (h->jacobi) {
    if (h->p2p || h->skip_top_x) return false;
    return true;
  }
  return (h->p2p || h->skip_top_x || h->fuse) ? false : true;
}
// mfs_vcg3d_slab_begin
bool old_slab_begin_lists(const OldEngine* h) {
  if (h->jacobi) return false;
  return h->fuse ? false : true;
}
// mfs_vcg3d_poll after a take-back: true switches the resident loop off, false the merged phases
bool old_poll_switches_resident(const OldEngine* h) { return old_vcg_resident_ok(h); }
// mfs_vcg3d_solve: the resident predicate of core_solve_batched
bool old_solve_resident(const OldEngine* h) { return old_vcg_resident_ok(h); }
// ------------------------------------------------------------------ end of the specification ----

int fails = 0;
void fail(const char* what, const OldEngine& h, bool aligned, bool masked, bool fused, const Tuple& o, const VMarchForm& f) {
  if (++fails > 20) return;
  std::printf("MISMATCH %s: dt %d N %dx%dx%d march %d knob %d bpc %d compress %d nt %d tw %d ready %d cus %d aligned %d masked %d fused %d\n"
              "  old: kind %d <%d,%d,%d,%d,%d> lds %zu bpc %d gmain %d\n  new: kind %d <%d,%d,%d,%d,%d> lds %zu bpc %d gmain %d\n",
              what, h.dt, h.g.N[0], h.g.N[1], h.g.N[2], h.march, h.env_march_block, h.march_bpc, h.compress, h.march_nt,
              h.cp.tw_block, h.classes_ready, h.c.cus, aligned, masked, fused, o.kind, o.nt, o.fuse, o.block, o.ring, o.comp, o.lds,
              o.bpc, o.gmain, (int)f.kind, f.nt, f.fuse, f.block, f.ring, f.comp, f.lds, f.bpc, f.gmain);
}

VMarchInputs inputs_of(const OldEngine& h, bool aligned, bool masked, bool fused) {
  VMarchInputs in{};
  in.elt = h.dt == MFS_F32 ? 4 : 8;
  in.Nx = h.g.N[0]; in.Ny = h.g.N[1]; in.Nz = h.g.N[2];
  in.march = h.march; in.block_knob = h.env_march_block; in.march_bpc = h.march_bpc; in.compress = h.compress;
  in.march_nt = h.march_nt; in.tw_block = h.cp.tw_block; in.aligned = aligned; in.masked = masked; in.fused = fused;
  in.cus = h.c.cus;
  return in;
}

std::set<int> produced;
long long cases = 0;

// one stencil launch, old against new.  fused: the launch of fused iteration j >= 1 (the loop asked vcg_fuse_ok first)
void check_launch(OldEngine h, bool aligned, bool masked, bool fused) {
  ++cases;
  const uintptr_t v = aligned ? 0x1000 : 0x1004, out = 0x2000;
  OldEngine ho = h;
  Tuple o;
  bool old_fused = false;
  if (fused) {
    // what mfs_vcg3d_iterate did with a fuse request on d -> q: the fused march where vcg_fuse_ok's march conditions hold
    ho.c.d = true; ho.c.dp = v; ho.c.qp = out;
    const int geom = ho.dt == MFS_F32 ? old_vcg_march_geom<float, 4>(&ho) : old_vcg_march_geom<double, 2>(&ho);
    old_fused = !masked && geom % 10 != 3 &&
                (ho.dt == MFS_F32 ? old_vcg_march_ok<float>(&ho, v, out) : old_vcg_march_ok<double>(&ho, v, out));
    if (ho.g.N[0] < 2 || ho.g.N[1] < 2 || ho.g.N[2] < 2) old_fused = false;
  }
  if (old_fused) o = ho.dt == MFS_F32 ? old_vcg_march_fused<float>(&ho) : old_vcg_march_fused<double>(&ho);
  else o = old_vcg_apply(&ho, v, out, masked);
  // the new launch site: resolve; build the classes where the form wants them and they are missing; resolve again
  OldEngine hn = h;
  VMarchForm f{};
  vmarch_form(inputs_of(hn, aligned, masked, fused), &f);
  int new_G = -1;
  if (f.kind == kVApplyMarch && f.comp_wanted && !hn.classes_ready) {
    hn.classes_ready = true;
    hn.cp.tw_block = f.rows_ok ? f.block : 0;
    new_G = f.block > 0 ? f.gmain : -1;
    vmarch_form(inputs_of(hn, aligned, masked, fused), &f);
  }
  const int kind = f.kind == kVApplyNone ? 0 : f.kind == kVApplyRows ? 1 : f.kind == kVApplyAll ? 2 : 3;
  if (o.kind < 0) { fail("old tree reached a removed kernel", h, aligned, masked, fused, o, f); return; }
  if (kind != o.kind) { fail("kind", h, aligned, masked, fused, o, f); return; }
  if (ho.classes_ready != hn.classes_ready || ho.cp.tw_block != hn.cp.tw_block)
    fail("classes built / tile size", h, aligned, masked, fused, o, f);
  if (ho.classes_ready && !h.classes_ready && ho.built_G != new_G) fail("grid of the cost-balanced cut", h, aligned, masked, fused, o, f);
  if (kind != 3) return;
  if (o.nt != f.nt || o.fuse != f.fuse || o.block != f.block || o.ring != f.ring || o.comp != f.comp || o.lds != f.lds ||
      o.bpc != f.bpc || o.gmain != f.gmain)
    fail("tuple", h, aligned, masked, fused, o, f);
  if (fused && !old_fused && f.fuse) fail("fused form where the old loop had none", h, aligned, masked, fused, o, f);
  if (f.lds > kVmMaxLds) fail("LDS beyond the CU's", h, aligned, masked, fused, o, f);
  if (!vmarch_reachable(f.nt, f.fuse, f.block, f.ring, f.comp)) fail("produced but not reachable", h, aligned, masked, fused, o, f);
  const int code = vmarch_code(f.nt, f.fuse, f.block, f.ring, f.comp);
  const VMarchTuple t = vmarch_decode(code);
  if (t.nt != f.nt || t.fuse != f.fuse || t.block != f.block || t.ring != f.ring || t.comp != f.comp)
    fail("code does not decode to the tuple", h, aligned, masked, fused, o, f);
  produced.insert(code);
}

OldEngine base_engine(int dt, int Nx, int Ny, int Nz) {
  OldEngine h{};
  h.g.N[0] = Nx; h.g.N[1] = Ny; h.g.N[2] = Nz;
  h.dt = dt;
  h.n = (long long)(Nx + 1) * Ny * Nz + (long long)Nx * (Ny + 1) * Nz + (long long)Nx * Ny * (Nz + 1);
  h.c.elt = dt == MFS_F32 ? 4 : 8;
  h.c.cus = 256;
  h.merge_slabs = 1;
  h.split_x = 1; h.march = 1; h.march_bpc = 2; h.compress = 1; h.march_nt = -1;
  h.env_march_block = 0; h.env_jacobi_z = -1;
  h.built_G = -1;
  return h;
}

}  // namespace

int main() {
  const int knobs[5] = {0, 256, 512, 5123, 77};
  // ---- 1. the geometry function alone: both dtypes x every Nz in 1 .. 1200 x every block knob value
  std::vector<int> nzs[2];
  for (int dt = 0; dt < 2; ++dt) {
    int prev[5] = {-1, -1, -1, -1, -1};
    bool prev_two = false;
    for (int Nz = 1; Nz <= 1200; ++Nz) {
      bool edge = false;
      for (int k = 0; k < 5; ++k) {
        OldEngine h = base_engine(dt, 8, 8, Nz);
        h.env_march_block = knobs[k];
        const int geom = dt == MFS_F32 ? old_vcg_march_geom<float, 4>(&h) : old_vcg_march_geom<double, 2>(&h);
        const VMarchGeom g = vmarch_geom(h.c.elt, Nz, knobs[k]);
        ++cases;
        if (g.block * 10 + g.ring != geom) {
          if (++fails <= 20) std::printf("MISMATCH geometry: dt %d Nz %d knob %d old %d new %d x %d\n", dt, Nz, knobs[k], geom, g.block, g.ring);
        }
        if (g.block > 0) {
          const size_t elt = h.c.elt;
          const int vec = (int)(16 / elt);
          const size_t hand = dt == MFS_F32 ? (size_t)(geom % 10) * 3 * (2 * Nz + g.block * 4) * 4 : (size_t)(geom % 10) * 3 * (2 * Nz + g.block * 2) * 8;
          if (vmarch_lds_bytes(elt, vec, g.block, g.ring, Nz) != hand && ++fails <= 20) std::printf("MISMATCH LDS bytes: dt %d Nz %d\n", dt, Nz);
        }
        if (Nz > 1 && geom != prev[k]) edge = true;
        prev[k] = geom;
      }
      const bool two = vmarch_lds_bytes(dt ? 8 : 4, dt ? 2 : 4, 256, 4, Nz) <= 80 * 1024;
      if (Nz > 1 && two != prev_two) edge = true;
      prev_two = two;
      if (edge || Nz <= 10 || Nz % 97 == 0 || Nz == 1200)
        for (int d = -2; d <= 2; ++d)
          if (Nz + d >= 1 && Nz + d <= 1200) nzs[dt].push_back(Nz + d);
    }
    std::sort(nzs[dt].begin(), nzs[dt].end());
    nzs[dt].erase(std::unique(nzs[dt].begin(), nzs[dt].end()), nzs[dt].end());
  }
  // ---- 2. the launch tree over the full product
  const int sides[4] = {1, 2, 3, 5};
  for (int dt = 0; dt < 2; ++dt)
  for (int Nz : nzs[dt])
  for (int pair = 0; pair < 17; ++pair)             // Nx, Ny in {1, 2, 3, 5}; one pair that crosses the 200 MB rule with Nz
  for (int march = 0; march < 2; ++march)
  for (int compress = 0; compress < 2; ++compress)
  for (int cls = 0; cls < 3; ++cls)                 // classes not built | built for 256 | built for 512
  for (int nt = -1; nt <= 1; ++nt)
  for (int k = 0; k < 5; ++k)
  for (int flags = 0; flags < 8; ++flags) {
    const int Nx = pair < 16 ? sides[pair / 4] : 512, Ny = pair < 16 ? sides[pair % 4] : 512;
    OldEngine h = base_engine(dt, Nx, Ny, Nz);
    h.march = march; h.compress = compress; h.march_nt = nt; h.env_march_block = knobs[k];
    h.march_bpc = (Nz & 1) ? 1 : 2;
    h.c.cus = pair == 16 ? 256 : 3;                 // small grids: total pairs on both sides of cus x bpc
    h.classes_ready = cls != 0; h.cp.tw_block = cls == 1 ? 256 : cls == 2 ? 512 : 0;
    check_launch(h, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0);
  }
  std::set<int> reach;
  for (int c : vmarch_codes()) reach.insert(c);
  for (int c = 0; c < kVMarchCodes; ++c) {
    const VMarchTuple t = vmarch_decode(c);
    if (vmarch_reachable(t) != (reach.count(c) != 0)) { ++fails; std::printf("MISMATCH table and vmarch_reachable at code %d\n", c); }
  }
  if (reach != produced || (int)reach.size() != vmarch_count()) {
    ++fails;
    std::printf("MISMATCH reachable set: %zu in the table, %zu produced\n", reach.size(), produced.size());
  }
  // ---- 3. the loop form over every combination of the loop knobs, on grids where the fused march exists / does not
  struct Grid { int dt, Nx, Ny, Nz, march; };
  const Grid grids[7] = {{MFS_F32, 12, 40, 32, 1}, {MFS_F32, 12, 40, 33, 1}, {MFS_F64, 6, 10, 512, 1}, {MFS_F64, 10, 14, 256, 1},
                         {MFS_F32, 12, 40, 32, 0}, {MFS_F64, 2, 5, 8, 1}, {MFS_F32, 512, 512, 512, 1}};
  std::set<int> loops;
  for (const Grid& gr : grids)
  for (int b = 0; b < (1 << 13); ++b)
  for (int resident = -1; resident <= 1; ++resident)
  for (int zk = -1; zk <= 1; ++zk)
  for (int al = 0; al < 3; ++al) {                  // all five vectors aligned | b misaligned | d misaligned
    OldEngine h = base_engine(gr.dt, gr.Nx, gr.Ny, gr.Nz);
    h.march = gr.march;
    h.jacobi = b & 1; h.fuse = (b >> 1) & 1; h.split_x = (b >> 2) & 1; h.p2p = (b >> 3) & 1; h.skip_top_x = (b >> 4) & 1;
    h.c.rdx_ok = (b >> 5) & 1; h.res.ok = (b >> 6) & 1; h.res_ar = (b >> 7) & 1; h.res.W = 64; h.c.cus = ((b >> 8) & 1) ? 256 : 32;
    h.c.x = (b >> 9) & 1; h.c.d = (b >> 10) & 1; h.is_setup = (b >> 11) & 1;
    if ((b >> 12) & 1) h.n = 64;                    // n on both sides of the z form's size rule
    h.resident = resident; h.env_jacobi_z = zk;
    h.c.vec_ok = al == 0; h.c.dp = al == 2 ? 0x1008 : 0x1000; h.c.qp = 0x2000;
    if (h.c.rdx_ok && !h.c.vec_ok) continue;        // core_rdx_ok needs core_vec_ok and a bound x
    if (h.c.rdx_ok && !h.c.x) continue;
    ++cases;
    VLoopInputs in{};
    in.bound = h.c.x; in.is_setup = h.is_setup; in.d_bound = h.c.d; in.vec_ok = h.c.vec_ok; in.rdx_ok = h.c.rdx_ok;
    in.jacobi = h.jacobi != 0; in.fuse = h.fuse != 0; in.split_x = h.split_x != 0; in.jacobi_z = zk;
    in.resident = h.resident != 0; in.res_fits = h.res.ok && h.res_ar && h.c.cus >= h.res.W;
    in.p2p = h.p2p; in.skip_top_x = h.skip_top_x != 0; in.n = h.n; in.elt = h.c.elt;
    if (in.fuse) {                                  // as vcg_loop_form (mfs_visc.hip) fills it
      VMarchForm mf{};
      vmarch_form(inputs_of(h, h.c.dp % 16 == 0 && h.c.qp % 16 == 0, false, true), &mf);
      in.fuse_march = mf.kind == kVApplyMarch && mf.fuse;
    }
    const VLoopForm f = vloop_form(in);
    const OldLoop o = old_iterate(&h);
    bool bad = o.kind != (int)f.kind || (o.kind == kVLoopPlain && o.split_x != f.split_x);
    bad = bad || old_loop_info(&h) != f.info;
    bad = bad || old_begin_lists(&h) != f.lists_begin || old_slab_begin_lists(&h) != f.lists_slab;
    bad = bad || old_poll_switches_resident(&h) != (f.kind == kVLoopResident) || old_solve_resident(&h) != (f.kind == kVLoopResident);
    // mfs_vcg3d_apply_kernel: the march for d -> q as bound
    VMarchForm af{};
    const bool dal = !h.c.d || (h.c.dp % 16 == 0 && h.c.qp % 16 == 0);
    vmarch_form(inputs_of(h, dal, false, false), &af);
    bad = bad || old_apply_kernel(&h) != (af.kind == kVApplyMarch ? 2 : 0);
    if (bad && ++fails <= 20)
      std::printf("MISMATCH loop: grid %dx%dx%d dt %d bits %x resident %d zk %d al %d: old kind %d split %d info %d lists %d/%d, "
                  "new kind %d split %d info %d lists %d/%d\n", gr.Nx, gr.Ny, gr.Nz, gr.dt, b, resident, zk, al, o.kind, o.split_x,
                  old_loop_info(&h), old_begin_lists(&h), old_slab_begin_lists(&h), (int)f.kind, f.split_x, f.info, f.lists_begin, f.lists_slab);
    loops.insert((int)f.kind * 2 + (f.kind == kVLoopPlain && f.split_x));
  }
  if (fails) { std::printf("FAILED: %d mismatches in %lld cases\n", fails, cases); return 1; }
  std::printf("ok %lld cases, %zu march forms, %zu loop forms\n", cases, produced.size(), loops.size());
  return 0;
}
