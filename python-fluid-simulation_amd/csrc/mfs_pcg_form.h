// mfs_pcg_form.h -- which instantiation of k_pcg_apply_march (mfs_pcg_apply.h) a stencil launch of the pressure engine takes.
//
// Plain C++17, no HIP: march_form() is the ONE place where the engine's knobs, the grid and the caller's fused request
// become the kernel's template arguments, and march_reachable() is the table of the tuples that can come out of it --
// launch_apply_v (mfs_pcg.hip) instantiates exactly those.  tests/c_abi/pcg_form_check.cpp holds both against the
// decision tree they replaced, over every input.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>

namespace mfs {

constexpr int kMarchBlock = 256;                  // threads of a march workgroup (= kApplyBlock)
constexpr size_t kMarchLdsMax = 64 * 1024;        // a longer LDS image: the march without it

// what the caller asks to ride in the launch: nothing | d = r + beta d_old | ... and the previous iteration's x update |
// ... and the previous iteration's bookkeeping (FuseArgs / BookArgs)
enum MarchFused { kFusedNone = 0, kFused = 1, kFusedXdef = 2, kFusedBook = 3, kFusedXdefBook = 4 };

struct MarchInputs {
  int variant, nt, nt_auto, compress, pd;         // the engine's knobs as stored (mfs_pcg3d_tune, _set_compress, _set_prefetch)
  bool asym, lane_mask;                           // density operator; the latest poll's lane-mask decision
  bool vec;                                       // VEC > 1: whole 16-byte vectors along z
  size_t elt;                                     // sizeof(T)
  int64_t n;                                      // cells of the grid
  int Nz;
  bool has_list, list_range;                      // the solve built a work list; the launch is one range and it is the list's
  int fused;                                      // MarchFused
};

// template arguments of k_pcg_apply_march after <T, VEC>, plus: direct (k_pcg_apply_direct instead, nothing else set) and
// listed (the launch carries the work list)
struct MarchForm {
  bool direct, lds;
  int nt;
  bool comp, fuse;
  int pd;
  bool asym, xdef, book, lmask, listed;
};

// a fused request needs whole vectors (kFormNeedsVec) and the LDS march (kFormNeedsLds)
enum { kFormOk = 0, kFormNeedsLds = 1, kFormNeedsVec = 2 };

// dynamic LDS of the LDS march: two images of a tile's operand row with its halos
constexpr size_t march_lds_bytes(bool vec, size_t elt, int Nz) {
  return 2 * ((size_t)kMarchBlock * (vec ? 16 / elt : 1) + 2 * (size_t)Nz) * elt;
}

inline int march_form(const MarchInputs& in, MarchForm* out) {
  MarchForm f{};
  const bool fused = in.fused != kFusedNone;
  if (fused && !in.vec) return kFormNeedsVec;
  int variant = in.asym ? (in.variant > 1 ? in.variant : 1) : in.variant;
  if (variant >= 2 && march_lds_bytes(in.vec, in.elt, in.Nz) > kMarchLdsMax) variant = 1;      // absurdly long rows
  if (variant == 0) { f.direct = true; *out = f; return kFormOk; }
  if (variant == 1 && fused) return kFormNeedsLds;
  f.lds = variant >= 2;
  f.asym = in.asym;
  f.comp = f.lds && in.compress != 0 && in.vec;
  f.fuse = fused;
  f.xdef = in.fused == kFusedXdef || in.fused == kFusedXdefBook;
  f.book = in.fused == kFusedBook || in.fused == kFusedXdefBook;
  const bool rider = f.xdef || f.book;
  // Nontemporal loads for the once-read coefficient streams pay off only when the apply's working set (6 arrays) cannot
  // sit in the 256 MiB Infinity Cache anyway; below that, default caching lets the next iteration hit on-die.  nt < 0 = auto.
  // bit 0: diag, cz   bit 1: cx   bit 2: cy.  Partial masks (A-B of the hints) exist on the dense plain symmetric march
  // only, at prefetch depth 1: 1, 3 and 5 as given, every other one as 7.
  const int nt = in.nt < 0 ? ((6.0 * (double)in.n * (double)in.elt > 200e6) ? in.nt_auto : 0) : (in.nt & 7);
  const bool partial = f.lds && !f.comp && !f.fuse && !f.asym && nt != 0 && nt != 7;
  f.nt = nt == 0 ? 0 : !f.lds ? 1 : (partial && (nt == 1 || nt == 3 || nt == 5)) ? nt : 7;
  f.pd = (f.lds && in.pd >= 2 && !in.asym && !rider && !partial) ? 2 : 1;
  // sparse work list: the fused launches of the loop visit only (tile, plane) pairs that compute anything
  f.listed = fused && in.has_list && in.compress != 0 && in.vec && in.list_range && f.lds;
  f.lmask = f.comp && f.listed && in.lane_mask && rider;
  *out = f;
  return kFormOk;
}

// the tuples march_form can produce: 67 with whole vectors, 13 of them on the scalar path (no compression, nothing fused)
constexpr bool march_reachable(bool vec, bool lds, int nt, bool comp, bool fuse, int pd, bool asym, bool xdef, bool book,
                               bool lmask) {
  if (pd != 1 && pd != 2) return false;
  if (!lds) return !comp && !fuse && pd == 1 && !xdef && !book && !lmask && (nt == 0 || nt == 1);
  if (!vec && (comp || fuse)) return false;
  if ((xdef || book || lmask) && !fuse) return false;
  if (xdef || book) return pd == 1 && (nt == 0 || nt == 7) && (!lmask || comp);
  if (lmask) return false;
  if (!comp && !fuse && !asym && pd == 1) return nt == 0 || nt == 1 || nt == 3 || nt == 5 || nt == 7;
  return (nt == 0 || nt == 7) && (pd == 1 || !asym);
}

// The reachable tuples as a table: each packed into one integer (march_code), in ascending order.  launch_apply_v
// (mfs_pcg.hip) instantiates one kernel per entry and picks by code; a new kernel form is a new line in march_reachable.
constexpr int kMarchCodes = 1 << 11;
constexpr int march_code(const MarchForm& f) {
  return (int)f.lds | f.nt << 1 | (int)f.comp << 4 | (int)f.fuse << 5 | (int)(f.pd == 2) << 6 | (int)f.asym << 7 |
         (int)f.xdef << 8 | (int)f.book << 9 | (int)f.lmask << 10;
}
constexpr MarchForm march_decode(int c) {
  return MarchForm{false, (c & 1) != 0, (c >> 1) & 7, (c >> 4 & 1) != 0, (c >> 5 & 1) != 0, (c >> 6 & 1) ? 2 : 1,
                   (c >> 7 & 1) != 0, (c >> 8 & 1) != 0, (c >> 9 & 1) != 0, (c >> 10 & 1) != 0, false};
}
constexpr bool march_reachable(bool vec, const MarchForm& f) {
  return march_reachable(vec, f.lds, f.nt, f.comp, f.fuse, f.pd, f.asym, f.xdef, f.book, f.lmask);
}
constexpr int march_count(bool vec) {
  int n = 0;
  for (int c = 0; c < kMarchCodes; ++c) n += march_reachable(vec, march_decode(c));
  return n;
}
static_assert(march_count(true) == 67 && march_count(false) == 13, "the reachable set: 67 vector forms, 13 scalar ones");

template <bool VECTOR>
constexpr std::array<int, march_count(VECTOR)> march_codes() {
  std::array<int, march_count(VECTOR)> a{};
  int n = 0;
  for (int c = 0; c < kMarchCodes; ++c)
    if (march_reachable(VECTOR, march_decode(c))) a[n++] = c;
  return a;
}

}  // namespace mfs
