// pcg_form_check.cpp -- march_form / march_reachable (csrc/mfs_pcg_form.h) against the decision tree they replaced.
//
// old_launch_apply / old_launch_apply_v below are launch_apply / launch_apply_v of mfs_pcg.hip as they stood before the resolver, transcribed: same
// variables, same branches in the same order, every launch macro replaced by a `return` of the template tuple it named
// (the macros' inner `if (nt) ... else ...` / `if (comp) ...` ladders folded into the tuple's arguments).  It is the
// specification: do not tidy it.  Stand-alone (built by tests/test_pcg_form.py with the host compiler and
// -fsanitize=address,undefined); prints "ok ..." and exits 0, or says what differs and exits 1.
#include <algorithm>
#include <cstdio>
#include <set>

#include "mfs_pcg_form.h"

using namespace mfs;

namespace {

constexpr int kApplyBlock = 256;
static_assert(kApplyBlock == kMarchBlock, "march workgroup size");

// the engine fields and launch arguments the old tree read
struct OldEngine {
  int variant, nt, nt_auto, compress, pd, asym;
  bool lane_mask;
  long long n;
  int Nz;
  bool skip_items;
  int skip_xb, skip_xe;
};
struct OldFuse { bool xdef, book; };

struct Tuple {
  int status;                     // 0 launched | 1 "needs the LDS march" | 2 "needs the vector path"
  bool direct, lds; int nt; bool comp, fuse; int pd; bool asym, xdef, book, lmask, listed;
};
Tuple refused(int status) { Tuple t{}; t.status = status; return t; }
Tuple launched(bool listed, bool lds, int nt, bool comp, bool fuse, int pd, bool asym, bool xdef = false, bool book = false,
               bool lmask = false) {
  return Tuple{0, false, lds, nt, comp, fuse, pd, asym, xdef, book, lmask, listed};
}

template <typename T, int VEC>
Tuple old_launch_apply_v(const OldEngine* h, int xb, int xe, int xb2, int xe2, const OldFuse* fz) {
  const bool asym = h->asym != 0;
  int variant = asym ? std::max(1, h->variant) : h->variant;
  const size_t lds = 2 * ((size_t)kApplyBlock * VEC + 2 * (size_t)h->Nz) * sizeof(T);
  if (variant >= 2 && lds > 64 * 1024) variant = 1;
  bool items = false;
  if (fz && h->skip_items && h->compress != 0 && VEC > 1 && xb == h->skip_xb && xe == h->skip_xe && xe2 == xb2 && variant >= 2)
    items = true;
  const bool lmask = items && h->lane_mask && VEC > 1;
  if (variant == 0) return Tuple{0, true, false, 0, false, false, 0, false, false, false, false, false};
  int nt = h->nt < 0 ? ((6.0 * (double)h->n * sizeof(T) > 200e6) ? h->nt_auto : 0) : (h->nt & 7);
  const bool comp = h->compress != 0 && VEC > 1;
  const int pd = (h->pd >= 2 && !asym) ? 2 : 1;
  if (variant == 1) {
    if (fz != nullptr) return refused(1);
    if (asym) return launched(items, false, nt ? 1 : 0, false, false, 1, true);
    else      return launched(items, false, nt ? 1 : 0, false, false, 1, false);
  } else if (fz && fz->book) {
    // MFS_GO_B(NTV, CMP, ASY, XDF): LMASK = CMP && lmask
    if (fz->xdef && asym) return launched(items, true, nt ? 7 : 0, comp, true, 1, true, true, true, comp && lmask);
    else if (fz->xdef)    return launched(items, true, nt ? 7 : 0, comp, true, 1, false, true, true, comp && lmask);
    else if (asym)        return launched(items, true, nt ? 7 : 0, comp, true, 1, true, false, true, comp && lmask);
    else                  return launched(items, true, nt ? 7 : 0, comp, true, 1, false, false, true, comp && lmask);
  } else if (fz && fz->xdef) {
    // MFS_GO_X(NTV, CMP, ASY): LMASK = CMP && lmask
    if (asym) return launched(items, true, nt ? 7 : 0, comp, true, 1, true, true, false, comp && lmask);
    else      return launched(items, true, nt ? 7 : 0, comp, true, 1, false, true, false, comp && lmask);
  } else if (asym) {
    if (fz) return launched(items, true, nt ? 7 : 0, comp, true, 1, true);
    else    return launched(items, true, nt ? 7 : 0, comp, false, 1, true);
  } else if (fz) {
    if (pd == 2) return launched(items, true, nt ? 7 : 0, comp, true, 2, false);
    else         return launched(items, true, nt ? 7 : 0, comp, true, 1, false);
  } else if (comp || nt == 0 || nt == 7) {
    if (pd == 2) return launched(items, true, nt ? 7 : 0, comp, false, 2, false);
    else         return launched(items, true, nt ? 7 : 0, comp, false, 1, false);
  } else {
    switch (nt) {
      case 1: return launched(items, true, 1, false, false, 1, false);
      case 3: return launched(items, true, 3, false, false, 1, false);
      case 5: return launched(items, true, 5, false, false, 1, false);
      default: return launched(items, true, 7, false, false, 1, false);
    }
  }
}

template <typename T, int VECOF>
Tuple old_launch_apply(const OldEngine* h, bool vec, int xb, int xe, int xb2, int xe2, const OldFuse* fz) {
  if (vec) return old_launch_apply_v<T, VECOF>(h, xb, xe, xb2, xe2, fz);
  if (fz != nullptr) return refused(2);
  return old_launch_apply_v<T, 1>(h, xb, xe, xb2, xe2, nullptr);
}

int code(bool lds, int nt, bool comp, bool fuse, int pd, bool asym, bool xdef, bool book, bool lmask) {
  return ((((((((lds * 8 + nt) * 2 + comp) * 2 + fuse) * 4 + pd) * 2 + asym) * 2 + xdef) * 2 + book) * 2 + lmask);
}

constexpr int count_reachable(bool vec) {
  int c = 0;
  for (int b = 0; b < 256; ++b)
    for (int nt = 0; nt < 8; ++nt)
      for (int pd = 0; pd <= 3; ++pd)
        c += march_reachable(vec, b & 1, nt, b & 2, b & 4, pd, b & 8, b & 16, b & 32, b & 64) && !(b & 128);
  return c;
}
static_assert(count_reachable(true) == 67, "reachable tuples with whole vectors");
static_assert(count_reachable(false) == 13, "reachable tuples on the scalar path");

int fails = 0;
void fail(const char* what, const OldEngine& h, bool vec, size_t elt, int fused, const Tuple& o, int st, const MarchForm& f) {
  if (++fails > 20) return;
  std::printf("MISMATCH %s: variant %d nt %d nt_auto %d compress %d pd %d asym %d lane %d n %lld Nz %d list %d vec %d elt %zu fused %d\n"
              "  old: status %d direct %d <%d,%d,%d,%d,%d,%d,%d,%d,%d> listed %d\n  new: status %d direct %d <%d,%d,%d,%d,%d,%d,%d,%d,%d> listed %d\n",
              what, h.variant, h.nt, h.nt_auto, h.compress, h.pd, h.asym, h.lane_mask, h.n, h.Nz, h.skip_items, vec, elt, fused,
              o.status, o.direct, o.lds, o.nt, o.comp, o.fuse, o.pd, o.asym, o.xdef, o.book, o.lmask, o.listed,
              st, f.direct, f.lds, f.nt, f.comp, f.fuse, f.pd, f.asym, f.xdef, f.book, f.lmask, f.listed);
}

}  // namespace

int main() {
  std::set<int> produced[2];      // [vec]
  long long cases = 0;
  const OldFuse fuses[5] = {{false, false}, {false, false}, {true, false}, {false, true}, {true, true}};
  const int nt_autos[4] = {7, 0, 1, 5};
  for (int elt_i = 0; elt_i < 2; ++elt_i)
  for (int vec = 0; vec < 2; ++vec)
  for (int variant = 0; variant <= 2; ++variant)
  for (int nt = -1; nt <= 7; ++nt)
  for (int nta = 0; nta < 4; ++nta)
  for (int big = 0; big < 2; ++big)              // n * elt on both sides of 200e6 / 6
  for (int longrow = 0; longrow < 2; ++longrow)  // LDS image fits / does not
  for (int compress = 0; compress < 2; ++compress)
  for (int pd = 1; pd <= 2; ++pd)
  for (int asym = 0; asym < 2; ++asym)
  for (int fused = 0; fused < 5; ++fused)
  for (int lane = 0; lane < 2; ++lane)
  for (int list = 0; list < 2; ++list)
  for (int range = 0; range < 3; ++range) {      // the list's range | another range | two ranges
    const size_t elt = elt_i ? 8 : 4;
    OldEngine h{};
    h.variant = variant; h.nt = nt; h.nt_auto = nt_autos[nta]; h.compress = compress; h.pd = pd; h.asym = asym;
    h.lane_mask = lane != 0;
    const long long edge = (long long)(200e6 / 6.0 / (double)elt);      // 6 n elt > 200e6 from edge + 1 on
    h.n = big ? edge + 1 : edge;
    const int nz_fit = (int)((64 * 1024 / (2 * elt) - (size_t)kApplyBlock * (vec ? 16 / elt : 1)) / 2);   // longest row whose image fits
    h.Nz = longrow ? nz_fit + 1 : nz_fit;
    h.skip_items = list != 0; h.skip_xb = 1; h.skip_xe = 11;
    const int xb = 1, xe = range == 1 ? 10 : 11, xb2 = 0, xe2 = range == 2 ? 1 : 0;
    const OldFuse* fz = fused ? &fuses[fused] : nullptr;
    const Tuple o = elt_i ? old_launch_apply<double, 2>(&h, vec != 0, xb, xe, xb2, xe2, fz)
                          : old_launch_apply<float, 4>(&h, vec != 0, xb, xe, xb2, xe2, fz);
    MarchInputs in{};
    in.variant = variant; in.nt = nt; in.nt_auto = h.nt_auto; in.compress = compress; in.pd = pd;
    in.asym = asym != 0; in.lane_mask = h.lane_mask; in.vec = vec != 0; in.elt = elt; in.n = h.n; in.Nz = h.Nz;
    in.has_list = h.skip_items; in.list_range = xb == h.skip_xb && xe == h.skip_xe && xe2 == xb2;
    in.fused = fused;
    MarchForm f{};
    const int st = march_form(in, &f);
    ++cases;
    const int want = o.status == 0 ? kFormOk : o.status == 1 ? kFormNeedsLds : kFormNeedsVec;
    if (st != want) { fail("status", h, vec, elt, fused, o, st, f); continue; }
    if (!vec && fused && st != kFormNeedsVec) fail("scalar fused must be refused", h, vec, elt, fused, o, st, f);
    if (st != kFormOk) continue;
    if (o.direct != f.direct) { fail("direct", h, vec, elt, fused, o, st, f); continue; }
    if (f.direct) continue;
    if (o.lds != f.lds || o.nt != f.nt || o.comp != f.comp || o.fuse != f.fuse || o.pd != f.pd || o.asym != f.asym ||
        o.xdef != f.xdef || o.book != f.book || o.lmask != f.lmask || o.listed != f.listed)
      fail("tuple", h, vec, elt, fused, o, st, f);
    // the kernel's static_asserts, restated
    if (!(!f.xdef || f.fuse) || !(!f.lmask || (f.comp && f.fuse && f.pd == 1)) || !(!f.book || f.fuse) || !(!f.fuse || f.lds))
      fail("static_assert of k_pcg_apply_march", h, vec, elt, fused, o, st, f);
    // lane masking only ever rides on a listed launch
    if (f.lmask && !f.listed) fail("lmask without the list", h, vec, elt, fused, o, st, f);
    if (!march_reachable(vec != 0, f.lds, f.nt, f.comp, f.fuse, f.pd, f.asym, f.xdef, f.book, f.lmask))
      fail("produced but not reachable", h, vec, elt, fused, o, st, f);
    produced[vec].insert(code(f.lds, f.nt, f.comp, f.fuse, f.pd, f.asym, f.xdef, f.book, f.lmask));
  }
  for (int vec = 0; vec < 2; ++vec) {
    std::set<int> reach;
    for (int b = 0; b < 128; ++b)
      for (int nt = 0; nt < 8; ++nt)
        for (int pd = 0; pd <= 3; ++pd)
          if (march_reachable(vec != 0, b & 1, nt, b & 2, b & 4, pd, b & 8, b & 16, b & 32, b & 64))
            reach.insert(code(b & 1, nt, b & 2, b & 4, pd, b & 8, b & 16, b & 32, b & 64));
    const size_t want = vec ? 67 : 13;
    if (reach != produced[vec] || reach.size() != want) {
      ++fails;
      std::printf("MISMATCH reachable set, vec %d: %zu reachable, %zu produced, %zu expected\n", vec, reach.size(),
                  produced[vec].size(), want);
    }
  }
  if (fails) { std::printf("FAILED: %d mismatches in %lld cases\n", fails, cases); return 1; }
  std::printf("ok %lld cases, %zu vector forms, %zu scalar forms\n", cases, produced[1].size(), produced[0].size());
  return 0;
}
