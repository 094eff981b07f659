// volume_sample_check.cpp -- csrc/mfs_volume.h on the host: the header alone, plain C++17, no HIP.
//
//   volume_sample_check FILE   reads a float32 and a float64 volume of the same extents, a pose and world points
//                              (tests/test_volume_sample.py writes FILE and states its layout) and prints, per point, the
//                              bits of pose_to_body's point and of volume_sample's outputs for both volumes
//   volume_sample_check        holds lattice_split against / and % on every point of three lattices
// Build with -ffp-contract=off: the header's arithmetic must round as written.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mfs_volume.h"

using namespace mfs;

static uint64_t bits(double v) {
  uint64_t u;
  memcpy(&u, &v, sizeof(u));
  return u;
}

template <typename T>
static bool read_n(FILE* f, std::vector<T>* out, size_t n) {
  out->resize(n);
  return fread(out->data(), sizeof(T), n, f) == n;
}

static int sample_file(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return fprintf(stderr, "cannot open %s\n", path), 2;
  std::vector<int64_t> head;          // n0, n1, n2, number of points
  std::vector<double> geom;           // origin (3), spacing, R row-major (9), T (3)
  std::vector<float> vol32;
  std::vector<double> vol64, pts;
  bool ok = read_n(f, &head, 4) && read_n(f, &geom, 16);
  const size_t nodes = ok ? (size_t)(head[0] * head[1] * head[2]) : 0;
  ok = ok && read_n(f, &vol32, nodes) && read_n(f, &vol64, nodes) && read_n(f, &pts, 3 * (size_t)head[3]);
  fclose(f);
  if (!ok) return fprintf(stderr, "short file %s\n", path), 2;

  Volumes V;
  memset(&V, 0, sizeof(V));
  for (int i = 0; i < 2; ++i) {       // entry 0: the float32 volume, entry 1: the float64 one
    V.vol[i] = i == 0 ? (const void*)vol32.data() : (const void*)vol64.data();
    V.dt[i] = i == 0 ? MFS_F32 : MFS_F64;
    V.h[i] = geom[3];
    for (int k = 0; k < 3; ++k) {
      V.n[i][k] = (int)head[k];
      V.org[i][k] = geom[k];
    }
  }
  double R[3][3], T[3];
  for (int k = 0; k < 3; ++k) {
    T[k] = geom[13 + k];
    for (int c = 0; c < 3; ++c) R[k][c] = geom[4 + 3 * k + c];
  }
  for (int64_t p = 0; p < head[3]; ++p) {
    double xb[3], g[3];
    bool inside = false;
    int cell[3] = {-1, -1, -1};
    pose_to_body(R, T, &pts[3 * p], xb);
    const double plain32 = volume_sample(V, 0, xb);
    const double full32 = volume_sample(V, 0, xb, &inside, cell, g);
    const double v64 = volume_sample(V, 1, xb);
    printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64
           " %016" PRIx64 " %016" PRIx64 " %d %d %d %d\n",
           bits(xb[0]), bits(xb[1]), bits(xb[2]), bits(plain32), bits(full32), bits(v64), bits(g[0]), bits(g[1]), bits(g[2]),
           (int)inside, cell[0], cell[1], cell[2]);
  }
  return 0;
}

static int64_t split_lattice(int64_t n0, int64_t n1, int64_t n2) {
  const int64_t total = n0 * n1 * n2;
  int64_t bad = 0;
  for (int64_t base = 0; base < total; base += 256)       // one workgroup of 256 lanes at a time, as the kernels
    for (int tid = 0; tid < 256 && base + tid < total; ++tid) {
      const int64_t p = base + tid;
      const LatticeIndex at = lattice_split(base, tid, n1, n2);
      if (at.i0 != p / (n1 * n2) || (int64_t)at.i1 != (p / n2) % n1 || (int64_t)at.i2 != p % n2) ++bad;
    }
  printf("lattice_split %" PRId64 " x %" PRId64 " x %" PRId64 ": %" PRId64 " points, %" PRId64 " wrong\n", n0, n1, n2, total,
         bad);
  return bad;
}

int main(int argc, char** argv) {
  if (argc > 1) return sample_file(argv[1]);
  // n2 below, near and above the block of 256, rows that straddle blocks
  const int64_t bad = split_lattice(7, 5, 11) + split_lattice(3, 130, 3) + split_lattice(2, 3, 300);
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
