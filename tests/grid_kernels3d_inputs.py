"""Inputs and error bounds shared by tests/test_grid_kernels3d_gpu.py (the stateless 3D face-grid kernels of
csrc/mfs_visc.hip against the numpy oracle) and tests/test_grid_kernels3d_inputs.py (the CPU checks that keep those GPU
tests from being vacuous).  The reference is oracle/mfs_oracle.py in float64 on the same rounded inputs.

Bounds for the rows and the boundary condition.  Kernel and oracle evaluate the same expression in float64; they differ by
FMA contraction, by association and by the rounding of the final store:  |got - want| <= (R + 2) 2^-53 M + u_out |want|,
u_out = 2^-24 or 2^-53 by the output code, M the oracle's magnitude output (`mag=`), and R the number of rounded
operations that a term passes through on its longest path through the kernel.  Relative errors of the factors of a
product add, so both operands' paths count.  Counted from csrc/mfs_visc.hip:

k_visc_row_direct<RHS=false> (apply), R = 23: the own term takes the 5 adds of the six face volumes (the doublings are
  exact), scale*mu (1), *s (1), vs[0] + . (1), * own (1) = 9, then the 14 tap accumulations.  A tap term takes
  k = scale*mu (1), * vs (1), * v (1) = 3 and at most 14 accumulations = 17.
k_visc_row_direct<RHS=true> (rhs), R = 17: own * vs[0] (1) + 14 accumulations = 15; a tap term 3 + 14 = 17.
k_grid_boundary_condition, R = 25: an averaged velocity takes the product (1, in float32 when velocities and masses
  are both float32, then identical in kernel and oracle), 3 adds of vsum (the add to 0.0 is exact), 3 adds of msum and
  the division (1) = 8; - sv (1); * sn_i (sn_i itself 1, the product 1) = 11; the two adds of s = 13; * sn_a (sn_a 1,
  product 1) = 15; * sn_inv (three squares of once-rounded differences 3, 2 adds, the division 1, the product 1) = 22;
  1 - sphi/dx (2) and the last product (1) = 25.  Where s changes sign within its error the min(0, s) branch may
  differ; |s| is then below its own error, which the same bound covers.
"""
import numpy as np

from oracle import mfs_oracle as O

DX = 0.05
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
R_APPLY, R_RHS, R_BC = 23, 17, 25

# no interior face in some or all components; the minimum with one; one long axis (longer than a wavefront, no multiple of
# it) in each position; odd extents whose face arrays cross several 256-thread blocks mid-row
GRIDS = [(1, 1, 1), (2, 2, 2), (2, 5, 3), (3, 3, 3), (70, 3, 3), (3, 70, 3), (3, 3, 70), (13, 9, 11), (17, 19, 23)]
INTERIOR_GRIDS = [g for g in GRIDS if min(g) >= 3]          # at least one interior face in every component
COVERAGE_GRIDS = [g for g in INTERIOR_GRIDS if max(g) >= 9]  # (3,3,3) has two interior faces per component: too few to
#                                                             hold every category of a coverage check
FLAT_GRID = (17, 19, 23)                                     # carries the flat patch of sphi (NaN in the boundary condition)
# (scale * mu): the diagonal dominates / the taps do
KS = [(0.125, 0.25), (40.0, 3.0)]
gid = lambda g: "%dx%dx%d" % tuple(g)  # noqa: E731


def face_shape(gres, a):
    return tuple(int(v) + (1 if k == a else 0) for k, v in enumerate(gres))


def doubled_shape(gres):
    return tuple(2 * int(v) + 1 for v in gres)


def interior(shape):
    """mask of the faces that are not on the array boundary"""
    m = np.zeros(shape, bool)
    if min(shape) >= 3:
        m[1:-1, 1:-1, 1:-1] = True
    return m


def face_of_doubled(G, a):
    """the doubled-grid array G sampled at every face of component a"""
    sl = [slice(1, None, 2)] * 3
    sl[a] = slice(0, None, 2)
    return G[tuple(sl)]


_CACHE = {}


def inputs(gres, seed=5):
    """float64 inputs of every kernel on the grid `gres`, built once per (gres, seed) and never modified:
    sphi: walls 1.2 cells thick on both ends of every axis of at least 9 cells and an ellipsoid placed off-centre (radii
          max(1.1, 0.2 N) cells, 3.2 across a thin grid with one long axis), times DX; on (17,19,23) a flat patch of 5^3
          doubled nodes inside the ellipsoid.
    vol:  in [0, 1] with exact zeros, exact ones and partial values.      v*, sv: non-zero everywhere.
    m*:   zero on a sprinkle of faces and, on a grid with a long axis, on a block of up to 8^3 faces over the upper half of
          the ellipsoid, which three sweeps do not fill.
    out*: a candidate solution for the write-back, non-zero everywhere."""
    key = (tuple(gres), seed)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(seed * 1000 + sum(p * int(g) for p, g in zip((1, 7, 49), gres)))
    N3 = [int(g) for g in gres]
    ax = [np.arange(2 * n + 1, dtype=np.float64).reshape([-1 if k == a else 1 for k in range(3)]) * 0.5 for a, n in enumerate(N3)]
    wall = np.full(doubled_shape(gres), np.inf)
    for a, n in enumerate(N3):
        if n >= 9:
            wall = np.minimum(wall, np.minimum(ax[a], n - ax[a]) - 1.2)
    c = [0.3 * N3[0], 0.35 * N3[1], 0.3 * N3[2]]
    thin = 3.2 if max(N3) >= 9 else 1.1      # a thin axis beside a long one is covered whole: the solid is several faces deep
    rad = [max(thin, 0.2 * n) for n in N3]
    ball = (np.sqrt(sum(((ax[a] - c[a]) / rad[a]) ** 2 for a in range(3))) - 1.0) * min(rad)
    sphi = np.minimum(wall, ball) * DX
    if tuple(gres) == FLAT_GRID:
        i0 = [int(round(2 * v)) for v in c]
        patch = tuple(slice(i - 2, i + 3) for i in i0)
        assert (sphi[patch] < 0).all()
        sphi[patch] = -0.75 * DX
    d = dict(gres=tuple(N3), dx=DX, sphi=sphi)
    d["vol"] = np.clip(rng.uniform(-0.3, 1.3, size=sphi.shape), 0.0, 1.0)
    d["sv"] = rng.uniform(0.1, 0.6, size=sphi.shape + (3,)) * rng.choice([-1.0, 1.0], size=sphi.shape + (3,))
    for a, cn in enumerate("xyz"):
        shp = face_shape(gres, a)
        d["v" + cn] = rng.uniform(0.25, 1.5, size=shp) * rng.choice([-1.0, 1.0], size=shp)
        d["out" + cn] = rng.uniform(0.25, 1.5, size=shp) * rng.choice([-1.0, 1.0], size=shp)
        m = (rng.uniform(size=shp) > 0.15) * rng.uniform(0.2, 1.5, size=shp)
        if max(N3) >= 9:         # from the ellipsoid's centre upwards (its lower half keeps its mass), whole thin axes
            m[tuple(slice(int(c[k]), int(c[k]) + 8) if N3[k] >= 9 else slice(None) for k in range(3))] = 0.0
        d["m" + cn] = m
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = d
    return d


def rounded(a, dt):
    """the float64 array as the kernel receives it at dtype dt, and back in float64 (exact) for the oracle"""
    return np.asarray(a).astype(dt).astype(np.float64)


def ratio(got, want, M, R, u_out, where):
    """err / bound over the faces `where`; faces without a finite bound (NaN or inf magnitude, NaN result) count as inf unless
    got and want are equal, or NaN both"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - want)
        bound = (R + 2) * 2.0 ** -53 * M + u_out * np.abs(want)
        r = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    r = np.where(np.isfinite(bound) & np.isfinite(err), r, np.where(same, 0.0, np.inf))
    return np.where(where, r, 0.0)


# ------------------------------------------------------------------------------------------------ oracle calls ---
def rows(d, scale, mu, rhs, vdt=np.float64, sdt=np.float64, voldt=np.float64, sentinel=np.nan):
    """(results, magnitudes) of visc_rhs3d / visc_apply3d per component on inputs rounded to the given dtypes; faces
    that the oracle does not write hold `sentinel`"""
    gres = d["gres"]
    V = [rounded(d["v" + c], vdt) for c in "xyz"]
    out = [np.full(face_shape(gres, a), sentinel) for a in range(3)]
    mag = {}
    if rhs:
        O.visc_rhs3d(gres, scale, mu, *V, rounded(d["sphi"], sdt), None, rounded(d["vol"], voldt), *out, mag=mag)
    else:
        O.visc_apply3d(gres, scale, mu, *V, *out, rounded(d["sphi"], sdt), rounded(d["vol"], voldt), mag=mag)
    return out, [mag[a] for a in range(3)]


def boundary_condition(d, vdt=np.float64, mdt=np.float64, sdt=np.float64, svdt=np.float64, dvdt=np.float64, reverse=False):
    """(dv, magnitudes) of nb_boundary_condition per component on inputs rounded to the given dtypes"""
    gres = d["gres"]
    gv = [d["v" + c].astype(vdt) for c in "xyz"]
    gm = [d["m" + c].astype(mdt) for c in "xyz"]
    if vdt != mdt:                   # the product is formed in float64 unless both are float32
        gv, gm = [a.astype(np.float64) for a in gv], [a.astype(np.float64) for a in gm]
    dv = [np.full(face_shape(gres, a), 9.0, dvdt) for a in range(3)]
    mag = {}
    O.nb_boundary_condition(gres, gv, gm, rounded(d["sphi"], sdt), rounded(d["sv"], svdt), d["dx"], dv, mag=mag, reverse=reverse)
    return dv, [mag[a] for a in range(3)]


def bc_categories(d, a, mdt=np.float64, sdt=np.float64):
    """masks over the faces of component a: array boundary, far (sphi/dx >= 1), empty (near, and the four masses of an
    averaged component are all zero), rest"""
    shp = face_shape(d["gres"], a)
    inner = interior(shp)
    far = inner & (face_of_doubled(rounded(d["sphi"], sdt), a) / d["dx"] >= 1)
    empty = np.zeros(shp, bool)
    if inner.any():
        offs = {0: ((1, [(-p, q, 0) for p in range(2) for q in range(2)]), (2, [(-p, 0, q) for p in range(2) for q in range(2)])),
                1: ((0, [(q, -p, 0) for p in range(2) for q in range(2)]), (2, [(0, -p, q) for p in range(2) for q in range(2)])),
                2: ((0, [(q, 0, -p) for p in range(2) for q in range(2)]), (1, [(0, q, -p) for p in range(2) for q in range(2)]))}[a]
        cnt = [s - 2 for s in shp]
        for comp, oo in offs:
            m = rounded(d["m" + "xyz"[comp]], mdt)
            tot = sum(m[tuple(slice(1 + o[k], 1 + o[k] + cnt[k]) for k in range(3))] for o in oo)
            empty[1:-1, 1:-1, 1:-1] |= tot == 0
    empty &= inner & ~far
    return ~inner, far, empty, inner & ~far & ~empty
