"""Inputs, planted mistakes and error bounds shared by tests/test_cell_kernels3d_gpu.py (the nine stateless 3D cell kernels
of csrc/mfs_pressure.hip and csrc/mfs_density.hip against the numpy oracle) and tests/test_cell_kernels3d_inputs.py (the
CPU checks that keep those GPU tests from being vacuous).  The reference is oracle/mfs_oracle.py in float64 on the same
rounded inputs; a planted mistake is a textual edit of a copy of one of its functions (`mistaken`).

Bound.  Kernel and oracle evaluate the same expression in float64; they differ by FMA contraction (mfs_pressure.hip; it is
switched off in mfs_density.hip) and by the rounding of the final store:  |got - want| <= (R + 2) 2^-53 M + u_out |want|,
u_out = 2^-24 or 2^-53 by the output code, M the oracle's magnitude output (`mag=`) and R the number of rounded operations
on the longest path of a term through the kernel (min, max, fabs and the conversions of float32 inputs are exact).
Counted from the kernel sources:

k_pressure_rhs3d (mfs_pressure.hip:113-132), R = 14: a term w * v / cs takes the product and the quotient (2) and at most
  the 12 accumulations into bv.
k_pressure_apply3d (:150-164), R = 11: a ghost term takes phi - nphi and the quotient of gf_theta (2, :136), w / theta (1),
  the 6 accumulations into diag, diag * v (1) and the add into val (1) = 11; a tap term takes w * v (1) and at most 6
  accumulations and the last add = 8.
k_pressure_update3d (:176-185), R = 8: theta takes l - r and the quotient of edge_in_fraction (2, mfs_common.h:58-59);
  p - p' (1), * c (1), / theta (1), + v (1), * w (1), the last add (1) = 8; the other term takes 1 - w, * sv and the last
  add = 3.
k_density_fix_volume (mfs_density.hip:122-123,135-142), R = 9: the 5 adds of the six w, / 6 (1), * cvol (1) = 7, and cvol
  itself is a product of three rounded on the host (2).  The other operand of the min is an input or cvol.
k_density_rhs (:155-162), R = 16: the 5 adds and / 6 (6), 1 - . (1), * cvol (1, cvol itself 2), * rho0 (1), + gm (1),
  / cell_vol (1), / rho0 (1), 1 - frac (1), / dt (1) = 16.  M carries the amplification of the two differences (see
  density_rhs3d in the oracle).
k_density_apply (:177-191), R = 11: as k_pressure_apply3d with 1 / theta for w / theta.
k_density_displacement (:204-210), R = 6: theta (2), p - p' (1), * dt (1), * cs (1), / theta (1).
k_solid_frac3d and k_density_advect are compared bit for bit.
"""
import functools
import inspect

import numpy as np

from grid_kernels3d_inputs import GRIDS, U, doubled_shape, face_shape, gid, ratio, rounded  # noqa: F401
from oracle import mfs_oracle as O

F32, F64 = np.float32, np.float64
CS = (0.05, 0.0625, 0.04)                  # three distinct cell sizes, tied to no extent: a swapped axis shows
BMIN = (-0.25, 0.5, 0.125)
RHO0, DT = 1000.0, 1.0 / 300.0
CVOL = CS[0] * CS[1] * CS[2]
R = dict(pressure_rhs=14, pressure_apply=11, pressure_update=8, fix_volume=9, density_rhs=16, density_apply=11,
         displacement=6)
INTERIOR_GRIDS = [g for g in GRIDS if min(g) >= 3]
THIN_GRIDS = [g for g in INTERIOR_GRIDS if max(g) >= 9 and min(g) == 3]     # one interior row of 68 cells
COVERAGE_GRIDS = [g for g in INTERIOR_GRIDS if min(g) >= 9]
WRITING_GRIDS = [g for g in GRIDS if min(g) >= 2]                           # update and displacement write faces
PARTICLE_COUNTS = [0, 1, 63, 257]
BIAS = [(0.0, 0.5, 0.5), (0.5, 0.0, 0.5), (0.5, 0.5, 0.0)]

# lphi[x, y, z] = PATTERN[(x + 3 y + 5 z + 10) % 17] (cell (1,1,1), all there is inside (3,3,3), is liquid): every step along an axis is coprime to 17, so a line of 17 cells along any
# axis meets every entry, and the pairs (entry, entry at distance +-1, +-3, +-5) hold for each of the six sides: liquid
# beside liquid, liquid beside air with theta strictly inside (0.01, 1), -1e-4 beside +1.0 (theta clamps at 0.01), -1e-4
# beside a zero (theta exactly 1), a liquid beside a zero, air beside liquid and air beside air (searched for, and
# asserted by tests/test_cell_kernels3d_inputs.py).  e: -1e-4, O: +1.0, z: 0.0, n: -0.0, L: liquid, A: air.
PATTERN = "zeeeeOenOALOLzLAO"
LIQUID, AIR = (-1.0, -0.75, -0.5, -0.25), (0.25, 0.5, 0.75)
LPHI_SET = (-1e-4, 1.0, 0.0, -0.0) + LIQUID + AIR
W_SET = (0.0, 0.0, 1.0, 1.0, 1.0, 0.25, 0.5, 0.75, 0.3, 0.9, 0.6180339887498949)
NODE_SET = np.array([-3, -1, -1, 1, 1, 3, -2, 2, 0.0, -0.0]) / 64          # corner nodes: sums of four are exact
CENTRE_SET = (0.04, 0.03, 0.05, 0.039, 0.041, 0.06, -0.02, 0.0, -0.0, 0.2)  # around min(CS) = 0.04 and max(CS) = 0.0625


def interior(shape):
    m = np.zeros(shape, bool)
    if min(shape) >= 3:
        m[1:-1, 1:-1, 1:-1] = True
    return m


def upper(shape):
    """mask of the entries with x, y, z >= 1: what the update and the displacement may write"""
    m = np.zeros(shape, bool)
    m[1:, 1:, 1:] = True
    return m


def _blobs(gres):
    """centres of the all-liquid crosses (cell and its six neighbours) that make fix_volume's `internal` true"""
    N3 = tuple(int(g) for g in gres)
    if min(N3) < 3:
        return []
    long_axes = [a for a in range(3) if N3[a] >= 9]
    if not long_axes:
        return []
    if len(long_axes) == 3:
        return [(x, y, z) for x in range(2, N3[0] - 2, 4) for y in range(2, N3[1] - 2, 4) for z in (2, N3[2] - 3)]
    a = long_axes[0]
    return [tuple(k if b == a else 1 for b in range(3)) for k in range(5, N3[a] - 2, 34)]


@functools.lru_cache(maxsize=None)
def inputs(gres, seed=11):
    """float64 inputs of every cell kernel on the grid `gres`, built once and never modified.
    lphi: PATTERN with seeded magnitudes for its liquid and air entries; on a grid of at least 9 cells everywhere the half
          x > Nx / 2 is drawn from LPHI_SET cell by cell (more combinations of neighbours); all-liquid crosses at _blobs and,
          on those grids, crosses with one arm in the air.
          Boundary cells follow the same rule, so they carry both signs.
    wx, wy, wz: drawn from W_SET face by face, the planes w*[N] included; the six faces of a cell of gm / gvol category 0
          or 1 are 1 (no solid: cell mass and cell volume can vanish); faces of a cross centre are 1 or 0.75.
    sphi: corner nodes (all indices even) from NODE_SET, cell centres (all odd) from CENTRE_SET (cross centres cycle
          through it), every other node a seeded value of either sign.
    sv:   components of magnitude 0.1-0.2, 1-2 and 10-20, both signs.      v*, pv, v: non-zero, both signs.
    gm, gvol by seeded category of the cell: 0 no mass and no solid (cell_mass = 0 < 1e-10), 1 no volume, no solid and a
          mass of 0.8e-7 (the floor of max(cell_vol, 1e-10), with a fraction of 0.8 that any other floor changes), 2 light
          (clamps at 0.5 unless solid fills the cell), 3 heavy (1.5), 4-5 in between; a cross centre holds a quarter of the cell volume."""
    N3 = tuple(int(g) for g in gres)
    rng = np.random.default_rng(seed * 1000 + sum(p * n for p, n in zip((1, 7, 49), N3)))
    X, Y, Z = np.meshgrid(*[np.arange(n) for n in N3], indexing="ij")
    sym = np.array(list(PATTERN))[(X + 3 * Y + 5 * Z + 10) % len(PATTERN)]
    table = {"e": -1e-4, "O": 1.0, "z": 0.0, "n": -0.0}
    lphi = np.zeros(N3)
    for s, val in table.items():
        lphi[sym == s] = val
    lphi = np.where(sym == "L", rng.choice(LIQUID, size=N3), lphi)
    lphi = np.where(sym == "A", rng.choice(AIR, size=N3), lphi)
    if min(N3) >= 9:
        lphi = np.where(X > N3[0] // 2, rng.choice(LPHI_SET, size=N3), lphi)
    blobs = _blobs(N3)
    for c in blobs:
        for off in ((0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            lphi[tuple(np.add(c, off))] = -0.5
    # crosses with one arm in the air, each arm in turn, away from the solid: `internal` hangs on every neighbour
    broken = [(c[0], c[1], N3[2] // 2) for c in blobs if c[2] == 2] if min(N3) >= 9 else []
    for k, c in enumerate(broken):
        for j, off in enumerate(((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (0, 0, 0))):
            lphi[tuple(np.add(c, off))] = 0.5 if j == k % 6 else -0.5
    d = dict(gres=N3, cs=CS, lphi=lphi)

    inner = interior(N3)
    cat = np.where(inner, rng.integers(0, 6, size=N3), 5)
    for c in blobs + broken:
        cat[c] = 6
    W = [rng.choice(W_SET, size=face_shape(N3, a)) for a in range(3)]
    for a in range(3):
        for side in (0, 1):
            sl = tuple(slice(side, side + n) if b == a else slice(0, n) for b, n in enumerate(N3))
            W[a][sl] = np.where(cat <= 1, 1.0, W[a][sl])
            W[a][sl] = np.where(cat == 6, rng.choice((1.0, 1.0, 0.75), size=N3), W[a][sl])
    d["wx"], d["wy"], d["wz"] = W
    vol = rng.uniform(0.3, 1.2, size=N3) * CVOL
    f = np.choose(np.clip(cat, 0, 5), [0.0, 0.0, 0.05, 2.5, 0.8, 1.15])
    gm = np.where(cat == 1, 0.8e-7, RHO0 * vol * f)
    gvol = np.where(cat == 1, 0.0, vol)
    gvol = np.where(cat == 6, 0.25 * CVOL, gvol)
    gm = np.where(cat == 6, RHO0 * 0.25 * CVOL, gm)
    d["gm"], d["gvol"], d["cat"] = gm, gvol, cat

    D2 = doubled_shape(N3)
    sphi = rng.uniform(0.01, 0.08, size=D2) * rng.choice([-1.0, 1.0], size=D2)
    sphi[::2, ::2, ::2] = rng.choice(NODE_SET, size=tuple(n + 1 for n in N3))
    sphi[1::2, 1::2, 1::2] = rng.choice(CENTRE_SET, size=N3)
    for k, c in enumerate(blobs):
        sphi[tuple(2 * v + 1 for v in c)] = CENTRE_SET[k % len(CENTRE_SET)]
    for c in broken:
        sphi[tuple(2 * v + 1 for v in c)] = 0.2
    d["sphi"] = sphi
    sv = rng.uniform(1.0, 2.0, size=D2 + (3,)) * rng.choice([-1.0, 1.0], size=D2 + (3,))
    d["sv"] = sv * np.array([0.1, 1.0, 10.0])
    signed = lambda shp: rng.uniform(0.25, 1.5, size=shp) * rng.choice([-1.0, 1.0], size=shp)  # noqa: E731
    for a, cn in enumerate("xyz"):
        d["v" + cn] = signed(face_shape(N3, a))
    d["pv"], d["v"] = signed(N3), signed(N3)
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def particles(shape, axis, P, seed=3):
    """P positions (float64, P x 3) for the advect of a sample array of `shape` whose samples sit at
    (index + BIAS[axis]) * CS + BMIN, cycling through: inside the sampled box; exactly on a sample point in every
    coordinate (the neighbouring doubles are tried until the weight is exactly 0 or 1: y, with a binary cell size and
    origin, always gets there, x and z at the indices that reproduce themselves); below the first sample and
    above the last one in one coordinate (the index clamp), inside in the others.  P = 1 is a single inside point."""
    rng = np.random.default_rng(seed + 17 * P + axis)
    s, bias, cs, bmin = (np.asarray(a, F64) for a in (shape, BIAS[axis], CS, BMIN))
    px = np.zeros((P, 3))
    for p in range(P):
        kind = p % 8
        u = rng.uniform(0.0, 1.0, size=3) * np.maximum(s - 1, 0.25)               # in sample units, inside
        if kind == 1:
            u = np.floor(rng.uniform(0.0, 1.0, size=3) * s)
        elif kind >= 2:
            a = (kind - 2) % 3
            u[a] = -rng.uniform(0.3, 2.5) if kind < 5 else s[a] - 1 + rng.uniform(0.3, 2.5)
        px[p] = (u + bias) * cs + bmin
        if kind == 1:                              # the neighbouring doubles too, until the weight is exactly 0 or 1
            for a in range(3):
                for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
                    cand = px[p, a] + k * np.spacing(px[p, a])
                    w = O._particle_cell(np.array([cand]), bmin[a], cs[a], bias[a])[1][0]
                    if w == 0 or w == 1:
                        px[p, a] = cand
                        break
    px.setflags(write=False)
    return px


def clamps(px, shape, axis):
    """per coordinate: (clamped low, clamped high, unclamped) masks over the particles, as the kernel's index clamp sees them"""
    gi, _ = O._particle_cell(px, BMIN, CS, BIAS[axis])
    return [(gi[:, a] < 0, gi[:, a] + 1 > shape[a] - 1, (gi[:, a] >= 0) & (gi[:, a] + 1 <= shape[a] - 1)) for a in range(3)]


# ------------------------------------------------------------------------------------------------ oracle calls ---
@functools.lru_cache(maxsize=None)
def mistaken(fn, old, new, count=1):
    """a copy of the oracle's function `fn` whose source has `old` replaced by `new` (`old` must occur `count` times)"""
    src = inspect.getsource(getattr(O, fn))
    assert src.count(old) == count, (fn, old, src.count(old))
    ns = dict(vars(O))
    exec(compile(src.replace(old, new), f"<{fn} with a planted mistake>", "exec"), ns)
    return ns[fn]


def _fn(name, mistake):
    if mistake is None or mistake[0] != name:
        return getattr(O, name)
    return mistaken(*mistake)


def dts(dt):
    """a dtype per argument group from one dtype, a dict, or None (all float64)"""
    class _All(dict):
        def __missing__(self, k):
            return F64 if isinstance(dt, dict) or dt is None else dt
    return _All(dt) if isinstance(dt, dict) else _All()


def solid_frac(d, sdt=F64, fill=7.5, mistake=None):
    """wx, wy, wz of compute_solid_frac3d on sphi rounded to sdt; the planes w*[N] keep `fill`"""
    w = [np.full(face_shape(d["gres"], a), fill) for a in range(3)]
    _fn("compute_solid_frac3d", mistake)(d["gres"], rounded(d["sphi"], sdt), *w)
    return w


def _w(d, dt):
    return [rounded(d[k], dt) for k in ("wx", "wy", "wz")]


def call(kernel, d, dt=None, sentinel=np.nan, mistake=None):
    """(results, magnitudes) of one of the seven bounded kernels on the inputs `d` rounded per argument group (`dts`);
    entries that the oracle does not write hold `sentinel` (update: the given velocities; fix_volume: boundary cells)"""
    t, g, out, mag = dts(dt), d["gres"], None, {}
    if kernel == "pressure_rhs":
        out = np.full(g, sentinel)
        _fn("pressure_rhs3d", mistake)(CS, g, *[rounded(d["v" + c], t["v"]) for c in "xyz"], None, rounded(d["sv"], t["sv"]),
                                       rounded(d["lphi"], t["lphi"]), out, *_w(d, t["w"]), mag=mag)
        return [out], [mag["b"]]
    if kernel in ("pressure_apply", "density_apply"):
        out = np.full(g, sentinel)
        _fn(kernel + "3d", mistake)(g, rounded(d["v"], t["v"]), out, *_w(d, t["w"]), rounded(d["lphi"], t["lphi"]), mag=mag)
        return [out], [mag["out"]]
    if kernel == "pressure_update":
        v = [rounded(d["v" + c], t["v"]) for c in "xyz"]
        _fn("pressure_update3d", mistake)(g, CS, *v, rounded(d["pv"], t["pv"]), *_w(d, t["w"]), rounded(d["sv"], t["sv"]),
                                          rounded(d["lphi"], t["lphi"]), mag=mag)
        return v, [mag[a] for a in range(3)]
    if kernel == "fix_volume":
        out = np.where(interior(g), rounded(d["gvol"], t["g"]), sentinel)
        _fn("density_fix_volume3d", mistake)(CS, g, None, out, rounded(d["sphi"], t["sphi"]), rounded(d["lphi"], t["lphi"]),
                                             *_w(d, t["w"]), mag=mag)
        return [out], [mag["gvol"]]
    if kernel == "density_rhs":
        out = np.full(g, sentinel)
        _fn("density_rhs3d", mistake)(RHO0, DT, g, CS, rounded(d["gm"], t["g"]), rounded(d["gvol"], t["g"]),
                                      rounded(d["lphi"], t["lphi"]), *_w(d, t["w"]), out, mag=mag)
        return [out], [mag["b"]]
    if kernel == "displacement":
        out = [np.full(face_shape(g, a), sentinel) for a in range(3)]
        _fn("density_displacement3d", mistake)(g, DT, CS, *out, rounded(d["pv"], t["pv"]), rounded(d["lphi"], t["lphi"]), mag=mag)
        return out, [mag[a] for a in range(3)]
    raise KeyError(kernel)


def written(kernel, d, dt=None):
    """per output array: the entries that the kernel writes and that carry a bound (fluid interior cells; faces with
    x, y, z >= 1, for the update only the active ones)"""
    t, g = dts(dt), d["gres"]
    L = rounded(d["lphi"], t["lphi"])
    if kernel in ("pressure_rhs", "pressure_apply", "density_apply", "density_rhs"):
        return [interior(g) & (L < 0)]
    if kernel == "fix_volume":
        return [interior(g)]
    out = []
    for a in range(3):
        m = upper(face_shape(g, a))
        if kernel == "pressure_update":
            act = np.zeros(m.shape, bool)
            C = (slice(1, g[0]), slice(1, g[1]), slice(1, g[2]))
            Mn = tuple(slice(1 - (a == b), g[b] - (a == b)) for b in range(3))
            act[C] = (L[C] < 0) | (L[Mn] < 0)
            m &= act
        else:
            m[tuple(slice(-1, None) if b == a else slice(None) for b in range(3))] = False
        out.append(m)
    return out


def advect(px, dval, axis, pdt=F64, ddt=F64, mistake=None):
    """positions after density_advect3d at the given dtypes"""
    p = np.array(px, dtype=pdt)
    _fn("density_advect3d", mistake)(p, np.asarray(dval).astype(ddt), BMIN, CS, BIAS[axis], axis)
    return p


# (name, kernel of `call` / "solid_frac" / "advect", (oracle function, old text, new text[, count]))
MISTAKES = [
    ("density -z tap weighted by wz[z]", "density_apply",
     ("density_apply3d", "((0, 0, -1), sh(wz, 0, 0, 1))", "((0, 0, -1), sh(wz, 0, 0, 0))")),
    ("pressure diagonal counts 1 for w", "pressure_apply",
     ("pressure_apply3d", "np.where(nf, w, w / _theta(phi, nphi))", "np.where(nf, 1.0, w / _theta(phi, nphi))")),
    ("theta floor removed (pressure apply)", "pressure_apply",
     ("pressure_apply3d", "w / _theta(phi, nphi)", "w / np.minimum(1.0, phi / (phi - nphi))")),
    ("theta floor removed (density apply)", "density_apply",
     ("density_apply3d", "1.0 / _theta(phi, nphi)", "1.0 / np.minimum(1.0, phi / (phi - nphi))")),
    ("theta floor removed (update)", "pressure_update",
     ("pressure_update3d", "np.maximum(0.01, edge_in_fraction(pc, pm))", "edge_in_fraction(pc, pm)")),
    ("theta floor removed (displacement)", "displacement",
     ("density_displacement3d", "np.maximum(0.01, edge_in_fraction(L[c], L[m]))", "edge_in_fraction(L[c], L[m])")),
    ("w <= 1 for w < 1", "pressure_rhs", ("pressure_rhs3d", "np.where(w < 1, w * s / c, 0.0)", "np.where(w <= 1, w * s / c, 0.0)")),
    ("sv components swapped (rhs)", "pressure_rhs", ("pressure_rhs3d", "sv = np.asarray(sv, F64)", "sv = np.asarray(sv, F64)[..., [0, 2, 1]]")),
    ("sv components swapped (update)", "pressure_update",
     ("pressure_update3d", "sv = np.asarray(sv, F64)", "sv = np.asarray(sv, F64)[..., [1, 0, 2]]")),
    ("cell sizes swapped (rhs)", "pressure_rhs",
     ("pressure_rhs3d", "cs = [float(c) for c in cell_size]", "cs = [float(cell_size[k]) for k in (0, 2, 1)]")),
    ("cell sizes swapped (update)", "pressure_update",
     ("pressure_update3d", "cs = [float(c) for c in cell_size]", "cs = [float(cell_size[k]) for k in (1, 0, 2)]")),
    ("cell sizes swapped (displacement)", "displacement",
     ("density_displacement3d", "cs = np.asarray(cell_size, F64)", "cs = np.asarray(cell_size, F64)[[2, 1, 0]]")),
    ("lphi <= 0 for lphi < 0 (pressure rhs)", "pressure_rhs", ("pressure_rhs3d", "[I] < 0", "[I] <= 0")),
    ("lphi <= 0 for lphi < 0 (pressure apply, neighbour)", "pressure_apply", ("pressure_apply3d", "nf = nphi < 0", "nf = nphi <= 0")),
    ("lphi <= 0 for lphi < 0 (pressure apply, cell)", "pressure_apply", ("pressure_apply3d", "np.where(phi < 0, val", "np.where(phi <= 0, val")),
    ("lphi <= 0 for lphi < 0 (density apply, neighbour)", "density_apply", ("density_apply3d", "nf = nphi < 0", "nf = nphi <= 0")),
    ("lphi <= 0 for lphi < 0 (density rhs)", "density_rhs", ("density_rhs3d", "[I] >= 0, 0.0", "[I] > 0, 0.0")),
    ("lphi <= 0 for lphi < 0 (update)", "pressure_update", ("pressure_update3d", "act = (pc < 0) | (pm < 0)", "act = (pc <= 0) | (pm <= 0)")),
    ("lphi <= 0 for lphi < 0 (fix_volume)", "fix_volume",
     ("density_fix_volume3d", "internal = internal & (sh(lphi, *off) < 0)", "internal = internal & (sh(lphi, *off) <= 0)")),
    ("max(cell_size) for min in fix_volume", "fix_volume", ("density_fix_volume3d", "float(np.min(cs))", "float(np.max(cs))")),
    ("fix_volume ignores near_solid", "fix_volume", ("density_fix_volume3d", "internal & ~near_solid", "internal")),
    ("fix_volume drops a neighbour from internal", "fix_volume", ("density_fix_volume3d", "(0, 0, 1), (0, 0, -1)):", "(0, 0, 1)):")),
    ("neighbour of the wrong axis in the displacement", "displacement",
     ("density_displacement3d", "slice(0, n - 1) if a == ax", "slice(0, n - 1) if a == (ax + 1) % 3")),
    ("density rhs without the mass threshold", "density_rhs", ("density_rhs3d", "np.where(cell_mass < 1e-10, 1.0, frac)", "frac")),
    ("density rhs without the volume floor", "density_rhs", ("density_rhs3d", "np.maximum(cell_vol, 1e-10)", "np.maximum(cell_vol, 1e-7)")),
    ("density rhs clamps at 0.4", "density_rhs", ("density_rhs3d", "np.maximum(0.5,", "np.maximum(0.4,")),
    ("density rhs clamps at 1.6", "density_rhs", ("density_rhs3d", "np.minimum(1.5,", "np.minimum(1.6,")),
    ("solid-fraction face from the wrong four nodes", "solid_frac",
     ("compute_solid_frac3d", "face_in_fraction(tlb, blb, tlf, blf)", "face_in_fraction(trb, blb, tlf, blf)")),
    ("advect with the bias of another axis", "advect",
     ("density_advect3d", "_particle_cell(px, bound_min, cell_size, grid_bias)",
      "_particle_cell(px, bound_min, cell_size, np.roll(np.asarray(grid_bias, F64), 1))")),
]
