"""Inputs, planted mistakes and error bounds shared by tests/test_sdf3d_branches_gpu.py (the three kernels of
csrc/mfs_sdf.hip -- k_sdf_evaluate, k_sdf_evaluate_grid, k_sdf_project -- against oracle/mfs_oracle.py) and
tests/test_sdf3d_inputs.py (the CPU checks that keep those GPU tests from being vacuous).  No torch, no GPU.

Three kinds of input.
GENERIC: rotated bodies of all six type codes (sphere, box, cylinder; solid and flipped) and one row of the mesh code 6,
  which the three kernels must leave alone wherever it sits (GENERIC_TABLES: first, middle, last).  Points are drawn at
  random and kept only where no compared quantity of `evaluate` or `project` (every gap that the oracle's `trace=` reports:
  disp against 0, max_disp against 0 and against disp, sd against 0, |y| against hh, the gap between the two largest
  candidates of the cylinder's max, the face distances of box_project against the nearest so far, every body's distance
  against the least so far, which holds best against second best) lies within MARGIN = 1e-6 of its threshold: the kernel's
  sqrt against the oracle's ** 0.5 cannot flip a branch.
EXACT: unrotated bodies (generate_rb(angle=0) leaves an exact identity) at dyadic centres with dyadic sizes, and points at
  which every intermediate of the owning body is exact, so that the comparisons hold by EQUALITY: EXACT_SCENES.  The
  expectation is bit equality with the oracle, the sign of a zero included, NaN matching NaN.
CHAIN: a sphere, a box and a cylinder that overlap; the box and the cylinder move points that the sphere moved.  With
  float32 positions, rounding after every body (the reference writes into the array row) and rounding once at the end give
  different float32 results at more than 1 % of the points (asserted on the CPU, the oracle decides).

NaN points (kept as the reference has them, 0 / 0 in the radial rescale):
  * `project` at the centre of a SOLID sphere: dist = 0, sd = -r < 0, d / dist * r is NaN in all three components.
    (`evaluate` there is -r; a flipped sphere's centre has sd = +r and is not moved.)
  * `project` on the axis of a solid cylinder whose max(sd, y - hh, -(y + hh)) picks the radial candidate (radius < half
    height, "thin"): x / dist * r is 0 / 0; to_world then multiplies NaN by the zeros of the identity and all three
    components are NaN.  On the axis of a cylinder with radius > half height the cap wins and the point moves to the cap.

Bound for the generic points.  Kernel (contraction off) and oracle evaluate the same expressions in float64 and differ by
the last bit of a sqrt at most and by the rounding of the final store:  |got - want| <= (R + 2) 2^-53 M + u_out |want|.
M is the oracle's magnitude output (`mag=`): the largest intermediate magnitude, a length (for a frame change the sum of
the |terms| of a row); in `project` times the gain r / dist of every radial projection the point went through, which is what
a last-bit difference from an earlier body can have grown to.  R counts the rounded operations on the longest path of a
term (fabs, max, the halving of a size and negation are exact), from csrc/mfs_sdf.hip:
  to_body (:45-54), R = 5: a product, at most three accumulations into t3 or tmp, the add of t3.
  to_world (:57-64), R = 5: a product, three accumulations, the add of T.
  sphere_eval (:68-73), R = 6: difference, square, two adds, sqrt, - r.
  box_eval (:84-97), R = 12: to_body (5), |.| - h (1), square (1), three accumulations (3), sqrt (1), + max_disp (1).
  cylinder_eval (:125-143), R = 12: to_body (5), square, add, sqrt, - r (4), then beside a cap sd * sd, the add, sqrt (3).
  sphere_project (:75-82), R = 8: dist as above (5), / dist, * r, + T.
  box_project (:99-123), R = 12: to_body (5), h - prb (1), += (1), to_world (5).
  cylinder_project (:145-177), R = 15: to_body (5), square, add, sqrt (3), / dist, * r (2), to_world (5).
evaluate takes the largest R of the kinds in the table; project the sum over its rows, each body working on what the
previous one left.  float32 positions in `project` are compared with the oracle's per-body rounding instead: equal, or one
float32 ulp apart at no more than 1 % of the points (`f32_verdict`).

Planted mistakes (MISTAKES) are textual edits of copies of the oracle's functions.  Four of the comparisons cannot be
told apart from their neighbours by any input, and are listed as EQUIVALENT with the reason, next to a mistake of the same
comparison that can be caught.
"""
import functools
import inspect

import numpy as np
from scipy.spatial.transform import Rotation

from grid_kernels3d_inputs import U, ratio  # noqa: F401
from oracle import mfs_oracle as O

F32, F64 = np.float32, np.float64
MARGIN = 1e-6
R_TO_BODY, R_TO_WORLD = 5, 5
R_EVAL = {0: 6, 1: 12, 2: 12}                     # by kind = type code // 2
R_PROJECT = {0: 8, 1: 12, 2: 15}
MESH_CODE = 6
SPHERE, BOX, CYL = 0, 2, 4                        # type codes; + 1: flipped


def body(code, params, centre=(0, 0, 0), axis=(0, 1, 0), angle=0, vel=(0, 0, 0)):
    """one (10, 4) block in generate_rb's layout; angle in degrees, 0 leaves an exact identity"""
    rb = np.zeros((10, 4))
    rb[0, 0] = code
    rb[0, 1:1 + len(params)] = params
    rb[1:5] = np.identity(4)
    rb[1:4, 3] = centre
    rb[5:9] = np.identity(4)
    if angle:
        ax = np.asarray(axis, F64)
        rb[5:8, :3] = Rotation.from_rotvec(ax / np.linalg.norm(ax) * angle * np.pi / 180).as_matrix()
    rb[9, :3] = vel
    return rb


def table(*rows):
    t = np.stack(rows) if rows else np.zeros((0, 10, 4))
    t.setflags(write=False)
    return t


def r_evaluate(rb):
    return max([R_EVAL[int(c // 2)] for c in rb[:, 0, 0] if c // 2 <= 2], default=0)


def r_project(rb):
    return sum(R_PROJECT[int(c // 2)] for c in rb[:, 0, 0] if c // 2 <= 2)


# ------------------------------------------------------------------------------------------------------ generic ---
_GENERIC = [body(BOX + 1, (1.2, 1.0, 1.1), (0, 0.5, 0), (1, 1, 0), 10, (0.3, -0.2, 0.1)),
            body(SPHERE + 1, (0.7,), (0.01, 0.5, -0.02), (0, 1, 0), 0, (-0.1, 0.25, 0.4)),
            body(CYL + 1, (0.6, 0.8), (0, 0.5, 0), (1, 0, 0.3), 8, (0.05, 0.6, -0.3)),
            body(SPHERE, (0.2,), (0.2, 0.5, 0.1), (0, 1, 0), 0, (0.2, 0.1, -0.4)),
            body(BOX, (0.4, 0.3, 0.35), (-0.2, 0.4, 0.0), (0, 1, 1), 30, (-0.3, 0.15, 0.2)),
            body(CYL, (0.15, 0.5), (0.0, 0.6, -0.2), (1, 0, 1), 35, (0.12, -0.5, 0.33))]
_MESH_ROW = body(MESH_CODE, (0.9, 0.3, 0.2), (0.05, 0.5, 0.0), (1, 2, 3), 40, (7.0, 8.0, 9.0))   # covers the scene if read
GENERIC_TABLES = {"first": table(_MESH_ROW, *_GENERIC), "middle": table(*_GENERIC[:3], _MESH_ROW, *_GENERIC[3:]),
                  "last": table(*_GENERIC, _MESH_ROW)}
GENERIC_KNOWN = table(*_GENERIC)
N_GENERIC = 1500
COUNTS = [1, 255, 256, 257, N_GENERIC]


def _margins(rb, pos, dtype=F64):
    """per point the least gap that `evaluate` and `project` meet, at positions stored in `dtype`"""
    p = np.asarray(pos).astype(dtype)
    te, tp = {}, {}
    O.sdf_evaluate(rb, np.zeros(len(p)), np.zeros((len(p), 3)), p, trace=te)
    O.sdf_project(rb, p.copy(), trace=tp)
    return np.minimum(te["point_margin"], tp["point_margin"])


@functools.lru_cache(maxsize=None)
def generic_points():
    """N_GENERIC points (float64, read-only) in and around the generic bodies, a third of them close to the solid ones,
    none within MARGIN of a threshold whether stored in float64 or float32"""
    rng = np.random.default_rng(2024)
    wide = rng.uniform([-0.85, -0.25, -0.85], [0.85, 1.25, 0.85], size=(2 * N_GENERIC, 3))
    near = rng.uniform([-0.42, 0.22, -0.42], [0.42, 0.85, 0.22], size=(N_GENERIC, 3))
    pos = np.concatenate([wide, near])[rng.permutation(3 * N_GENERIC)]
    ok = (_margins(GENERIC_KNOWN, pos) > MARGIN) & (_margins(GENERIC_KNOWN, pos, F32) > MARGIN)
    pos = pos[ok][:N_GENERIC]
    assert len(pos) == N_GENERIC
    pos.setflags(write=False)
    return pos


# -------------------------------------------------------------------------------------------------------- exact ---
V = [(0.5, -0.25, 0.125), (-1.5, 2.0, 0.75), (3.0, 0.375, -0.625), (0.0625, 4.0, -2.5), (1.25, 1.75, 2.25),
     (-0.875, -3.5, 6.0), (2.5, -4.5, 8.5), (9.0, -0.5, 0.25), (-7.0, 1.5, 11.0)]
# solid bodies, far enough apart that each point belongs to one of them (the last two touch)
_SOLIDS = table(body(BOX, (1.0, 0.5, 0.25), (0, 0, 0), vel=V[0]),               # 0
                body(SPHERE, (0.625,), (2, 0, 0), vel=V[1]),                    # 1
                body(CYL, (0.625, 0.5), (0, 4, 0), vel=V[2]),                   # 2  radius > half height ("fat")
                body(CYL, (0.125, 1.0), (0, 8, 0), vel=V[3]),                   # 3  radius < half height ("thin")
                body(BOX, (0.5, 0.5, 0.5), (0, -2, 0), vel=V[4]),               # 4  a cube: all six faces tie at its centre
                body(SPHERE, (0.5,), (0, 16, 0), vel=V[5]),                     # 5, 6: coincident, different velocities
                body(SPHERE, (0.5,), (0, 16, 0), vel=V[6]),
                body(SPHERE, (0.5,), (0, 20, 0), vel=V[7]),                     # 7, 8: touch at (0.5, 20, 0)
                body(BOX, (1.0, 1.0, 1.0), (1, 20, 0), vel=V[8]))
_SOLID_POINTS = [
    ("box face", (0.5, 0.1, 0)), ("box face -x", (-0.5, 0.1, 0.0625)), ("box edge", (0.5, 0.25, 0)),
    ("box corner", (0.5, 0.25, 0.125)), ("box corner ---", (-0.5, -0.25, -0.125)),
    ("box inside, +x and +y tie", (0.4375, 0.1875, 0)), ("box inside, -x and -y tie", (-0.4375, -0.1875, 0)),
    ("box inside, +y and -z tie", (0, 0.1875, -0.0625)), ("cube centre, six faces tie", (0, -2, 0)),
    ("cube inside, -z nearest", (0, -2, -0.125)), ("box outside, off an edge", (0.875, 0.75, 0)),
    ("sphere surface", (2.375, 0.5, 0)), ("sphere surface on an axis", (2, 0.625, 0)), ("sphere centre", (2, 0, 0)),
    ("sphere inside", (2.1875, 0.25, 0)), ("sphere outside", (2.75, 1.0, 0)),
    ("fat cylinder rim", (0.375, 4.25, 0.5)), ("fat cylinder side", (0.375, 4, 0.5)), ("fat cylinder lower rim", (0.375, 3.75, 0.5)),
    ("fat cylinder cap plane inside the radius", (0.1, 4.25, 0.1)), ("fat cylinder lower cap plane inside", (0.1, 3.75, 0.1)),
    ("fat cylinder cap plane outside the radius", (0.75, 4.25, 1.0)), ("fat cylinder above the cap, inside", (0.375, 4.5, 0)),
    ("fat cylinder below the cap, outside", (0, 3.25, 1.0)), ("fat cylinder axis", (0, 4, 0)),
    ("fat cylinder axis, upper half", (0, 4.125, 0)), ("fat cylinder axis, lower half", (0, 3.875, 0)),
    ("fat cylinder inside, radial and top tie", (0.5, 4.125, 0)), ("fat cylinder inside, radial and bottom tie", (0.5, 3.875, 0)),
    ("fat cylinder inside, three-way tie", (0.375, 4, 0)), ("fat cylinder inside, radial wins", (0.5, 4, 0)),
    ("thin cylinder axis", (0, 8, 0)), ("thin cylinder inside, radial wins", (0.0625, 8.25, 0)),
    ("thin cylinder inside, top wins", (0.03125, 8.484375, 0)),
    ("coincident spheres, inside", (0.25, 16, 0)), ("coincident spheres, surface", (0, 16.5, 0)),
    ("sphere and box touch", (0.5, 20, 0)), ("farther than 100 from everything", (500, 0, 0)),
]
_FLIPPED_BOX = table(body(BOX + 1, (1.0, 0.5, 0.25), (0, 0, 0), vel=V[0]))
_FLIPPED_BOX_POINTS = [("flipped box face", (0.5, 0.1, 0)), ("flipped box edge", (0.5, 0.25, 0)),
                       ("flipped box corner", (-0.5, 0.25, -0.125)), ("flipped box inside, two faces tie", (0.4375, 0.1875, 0)),
                       ("flipped box outside one face", (0.75, 0.1, 0)), ("flipped box outside an edge", (0.875, -0.75, 0.0625)),
                       ("flipped box centre", (0, 0, 0)), ("far, a flipped body in the table", (500, 0, 0))]
_FLIPPED_SPHERE = table(body(SPHERE + 1, (0.625,), (2, 0, 0), vel=V[1]))
_FLIPPED_SPHERE_POINTS = [("flipped sphere surface", (2.375, 0.5, 0)), ("flipped sphere centre", (2, 0, 0)),
                          ("flipped sphere inside", (2.1875, 0.25, 0)), ("flipped sphere outside", (2.75, 1.0, 0)),
                          ("far, a flipped sphere in the table", (502, 0, 0))]
# radius 25/32 with the point (7/32, ., 24/32): dist == r exactly, and x / dist * r is one ulp off x, so that the rescale shows
_FLIPPED_CYL = table(body(CYL + 1, (0.78125, 0.5), (0, 4, 0), vel=V[2]))
_FLIPPED_CYL_POINTS = [("flipped cylinder rim", (0.21875, 4.25, 0.75)), ("flipped cylinder side", (0.21875, 4, 0.75)),
                       ("flipped cylinder beyond the rim's height, on the radius", (0.21875, 4.5, 0.75)),
                       ("flipped cylinder cap plane inside", (0.1, 4.25, 0.1)), ("flipped cylinder lower cap plane inside", (0.1, 3.75, 0.1)),
                       ("flipped cylinder above the cap, inside", (0.25, 4.5, 0)), ("flipped cylinder outside the radius", (0, 4.125, 1.5)),
                       ("flipped cylinder outside radius and cap", (0, 3.25, 1.15625)), ("flipped cylinder axis", (0, 4, 0)),
                       ("flipped cylinder inside", (0.25, 4.125, 0)), ("far, a flipped cylinder in the table", (500, 4, 0))]
# a solid box first: the far point takes no solid body, then the flipped one wins with a large negative distance
_MIXED = table(body(BOX, (1.0, 0.5, 0.25), (0, 0, 0), vel=V[0]), body(BOX + 1, (4.0, 4.0, 4.0), (0, 0, 0), vel=V[4]))
_MIXED_POINTS = [("far, solid then flipped", (500, 0, 0)), ("on the solid box inside the flipped one", (0.5, 0.1, 0)),
                 ("inside both", (0.25, 0.0625, 0))]


def _scene(rb, named):
    pts = np.array([p for _, p in named], F64)
    pts.setflags(write=False)
    return rb, pts, [n for n, _ in named]


EXACT_SCENES = {"solids": _scene(_SOLIDS, _SOLID_POINTS), "flipped box": _scene(_FLIPPED_BOX, _FLIPPED_BOX_POINTS),
                "flipped sphere": _scene(_FLIPPED_SPHERE, _FLIPPED_SPHERE_POINTS),
                "flipped cylinder": _scene(_FLIPPED_CYL, _FLIPPED_CYL_POINTS), "solid and flipped box": _scene(_MIXED, _MIXED_POINTS)}
# points that `project` turns into NaN (see the docstring), by scene
NAN_POINTS = {"solids": ["sphere centre", "thin cylinder axis"]}

# the node grid of evaluate_grid over the box and the sphere of "solids": dyadic everywhere, so the in-kernel position
# bound_min + (index + bias) * cell_size is exact; nodes lie on the box's faces, edges, corners and centre, on the sphere's
# centre and, with bias 0.5 along x only, elsewhere
GRID = dict(res=(7, 5, 5), bound_min=(-1.0, -0.5, -0.25), cell_size=(0.5, 0.25, 0.125), biases=((0, 0, 0), (0.5, 0, 0)))


def grid_nodes(bias):
    idx = np.stack(np.meshgrid(*[np.arange(r, dtype=F32) for r in GRID["res"]], indexing="ij"), axis=-1)
    return np.asarray(GRID["bound_min"], F64) + (idx + np.asarray(bias, F32)).astype(F64) * np.asarray(GRID["cell_size"], F64)


# -------------------------------------------------------------------------------------------------------- chain ---
CHAIN = table(body(SPHERE, (0.3,), (0, 0.5, 0), vel=V[0]),
              body(BOX, (0.5, 0.3, 0.4), (0.25, 0.55, 0.05), (1, 2, 0.5), 25, V[1]),
              body(CYL, (0.2, 0.5), (0.3, 0.75, 0.1), (1, 0, 1), 40, V[2]),
              body(SPHERE, (0.25,), (0.45, 0.9, 0.0), vel=V[3]))
N_CHAIN = 1200


@functools.lru_cache(maxsize=None)
def chain_points():
    """points in the union of the chain's bodies, clear of every threshold at both storage types"""
    rng = np.random.default_rng(77)
    pos = rng.uniform([-0.3, 0.2, -0.3], [0.7, 1.15, 0.4], size=(6 * N_CHAIN, 3))
    sd = np.zeros(len(pos))
    O.sdf_evaluate(CHAIN, sd, np.zeros((len(pos), 3)), pos)
    pos = pos[sd < -0.01]
    ok = (_margins(CHAIN, pos) > MARGIN) & (_margins(CHAIN, pos, F32) > MARGIN)
    pos = pos[ok][:N_CHAIN]
    assert len(pos) == N_CHAIN
    pos.setflags(write=False)
    return pos


# ------------------------------------------------------------------------------------------------ oracle calls ---
_CHAIN_OF_FUNCTIONS = ("_sdf_to_body", "_sdf_to_world", "_sdf_eval_one", "sdf_evaluate", "sdf_project")


@functools.lru_cache(maxsize=None)
def mistaken(fn, old, new, count=1):
    """the oracle's rigid-body functions, re-made in a namespace of their own in which the source of `fn` has `old`
    replaced by `new` (`old` must occur `count` times); the others are re-made unchanged, so that they call the copy"""
    ns = dict(vars(O))
    for name in _CHAIN_OF_FUNCTIONS:
        src = inspect.getsource(getattr(O, name))
        if name == fn:
            assert src.count(old) == count, (fn, old, src.count(old))
            src = src.replace(old, new)
        exec(compile(src, f"<{name}, with a planted mistake in {fn}>", "exec"), ns)
    return ns


def _ns(mistake):
    return vars(O) if mistake is None else mistaken(*mistake)


def evaluate(rb, pos, pdt=F64, mistake=None, trace=None):
    """(sd, vel, M) of the oracle at the positions stored in pdt; vel is zero where it is not written"""
    p = np.asarray(pos).astype(pdt)
    sd, vel, mag = np.zeros(len(p)), np.zeros((len(p), 3)), {}
    with np.errstate(all="ignore"):
        _ns(mistake)["sdf_evaluate"](np.asarray(rb), sd, vel, p, trace=trace, mag=mag)
    return sd, vel, mag["sd"]


def project(rb, pos, pdt=F64, mistake=None, trace=None, round_each=True):
    """(positions after the oracle's project at dtype pdt, M)"""
    p = np.array(pos).astype(pdt)
    mag = {}
    with np.errstate(all="ignore"):
        _ns(mistake)["sdf_project"](np.asarray(rb), p, trace=trace, mag=mag, round_each=round_each)
    return p, mag["position"]


# ------------------------------------------------------------------------------------------- the comparisons ---
_INT = {np.dtype(F32): np.int32, np.dtype(F64): np.int64}


def bit_mismatches(got, want):
    """boolean per element: not the same bits (a zero's sign counts), NaN matching any NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    same = got.view(_INT[got.dtype]) == want.view(_INT[want.dtype])
    return ~(same | (np.isnan(got) & np.isnan(want)))


def excess(got, want, M, R, odt=F64):
    """err / bound per element (`ratio`); M per point, broadcast over a point's components"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    M = np.asarray(M, F64).reshape(M.shape + (1,) * (want.ndim - np.ndim(M)))
    return ratio(got, want, np.broadcast_to(M, want.shape), R, U[odt], np.ones(want.shape, bool))


F32_SLACK_SHARE = 0.01


def f32_verdict(got, want):
    """(points more than one float32 ulp off in some component, share of points that differ at all) of float32 positions;
    the test wants 0 of the first and at most F32_SLACK_SHARE of the second.  NaN must match NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32
    both_nan = np.isnan(got) & np.isnan(want)
    with np.errstate(invalid="ignore"):
        off = np.abs(got.astype(F64) - want.astype(F64)) / np.spacing(np.abs(want)).astype(F64)
    off = np.where(both_nan, 0.0, np.where(np.isfinite(off), off, np.inf))
    return int((off > 1).any(axis=1).sum()), float((off > 0).any(axis=1).mean())


# ------------------------------------------------------------------------------------------------ the mistakes ---
_FACE_TESTS = '''                        if _tr(trace, "box_project h - prb < dist", h[k] - prb[k] < dist_xyz, h[k] - prb[k] - dist_xyz):
                            dist_xyz, index = h[k] - prb[k], k * 2
                        if _tr(trace, "box_project prb + h < dist", prb[k] + h[k] < dist_xyz, prb[k] + h[k] - dist_xyz):
                            dist_xyz, index = prb[k] + h[k], k * 2 + 1
'''
_FACE_TESTS_SWAPPED = "".join(_FACE_TESTS.splitlines(keepends=True)[k] for k in (2, 3, 0, 1))

# (name, (oracle function, old text, new text[, count]), where it must show: "generic" (err / bound), "exact" (bits) or "f32"
#  (the float32 chain), or "equivalent: reason")
MISTAKES = [
    ("d < min_sd to <=", ("sdf_evaluate", ", d < min_sd,", ", d <= min_sd,"), "exact"),
    ("min_sd <= 0 to < 0", ("sdf_evaluate", ", min_sd <= 0,", ", min_sd < 0,"), "exact"),
    ("start value 100 to 1000", ("sdf_evaluate", "min_sd, idx = 100, 0", "min_sd, idx = 1000, 0"), "exact"),
    ("R for R^T in to_body", ("_sdf_to_body", "Rm[j, i]", "Rm[i, j]", 4), "generic"),
    ("translation applied before the rotation", ("_sdf_to_body", "t3 -= Rm[j, i] * T[j, 3]", "t3 -= (i == j) * T[j, 3]"), "generic"),
    ("disp > 0 to >= 0", ("_sdf_eval_one", ", disp > 0, disp)", ", disp >= 0, disp)"),
     "equivalent: disp == 0 adds 0 * 0 to a sum that is +0.0 or positive"),
    ("disp > 0 dropped (every axis adds its square)", ("_sdf_eval_one", ", disp > 0, disp)", ", True, disp)"), "generic"),
    ("max_disp < 0 to <= 0", ("_sdf_eval_one", ", mx < 0, mx)", ", mx <= 0, mx)"),
     "equivalent: max_disp == 0 means no disp is positive, the root is +0.0 and adding 0 leaves it"),
    ("max_disp added whatever its sign", ("_sdf_eval_one", ", mx < 0, mx)", ", True, mx)"), "generic"),
    ("the two face tests of box_project swapped", ("sdf_project", _FACE_TESTS, _FACE_TESTS_SWAPPED), "exact"),
    ("a flipped box clamped only when in_out == 0", ("sdf_project", "if flipped:                                  # `% 2 and ~(in_out)`",
                                                     "if flipped and in_out == 0:  # `% 2 and ~(in_out)`"), "generic"),
    ("prb[1] > hh to >= (eval)", ("_sdf_eval_one", ", prb[1] > hh, prb[1] - hh)", ", prb[1] >= hh, prb[1] - hh)"),
     "equivalent: at prb[1] == hh the clipped height is hh on either side of the test"),
    ("prb[1] > hh to >= (project)", ("sdf_project", ", prb[1] > hh, prb[1] - hh)", ", prb[1] >= hh, prb[1] - hh)"),
     "equivalent: at prb[1] == hh the clipped height is hh on either side of the test"),
    ("prb[1] > hh compared with 0", ("_sdf_eval_one", ", prb[1] > hh, prb[1] - hh)", ", prb[1] > 0, prb[1] - hh)"), "generic"),
    ("the cap test by >= instead of ==", ("_sdf_eval_one", ", y_clip == hh) or", ", y_clip >= hh) or"),
     "equivalent: the clipped height never exceeds hh, so >= hh holds exactly where == hh does"),
    ("the lower cap test dropped", ("_sdf_eval_one", ', y_clip == hh) or _tr(trace, "cylinder_eval y_clip == -hh", y_clip == -hh)',
                                    ", y_clip == hh)"), "generic"),
    ("a flip sign dropped on the cylinder", ("_sdf_eval_one", "return -sd if flipped else sd", "return -sd if flipped and kind != 2 else sd"),
     "generic"),
    ("sd >= 0 to sd > 0 in the flipped cylinder's projection", ("sdf_project", ", sd >= 0, sd)", ", sd > 0, sd)"), "exact"),
    ("mv == prb[1] - hh answering -hh", ("sdf_project", "mv == prb[1] - hh):\n                        prb[1] = hh",
                                         "mv == prb[1] - hh):\n                        prb[1] = -hh"), "generic"),
    ("no float32 rounding between bodies", ("sdf_project", "if round_each:", "if False:"), "f32"),
    ("the sphere projected to radius p[2]", ("sdf_project", "pos = d / dist * rb[0, 1] + c", "pos = d / dist * rb[0, 2] + c"), "generic"),
    ("an unknown type code read as a cylinder (evaluate)", ("sdf_evaluate", "if int(rb_d[i, 0, 0] // 2) > 2:", "if False:"), "generic"),
    ("an unknown type code read as a cylinder (project)", ("sdf_project", "elif kind == 2:", "else:"), "generic"),
]
