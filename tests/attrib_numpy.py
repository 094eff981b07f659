"""The float64 oracle of mfs.attrib (csrc/mfs_attrib.hip): every query against every particle.

Definition.  Particles x_i carry values a_i, rounded to float32 on load; queries y_q; influence radius R.  d = x_i - y_q,
t = 1 - |d|^2 / R^2, w_qi = t^3 where t > 0, otherwise 0 (strict); K_q = #{i: w_qi > 0}, W_q = sum_i w_qi,
A_q = sum_i w_qi a_i / W_q where W_q > 0 and `fill` where W_q == 0.  A particle whose position is not finite adds nothing;
a query that is not finite or lies outside the box (default: the bounding box of the finite queries) is uncovered.
The bins (cubic, edge R, origin lo - R, m_a = floor((hi_a - lo_a) / R) + 3) cover every point within R of the box, so they
do not show in the definition: `gather` has none.

`gather32` restates the kernel's operation sequence in float32: positions relative to the low corner of the query's bin,
subtracted in float64 and rounded to float32; d, |d|^2, t = max(1 - |d|^2 * float32(1 / R^2), 0), w = t t t in float32; W
and the C sums accumulated in float32 in the kernel's order (ascending bin key, the caller's order inside a bin).

The band: the queries with some |t_qi| <= band_eps -- a rounding could turn whether that particle contributes, and with
it whether the query is covered.  band_eps = 32 u32 + 64 eps64 max(1, max |x - origin| / R): the first term covers the
float32 evaluation of t (error below 20 u32, see `bound`), the second the float64 subtraction of the bin's corner, scaled
by magnitude as tests/seed_numpy.py scales its band.

The bound, per query and channel, u32 = 2^-24 (derivation: DESIGN.md 4.17):

    u32 * [ C1 sum_i t_i^2 |a_i - A_q| / W_q  +  (2 K_q + C2) sum_i w_i |a_i| / W_q ],      C1 = 64, C2 = 8.

First term, the weights' rounding at the rim: a bin-relative coordinate is below 2 R in magnitude, so rounding the
particle's and the query's to float32 and subtracting them costs at most (2 + 1 + 1) u32 R per component of d, hence
2 |d| sqrt(3) 4 u32 R <= 14 u32 R^2 in |d|^2, plus 3 u32 for its products and sums, 2 u32 for float32(1 / R^2) and the
product, 1 u32 for the subtraction from 1: |dt| <= 20 u32, and dw = 3 t^2 dt + 2 u32 w for the two products.  A weight
error dw_i moves A by dw_i (a_i - A) / W: 60 u32 sum t_i^2 |a_i - A| / W, C1 = 64 leaves room for second order, and the
2 u32 w_i |a_i - A| part is at most 4 u32 sum w |a| / W.  Second term: K fused multiply-adds into each sum (a zero weight
adds exactly zero and costs no rounding) are K u32 sum w |a| for the numerator and (K - 1) u32 W |A| for the denominator,
the values' rounding to float32 and the quotient one u32 each: (2 K + 1) + 4 = 2 K + 5 <= 2 K + C2.
"""
import numpy as np

import skin_numpy as SK

U32 = 2.0 ** -24
EPS64 = float(np.finfo(np.float64).eps)
C1, C2 = 64.0, 8.0
F32 = np.float32


def lattice(box, R):
    """(origin, shape): origin = lo - R, m_a = floor((hi_a - lo_a) / R) + 3"""
    lo, hi = (np.asarray(v, np.float64) for v in box)
    return lo - np.float64(R), tuple(int(np.floor((b - a) / np.float64(R))) + 3 for a, b in zip(lo, hi))


def cells(x, origin, shape, R):
    """(bin indices (N, 3) int64, key (N,) int64): the sentinel key prod(shape) outside the lattice or not finite"""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        c = np.floor((x - origin) / np.float64(R))
        ok = ((c >= 0) & (c <= np.asarray(shape, np.float64) - 1)).all(axis=1)
    c = np.where(ok[:, None], c, 0).astype(np.int64)
    key = np.where(ok, (c[:, 0] * shape[1] + c[:, 1]) * shape[2] + c[:, 2], int(np.prod(shape)))
    return c, key


def default_box(points):
    """the bounding box of the finite queries, None when there is none"""
    y = np.asarray(points, np.float64).reshape(-1, 3)
    y = y[np.isfinite(y).all(axis=1)]
    return (y.min(axis=0), y.max(axis=0)) if len(y) else None


def _inside(points, box):
    y = np.asarray(points, np.float64).reshape(-1, 3)
    if box is None:
        return np.zeros(len(y), bool)
    with np.errstate(invalid="ignore"):
        return np.isfinite(y).all(axis=1) & (y >= np.asarray(box[0], np.float64)).all(axis=1) & \
            (y <= np.asarray(box[1], np.float64)).all(axis=1)


def pair_t(px, points, R):
    """t (Q, P) float64; -inf for a particle or a query that is not finite or a query outside... (the caller masks)"""
    x, y = np.asarray(px, np.float64).reshape(-1, 3), np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = x[None, :, :] - y[:, None, :]
        t = 1.0 - ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / (np.float64(R) * np.float64(R))
    return np.where(np.isfinite(t), t, -np.inf)


def gather(px, values, points, R, box=None, fill=np.nan):
    """dict: K (Q,) int, W (Q,), A (Q, C) float64 (`fill` where K == 0), t (Q, P), inside (Q,), box, bound (Q, C),
    band (Q,) bool, eps"""
    px = np.asarray(px, np.float64).reshape(-1, 3)
    y = np.asarray(points, np.float64).reshape(-1, 3)
    a = np.asarray(values).reshape(len(px), -1).astype(F32).astype(np.float64)
    if box is None:
        box = default_box(y)
    inside = _inside(y, box)
    t = pair_t(px, y, R)
    t[~inside] = -np.inf
    w = np.where(t > 0, t * t * t, 0.0)
    K, W = (w > 0).sum(axis=1), w.sum(axis=1)
    A = np.full((len(y), a.shape[1]), np.float64(fill))
    bound = np.zeros_like(A)
    cov = np.flatnonzero(K > 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(a.shape[1]):
            ac = np.where(w[cov] > 0, a[None, :, c], 0.0)                # 0 * NaN of a particle out of reach must not count
            A[cov, c] = (w[cov] * ac).sum(axis=1) / W[cov]
            rim = (np.where(w[cov] > 0, t[cov] ** 2, 0.0) * np.abs(ac - A[cov, c][:, None])).sum(axis=1) / W[cov]
            mass = (w[cov] * np.abs(ac)).sum(axis=1) / W[cov]
            bound[cov, c] = U32 * (C1 * rim + (2.0 * K[cov] + C2) * mass)
    origin = np.zeros(3) if box is None else lattice(box, R)[0]
    finite = px[np.isfinite(px).all(axis=1)]
    reach = max([1.0] + [float(np.abs(v - origin).max()) / R for v in (finite, y[inside]) if len(v)])
    eps = 32.0 * U32 + 64.0 * EPS64 * reach
    band = (np.abs(t) <= eps).any(axis=1) if t.shape[1] else np.zeros(len(y), bool)
    return dict(K=K, W=W, A=A, t=t, inside=inside, box=box, bound=bound, band=band, eps=eps)


def gather32(px, values, points, R, box=None, fill=np.nan, mutant=None):
    """(A (Q, C) float32, W (Q,) float32): the kernel's operation sequence in float32.
    mutant: None; "t2": w = t^2; "drop_bin": the neighbour bin (0, 0, +1) of every query is left out."""
    px = np.asarray(px, np.float64).reshape(-1, 3)
    y = np.asarray(points, np.float64).reshape(-1, 3)
    a = np.asarray(values).reshape(len(px), -1).astype(F32)
    Q, C = len(y), a.shape[1]
    A, W = np.full((Q, C), F32(fill)), np.zeros(Q, F32)
    if box is None:
        box = default_box(y)
    live = np.flatnonzero(_inside(y, box))
    if box is None or not len(live) or not len(px):
        return A, W
    origin, shape = lattice(box, R)
    qc, _ = cells(y[live], origin, shape, R)
    pc, pkey = cells(px, origin, shape, R)
    corner = origin + qc.astype(np.float64) * np.float64(R)
    y32 = (y[live] - corner).astype(F32)
    inv = F32(1.0 / (np.float64(R) * np.float64(R)))
    Wl, S = np.zeros(len(live), F32), np.zeros((len(live), C), F32)
    for i in np.argsort(pkey, kind="stable"):
        if pkey[i] == int(np.prod(shape)):
            break                                                        # the sentinel sorts last: not finite, or outside
        near = (np.abs(pc[i] - qc) <= 1).all(axis=1)
        if mutant == "drop_bin":
            near &= ~((pc[i, 0] == qc[:, 0]) & (pc[i, 1] == qc[:, 1]) & (pc[i, 2] == qc[:, 2] + 1))
        p32 = (px[i] - corner).astype(F32)
        d = p32 - y32
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t = np.maximum(F32(1.0) - d2 * inv, F32(0.0))
        w = np.where(near, t * t if mutant == "t2" else t * t * t, F32(0.0)).astype(F32)
        Wl = Wl + w
        with np.errstate(invalid="ignore", over="ignore"):
            S = S + w[:, None] * np.where(w[:, None] > 0, a[i][None, :], F32(0.0))
    cov = Wl > 0
    with np.errstate(invalid="ignore", over="ignore"):
        A[live[cov]] = S[cov] / Wl[cov][:, None]
    W[live] = Wl
    return A, W


def excess(A, ref):
    """(Q, C): |A - A_ref| / bound at the covered queries (0 where both are the same non-finite value), 0 elsewhere"""
    cov = ref["K"] > 0
    out = np.zeros(ref["A"].shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(np.asarray(A, np.float64)[cov] - ref["A"][cov]) / ref["bound"][cov]
    same = (np.asarray(A, np.float64)[cov] == ref["A"][cov]) | (np.isnan(A[cov]) & np.isnan(ref["A"][cov]))
    out[cov] = np.where(same, 0.0, np.where(np.isnan(e), np.inf, e))
    return out


# ------------------------------------------------------------------------------------------------------ the cases ----
H = 0.05
R = 2.5 * H
OFFSET = np.array([1.0, 2.0, 0.5])


def cloud_values(px, seed=5):
    """(P, 4) float64: a speed (>= 0), a signed field, a field linear in x, a field with an offset far above its spread"""
    rng = np.random.default_rng(seed)
    n = len(px)
    return np.stack([np.abs(rng.standard_normal(n)) * 2.0, rng.standard_normal(n), 3.0 * px[:, 0] - 1.0,
                     100.0 + 0.1 * rng.standard_normal(n)], axis=1)


def case_cloud(seed=0):
    """the 1680-particle jittered cloud of tests/skin_numpy.py at OFFSET; 2000 queries that reach R beyond it on every side"""
    px = SK.cloud() + OFFSET
    rng = np.random.default_rng(100 + seed)
    lo, hi = px.min(axis=0) - R, px.max(axis=0) + R
    return px, cloud_values(px), lo + (hi - lo) * rng.random((2000, 3)), R, None


def case_crowded_bin():
    """600 particles inside one bin (three LDS batches, the last partial), queries in and around it"""
    rng = np.random.default_rng(7)
    px = OFFSET + 0.3 * R + 0.4 * R * rng.random((600, 3))
    q = OFFSET - 0.9 * R + 2.8 * R * rng.random((150, 3))
    box = (OFFSET - R, OFFSET + 2.0 * R)                                # the particles' bin is [OFFSET, OFFSET + R)
    return px, cloud_values(px), q, R, box


def case_crowded_queries():
    """300 queries inside one bin (two work items, the second partial) among 200 particles"""
    rng = np.random.default_rng(8)
    px = OFFSET - R + 3.0 * R * rng.random((200, 3))
    q = OFFSET + 0.05 * R + 0.9 * R * rng.random((300, 3))
    return px, cloud_values(px), q, R, (OFFSET, OFFSET + R)


def case_one_point():
    """all queries at one point: the smallest lattice, (3, 3, 3)"""
    rng = np.random.default_rng(9)
    px = OFFSET - 1.5 * R + 3.0 * R * rng.random((300, 3))
    return px, cloud_values(px), np.tile(OFFSET + 0.25 * R, (40, 1)), R, None


def case_faces():
    """an explicit box: queries on its faces and corners (inside), just beyond them and far away (uncovered)"""
    px = SK.cloud() + OFFSET
    lo, hi = px.min(axis=0) + 0.1, px.max(axis=0) - 0.1
    rng = np.random.default_rng(11)
    q = lo + (hi - lo) * rng.random((240, 3))
    for k in range(3):
        q[20 * k:20 * k + 10, k] = lo[k]
        q[20 * k + 10:20 * k + 20, k] = hi[k]
    q[60], q[61] = lo, hi
    q[62:92] = q[0:30] + np.where(q[0:30] == lo, -1e-9, 0.0) + np.where(q[0:30] == hi, 1e-9, 0.0)     # just outside
    q[92] = hi + 10.0
    q[93] = lo - 1e6
    return px, cloud_values(px), q, R, (lo, hi)


def case_non_finite():
    """NaN and inf among the queries and the particles; a NaN and an inf value on contributing particles"""
    px, vals, q, r, _ = case_cloud(seed=1)
    px, vals, q = px.copy(), vals.copy(), q[:400].copy()
    px[5], px[17, 1], px[900, 2] = np.nan, np.inf, -np.inf
    q[3], q[8, 0], q[11, 2] = np.nan, np.inf, -np.inf
    vals[100, 0], vals[200, 1], vals[300, 2] = np.nan, np.inf, np.nan
    vals[5] = np.nan                                                     # on a particle that adds nothing
    return px, vals, q, r, None


def case_exactly_R():
    """dyadic coordinates: a particle exactly R = 0.25 from a query does not contribute (strict), one just inside does"""
    px = np.array([[1.0, 2.0, 0.5], [1.5, 2.0, 0.5], [1.5, 2.25, 0.5], [3.0, 2.0, 0.5]])
    vals = np.array([[1.0, 0, 0, 0], [2.0, 1, 0, 0], [4.0, 0, 1, 0], [8.0, 0, 0, 1]])
    q = np.array([[1.25, 2.0, 0.5],            # exactly R from particle 0: uncovered
                  [1.125, 2.0, 0.5],           # particle 0 alone
                  [1.5, 2.125, 0.5],           # the midpoint of particles 1 and 2: their mean
                  [1.5, 2.0, 0.75],            # exactly R from particle 1, sqrt(2) R from particle 2: uncovered
                  [2.75, 2.0, 0.5],            # exactly R from particle 3
                  [2.875, 2.0, 0.5]])
    return px, vals, q, 0.25, None


CASES = {"cloud": case_cloud, "crowded_bin": case_crowded_bin, "crowded_queries": case_crowded_queries,
         "one_point": case_one_point, "faces": case_faces, "non_finite": case_non_finite, "exactly_R": case_exactly_R}
