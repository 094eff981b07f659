"""Test meshes and the numpy oracle for triangle-mesh solids (mfs/meshsdf.py, solver/sdf3D.py MeshBody, csrc/mfs_meshsdf.hip).

Meshes are generated, never stored: closed, outward oriented (counter-clockwise seen from outside), float32 vertices.
The oracle is independent of the kernels where that matters: distance = brute force over all triangles as the minimum of
the three segment distances and, where the projection falls inside, the plane distance (the kernel walks Ericson's
regions); sign = the generalised winding number (the solid-angle sum; the kernel counts ray crossings).  The trilinear
sampling, the union rule and the projection are restated operation by operation in float64.
"""
import numpy as np


# ------------------------------------------------------------------------------------------------------ meshes ----
def _outward(v, f):
    """flip all faces if the signed volume is negative"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    return v.astype(np.float32), (f if vol > 0 else f[:, ::-1]).astype(np.int32).copy()


def icosphere(subdivisions, radius=1.0):
    t = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        cache, nf = {}, []

        def mid(i, j):
            key = (min(i, j), max(i, j))
            if key not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return _outward(np.asarray(v) * radius, np.asarray(f))


def box(size=(1.0, 1.0, 1.0), center=(0.0, 0.0, 0.0)):
    h = np.asarray(size, np.float64) / 2
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64) * h + np.asarray(center)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return _outward(v, np.asarray(f))


def octahedron(radius=1.0):
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * radius
    f = []
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                odd = (sx + sy + sz) % 2
                f.append((sx, sy, sz) if not odd else (sx, sz, sy))
    return _outward(v, np.asarray(f))


def torus(R=1.0, r=0.4, nu=16, nv=12):
    """around axis 2: a ray along axis 0 through the hole crosses the surface four times"""
    u, w = np.meshgrid(np.arange(nu) * 2 * np.pi / nu, np.arange(nv) * 2 * np.pi / nv, indexing="ij")
    v = np.stack([(R + r * np.cos(w)) * np.cos(u), (R + r * np.cos(w)) * np.sin(u), r * np.sin(w)], axis=-1).reshape(-1, 3)
    idx = lambda i, j: (i % nu) * nv + (j % nv)  # noqa: E731
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(a, b, c), (a, c, d)]
    return _outward(v, np.asarray(f))


def l_prism():
    """An L (unit squares (0..2, 0..1) and (0..1, 0..2)) mapped by (x, y) -> (x - y, x + y), so that its arms point up
    along axis 1 at 45 degrees, in the plane of axes (0, 1); extruded over 0..1 along axis 2.  All coordinates are
    integers.  A ray along axis 0 at height 2 < x1 < 3 crosses four times; the ray at x1 = 2 starts and ends on a convex
    edge and passes through the re-entrant edge (0, 2, .); the ray at x1 = 3 touches the two tip edges.  20 triangles."""
    poly = np.array([(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)], np.float64)
    poly = np.stack([poly[:, 0] - poly[:, 1], poly[:, 0] + poly[:, 1]], axis=1)
    n = len(poly)
    v = np.concatenate([np.c_[poly, np.zeros(n)], np.c_[poly, np.ones(n)]])
    f = []
    for k in range(1, n - 1):                      # the fan about corner 0 stays inside the L
        f += [(0, k + 1, k), (n, n + k, n + k + 1)]
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, n + j), (i, n + j, n + i)]
    return _outward(v, np.asarray(f))


MESHES = {"icosphere": lambda: icosphere(2, 1.0), "box": lambda: box((1.0, 1.5, 0.75)), "octahedron": lambda: octahedron(1.0),
          "torus": lambda: torus(), "l_prism": l_prism}


def with_split_triangle(v, f, k=0):
    """triangle k cut in two through the midpoint of its edge (a, b) -- and the neighbour across that edge as well, so the
    surface stays a closed manifold without a T-junction: F + 2 triangles"""
    v, f = v.astype(np.float64), [tuple(t) for t in f]
    a, b, c = f[k]
    m = len(v)
    v = np.concatenate([v, [(v[a] + v[b]) / 2]])
    nb = next(i for i, t in enumerate(f) if i != k and a in t and b in t)
    t = f[nb]
    d = next(x for x in t if x not in (a, b))
    out = [x for i, x in enumerate(f) if i not in (k, nb)] + [(a, m, c), (m, b, c), (b, m, d), (m, a, d)]
    return v.astype(np.float32), np.asarray(out, np.int32)


def with_zero_area_triangle(v, f):
    """one more triangle (a, b, b): the edge (a, b) of triangle 0 as a triangle of zero area"""
    a, b, _ = f[0]
    return v, np.concatenate([f, [[a, b, b]]]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------ oracle ----
def lattice_nodes(shape, origin, spacing):
    """(n0, n1, n2, 3) float64 node positions, origin + index * spacing"""
    ax = [np.float64(origin[k]) + np.arange(shape[k], dtype=np.float64) * np.float64(spacing) for k in range(3)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _segment_d2(p, a, b):
    ab = b - a
    den = _dot(ab, ab)
    t = _dot(p - a, ab) / den if den > 0 else p.dtype.type(0)
    t = np.clip(t, 0, 1)
    q = p - (a + t[..., None] * ab) if den > 0 else p - a
    return _dot(q, q)


def distance(points, v, f, dtype=np.float64):
    """unsigned distance of every point to the mesh by brute force, all arithmetic in `dtype`"""
    p = np.asarray(points).reshape(-1, 3).astype(dtype)
    tri = v.astype(dtype)[f]
    best = np.full(len(p), np.inf, dtype)
    for a, b, c in tri:
        d2 = np.minimum(np.minimum(_segment_d2(p, a, b), _segment_d2(p, b, c)), _segment_d2(p, c, a))
        n = np.cross(b - a, c - a)
        nn = _dot(n, n)
        if nn > 0:
            inside = ((_dot(np.cross(b - a, p - a), n) >= 0) & (_dot(np.cross(c - b, p - b), n) >= 0)
                      & (_dot(np.cross(a - c, p - c), n) >= 0))
            dp = _dot(p - a, n)
            d2 = np.where(inside, dp * dp / nn, d2)
        best = np.minimum(best, d2)
    return np.sqrt(best).reshape(np.asarray(points).shape[:-1])


def winding_number(points, v, f):
    """generalised winding number (Van Oosterom and Strackee's solid angle of every triangle, summed, over 4 pi): 1 inside
    a closed outward-oriented surface, 0 outside"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    total = np.zeros(len(p))
    for a, b, c in v.astype(np.float64)[f]:
        a, b, c = a - p, b - p, c - p
        la, lb, lc = (np.sqrt(_dot(x, x)) for x in (a, b, c))
        num = _dot(a, np.cross(b, c))
        den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
        total += 2.0 * np.arctan2(num, den)
    return (total / (4 * np.pi)).reshape(np.asarray(points).shape[:-1])


def signed_distance(points, v, f):
    d = distance(points, v, f)
    return np.where(winding_number(points, v, f) > 0.5, -d, d)


def box_sdf(points, size, center=(0.0, 0.0, 0.0)):
    q = np.abs(np.asarray(points, np.float64) - np.asarray(center)) - np.asarray(size, np.float64) / 2
    return np.sqrt((np.maximum(q, 0) ** 2).sum(axis=-1)) + np.minimum(q.max(axis=-1), 0)


def max_facet_half_angle(v, f):
    """largest angle between a facet's corner direction and its circumcentre direction, for a mesh inscribed in a sphere
    about the origin: every facet lies beyond r cos(theta) from the centre"""
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1)[:, None]
    r = np.linalg.norm(a, axis=1)
    return float(np.arccos(np.clip(_dot(a, n) / r, -1, 1)).max())


# ------------------------------------------------------------------- posed bodies: restatement of the kernels ----
def grid_positions(res, bound_min, cell_size, bias):
    """evaluate_grid's rule: (double)(float)bound_min + (double)((float)i + (float)bias) * cell_size"""
    ax = []
    for k in range(3):
        i = np.arange(res[k], dtype=np.float32) + np.float32(bias[k])
        ax.append(np.float64(np.float32(bound_min[k])) + i.astype(np.float64) * np.float64(cell_size[k]))
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def to_body(row, x):
    """x_b = R^T (x - T) for one (10, 4) row"""
    T, R = row[1:4, 3], row[5:8, :3]
    d = x - T
    return np.stack([(R[0, i] * d[..., 0] + R[1, i] * d[..., 1]) + R[2, i] * d[..., 2] for i in range(3)], axis=-1)


def sample(vol, origin, h, xb, gradient=False):
    """trilinear sample of the float32 volume at body-frame points; outside: the sample at the clamped point plus the distance
    to the volume's box.  gradient=True: also the gradient of that function (body frame)."""
    vol = np.asarray(vol)
    assert vol.dtype == np.float32
    n = vol.shape
    h = np.float64(h)
    c, fr, e, inside = [], [], [], []
    for k in range(3):
        t = (xb[..., k] - np.float64(origin[k])) / h
        tc = np.minimum(np.maximum(t, 0.0), np.float64(n[k] - 1))
        ci = np.minimum(np.floor(tc).astype(np.int64), n[k] - 2)
        c.append(ci)
        fr.append(tc - ci.astype(np.float64))
        e.append((t - tc) * h)
        inside.append(t == tc)
    V = lambda a, b, d: vol[c[0] + a, c[1] + b, c[2] + d].astype(np.float64)  # noqa: E731
    f0, f1, f2 = fr
    g0, g1, g2 = 1.0 - f0, 1.0 - f1, 1.0 - f2
    c00, c01 = V(0, 0, 0) * g2 + V(0, 0, 1) * f2, V(0, 1, 0) * g2 + V(0, 1, 1) * f2
    c10, c11 = V(1, 0, 0) * g2 + V(1, 0, 1) * f2, V(1, 1, 0) * g2 + V(1, 1, 1) * f2
    c0, c1 = c00 * g1 + c01 * f1, c10 * g1 + c11 * f1
    dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    value = (c0 * g0 + c1 * f0) + dist
    if not gradient:
        return value
    a00, a01 = V(0, 0, 0) * g1 + V(0, 1, 0) * f1, V(0, 0, 1) * g1 + V(0, 1, 1) * f1
    a10, a11 = V(1, 0, 0) * g1 + V(1, 1, 0) * f1, V(1, 0, 1) * g1 + V(1, 1, 1) * f1
    g = [np.where(inside[0], (c1 - c0) / h, 0.0),
         np.where(inside[1], ((c01 - c00) * g0 + (c11 - c10) * f0) / h, 0.0),
         np.where(inside[2], ((a01 - a00) * g0 + (a11 - a10) * f0) / h, 0.0)]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = [np.where(dist > 0, gk + ek / dist, gk) for gk, ek in zip(g, e)]
    return value, np.stack(g, axis=-1)


def union(rows, volumes, sd, vel, pos, rb_w=None):
    """sd / vel (float64 copies of what the arrays hold on entry) after every body in turn: d < sd -> sd = d,
    vel = v + w x (x - T) where d <= 0 else 0.  volumes: [(vol, origin, spacing), ...].  Returns (sd, vel, winner) with
    winner = -1 where no body won."""
    sd, vel = np.array(sd, np.float64), np.array(vel, np.float64)
    winner = np.full(sd.shape, -1)
    for i, (row, (vol, origin, h)) in enumerate(zip(rows, volumes)):
        d = sample(vol, origin, h, to_body(row, pos))
        win = d < sd
        sd = np.where(win, d, sd)
        winner = np.where(win, i, winner)
        v = np.broadcast_to(row[9, :3], pos.shape).copy()
        if rb_w is not None:
            w, x = rb_w[i], pos - row[1:4, 3]
            v = np.stack([row[9, 0] + (w[1] * x[..., 2] - w[2] * x[..., 1]), row[9, 1] + (w[2] * x[..., 0] - w[0] * x[..., 2]),
                          row[9, 2] + (w[0] * x[..., 1] - w[1] * x[..., 0])], axis=-1)
        v = np.where((d <= 0)[..., None], v, 0.0)
        vel = np.where(win[..., None], v, vel)
    return sd, vel, winner


def project(rows, volumes, position):
    """positions after every body in turn; float32 positions round per body.  Returns (positions, moved mask)."""
    dtype = position.dtype
    pos = position.astype(np.float64)
    moved = np.zeros(len(pos), bool)
    for row, (vol, origin, h) in zip(rows, volumes):
        R = row[5:8, :3]
        xb = to_body(row, pos)
        d, g = sample(vol, origin, h, xb, gradient=True)
        nn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        flat = (d < 0) & ~(nn > 0)
        if flat.any():
            for k in range(3):
                step = np.zeros(3)
                step[k] = h
                g[flat, k] = sample(vol, origin, h, xb[flat] + step) - sample(vol, origin, h, xb[flat] - step)
            nn = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        act = (d < 0) & (nn > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            n = g / nn[:, None]
        new = pos.copy()
        for k in range(3):
            nw = (R[k, 0] * n[:, 0] + R[k, 1] * n[:, 1]) + R[k, 2] * n[:, 2]
            new[:, k] = pos[:, k] - d * nw
        new = new.astype(dtype).astype(np.float64)
        pos = np.where(act[:, None], new, pos)
        moved |= act
    return pos.astype(dtype), moved


def straight_move_interval(vol, origin, h, xb0, xb1):
    """Bounds that need no restatement of the projection.  f, the trilinear interpolant of `vol`, changes along the straight
    move xb0 -> xb1 (body frame, both inside the volume) by |xb1 - xb0| times an average of grad f . u, u the unit direction.
    Component k of grad f at any point of a cell is a convex combination of that cell's four k-edge differences / h, so over
    the cells the segment's bounding box touches it lies in [a_k, b_k], the range of those differences, and
    grad f . u in [m, M] = sum_k [min, max](a_k u_k, b_k u_k).  Returns (lo, hi, G): f(xb1) in [f(xb0) + lo, f(xb0) + hi],
    and G >= |grad f| there (for the effect of rounding xb1)."""
    vol = np.asarray(vol, np.float64)
    n = np.array(vol.shape)
    lo, hi, G = (np.zeros(len(xb0)) for _ in range(3))
    for p, (x0, x1) in enumerate(zip(xb0, xb1)):
        c0 = np.clip(np.floor((np.minimum(x0, x1) - origin) / h).astype(int), 0, n - 2)
        c1 = np.clip(np.floor((np.maximum(x0, x1) - origin) / h).astype(int), 0, n - 2)
        sub = vol[c0[0]:c1[0] + 2, c0[1]:c1[1] + 2, c0[2]:c1[2] + 2]
        step = x1 - x0
        length = np.sqrt((step * step).sum())
        u = step / length if length > 0 else np.zeros(3)
        for k in range(3):
            d = np.diff(sub, axis=k) / h
            a, b = d.min(), d.max()
            lo[p] += min(a * u[k], b * u[k]) * length
            hi[p] += max(a * u[k], b * u[k]) * length
            G[p] += max(abs(a), abs(b)) ** 2
    return lo, hi, np.sqrt(G)
