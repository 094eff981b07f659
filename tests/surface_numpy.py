"""Numpy restatement of the surface-extraction contract (DESIGN.md "Surface extraction"; test helper, plain loops).

Independent of csrc/mfs_surface.hip on purpose: the kernels orient faces by the parity of a permutation, this file by
geometry -- it puts every vertex at its edge's MIDPOINT, takes the face normal there and compares it with the direction
from the simplex's inside corners to its outside corners.  (Midpoints, not the true positions: an exact hit puts several
vertices on one point and leaves no normal to look at; orientation is combinatorial.)  `closed` is np.pad with `outside`.
Also the checkers of the tests: closed manifold, Euler characteristic, signed volume, canonical face order, and the 2D
analogues.
"""
import itertools

import numpy as np

SLOTS3 = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
SLOTS2 = ((1, 0), (0, 1), (1, 1))


def _chains(dim):
    """corner chains of the Kuhn simplices of the unit cell: c, c+e_p1, c+e_p1+e_p2, ..."""
    out = []
    for perm in itertools.permutations(range(dim)):
        c = np.zeros(dim, np.int64)
        chain = [tuple(c)]
        for a in perm:
            c = c.copy()
            c[a] += 1
            chain.append(tuple(c))
        out.append(chain)
    return out


def _vertices(phi, level, origin, spacing, slots, want_normals, ext):
    """one vertex per owned edge whose ends differ: nodes of the (padded) lattice in C order, then slots.  `ext`: width of
    the padding -- lattice node p is array index p - ext.  Returns positions (fp64), the map (node, slot) -> index, the
    normals (or None) and the inside flags."""
    dim = phi.ndim
    inside = phi < level                                    # NaN < level is False
    grads = None
    if want_normals:
        grads = np.zeros(phi.shape + (dim,))
        for d in range(dim):
            n = phi.shape[d]
            for i in range(n):
                lo, hi = max(i - 1, 0), min(i + 1, n - 1)
                sl_lo = [slice(None)] * dim
                sl_hi = [slice(None)] * dim
                sl_i = [slice(None)] * dim
                sl_lo[d], sl_hi[d], sl_i[d] = lo, hi, i
                grads[tuple(sl_i) + (d,)] = (phi[tuple(sl_hi)] - phi[tuple(sl_lo)]) / ((hi - lo) * spacing[d])
    pos, nrm, index = [], [], {}
    for p in np.ndindex(*phi.shape):
        for s_i, s in enumerate(slots):
            q = tuple(a + b for a, b in zip(p, s))
            if any(q[d] >= phi.shape[d] for d in range(dim)) or inside[p] == inside[q]:
                continue
            t = (level - phi[p]) / (phi[q] - phi[p])
            index[(p, s_i)] = len(pos)
            pos.append(origin + (np.asarray(p, np.float64) - ext + t * np.asarray(s, np.float64)) * spacing)
            if want_normals:
                g = (1.0 - t) * grads[p] + t * grads[q]
                ln = np.sqrt((g * g).sum())
                nrm.append(g / ln if ln > 0 else np.zeros(dim))
    pos = np.array(pos, np.float64).reshape(-1, dim)
    return pos, index, (np.array(nrm, np.float64).reshape(-1, dim) if want_normals else None), inside


def _prepare(phi, level, origin, spacing, closed, outside):
    phi = np.asarray(phi).astype(np.float64)                # fp32 samples are widened first
    dim = phi.ndim
    origin = np.broadcast_to(np.asarray(origin, np.float64), (dim,)).copy()
    spacing = np.broadcast_to(np.asarray(spacing, np.float64), (dim,)).copy()
    if closed:
        assert outside is not None and outside > level
        phi = np.pad(phi, 1, constant_values=float(outside))
    return phi, float(level), origin, spacing, (1 if closed else 0)


def isosurface(phi, level=0.0, origin=(0, 0, 0), spacing=1.0, closed=False, outside=None, normals=False):
    """-> vertices (V,3) float64, faces (F,3) int64, normals (V,3) float64 or None"""
    phi, level, origin, spacing, ext = _prepare(phi, level, origin, spacing, closed, outside)
    V, index, N, inside = _vertices(phi, level, origin, spacing, SLOTS3, normals, ext)
    chains = _chains(3)
    faces = []

    def vid(a, b):                                           # a before b in the chain: a owns the edge
        return index[(a, SLOTS3.index(tuple(y - x for x, y in zip(a, b))))]

    def mid(a, b):
        return 0.5 * (np.asarray(a, np.float64) + np.asarray(b, np.float64))

    for c in np.ndindex(*(n - 1 for n in phi.shape)):
        cube = inside[c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 2]
        if cube.all() or not cube.any():
            continue
        for chain in chains:
            nodes = [tuple(a + b for a, b in zip(c, off)) for off in chain]
            ins = [k for k in range(4) if inside[nodes[k]]]
            out = [k for k in range(4) if not inside[nodes[k]]]
            if not ins or not out:
                continue
            if len(ins) == 2:
                (A, B), (C, D) = ins, out
                cyc = [(A, C), (A, D), (B, D), (B, C)]
            elif len(ins) == 1:
                cyc = [(ins[0], k) for k in out]
            else:
                cyc = [(out[0], k) for k in ins]
            edges = [(min(u, v), max(u, v)) for u, v in cyc]
            pts = [mid(nodes[u], nodes[v]) for u, v in edges]
            ids = [vid(nodes[u], nodes[v]) for u, v in edges]
            normal = np.cross(pts[1] - pts[0], pts[2] - pts[0])
            outward = np.mean([nodes[k] for k in out], axis=0) - np.mean([nodes[k] for k in ins], axis=0)
            d = float(normal @ outward)
            assert abs(d) > 1e-9
            if d < 0:
                ids = ids[::-1]
                ids = ids[-1:] + ids[:-1]                    # keep the cycle's first vertex first: the diagonal stays AC-BD
            faces.append((ids[0], ids[1], ids[2]))
            if len(ids) == 4:
                faces.append((ids[0], ids[2], ids[3]))
    return V, np.array(faces, np.int64).reshape(-1, 3), N


def contour(phi, level=0.0, origin=(0, 0), spacing=1.0, closed=False, outside=None):
    """-> vertices (V,2) float64, segments (S,2) int64; the inside lies on the left of every segment"""
    phi, level, origin, spacing, ext = _prepare(phi, level, origin, spacing, closed, outside)
    V, index, _, inside = _vertices(phi, level, origin, spacing, SLOTS2, False, ext)
    segs = []
    for c in np.ndindex(*(n - 1 for n in phi.shape)):
        for chain in _chains(2):
            nodes = [tuple(a + b for a, b in zip(c, off)) for off in chain]
            ins = [k for k in range(3) if inside[nodes[k]]]
            out = [k for k in range(3) if not inside[nodes[k]]]
            if not ins or not out:
                continue
            lone, rest = (ins[0], out) if len(ins) == 1 else (out[0], ins)
            edges = [(min(lone, k), max(lone, k)) for k in rest]
            pts = [0.5 * (np.asarray(nodes[u], np.float64) + np.asarray(nodes[v], np.float64)) for u, v in edges]
            ids = [index[(nodes[u], SLOTS2.index(tuple(y - x for x, y in zip(nodes[u], nodes[v]))))] for u, v in edges]
            d = pts[1] - pts[0]
            left = np.array([-d[1], d[0]])
            toward_inside = np.mean([nodes[k] for k in ins], axis=0) - np.mean([nodes[k] for k in out], axis=0)
            if float(left @ toward_inside) < 0:
                ids = ids[::-1]
            segs.append(tuple(ids))
    return V, np.array(segs, np.int64).reshape(-1, 2)


# ------------------------------------------------------------------ checkers ----
def canonical_faces(F):
    """rotate each face to put its smallest index first (orientation kept), then lexsort the rows"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return F
    k = np.argmin(F, axis=1)
    rows = np.arange(len(F))
    G = np.stack([F[rows, k], F[rows, (k + 1) % 3], F[rows, (k + 2) % 3]], axis=1)
    return G[np.lexsort((G[:, 2], G[:, 1], G[:, 0]))]


def canonical_segments(S):
    S = np.asarray(S, np.int64).reshape(-1, 2)
    return S[np.lexsort((S[:, 1], S[:, 0]))] if len(S) else S


def is_closed_manifold(F, nverts=None):
    """every directed edge appears exactly once and its reverse exactly once (vectorised: fine at millions of faces)"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    if len(F) == 0:
        return True
    n = int(nverts if nverts is not None else F.max() + 1)
    a = np.concatenate([F[:, 0], F[:, 1], F[:, 2]])
    b = np.concatenate([F[:, 1], F[:, 2], F[:, 0]])
    if (a == b).any():
        return False
    fwd = np.unique(a * n + b)
    if len(fwd) != len(a):
        return False
    return np.array_equal(fwd, np.unique(b * n + a))


def euler(V, F):
    """V - E + F over the vertices the faces use"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    nv = len(V) if not np.isscalar(V) else int(V)
    e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
    e.sort(axis=1)
    return nv - len(np.unique(e[:, 0] * max(nv, 1) + e[:, 1])) + len(F)


def signed_volume(V, F):
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    a, b, c = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def all_vertices_used(V, F):
    return len(np.unique(np.asarray(F).reshape(-1))) == len(V)


def is_closed_contour(S, nverts):
    """every vertex is the start of exactly one segment and the end of exactly one"""
    S = np.asarray(S, np.int64).reshape(-1, 2)
    return (np.array_equal(np.bincount(S[:, 0], minlength=nverts), np.ones(nverts, np.int64))
            and np.array_equal(np.bincount(S[:, 1], minlength=nverts), np.ones(nverts, np.int64)))


def loops(S, nverts):
    """the loops of a closed contour, each a list of vertex indices in segment direction"""
    S = np.asarray(S, np.int64).reshape(-1, 2)
    nxt = np.full(nverts, -1, np.int64)
    nxt[S[:, 0]] = S[:, 1]
    seen = np.zeros(nverts, bool)
    out = []
    for v0 in range(nverts):
        if seen[v0] or nxt[v0] < 0:
            continue
        loop, v = [], v0
        while not seen[v]:
            seen[v] = True
            loop.append(v)
            v = int(nxt[v])
        out.append(loop)
    return out


def shoelace(V, loop):
    P = np.asarray(V, np.float64)[np.asarray(loop)]
    x, y = P[:, 0], P[:, 1]
    return float(0.5 * (x * np.roll(y, -1) - np.roll(x, -1) * y).sum())


def signed_area(V, S):
    V = np.asarray(V, np.float64)
    S = np.asarray(S, np.int64).reshape(-1, 2)
    a, b = V[S[:, 0]], V[S[:, 1]]
    return float(0.5 * (a[:, 0] * b[:, 1] - b[:, 0] * a[:, 1]).sum())


# ------------------------------------------------------------------- the cases ----
def grid_points(shape, origin, spacing):
    dim = len(shape)
    origin = np.broadcast_to(np.asarray(origin, np.float64), (dim,))
    spacing = np.broadcast_to(np.asarray(spacing, np.float64), (dim,))
    ax = [origin[d] + np.arange(shape[d], dtype=np.float64) * spacing[d] for d in range(dim)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1)


def sphere_sdf(X, centre, radius):
    return np.sqrt(((X - np.asarray(centre, np.float64)) ** 2).sum(-1)) - radius


def torus_sdf(X, centre, R, r):
    """torus around the z axis through `centre`"""
    d = X - np.asarray(centre, np.float64)
    return np.sqrt((np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2) - R) ** 2 + d[..., 2] ** 2) - r


def case_sphere():
    shape, sp = (13, 9, 21), np.array([0.11, 0.17, 0.07])
    X = grid_points(shape, 0.0, sp)
    centre = 0.5 * (np.asarray(shape) - 1) * sp
    return dict(phi=sphere_sdf(X, centre, 0.42), spacing=sp, origin=np.zeros(3), chi=2,
                analytic=4.0 / 3.0 * np.pi * 0.42 ** 3, cap=9 * sp.max() ** 2 / (8 * 0.42 ** 2))


def case_torus():
    shape, h = (24, 20, 28), 1.0 / 24
    X = grid_points(shape, 0.0, h)
    centre = 0.5 * (np.asarray(shape) - 1) * h
    return dict(phi=torus_sdf(X, centre, 0.25, 0.09), spacing=h, origin=np.zeros(3), chi=0,
                analytic=2 * np.pi ** 2 * 0.25 * 0.09 ** 2, cap=9 * h ** 2 / (8 * 0.09 ** 2))


def case_two_spheres():
    X = grid_points((17, 10, 11), 0.0, 1.0)
    phi = np.minimum(sphere_sdf(X, (4.3, 4.6, 5.2), 3.1), sphere_sdf(X, (12.1, 4.4, 4.9), 2.7))
    return dict(phi=phi, spacing=1.0, origin=np.zeros(3), chi=4)


def case_octahedron():
    """the exact-hit case: integer samples, a third of the crossed edges end ON the level.  The field is linear on
    every Kuhn simplex, so the mesh is the octahedron itself: volume 4/3 * 3^3 = 36"""
    X = grid_points((17, 10, 11), 0.0, 1.0)
    phi = np.abs(X[..., 0] - 8) + np.abs(X[..., 1] - 4) + np.abs(X[..., 2] - 5) - 3
    return dict(phi=phi, spacing=1.0, origin=np.zeros(3), chi=2, analytic=36.0)


def case_union():
    """several scan blocks (40 x 36 x 33 = 47 520 nodes): a torus and two spheres, disjoint: chi = 0 + 2 + 2"""
    X = grid_points((40, 36, 33), 0.0, 1.0)
    phi = np.minimum(torus_sdf(X, (14.2, 13.7, 8.3), 8.0, 3.2),
                     np.minimum(sphere_sdf(X, (30.3, 26.1, 10.4), 6.3), sphere_sdf(X, (20.6, 18.2, 24.7), 6.9)))
    return dict(phi=phi, spacing=1.0, origin=np.zeros(3), chi=4)


def case_circle():
    shape, sp = (19, 14), np.array([0.13, 0.09])
    X = grid_points(shape, 0.0, sp)
    return dict(phi=sphere_sdf(X, 0.5 * (np.asarray(shape) - 1) * sp, 0.45), spacing=sp, origin=np.zeros(2))


def case_diamond():
    X = grid_points((17, 13), 0.0, 1.0)
    return dict(phi=np.abs(X[..., 0] - 8) + np.abs(X[..., 1] - 6) - 3, spacing=1.0, origin=np.zeros(2), analytic=18.0)


def case_discs():
    """300 x 210 (63 000 nodes): three discs and an annulus -- five loops, the annulus' inner one clockwise"""
    X = grid_points((300, 210), 0.0, 1.0)
    ring = np.abs(sphere_sdf(X, (200.3, 120.6), 50.0)) - 14.0
    phi = np.minimum.reduce([sphere_sdf(X, (50.2, 50.7), 30.0), sphere_sdf(X, (60.4, 150.1), 25.0),
                             sphere_sdf(X, (200.3, 120.6), 18.0), ring])
    return dict(phi=phi, spacing=1.0, origin=np.zeros(2))
