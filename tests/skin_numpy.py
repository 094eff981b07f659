"""The liquid skin's field by brute force (the oracle of mfs.skin; DESIGN.md "Liquid skin"): every node against every
particle, float64.

    d_i = x_i - x,  q_i = 1 - |d_i|^2 / R^2,  w_i = q_i^3 if q_i > 0 else 0,  W = sum w_i
    phi(x) = |sum w_i d_i| / W - r  if W > 0,   R - r  if W == 0

dtype=np.float32 runs the same formula in float32 on positions taken relative to the lattice origin in float64 first:
the yardstick E32 = max |field32 - field64| of what float32 arithmetic costs on a given case."""
import numpy as np


def nodes(shape, origin, spacing):
    """(n0,n1,n2,3) float64 node positions RELATIVE to `origin` and the origin as a float64 triple"""
    ax = [np.arange(int(n), dtype=np.float64) * float(spacing) for n in shape]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1), np.asarray(origin, np.float64).reshape(3)


def background(radius, influence, dtype=np.float64):
    return dtype(np.float64(influence) - np.float64(radius))


def field(px, shape, origin, spacing, radius, influence, dtype=np.float64, chunk=512):
    """-> (phi of `dtype` (n0,n1,n2), K int64 (n0,n1,n2): the particles with q > 0 at each node)"""
    rel, org = nodes(shape, origin, spacing)
    X = rel.reshape(-1, 3).astype(dtype)                                  # relative to the origin, then rounded
    P = (np.asarray(px, np.float64).reshape(-1, 3) - org).astype(dtype)
    r, R = dtype(radius), dtype(influence)
    R2 = R * R
    phi = np.full(len(X), background(radius, influence, dtype), dtype)
    K = np.zeros(len(X), np.int64)
    if len(P):
        for a in range(0, len(X), chunk):
            d = P[None, :, :] - X[a:a + chunk, None, :]                   # (nodes, particles, 3)
            q = dtype(1) - (d * d).sum(-1) / R2
            w = np.where(q > 0, q * q * q, dtype(0))
            W = w.sum(-1)
            K[a:a + chunk] = (q > 0).sum(-1)
            hit = W > 0
            m = (w[hit, :, None] * d[hit]).sum(1) / W[hit, None]          # divided first: w d squares underflow at the rim
            phi[a:a + chunk][hit] = np.sqrt((m * m).sum(-1)) - r
    assert phi.dtype == dtype
    return phi.reshape(shape), K.reshape(shape)


def e32(px, shape, origin, spacing, radius, influence, phi64=None):
    """largest deviation over the lattice of the float32 run from the float64 run"""
    if phi64 is None:
        phi64 = field(px, shape, origin, spacing, radius, influence)[0]
    phi32 = field(px, shape, origin, spacing, radius, influence, np.float32)[0]
    return float(np.abs(phi32.astype(np.float64) - phi64).max())


def cloud(counts=(12, 10, 14), h=0.05, start=0.31, jitter=0.3, seed=0):
    """a jittered block of particles: start + (idx + 0.5) h + jitter h N(0,1)"""
    rng = np.random.default_rng(seed)
    idx = np.stack(np.meshgrid(*[np.arange(c) for c in counts], indexing="ij"), axis=-1).reshape(-1, 3)
    return start + (idx + 0.5) * h + jitter * h * rng.standard_normal(idx.shape)
