"""The float64 oracle of liquid seeding (mfs/seed.py, csrc/mfs_seed.hip), operation by operation.

Sites: a lattice of shape (n0, n1, n2), site (i, j, k) with the 64-bit index s = (i * n1 + j) * n2 + k.  Jitter: with
mix(x) = {x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16} on uint32, h = mix(seed_lo),
h = mix(h ^ seed_hi), h = mix(h ^ s_lo), h = mix(h ^ s_hi), h_a = mix(h + (a + 1) * 0x9E3779B9) and
u_a = (h_a >> 8) * 2^-24 - 0.5.  Position: origin + ((idx + 0.5) + jitter * U) * h in float64.  A shape is
(vol, origin, spacing, R, T): its value at x is `sample` at R^T (x - T).  A site is kept iff min over includes < 0 and
min over excludes > clearance; np.minimum carries a NaN, so a NaN sample keeps nothing.

The band: sites whose decision a rounding of the sampler could turn, |include min| <= eps or |exclude min - clearance|
<= eps with eps = 64 * eps64 * max(1, max |phi|, largest |x - volume origin|) -- the bound tests/test_mesh_timestep_gpu.py
uses for this sampler (TOL64), scaled by the magnitudes that enter it.
"""
import numpy as np

import meshsdf_numpy as M

EPS64 = float(np.finfo(np.float64).eps)
IDENTITY = (np.eye(3), np.zeros(3))


def mix(x):
    x = np.asarray(x, np.uint32).copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def hash3(seed, s):
    """(len(s), 3) uint32: h_a of every site index in `s` (uint64)"""
    s = np.asarray(s, np.uint64)
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    with np.errstate(over="ignore"):
        h = mix(np.uint32(seed & 0xffffffff))
        h = mix(h ^ np.uint32(seed >> 32))
        h = mix(h ^ (s & np.uint64(0xffffffff)).astype(np.uint32))
        h = mix(h ^ (s >> np.uint64(32)).astype(np.uint32))
        return np.stack([mix(h + np.uint32(((a + 1) * 0x9E3779B9) & 0xffffffff)) for a in range(3)], axis=-1)


def uniform(seed, s):
    """(len(s), 3) float64 in [-0.5, 0.5)"""
    return (hash3(seed, s) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 - 0.5


def site_indices(shape):
    """(sites, 3) float64 lattice indices in ascending s"""
    ax = [np.arange(n, dtype=np.float64) for n in shape]
    return np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, 3)


def positions(shape, origin, h, jitter=1.0, seed=0, s=None):
    """float64 positions of the sites `s` (default: all, ascending)"""
    idx = site_indices(shape)
    if s is None:
        s = np.arange(len(idx), dtype=np.uint64)
    else:
        idx = idx[np.asarray(s, np.int64)]
    U = uniform(seed, s)
    return np.asarray(origin, np.float64) + ((idx + 0.5) + float(jitter) * U) * np.float64(h)


def to_body(R, T, x):
    """x_b = R^T (x - T), grouped as the kernels' pose_to_body (meshsdf_numpy.to_body for a (10, 4) row)"""
    d = x - np.asarray(T, np.float64)
    return np.stack([(R[0, i] * d[..., 0] + R[1, i] * d[..., 1]) + R[2, i] * d[..., 2] for i in range(3)], axis=-1)


def sample(vol, origin, h, xb):
    """meshsdf_numpy.sample's value for a float32 OR float64 volume: trilinear in float64; outside: the sample at the
    clamped point plus the distance to the volume's box"""
    vol = np.asarray(vol)
    assert vol.dtype in (np.float32, np.float64)
    n = vol.shape
    h = np.float64(h)
    c, fr, e = [], [], []
    for k in range(3):
        t = (xb[..., k] - np.float64(origin[k])) / h
        tc = np.minimum(np.maximum(t, 0.0), np.float64(n[k] - 1))
        ci = np.minimum(np.floor(tc).astype(np.int64), n[k] - 2)
        c.append(ci)
        fr.append(tc - ci.astype(np.float64))
        e.append((t - tc) * h)
    V = lambda a, b, d: vol[c[0] + a, c[1] + b, c[2] + d].astype(np.float64)  # noqa: E731
    f0, f1, f2 = fr
    g0, g1, g2 = 1.0 - f0, 1.0 - f1, 1.0 - f2
    with np.errstate(invalid="ignore"):                                  # inf * 0 where a volume holds +inf
        c00, c01 = V(0, 0, 0) * g2 + V(0, 0, 1) * f2, V(0, 1, 0) * g2 + V(0, 1, 1) * f2
        c10, c11 = V(1, 0, 0) * g2 + V(1, 0, 1) * f2, V(1, 1, 0) * g2 + V(1, 1, 1) * f2
        c0, c1 = c00 * g1 + c01 * f1, c10 * g1 + c11 * f1
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        return (c0 * g0 + c1 * f0) + dist


def shape_of(vol, origin, spacing, pose=IDENTITY):
    """one shape of the oracle: (vol, origin, spacing, R, T)"""
    return (np.asarray(vol), tuple(float(v) for v in origin), float(spacing), np.asarray(pose[0], np.float64),
            np.asarray(pose[1], np.float64))


def pose_of_row(row):
    """(R, T) of a packed (10, 4) body row (solver.sdf3D)"""
    row = np.asarray(row, np.float64).reshape(10, 4)
    return row[5:8, :3], row[1:4, 3]


def _min_over(shapes, x):
    m = np.full(len(x), np.inf)
    for vol, origin, h, R, T in shapes:
        m = np.minimum(m, sample(vol, origin, h, to_body(R, T, x)))      # np.minimum keeps a NaN
    return m


def band_eps(shapes, x):
    """64 eps64 max(1, max |phi| (finite), largest |x - volume origin|) over the shapes"""
    big = 1.0
    for vol, origin, h, R, T in shapes:
        fin = np.abs(vol[np.isfinite(vol)])
        big = max(big, float(fin.max()) if fin.size else 0.0)
        if len(x):
            big = max(big, float(np.sqrt(((to_body(R, T, x) - np.asarray(origin)) ** 2).sum(axis=-1)).max()))
    return 64 * EPS64 * big


def decide(include, exclude, x, clearance=0.0):
    """(kept mask, band mask, include min, exclude min) for positions x"""
    assert len(include) >= 1 and len(include) + len(exclude) <= 16
    inc, exc = _min_over(include, x), _min_over(exclude, x)
    with np.errstate(invalid="ignore"):
        kept = (inc < 0) & (exc > clearance)
        eps = band_eps(list(include) + list(exclude), x)
        band = np.abs(inc) <= eps
        if exclude:
            band |= np.abs(exc - clearance) <= eps
    return kept, band, inc, exc


def fill(include, shape, origin, h, exclude=(), clearance=0.0, jitter=1.0, seed=0):
    """(px (P, 3) float64, sites (P,) int64, number of band sites): the oracle of mfs.seed.fill(..., return_sites=True)"""
    if not (0.0 <= jitter <= 1.0):
        raise ValueError("jitter must be in [0, 1]")
    if len(include) < 1:
        raise ValueError("at least 1 include shape")
    if len(include) + len(exclude) > 16:
        raise ValueError("at most 16 shapes")
    x = positions(shape, origin, h, jitter, seed)
    kept, band, _, _ = decide(include, exclude, x, clearance)
    return x[kept], np.flatnonzero(kept).astype(np.int64), int(band.sum())


# ------------------------------------------------------------------------------------------ shared test scenes ----
def nodes(shape, origin, h):
    return M.lattice_nodes(shape, origin, h)


def torus_volume():
    """a torus (R 0.15, r 0.06) about axis 2 as a float32 volume 41 x 41 x 21, spacing 0.0125"""
    origin, h, shape = (-0.25, -0.25, -0.125), 0.0125, (41, 41, 21)
    p = nodes(shape, origin, h)
    q = np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2) - 0.15
    return (np.sqrt(q * q + p[..., 2] ** 2) - 0.06).astype(np.float32), origin, h


def rotation(axis, angle_degrees):
    from scipy.spatial.transform import Rotation
    ax = np.asarray(axis, np.float64)
    return Rotation.from_rotvec(ax / np.linalg.norm(ax) * angle_degrees * np.pi / 180).as_matrix()   # as solver.sdf3D.get_R


MAIN = dict(shape=(70, 66, 68), origin=(-0.2, 0.1, -0.22), h=0.00625, jitter=1.0, seed=7,
            center=(0.02, 0.31, -0.01), axis=(1, 2, 0.5), angle=33)


def main_case():
    """the parity case of tests/test_seed_gpu.py: (include shapes, exclude shapes) of the oracle.  Include: the torus
    volume posed at MAIN's centre / axis / angle; exclude: min(y - 0.27, |x - (0.1, 0.33, 0)| - 0.05) as a float64 volume on
    the sites' own node lattice (71 x 67 x 69)."""
    vol, org, h = torus_volume()
    inc = shape_of(vol, org, h, (rotation(MAIN["axis"], MAIN["angle"]), np.asarray(MAIN["center"], np.float64)))
    eshape = tuple(n + 1 for n in MAIN["shape"])
    p = nodes(eshape, MAIN["origin"], MAIN["h"])
    ball = np.sqrt(((p - np.array([0.1, 0.33, 0.0])) ** 2).sum(axis=-1)) - 0.05
    exc = shape_of(np.minimum(p[..., 1] - 0.27, ball), MAIN["origin"], MAIN["h"])
    return [inc], [exc]
