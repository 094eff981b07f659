"""mfs.skin on the MI355X against the brute-force oracle (tests/skin_numpy.py).

Tolerance, the project's E32 rule (as tests/test_meshsdf_gpu.py): E32 is the largest deviation over the lattice of the
oracle run in float32 from the oracle run in float64, recomputed and printed by every run; the GPU must stay within
4 * E32 of the float64 oracle at EVERY node.  On the cloud below E32 is 1.6e-7 on the CPU (8.6e-8 to 2.7e-7 over four
seeds); float32 variants with other local origins, another operation order, reversed sums and (R^2 - d^2) / R^2 stayed at
or below 1.35 * E32, so 4 x covers the kernel's brick-local origin, its order of summation and FMA contraction.
Measured on the MI355X (for the reader; printed by every run): cloud 0.39 E32, its float32 particles 0.54, overhang
0.52 / 0.44, ties 1.00 (E32 5e-9 there).
Lattice extents are no multiples of the 4 x 8 x 8 brick; the cloud fills several LDS batches per brick, the last partial."""
import functools

import numpy as np
import pytest
import torch

import skin_numpy as S
import surface_numpy as SN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
H = 0.05
SHAPE = (27, 23, 30)

# name -> (particles, shape, origin, spacing, radius, influence)
TIE_POINTS = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, 0.5], [0.75, 0.5, 0.5], [1.0, 1.0, 0.875], [0.25, 1.25, 1.0]])
CASES = {
    "cloud": lambda: (S.cloud(), SHAPE, (0.1, 0.12, 0.08), H, H, 2.5 * H),
    "cloud32": lambda: (S.cloud().astype(np.float32), SHAPE, (0.1, 0.12, 0.08), H, H, 2.5 * H),
    # the cloud hangs over the low side of axis 0 (its first layers farther than the ring of bins) and the high side of axis 2
    "overhang": lambda: (S.cloud(), SHAPE, (0.62, 0.12, -0.55), H, H, 2.5 * H),
    "overhang32": lambda: (S.cloud().astype(np.float32), SHAPE, (0.62, 0.12, -0.55), H, H, 2.5 * H),
    # dyadic coordinates, particles on nodes, the first two coincident
    "ties": lambda: (TIE_POINTS, (11, 13, 10), (0.0, 0.0, 0.0), 0.125, 0.125, 0.25),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """(px, shape, origin, h, r, R, phi64, K, tol) -- computed once per case, never modified"""
    px, shape, origin, h, r, R = CASES[name]()
    phi64, K = S.field(px, shape, origin, h, r, R)
    e32 = S.e32(px, shape, origin, h, r, R, phi64)
    for a in (px, phi64, K):
        a.setflags(write=False)
    print(f"{name}: {len(px)} particles, lattice {shape} = {K.size} nodes, {(K == 0).mean():.1%} background, K up to {K.max()}, "
          f"E32 {e32:.3e}, tolerance {4 * e32:.3e}")
    return px, shape, origin, h, r, R, phi64, K, 4 * e32


def gpu_field(name, px=None):
    from mfs import skin
    p0, shape, origin, h, r, R = reference(name)[:6]
    return skin.field(torch.tensor(p0 if px is None else px, device=DEV), shape, origin, h, r, R)


def check(name, px=None):
    _, shape, origin, h, r, R, phi64, K, tol = reference(name)
    f = gpu_field(name, px)
    assert f.phi.dtype == torch.float32 and tuple(f.phi.shape) == shape and f.phi.is_contiguous() and f.phi.is_cuda
    assert f.origin == tuple(float(v) for v in origin) and (f.spacing, f.radius, f.influence) == (h, r, R)
    assert f.background == float(np.float32(R - r))
    phi = N(f.phi)
    err = float(np.abs(phi.astype(np.float64) - phi64).max())
    print(f"{name}: GPU error {err:.3e} = {err / (tol / 4):.2f} E32 (tolerance {tol:.3e})")
    assert np.isfinite(phi).all() and err <= tol
    assert (phi[K == 0] == np.float32(f.background)).all()              # exactly the background where nothing reaches
    return f, phi


@pytest.mark.parametrize("name", ["cloud", "cloud32"])
def test_the_cloud_matches_the_oracle(name):
    px, shape, _, _, r, _, phi64, K, _ = reference(name)
    assert px.shape == (1680, 3) and K.size == 18630 and any(s % 8 for s in shape) and shape[0] % 4
    assert 0.77 < (K == 0).mean() < 0.79 and K.max() >= 70 and phi64.min() < -0.98 * r
    check(name)


@pytest.mark.parametrize("name", ["overhang", "overhang32"])
def test_particles_outside_the_lattice_contribute_within_R(name):
    px, shape, origin, h, r, R, phi64, K, _ = reference(name)
    p = np.asarray(px, np.float64)
    lo, hi = np.asarray(origin), np.asarray(origin) + (np.asarray(shape) - 1) * h
    outside = ((p < lo) | (p > hi)).any(axis=1)
    beyond = p[:, 0] < lo[0] - 4 * h                                     # beyond the ring of bins along axis 0
    assert (p[:, 2] > hi[2]).sum() > 100 and (p[:, 0] < lo[0]).sum() > 100 and beyond.sum() > 100
    # what the particles outside add: the oracle on the inside ones alone differs at many nodes
    _, K_in = S.field(p[~outside], shape, origin, h, r, R)
    assert ((K > K_in) & (K_in > 0)).sum() > 500 and ((K > 0) & (K_in == 0)).sum() > 0
    _, K_near = S.field(p[~beyond], shape, origin, h, r, R)
    np.testing.assert_array_equal(K_near, K)                             # those beyond the ring reach no node
    check(name)


def test_ties_exactly_R_away_and_coincident_particles():
    px, shape, origin, h, r, R, phi64, K, _ = reference("ties")
    rel, _ = S.nodes(shape, origin, h)
    d2 = ((rel[..., None, :] - px) ** 2).sum(-1)                         # exact: dyadic
    on_rim = (d2 == R * R).any(-1) & (K == 0)
    assert on_rim.sum() >= 15 and (d2 == 0).any(-1).sum() == 4           # every particle on a node, two on the same one
    f, phi = check("ties")
    assert (phi[on_rim] == np.float32(R - r)).all()
    # two coincident particles weigh as one where they are alone (2 w d / 2 w is w d / w, bit for bit)
    alone = (K == 2) & (d2[..., 0] < R * R) & ((d2[..., 2:] >= R * R).all(-1))
    assert alone.sum() >= 10
    single = N(gpu_field("ties", px[1:]).phi)
    np.testing.assert_array_equal(phi[alone], single[alone])
    assert phi[tuple(np.argwhere(d2[..., 0] == 0)[0])] == np.float32(-r)  # on the particle itself: |0| - r


def test_no_particles_is_all_background_and_an_empty_mesh():
    from mfs import skin
    for dtype in (torch.float32, torch.float64):
        px = torch.zeros((0, 3), dtype=dtype, device=DEV)
        f = skin.field(px, (9, 10, 11), (0.3, 0.2, 0.1), H)
        assert f.radius == pytest.approx(1.02 * np.sqrt(3) / 2 * H, rel=1e-15) and f.influence == 3 * f.radius
        assert f.background == float(np.float32(f.influence - f.radius))
        assert tuple(f.phi.shape) == (9, 10, 11) and bool((f.phi == f.background).all())
        m = skin.mesh(px, (9, 10, 11), (0.3, 0.2, 0.1), H, normals=True)
        assert tuple(m.vertices.shape) == (0, 3) and tuple(m.faces.shape) == (0, 3) and tuple(m.normals.shape) == (0, 3)


def test_particles_far_from_the_lattice_or_not_finite_are_ignored():
    from mfs import skin
    px = torch.tensor([[50.0, 0.1, 0.1], [0.1, -9.0, 0.1], [float("nan"), 0.1, 0.1], [0.1, float("inf"), 0.1]], device=DEV)
    f = skin.field(px, (9, 10, 11), (0.0, 0.0, 0.0), H)
    assert bool((f.phi == f.background).all())


def test_two_calls_are_bitwise_equal_and_a_shuffle_stays_within_the_tolerance():
    px = reference("cloud")[0]
    a, b = gpu_field("cloud"), gpu_field("cloud")
    assert torch.equal(a.phi, b.phi)
    perm = np.random.default_rng(1).permutation(len(px))
    check("cloud", px[perm])
    c = gpu_field("cloud", px[perm])
    assert torch.equal(c.phi, gpu_field("cloud", px[perm]).phi)


@pytest.mark.parametrize("normals", [False, True])
def test_mesh_is_field_then_isosurface(normals):
    from mfs import skin
    from mfs.surface import isosurface
    px, shape, origin, h, r, R = reference("cloud")[:6]
    p = torch.tensor(px, device=DEV)
    m = skin.mesh(p, shape, origin, h, r, R, normals=normals)
    f = skin.field(p, shape, origin, h, r, R)
    ref = isosurface(f.phi, 0.0, origin, h, closed=True, outside=f.background, normals=normals)
    assert m.vertices.shape[0] > 1000 and torch.equal(m.vertices, ref.vertices) and torch.equal(m.faces, ref.faces)
    assert (m.normals is None and ref.normals is None) if not normals else torch.equal(m.normals, ref.normals)
    F = N(m.faces)
    assert SN.is_closed_manifold(F, m.vertices.shape[0])


def test_one_particle_is_a_sphere():
    from mfs import skin
    h, r, R = H, 3 * H, 4 * H                                            # R at the limit of one ring of bricks
    c = np.array([[0.31, 0.283, 0.337]])
    m = skin.mesh(torch.as_tensor(c, device=DEV), (13, 12, 14), (0.0, 0.0, 0.0), h, r, R)
    V, F = N(m.vertices).astype(np.float64), N(m.faces)
    assert SN.is_closed_manifold(F, len(V)) and SN.euler(V, F) == 2
    # linear interpolation along a Kuhn edge of length <= sqrt(3) h, where phi'' <= 1 / (r - sqrt(3) h)
    bound = 3 * h * h / (8 * (r - np.sqrt(3) * h))
    off = np.abs(np.linalg.norm(V - c, axis=1) - r).max()
    print(f"one particle: {len(V)} vertices, farthest from the sphere {off / h:.3f} h (bound {bound / h:.3f} h)")
    assert off <= bound


def line(start, direction, n=40, h=H):
    d = np.asarray(direction, np.float64)
    return np.asarray(start, np.float64) * h + np.arange(n)[:, None] * h * d / np.linalg.norm(d)


THREADS = {
    "x_cell_centred": (line((5, 6.5, 6.5), (1, 0, 0)), (50, 13, 13)),
    "x_on_nodes": (line((5, 6, 6), (1, 0, 0)), (50, 13, 13)),
    "x_offset": (line((5, 6.25, 6.4), (1, 0, 0)), (50, 13, 13)),
    "oblique": (line((3.5, 3.5, 3.5), (1, 0.6, 0.35)), (45, 32, 24)),
}


@pytest.mark.parametrize("name", sorted(THREADS))
def test_a_thread_one_particle_thick_is_one_closed_tube(name):
    from mfs import skin
    px, shape = THREADS[name]
    m = skin.mesh(torch.as_tensor(px, device=DEV), shape, (0.0, 0.0, 0.0), H)        # default radii
    V, F = N(m.vertices), N(m.faces)
    assert len(V) > 300 and SN.is_closed_manifold(F, len(V)) and SN.euler(V, F) == 2
    # One particle thick: no vertex farther than r from the segment.  |sum w d| / W is the distance to a point of the
    # particles' convex hull, so phi >= f = dist(segment) - r at every node a particle reaches (and the unreached end of a
    # crossed edge, <= r + sqrt(3) h < R from the segment, holds R - r >= f); f is convex along the edge, so at the zero
    # of the edge's linear interpolant f <= 0.
    a, d = px[0], (px[-1] - px[0]) / np.linalg.norm(px[-1] - px[0])
    w = V.astype(np.float64) - a
    t = np.clip(w @ d, 0, np.linalg.norm(px[-1] - px[0]))
    # slack: float32 vertex coordinates up to 2.3 (1.4e-7) and float32 phi (a few 1e-7, |grad phi| about 1)
    assert np.linalg.norm(w - t[:, None] * d, axis=1).max() <= skin.default_radius(H) + 2e-6


def test_a_larger_influence_is_refused_with_the_limit():
    from mfs import _lib, skin
    px = torch.zeros((1, 3), dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match=r"must not exceed 4 \* spacing"):
        skin.field(px, (9, 9, 9), (0, 0, 0), H, 3 * H, 4.01 * H)
    lib = _lib.load()
    phi = torch.zeros((9, 9, 9), dtype=torch.float32, device=DEV)
    st = lib.mfs_skin_field3d(_lib.i64x((9, 9, 9)), _lib.f64x((0, 0, 0)), H, 3 * H, 4.01 * H, None, 1, 0, None, phi.data_ptr(),
                              None, None)
    assert st == -1 and b"4 * spacing" in lib.mfs_last_error() and bool((phi == 0).all())
