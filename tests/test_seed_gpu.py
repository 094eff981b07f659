"""mfs.seed on the MI355X against tests/seed_numpy.py.  Wherever the oracle's decisions are compared site by site the
test first asserts that the oracle's band -- the sites a rounding of the sampler could turn -- is empty, so no site is left
out of a comparison; positions are compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import meshsdf_numpy as M
import seed_numpy as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731


def volume(vol, origin, h):
    """an oracle volume on the GPU as a bare shape of mfs.seed (.phi / .origin / .spacing)"""
    from mfs.meshsdf import MeshSDF
    return MeshSDF(torch.as_tensor(np.ascontiguousarray(vol), device=DEV), tuple(float(v) for v in origin), float(h), 0.0)


def gpu_shape(o):
    """an oracle shape (vol, origin, h, R, T) as an mfs.seed.Shape with exactly that pose"""
    from mfs import seed
    s = seed.as_shape(volume(o[0], o[1], o[2]))
    s.R, s.T = np.ascontiguousarray(o[3]), np.asarray(o[4])
    return s


def constant(value, dtype=np.float32):
    """one value everywhere the tests look: a volume of one cell of side 100 about the origin"""
    return S.shape_of(np.full((2, 2, 2), value, dtype), (-50, -50, -50), 100.0)


@pytest.fixture(scope="module")
def main():
    """the parity case: the oracle's answer, computed once"""
    inc, exc = S.main_case()
    px, sites, band = S.fill(inc, S.MAIN["shape"], S.MAIN["origin"], S.MAIN["h"], exc, 0.0, S.MAIN["jitter"], S.MAIN["seed"])
    return inc, exc, px, sites, band


def test_parity_with_the_oracle_on_a_posed_torus_against_a_floor_and_a_ball(main):
    from mfs import seed
    inc, exc, ref_px, ref_sites, band = main
    m = S.MAIN
    assert band == 0 and len(ref_sites) == 25284                         # nothing is left out of the comparison
    torus = seed.Shape(volume(*inc[0][:3]), center=m["center"], axis=m["axis"], angle=m["angle"])
    np.testing.assert_array_equal(torus.R, inc[0][3])
    solid = volume(*exc[0][:3])
    assert torus.volume.phi.dtype == torch.float32 and solid.phi.dtype == torch.float64
    args = dict(shape=m["shape"], origin=m["origin"], spacing=m["h"], exclude=[solid], jitter=m["jitter"], seed=m["seed"])
    stats = {}
    px, sites = seed.fill(torus, return_sites=True, stats=stats, **args)
    assert px.dtype == torch.float64 and tuple(px.shape) == (25284, 3) and sites.dtype == torch.int64
    assert stats == dict(sites=314160, blocks=1228, kept=25284)
    np.testing.assert_array_equal(N(sites), ref_sites)
    assert N(px).tobytes() == ref_px.tobytes()                            # bit for bit
    assert seed.count(torus, **args) == 25284
    px32 = seed.fill([torus], dtype=torch.float32, **args)
    assert px32.dtype == torch.float32 and torch.equal(px32, px.to(torch.float32))
    again, sites2 = seed.fill(torus, return_sites=True, **args)
    assert N(again).tobytes() == N(px).tobytes() and torch.equal(sites2, sites)
    assert torch.equal(seed.fill(torus, **args), px)                      # without the site indices


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 300), (3, 5, 7), (2, 129, 2), (1, 257, 1)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_block_edges_and_thin_lattices(shape, dtype):
    from mfs import seed
    origin, h = (0.3, -0.2, 0.1), 0.07
    n = int(np.prod(shape))
    px, sites = seed.fill(volume(*constant(-1.0, dtype)[:3]), shape, origin, h, seed=11, return_sites=True)
    np.testing.assert_array_equal(N(sites), np.arange(n))
    assert N(px).tobytes() == S.positions(shape, origin, h, 1.0, 11).tobytes()
    stats = {}
    none = seed.fill(volume(*constant(1.0, dtype)[:3]), shape, origin, h, seed=11, stats=stats)
    assert tuple(none.shape) == (0, 3) and none.dtype == torch.float64
    assert none.device == torch.device(DEV)
    assert stats == dict(sites=n, blocks=(n + 255) // 256, kept=0)
    p0, s0 = seed.fill(volume(*constant(1.0, dtype)[:3]), shape, origin, h, return_sites=True, dtype=torch.float32)
    assert tuple(p0.shape) == (0, 3) and p0.dtype == torch.float32 and tuple(s0.shape) == (0,) and s0.dtype == torch.int64
    assert seed.count(volume(*constant(1.0, dtype)[:3]), shape, origin, h) == 0


def ball(shape, origin, h, centre, radius, dtype):
    p = S.nodes(shape, origin, h)
    return S.shape_of((np.sqrt(((p - np.asarray(centre)) ** 2).sum(axis=-1)) - radius).astype(dtype), origin, h)


def test_two_overlapping_includes_and_an_exclude_with_clearance():
    from mfs import seed
    a = ball((17, 17, 17), (0, 0, 0), 0.0625, (0.4, 0.5, 0.5), 0.27, np.float32)
    b = ball((13, 13, 13), (0.2, 0.1, 0.1), 0.0625, (0.62, 0.5, 0.5), 0.22, np.float64)
    shape, origin, h = (33, 31, 35), (0.013, 0.021, -0.017), 0.03
    both, sites, band = S.fill([a, b], shape, origin, h, seed=3)
    only_a, only_b = S.fill([a], shape, origin, h, seed=3)[1], S.fill([b], shape, origin, h, seed=3)[1]
    assert band == 0 and len(np.intersect1d(only_a, only_b)) > 500       # they do overlap
    np.testing.assert_array_equal(sites, np.union1d(only_a, only_b))     # the min rule: a union, no site twice
    px, got = seed.fill([gpu_shape(a), gpu_shape(b)], shape, origin, h, seed=3, return_sites=True)
    assert len(np.unique(N(got))) == len(got)
    np.testing.assert_array_equal(N(got), sites)
    assert N(px).tobytes() == both.tobytes()
    # an exclude with a clearance trims exactly the oracle's sites
    wall = S.shape_of((S.nodes((9, 9, 9), (0, 0, 0), 0.125)[..., 1] - 0.41).astype(np.float32), (0, 0, 0), 0.125)   # solid below y = 0.41
    for clearance in (0.0, 0.0371):
        ref_px, ref_sites, band = S.fill([a, b], shape, origin, h, [wall], clearance, 1.0, 3)
        assert band == 0 and 0 < len(ref_sites) < len(sites)
        px, got = seed.fill([gpu_shape(a), gpu_shape(b)], shape, origin, h, exclude=gpu_shape(wall), clearance=clearance,
                            seed=3, return_sites=True)
        np.testing.assert_array_equal(N(got), ref_sites)
        assert N(px).tobytes() == ref_px.tobytes()
        assert (ref_px[:, 1] > 0.41 + clearance - 1e-12).all()
    assert len(S.fill([a, b], shape, origin, h, [wall], 0.0371, 1.0, 3)[1]) < len(S.fill([a, b], shape, origin, h, [wall], 0.0, 1.0, 3)[1])


def test_sites_beyond_an_include_volumes_box_follow_the_clamp_plus_distance_rule():
    from mfs import seed
    # phi = x - 0.75 on the box [0, 0.5]^3: -0.75 on its face x = 0 and -0.25 on its face x = 0.5, so by the clamped sample
    # plus the distance the liquid goes on 0.75 past the first face and 0.25 past the second, and sideways to where the
    # distance to the box reaches 0.75 - (clamped x).  The lattice is dyadic along x and not along y and z, so no centre
    # samples an exact zero.
    vol = S.shape_of((S.nodes((5, 5, 5), (0, 0, 0), 0.125)[..., 0] - 0.75).astype(np.float64), (0, 0, 0), 0.125)
    shape, origin, h = (40, 24, 24), (-1.0, -0.503, -0.497), 0.0625      # x in [-1, 1.5): far beyond both faces
    rule = lambda x: np.clip(x, 0.0, 0.5)[:, 0] - 0.75 + np.linalg.norm(x - np.clip(x, 0.0, 0.5), axis=1)  # noqa: E731
    for jitter, sd in ((0.0, 0), (1.0, 5)):
        ref_px, ref_sites, band = S.fill([vol], shape, origin, h, jitter=jitter, seed=sd)
        assert band == 0
        px, sites = seed.fill(gpu_shape(vol), shape, origin, h, jitter=jitter, seed=sd, return_sites=True)
        np.testing.assert_array_equal(N(sites), ref_sites)
        assert N(px).tobytes() == ref_px.tobytes()
        every = S.positions(shape, origin, h, jitter, sd)
        value = rule(every)                                              # the closed form, away from its own rounding
        assert np.abs(value).min() > 1e-9
        np.testing.assert_array_equal(N(sites), np.flatnonzero(value < 0))
        x = N(px)
        assert x[:, 0].min() < -0.5 and x[:, 0].max() > 0.7 and x[:, 1].min() < -0.4 and x[:, 2].max() > 0.9   # beyond the box
    # jitter 0, the row of sites through the box at (j, k) = (12, 12): the centres next to -0.75 and +0.75, exclusive
    px, sites = seed.fill(gpu_shape(vol), shape, origin, h, jitter=0.0, return_sites=True)
    i, j, k = np.unravel_index(N(sites), shape)
    row = N(px)[(j == 12) & (k == 12)]
    assert 0 < row[0, 1] < 0.5 and 0 < row[0, 2] < 0.5 and row[:, 0].min() == -0.71875 and row[:, 0].max() == 0.71875


def test_jitter_zero_gives_exact_centres_and_jitter_stays_inside_the_cell():
    from mfs import seed
    shape, origin, h = (9, 10, 31), (0.3, -0.2, 0.1), 0.07
    neg = volume(*constant(-1.0)[:3])
    px, sites = seed.fill(neg, shape, origin, h, jitter=0.0, seed=99, return_sites=True)
    idx = np.stack(np.unravel_index(N(sites), shape), axis=-1).astype(np.float64)
    assert N(px).tobytes() == (np.asarray(origin) + (idx + 0.5) * h).tobytes()
    assert torch.equal(px, seed.fill(neg, shape, origin, h, jitter=0.0, seed=5))              # the seed does not matter
    for jitter, sd in ((1.0, 1), (0.25, 2 ** 40 + 7), (1.0, 2 ** 64 - 1)):
        got = N(seed.fill(neg, shape, origin, h, jitter=jitter, seed=sd))
        assert got.tobytes() == S.positions(shape, origin, h, jitter, sd).tobytes()
        assert (np.abs((got - np.asarray(origin)) / h - (idx + 0.5)) <= 0.5 * jitter + 1e-12).all()
    assert not torch.equal(seed.fill(neg, shape, origin, h, seed=1), seed.fill(neg, shape, origin, h, seed=2))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_and_inf_in_a_volume_keep_nothing_there(dtype):
    from mfs import seed
    vol = np.full((6, 6, 6), -1.0, dtype)
    vol[1, 1, 1], vol[4, 3, 2] = np.nan, np.inf
    o = S.shape_of(vol, (0, 0, 0), 0.2)
    shape, origin, h = (20, 20, 20), (0, 0, 0), 0.05                     # 4 sites per cell of the volume along each axis
    x = S.positions(shape, origin, h, 1.0, 2)
    kept, band, v, _ = S.decide([o], [], x)
    assert not band.any() and int(np.isnan(v).sum()) >= 8 * 64 and 0 < int(np.isposinf(v).sum())
    assert not kept[~np.isfinite(v)].any() and kept[np.isfinite(v)].all()
    px, sites = seed.fill(gpu_shape(o), shape, origin, h, seed=2, return_sites=True)
    np.testing.assert_array_equal(N(sites), np.flatnonzero(kept))
    cells = np.floor(N(px) / 0.2).astype(int)                            # no particle in a cell that touches either node
    for node in ((1, 1, 1), (4, 3, 2)):
        assert not ((cells >= np.asarray(node) - 1) & (cells <= np.asarray(node))).all(axis=1).any()
    # as an exclude, a NaN keeps nothing either: exc > clearance is false
    got = seed.fill(volume(*constant(-1.0)[:3]), shape, origin, h, exclude=gpu_shape(S.shape_of(np.where(np.isnan(vol), np.nan, 1.0).astype(dtype), (0, 0, 0), 0.2)),
                    seed=2, return_sites=True)[1]
    np.testing.assert_array_equal(N(got), np.flatnonzero(~np.isnan(v)))


@pytest.fixture(scope="module")
def sphere_sdf():
    from mfs import meshsdf
    from mfs.surface import Mesh
    v, f = M.icosphere(2, 0.2)
    return meshsdf.build(Mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV)), 0.025)


def test_shapes_from_meshes_and_bodies(sphere_sdf):
    import solver.sdf3D as sdf
    from mfs import seed
    vol = (N(sphere_sdf.phi), sphere_sdf.origin, sphere_sdf.spacing)     # the oracle samples the volume the GPU built
    shape, origin, h = (40, 44, 36), (-0.3, -0.33, -0.27), 0.015
    ref_px, ref_sites, band = S.fill([S.shape_of(*vol)], shape, origin, h, seed=21)
    assert band == 0
    px, sites = seed.fill(sphere_sdf, shape, origin, h, seed=21, return_sites=True)           # a MeshSDF, bare
    np.testing.assert_array_equal(N(sites), ref_sites)
    assert N(px).tobytes() == ref_px.tobytes()
    r = np.linalg.norm(ref_px, axis=1)
    inner = 0.2 * np.cos(M.max_facet_half_angle(*M.icosphere(2, 0.2)))   # the mesh lies between these two spheres
    assert r.max() < 0.2 + 0.5 * sphere_sdf.spacing and len(ref_px) > 4 / 3 * np.pi * (inner - 0.03) ** 3 / h ** 3
    # the same volume in a posed MeshBody
    body = sdf.MeshBody(sphere_sdf, center=(0.05, -0.02, 0.04), axis=(1, 2, 0.5), angle=33)
    pose = S.pose_of_row(body.row)
    ref_px, ref_sites, band = S.fill([S.shape_of(*vol, pose)], shape, origin, h, seed=21)
    assert band == 0
    px, sites = seed.fill([body], shape, origin, h, seed=21, return_sites=True)
    np.testing.assert_array_equal(N(sites), ref_sites)
    assert N(px).tobytes() == ref_px.tobytes()
    same = seed.fill(seed.Shape(sphere_sdf, center=(0.05, -0.02, 0.04), axis=(1, 2, 0.5), angle=33), shape, origin, h, seed=21)
    assert torch.equal(same, px)
    # a body as an exclude: the liquid of the bare sphere minus the posed one
    ref = S.fill([S.shape_of(*vol)], shape, origin, h, [S.shape_of(*vol, pose)], 0.0, 1.0, 21)
    assert ref[2] == 0 and 0 < len(ref[1]) < len(r)
    np.testing.assert_array_equal(N(seed.fill(sphere_sdf, shape, origin, h, exclude=[body], seed=21, return_sites=True)[1]), ref[1])


def test_a_skin_field_is_a_shape(sphere_sdf):
    """a previous run's skin as the liquid: SkinField has .phi / .origin / .spacing"""
    from mfs import seed, skin
    first = seed.fill(sphere_sdf, (32, 32, 32), (-0.24, -0.24, -0.24), 0.015, seed=4)
    f = skin.field(first, (41, 41, 41), (-0.3, -0.3, -0.3), 0.015)
    ref_px, ref_sites, band = S.fill([S.shape_of(N(f.phi), f.origin, f.spacing)], (30, 30, 30), (-0.3, -0.3, -0.3), 0.02, seed=8)
    assert band == 0 and len(ref_sites) > 1000
    px, sites = seed.fill(f, (30, 30, 30), (-0.3, -0.3, -0.3), 0.02, seed=8, return_sites=True)
    np.testing.assert_array_equal(N(sites), ref_sites)
    assert N(px).tobytes() == ref_px.tobytes()


def test_the_c_entry_points_refuse_bad_arguments_before_any_launch():
    from mfs import _lib
    lib = _lib.load()
    assert lib.mfs_seed_blocks3d(_lib.i64x((70, 66, 68))) == 1228 and lib.mfs_seed_blocks3d(_lib.i64x((1, 257, 1))) == 2
    assert lib.mfs_seed_blocks3d(None) == 0 and lib.mfs_seed_blocks3d(_lib.i64x((0, 4, 4))) == 0
    g, o, h = _lib.i64x((4, 5, 6)), _lib.f64x((0, 0, 0)), 0.1
    err = lambda: lib.mfs_last_error()  # noqa: E731
    buf = torch.zeros(64, dtype=torch.int64)                               # host memory: never dereferenced, nothing launches
    p = ctypes.c_void_p(buf.data_ptr())

    def shapes(m):
        vols = (ctypes.c_void_p * max(m, 1))(*([buf.data_ptr()] * max(m, 1)))
        pose = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        return (vols, (ctypes.c_int * max(m, 1))(*([1] * max(m, 1))), _lib.i64x([2, 2, 2] * max(m, 1)), _lib.f64x([0.0] * 3 * max(m, 1)),
                _lib.f64x([1.0] * max(m, 1)), _lib.f64x(pose * max(m, 1)))

    count = lambda g, o, h, jitter, ni, ne, sh, counts, masks: lib.mfs_seed_count3d(  # noqa: E731
        g, o, h, jitter, 7, ni, ne, *sh, 0.0, counts, masks, None)
    assert count(None, o, h, 1.0, 1, 0, shapes(1), p, p) == -1 and b"null" in err()
    assert count(g, None, h, 1.0, 1, 0, shapes(1), p, p) == -1 and b"null" in err()
    assert count(g, o, h, 1.0, 1, 0, (None,) + shapes(1)[1:], p, p) == -1 and b"null shape description" in err()
    null_volume = ((ctypes.c_void_p * 1)(None),) + shapes(1)[1:]
    assert count(g, o, h, 1.0, 1, 0, null_volume, p, p) == -1 and b"null shape volume" in err()
    assert count(g, o, h, 1.0, 1, 0, shapes(1), None, None) == -1 and b"null counts" in err()
    assert count(g, o, h, 1.0, 9, 8, shapes(17), p, p) == -1 and b"at most 16" in err()
    assert count(g, o, h, 1.0, 17, 0, shapes(17), p, p) == -1 and b"at most 16" in err()
    assert count(g, o, h, 1.0, 0, 1, shapes(1), p, p) == -1 and b"at least one include" in err()
    assert count(g, o, h, 1.5, 1, 0, shapes(1), p, p) == -1 and b"jitter" in err()
    assert count(g, o, h, -0.5, 1, 0, shapes(1), p, p) == -1 and b"jitter" in err()
    assert count(g, o, 0.0, 1.0, 1, 0, shapes(1), p, p) == -1 and b"spacing" in err()
    assert count(_lib.i64x((4, 0, 6)), o, h, 1.0, 1, 0, shapes(1), p, p) == -1 and b"extents" in err()
    assert count(_lib.i64x((2 ** 30, 512, 1)), o, h, 1.0, 1, 0, shapes(1), p, p) == -1 and b"workgroups" in err()
    thin = shapes(1)[:2] + (_lib.i64x([2, 1, 2]),) + shapes(1)[3:]
    assert count(g, o, h, 1.0, 1, 0, thin, p, p) == -1 and b"extents" in err()
    fill = lambda g, o, h, jitter, masks, offsets, px, dt, cap: lib.mfs_seed_fill3d(  # noqa: E731
        g, o, h, jitter, 7, masks, offsets, px, dt, None, cap, None)
    assert fill(g, o, h, 1.0, None, p, p, 1, 5) == -1 and b"null" in err()
    assert fill(g, o, h, 1.0, p, p, None, 1, 5) == -1 and b"null" in err()
    assert fill(None, o, h, 1.0, p, p, p, 1, 5) == -1 and b"null" in err()
    assert fill(g, o, h, 1.5, p, p, p, 1, 5) == -1 and b"jitter" in err()
    assert fill(g, o, h, 1.0, p, p, p, 7, 5) == -1 and b"dtype" in err()
    assert fill(g, o, h, 1.0, p, p, p, 1, 121) == -1 and b"capacity" in err()
    assert fill(g, o, h, 1.0, None, None, None, 1, 0) == 0                # nothing to store: no launch


def test_python_refuses_volumes_on_the_wrong_device():
    from mfs import seed
    gpu, cpu = volume(*constant(-1.0)[:3]), volume(*constant(-1.0)[:3])._replace(phi=torch.full((2, 2, 2), -1.0))
    with pytest.raises(TypeError, match="GPU"):
        seed.fill(gpu, (2, 2, 2), (0, 0, 0), 0.5, exclude=[cpu])
    with pytest.raises(TypeError, match="GPU"):
        seed.count([gpu, cpu], (2, 2, 2), (0, 0, 0), 0.5)
