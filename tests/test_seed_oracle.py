"""tests/seed_numpy.py, the oracle of liquid seeding, pinned to closed forms and to literal hash values; the quality of
the jitter hash; and what mfs.seed refuses without a device."""
import numpy as np
import pytest
import torch

import meshsdf_numpy as M
import seed_numpy as S


def halfspace(shape, origin, h, axis, offset, dtype=np.float64):
    """phi = x_axis - offset on a node lattice"""
    return (S.nodes(shape, origin, h)[..., axis] - offset).astype(dtype)


def test_jitter_zero_and_a_negative_volume_keep_every_site_at_its_centre():
    vol = S.shape_of(np.full((3, 3, 3), -1.0), (0, 0, 0), 0.5)
    shape, origin, h = (3, 5, 7), (0.125, -0.25, 0.0), 0.0625
    px, sites, band = S.fill([vol], shape, origin, h, jitter=0.0, seed=99)
    assert len(px) == 3 * 5 * 7 and band == 0
    np.testing.assert_array_equal(sites, np.arange(105))
    idx = np.stack(np.unravel_index(sites, shape), axis=-1)
    np.testing.assert_array_equal(px, np.asarray(origin) + (idx + 0.5) * h)       # dyadic: exact
    # jitter 1: still every site, every particle inside its own cell
    px1, sites1, _ = S.fill([vol], shape, origin, h, jitter=1.0, seed=99)
    assert len(px1) == 105 and (np.floor((px1 - np.asarray(origin)) / h) == idx).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_half_space_on_dyadic_coordinates_gives_the_closed_form_count(axis, dtype):
    # phi = x - 0.5 on nodes 0, 0.125, ..; sites of 0.0625 from 0: centres (i + 0.5) / 16 < 0.5 iff i <= 7
    vol = S.shape_of(halfspace((9, 9, 9), (0, 0, 0), 0.125, axis, 0.5, dtype), (0, 0, 0), 0.125)
    shape = (12, 13, 14)
    px, sites, band = S.fill([vol], shape, (0, 0, 0), 0.0625, jitter=0.0)
    assert len(px) == 8 * np.prod(shape) // shape[axis] and band == 0
    assert (px[:, axis] < 0.5).all() and sorted(set(np.unravel_index(sites, shape)[axis])) == list(range(8))
    # with jitter the count is the same: a particle stays inside its cell and no cell straddles x = 0.5
    assert len(S.fill([vol], shape, (0, 0, 0), 0.0625, jitter=1.0, seed=3)[0]) == len(px)


def test_both_comparisons_are_strict_at_exact_zeros():
    # centres at i / 16 exactly: origin -1/32.  include x - 0.5: the centre 0.5 (i = 8) samples exactly 0 and is NOT kept.
    inc = S.shape_of(halfspace((9, 3, 3), (0, 0, 0), 0.125, 0, 0.5), (0, 0, 0), 0.125)
    shape, origin, h = (12, 2, 2), (-0.03125, 0.0625, 0.0625), 0.0625
    x = S.positions(shape, origin, h, 0.0)
    kept, band, v, _ = S.decide([inc], [], x)
    i = np.unravel_index(np.arange(len(x)), shape)[0]
    assert (v[i == 8] == 0.0).all() and band[i == 8].all() and not band[i != 8].any()
    assert not kept[i == 8].any() and kept[i < 8].all() and not kept[i > 8].any()
    # exclude x - 0.25 with clearance 0.125: the centre 0.375 (i = 6) samples exactly the clearance and is NOT kept
    exc = S.shape_of(halfspace((9, 3, 3), (0, 0, 0), 0.125, 0, 0.25), (0, 0, 0), 0.125)
    kept, band, _, e = S.decide([inc], [exc], x, clearance=0.125)
    assert (e[i == 6] == 0.125).all() and set(i[kept]) == {7} and set(i[band]) == {6, 8}
    px, sites, nband = S.fill([inc], shape, origin, h, exclude=[exc], clearance=0.125, jitter=0.0)
    assert len(px) == 4 and nband == 8 and (px[:, 0] == 0.4375).all()
    # no excludes: the second condition is true
    assert S.decide([inc], [], x)[0].sum() == 8 * 4


def test_a_nan_sample_keeps_nothing():
    vol = np.full((3, 3, 3), -1.0)
    vol[1, 1, 1] = np.nan
    shape = (4, 4, 4)
    x = S.positions(shape, (0, 0, 0), 0.5, 1.0, 1)
    kept, _, v, _ = S.decide([S.shape_of(vol, (0, 0, 0), 1.0)], [], x)
    assert np.isnan(v).all() and not kept.any()                          # every cell of the volume touches the NaN node
    neg = S.shape_of(np.full((3, 3, 3), -1.0), (0, 0, 0), 1.0)
    kept, _, _, e = S.decide([neg], [S.shape_of(np.where(np.isnan(vol), np.nan, 1.0), (0, 0, 0), 1.0)], x)
    assert np.isnan(e).all() and not kept.any()
    # ... also next to a finite shape: the minimum carries the NaN
    assert not S.decide([neg, S.shape_of(vol, (0, 0, 0), 1.0)], [], x)[0].any()


def _mix_int(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xffffffff
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xffffffff
    x ^= x >> 16
    return x


def _hash_int(seed, s, a):
    h = _mix_int(seed & 0xffffffff)
    h = _mix_int(h ^ (seed >> 32))
    h = _mix_int(h ^ (s & 0xffffffff))
    h = _mix_int(h ^ (s >> 32))
    return _mix_int((h + (a + 1) * 0x9E3779B9) & 0xffffffff)


def test_hash_values_are_pinned():
    got = S.hash3(0, [0, 1, 5, 2 ** 32 + 5])
    assert got.dtype == np.uint32
    assert got.tolist() == [[0x01fce552, 0x04f8d29e, 0x0f8c1dbd], [0xb1313766, 0xcea49462, 0x884ac058],
                            [0xacb7ae16, 0xda790f8a, 0x5e415d77], [0x340705f6, 0xe2452bdc, 0x2019a50b]]
    for seed in (0, 7, 2 ** 40 + 7, 2 ** 64 - 1):                         # plain integers against numpy's uint32
        s = [0, 3, 255, 256, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 11]
        assert S.hash3(seed, s).tolist() == [[_hash_int(seed, v, a) for a in range(3)] for v in s]
    u = S.uniform(0, [0])
    assert u[0, 0] == (0x01fce552 >> 8) * 2.0 ** -24 - 0.5
    u = S.uniform(12345, np.arange(4096))
    assert u.min() >= -0.5 and u.max() < 0.5


def test_seed_and_the_high_word_of_the_site_index_enter_the_hash():
    s = np.arange(1000)
    assert (S.hash3(0, s) != S.hash3(1, s)).all(axis=1).mean() > 0.99
    assert (S.hash3(5, s) != S.hash3(2 ** 32 + 5, s)).all(axis=1).mean() > 0.99      # seed_hi
    a, b = S.hash3(0, [5]), S.hash3(0, [2 ** 32 + 5])                                 # s_hi
    assert (a != b).all()
    shape, origin = (3, 4, 5), (0, 0, 0)
    assert not np.array_equal(S.positions(shape, origin, 0.1, 1.0, 0), S.positions(shape, origin, 0.1, 1.0, 1))
    np.testing.assert_array_equal(S.positions(shape, origin, 0.1, 1.0, 4), S.positions(shape, origin, 0.1, 1.0, 4))


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 40 + 7])
def test_hash_quality_on_the_lattice_of_the_gpu_tests(seed):
    """conditions, not measurements: per-axis mean within 5 sigma (sigma = 1 / sqrt(12 N)); |correlation| sqrt(N) < 5
    between axes and between lattice neighbours along each axis; chi^2 on 64 bins (63 degrees of freedom) < 130"""
    shape = S.MAIN["shape"]
    n = int(np.prod(shape))
    u = S.uniform(seed, np.arange(n, dtype=np.uint64))
    assert (np.abs(u.mean(axis=0)) < 5.0 / np.sqrt(12.0 * n)).all(), u.mean(axis=0) * np.sqrt(12.0 * n)
    corr = lambda a, b: abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) * np.sqrt(a.size)  # noqa: E731
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert corr(u[:, a], u[:, b]) < 5, (a, b)
    g = u.reshape(shape + (3,))
    for comp in range(3):
        for axis in range(3):
            lo = [slice(None)] * 3
            hi = [slice(None)] * 3
            lo[axis], hi[axis] = slice(0, -1), slice(1, None)
            assert corr(g[tuple(lo) + (comp,)], g[tuple(hi) + (comp,)]) < 5, (comp, axis)
    for comp in range(3):
        hist = np.bincount(np.floor((u[:, comp] + 0.5) * 64).astype(np.int64), minlength=64)
        assert len(hist) == 64
        chi2 = ((hist - n / 64.0) ** 2 / (n / 64.0)).sum()
        assert chi2 < 130, (comp, chi2)


def test_the_float32_sampler_is_the_mesh_solids_sampler():
    rng = np.random.default_rng(5)
    vol = rng.standard_normal((6, 7, 5)).astype(np.float32)
    origin, h = (-0.3, 0.1, 0.2), 0.11
    xb = rng.uniform(-0.6, 1.0, size=(4000, 3))                          # inside, outside, beyond every face
    np.testing.assert_array_equal(S.sample(vol, origin, h, xb), M.sample(vol, origin, h, xb))
    np.testing.assert_array_equal(S.sample(vol.astype(np.float64), origin, h, xb), M.sample(vol, origin, h, xb))
    row = np.zeros((10, 4))
    row[1:4, 3] = (0.1, -0.2, 0.3)
    row[5:8, :3] = S.rotation((1, 2, 0.5), 33)
    np.testing.assert_array_equal(S.to_body(*S.pose_of_row(row), xb), M.to_body(row, xb))
    # beyond the box: the clamped sample plus the distance
    far = np.array([[-0.3 - 0.25, 0.1 + 0.11, 0.2 + 0.22]])
    assert S.sample(vol, origin, h, far)[0] == pytest.approx(float(vol[0, 1, 2]) + 0.25, abs=1e-15)


def test_the_main_case_of_the_gpu_tests():
    inc, exc = S.main_case()
    x = S.positions(S.MAIN["shape"], S.MAIN["origin"], S.MAIN["h"], S.MAIN["jitter"], S.MAIN["seed"])
    kept, band, vi, ve = S.decide(inc, exc, x)
    assert len(x) == 314160 and int((vi < 0).sum()) == 43335 and int(kept.sum()) == 25284 and int(band.sum()) == 0
    assert 2e-7 < min(np.abs(vi).min(), np.abs(ve).min()) < 3e-7 and S.band_eps(inc + exc, x) < 1e-13


def test_oracle_argument_errors():
    neg = S.shape_of(np.full((2, 2, 2), -1.0), (0, 0, 0), 1.0)
    with pytest.raises(ValueError, match="jitter"):
        S.fill([neg], (2, 2, 2), (0, 0, 0), 0.5, jitter=1.5)
    with pytest.raises(ValueError, match="include"):
        S.fill([], (2, 2, 2), (0, 0, 0), 0.5)
    with pytest.raises(ValueError, match="16"):
        S.fill([neg] * 9, (2, 2, 2), (0, 0, 0), 0.5, exclude=[neg] * 8)


def test_check_sizes_needs_no_device():
    from mfs import seed
    assert seed.check_sizes((70, 66, 68)) == (314160, 1228)
    assert seed.check_sizes((1, 1, 1)) == (1, 1) and seed.check_sizes((1, 257, 1)) == (257, 2)
    assert seed.check_sizes((2 ** 30, 511, 1))[1] == 2 ** 31 - 2 ** 22
    with pytest.raises(ValueError, match="workgroups"):
        seed.check_sizes((2 ** 30, 512, 1))
    with pytest.raises(ValueError, match="2\\^30"):
        seed.check_sizes((2 ** 30 + 1, 1, 1))
    with pytest.raises(ValueError, match="three extents"):
        seed.check_sizes((4, 4))
    with pytest.raises(ValueError, match="three extents"):
        seed.check_sizes((4, 0, 4))


def test_argument_errors_come_before_any_device_work():
    from mfs import seed
    from mfs.meshsdf import MeshSDF
    vol = MeshSDF(torch.full((3, 3, 3), -1.0), (0.0, 0.0, 0.0), 0.5, 1.0)
    ok = dict(shape=(4, 4, 4), origin=(0, 0, 0), spacing=0.25)
    for call in (seed.fill, seed.count):
        with pytest.raises(TypeError, match="GPU"):                      # a CPU tensor: no fallback
            call(vol, **ok)
        with pytest.raises(TypeError, match="GPU"):
            call([seed.Shape(vol, center=(0.1, 0, 0), axis=(0, 0, 1), angle=30)], exclude=vol, **ok)
        with pytest.raises(TypeError, match="GPU"):
            call(vol._replace(phi=np.full((3, 3, 3), -1.0)), **ok)
        with pytest.raises(TypeError, match="Shape"):
            call([3.0], **ok)
        for kw in (dict(spacing=0.0), dict(spacing=float("nan")), dict(origin=(0, float("inf"), 0)), dict(shape=(4, 4)),
                   dict(shape=(4, 0, 4)), dict(shape=(2 ** 30, 512, 1)), dict(dtype=torch.float16),
                   dict(clearance=float("nan")), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)):
            with pytest.raises(ValueError):
                call(vol, **{**ok, **kw})
        with pytest.raises(ValueError, match=r"jitter must be in \[0, 1\]"):
            call(vol, **ok, jitter=1.5)
        with pytest.raises(ValueError, match=r"jitter must be in \[0, 1\]"):
            call(vol, **ok, jitter=-0.1)
        with pytest.raises(ValueError, match="at least 1"):
            call([], **ok)
        with pytest.raises(ValueError, match="at most 16"):
            call([vol] * 9, exclude=[vol] * 8, **ok)
        for bad in (torch.zeros((3, 3)), torch.zeros((3, 1, 3)), torch.zeros((3, 3, 3), dtype=torch.float16),
                    torch.zeros((3, 3, 6))[:, :, ::2]):
            with pytest.raises(ValueError, match="phi"):
                call(vol._replace(phi=bad), **ok)
        with pytest.raises(ValueError, match="spacing"):
            call(vol._replace(spacing=0.0), **ok)


def test_shapes_take_the_pose_convention_of_mesh_bodies():
    from mfs import seed
    from mfs.meshsdf import MeshSDF
    from solver import sdf3D
    vol = MeshSDF(torch.full((3, 3, 3), -1.0), (0.0, 0.0, 0.0), 0.5, 1.0)
    s = seed.Shape(vol, center=(0.02, 0.31, -0.01), axis=(1, 2, 0.5), angle=33)
    np.testing.assert_array_equal(s.R, S.rotation((1, 2, 0.5), 33))
    np.testing.assert_array_equal(s.T, [0.02, 0.31, -0.01])
    bare = seed.as_shape(vol)
    assert bare.volume is vol and (bare.R == np.eye(3)).all() and (bare.T == 0).all() and seed.as_shape(s) is s
    body = sdf3D.MeshBody.__new__(sdf3D.MeshBody)                         # the constructor wants a GPU volume
    body.sdf, body.row = vol, np.zeros((1, 10, 4))
    body.row[0, 1:5, :], body.row[0, 5:9, :] = sdf3D.get_T((0.02, 0.31, -0.01)), sdf3D.get_R([1, 2, 0.5], 33)
    b = seed.as_shape(body)
    assert b.volume is vol and (b.R == s.R).all() and (b.T == s.T).all()
