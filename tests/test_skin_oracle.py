"""tests/skin_numpy.py, the oracle of the liquid skin, pinned to closed forms; and what mfs.skin refuses without a device."""
import numpy as np
import pytest
import torch

import skin_numpy as S


def test_one_particle_is_its_exact_sphere_inside_R_and_background_outside():
    h, r, R = 0.05, 0.15, 0.2
    xp = np.array([0.31, 0.283, 0.337])
    shape = (13, 12, 14)
    phi, K = S.field(xp[None], shape, (0, 0, 0), h, r, R)
    rel, _ = S.nodes(shape, (0, 0, 0), h)
    dist = np.linalg.norm(rel - xp, axis=-1)
    inside = dist < R
    assert 30 < inside.sum() < inside.size - 30 and (np.abs(dist - R) > 1e-6).all()
    np.testing.assert_array_equal(K, inside.astype(np.int64))
    np.testing.assert_allclose(phi[inside], dist[inside] - r, rtol=0, atol=1e-15)
    assert (phi[~inside] == R - r).all() and S.background(r, R) == R - r
    # continuous at the rim: the sphere's distance there is the background
    assert phi[inside].max() < R - r and phi[inside].max() > R - r - h


def test_two_particles_give_minus_r_at_their_midpoint():
    h, r, R = 0.125, 0.2, 0.45
    a, b = np.array([0.375 - 0.11, 0.5, 0.25]), np.array([0.375 + 0.11, 0.5, 0.25])
    phi, K = S.field(np.stack([a, b]), (8, 9, 5), (0, 0, 0), h, r, R)
    assert K[3, 4, 2] == 2 and phi[3, 4, 2] == pytest.approx(-r, abs=1e-16)
    phi32, _ = S.field(np.stack([a, b]), (8, 9, 5), (0, 0, 0), h, r, R, np.float32)
    assert phi32.dtype == np.float32 and phi32[3, 4, 2] == pytest.approx(-r, abs=1e-7)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_particle_exactly_R_away_contributes_nothing(dtype):
    h, r, R = 0.125, 0.125, 0.25                                        # dyadic: every product below is exact
    phi, K = S.field(np.array([[0.5, 0.5, 0.5]]), (9, 9, 9), (0, 0, 0), h, r, R, dtype)
    assert K[4, 4, 4] == 1 and phi[4, 4, 4] == -r
    for node in ((2, 4, 4), (6, 4, 4), (4, 2, 4), (4, 4, 6)):           # exactly R = 2 h away along an axis
        assert K[node] == 0 and phi[node] == R - r
    assert K[3, 4, 4] == 1 and phi[3, 4, 4] == h - r
    assert K.sum() == 1 + 6 + 12 + 8                                    # |offset|^2 in h^2: 0, 1, 2, 3 -- 4 is out


def test_no_particles_is_all_background():
    phi, K = S.field(np.zeros((0, 3)), (3, 4, 5), (1, 2, 3), 0.1, 0.1, 0.25)
    assert (phi == 0.25 - 0.1).all() and (K == 0).all()


def test_the_cloud_of_the_gpu_tests():
    px = S.cloud()
    assert px.shape == (1680, 3)
    phi, K = S.field(px, (27, 23, 30), (0.1, 0.12, 0.08), 0.05, 0.05, 0.125)
    assert phi.size == 18630 and 0.77 < (K == 0).mean() < 0.79 and K.max() == 75
    assert -0.05 <= phi.min() < -0.049                                  # interior nodes come out near -r


def test_check_sizes_needs_no_device():
    from mfs import skin
    assert skin.check_sizes((27, 23, 30), 1680) == 18630
    assert skin.check_sizes((1024, 1024, 2047)) == 2 ** 31 - 2 ** 20
    with pytest.raises(ValueError, match="nodes do not fit"):
        skin.check_sizes((2048, 1024, 1024))
    with pytest.raises(ValueError, match="particles do not fit"):
        skin.check_sizes((4, 4, 4), 2 ** 31)
    with pytest.raises(ValueError, match=">= 2"):
        skin.check_sizes((4, 1, 4))
    with pytest.raises(ValueError, match="three extents"):
        skin.check_sizes((4, 4))


def test_the_c_entry_points_refuse_bad_arguments_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    lib = _lib.load()
    g, o, h = _lib.i64x((9, 10, 11)), _lib.f64x((0, 0, 0)), 0.05
    assert lib.mfs_skin_bricks3d(g) == 3 * 2 * 2 and lib.mfs_skin_bins3d(g) == 5 * 4 * 4
    assert lib.mfs_skin_bricks3d(None) == 0 and lib.mfs_skin_bins3d(_lib.i64x((0, 4, 4))) == 0
    field = lambda *a: lib.mfs_skin_field3d(*a, None)  # noqa: E731
    assert field(g, o, h, h, 2.5 * h, None, 1, 0, None, None, None) == -1 and b"null" in lib.mfs_last_error()
    assert field(g, o, h, h, 2.5 * h, None, 1, 5, None, None, None) == -1 and b"null particles" in lib.mfs_last_error()
    assert field(None, o, h, h, 2.5 * h, None, 1, 0, None, None, None) == -1 and b"null" in lib.mfs_last_error()
    assert field(g, o, h, h, 4.5 * h, None, 1, 0, None, None, None) == -1 and b"4 * spacing" in lib.mfs_last_error()
    assert field(g, o, h, h, h, None, 1, 0, None, None, None) == -1 and b"radius < influence" in lib.mfs_last_error()
    assert field(g, o, 0.0, h, 2.5 * h, None, 1, 0, None, None, None) == -1 and b"spacing" in lib.mfs_last_error()
    assert field(g, o, h, h, 2.5 * h, None, 7, 0, None, None, None) == -1 and b"dtype" in lib.mfs_last_error()
    assert field(g, o, h, h, 2.5 * h, None, 1, 2 ** 31, None, None, None) == -1 and b"2^31" in lib.mfs_last_error()
    assert field(_lib.i64x((2048, 1024, 1024)), o, h, h, 2.5 * h, None, 1, 0, None, None, None) == -1
    assert b"2^31" in lib.mfs_last_error()
    keys = lambda *a: lib.mfs_skin_keys3d(*a, None)  # noqa: E731
    assert keys(g, o, h, None, 1, 5, None) == -1 and b"null" in lib.mfs_last_error()
    assert keys(g, o, h, None, 1, 2 ** 31, None) == -1 and b"2^31" in lib.mfs_last_error()
    assert keys(g, o, h, None, 1, 0, None) == 0                          # nothing to do: no launch


def test_defaults_follow_the_level_set_radius_rule():
    from mfs import skin
    assert skin.default_radius(0.05) == pytest.approx(1.02 * np.sqrt(3) / 2 * 0.05, rel=1e-15)
    assert 3 * skin.default_radius(1.0) < skin.REACH                     # the default influence fits one ring of bricks


def test_argument_errors_come_before_any_device_work():
    from mfs import skin
    px = torch.zeros((5, 3), dtype=torch.float64)
    ok = dict(shape=(5, 6, 7), origin=(0, 0, 0), spacing=0.1)
    with pytest.raises(TypeError, match="GPU"):
        skin.field(px, **ok)
    with pytest.raises(TypeError, match="GPU"):
        skin.mesh(px, **ok)
    with pytest.raises(TypeError, match="GPU"):
        skin.field(np.zeros((5, 3)), **ok)
    for bad in (torch.zeros((5, 2), dtype=torch.float64), torch.zeros(15, dtype=torch.float64),
                torch.zeros((5, 3), dtype=torch.float16), torch.zeros((5, 3), dtype=torch.int64),
                torch.zeros((3, 5), dtype=torch.float64).t()):
        with pytest.raises(ValueError, match="px"):
            skin.field(bad, **ok)
    for kw in (dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=float("nan")), dict(radius=0.0), dict(radius=-0.1),
               dict(radius=0.1, influence=0.1), dict(radius=0.1, influence=0.05), dict(origin=(0, float("inf"), 0)),
               dict(shape=(5, 1, 7)), dict(shape=(2048, 1024, 1024))):
        with pytest.raises(ValueError):
            skin.field(px, **{**ok, **kw})
    with pytest.raises(ValueError, match=r"must not exceed 4 \* spacing"):
        skin.field(px, **ok, radius=0.3, influence=0.41)
    with pytest.raises(ValueError, match=r"must not exceed 4 \* spacing"):
        skin.field(px, **ok, radius=1.4 * 0.1)                           # its default influence, 3 r, is 4.2 h
