"""2D rigid-body signed distances on the MI355X against goldens produced by executing the reference's solver/sdf2D.py
(tests/golden/make_goldens_density2d.py, sdf2d_*), through the drop-in module's own generate_rb / set_vel_rb (so the
packed body layout is checked too), and at 1 M points against the numpy restatement (tests/density2d_numpy.py).
Tolerances of tests/test_sdf_gpu.py: sd 1e-13 (sqrt vs pow, FMA contraction off), velocities exact, float64 positions
1e-15, float32 positions 1.2e-7."""
import numpy as np
import pytest
import torch

import density2d_numpy as DN
from conftest import golden, golden_names
from mfs import scenes
import solver.sdf2D as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
N = lambda t: t.detach().cpu().numpy()  # noqa: E731


def scene_bodies(sc):
    rb_d, rb_map = None, {}
    for i, b in enumerate(sc["bodies"]):
        rb_d, rb_map = S.generate_rb(rb_d, rb_map, b["name"], b["rbparam"], flip=b["flip"], center=b["center"],
                                     angle=b["angle"], device=DEV)
        S.set_vel_rb(rb_d, i, b["vel"])
    return rb_d, rb_map


def test_generate_rb_layout_matches_reference():
    rb_d, rb_map = scene_bodies(scenes.density_scene_2d((32, 32), 41))
    assert rb_map == {"tank": 0, "bar": 1, "ball": 2}
    np.testing.assert_allclose(N(rb_d), golden("sdf2d_a_f64")["rb_d"], rtol=0, atol=1e-16)
    assert S.generate_rb(rb_d, rb_map, "x", ["cylinder", 1, 2]) is rb_d            # unknown shape: the bare rb_d
    S.transform_rb(rb_d, 1, center=[0.1, 0.2], axis=[0, 1], angle=90)
    np.testing.assert_allclose(N(rb_d[1, 1:3, 2]), [0.1, 0.2])
    np.testing.assert_allclose(N(rb_d[1, 4:6, :2]), [[0, -1], [1, 0]], atol=1e-15)


@pytest.mark.parametrize("name", golden_names("sdf2d_"))
def test_evaluate_and_project(name):
    g = golden(name)
    rb_d, pos = T(g["rb_d"]), T(g["position"])
    n = pos.shape[0]
    sd = torch.full((n,), 9.0, dtype=torch.float64, device=DEV)
    vel = torch.full((n, 2), 9.0, dtype=torch.float64, device=DEV)
    S.evaluate(rb_d, sd, vel, pos)
    np.testing.assert_allclose(N(sd), g["sd"], rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(N(vel), g["vel"])
    proj = pos.clone()
    S.project(rb_d, proj)
    np.testing.assert_allclose(N(proj), g["projected"], rtol=0, atol=1e-15 if proj.dtype == torch.float64 else 1.2e-7)
    # any leading shape with last dimension 2
    P2 = pos[:1000].reshape(10, 100, 2).contiguous()
    sd2 = torch.zeros(10, 100, dtype=torch.float64, device=DEV)
    vel2 = torch.ones(10, 100, 2, dtype=torch.float64, device=DEV)
    S.evaluate(rb_d, sd2, vel2, P2)
    np.testing.assert_array_equal(N(sd2).reshape(-1), N(sd)[:1000])
    np.testing.assert_array_equal(N(vel2).reshape(-1, 2), N(vel)[:1000])


def test_box_faces_sphere_centres_and_ties():
    """points exactly on a box face, at a sphere's centre (solid: stays; flipped: goes to (cx + r, cy)), within 1e-4 of
    it, two coincident bodies (the first wins the tie, so its velocity is reported), and a flipped sphere elsewhere"""
    rb_d, m = S.generate_rb(None, {}, "a", ["box", 1.0, 0.5], flip=False, center=[0.0, 0.0], device=DEV)
    rb_d, m = S.generate_rb(rb_d, m, "b", ["box", 1.0, 0.5], flip=False, center=[0.0, 0.0], device=DEV)
    rb_d, m = S.generate_rb(rb_d, m, "s", ["sphere", 0.25], flip=False, center=[2.0, 0.0], device=DEV)
    rb_d, m = S.generate_rb(rb_d, m, "f", ["sphere", 0.5], flip=True, center=[4.0, 1.0], device=DEV)
    S.set_vel_rb(rb_d, 0, [1.0, 2.0])
    S.set_vel_rb(rb_d, 1, [3.0, 4.0])
    pos = np.array([[0.5, 0.1], [0.0, -0.25], [0.5, 0.25], [0.2, 0.1], [2.0, 0.0], [2.00005, 0.0], [4.0, 1.0], [2.1, 0.0]])
    sd = torch.zeros(len(pos), dtype=torch.float64, device=DEV)
    vel = torch.zeros(len(pos), 2, dtype=torch.float64, device=DEV)
    S.evaluate(rb_d, sd, vel, T(pos))
    rsd, rvel = DN.sdf_evaluate(N(rb_d), pos)
    np.testing.assert_allclose(N(sd), rsd, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(N(vel), rvel)
    # everything outside the flipped sphere is "inside" it (its distance is negated), so it wins at all these points but
    # its own centre's neighbourhood: negative distances, its zero velocity
    assert (N(sd)[:6] < -1.5).all() and not N(vel)[:6].any()
    # the three solid bodies alone: on a face / a corner the distance is exactly 0, which counts as inside (`<= 0`), and
    # of the two coincident boxes the first wins the tie (`d < min_sd`), so ITS velocity is reported
    solid = rb_d[:3].contiguous()
    S.evaluate(solid, sd, vel, T(pos))
    rsd, rvel = DN.sdf_evaluate(N(solid), pos)
    np.testing.assert_allclose(N(sd), rsd, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(N(vel), rvel)
    assert N(sd)[0] == 0.0 and N(sd)[1] == 0.0 and N(sd)[2] == 0.0
    np.testing.assert_array_equal(N(vel)[:4], [[1.0, 2.0]] * 4)
    assert N(sd)[4] == -0.25 and not N(vel)[4:].any()                       # the sphere's centre; sphere velocity 0
    assert N(sd)[6] > 0                                                     # outside all three
    proj, rproj = T(pos), pos.copy()
    S.project(rb_d, proj)
    DN.sdf_project(N(rb_d), rproj)
    np.testing.assert_allclose(N(proj), rproj, rtol=0, atol=1e-15)
    # every point ends in the flipped sphere (it is applied last); the one at its centre went to (cx + r, cy)
    np.testing.assert_array_equal(N(proj)[6], [4.5, 1.0])


@pytest.mark.parametrize("dt", [np.float64, np.float32], ids=["f64", "f32"])
def test_one_million_points_against_the_restatement(dt):
    sc = scenes.density_scene_2d((64, 48), 5, bound_size=(1.0, 0.8))
    rng = np.random.default_rng(8)
    lo, sz = np.array(sc["bound_min"]), np.array(sc["bound_size"])
    pos = rng.uniform(lo - 0.05 * sz, lo + 1.05 * sz, size=(1 << 20, 2)).astype(dt)
    rb_d = T(sc["rb_d"])
    sd = torch.zeros(len(pos), dtype=torch.float64, device=DEV)
    vel = torch.zeros(len(pos), 2, dtype=torch.float64, device=DEV)
    S.evaluate(rb_d, sd, vel, T(pos))
    rsd, rvel = DN.sdf_evaluate(sc["rb_d"], pos)
    np.testing.assert_allclose(N(sd), rsd, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(N(vel), rvel)
    proj, rproj = T(pos), pos.copy()
    S.project(rb_d, proj)
    DN.sdf_project(sc["rb_d"], rproj)
    np.testing.assert_allclose(N(proj), rproj, rtol=0, atol=1e-15 if dt == np.float64 else 1.2e-7)
    # at least the points outside the container move: the sample box is 1.1 x 1.1 of the bounds and the container
    # (1 - 3/64) x (1 - 3/48) of them, so 1 - 0.893 / 1.21 = 26 % lie outside it (the bodies and last-bit rewrites add more)
    assert (N(proj) != pos).any(axis=1).mean() > 0.25


def test_no_bodies_and_misuse():
    rb = torch.zeros((0, 8, 3), dtype=torch.float64, device=DEV)
    pos = torch.rand((50, 2), dtype=torch.float64, device=DEV)
    sd, vel = torch.zeros(50, dtype=torch.float64, device=DEV), torch.ones((50, 2), dtype=torch.float64, device=DEV)
    S.evaluate(rb, sd, vel, pos)
    assert float(sd.min()) == 100.0 and float(vel.abs().max()) == 0.0
    before = pos.clone()
    S.project(rb, pos)
    assert torch.equal(pos, before)
    with pytest.raises(ValueError, match="rb_d"):
        S.project(torch.zeros((1, 10, 4), dtype=torch.float64, device=DEV), pos)
