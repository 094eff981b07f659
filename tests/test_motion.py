"""mfs.motion on CPU tensors: `BodyKinematics` integrates prescribed linear / angular velocities into the packed rigid
bodies of solver.sdf3D / solver.sdf2D, in place; the slab time steps refuse moving bodies before they need a process group."""
import numpy as np
import pytest
import torch

from mfs.motion import BodyKinematics, Motion
import notebook_sim as NSIM
import solver.sdf2D as S2
import solver.sdf3D as S3


def bodies3():
    rb_d, rb_map = S3.generate_rb(None, {}, "tank", ['box', 0.5, 0.8, 0.5], flip=True, center=[0, 0.5, 0], device="cpu")
    rb_d, rb_map = S3.generate_rb(rb_d, rb_map, "ball", ['sphere', 0.08], center=[-0.1, 0.5, 0.0])
    rb_d, rb_map = S3.generate_rb(rb_d, rb_map, "bar", ['box', 0.3, 0.1, 0.2], center=[0.1, 0.3, 0.05], axis=[0, 0, 1], angle=20)
    rb_d, rb_map = S3.generate_rb(rb_d, rb_map, "can", ['cylinder', 0.05, 0.4], center=[0.0, 0.4, 0.1], axis=[1, 0, 1], angle=35)
    return rb_d, rb_map


def bodies2():
    rb_d, rb_map = S2.generate_rb(None, {}, "tank", ['box', 1.0, 1.4], flip=True, center=[0.3, 0.8], device="cpu")
    rb_d, rb_map = S2.generate_rb(rb_d, rb_map, "paddle", ['box', 0.3, 0.05], center=[0.2, 0.4], angle=25)
    rb_d, rb_map = S2.generate_rb(rb_d, rb_map, "disc", ['sphere', 0.1], center=[0.5, 0.6])
    return rb_d, rb_map


DTS = [1 / 300, 0.0017, 1 / 300, 0.0005, 0.0029]


def test_constant_velocity_over_uneven_steps_3d():
    rb_d, m = bodies3()
    v = np.array([0.6, -0.1, 0.15])
    kin = BodyKinematics(rb_d, {m["ball"]: Motion(velocity=v)}, 3)
    t = 0.0
    for dt in DTS:
        kin.advance(t, dt)
        t += dt
    i = m["ball"]
    np.testing.assert_allclose(rb_d[i, 1:4, 3].numpy(), np.array([-0.1, 0.5, 0.0]) + v * sum(DTS), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(rb_d[i, 9, :3].numpy(), v)                       # row 9: what `evaluate` hands out as sv
    np.testing.assert_array_equal(rb_d[i, 1:5, :3].numpy(), np.identity(4)[:, :3])  # the rest of the translation block
    np.testing.assert_array_equal(rb_d[i, 5:9].numpy(), np.identity(4))            # omega = 0: the rotation stays put
    assert float(kin.rb_w.abs().max()) == 0.0 and tuple(kin.rb_w.shape) == (4, 3)


def test_constant_velocity_over_uneven_steps_2d():
    rb_d, m = bodies2()
    v = np.array([0.3, 0.0])
    kin = BodyKinematics(rb_d, {m["disc"]: Motion(velocity=v)}, 2)
    t = 0.0
    for dt in DTS:
        kin.advance(t, dt)
        t += dt
    np.testing.assert_allclose(rb_d[m["disc"], 1:3, 2].numpy(), np.array([0.5, 0.6]) + v * sum(DTS), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(rb_d[m["disc"], 7, :2].numpy(), v)
    assert tuple(kin.rb_w.shape) == (3,)


def test_constant_omega_about_a_tilted_axis():
    """40 steps of w = |w| axis: the rotation is get_R(axis, total angle) (the body started unrotated), orthonormal to 1e-14"""
    rb_d, m = bodies3()
    axis = np.array([1.0, 2.0, -0.5])
    axis /= np.linalg.norm(axis)
    rate, dt = 2.5, 1 / 300
    kin = BodyKinematics(rb_d, {m["ball"]: Motion(omega=rate * axis)}, 3)
    for s in range(40):
        kin.advance(s * dt, dt)
    R = rb_d[m["ball"], 5:9].numpy()
    want = S3.get_R(list(axis), np.degrees(rate * dt * 40))
    np.testing.assert_allclose(R, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(R[:3, :3].T @ R[:3, :3], np.identity(3), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(kin.rb_w[m["ball"]].numpy(), rate * axis)
    np.testing.assert_array_equal(rb_d[m["ball"], 1:4, 3].numpy(), [-0.1, 0.5, 0.0])   # about its own centre


def test_rotation_composes_with_the_initial_pose():
    """a body that starts rotated: R <- Rot(w dt) R, in 3D (same axis: angles add) and in 2D"""
    rb_d, m = bodies3()
    kin = BodyKinematics(rb_d, {m["bar"]: Motion(omega=[0, 0, 1.5])}, 3)
    for s in range(10):
        kin.advance(0.0, 0.002)
    np.testing.assert_allclose(rb_d[m["bar"], 5:9].numpy(), S3.get_R([0, 0, 1], 20 + np.degrees(1.5 * 0.02)), rtol=0, atol=1e-12)
    rb2, m2 = bodies2()
    kin2 = BodyKinematics(rb2, {m2["paddle"]: Motion(omega=2.0)}, 2)
    for s in range(10):
        kin2.advance(0.0, 0.002)
    np.testing.assert_allclose(rb2[m2["paddle"], 4:7].numpy(), S2.get_R(None, 25 + np.degrees(2.0 * 0.02)), rtol=0, atol=1e-12)
    assert float(kin2.rb_w[m2["paddle"]]) == 2.0


def test_schedules_are_sampled_at_the_start_of_the_step():
    rb_d, m = bodies3()
    seen = []

    def vel(t):
        seen.append(t)
        return [t, 0.0, 2 * t]

    kin = BodyKinematics(rb_d, {m["ball"]: Motion(velocity=vel, omega=lambda t: [0.0, 10 * t, 0.0])}, 3)
    kin.advance(0.5, 0.1)
    assert seen == [0.5]
    np.testing.assert_allclose(rb_d[m["ball"], 1:4, 3].numpy(), [-0.1 + 0.05, 0.5, 0.1], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(rb_d[m["ball"], 9, :3].numpy(), [0.5, 0.0, 1.0])
    np.testing.assert_array_equal(kin.rb_w[m["ball"]].numpy(), [0.0, 5.0, 0.0])
    np.testing.assert_allclose(rb_d[m["ball"], 5:9].numpy(), S3.get_R([0, 1, 0], np.degrees(0.5)), rtol=0, atol=1e-15)
    kin.advance(0.6, 0.1)
    assert seen == [0.5, 0.6]
    np.testing.assert_allclose(rb_d[m["ball"], 1:4, 3].numpy(), [-0.1 + 0.05 + 0.06, 0.5, 0.1 + 0.12], rtol=0, atol=1e-15)


def test_bodies_at_rest_keep_their_rows_bit_for_bit():
    rb_d, m = bodies3()
    S3.set_vel_rb(rb_d, m["can"], [0.1, 0.2, 0.3])
    before = rb_d.clone()
    kin = BodyKinematics(rb_d, {m["ball"]: Motion(velocity=[0.6, 0, 0.15], omega=[0, 1, 0])}, 3)
    same = torch.equal(rb_d, before)
    for s in range(7):
        kin.advance(s / 300, 1 / 300)
    rest = [i for i in range(4) if i != m["ball"]]
    assert same and torch.equal(rb_d[rest], before[rest])
    assert torch.equal(rb_d[m["ball"], 0], before[m["ball"], 0])          # the shape parameters never change
    assert not torch.equal(rb_d[m["ball"]], before[m["ball"]])
    assert float(kin.rb_w[rest].abs().max()) == 0.0
    rb2, m2 = bodies2()
    before2 = rb2.clone()
    kin2 = BodyKinematics(rb2, {m2["paddle"]: Motion(omega=2.0)}, 2)
    kin2.advance(0.0, 0.01)
    rest2 = [m2["tank"], m2["disc"]]
    assert torch.equal(rb2[rest2], before2[rest2]) and not torch.equal(rb2[m2["paddle"]], before2[m2["paddle"]])


def test_max_surface_speed():
    rb_d, m = bodies3()
    v, w = np.array([0.3, 0.0, 0.4]), np.array([0.0, 2.0, 0.0])
    for name, rho in (("ball", 0.08), ("bar", np.sqrt(0.3 ** 2 + 0.1 ** 2 + 0.2 ** 2)), ("can", np.sqrt(0.05 ** 2 + 0.4 ** 2))):
        kin = BodyKinematics(rb_d, {m[name]: Motion(velocity=v, omega=w)}, 3)
        assert kin.max_surface_speed(0.0) == pytest.approx(0.5 + 2.0 * rho, rel=1e-14)
    # the maximum over the moving bodies, schedules evaluated at t
    kin = BodyKinematics(rb_d, {m["ball"]: Motion(velocity=lambda t: [t, 0, 0]), m["can"]: Motion(velocity=[0, 0.2, 0])}, 3)
    assert kin.max_surface_speed(0.0) == pytest.approx(0.2) and kin.max_surface_speed(3.0) == pytest.approx(3.0)
    rb2, m2 = bodies2()
    kin2 = BodyKinematics(rb2, {m2["paddle"]: Motion(velocity=[0.3, 0.4], omega=-2.0)}, 2)
    assert kin2.max_surface_speed(0.0) == pytest.approx(0.5 + 2.0 * np.sqrt(0.3 ** 2 + 0.05 ** 2), rel=1e-14)
    assert BodyKinematics(rb2, {}, 2).max_surface_speed(0.0) == 0.0


def test_misuse():
    rb_d, m = bodies3()
    with pytest.raises(ValueError, match="no body 7"):
        BodyKinematics(rb_d, {7: Motion()}, 3)
    with pytest.raises(TypeError, match="Motion"):
        BodyKinematics(rb_d, {0: [1, 0, 0]}, 3)
    with pytest.raises(ValueError, match="rb_d"):
        BodyKinematics(rb_d, {0: Motion()}, 2)


@pytest.mark.parametrize("cls", [NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation])
def test_the_slab_time_steps_refuse_moving_bodies(cls):
    """at the argument check: no process group, no device, no scene is needed to get the answer"""
    with pytest.raises(ValueError, match="motion"):
        cls(dist=None, motion={1: Motion(velocity=[0.1, 0, 0])})
