"""Moving rigid bodies in the 3D time step (NotebookSimulation(..., motion=...)) on the MI355X against a golden produced by
executing the reference (tests/golden/make_goldens_moving.py): the scene of tests/test_timestep_gpu.py plus a sphere of
radius 0.08 that starts 0.06 inside the fluid block and moves at (0.6, 0, 0.15); three steps, each of which the generator
runs as advect -> centre += v dt -> the reference's transform_rb, set_vel_rb, evaluate -> project -> the rest.
Bounds: the solid level set per step as tests/test_timestep_gpu.py::test_scene_setup_matches_reference asks (rtol 1e-13,
atol 1e-15), the step state within test_two_full_steps' bounds."""
import numpy as np
import pytest
import torch

from conftest import golden
from mfs.motion import Motion
import notebook_sim as NSIM
import solver.sdf3D as sdf
from solver.SolidFraction3D import compute_solid_frac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
NAME = "step_moving_12x16x12"


def build(g, omega=None):
    gres = tuple(int(v) for v in g["gres"])
    gdx = float(g["gdx"])
    size = np.array(gres) * gdx
    rb_d, rb_map = sdf.generate_rb(None, {}, 'cube', ['box', size[0] - 2 * gdx, size[1] - 2 * gdx, size[2] - 2 * gdx], flip=True,
                                   center=[0, size[1] / 2, 0], axis=[0., 1, 0], angle=0, device=DEV)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.05, 0.8], flip=False, center=[-0.12, 0.2, 0],
                                   axis=[0., 0, 1], angle=-35)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ball', ['sphere', 0.08], flip=False, center=[-0.1, 0.5, 0.0])
    np.testing.assert_allclose(N(rb_d), g["rb_d"], rtol=0, atol=1e-16)
    assert rb_map["ball"] == int(g["ball"])
    motion = {rb_map["ball"]: Motion(velocity=g["ball_v"], omega=omega)}
    sim = NSIM.NotebookSimulation(gres, gdx, [-0.3, 0, -0.3], rb_d, g["px0"], float(g["pdx"]), rho=float(g["rho"]),
                                  mu=float(g["mu"]), dt=float(g["dt"]), device=DEV, motion=motion)
    sim.particle.v.copy_(torch.as_tensor(g["pv0"], device=DEV))
    return sim, rb_d


def test_three_steps_against_the_executed_reference():
    g = golden(NAME)
    sim, rb_d = build(g)
    np.testing.assert_allclose(N(sim.solid_levelset.phi), g["sphi0"], rtol=1e-13, atol=1e-15)
    assert int(g["steps"]) == 3 and int(g["moved_by_sphere"][0]) >= 50
    timings = {}
    for s in range(3):
        dt = sim.step(timings=timings)
        assert dt == pytest.approx(float(g["dts"][s]), rel=1e-12)
        np.testing.assert_allclose(N(sim.solid_levelset.phi), g[f"sphi{s + 1}"], rtol=1e-13, atol=1e-15)
        px, pv = N(sim.particle.x), N(sim.particle.v)
        move = np.abs(g[f"px{s + 1}"] - g["px0"]).max()
        gvy = g[f"gvy{s + 1}"]
        devs = dict(px=np.abs(px - g[f"px{s + 1}"]).max() / (move * (s + 1)),
                    pv=np.abs(pv - g[f"pv{s + 1}"]).max() / np.abs(g[f"pv{s + 1}"]).max(),
                    lphi=np.abs(N(sim.fluid_levelset.phi) - g[f"lphi{s + 1}"]).max() / float(g["gdx"]),
                    gvy=np.abs(N(sim.grid.y.v) - gvy).max() / np.abs(gvy).max())
        print(f"STEP {s + 1}: deviation / scale {devs} (bounds 1e-4, 2e-3, 1e-4, 5e-3); iterations "
              f"{sim.DensitySolver.iterations} {sim.ViscositySolver.iterations} {sim.PressureSolver.iterations}")
        # positions: the step moves particles by `move`; agreement to 1e-4 of that
        np.testing.assert_allclose(px, g[f"px{s + 1}"], rtol=0, atol=1e-4 * move * (s + 1))
        np.testing.assert_allclose(pv, g[f"pv{s + 1}"], rtol=0, atol=2e-3 * np.abs(g[f"pv{s + 1}"]).max())
        np.testing.assert_allclose(N(sim.fluid_levelset.phi), g[f"lphi{s + 1}"], rtol=0, atol=1e-4 * float(g["gdx"]))
        np.testing.assert_allclose(N(sim.grid.y.v), gvy, rtol=0, atol=5e-3 * np.abs(gvy).max())
    assert sim.iterations == 3 and set(timings) >= {"solid", "density", "viscosity", "pressure", "p2g", "g2p"}
    np.testing.assert_allclose(N(rb_d[2, 1:4, 3]), np.array([-0.1, 0.5, 0.0]) + g["ball_v"] * g["dts"].sum(), rtol=0, atol=1e-12)


def test_a_translating_and_rotating_sphere_leaves_no_stale_state():
    g = golden(NAME)
    omega = np.array([0.0, 3.0, -1.5])
    sim, rb_d = build(g, omega=omega)
    before = rb_d.clone()
    dts = [sim.step() for _ in range(3)]
    sl, ds, p = sim.solid_levelset, sim.DensitySolver, sim.particle
    assert all(bool(torch.isfinite(t).all()) for t in (p.x, p.v, sim.grid.x.v, sim.grid.y.v, sim.grid.z.v, sl.phi, sl.v))
    assert sim.rb_d is rb_d and torch.equal(rb_d[:2], before[:2]) and not torch.equal(rb_d[2], before[2])
    np.testing.assert_allclose(N(rb_d[2, 1:4, 3]), np.array([-0.1, 0.5, 0.0]) + g["ball_v"] * sum(dts), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(N(rb_d[2, 9, :3]), g["ball_v"])
    np.testing.assert_allclose(N(rb_d[2, 5:9]), sdf.get_R(list(omega), np.degrees(np.linalg.norm(omega) * sum(dts))), rtol=0, atol=1e-14)
    np.testing.assert_array_equal(N(sim.kinematics.rb_w), [[0, 0, 0], [0, 0, 0], list(omega)])
    phi, v = torch.full_like(sl.phi, float("nan")), torch.full_like(sl.v, float("nan"))
    sdf.evaluate_grid(rb_d, phi, v, sl.bound_min, sl.cell_size, sl.bias, rb_w=sim.kinematics.rb_w)
    assert torch.equal(sl.phi, phi) and torch.equal(sl.v, v)
    # the rotation is in sv: inside the sphere the y component is w x r alone (the sphere's own v_y is 0)
    ball = torch.as_tensor(N(phi) <= 0, device=DEV) & (v[..., 0] != 0)
    assert bool(ball.any()) and bool((v[..., 1][ball] != 0).any())
    w = [torch.zeros_like(t) for t in (ds.wx, ds.wy, ds.wz)]
    compute_solid_frac(sim.GRES, phi, *w)
    assert torch.equal(ds.wx, w[0]) and torch.equal(ds.wy, w[1]) and torch.equal(ds.wz, w[2])
