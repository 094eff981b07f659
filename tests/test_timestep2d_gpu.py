"""Whole 2D time steps (notebook_sim2d.NotebookSimulation2D) on the MI355X against the numpy time step
(tests/notebook2d_numpy.py `step`: the kernels' restatement composed with the oracle's 2D pressure solve,
tests/visc2d_numpy.py and tests/density2d_numpy.py) on the dam break of tests/timestep2d_scene.py at 24 x 32.

Tolerances of the step: those of tests/test_timestep_gpu.py::test_two_full_steps -- the step is the same composition of
three CG solves stopped at the solvers' own absolute tolerances, whose iterates are chaotic in rounding, so the state after
a step agrees to solver-tolerance level: positions 1e-4 of the move per step, particle velocities 2e-3 of their maximum,
level set 1e-4 gdx, grid.y.v 5e-3 of its maximum; dt to rel 1e-12."""
import numpy as np
import pytest
import torch

import notebook2d_numpy as R
import notebook_sim2d as NSIM
import solver.sdf2D as sdf
from timestep2d_scene import dam_break

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
STAGES = {"advect+project", "levelset+volume", "density", "p2g", "viscosity", "pressure", "extrapolate+bc", "g2p"}


def build(sc):
    rb_d, rb_map = None, {}
    for b in sc["bodies"]:
        rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, b["name"], b["rbparam"], flip=b["flip"], center=b["center"], angle=b["angle"],
                                       device=DEV)
    sim = NSIM.NotebookSimulation2D(sc["gres"], sc["gdx"], sc["bound_min"], rb_d, sc["px"], sc["pdx"], mu=sc["mu"], device=DEV)
    sim.particle.v.copy_(torch.as_tensor(sc["pv"], device=DEV))
    return sim


@pytest.fixture(scope="module")
def scene():
    sc = dam_break((24, 32))
    ref = R.make_state(sc["gres"], sc["gdx"], sc["bound_min"], sc["rb_d"], sc["px"], sc["pdx"], mu=sc["mu"])
    ref.pv[...] = sc["pv"]
    return sc, ref


def test_setup_matches_the_restatement(scene):
    sc, ref = scene
    sim = build(sc)
    np.testing.assert_allclose(N(sim.rb_d), sc["rb_d"], rtol=0, atol=1e-16)
    np.testing.assert_allclose(N(sim.solid_levelset.pos), ref.pos, rtol=0, atol=0)
    np.testing.assert_allclose(N(sim.solid_levelset.phi), ref.sphi, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(N(sim.solid_levelset.v), ref.sv)
    p, g = sim.particle, sim.grid
    cells = np.unique(np.floor((sc["px"] - np.asarray(sc["bound_min"])) / sc["gdx"]).astype(np.int64), axis=0)
    assert 3.0 <= p.num_particles / len(cells) <= 4.5                              # about 4 particles per liquid cell
    np.testing.assert_array_equal(N(p.x), ref.px)
    np.testing.assert_array_equal(N(p.m), ref.pm)
    assert p.vol == ref.pvol and p.cx.shape == p.cy.shape == p.v.shape == (p.num_particles, 2)
    assert sim.BOUND_MIN.dtype == sim.BOUND_SIZE.dtype == np.float32 and g.cell_size.dtype == np.float64
    np.testing.assert_array_equal(g.cell_size, ref.cell_size)
    np.testing.assert_array_equal(sim.solid_levelset.cell_size, ref.dcell_size)
    assert tuple(g.x.bias) == (0, .5) and tuple(g.y.bias) == (.5, 0) and g.x.bias.dtype == np.float32
    for c, shape in ((g.x, (25, 32)), (g.y, (24, 33))):
        assert all(tuple(t.shape) == shape and t.dtype == torch.float32 for t in (c.m, c.v, c.dv))
    assert tuple(sim.solid_levelset.phi.shape) == tuple(sim.fluid_volume.vol.shape) == (49, 65)
    assert tuple(sim.solid_levelset.v.shape) == (49, 65, 2) and sim.fluid_levelset.phi.dtype == torch.float64


def test_two_full_steps(scene):
    sc, ref0 = scene
    sim = build(sc)
    ref = R.make_state(sc["gres"], sc["gdx"], sc["bound_min"], sc["rb_d"], sc["px"], sc["pdx"], mu=sc["mu"])
    ref.pv[...] = sc["pv"]
    timings = {}
    for s in range(2):
        dt = sim.step(timings=timings)
        assert dt == pytest.approx(R.step(ref), rel=1e-12)
        px, pv = N(sim.particle.x), N(sim.particle.v)
        move = np.abs(ref.px - sc["px"]).max()
        devs = dict(px=np.abs(px - ref.px).max() / (move * (s + 1)), pv=np.abs(pv - ref.pv).max() / np.abs(ref.pv).max(),
                    lphi=np.abs(N(sim.fluid_levelset.phi) - ref.lphi).max() / sc["gdx"],
                    gvy=np.abs(N(sim.grid.y.v) - ref.gv[1]).max() / np.abs(ref.gv[1]).max())
        print(f"STEP {s + 1}: deviation / scale {devs} (bounds 1e-4, 2e-3, 1e-4, 5e-3); iterations GPU "
              f"{sim.DensitySolver.iterations} {sim.ViscositySolver.iterations} {sim.PressureSolver.iterations} numpy {ref.iters}")
        # positions: the step moves particles by `move`; agreement to 1e-4 of that
        np.testing.assert_allclose(px, ref.px, rtol=0, atol=1e-4 * move * (s + 1))
        np.testing.assert_allclose(pv, ref.pv, rtol=0, atol=2e-3 * np.abs(ref.pv).max())
        np.testing.assert_allclose(N(sim.fluid_levelset.phi), ref.lphi, rtol=0, atol=1e-4 * sc["gdx"])
        np.testing.assert_allclose(N(sim.grid.y.v), ref.gv[1], rtol=0, atol=5e-3 * np.abs(ref.gv[1]).max())
    assert sim.iterations == 2 and set(timings) >= STAGES
    assert sim.PressureSolver.iterations > 0 and sim.ViscositySolver.iterations > 0 and sim.DensitySolver.iterations > 0


def test_twenty_steps_stay_in_the_box(scene):
    """The box is the simulation domain [BOUND_MIN, BOUND_MIN + BOUND_SIZE], whose outermost cell layer is the container's
    wall.  Not the container's inner surface: as in the 3D step, `project` runs BEFORE the density solve displaces the
    particles, so a step may end with particles a fraction of a cell inside the wall (the next step's projection puts them
    back); what must never happen is a particle beyond the wall layer, where every index clamps."""
    sc, _ = scene
    sim = build(sc)
    assert (N(sim.particle.x) < sc["box"][0]).any()                                  # some start inside the wall: project acts
    for _ in range(20):
        sim.step()
    px, pv = N(sim.particle.x), N(sim.particle.v)
    lo = sim.BOUND_MIN.astype(np.float64)
    hi = lo + sim.BOUND_SIZE.astype(np.float64)
    assert np.isfinite(px).all() and np.isfinite(pv).all()
    assert (px > lo).all() and (px < hi).all()
    inner = px.copy()
    sdf.project(sim.rb_d, sim.particle.x)                                            # ... and the wall is within reach
    assert np.abs(N(sim.particle.x) - inner).max() < sc["gdx"]
    dcs = sim.fluid_volume.cell_size
    assert float(sim.fluid_volume.vol.abs().max()) <= dcs[0] * dcs[1]
    assert sim.iterations == 20 and sim.current_time == pytest.approx(20 / 300.0)
