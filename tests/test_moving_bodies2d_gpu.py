"""Moving rigid bodies in the 2D time step (NotebookSimulation2D(..., motion=...)) on the MI355X: the 24 x 32 dam break of
tests/timestep2d_scene.py with a piston at the water column's free side moving at v = (0.3, 0) and a paddle in the water
turning at 2 rad/s -- both slower than the collapsing column, so the step's move scale is the static scene's.

Reference: the numpy time step (tests/notebook2d_numpy.py `step`) composed with the moving bodies here -- before each
`R.step(ref)` a numpy copy of the poses is advanced by the dt that step will take and `ref.rb_d`, `ref.sphi`, `ref.sv` are
recomputed (tests/test_sdf_grid_gpu.py's restatement: winner from the per-body distances, v + w x r).  The restatement
advects, then projects at `ref.rb_d`: with the pose already advanced that is the driver's order.
Bounds: those of tests/test_timestep2d_gpu.py::test_two_full_steps."""
import numpy as np
import pytest
import torch

import density2d_numpy as D2
import notebook2d_numpy as R
import notebook_sim2d as NSIM
import solver.sdf2D as sdf
from mfs import scenes
from mfs.motion import Motion
from solver.SolidFraction2D import compute_solid_frac
from test_sdf_grid_gpu import restated
from timestep2d_scene import dam_break

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
STAGES = {"advect+project", "levelset+volume", "density", "p2g", "viscosity", "pressure", "extrapolate+bc", "g2p"}
V_PISTON, W_PADDLE = (0.3, 0.0), 2.0


def moving_dam_break():
    """the dam break plus body 2, the piston (overlaps the column's free side, x = 0.225, by a cell's half), and body 3, the paddle"""
    sc = dam_break((24, 32))
    sc["bodies"] = sc["bodies"] + [
        dict(name="piston", rbparam=["box", 0.1, 0.5], flip=False, center=[0.25, 1.0], angle=0),
        dict(name="paddle", rbparam=["box", 0.2, 0.04], flip=False, center=[0.0, 0.95], angle=0)]
    sc["rb_d"] = np.stack([scenes._rb2(b["rbparam"][0], b["rbparam"][1:], b["flip"], b["center"], b["angle"]) for b in sc["bodies"]])
    sc["motion"] = {2: dict(velocity=V_PISTON, omega=0.0), 3: dict(velocity=(0.0, 0.0), omega=W_PADDLE)}
    return sc


def build(sc, moving=True):
    rb_d, rb_map = None, {}
    for b in sc["bodies"]:
        rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, b["name"], b["rbparam"], flip=b["flip"], center=b["center"], angle=b["angle"],
                                       device=DEV)
    motion = {i: Motion(**m) for i, m in sc["motion"].items()} if moving else None
    sim = NSIM.NotebookSimulation2D(sc["gres"], sc["gdx"], sc["bound_min"], rb_d, sc["px"], sc["pdx"], mu=sc["mu"], device=DEV,
                                    motion=motion)
    sim.particle.v.copy_(torch.as_tensor(sc["pv"], device=DEV))
    return sim, rb_d


class NumpyBodies:
    """the moving bodies' poses in numpy (centre and angle), written into the restatement's state before each step"""

    def __init__(self, sc):
        self.motion = sc["motion"]
        self.T = {i: sc["rb_d"][i, 1:3, 2].copy() for i in self.motion}
        self.angle = {i: float(np.arctan2(sc["rb_d"][i, 5, 0], sc["rb_d"][i, 4, 0])) for i in self.motion}
        self.rho = {i: float(np.linalg.norm(sc["rb_d"][i, 0, 1:])) for i in self.motion}
        self.bound = max(np.hypot(*m["velocity"]) + abs(m["omega"]) * self.rho[i] for i, m in self.motion.items())

    def step(self, ref):
        """advance by the dt `R.step(ref, duration_left=...)` is about to take; returns that duration_left"""
        left = ref.gdx / max(1e-10, self.bound)
        vmax = np.sqrt((ref.pv ** 2).sum(axis=-1)).max()
        dt = min(ref.DT, ref.gdx / max(1e-10, float(vmax)), left)
        rb = ref.rb_d = ref.rb_d.copy()
        rb_w = np.zeros(len(rb))
        for i, m in self.motion.items():
            self.T[i] = self.T[i] + np.asarray(m["velocity"]) * dt
            self.angle[i] += m["omega"] * dt
            c, s = np.cos(self.angle[i]), np.sin(self.angle[i])
            rb[i, 1:3, 2], rb[i, 4:6, :2], rb[i, 7, :2], rb_w[i] = self.T[i], ((c, -s), (s, c)), m["velocity"], m["omega"]
        sphi = D2.sdf_evaluate(rb, ref.pos)[0]
        sv, skipped, best = restated(2, rb, rb_w, ref.pos, sphi.reshape(-1) <= 0)
        assert not skipped.any() and np.array_equal(best, sphi.reshape(-1))
        ref.sphi, ref.sv = sphi, sv.reshape(ref.pos.shape)
        return left


def make_ref(sc):
    ref = R.make_state(sc["gres"], sc["gdx"], sc["bound_min"], sc["rb_d"], sc["px"], sc["pdx"], mu=sc["mu"])
    ref.pv[...] = sc["pv"]
    return ref


def test_two_full_steps_with_moving_bodies():
    sc = moving_dam_break()
    sim, _ = build(sc)
    ref, nb = make_ref(sc), NumpyBodies(sc)
    assert (D2.sdf_evaluate(sc["rb_d"][2:3], sc["px"])[0] < 0).sum() >= 10          # the piston overlaps the column
    assert (D2.sdf_evaluate(sc["rb_d"][3:4], sc["px"])[0] < 0).sum() >= 10          # the paddle is in the water
    assert nb.bound < np.sqrt((sc["pv"] ** 2).sum(axis=-1)).max()                   # both slower than the column
    timings = {}
    for s in range(2):
        dt = sim.step(timings=timings)
        left = nb.step(ref)
        assert dt == pytest.approx(R.step(ref, duration_left=left), rel=1e-12)
        np.testing.assert_allclose(N(sim.rb_d), ref.rb_d, rtol=0, atol=1e-15)
        np.testing.assert_allclose(N(sim.solid_levelset.phi), ref.sphi, rtol=1e-13, atol=1e-15)
        assert (ref.sv[ref.sphi <= 0] != 0).any()
        px, pv = N(sim.particle.x), N(sim.particle.v)
        move = np.abs(ref.px - sc["px"]).max()
        devs = dict(px=np.abs(px - ref.px).max() / (move * (s + 1)), pv=np.abs(pv - ref.pv).max() / np.abs(ref.pv).max(),
                    lphi=np.abs(N(sim.fluid_levelset.phi) - ref.lphi).max() / sc["gdx"],
                    gvy=np.abs(N(sim.grid.y.v) - ref.gv[1]).max() / np.abs(ref.gv[1]).max())
        print(f"STEP {s + 1}: deviation / scale {devs} (bounds 1e-4, 2e-3, 1e-4, 5e-3); iterations GPU "
              f"{sim.DensitySolver.iterations} {sim.ViscositySolver.iterations} {sim.PressureSolver.iterations} numpy {ref.iters}")
        np.testing.assert_allclose(px, ref.px, rtol=0, atol=1e-4 * move * (s + 1))
        np.testing.assert_allclose(pv, ref.pv, rtol=0, atol=2e-3 * np.abs(ref.pv).max())
        np.testing.assert_allclose(N(sim.fluid_levelset.phi), ref.lphi, rtol=0, atol=1e-4 * sc["gdx"])
        np.testing.assert_allclose(N(sim.grid.y.v), ref.gv[1], rtol=0, atol=5e-3 * np.abs(ref.gv[1]).max())
    assert sim.iterations == 2 and set(timings) >= STAGES | {"solid"}


def test_no_stale_state_after_five_steps():
    sc = moving_dam_break()
    sim, rb_d = build(sc)
    c0 = N(rb_d[2, 1:3, 2]).copy()
    before = rb_d.clone()
    dts = [sim.step() for _ in range(5)]
    sl, ds = sim.solid_levelset, sim.DensitySolver
    assert sim.rb_d is rb_d and not torch.equal(rb_d, before)                        # the caller's tensor is the one updated
    assert torch.equal(rb_d[:2], before[:2]) and torch.equal(rb_d[:, 0], before[:, 0])
    np.testing.assert_allclose(N(rb_d[2, 1:3, 2]), c0 + np.asarray(V_PISTON) * sum(dts), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(N(rb_d[2, 7, :2]), V_PISTON)
    np.testing.assert_array_equal(N(sim.kinematics.rb_w), [0.0, 0.0, 0.0, W_PADDLE])
    c, s = np.cos(W_PADDLE * sum(dts)), np.sin(W_PADDLE * sum(dts))
    np.testing.assert_allclose(N(rb_d[3, 4:6, :2]), ((c, -s), (s, c)), rtol=0, atol=1e-14)
    phi, v = torch.full_like(sl.phi, float("nan")), torch.full_like(sl.v, float("nan"))
    sdf.evaluate_grid(rb_d, phi, v, sl.bound_min, sl.cell_size, sl.bias, rb_w=sim.kinematics.rb_w)
    assert torch.equal(sl.phi, phi) and torch.equal(sl.v, v)
    assert bool((v[..., 1][phi <= 0] != 0).any())                                    # the paddle's rotation is in sv
    wx, wy = torch.zeros_like(ds.wx), torch.zeros_like(ds.wy)
    compute_solid_frac(sim.GRES, phi, wx, wy)
    assert torch.equal(ds.wx, wx) and torch.equal(ds.wy, wy)
    assert sim.current_time == pytest.approx(sum(dts), rel=1e-14)


POOL_FACE = 0.53


def pool_scene():
    """a still pool (a lattice of particles, jitter 2 % of the spacing) between a piston and the tank's right wall, on the
    floor.  The tank's walls are 1.5 cells thick here: with the dam break's walls ON the cell faces the wall nodes' level
    set is exactly 0, the faces count as open and a pool at rest drains into the wall cells (the column of the dam break
    never rests on anything long enough to show it) -- which would bury the piston's effect in the still pool's own motion."""
    sc = dam_break((24, 32))
    gdx, pdx = sc["gdx"], sc["pdx"]
    bmin, size = np.asarray(sc["bound_min"]), np.array([24, 32]) * gdx
    lo = np.array([POOL_FACE, bmin[1] + 1.5 * gdx])
    hi = np.array([bmin[0] + size[0] - 1.5 * gdx, lo[1] + 0.3])
    dims = np.round((hi - lo) / pdx).astype(np.int64)
    ii, jj = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), indexing="ij")
    pos = lo + (np.stack([ii, jj], axis=-1).reshape(-1, 2) + 0.5) * ((hi - lo) / dims)
    sc["px"] = pos + np.random.default_rng(7).standard_normal(pos.shape) * pdx * 0.02
    sc["pv"] = np.zeros_like(sc["px"])
    ctr = bmin + 0.5 * size
    sc["bodies"] = [dict(name="tank", rbparam=["box", float(size[0] - 3 * gdx), float(size[1] - 3 * gdx)], flip=True,
                         center=[float(ctr[0]), float(ctr[1])], angle=0),
                    dict(name="piston", rbparam=["box", 0.2, 0.6], flip=False, center=[POOL_FACE - 0.1, 0.35], angle=0)]
    sc["rb_d"] = np.stack([scenes._rb2(b["rbparam"][0], b["rbparam"][1:], b["flip"], b["center"], b["angle"]) for b in sc["bodies"]])
    sc["motion"] = {1: dict(velocity=V_PISTON, omega=0.0)}
    return sc


def test_a_piston_pushes_a_still_pool():
    sc = pool_scene()
    sim, rb_d = build(sc)
    still, _ = build(sc, moving=False)
    timings, timings_still = {}, {}
    for _ in range(15):
        sim.step(timings=timings)
        still.step(timings=timings_still)
    assert "solid" in timings and "solid" not in timings_still and set(timings_still) == STAGES
    px, pv = N(sim.particle.x), N(sim.particle.v)
    lo = sim.BOUND_MIN.astype(np.float64)
    hi = lo + sim.BOUND_SIZE.astype(np.float64)
    assert np.isfinite(px).all() and np.isfinite(pv).all() and (px > lo).all() and (px < hi).all()
    # `project` runs before the density solve displaces the particles: a step may end with particles a fraction of a cell
    # inside the piston (the next projection puts them back), never a cell deep
    sd = D2.sdf_evaluate(N(rb_d)[1:2], px)[0]
    assert sd.min() >= -sc["gdx"], sd.min()
    assert N(rb_d)[1, 1, 2] == pytest.approx(POOL_FACE - 0.1 + V_PISTON[0] * sim.current_time, abs=1e-12)
    mean, mean_still = pv[:, 0].mean(), N(still.particle.v)[:, 0].mean()
    print(f"mean v_x: piston {mean:.4e}, at rest {mean_still:.4e}; min sd to the piston {sd.min():.3e}")
    assert mean > 0 and abs(mean_still) < 0.1 * mean
