"""notebook_sim.seed_particles on the MI355X: the scene of tests/test_mesh_timestep_gpu.py (12 x 16 x 12: a pool with a
ramp, plus a box mesh as a solid) with the liquid seeded from a sphere mesh that overlaps the box mesh, checked against
tests/seed_numpy.py on the solid level set the GPU built, then stepped."""
import numpy as np
import pytest
import torch

import meshsdf_numpy as M
import seed_numpy as S
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
BOUND_MIN = [-0.3, 0, -0.3]
CENTER, AXIS, ANGLE = (-0.1435, 0.45, 0.0), (0, 0, 1), 20       # the box mesh of tests/test_mesh_timestep_gpu.py
LIQUID = dict(center=(-0.02, 0.5, 0.0), axis=(1, 2, 0.5), angle=33)     # a sphere of radius 0.12 above the ramp


def scene(g):
    import solver.sdf3D as sdf
    gres, gdx = tuple(int(v) for v in g["gres"]), float(g["gdx"])
    size = np.array(gres) * gdx
    rb_d, rb_map = sdf.generate_rb(None, {}, 'cube', ['box', size[0] - 2 * gdx, size[1] - 2 * gdx, size[2] - 2 * gdx], flip=True,
                                   center=[0, size[1] / 2, 0], axis=[0., 1, 0], angle=0, device=DEV)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.05, 0.8], flip=False, center=[-0.12, 0.2, 0],
                                   axis=[0., 0, 1], angle=-35)
    return gres, gdx, rb_d


def build(v, f, spacing):
    from mfs import meshsdf
    from mfs.surface import Mesh
    return meshsdf.build(Mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV)), spacing)


@pytest.fixture(scope="module")
def setup():
    import notebook_sim as NSIM
    import solver.sdf3D as sdf
    from mfs import seed
    g = golden("step_a_12x16x12")
    gres, gdx, rb_d = scene(g)
    body = sdf.MeshBody(build(*M.box((0.1, 0.1, 0.1)), 0.0125), center=CENTER, axis=AXIS, angle=ANGLE)
    liquid = seed.Shape(build(*M.icosphere(2, 0.12), 0.0125), **LIQUID)
    px = NSIM.seed_particles(gres, gdx, BOUND_MIN, liquid, rb_d=rb_d, mesh_bodies=[body], seed=17, device=DEV)
    solid = NSIM.solid_volume(gres, gdx, BOUND_MIN, rb_d, [body], DEV)
    return g, gres, gdx, rb_d, body, liquid, px, solid


def oracle(setup, clearance=0.0, seed=17):
    g, gres, gdx, rb_d, body, liquid, px, solid = setup
    inc = S.shape_of(N(liquid.volume.phi), liquid.volume.origin, liquid.volume.spacing, (liquid.R, liquid.T))
    exc = S.shape_of(N(solid.phi), solid.origin, solid.spacing)
    return inc, exc, S.fill([inc], tuple(2 * v for v in gres), solid.origin, solid.spacing, [exc], clearance, 1.0, seed)


def test_the_solid_volume_is_the_constructors_level_set(setup):
    import notebook_sim as NSIM
    g, gres, gdx, rb_d, body, liquid, px, solid = setup
    sim = NSIM.NotebookSimulation(gres, gdx, BOUND_MIN, rb_d, px, gdx / 2, device=DEV, mesh_bodies=[body])
    assert tuple(solid.phi.shape) == tuple(sim.solid_levelset.phi.shape) == tuple(2 * v + 1 for v in gres)
    np.testing.assert_allclose(N(solid.phi), N(sim.solid_levelset.phi), rtol=0, atol=64 * S.EPS64 * 2.0)
    assert solid.origin == tuple(float(np.float64(np.float32(v))) for v in BOUND_MIN) and solid.spacing == gdx / 2
    assert int((N(solid.phi) < 0).sum()) > 1000 and float(N(solid.phi).min()) < -0.04       # walls, ramp and box mesh


def test_seeded_particles_avoid_the_solids_and_match_the_oracle(setup):
    g, gres, gdx, rb_d, body, liquid, px, solid = setup
    inc, exc, (ref_px, ref_sites, band) = oracle(setup)
    assert band == 0
    x = N(px)
    assert px.dtype == torch.float64 and px.is_cuda and x.shape == (len(ref_sites), 3) and len(x) > 200      # P
    assert x.tobytes() == ref_px.tobytes()
    d = S.sample(exc[0], exc[1], exc[2], x)
    assert (d > 0).all()                                                  # every particle is outside every solid
    lo = np.asarray(BOUND_MIN, np.float64)
    assert (x >= lo).all() and (x <= lo + np.asarray(gres) * gdx).all()
    # the box mesh did trim the sphere: without solids there are more particles, and the extra ones are in the box mesh, up to
    # what interpolating its 1-Lipschitz distance on cells of gdx / 2 can differ from it (a cell's diagonal)
    sites = tuple(2 * v for v in gres)
    extra = np.setdiff1d(S.fill([inc], sites, solid.origin, solid.spacing, seed=17)[1], ref_sites)
    vol, row = (N(body.sdf.phi), body.sdf.origin, body.sdf.spacing), body.row[0]
    d = M.sample(*vol, M.to_body(row, S.positions(sites, solid.origin, solid.spacing, 1.0, 17, extra)))
    assert len(extra) > 10 and (d <= np.sqrt(3) * gdx / 2).all() and d.min() < -0.02


def test_a_clearance_keeps_the_liquid_off_the_solids(setup):
    import notebook_sim as NSIM
    g, gres, gdx, rb_d, body, liquid, px, solid = setup
    inc, exc, (ref_px, ref_sites, band) = oracle(setup, clearance=0.02, seed=17)
    assert band == 0
    got = NSIM.seed_particles(gres, gdx, BOUND_MIN, [liquid], rb_d=rb_d, mesh_bodies=[body], clearance=0.02, seed=17, device=DEV)
    assert N(got).tobytes() == ref_px.tobytes() and 0 < len(ref_px) < px.shape[0]
    assert (S.sample(exc[0], exc[1], exc[2], N(got)) > 0.02).all()


def test_the_simulation_takes_the_particles_and_steps(setup):
    import notebook_sim as NSIM
    g, gres, gdx, rb_d, body, liquid, px, solid = setup
    sim = NSIM.NotebookSimulation(gres, gdx, BOUND_MIN, rb_d, px, gdx / 2, rho=float(g["rho"]), mu=float(g["mu"]),
                                  dt=float(g["dt"]), device=DEV, mesh_bodies=[body])
    n = px.shape[0]
    assert sim.particle.num_particles == n and sim.PDX == gdx / 2
    for _ in range(2):
        sim.step()
        assert sim.particle.num_particles == n and tuple(sim.particle.x.shape) == (n, 3)
        assert all(bool(torch.isfinite(t).all()) for t in (sim.particle.x, sim.particle.v, sim.grid.x.v, sim.grid.y.v, sim.grid.z.v))
    assert sim.iterations == 2 and float(sim.particle.v[:, 1].mean()) < 0            # it falls
