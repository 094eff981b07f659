"""Triangle-mesh bodies in the 3D time step (NotebookSimulation(..., mesh_bodies=[...])) on the MI355X: the scene of
tests/test_timestep_gpu.py (12 x 16 x 12, golden step_a_12x16x12 for the particles) plus a box mesh of side 0.1 that the fluid
block runs into.  The solid level set and the projection are compared with the numpy restatement
(tests/meshsdf_numpy.py) on the body's own float32 volume; bounds as in tests/test_mesh_solids_gpu.py.
Where particles end up is asserted at the projection inside the step (the density solve moves them again before the step
ends, so no bound on the end-of-step depth follows from the projection), per particle, by the bound of
meshsdf_numpy.straight_move_interval, which does not use the restatement of the projection."""
import numpy as np
import pytest
import torch

import meshsdf_numpy as M
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
TOL64 = 64 * float(np.finfo(np.float64).eps) * 2.0
CENTER, AXIS, ANGLE = (-0.1435, 0.45, 0.0), (0, 0, 1), 20       # 0.8 mm from the block, which moves at -0.5 along x


def scene(g):
    import solver.sdf3D as sdf
    gres, gdx = tuple(int(v) for v in g["gres"]), float(g["gdx"])
    size = np.array(gres) * gdx
    rb_d, rb_map = sdf.generate_rb(None, {}, 'cube', ['box', size[0] - 2 * gdx, size[1] - 2 * gdx, size[2] - 2 * gdx], flip=True,
                                   center=[0, size[1] / 2, 0], axis=[0., 1, 0], angle=0, device=DEV)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.05, 0.8], flip=False, center=[-0.12, 0.2, 0],
                                   axis=[0., 0, 1], angle=-35)
    return gres, gdx, rb_d


@pytest.fixture(scope="module")
def box_sdf():
    from mfs import meshsdf
    from mfs.surface import Mesh
    v, f = M.box((0.1, 0.1, 0.1))
    return meshsdf.build(Mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV)), 0.0125)


def simulation(g, mesh_bodies, cls=None, pv=None, **kw):
    import notebook_sim as NSIM
    gres, gdx, rb_d = scene(g)
    sim = (cls or NSIM.NotebookSimulation)(gres, gdx, [-0.3, 0, -0.3], rb_d, g["px0"], float(g["pdx"]), rho=float(g["rho"]),
                                           mu=float(g["mu"]), dt=float(g["dt"]), device=DEV, mesh_bodies=mesh_bodies, **kw)
    sim.particle.v.copy_(torch.as_tensor(g["pv0"] if pv is None else pv, device=DEV))
    return sim


def restated_level_set(sim, plain, rb_w=None):
    """min(analytic table, mesh bodies) and its velocity from the state of `plain`, a simulation without mesh bodies"""
    import solver.sdf3D as sdf
    vols = [(N(b.sdf.phi), b.sdf.origin, b.sdf.spacing) for b in sim.mesh_bodies]
    sl = plain.solid_levelset
    if rb_w is not None:                      # a moving body: the step rebuilt the analytic part with evaluate_grid
        sdf.evaluate_grid(plain.rb_d, sl.phi, sl.v, sl.bound_min, sl.cell_size, sl.bias)
    return M.union(N(sim.mesh_rb), vols, N(sl.phi), N(sl.v), N(sim.solid_levelset.pos), rb_w)


def test_a_static_box_mesh_in_the_pool(box_sdf, monkeypatch):
    import solver.sdf3D as sdf
    g = golden("step_a_12x16x12")
    body = sdf.MeshBody(box_sdf, center=CENTER, axis=AXIS, angle=ANGLE)
    fast = 8 * g["pv0"]                        # the block runs into the body at 4 m/s: a few particles enter it in a step
    sim, plain = simulation(g, [body], pv=fast), simulation(g, None)
    assert plain.mesh_bodies is None and sim.mesh_kinematics is None and sim.kinematics is None
    ref_phi, ref_v, winner = restated_level_set(sim, plain)
    assert ((winner == 0) & (ref_phi < 0)).sum() > 20
    np.testing.assert_allclose(N(sim.solid_levelset.phi), ref_phi, rtol=0, atol=TOL64)
    np.testing.assert_allclose(N(sim.solid_levelset.v), ref_v, rtol=0, atol=TOL64)
    vol, row = (N(box_sdf.phi), box_sdf.origin, box_sdf.spacing), N(sim.mesh_rb)[0]
    sample = lambda x: M.sample(*vol, M.to_body(row, x))  # noqa: E731

    calls, real_project, real_mesh = [], sdf.project, sdf.project_mesh

    def project(rb_d, x):
        calls.append("project")
        real_project(rb_d, x)

    def project_mesh(rb, bodies, x):
        before = N(x).copy()
        real_mesh(rb, bodies, x)
        calls.append(("project_mesh", before, N(x).copy()))
    monkeypatch.setattr(sdf, "project", project)
    monkeypatch.setattr(sdf, "project_mesh", project_mesh)
    n, pushed = sim.particle.num_particles, 0
    assert sample(N(sim.particle.x)).min() > 0                                      # every particle starts outside the body
    for s in range(3):
        del calls[:]
        dt = sim.step()
        assert [c if isinstance(c, str) else c[0] for c in calls] == ["project", "project_mesh"]   # right after sdf.project
        _, before, after = calls[1]
        ref, moved = M.project(row[None], [vol], before)
        np.testing.assert_allclose(after, ref, rtol=0, atol=TOL64)
        d0, d1 = sample(before), sample(after)
        assert (moved == (d0 < 0)).all() and (after[~moved] == before[~moved]).all()
        # Where the projection leaves a particle, without the restatement: it moved by |d0| (checked), and along that
        # straight move the sampled field changes by |d0| times an average of grad f . u, which the volume's own edge
        # differences bound (meshsdf_numpy.straight_move_interval).  So no particle ends deeper than -tol_i = d0 + lo_i:
        # a few float64 roundings where the field is linear (the faces), a fraction of |d0| next to an edge.
        if moved.any():
            b0, b1 = M.to_body(row, before[moved]), M.to_body(row, after[moved])
            np.testing.assert_allclose(np.linalg.norm(b1 - b0, axis=1), -d0[moved], rtol=0, atol=TOL64)
            lo, hi, _ = M.straight_move_interval(vol[0], np.asarray(vol[1]), vol[2], b0, b1)
            print(f"step {s + 1}: dt {dt:.5f}, {int(moved.sum())} particles pushed out, d before {d0[moved]}, after {d1[moved]}, "
                  f"bounds {d0[moved] + lo} .. {d0[moved] + hi}")
            assert (d1[moved] >= d0[moved] + lo - TOL64).all() and (d1[moved] <= d0[moved] + hi + TOL64).all()
            assert (np.abs(d1[moved]) < np.abs(d0[moved])).all()
        pushed += int(moved.sum())
        x = N(sim.particle.x)
        assert sim.particle.num_particles == n and x.shape == (n, 3)
        assert all(bool(torch.isfinite(t).all()) for t in (sim.particle.x, sim.particle.v, sim.grid.x.v, sim.grid.y.v, sim.grid.z.v))
        np.testing.assert_allclose(N(sim.solid_levelset.phi), ref_phi, rtol=0, atol=TOL64)         # static: untouched
    assert pushed >= 3 and sim.iterations == 3


def test_a_moving_box_mesh(box_sdf):
    import solver.sdf3D as sdf
    from mfs.motion import Motion
    from scipy.spatial.transform import Rotation
    g = golden("step_a_12x16x12")
    v, w = np.array([0.2, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    body = sdf.MeshBody(box_sdf, center=CENTER, axis=AXIS, angle=ANGLE, motion=Motion(velocity=tuple(v), omega=tuple(w)))
    sim, plain = simulation(g, [body]), simulation(g, None)
    assert sim.kinematics is None and sim.mesh_kinematics is not None
    speed = np.linalg.norm(v) + np.linalg.norm(w) * box_sdf.radius
    assert sim.mesh_kinematics.max_surface_speed(0.0) == pytest.approx(speed, rel=1e-14)
    assert box_sdf.radius == pytest.approx(0.05 * np.sqrt(3), rel=1e-6)
    dts = []
    for _ in range(3):
        dts.append(sim.step())
        assert dts[-1] <= sim.GDX / speed
    total = sum(dts)
    row = N(sim.mesh_rb)[0]
    np.testing.assert_allclose(row[1:4, 3], np.asarray(CENTER) + v * total, rtol=0, atol=1e-14)
    R = (Rotation.from_rotvec(w * total) * Rotation.from_matrix(sdf.get_R(list(AXIS), ANGLE)[:3, :3])).as_matrix()
    np.testing.assert_allclose(row[5:8, :3], R, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(row[9, :3], v)
    assert row[0, 0] == 6 and row[0, 1] == box_sdf.radius
    # the level set was rebuilt (no analytic body moves): analytic table, then the mesh at its pose, with w x (x - T)
    ref_phi, ref_v, winner = restated_level_set(sim, plain, rb_w=w[None])
    inside = (winner == 0) & (ref_phi < 0)
    assert inside.sum() > 20
    np.testing.assert_allclose(N(sim.solid_levelset.phi), ref_phi, rtol=0, atol=TOL64)
    np.testing.assert_allclose(N(sim.solid_levelset.v), ref_v, rtol=0, atol=TOL64)
    x = N(sim.solid_levelset.pos)[inside] - row[1:4, 3]
    np.testing.assert_allclose(N(sim.solid_levelset.v)[inside], v + np.cross(w, x), rtol=0, atol=TOL64)
    assert all(bool(torch.isfinite(t).all()) for t in (sim.particle.x, sim.particle.v))


def test_the_surface_speed_clamp_sets_dt(box_sdf):
    """a body fast enough that GDX / max_surface_speed is the smallest of the step's limits: the step takes exactly that"""
    import solver.sdf3D as sdf
    from mfs.motion import Motion
    g = golden("step_a_12x16x12")
    body = sdf.MeshBody(box_sdf, center=(0.2, 0.65, 0.1), motion=Motion(velocity=(0.0, 0.0, -25.0), omega=(0, 0, 2.0)))
    sim = simulation(g, [body], pv=np.zeros_like(g["pv0"]))
    dt = sim.step()
    assert dt == sim.GDX / (25.0 + 2.0 * box_sdf.radius) and dt < sim.DT
    np.testing.assert_allclose(N(sim.mesh_rb)[0, 1:4, 3], [0.2, 0.65, 0.1 - 25.0 * dt], rtol=0, atol=1e-14)


def test_mesh_bodies_are_single_gpu_and_3d(box_sdf):
    import notebook_sim as NSIM
    import notebook_sim2d as NSIM2
    import solver.sdf3D as sdf
    g = golden("step_a_12x16x12")
    body = sdf.MeshBody(box_sdf, center=CENTER)
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        with pytest.raises(NotImplementedError, match="mesh"):
            simulation(g, [body], cls=cls, dist=None)
    with pytest.raises(NotImplementedError, match="mesh"):
        NSIM2.NotebookSimulation2D((8, 8), 0.1, [0, 0], None, np.zeros((1, 2)), 0.05, device=DEV, mesh_bodies=[body])
