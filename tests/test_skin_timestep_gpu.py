"""NotebookSimulation.skin() on the MI355X: the scene of tests/test_mesh_timestep_gpu.py (12 x 16 x 12, golden
step_a_12x16x12: a pool with a ramp, a block of liquid) after one step."""
import numpy as np
import pytest
import torch

import surface_numpy as SN
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731


@pytest.fixture(scope="module")
def sim():
    import notebook_sim as NSIM
    import solver.sdf3D as sdf
    g = golden("step_a_12x16x12")
    gres, gdx = tuple(int(v) for v in g["gres"]), float(g["gdx"])
    size = np.array(gres) * gdx
    rb_d, rb_map = sdf.generate_rb(None, {}, 'cube', ['box', size[0] - 2 * gdx, size[1] - 2 * gdx, size[2] - 2 * gdx], flip=True,
                                   center=[0, size[1] / 2, 0], axis=[0., 1, 0], angle=0, device=DEV)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.05, 0.8], flip=False, center=[-0.12, 0.2, 0],
                                   axis=[0., 0, 1], angle=-35)
    s = NSIM.NotebookSimulation(gres, gdx, [-0.3, 0, -0.3], rb_d, g["px0"], float(g["pdx"]), rho=float(g["rho"]),
                                mu=float(g["mu"]), dt=float(g["dt"]), device=DEV)
    s.particle.v.copy_(torch.as_tensor(g["pv0"], device=DEV))
    s.step()
    return s


def lattice(sim):
    return tuple(2 * v + 1 for v in sim.GRES), np.asarray(sim.BOUND_MIN, np.float64), 0.5 * sim.GDX


def test_the_skin_is_a_closed_manifold(sim):
    m = sim.skin(normals=True)
    V, F = N(m.vertices), N(m.faces)
    assert m.vertices.dtype == torch.float32 and m.faces.dtype == torch.int32 and m.normals.shape == m.vertices.shape
    assert len(V) > 500 and SN.is_closed_manifold(F, len(V)) and SN.all_vertices_used(V, F)
    assert SN.signed_volume(V.astype(np.float64), F) > 0
    shape, origin, h = lattice(sim)
    assert (V >= origin - 1e-6).all() and (V <= origin + (np.asarray(shape) - 1) * h + 1e-6).all()
    x = N(sim.particle.x)
    print(f"skin: {len(V)} vertices, {len(F)} faces, volume {SN.signed_volume(V.astype(np.float64), F):.5f} "
          f"({len(x)} particles x PDX^3 = {len(x) * sim.PDX ** 3:.5f})")


def test_unclipped_it_is_the_direct_call_on_the_particles(sim):
    from mfs import skin
    shape, origin, h = lattice(sim)
    a = sim.skin(clip=False, normals=True)
    b = skin.mesh(sim.particle.x, shape, origin, h, normals=True)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.normals, b.normals)
    f, g = sim.skin_field(clip=False), skin.field(sim.particle.x, shape, origin, h)
    assert torch.equal(f.phi, g.phi) and f[1:] == g[1:] and f.phi.dtype == torch.float32
    assert f.spacing == sim.GDX / 2 and f.radius == skin.default_radius(sim.GDX / 2) and f.influence == 3 * f.radius
    assert SN.is_closed_manifold(N(a.faces), a.vertices.shape[0])


def test_clipping_is_the_maximum_with_the_negated_solid_level_set(sim):
    from mfs import skin
    from mfs.surface import isosurface
    shape, origin, h = lattice(sim)
    raw = skin.field(sim.particle.x, shape, origin, h)
    ref = torch.maximum(raw.phi, -sim.solid_levelset.phi)
    f = sim.skin_field()
    assert tuple(f.phi.shape) == tuple(sim.solid_levelset.phi.shape) == shape
    assert torch.equal(f.phi, ref) and f[1:] == raw[1:]
    m, k = sim.skin(), isosurface(ref, 0.0, origin, h, closed=True, outside=raw.background)
    assert torch.equal(m.vertices, k.vertices) and torch.equal(m.faces, k.faces) and m.normals is None
    # other radii go through
    thin = sim.skin_field(radius=0.4 * sim.GDX, influence=1.1 * sim.GDX)
    assert (thin.radius, thin.influence) == (0.4 * sim.GDX, 1.1 * sim.GDX)
    assert torch.equal(thin.phi, torch.maximum(skin.field(sim.particle.x, shape, origin, h, 0.4 * sim.GDX, 1.1 * sim.GDX).phi,
                                               -sim.solid_levelset.phi))


def test_clipping_trims_the_rind_of_liquid_resting_on_a_solid(sim):
    """after one step the block is still in the air and nothing is trimmed; moved down until its lowest particle is half
    a node inside the pool's floor (the face of the container, one GDX above the bounds), its skin reaches the node plane
    below the floor, and the clip takes that away"""
    from mfs import skin
    shape, origin, h = lattice(sim)
    x = sim.particle.x
    saved = x.clone()
    try:
        x[:, 1] -= x[:, 1].min() - (sim.BOUND_MIN[1] + sim.GDX - 0.5 * h)
        raw, f = skin.field(x, shape, origin, h), sim.skin_field()
        solid = sim.solid_levelset.phi
        trimmed = (raw.phi < 0) & (f.phi >= 0)
        print(f"clip: {int(trimmed.sum())} of {int((raw.phi < 0).sum())} inside nodes trimmed")
        assert int(trimmed.sum()) > 50 and bool((solid[trimmed] <= 0).all()) and int((solid[trimmed] < -0.5 * h).sum()) > 30
        assert not bool(((f.phi < 0) & (solid < 0)).any())                # no liquid left inside the solid
        m = sim.skin()
        assert SN.is_closed_manifold(N(m.faces), m.vertices.shape[0])
    finally:
        x.copy_(saved)


def test_the_slab_sharded_and_2d_classes_do_not_support_it():
    import notebook_sim as NSIM
    import notebook_sim2d as NSIM2
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        inst = cls.__new__(cls)                                          # no process group needed to ask
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.skin()
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.skin_field(clip=False)
    with pytest.raises(NotImplementedError, match="3D"):
        NSIM2.NotebookSimulation2D.__new__(NSIM2.NotebookSimulation2D).skin()
