"""NotebookSimulation.render() on the MI355X: the scene of tests/test_skin_timestep_gpu.py (12 x 16 x 12, golden
step_a_12x16x12: a closed pool with a ramp, a block of liquid) after two steps, seen orthographically down the box's
diagonal with the near plane cutting the pool open.

The fields of a run are not made for an empty band (flat regions, samples on nodes), so for this one case the oracle's band
may hold up to 2 % of the pixels and the comparison leaves those out.  On a synthetic stand-in of the scene on the CPU -- the
pool and the ramp as exact distances on the same 25 x 33 x 25 lattice, a rounded block of liquid clipped against them --
this view has an empty band (1018 hits of 3072 pixels, 292 of them in the cut wall at sample 0)."""
import numpy as np
import pytest
import torch

import render_numpy as RN
import seed_numpy as S
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
W, H, NEAR, K = 64, 48, 1.9, 68
CENTRE, TOWARDS = np.array([0.0, 0.4, 0.0]), np.array([1.0, 0.8, 1.0])


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
    s.step()
    return s


def view(sim):
    from mfs import render
    step = 0.25 * sim.GDX                                                # half the lattice's spacing: the default
    eye = CENTRE + 2.0 * TOWARDS / np.sqrt(TOWARDS @ TOWARDS)
    cam = render.Camera(eye, CENTRE, ortho_height=1.3, width=W, height=H, near=NEAR, far=NEAR + (K - 0.5) * step)
    return cam, step


def test_render_returns_an_image_with_liquid_solid_and_background(sim):
    from mfs import render
    cam, step = view(sim)
    rgb = sim.render(cam, colors=[(0, 0, 255), (255, 0, 0)])
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (H, W, 3) and rgb.device == torch.device(DEV)
    a = N(rgb).astype(int)
    liquid = (a[..., 0] == 0) & (a[..., 1] == 0) & (a[..., 2] >= 64)     # albedo x (0.25 + 0.75 lambert): at least a quarter
    solid = (a[..., 1] == 0) & (a[..., 2] == 0) & (a[..., 0] >= 64)
    back = (a == 255).all(axis=-1)
    print(f"render: {liquid.sum()} liquid, {solid.sum()} solid, {back.sum()} background pixels of {W * H}")
    assert liquid.sum() > 10 and solid.sum() > 200 and back.sum() > 200 and (liquid | solid | back).all()
    res = sim.render_result(cam)
    assert res.step == step and res.num_steps == K and res.num_shapes == 2
    np.testing.assert_array_equal(N(res.shape_id) == 0, liquid)
    np.testing.assert_array_equal(N(res.shape_id) == 1, solid)
    # the default colours, and one of the two alone
    assert torch.equal(sim.render(cam), render.shade(res, cam, [render.LIQUID_COLOR, render.SOLID_COLOR]))
    alone = sim.render_result(cam, what="solid")
    assert alone.num_shapes == 1 and bool(((alone.shape_id == 0) == (alone.steps >= 0)).all())
    assert int((alone.steps >= 0).sum()) >= int(solid.sum())
    with pytest.raises(ValueError, match="what"):
        sim.render(cam, what=("liquid", "air"))


def test_render_result_agrees_with_the_oracle_on_the_runs_own_fields(sim):
    cam, step = view(sim)
    f = sim.skin_field()
    shapes = [S.shape_of(N(f.phi), f.origin, f.spacing), S.shape_of(N(sim.solid_levelset.phi), f.origin, f.spacing)]
    assert shapes[0][0].shape == shapes[1][0].shape == (25, 33, 25) and f.spacing == 2 * step
    ref = RN.render(shapes, cam.basis(), W, H, NEAR, step, K)
    out = ~ref["band"]
    print(f"oracle: band {RN.band(ref)} of {W * H} pixels, {int((ref['steps'] >= 0).sum())} hits")
    assert RN.band(ref) <= 0.02 * W * H
    res = sim.render_result(cam)
    np.testing.assert_array_equal(N(res.steps)[out], ref["steps"][out])
    np.testing.assert_array_equal(N(res.shape_id)[out], ref["shape_id"][out])
    sec = out & ref["secant"]
    assert (np.abs(N(res.depth)[sec] - ref["depth"][sec]) <= ref["depth_bound"][sec]).all()
    assert (ref["shape_id"][out] == 0).any() and (ref["shape_id"][out] == 1).any() and (ref["shape_id"][out] == -1).any()


def test_the_slab_and_sharded_classes_do_not_support_it():
    import notebook_sim as NSIM
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        inst = cls.__new__(cls)                                          # no process group needed to ask
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.render(None)
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.render_result(None)
