"""NotebookSimulation.render(look=...) on the MI355X: the scene and the camera of tests/test_render_timestep_gpu.py (12 x 16 x
12, golden step_a_12x16x12, two steps; orthographic down the box's diagonal, the near plane cutting the pool open) with
look="water": the skin refracts and absorbs, the pool and the ramp are opaque and cast shadows, 2 x 2 rays per pixel.

As there, the fields of a run are not made for an empty band, so the oracle's band may hold up to 2 % of the rays and the
comparison leaves those out."""
import numpy as np
import pytest
import torch

import render_paths_numpy as RP
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


def test_a_water_look_of_a_run_agrees_with_the_oracle_and_leaves_the_plain_render_alone(sim):
    from mfs import render
    step = 0.25 * sim.GDX
    eye = CENTRE + 2.0 * TOWARDS / np.sqrt(TOWARDS @ TOWARDS)
    cam = render.Camera(eye, CENTRE, ortho_height=1.3, width=W, height=H, near=NEAR, far=NEAR + (K - 0.5) * step)
    before = sim.render(cam)
    rgb = sim.render(cam, look="water")
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (H, W, 3) and rgb.device == torch.device(DEV)
    assert not torch.equal(rgb, before)
    res, look = render.simulation_paths(sim, cam, ("liquid", "solid"), "water", trace=True)
    assert (res.step, res.num_steps, res.samples, res.num_shapes) == (step, K, 2, 2) and tuple(res.color.shape) == (2 * H, 2 * W, 3)
    assert torch.equal(render.resolve(res), rgb)
    assert torch.equal(sim.render(cam, look=look), rgb)                   # the same Look, given as one

    f = sim.skin_field()
    shapes = [S.shape_of(N(f.phi), f.origin, f.spacing), S.shape_of(N(sim.solid_levelset.phi), f.origin, f.spacing)]
    mats = [RP.liquid(m.color, m.ior, m.absorb) if m.is_liquid else RP.opaque(m.color) for m in look.materials]
    ref = RP.trace(shapes, mats, cam.basis(), 2 * W, 2 * H, NEAR, step, K, light=look.light)
    out = ~ref["band"]
    print(f"oracle: band {RP.band(ref)} of {4 * W * H} rays; {ref['counts']}")
    assert RP.band(ref) <= 0.02 * 4 * W * H
    assert ref["counts"]["liquid"] > 40 and ref["counts"]["opaque"] > 800
    np.testing.assert_array_equal(N(res.steps)[out], ref["steps"][out])
    np.testing.assert_array_equal(N(res.shape_id)[out], ref["shape_id"][out])
    dl = np.abs(N(res.length) - ref["length"])[out]
    dc = np.abs(N(res.color) - ref["color"]).max(axis=-1)[out]
    print(f"length: largest difference {dl.max():.3e} (largest bound {ref['length_bound'][out].max():.3e}); colour: {dc.max():.3e} "
          f"(largest bound {ref['color_bound'][out].max():.3e})")
    assert (dl <= ref["length_bound"][out]).all() and (dc <= ref["color_bound"][out]).all()

    assert torch.equal(sim.render(cam), before)                           # the plain render: the bits it returned before
    with pytest.raises(ValueError, match="water"):
        sim.render(cam, look="wine")
