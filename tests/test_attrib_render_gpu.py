"""NotebookSimulation.render(color_by=...) and sample_particles on the MI355X: the scene of tests/test_skin_timestep_gpu.py
and tests/test_render_timestep_gpu.py (12 x 16 x 12, golden step_a_12x16x12) after one step, seen orthographically down
the box's diagonal, 96 x 64 pixels, aimed at the block of liquid, with the near plane between the block and the pool's
walls in front of it, which it cuts open.

The oracle starts from the GPU's own RenderResult (tests/test_render_timestep_gpu.py checks that), so only new code is
under test: hit points by the oracle's rays, the brute-force gather (tests/attrib_numpy.py), the colormap and the shading
formula in float64.  A liquid pixel's value before rounding, 255 albedo (0.25 + 0.75 lambert), carries the gather's bound
through the colormap: |d albedo| <= slope * bound / (hi - lo) + 8 u32 (the colormap's own float32 operations: two for t,
two for the position in the segment, a product, a sum, two rounded colours).  Pixels whose value lies within that of a
rounding boundary k + 1/2 form the band: there the byte may differ by one level, everywhere else it is equal.  The band
must hold at most 5 % of the liquid pixels: the bound is about 1e-5 of the value, so the band's expected share is about
2 * 255 * 1e-5 = 0.5 %; the share is printed by every run and the test fails above 5 %."""
import os

import numpy as np
import pytest
import torch

import attrib_numpy as A
import render_numpy as RN
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
W, H, NEAR, K = 96, 64, 1.7, 90
CENTRE, TOWARDS = np.array([0.02, 0.5, 0.0]), np.array([1.0, 0.8, 1.0])          # the block of liquid's centre


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


@pytest.fixture(scope="module")
def view(sim):
    from mfs import render
    step = 0.25 * sim.GDX
    eye = CENTRE + 2.0 * TOWARDS / np.sqrt(TOWARDS @ TOWARDS)
    return render.Camera(eye, CENTRE, ortho_height=0.65, width=W, height=H, near=NEAR, far=NEAR + (K - 0.5) * step)


@pytest.fixture(scope="module")
def seen(sim, view):
    """what the oracle starts from, computed once: the GPU's RenderResult as arrays, the oracle's hit points, the plain image"""
    from mfs import render, skin
    res = sim.render_result(view)
    o, d = RN.rays(view.basis(), W, H)
    depth, ident = N(res.depth).reshape(-1), N(res.shape_id).reshape(-1)
    with np.errstate(invalid="ignore"):
        pts = o + np.where(ident >= 0, depth, np.nan)[:, None] * d
    lo = np.asarray(sim.BOUND_MIN, np.float64)
    box = (lo, lo + np.asarray(sim.BOUND_SIZE, np.float64))
    R = 3.0 * skin.default_radius(0.5 * sim.GDX)
    out = dict(res=res, d=d, pts=pts, ident=ident, normal=N(res.normal).reshape(-1, 3).astype(np.float64), box=box, R=R,
               plain=N(sim.render(view)), px=N(sim.particle.x), pv=N(sim.particle.v), liquid=ident == 0)
    assert sim.skin_field().influence == R and out["liquid"].sum() > 250 and (ident == 1).sum() > 100 and (ident < 0).sum() > 100
    return out


def colormap64(stops, v, lo, hi):
    """mfs.render.Colormap.apply in float64"""
    ts = np.array([s[0] for s in stops], np.float64)
    cs = np.array([s[1] for s in stops], np.float64) / 255.0
    t = np.clip((v - lo) / (hi - lo), 0.0, 1.0)
    k = np.clip(np.searchsorted(ts, t, side="right") - 1, 0, len(ts) - 2)
    return cs[k] + (cs[k + 1] - cs[k]) * ((t - ts[k]) / (ts[k + 1] - ts[k]))[:, None]


def lambert(seen):
    n, l = seen["normal"], -seen["d"]
    return 0.25 + 0.75 * np.maximum(0.0, (n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1]) + n[:, 2] * l[:, 2])


def compare(rgb, seen, albedo, dalbedo, what):
    """the per-pixel assertions of the module docstring; albedo, dalbedo: (liquid pixels, 3) float64"""
    from mfs import render
    liq = seen["liquid"]
    got = rgb.reshape(-1, 3).astype(int)
    np.testing.assert_array_equal(got[~liq], seen["plain"].reshape(-1, 3)[~liq])       # solids and background: untouched
    w = lambert(seen)[liq][:, None]
    value = 255.0 * (albedo * w)
    want = np.clip(np.floor(value + 0.5), 0, 255).astype(int)
    slack = 255.0 * w * dalbedo + 1e-9
    band = (np.abs(value - (np.floor(value) + 0.5)) <= slack).any(axis=1)
    diff = np.abs(got[liq] - want)
    print(f"{what}: {liq.sum()} liquid pixels, band {band.sum()} ({band.mean():.2%}), {int((diff > 0).any(axis=1).sum())} pixels differ, "
          f"largest difference {diff.max()}, slack up to {slack.max():.2e} levels")
    assert band.mean() <= 0.05
    assert diff.max() <= 1
    np.testing.assert_array_equal(got[liq][~band], want[~band])
    assert len(np.unique(got[liq], axis=0)) > 20                                         # the liquid is not one flat colour


def test_hit_points_equal_the_oracles(seen, view):
    from mfs import render
    pts = N(render.hit_points(seen["res"], view)).reshape(-1, 3)
    hit = seen["ident"] >= 0
    assert np.isnan(pts[~hit]).all()
    assert np.abs(pts[hit] - seen["pts"][hit]).max() <= 8 * RN.EPS64 * 4.0             # coordinates below 4 in magnitude


def test_color_by_speed_matches_the_oracle(sim, view, seen):
    from mfs import render
    liq = seen["liquid"]
    speed = np.sqrt((seen["pv"] ** 2).sum(axis=1))
    ref = A.gather(seen["px"], speed, seen["pts"][liq], seen["R"], seen["box"])
    assert (ref["K"] > 0).all() and ref["W"].min() > 1e-6                # every skin hit lies within reach of a particle
    hi = float(torch.linalg.vector_norm(sim.particle.v, dim=1).max().item())
    stops = render.Colormap.PRESETS["speed"]
    slope = render.Colormap("speed").slope()
    albedo = colormap64(stops, ref["A"][:, 0], 0.0, hi)
    dalbedo = slope * ref["bound"] / hi + 8 * A.U32
    rgb = N(sim.render(view, color_by="speed"))
    assert rgb.dtype == np.uint8 and rgb.shape == (H, W, 3)
    compare(rgb, seen, albedo, dalbedo, "speed")
    # the same through a tensor, an explicit range and a Colormap object
    again = sim.render(view, color_by=torch.linalg.vector_norm(sim.particle.v, dim=1), color_range=(0.0, hi),
                       colormap=render.Colormap(stops))
    np.testing.assert_array_equal(N(again), rgb)
    # a preset of three stops over a narrower range: values clamped at both ends
    lo2, hi2 = 0.1 * hi, 0.9 * hi
    other = render.Colormap("diverging")
    compare(N(sim.render(view, color_by="speed", color_range=(lo2, hi2), colormap="diverging")), seen,
            colormap64(render.Colormap.PRESETS["diverging"], ref["A"][:, 0], lo2, hi2),
            other.slope() * ref["bound"] / (hi2 - lo2) + 8 * A.U32, "diverging")


def test_color_by_none_is_the_plain_image_and_look_is_refused(sim, view, seen):
    np.testing.assert_array_equal(N(sim.render(view, color_by=None)), seen["plain"])
    with pytest.raises(ValueError, match="color_by and look"):
        sim.render(view, color_by="speed", look="water")
    with pytest.raises(ValueError, match="liquid"):
        sim.render(view, what="solid", color_by="speed")
    with pytest.raises(ValueError, match="color_by"):
        sim.render(view, color_by=torch.zeros(7, device=DEV))
    with pytest.raises(ValueError, match="color_by"):
        sim.render(view, color_by="age")
    with pytest.raises(ValueError, match="color_range"):
        sim.render(view, color_by="speed", color_range=(1.0, 1.0))


def test_a_dye_splits_the_liquid_in_two_colours(sim, view, seen):
    px, liq = seen["px"], seen["liquid"]
    across = np.array([1.0, 0.0, -1.0]) / np.sqrt(2.0)                   # the image's horizontal: both halves face the camera
    plane = float(np.median(px @ across))
    dye = np.where((px @ across)[:, None] < plane, [[1.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]])
    rgb = N(sim.render(view, color_by=torch.tensor(dye, device=DEV))).reshape(-1, 3).astype(int)
    x = seen["pts"] @ across
    with np.errstate(invalid="ignore"):
        left, right = liq & (x < plane - seen["R"]), liq & (x > plane + seen["R"])
    print(f"dye: {left.sum()} pixels of the first liquid, {right.sum()} of the second, {(liq & ~left & ~right).sum()} between")
    assert left.sum() > 20 and right.sum() > 20
    assert (rgb[left, 0] >= 64).all() and (rgb[left, 1:] == 0).all()     # albedo x (0.25 + 0.75 lambert): at least a quarter
    assert (rgb[right, 2] >= 64).all() and (rgb[right, :2] == 0).all()
    np.testing.assert_array_equal(rgb[~liq], seen["plain"].reshape(-1, 3)[~liq])
    ref = A.gather(px, dye, seen["pts"][liq], seen["R"], seen["box"])
    compare(rgb.reshape(H, W, 3), seen, np.clip(ref["A"], 0.0, 1.0), ref["bound"] + A.U32, "dye")


def test_sample_particles_at_the_skins_vertices(sim, seen, tmp_path):
    from mfs import attrib, render, surface
    mesh = sim.skin()
    vel, weight = sim.sample_particles(mesh.vertices)
    V = int(mesh.vertices.shape[0])
    assert V > 500 and tuple(vel.shape) == (V, 3) and tuple(weight.shape) == (V,)
    direct = attrib.gather(mesh.vertices, sim.particle.x, sim.particle.v, seen["R"], seen["box"])
    assert torch.equal(vel.view(torch.int32), direct[0].view(torch.int32)) and torch.equal(weight, direct[1])
    assert torch.equal(attrib.at_vertices(mesh, sim.particle.x, sim.particle.v, seen["R"], seen["box"])[0].view(torch.int32),
                       vel.view(torch.int32))
    some = np.random.default_rng(2).choice(V, 300, replace=False)
    ref = A.gather(seen["px"], seen["pv"], N(mesh.vertices)[some].astype(np.float64), seen["R"], seen["box"])
    assert (ref["K"] > 0).all() and A.excess(N(vel)[some], ref).max() <= 1.0
    speed, _ = sim.sample_particles(mesh.vertices, "speed")
    assert tuple(speed.shape) == (V, 1) and bool((speed >= 0).all())
    with pytest.raises(ValueError, match="values"):
        sim.sample_particles(mesh.vertices, "age")
    # coloured export: the vertices come back
    colors = render.Colormap("speed").apply(speed[:, 0], 0.0, float(speed.max().item()))
    path = os.path.join(tmp_path, "skin.obj")
    attrib.save_obj(path, mesh, colors)
    rv, rf = surface.read_obj(path)
    np.testing.assert_array_equal(rv, N(mesh.vertices))
    np.testing.assert_array_equal(rf, N(mesh.faces))
