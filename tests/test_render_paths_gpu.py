"""mfs.render's paths (Scene.trace / resolve: shadows, a refracting liquid, supersampling) on the MI355X against
tests/render_paths_numpy.py.  Every comparison first asserts the size of the oracle's band -- the rays a rounding could turn,
or whose derived colour bound exceeds 1e-6 -- and then demands, on every ray outside it: equal step indices and shape ids
in all four slots, the length inside the liquid and the float colour within the bounds the oracle derives per ray, bytes
within one level; the same bits from a second call and from skip=False."""
import numpy as np
import pytest
import torch

import render_numpy as RN
import render_paths_numpy as RP
import seed_numpy as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
LIGHT = (0.3, 2.0, 0.4)
WATER = ("liquid", (40, 120, 230), 1.33, (2.0, 1.0, 0.3))
STONE = ("opaque", (190, 185, 175))


def volume(vol, origin, h):
    from mfs.meshsdf import MeshSDF
    return MeshSDF(torch.as_tensor(np.ascontiguousarray(vol), device=DEV), tuple(float(v) for v in origin), float(h), 0.0)


def gpu_shape(o):
    """an oracle shape (vol, origin, h, R, T) as an mfs.seed.Shape with exactly that pose"""
    from mfs import seed
    s = seed.as_shape(volume(o[0], o[1], o[2]))
    s.R, s.T = np.ascontiguousarray(o[3]), np.asarray(o[4])
    return s


def camera(eye, target, W, H, near, step, K, **kw):
    """(mfs.render.Camera, the oracle's camera) with a far end that makes ceil((far - near) / step) == K"""
    from mfs import render
    cam = render.Camera(eye, target, width=W, height=H, near=near, far=near + (K - 0.5) * step, **kw)
    assert render.plan([], cam, step)[3] == K
    return cam, cam.basis()


def looks(materials, light=LIGHT, **kw):
    """(mfs.render.Look, the oracle's materials, the oracle's keywords) of one description"""
    from mfs import render
    mine = [render.Material.liquid(m[1], m[2], m[3]) if m[0] == "liquid" else render.Material.opaque(m[1]) for m in materials]
    theirs = [RP.liquid(m[1], m[2], m[3]) if m[0] == "liquid" else RP.opaque(m[1]) for m in materials]
    look = render.Look(mine, light, **kw)
    okw = dict(light=None if light is None else RP.unit(light), background=kw.get("background", (255, 255, 255)),
               shadows=kw.get("shadows", True), bias=kw.get("bias"), K_shadow=kw.get("shadow_steps"), K_inside=kw.get("inside_steps"))
    return look, theirs, okw


def same_bits(a, b):
    return all(torch.equal(x, y) and N(x).tobytes() == N(y).tobytes() for x, y in zip(a[:4], b[:4]))


def agree(res, ref, tag=""):
    """every output against the oracle's on the rays outside its band"""
    w = ~ref["band"]
    assert res.color.dtype == torch.float64 and res.length.dtype == torch.float64
    assert res.steps.dtype == torch.int32 and res.shape_id.dtype == torch.int32
    assert tuple(res.color.shape) == ref["color"].shape and tuple(res.steps.shape) == ref["steps"].shape
    assert tuple(res.shape_id.shape) == ref["shape_id"].shape and tuple(res.length.shape) == ref["length"].shape
    np.testing.assert_array_equal(N(res.steps)[w], ref["steps"][w])
    np.testing.assert_array_equal(N(res.shape_id)[w], ref["shape_id"][w])
    dl = np.abs(N(res.length) - ref["length"])[w]
    dc = np.abs(N(res.color) - ref["color"]).max(axis=-1)[w]
    big = lambda v: float(v.max()) if v.size else 0.0  # noqa: E731
    print(f"{tag}: length: largest difference {big(dl):.3e} (largest bound {big(ref['length_bound'][w]):.3e}); colour: "
          f"{big(dc):.3e} (largest bound {big(ref['color_bound'][w]):.3e}); band {RP.band(ref)}")
    assert (dl <= ref["length_bound"][w]).all()
    assert (dc <= ref["color_bound"][w]).all()


def check(shapes, materials, cam_args, W, H, near, step, K, samples=1, band=0, light=LIGHT, **kw):
    """the oracle and the GPU on one scene: band size first, then everything; returns (ref, res, scene, cam, look)"""
    from mfs import render
    look, mats, okw = looks(materials, light, samples=samples, **kw)
    cam, b = camera(*cam_args[:2], W, H, near, step, K, **cam_args[2])
    ref = RP.trace(shapes, mats, b, samples * W, samples * H, near, step, K, **okw)
    assert RP.band(ref) <= band, RP.band(ref)
    scene = render.Scene([gpu_shape(s) for s in shapes])
    st, full = {}, {}
    res = scene.trace(cam, look, step=step, stats=st)
    assert (res.near, res.step, res.num_steps, res.num_shapes, res.samples) == (near, step, K, len(shapes), samples)
    agree(res, ref, f"{W} x {H} x {samples}^2")
    assert same_bits(res, scene.trace(cam, look, step=step))              # a second call: the same bits
    plain = scene.trace(cam, look, step=step, skip=False, stats=full)
    assert same_bits(res, plain)                                          # the skips are invisible
    assert full["samples"] == ref["samples"] and st["samples"] <= full["samples"]
    assert st["pixels"] == samples * samples * W * H and st["hits"] == int((ref["steps"][..., 0] >= 0).sum())
    rgb = render.resolve(res)
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (H, W, 3) and rgb.device == torch.device(DEV)
    assert N(rgb).tobytes() == RP.resolve(N(res.color), samples).tobytes()   # the fixed-order mean of its own colours
    if RP.band(ref) == 0:
        assert np.abs(N(rgb).astype(int) - RP.resolve(ref["color"], samples).astype(int)).max() <= 1
    return ref, res, scene, cam, look, (st, full)


# ------------------------------------------------------------------------------------------------- the parity case ----
PARITY = dict(eye=(0.45, 0.62, 0.55), target=(0.02, 0.31, -0.01), W=48, H=40, near=0.2, step=0.003125, K=400)
VIEWS = {"perspective": (dict(fov=40.0), dict(liquid=371, opaque=706, exits=343, met_inside=28, shadowed=13, opaque_after_exit=60)),
         "orthographic": (dict(ortho_height=0.34 * 40 / 48 * 2),
                          dict(liquid=316, opaque=721, exits=291, met_inside=25, shadowed=36, opaque_after_exit=132))}


def parity_shapes():
    inc, exc = S.main_case()
    return inc + exc


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_parity_with_the_oracle_on_a_refracting_torus_over_a_floor_and_a_ball(view):
    """the posed float32 torus as the liquid, the float64 floor and ball opaque: the band is empty, the outcomes of the
    paths are the prototype's (shadows are counted over every surface finally shaded, after slots 1 and 2 too)"""
    p = PARITY
    kw, counts = VIEWS[view]
    ref, res, scene, cam, look, (st, full) = check(parity_shapes(), [WATER, STONE], (p["eye"], p["target"], kw), p["W"], p["H"],
                                                   p["near"], p["step"], p["K"])
    got = {k: ref["counts"][k] for k in counts}
    assert got == counts and ref["counts"]["reflected"] == 0 and ref["counts"]["inside_miss"] == 0
    assert scene.shapes[0].volume.phi.dtype == torch.float32 and scene.shapes[1].volume.phi.dtype == torch.float64
    assert res.bias == 4 * p["step"] and res.shadow_steps == res.inside_steps == p["K"]
    print(f"{view}: {st['samples']} shape samples with the skips, {full['samples']} without")
    assert 0 < st["samples"] < full["samples"]
    ids = N(res.shape_id)
    assert ((ids[..., 1] == -2) == (ids[..., 0] != 0)).all()               # slot 1 runs exactly behind a liquid hit
    inside = N(res.length)[ids[..., 0] == 0]                             # 0 where a grazing ray's start is outside already
    assert (N(res.length)[ids[..., 0] != 0] == 0).all() and (inside >= 0).all() and (inside > 0).sum() > 250
    assert scene.bricks_max[0] is not None and scene.bricks_max[1] is None   # maxima of the liquid alone


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_opaque_materials_without_shadows_repeat_todays_shading_byte_for_byte(view):
    from mfs import render
    p = PARITY
    colors = [(230, 120, 40), (40, 120, 230)]
    cam, _ = camera(p["eye"], p["target"], p["W"], p["H"], p["near"], p["step"], p["K"], **VIEWS[view][0])
    scene = render.Scene([gpu_shape(s) for s in parity_shapes()])
    today = scene.render(cam, step=p["step"])
    for light in (None, LIGHT):
        look = render.Look([render.Material.opaque(c) for c in colors], light, background=(9, 8, 7), shadows=False)
        res = scene.trace(cam, look, step=p["step"])
        assert torch.equal(render.resolve(res), render.shade(today, cam, colors, background=(9, 8, 7), light=light))
        assert torch.equal(res.steps[..., 0], today.steps) and torch.equal(res.shape_id[..., 0], today.shape_id)
        assert bool((res.steps[..., 1:] == -2).all()) and not bool(res.length.any())
        assert torch.equal(render.image_paths(scene.shapes, cam, look, step=p["step"]), render.resolve(res))
    assert scene.bricks_max == [None, None]                               # no liquid: no maxima are built


def liquid_box():
    """a float64 box, half extents (0.1, 0.05, 0.1) about the origin, as an exact distance on 49 x 33 x 49 nodes"""
    org, h = (-0.15, -0.1, -0.15), 0.00625
    q = np.abs(S.nodes((49, 33, 49), org, h)) - np.array([0.1, 0.05, 0.1])
    return S.shape_of(np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=-1)) + np.minimum(q.max(axis=-1), 0.0), org, h)


def test_total_internal_reflection_in_a_box_of_liquid():
    """rays that enter the top of the box and meet a side wall from inside beyond the critical angle"""
    ref, res, *_ = check([liquid_box()], [WATER], ((0.5, -0.02, 0.12), (0, 0.03, 0), dict(fov=30.0)), 24, 20, 0.2, 0.003125, 200)
    c = ref["counts"]
    assert (c["liquid"], c["exits"], c["reflected"], c["opaque"]) == (154, 154, 53, 0)
    ids, steps = N(res.shape_id), N(res.steps)
    tir = (ids[..., 1] == 0) & (steps[..., 2] == -2)                      # left the liquid's surface, no march after it
    assert int(tir.sum()) == 53 and (N(res.length)[tir] > 0).all()


# --------------------------------------------------------------------------------------------------- supersampling ----
def test_supersampling_is_the_fixed_order_mean_of_the_finer_trace():
    """9 x 8 pixels, 2 x 2 rays each: the trace is the 18 x 16 image's, the bytes the mean of its colours in row-major
    order (asserted bit for bit in `check`), and they differ from one ray per pixel"""
    from mfs import render
    p = PARITY
    args = (p["eye"], p["target"], VIEWS["perspective"][0])
    ref, res, scene, cam, look, _ = check(parity_shapes(), [WATER, STONE], args, 9, 8, p["near"], p["step"], p["K"], samples=2)
    assert tuple(res.color.shape) == (16, 18, 3)
    fine, _ = camera(p["eye"], p["target"], 18, 16, p["near"], p["step"], p["K"], **VIEWS["perspective"][0])
    one = render.Look(look.materials, LIGHT)
    assert same_bits(res, scene.trace(fine, one, step=p["step"]))          # the same camera at (2 W, 2 H)
    coarse = render.resolve(scene.trace(cam, one, step=p["step"]))
    assert tuple(coarse.shape) == (8, 9, 3) and not torch.equal(coarse, render.resolve(res))


# ------------------------------------------------------------------------------------------------------- the edges ----
def ball(shape, origin, h, centre, radius, dtype):
    p = S.nodes(shape, origin, h)
    return S.shape_of((np.sqrt(((p - np.asarray(centre)) ** 2).sum(axis=-1)) - radius).astype(dtype), origin, h)


def thin_and_tiny():
    """the small volumes of tests/test_render_gpu.py: a float64 volume one cell thick that cuts a ball (the liquid here), and a
    posed float32 volume of 2 x 2 x 2 nodes cut by a plane (opaque)"""
    thin = ball((10, 2, 17), (0, 0, 0), 0.1, (0.45, 0.05, 0.8), 0.3, np.float64)
    i = np.arange(2.0)
    cell = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) - 1.2).astype(np.float32)
    return [thin, S.shape_of(cell, (0.55, 0.12, 0.75), 0.4, (S.rotation((1, 1, 0), 20), np.array([0.1, 0.0, 0.0])))]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (17, 3)])
def test_partial_tiles_with_three_by_three_rays_per_pixel(H, W):
    """images that fill no tile, a wave with few live lanes, a workgroup edge inside the supersampled image"""
    args = ((1.4, 1.1, 2.1), (0.6, 0.05, 0.8), dict(ortho_height=H * 1.6 / max(H, W)))
    ref, res, *_ = check(thin_and_tiny(), [WATER, STONE], args, W, H, 0.3, 0.02, 150, samples=3)
    assert tuple(res.color.shape) == (3 * H, 3 * W, 3) and (ref["steps"][..., 0] >= 0).any()


def all_negative():
    p = S.nodes((5, 5, 5), (-1, -1, -1), 0.5)
    return S.shape_of(-(1.0 + 0.3 * p[..., 0] + 0.2 * p[..., 1]), (-1, -1, -1), 0.5)     # negative on all of [-1, 1]^3


def test_a_camera_inside_the_liquid_hits_at_its_first_sample_and_the_path_goes_on():
    ref, res, *_ = check([all_negative()], [WATER], ((0.1, 0.05, -0.2), (0.9, 0.3, 0.4), dict(fov=60.0)), 9, 8, 0.125, 0.05, 30)
    steps, ids = N(res.steps), N(res.shape_id)
    assert (steps[..., 0] == 0).all() and (ids[..., 0] == 0).all()        # no secant: the hit is at near itself
    assert (steps[..., 1] >= 0).all() and (ids[..., 1] == 0).all()        # the inside march ran and left the box


def test_a_liquid_that_fills_its_box_is_left_at_a_sample_without_a_secant():
    """outside the box the negated shape is -inf: a non-finite hit, depth = t_k, a whole number of steps"""
    step = 0.05
    ref, res, *_ = check([all_negative()], [WATER], ((0.4, 0.3, 3.0), (0.0, 0.0, 0.0), dict(ortho_height=1.2)), 9, 8, 1.0, step, 80)
    ids, length = N(res.shape_id), N(res.length)
    assert (ids[..., 0] == 0).all() and (ids[..., 1] == 0).all()
    np.testing.assert_array_equal(length, N(res.steps)[..., 1] * np.float64(step))
    assert (ref["length_bound"] == 0).all()


def test_a_scene_of_liquid_alone_samples_nothing_in_its_shadow_marches():
    """a ring seen nearly edge-on: rays leave the near tube and meet the far one (slot 2), and that surface's shadow ray has
    no shape to sample"""
    ring = [S.shape_of(*S.torus_volume())]
    args = (RING["eye"], RING["target"], dict(fov=40.0))
    ref, res, *_ = check(ring, [WATER], args, 24, 20, RING["near"], RING["step"], RING["K"])
    ids = N(res.shape_id)
    assert (ids[..., 2] == 0).sum() > 5 and ((ids[..., 3] == -1) == (ids[..., 2] == 0)).all()
    assert ((ids[..., 3] == -2) == (ids[..., 2] != 0)).all()
    only = RP.trace(ring, [RP.liquid(*WATER[1:])], camera(RING["eye"], RING["target"], 24, 20, RING["near"], RING["step"], RING["K"], fov=40.0)[1],
                    24, 20, RING["near"], RING["step"], RING["K"], light=RP.unit(LIGHT), shadows=False)
    assert only["samples"] == ref["samples"] and np.array_equal(only["color"], ref["color"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_nan_node_in_the_liquid_is_skipped_by_neither_grid(dtype):
    from mfs import render
    vol = ball((20, 20, 20), (0, 0, 0), 0.05, (0.5, 0.5, 0.5), 0.3, dtype)[0].copy()
    vol[10, 11, 10] = np.nan                                             # inside the ball: the inside marches pass its cells
    shape = S.shape_of(vol, (0, 0, 0), 0.05)
    args = ((1.5, 1.2, 1.9), (0.5, 0.5, 0.5), dict(fov=35.0))
    ref, res, scene, *_ = check([shape], [WATER], args, 24, 20, 0.3, 0.01, 300)
    lo, hi = N(scene.bricks[0]), N(scene.bricks_max[0])
    assert hi.tobytes() == RP.bricks_max(vol).tobytes() and lo.tobytes() == RN.bricks(vol).tobytes()
    assert np.isposinf(hi[1, 1, 1]) and np.isneginf(lo[1, 1, 1]) and np.isinf(hi).sum() == 1
    assert (~ref["band"] & (ref["steps"][..., 1] >= 0)).sum() > 20        # paths through the ball are compared


@pytest.mark.parametrize("absorb", [(0.0, 0.0, 0.0), (1e6, 3e5, 2e7)])
def test_no_absorption_and_a_very_large_one(absorb):
    p = PARITY
    mats = [("liquid", (40, 120, 230), 1.33, absorb), STONE]
    ref, res, *_ = check(parity_shapes(), mats, (p["eye"], p["target"], VIEWS["perspective"][0]), 12, 10, p["near"], p["step"],
                         p["K"])
    wet = ref["steps"][..., 0] >= 0
    wet &= ref["shape_id"][..., 0] == 0
    assert wet.sum() > 5 and np.isfinite(N(res.color)).all()


def test_sixteen_shapes_with_every_other_one_a_liquid():
    rng = np.random.default_rng(11)
    shapes, mats = [], []
    for k in range(16):                                                  # balls of 5^3 nodes on a 4 x 4 raster, alternating dtypes
        c = (0.3 * (k % 4) + 0.013 * k, 0.3 * (k // 4), 0.02 * float(rng.standard_normal()))
        shapes.append(ball((5, 5, 5), (c[0] - 0.1, c[1] - 0.1, c[2] - 0.1), 0.05, c, 0.08, (np.float32, np.float64)[k % 2]))
        mats.append(("liquid", (10 * k, 120, 230), 1.2 + 0.1 * k, (1.0, 2.0, 3.0)) if k % 3 else ("opaque", (200, 10 * k, 90)))
    args = ((0.47, 0.44, 2.0), (0.47, 0.44, 0.0), dict(ortho_height=1.4))
    ref, res, *_ = check(shapes, mats, args, 24, 22, 1.0, 0.0125, 180)
    assert len(np.unique(ref["shape_id"][..., 0])) == 17                  # every shape, and the background


def test_brick_maxima_equal_the_oracles_bit_for_bit():
    from mfs import render
    rng = np.random.default_rng(2)
    odd = rng.standard_normal((10, 2, 17))
    odd[9, 1, 16] = 7.0                                                  # the last node belongs to the last brick alone
    for vol in (S.torus_volume()[0], odd, odd.astype(np.float32), rng.standard_normal((2, 2, 2)),
                rng.standard_normal((9, 10, 18)).astype(np.float32)):
        scene = render.Scene(volume(vol, (0, 0, 0), 0.1))
        got, want = N(scene._maxima(0)), RP.bricks_max(vol)
        assert got.dtype == np.float64 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert RP.bricks_max(odd)[1, 0, 1] == 7.0
    # refresh() follows the volume's contents, for the maxima that were built
    scene.shapes[0].volume.phi[8, 9, 17] = 50.0
    scene.refresh()
    assert (N(scene.bricks_max[0])[:, 1, 2] == 50.0).all()
    assert N(scene.bricks_max[0]).tobytes() == RP.bricks_max(N(scene.shapes[0].volume.phi)).tobytes()


RING = dict(eye=(0.6, 0.05, 0.03), target=(0.0, 0.0, 0.0), near=0.2, step=0.003125, K=320)
