"""mfs.render on the MI355X against tests/render_numpy.py.  Before any pixel-wise comparison the test asserts that the
oracle's band -- the pixels a rounding could turn -- is empty, so no pixel is left out: step indices and shape ids are
then equal everywhere, depths and normals within the bounds the oracle derives per pixel."""
import numpy as np
import pytest
import torch

import render_numpy as RN
import seed_numpy as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
COLORS = [(230, 120, 40), (40, 120, 230)]


def volume(vol, origin, h):
    """an oracle volume on the GPU as a bare shape of mfs.seed (.phi / .origin / .spacing)"""
    from mfs.meshsdf import MeshSDF
    return MeshSDF(torch.as_tensor(np.ascontiguousarray(vol), device=DEV), tuple(float(v) for v in origin), float(h), 0.0)


def gpu_shape(o):
    """an oracle shape (vol, origin, h, R, T) as an mfs.seed.Shape with exactly that pose"""
    from mfs import seed
    s = seed.as_shape(volume(o[0], o[1], o[2]))
    s.R, s.T = np.ascontiguousarray(o[3]), np.asarray(o[4])
    return s


def camera(eye, target, W, H, near, step, K, **kw):
    """(mfs.render.Camera, the oracle's camera) with a far end that makes ceil((far - near) / step) == K whatever the rounding"""
    from mfs import render
    cam = render.Camera(eye, target, width=W, height=H, near=near, far=near + (K - 0.5) * step, **kw)
    assert render.plan([], cam, step)[3] == K
    b = cam.basis()
    o = RN.basis(eye, target, kw.get("up", (0, 1, 0)), kw.get("fov", 40.0), kw.get("ortho_height"), W, H)
    assert all(np.array_equal(b[k], o[k]) for k in ("eye", "f", "r", "u")) and b["half_w"] == o["half_w"] and b["half_h"] == o["half_h"]
    return cam, b


def agree(res, ref, where=None):
    """the four outputs against the oracle's on the pixels `where` (default: all)"""
    w = np.ones(ref["steps"].shape, bool) if where is None else where
    assert res.depth.dtype == torch.float64 and res.normal.dtype == torch.float32
    assert res.shape_id.dtype == torch.int32 and res.steps.dtype == torch.int32
    assert tuple(res.normal.shape) == ref["normal"].shape and res.depth.device == torch.device(DEV)
    np.testing.assert_array_equal(N(res.steps)[w], ref["steps"][w])
    np.testing.assert_array_equal(N(res.shape_id)[w], ref["shape_id"][w])
    depth, hit = N(res.depth), ref["steps"] >= 0
    assert np.isposinf(depth[w & ~hit]).all() and not N(res.normal)[w & ~hit].any()
    exact = w & hit & ~ref["secant"]
    np.testing.assert_array_equal(depth[exact], ref["depth"][exact])     # no secant: t_k itself
    sec = w & ref["secant"]
    dd = np.abs(depth[sec] - ref["depth"][sec])
    dn = np.abs(N(res.normal).astype(np.float64) - ref["normal"].astype(np.float64)).max(axis=-1)
    print(f"depth: largest difference {dd.max() if dd.size else 0.0:.3e} (largest bound {ref['depth_bound'].max():.3e}); normal: "
          f"{dn[w & hit].max() if (w & hit).any() else 0.0:.3e} (largest bound {ref['normal_bound'].max():.3e})")
    assert (dd <= ref["depth_bound"][sec]).all()
    assert (dn[w & hit] <= ref["normal_bound"][w & hit]).all()


def same_bits(a, b):
    return all(torch.equal(x, y) and N(x).tobytes() == N(y).tobytes() for x, y in zip(a[:4], b[:4]))


# ------------------------------------------------------------------------------------------------- the parity case ----
PARITY = dict(eye=(0.45, 0.62, 0.55), target=(0.02, 0.31, -0.01), W=48, H=40, near=0.2, step=0.003125, K=400)
VIEWS = {"perspective": (dict(fov=40.0), (1077, 371, 706, 279)), "orthographic": (dict(ortho_height=0.34 * 40 / 48 * 2), (1037, 316, 721, 380))}


@pytest.fixture(scope="module")
def parity():
    """seed_numpy.main_case() as a two-shape scene: the posed float32 torus, the float64 floor and ball; on the GPU once"""
    from mfs import render
    inc, exc = S.main_case()
    shapes = inc + exc
    scene = render.Scene([gpu_shape(s) for s in shapes])
    assert scene.shapes[0].volume.phi.dtype == torch.float32 and scene.shapes[1].volume.phi.dtype == torch.float64
    return shapes, scene


@pytest.mark.parametrize("view", sorted(VIEWS))
def test_parity_with_the_oracle_on_a_posed_torus_over_a_floor_and_a_ball(parity, view):
    from mfs import render
    shapes, scene = parity
    kw, (hits, torus, floor, plain) = VIEWS[view]
    p = PARITY
    cam, b = camera(p["eye"], p["target"], p["W"], p["H"], p["near"], p["step"], p["K"], **kw)
    ref = RN.render(shapes, b, p["W"], p["H"], p["near"], p["step"], p["K"])
    hit = ref["steps"] >= 0
    assert RN.band(ref) == 0                                             # nothing is left out of the comparison
    assert (int(hit.sum()), int((ref["shape_id"] == 0).sum()), int((ref["shape_id"] == 1).sum()), int((hit & ~ref["secant"]).sum())) == (hits, torus, floor, plain)
    st = {}
    res = scene.render(cam, step=p["step"], stats=st)
    assert (res.near, res.step, res.num_steps, res.num_shapes) == (p["near"], p["step"], p["K"], 2)
    agree(res, ref)
    assert st["pixels"] == 1920 and st["hits"] == hits and st["num_steps"] == 400
    assert same_bits(res, scene.render(cam, step=p["step"]))              # a second call: the same bits
    full = {}
    plain_res = scene.render(cam, step=p["step"], skip=False, stats=full)
    assert same_bits(res, plain_res)                                      # the skips are invisible
    print(f"{view}: {st['samples']} shape samples with the skips, {full['samples']} without")
    assert full["samples"] == ref["samples"] and 0 < st["samples"] < full["samples"]
    rgb = render.shade(res, cam, COLORS, background=(9, 8, 7))
    want = RN.shade(ref, COLORS, background=(9, 8, 7))
    assert rgb.dtype == torch.uint8 and tuple(rgb.shape) == (p["H"], p["W"], 3) and rgb.device == torch.device(DEV)
    assert np.abs(N(rgb).astype(int) - want.astype(int)).max() <= 1
    assert (N(rgb)[~hit] == (9, 8, 7)).all() and torch.equal(rgb, render.shade(plain_res, cam, COLORS, background=(9, 8, 7)))
    lit = render.shade(res, cam, COLORS, light=(0.3, 2.0, 0.4))
    want = RN.shade(ref, COLORS, light=np.array([0.3, 2.0, 0.4]) / np.sqrt((0.3 * 0.3 + 2.0 * 2.0) + 0.4 * 0.4))
    assert np.abs(N(lit).astype(int) - want.astype(int)).max() <= 1 and not torch.equal(lit, rgb)
    assert torch.equal(render.image(scene.shapes, cam, COLORS, background=(9, 8, 7), step=p["step"]), rgb)


# ------------------------------------------------------------------------------------------------------- the edges ----
def ball(shape, origin, h, centre, radius, dtype):
    p = S.nodes(shape, origin, h)
    return S.shape_of((np.sqrt(((p - np.asarray(centre)) ** 2).sum(axis=-1)) - radius).astype(dtype), origin, h)


def thin_and_tiny():
    """a float64 volume of 10 x 2 x 17 nodes -- one cell thick, bricks clipped on every axis -- that cuts a ball, and a posed
    float32 volume of 2 x 2 x 2 nodes, one cell cut by a plane"""
    thin = ball((10, 2, 17), (0, 0, 0), 0.1, (0.45, 0.05, 0.8), 0.3, np.float64)
    i = np.arange(2.0)
    cell = ((i[:, None, None] + i[None, :, None] + i[None, None, :]) - 1.2).astype(np.float32)
    return [thin, S.shape_of(cell, (0.55, 0.12, 0.75), 0.4, (S.rotation((1, 1, 0), 20), np.array([0.1, 0.0, 0.0])))]


@pytest.mark.parametrize("H,W", [(1, 1), (1, 70), (9, 8), (17, 3)])
def test_partial_tiles_and_small_volumes(H, W):
    """images that fill no tile, a wave with one live lane, a workgroup edge inside the image"""
    from mfs import render
    shapes = thin_and_tiny()
    near, step, K = 0.3, 0.02, 150
    cam, b = camera((1.4, 1.1, 2.1), (0.6, 0.05, 0.8), W, H, near, step, K, ortho_height=H * 1.6 / max(H, W))
    ref = RN.render(shapes, b, W, H, near, step, K)
    assert RN.band(ref) == 0 and (ref["steps"] >= 0).any()
    scene = render.Scene([gpu_shape(s) for s in shapes])
    st, full = {}, {}
    res = scene.render(cam, step=step, stats=st)
    agree(res, ref)
    assert same_bits(res, scene.render(cam, step=step, skip=False, stats=full))
    assert full["samples"] == ref["samples"] and st["samples"] < full["samples"] and st["hits"] == int((ref["steps"] >= 0).sum())
    rgb = render.shade(res, cam, COLORS)
    assert tuple(rgb.shape) == (H, W, 3) and np.abs(N(rgb).astype(int) - RN.shade(ref, COLORS).astype(int)).max() <= 1


def test_both_small_volumes_are_seen():
    shapes = thin_and_tiny()
    _, b = camera((1.4, 1.1, 2.1), (0.6, 0.05, 0.8), 70, 1, 0.3, 0.02, 150, ortho_height=1.6 / 70)
    ref = RN.render(shapes, b, 70, 1, 0.3, 0.02, 150)
    assert (ref["shape_id"] == 0).sum() > 10 and (ref["shape_id"] == 1).sum() > 10 and ref["secant"].sum() > 10


def test_a_volume_that_is_positive_everywhere_is_never_hit():
    from mfs import render
    pos = S.shape_of(np.full((4, 5, 6), 0.25, np.float32), (-0.4, -0.4, -0.4), 0.2)
    cam, _ = camera((0.1, 0.2, 3.0), (0.0, 0.0, 0.0), 20, 18, 1.0, 0.05, 80)
    st = {}
    res = render.Scene(gpu_shape(pos)).render(cam, step=0.05, stats=st)
    assert st["hits"] == 0 and st["pixels"] == 360 and st["num_steps"] == 80
    assert bool((res.steps == -1).all()) and bool((res.shape_id == -1).all()) and bool(torch.isposinf(res.depth).all())
    assert not bool(res.normal.any())
    assert (N(render.shade(res, cam, [(1, 2, 3)], background=(200, 100, 50))) == (200, 100, 50)).all()


def test_a_camera_inside_the_liquid_hits_at_its_first_sample():
    from mfs import render
    p = S.nodes((5, 5, 5), (-1, -1, -1), 0.5)
    neg = S.shape_of(-(1.0 + 0.3 * p[..., 0] + 0.2 * p[..., 1]), (-1, -1, -1), 0.5)     # negative on all of [-1, 1]^3
    near, step, K = 0.125, 0.05, 30
    cam, b = camera((0.1, 0.05, -0.2), (0.9, 0.3, 0.4), 9, 8, near, step, K, fov=60.0)
    ref = RN.render([neg], b, 9, 8, near, step, K)
    assert RN.band(ref) == 0 and (ref["steps"] == 0).all() and not ref["secant"].any()
    res = render.Scene(gpu_shape(neg)).render(cam, step=step)
    assert bool((res.steps == 0).all()) and bool((res.depth == near).all()) and bool((res.shape_id == 0).all())
    agree(res, ref)


def test_rays_that_meet_no_box_evaluate_no_sample():
    from mfs import render
    neg = S.shape_of(np.full((3, 3, 3), -1.0), (0, 0, 0), 0.5)           # the box [0, 1]^3
    cam, _ = camera((5.0, 5.0, 5.0), (6.0, 5.5, 7.0), 9, 8, 0.0, 0.1, 50)
    scene = render.Scene(gpu_shape(neg))
    st, full = {}, {}
    res = scene.render(cam, step=0.1, stats=st)
    assert same_bits(res, scene.render(cam, step=0.1, skip=False, stats=full))
    assert st["hits"] == full["hits"] == 0 and st["samples"] == 0 and full["samples"] == 72 * 50


def test_sixteen_shapes_are_accepted_and_seventeen_refused():
    from mfs import render
    rng = np.random.default_rng(11)
    shapes = []
    for k in range(16):                                                  # balls of 5^3 nodes on a 4 x 4 raster, alternating dtypes
        c = (0.3 * (k % 4) + 0.013 * k, 0.3 * (k // 4), 0.02 * float(rng.standard_normal()))
        shapes.append(ball((5, 5, 5), (c[0] - 0.1, c[1] - 0.1, c[2] - 0.1), 0.05, c, 0.08, (np.float32, np.float64)[k % 2]))
    near, step, K = 1.0, 0.0125, 180
    cam, b = camera((0.47, 0.44, 2.0), (0.47, 0.44, 0.0), 24, 22, near, step, K, ortho_height=1.4)
    ref = RN.render(shapes, b, 24, 22, near, step, K)
    assert RN.band(ref) == 0 and len(np.unique(ref["shape_id"])) == 17    # every shape, and the background
    scene = render.Scene([gpu_shape(s) for s in shapes])
    res = scene.render(cam, step=step)
    agree(res, ref)
    assert same_bits(res, scene.render(cam, step=step, skip=False))
    with pytest.raises(ValueError, match="1 .. 16"):
        render.Scene(scene.shapes + [scene.shapes[0]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_nan_node_is_passed_over_and_its_brick_never_skipped(dtype):
    from mfs import render
    vol = ball((20, 20, 20), (0, 0, 0), 0.05, (0.5, 0.5, 0.5), 0.3, dtype)[0].copy()
    node = (13, 17, 14)                                                  # outside the ball, towards the camera: rays pass its cells on their way in
    vol[node] = np.nan
    shape = S.shape_of(vol, (0, 0, 0), 0.05)
    near, step, K = 0.3, 0.01, 300
    cam, b = camera((1.5, 1.2, 1.9), (0.5, 0.5, 0.5), 24, 20, near, step, K, fov=35.0)

    def touches(i, u):                                                   # a sample in one of the eight cells around the node
        return ((u > np.asarray(node) - 1.0) & (u < np.asarray(node) + 1.0)).all(axis=-1)

    ref = RN.render([shape], b, 24, 20, near, step, K, touched=touches)
    assert ref["touched"].sum() > 5 and not (ref["band"] & ~ref["touched"]).any()
    scene = render.Scene(gpu_shape(shape))
    bricks = N(scene.bricks[0])
    assert np.array_equal(bricks, RN.bricks(vol)) and np.isneginf(bricks[1, 2, 1]) and np.isneginf(bricks).sum() == 1
    res = scene.render(cam, step=step)
    agree(res, ref, ~ref["band"])
    assert same_bits(res, scene.render(cam, step=step, skip=False))
    assert (ref["steps"] >= 0)[ref["touched"]].any()                      # rays that crossed the NaN cells still find the ball


# ------------------------------------------------------------------------------------------------------ the bricks ----
def test_brick_minima_equal_the_oracles_bit_for_bit():
    from mfs import render
    rng = np.random.default_rng(2)
    torus = S.torus_volume()[0]
    odd = rng.standard_normal((10, 2, 17))
    odd[9, 1, 16] = -7.0                                                 # the last node belongs to the last brick alone
    for vol in (torus, odd, odd.astype(np.float32), rng.standard_normal((2, 2, 2)), rng.standard_normal((9, 10, 18)).astype(np.float32)):
        scene = render.Scene(volume(vol, (0, 0, 0), 0.1))
        got, want = N(scene.bricks[0]), RN.bricks(vol)
        assert got.dtype == np.float64 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert N(scene.bricks[0]).shape == (1, 2, 3) and RN.bricks(odd)[1, 0, 1] == -7.0
    # refresh() follows the volume's contents
    scene.shapes[0].volume.phi[8, 9, 17] = -50.0
    assert N(scene.bricks[0]).min() > -50.0
    scene.refresh()
    assert (N(scene.bricks[0])[:, 1, 2] == -50.0).all() and N(scene.bricks[0]).tobytes() == RN.bricks(N(scene.shapes[0].volume.phi)).tobytes()


def test_near_and_far_default_to_the_shapes_boxes():
    from mfs import render
    b = ball((17, 17, 17), (-0.4, -0.4, -0.4), 0.05, (0, 0, 0), 0.3, np.float32)
    scene = render.Scene(gpu_shape(b))
    free = render.Camera((0.3, 0.5, 2.0), (0, 0, 0), width=16, height=12)
    res = scene.render(free)
    assert res.step == 0.025 and 0 < res.near < np.linalg.norm((0.3, 0.5, 2.0)) - 0.3 and res.far > np.linalg.norm((0.3, 0.5, 2.0)) + 0.3 and res.num_steps == int(np.ceil((res.far - res.near) / res.step))
    fixed = render.Camera((0.3, 0.5, 2.0), (0, 0, 0), width=16, height=12, near=res.near, far=res.far)
    assert same_bits(res, scene.render(fixed)) and int((res.steps >= 0).sum()) > 10
