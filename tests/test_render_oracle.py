"""The ray marcher without a GPU: tests/render_numpy.py on cases with a closed form, mfs.render's host side (camera, refusals,
PNG writer) and the C entry points' argument checks, which all return before any launch."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest
import torch

import render_numpy as RN
import seed_numpy as S

NEW = ("mfs_render_brick_count3d", "mfs_render_bricks3d", "mfs_render_march3d", "mfs_render_shade3d")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    return _lib.load()


def ball(shape, origin, h, centre, radius, dtype=np.float64):
    p = S.nodes(shape, origin, h)
    return S.shape_of((np.sqrt(((p - np.asarray(centre)) ** 2).sum(axis=-1)) - radius).astype(dtype), origin, h)


# ------------------------------------------------------------------------------------------------------ the oracle ----
H_BALL, R_BALL = 0.025, 0.3


def test_a_ball_seen_head_on_is_at_near_plus_the_distance_and_its_normal_faces_the_camera():
    """one ray through the centre of a float64 ball that sits on a node: the field along it is |z| - r at the nodes and
    linear between them, so the only error is the secant's, and by symmetry the normal is -d exactly"""
    vol = ball((33, 33, 33), (-0.4, -0.4, -0.4), H_BALL, (0, 0, 0), R_BALL)
    cam = RN.basis((0, 0, 2.003), (0, 0, 0), ortho_height=0.5, width=1, height=1)
    near, step = 1.0, 0.5 * H_BALL
    r = RN.render([vol], cam, 1, 1, near, step, 160)
    assert RN.band(r) == 0 and r["steps"][0, 0] >= 0 and r["secant"][0, 0]
    distance = (2.003 - near) - R_BALL                                   # from the near plane to the sphere
    bound = H_BALL ** 2 / (8 * R_BALL) + step ** 2 / (8 * R_BALL)        # trilinear + secant (module test below)
    assert abs(r["depth"][0, 0] - (near + distance)) <= bound
    np.testing.assert_array_equal(r["normal"][0, 0], (-r["d"][0]).astype(np.float32))
    assert r["steps"][0, 0] == int(np.ceil(distance / step))             # the first sample past the surface


def test_depths_of_a_ball_are_within_the_trilinear_and_the_secant_error():
    """Orthographic rays along -z onto a ball of radius r sampled at spacing h.  The interpolant never undercuts a convex
    field and exceeds it by at most h^2 / 8 times the sum of the second derivatives across the ray; the secant through
    two samples `step` apart adds step^2 / 8 times the second derivative along the ray, sin^2 / rho <= 1 / r.  A field
    error E moves the root by E / cos, cos = |d . n| at the hit.
    Rays in the node plane x = 0 (the centre column): the interpolant is bilinear there and the field in that plane is the
    planar distance, whose second derivatives sum to 1 / rho: E = h^2 / (8 r).
    All rays: two curvatures, 2 / rho, over a cell that reaches 2 h inwards: E = 2 h^2 / (8 (r - 2 h))."""
    h, rad, W, Hh = H_BALL, R_BALL, 15, 15
    vol = ball((33, 33, 33), (-0.4, -0.4, -0.4), h, (0, 0, 0), rad)
    cam = RN.basis((0, 0.007, 2.003), (0, 0.007, 0), ortho_height=0.5, width=W, height=Hh)
    near, step = 1.0, 0.5 * h
    r = RN.render([vol], cam, W, Hh, near, step, 160)
    assert RN.band(r) == 0
    o = r["o"].reshape(Hh, W, 3)
    assert (o[:, W // 2, 0] == 0).all()
    rho2 = o[..., 0] ** 2 + o[..., 1] ** 2
    inside = rho2 < rad * rad
    true = np.where(inside, 2.003 - np.sqrt(np.maximum(rad * rad - rho2, 0)), np.inf)
    cos = np.sqrt(np.maximum(rad * rad - rho2, 0)) / rad
    clear = np.abs(np.sqrt(rho2) - rad) > h                              # a silhouette pixel may fall on either side
    np.testing.assert_array_equal((r["steps"] >= 0)[clear], inside[clear])
    m = inside & (cos >= 0.5)
    assert m.sum() > 150 and m[:, W // 2].sum() == 15
    with np.errstate(invalid="ignore"):                                  # inf - inf at the misses, masked out
        err = np.where(m, r["depth"] - true, 0.0)
    print(f"ball: largest depth error x cos, centre column {np.abs(err * cos)[:, W // 2].max():.3e} (bound "
          f"{h * h / (8 * rad) + step * step / (8 * rad):.3e}), all {np.abs(err * cos).max():.3e}")
    assert (err >= -step * step / (8 * rad) / 0.5).all()                 # found deeper, never shallower than the secant's share
    col = np.zeros_like(m)
    col[:, W // 2] = m[:, W // 2]
    assert (np.abs(err * cos)[col] <= h * h / (8 * rad) + step * step / (8 * rad)).all()
    assert (np.abs(err * cos)[m] <= 2 * h * h / (8 * (rad - 2 * h)) + step * step / (8 * rad)).all()
    # the normals: those of the sphere, to the field's error over the half spacing of the difference
    n = r["normal"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        xh = o + r["depth"][..., None] * r["d"].reshape(Hh, W, 3)
    radial = xh / np.linalg.norm(np.where(m[..., None], xh, 1.0), axis=-1, keepdims=True)
    assert np.abs(np.where(m[..., None], n - radial, 0.0)).max() <= 2 * (2 * h * h / (8 * (rad - 2 * h))) / (0.5 * h)


def test_a_box_is_closed_against_its_border():
    """a volume that is negative everywhere shows as its box: a ray from outside hits at its first sample inside the box,
    without a secant (the sample before is +inf), and a ray past the box meets nothing"""
    p = S.nodes((5, 6, 4), (0.1, 0.2, 0.3), 0.25)
    vol = S.shape_of(-(1.0 + p[..., 0] + 2 * p[..., 1]), (0.1, 0.2, 0.3), 0.25)     # box [0.1, 1.1] x [0.2, 1.45] x [0.3, 1.05]
    W, Hh, near, step, K = 12, 10, 0.0, 0.013, 400
    cam = RN.basis((0.63, 0.81, 4.0), (0.63, 0.81, 0.0), ortho_height=2.0, width=W, height=Hh)
    r = RN.render([vol], cam, W, Hh, near, step, K)
    assert RN.band(r) == 0
    o = r["o"].reshape(Hh, W, 3)
    over = (o[..., 0] >= 0.1) & (o[..., 0] <= 1.1) & (o[..., 1] >= 0.2) & (o[..., 1] <= 1.45)
    assert 0 < over.sum() < W * Hh
    np.testing.assert_array_equal(r["steps"] >= 0, over)
    k = int(np.ceil((4.0 - 1.05) / step))                                # the first sample at or below the top face z = 1.05
    assert (r["steps"][over] == k).all() and not r["secant"].any()
    assert (r["depth"][over] == near + k * step).all() and np.isposinf(r["depth"][~over]).all()
    assert (r["shape_id"][over] == 0).all() and (r["shape_id"][~over] == -1).all()
    # the render rule is not seeding's: just outside the box the seeding sample is still negative, the render value +inf
    x = np.array([[0.6, 0.8, 1.05 + 1e-6], [0.6, 0.8, 1.05]])
    v, _ = RN.value(vol, x)
    assert np.isposinf(v[0]) and v[1] < 0 and S.sample(vol[0], vol[1], vol[2], x)[0] < 0


def test_the_first_shape_that_attains_the_minimum_names_the_pixel_and_a_nan_is_passed_over():
    a = S.shape_of(np.full((3, 3, 3), -1.0), (0, 0, 0), 1.0)
    b = S.shape_of(np.full((3, 3, 3), -1.0, np.float32), (0, 0, 0), 1.0)
    c = S.shape_of(np.full((3, 3, 3), np.nan), (0, 0, 0), 1.0)
    x = np.array([[1.0, 1.2, 0.7]])
    assert RN.scene([a, b], x)[1][0] == 0 and RN.scene([c, b, a], x)[1][0] == 1 and RN.scene([c], x)[1][0] == -1
    assert np.isposinf(RN.scene([c], x)[0][0])


def test_bricks_are_minima_over_nine_cubed_nodes_clipped_at_the_end():
    rng = np.random.default_rng(3)
    vol = rng.standard_normal((10, 2, 17)).astype(np.float32)
    b = RN.bricks(vol)
    assert b.shape == (2, 1, 2) and b.dtype == np.float64
    assert b[0, 0, 0] == vol[0:9, :, 0:9].min() and b[1, 0, 1] == vol[8:10, :, 8:17].min() and b[0, 0, 1] == vol[0:9, :, 8:17].min()
    vol[8, 1, 8] = np.nan                                                # a node that all four bricks share
    assert np.isneginf(RN.bricks(vol)).all()
    assert RN.bricks(np.ones((2, 2, 2))).shape == (1, 1, 1) and RN.bricks(np.ones((9, 9, 9))).shape == (1, 1, 1)
    assert RN.bricks(np.ones((10, 9, 18))).shape == (2, 1, 3)


def test_shading_is_lambert_with_a_headlight():
    res = dict(steps=np.array([[3, -1]]), shape_id=np.array([[1, -1]], np.int32), d=np.array([[0, 0, -1.0], [0, 0, -1.0]]),
               normal=np.array([[[0, 0.6, 0.8], [0, 0, 0]]], np.float32))
    rgb = RN.shade(res, [(0, 0, 0), (255, 100, 0)], background=(1, 2, 3))
    lam = float(np.float32(0.8))
    assert rgb.dtype == np.uint8 and rgb.shape == (1, 2, 3)
    assert tuple(rgb[0, 0]) == (int(np.floor(255 * (0.25 + 0.75 * lam) + 0.5)), int(np.floor(100 * (0.25 + 0.75 * lam) + 0.5)), 0)
    assert tuple(rgb[0, 1]) == (1, 2, 3)
    away = RN.shade(res, [(0, 0, 0), (200, 200, 200)], light=(0, 0, -1.0))
    assert tuple(away[0, 0]) == (50, 50, 50)                              # the ambient quarter


# ------------------------------------------------------------------------------------------- mfs.render, host side ----
def test_the_camera_frame_is_orthonormal_and_is_the_oracles():
    from mfs import render
    for kw in (dict(fov=40.0), dict(ortho_height=0.7), dict(fov=75.0, up=(0.1, 1.0, 0.3))):
        cam = render.Camera((0.45, 0.62, 0.55), (0.02, 0.31, -0.01), width=48, height=40, **kw)
        b, o = cam.basis(), RN.basis((0.45, 0.62, 0.55), (0.02, 0.31, -0.01), kw.get("up", (0, 1, 0)), kw.get("fov", 40.0),
                                     kw.get("ortho_height"), 48, 40)
        for k in ("eye", "f", "r", "u"):
            assert b[k].dtype == np.float64 and b[k].tobytes() == o[k].tobytes()
        assert (b["half_w"], b["half_h"], b["ortho"]) == (o["half_w"], o["half_h"], o["ortho"])
        M = np.stack([b["r"], b["u"], b["f"]])
        np.testing.assert_allclose(M @ M.T, np.eye(3), atol=4 * S.EPS64)
        assert np.linalg.det(M) < 0 and b["u"] @ cam.up > 0              # r, u, f: right, up, into the image
        assert b["half_w"] == b["half_h"] * 48 / 40
        assert cam.packed() == [*b["eye"], *b["f"], *b["r"], *b["u"], b["half_w"], b["half_h"]]
    assert render.Camera((0, 0, 1), (0, 0, 0)).basis()["half_h"] == float(np.tan(np.deg2rad(40.0) / 2))


class Vol:
    def __init__(self, phi, origin=(0, 0, 0), spacing=0.1):
        self.phi, self.origin, self.spacing = phi, origin, spacing


def test_refusals_that_need_no_device():
    from mfs import render
    cam = render.Camera((0, 0, 3), (0, 0, 0), width=8, height=8, near=1.0, far=4.0)
    for bad in (dict(width=0), dict(height=16385), dict(fov=0.0), dict(fov=180.0), dict(ortho_height=0.0), dict(near=float("nan")),
                dict(near=2.0, far=2.0), dict(up=(0, 0, 1)), dict(up=(0, 0, 0)), dict(eye=(0, 0, 0)), dict(eye=(float("inf"), 0, 0))):
        kw = dict(eye=(0, 0, 3), target=(0, 0, 0), width=8, height=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            render.Camera(**kw)
    assert render.check_sizes(48, 40, 400) == (1920, 9) and render.check_sizes(1, 1) == (1, 1)
    assert render.check_sizes(16384, 16384, 65536) == (2 ** 28, 2 ** 20)
    for bad in ((0, 4, 1), (4, 16385, 1), (4, 4, 0), (4, 4, 65537)):
        with pytest.raises(ValueError):
            render.check_sizes(*bad)
    cpu = Vol(torch.full((4, 4, 4), -1.0))
    white = [(255, 255, 255)]
    with pytest.raises(TypeError, match="GPU only"):                      # no CPU fallback
        render.Scene(cpu)
    with pytest.raises(TypeError, match="GPU only"):
        render.image([cpu], cam, white)
    with pytest.raises(ValueError, match="1 .. 16"):
        render.Scene([cpu] * 17)
    with pytest.raises(ValueError, match="1 .. 16"):
        render.Scene([])
    # what a host can refuse comes before the device check
    for shapes, kw in (([Vol(torch.zeros(4, 4))], {}), ([Vol(torch.zeros(4, 1, 4))], {}), ([Vol(torch.zeros(4, 4, 4, dtype=torch.float16))], {}),
                       ([Vol(torch.zeros(4, 4, 8)[:, :, ::2])], {}), ([Vol(torch.zeros(4, 4, 4), spacing=0.0)], {}),
                       ([Vol(torch.zeros(4, 4, 4), origin=(0, float("nan"), 0))], {}), ([cpu], dict(step=0.0)),
                       ([cpu], dict(step=3.0 / 65537)), ([cpu], dict(colors=[])), ([cpu], dict(colors=[(0, 0, 256)])),
                       ([cpu, cpu], dict(colors=white))):
        args = dict(colors=white)
        args.update(kw)
        with pytest.raises(ValueError):
            render.image(shapes, cam, **args)
    with pytest.raises(TypeError):
        render.image([Vol(np.zeros((4, 4, 4)))], cam, white)
    with pytest.raises(TypeError, match="Camera"):
        render.image([cpu], None, white)
    listed = render._shapes([cpu], device=False)
    assert render.plan(listed, cam) == (1.0, 4.0, 0.05, 60) and render.plan(listed, cam, 3.0 / 65536)[3] == 65536
    # near and far from the shape's box, one step wider: the box [0, 0.3]^3 seen from (0, 0, 3) down the z axis
    near, far, step, K = render.plan(listed, render.Camera((0, 0, 3), (0, 0, 0), ortho_height=1.0, width=8, height=8))
    assert (near, far) == pytest.approx((2.7 - 0.05, 3.0 + 0.05), abs=1e-12) and K == 8
    near, far, _, _ = render.plan(listed, render.Camera((0, 0, 3), (0, 0, 0), width=8, height=8))
    assert (near, far) == pytest.approx((2.7 - 0.05, float(np.sqrt(0.3 ** 2 + 0.3 ** 2 + 3.0 ** 2)) + 0.05), abs=1e-12)
    assert render.plan(listed, render.Camera((0.1, 0.1, 0.1), (0, 0, 0), width=8, height=8))[0] == 0.0    # an eye inside the box
    with pytest.raises(TypeError, match="RenderResult"):
        render.shade(None, cam, white)


def test_the_slab_classes_do_not_render():
    import notebook_sim as NSIM
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        inst = cls.__new__(cls)                                          # no process group needed to ask
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.render(None)
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.render_result(None)
    assert callable(NSIM.NotebookSimulation.render) and callable(NSIM.NotebookSimulation.render_result)


def test_save_png_round_trips(tmp_path):
    from mfs import render
    rng = np.random.default_rng(5)
    for shape in ((7, 5, 3), (1, 1, 3), (40, 48, 3)):
        rgb = rng.integers(0, 256, shape, dtype=np.uint8)
        path = os.path.join(tmp_path, "a.png")
        render.save_png(path, torch.as_tensor(rgb))
        raw = open(path, "rb").read()
        assert raw[:8] == b"\x89PNG\r\n\x1a\n" and raw[12:16] == b"IHDR" and raw[-8:-4] == b"IEND"
        assert struct.unpack(">IIBBBBB", raw[16:29]) == (shape[1], shape[0], 8, 2, 0, 0, 0)
        assert struct.unpack(">I", raw[29:33])[0] == zlib.crc32(raw[12:29])
        n = struct.unpack(">I", raw[33:37])[0]
        assert raw[37:41] == b"IDAT"
        rows = np.frombuffer(zlib.decompress(raw[41:41 + n]), np.uint8).reshape(shape[0], 1 + 3 * shape[1])
        assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(shape), rgb)
        from PIL import Image
        with Image.open(path) as im:
            assert im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)
        render.save_png(path, rgb)                                       # an array as well
        assert open(path, "rb").read() == raw
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            render.save_png(os.path.join(tmp_path, "b.png"), bad)


# --------------------------------------------------------------------------------------------------------- C ABI ----
def test_new_symbols_are_exported_and_typed(lib):
    from mfs import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfs.h")).read()
    assert all(name + "(" in header for name in NEW) and "#define MFS_ABI_VERSION 3 " in header
    assert lib.mfs_abi_version() == 3


def test_the_c_entry_points_refuse_bad_arguments_before_any_launch(lib):
    """every rejection below returns before a kernel launch or any other device call: this runs on a CPU-only machine"""
    from mfs import _lib
    err = lambda: lib.mfs_last_error()  # noqa: E731
    buf = torch.zeros(64, dtype=torch.int64)                               # host memory: never dereferenced, nothing launches
    p = C.c_void_p(buf.data_ptr())
    e = _lib.i64x
    assert lib.mfs_render_brick_count3d(e((41, 41, 21))) == 75 and lib.mfs_render_brick_count3d(e((10, 2, 17))) == 4
    assert lib.mfs_render_brick_count3d(e((2, 2, 2))) == 1 and lib.mfs_render_brick_count3d(e((9, 10, 18))) == 6
    assert lib.mfs_render_brick_count3d(None) == 0 and lib.mfs_render_brick_count3d(e((2, 1, 2))) == 0
    assert lib.mfs_render_brick_count3d(e((2048, 2048, 512))) == 0
    assert lib.mfs_render_bricks3d(None, 1, e((4, 4, 4)), p, None) == -1 and b"null" in err()
    assert lib.mfs_render_bricks3d(p, 1, None, p, None) == -1 and b"null" in err()
    assert lib.mfs_render_bricks3d(p, 1, e((4, 4, 4)), None, None) == -1 and b"null" in err()
    assert lib.mfs_render_bricks3d(p, 5, e((4, 4, 4)), p, None) == -1 and b"dtype" in err()
    assert lib.mfs_render_bricks3d(p, 1, e((4, 1, 4)), p, None) == -1 and b"extents" in err()

    cam = [0, 0, 3, 0, 0, -1, 1, 0, 0, 0, 1, 0, 0.5, 0.5]

    def shapes(m, extents=(2, 2, 2), spacing=1.0):
        n = max(m, 1)
        ptrs = (C.c_void_p * n)(*([buf.data_ptr()] * n))
        pose = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]
        return [ptrs, (C.c_int * n)(*([1] * n)), e(list(extents) * n), _lib.f64x([0.0] * 3 * n), _lib.f64x([spacing] * n),
                _lib.f64x(pose * n), (C.c_void_p * n)(*([buf.data_ptr()] * n))]

    def march(camera=cam, W=8, H=8, near=0.0, step=0.1, K=10, m=1, sh=None, skip=1, out=(p, p, p, p)):
        sh = shapes(m) if sh is None else sh
        return lib.mfs_render_march3d(None if camera is None else _lib.f64x(camera), 0, W, H, near, step, K, m, *sh, skip, *out,
                                      None, None)

    assert march(camera=None) == -1 and b"null camera" in err()
    for W, H in ((0, 8), (8, 0), (16385, 8), (8, 16385)):
        assert march(W=W, H=H) == -1 and b"16384" in err()
    for K in (0, 65537):
        assert march(K=K) == -1 and b"65536" in err()
    assert march(step=0.0) == -1 and b"step" in err()
    assert march(near=float("inf")) == -1 and b"near" in err()
    assert march(camera=cam[:4] + [float("nan")] + cam[5:]) == -1 and b"finite" in err()
    assert march(camera=cam[:3] + [0, 0, 0] + cam[6:]) == -1 and b"degenerate" in err()
    assert march(camera=cam[:12] + [0.0, 0.5]) == -1 and b"half" in err()
    assert march(m=0) == -1 and b"1 to 16" in err()
    assert march(m=17, sh=shapes(17)) == -1 and b"1 to 16" in err()
    assert march(sh=[None] + shapes(1)[1:]) == -1 and b"null shape description" in err()
    assert march(sh=[(C.c_void_p * 1)(None)] + shapes(1)[1:]) == -1 and b"null shape volume" in err()
    assert march(sh=shapes(1)[:6] + [None]) == -1 and b"null brick" in err()
    assert march(sh=shapes(1)[:6] + [(C.c_void_p * 1)(None)]) == -1 and b"null brick" in err()
    assert march(sh=shapes(1, extents=(2, 1, 2))) == -1 and b"extents" in err()
    assert march(sh=shapes(1, spacing=0.0)) == -1 and b"spacing" in err()
    for k in range(4):
        out = [p, p, p, p]
        out[k] = None
        assert march(out=out) == -1 and b"null output" in err()

    def shade(camera=cam, W=8, H=8, normal=p, ident=p, n=1, albedo=(1.0, 1.0, 1.0), bg=(255, 255, 255), light=None, rgb=p):
        return lib.mfs_render_shade3d(None if camera is None else _lib.f64x(camera), 0, W, H, normal, ident, n,
                                      None if albedo is None else _lib.f64x(albedo * max(n, 1)),
                                      None if bg is None else (C.c_int * 3)(*bg), None if light is None else _lib.f64x(light), rgb, None)

    assert shade(camera=None) == -1 and b"null camera" in err()
    assert shade(W=0) == -1 and b"16384" in err()
    assert shade(normal=None) == -1 and b"null" in err()
    assert shade(ident=None) == -1 and b"null" in err()
    assert shade(rgb=None) == -1 and b"null" in err()
    assert shade(n=0) == -1 and b"colours" in err()
    assert shade(n=17) == -1 and b"colours" in err()
    assert shade(albedo=None) == -1 and b"null" in err()
    assert shade(bg=None) == -1 and b"null" in err()
    assert shade(bg=(0, 256, 0)) == -1 and b"background" in err()
    assert shade(albedo=(1.0, float("nan"), 1.0)) == -1 and b"albedo" in err()
    assert shade(light=(0.0, float("inf"), 0.0)) == -1 and b"light" in err()
