"""The path renderer without a GPU: tests/render_paths_numpy.py on cases with a closed form, the host side of mfs.render's
Material / Look / trace planning (every refusal that needs no device comes before the device check) and the new C entry
points' argument checks, which all return before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import render_numpy as RN
import render_paths_numpy as RP
import seed_numpy as S

NEW = ("mfs_render_bricks_max3d", "mfs_render_paths3d", "mfs_render_resolve3d")
EPS64 = RP.EPS64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    return _lib.load()


class Vol:
    def __init__(self, phi, origin=(0.0, 0.0, 0.0), spacing=0.1):
        self.phi, self.origin, self.spacing = phi, origin, spacing


# ------------------------------------------------------------------------------------------------------ the oracle ----
def test_the_shadow_of_a_ball_on_a_floor_ends_where_geometry_puts_it_within_one_pixel():
    """Orthographic, straight down onto the floor y = 0 (a float64 volume that is y exactly) with a float64 ball of radius r
    above it.  A floor point x is in shadow iff the line x + s l passes the centre closer than r; moving x by one pixel moves
    that distance by at most one pixel, so every floor pixel further than a pixel (plus the ball's trilinear error
    h^2 / (8 r) and the bias, which lifts the shadow ray's origin off the floor) from the edge must be classified exactly."""
    r, centre, hb = 0.1, np.array([0.0, 0.3, 0.0]), 0.0125
    pf = S.nodes((41, 9, 41), (-0.5, -0.1, -0.5), 0.025)
    floor = S.shape_of(pf[..., 1].copy(), (-0.5, -0.1, -0.5), 0.025)
    pb = S.nodes((33, 33, 33), (-0.2, 0.1, -0.2), hb)
    ball = S.shape_of(np.sqrt(((pb - centre) ** 2).sum(axis=-1)) - r, (-0.2, 0.1, -0.2), hb)
    W = H = 45
    px, near, step, K = 0.9 / H, 0.3, 0.005, 160
    cam = RN.basis((0.0031, 1.0017, -0.0047), (0.0031, 0, -0.0047), up=(0, 0, -1), ortho_height=0.9, width=W, height=H)   # off the node planes
    light = RP.unit((0.5, 1.0, 0.2))
    ref = RP.trace([floor, ball], [RP.opaque((200, 200, 200)), RP.opaque((200, 50, 50))], cam, W, H, near, step, K, light=light)
    assert RP.band(ref) == 0
    on_floor = ref["shape_id"][..., 0] == 0
    assert on_floor.sum() > 1500 and (ref["shape_id"][..., 0] == 1).sum() > 50 and (ref["steps"][..., 1:3] == -2).all()
    x = (ref["o"] + 1.0017 * ref["d"]).reshape(H, W, 3)                   # the eye is 1.0017 above the floor
    assert np.abs(x[..., 1]).max() < 1e-12
    to = centre - x
    dist = np.sqrt(np.maximum((to * to).sum(axis=-1) - (to @ light) ** 2, 0.0))
    shadowed = ref["steps"][..., 3] >= 0
    sure = on_floor & (np.abs(dist - r) > px + hb * hb / (8 * r) + 4 * step)
    assert (sure & (dist < r)).sum() > 30 and (on_floor & ~sure).sum() > 10
    np.testing.assert_array_equal(shadowed[sure], (dist < r)[sure])
    lit = sure & ~shadowed                                               # 0.25 + 0.75 n . l on the floor, 0.25 in the shadow
    np.testing.assert_allclose(ref["color"][lit], np.broadcast_to((200 / 255) * (0.25 + 0.75 * light[1]), (lit.sum(), 3)), atol=1e-7)
    np.testing.assert_array_equal(ref["color"][sure & shadowed], np.float64(200 / 255) * 0.25)
    # without shadows no slot 3 runs, and the ball's own far side is the only dark place
    plain = RP.trace([floor, ball], [RP.opaque((200, 200, 200)), RP.opaque((200, 50, 50))], cam, W, H, near, step, K, light=light,
                     shadows=False)
    assert (plain["steps"][..., 3] == -2).all() and np.array_equal(plain["steps"][..., 0], ref["steps"][..., 0])


SLAB = dict(D=0.2, h=0.025, ior=1.33, absorb=(2.0, 1.0, 0.3))


def slab():
    """the liquid between y = -0.1 and y = 0.1 on 41 x 17 x 41 float64 nodes: |y| - 0.1, planes on node planes, so the
    interpolant is the field itself along any ray and the secant is exact: both error terms of DESIGN.md 4.16 vanish and only
    roundings remain"""
    p = S.nodes((41, 17, 41), (-0.5, -0.2, -0.5), SLAB["h"])
    return S.shape_of(np.abs(p[..., 1]) - SLAB["D"] / 2, (-0.5, -0.2, -0.5), SLAB["h"])


def test_a_ray_through_a_flat_slab_leaves_parallel_to_its_entry_displaced_by_the_analytic_amount():
    shape, step = slab(), 0.004
    bias, n_i, D = 4 * step, SLAB["ior"], SLAB["D"]
    d = RP.unit((0.6, -0.7, 0.2))[None]
    o = np.array([[-0.3, 0.45, -0.1]])
    zero, air, all_ = np.zeros(1), np.full(1, -1), np.ones(1, bool)
    s0 = RP.segment([shape], o, d, 0.1, step, 200, air, all_, zero, zero)
    assert s0["steps"][0] > 0 and not s0["band"][0] and abs(s0["x"][0, 1] - D / 2) < 1e-13
    np.testing.assert_allclose(s0["n"][0], (0, 1, 0), atol=1e-13)
    t1, nf, c, k, _, _ = RP.refract(d, s0["n"], np.array([1 / n_i]), zero, zero)
    ci = -d[0, 1]
    sin_t = np.sqrt(1 - ci * ci) / n_i
    cos_t = np.sqrt(1 - sin_t * sin_t)
    assert abs(c[0] - ci) < 1e-13 and abs(-t1[0, 1] - cos_t) < 1e-13     # Snell
    s1 = RP.segment([shape], s0["x"] - bias * nf, t1, 0.0, step, 200, np.zeros(1, int), all_, zero, zero)
    assert s1["id"][0] == 0 and not s1["band"][0]
    tol = 64 * EPS64                                                     # trilinear and secant terms are 0 here (see `slab`)
    assert abs(s1["depth"][0] - (D - bias) / cos_t) <= tol               # the segment starts `bias` below the surface
    np.testing.assert_allclose(s1["n"][0], (0, -1, 0), atol=1e-13)       # outward at the exit
    t2, nf2, c2, k2, _, _ = RP.refract(t1, s1["n"], np.array([n_i]), zero, zero)
    assert k2[0] > 0 and np.abs(t2 - d).max() <= tol                     # parallel to the entry
    # lateral displacement from the incoming line: (D - bias) sin(i - t) / cos t from the segment, bias sin(i) from its start
    moved = s1["x"][0] - s0["x"][0]
    lateral = moved - (moved @ d[0]) * d[0]
    sin_i = np.sqrt(1 - ci * ci)
    want = (D - bias) * (sin_i * cos_t - ci * sin_t) / cos_t + bias * sin_i
    assert abs(np.sqrt(lateral @ lateral) - want) <= tol


def test_the_colour_through_a_slab_is_fresnel_and_beer_lambert():
    """straight down through the slab onto the white background: R = r0 and T = exp(-absorb * (D - bias)); at a slant the
    length is (D - bias) / cos t"""
    shape, step = slab(), 0.0037                                         # no sample falls on a node plane or a face
    bias, n_i, D, a = 4 * step, SLAB["ior"], SLAB["D"], np.array(SLAB["absorb"])
    mats = [RP.liquid((40, 120, 230), n_i, SLAB["absorb"])]
    cam = RN.basis((0.013, 1.0017, 0.021), (0.013, 0, 0.021), up=(0, 0, -1), ortho_height=0.1, width=3, height=3)
    ref = RP.trace([shape], mats, cam, 3, 3, 0.5, step, 200, light=RP.unit((0.3, 2.0, 0.4)))
    r0 = ((n_i - 1) / (n_i + 1)) ** 2
    assert RP.band(ref) == 0 and (ref["shape_id"][..., 1] == 0).all() and (ref["steps"][..., 2] == -1).all()
    np.testing.assert_allclose(ref["length"], D - bias, rtol=0, atol=64 * EPS64)
    np.testing.assert_allclose(ref["color"], np.broadcast_to(r0 + (1 - r0) * np.exp(-a * (D - bias)), (3, 3, 3)), rtol=0, atol=64 * EPS64)
    assert (ref["length_bound"] < 1e-10).all() and (ref["color_bound"] < 1e-9).all()     # the derived bounds stay useful
    tilted = RN.basis((0.4, 1.0, 0.1), (0.0, 0.0, 0.0), ortho_height=0.1, width=2, height=2)
    ref = RP.trace([shape], mats, tilted, 2, 2, 0.5, step, 300, light=RP.unit((0.3, 2.0, 0.4)))
    ci = -tilted["f"][1]
    cos_t = np.sqrt(1 - (1 - ci * ci) / n_i ** 2)
    R = r0 + (1 - r0) * (1 - ci) ** 5
    assert RP.band(ref) == 0
    np.testing.assert_allclose(ref["length"], (D - bias) / cos_t, rtol=0, atol=64 * EPS64)
    np.testing.assert_allclose(ref["color"], np.broadcast_to(R + (1 - R) * np.exp(-a * (D - bias) / cos_t), (2, 2, 3)), rtol=0, atol=1e-13)


def test_brick_maxima_against_a_loop_over_the_nodes():
    rng = np.random.default_rng(4)
    vol = rng.standard_normal((19, 10, 26)).astype(np.float32)
    vol[17, 3, 9] = np.nan
    got = RP.bricks_max(vol)
    assert got.shape == (3, 2, 4) and got.dtype == np.float64
    want = np.full(got.shape, -np.inf)
    for i in range(19):
        for j in range(10):
            for k in range(26):
                for b0 in {min(i // 8, 2), min(max(i - 1, 0) // 8, 2)}:
                    for b1 in {min(j // 8, 1), min(max(j - 1, 0) // 8, 1)}:
                        for b2 in {min(k // 8, 3), min(max(k - 1, 0) // 8, 3)}:          # a node on a brick's face is in both
                            v = np.float64(vol[i, j, k])
                            want[b0, b1, b2] = np.inf if np.isnan(v) else max(want[b0, b1, b2], v)
    assert got.tobytes() == want.tobytes() and np.isposinf(got[2, 0, 1]) and np.isinf(got).sum() == 1
    assert (RP.bricks_max(-vol)[np.isfinite(got)] == -RN.bricks(vol)[np.isfinite(got)]).all()


def test_resolve_is_the_row_major_mean_and_rounds_half_up():
    c = np.zeros((2, 4, 3))
    c[0, 0], c[0, 1], c[1, 0], c[1, 1] = 0.1, 0.2, 0.3, 0.7
    c[:, 2:] = 0.5 / 255                                                 # 255 c + 0.5 = 1 exactly
    out = RP.resolve(c, 2)
    assert out.shape == (1, 2, 3) and out.dtype == np.uint8
    assert out[0, 0, 0] == int(np.floor(255.0 * ((((0.1 + 0.2) + 0.3) + 0.7) / 4.0) + 0.5)) and out[0, 1, 0] == 1
    assert np.array_equal(RP.resolve(np.array([[[np.nan, 2.0, -1.0]]])), np.array([[[0, 255, 0]]], np.uint8))


# ------------------------------------------------------------------------------------------------------- refusals ----
def test_materials_and_looks_refuse_what_a_host_can_refuse():
    from mfs import render
    M, L = render.Material, render.Look
    for bad in (lambda: M.opaque((0, 0, 256)), lambda: M.opaque((0, 0)), lambda: M.liquid((1, 2, 3), ior=1.0),
                lambda: M.liquid((1, 2, 3), ior=4.5), lambda: M.liquid((1, 2, 3), ior=float("nan")),
                lambda: M.liquid((1, 2, 3), absorb=(0, -1, 0)), lambda: M.liquid((1, 2, 3), absorb=(0, float("inf"), 0)),
                lambda: M.liquid((1, 2, 3), absorb=(0, float("nan"), 0))):
        with pytest.raises(ValueError):
            bad()
    one = [M.opaque((1, 2, 3))]
    for kw in (dict(samples=0), dict(samples=5), dict(samples=1.5), dict(bias=-1.0), dict(bias=float("nan")), dict(shadow_steps=0),
               dict(shadow_steps=65537), dict(inside_steps=0), dict(inside_steps=65537), dict(background=(0, 0, 256)),
               dict(background=(0, 0)), dict(light=(0, 0, 0)), dict(light=(0, float("nan"), 1))):
        args = dict(light=None)
        args.update(kw)
        with pytest.raises(ValueError):
            L(one, **args)
    for mats in ([], one * 17, [(1, 2, 3)]):
        with pytest.raises(ValueError):
            L(mats, None)
    w = M.liquid((1, 2, 3))
    assert w.is_liquid and w.ior == 1.33 and not one[0].is_liquid and M.liquid((1, 2, 3), ior=4.0).ior == 4.0
    assert w.packed()[:5] == [1.0, 1 / 255, 2 / 255, 3 / 255, 1.33] and one[0].packed() == [0.0, 1 / 255, 2 / 255, 3 / 255, 0.0, 0.0, 0.0, 0.0]
    look = L([w, one[0]], (0, 3, 4), samples=4, shadow_steps=65536)
    assert np.array_equal(look.light, (0.0, 0.6, 0.8)) and look.shadows and look.samples == 4 and look.bias is None
    water = L.water()
    assert water.materials[0].is_liquid and not water.materials[1].is_liquid and water.samples == 2 and water.shadows


def test_trace_planning_refuses_before_the_device_check():
    from mfs import render
    M, L = render.Material, render.Look
    cam = render.Camera((0, 0, 3), (0, 0, 0), width=8, height=8, near=1.0, far=4.0)
    cpu = Vol(torch.full((4, 4, 4), -1.0))
    look = L([M.liquid((1, 2, 3))], None)
    with pytest.raises(TypeError, match="GPU only"):                      # no CPU fallback
        render.image_paths([cpu], cam, look)
    wide = render.Camera((0, 0, 3), (0, 0, 0), width=5000, height=8, near=1.0, far=4.0)
    for shapes, camera, lk, kw in (([cpu, cpu], cam, look, {}), ([cpu], cam, L([M.opaque((1, 2, 3))] * 2, None), {}),
                                   ([cpu], wide, L([M.opaque((1, 2, 3))], None, samples=4), {}), ([cpu], cam, look, dict(step=0.0)),
                                   ([cpu], cam, look, dict(step=3.0 / 65537)), ([Vol(torch.zeros(4, 1, 4))], cam, look, {}),
                                   ([cpu] * 17, cam, look, {})):
        with pytest.raises(ValueError):
            render.image_paths(shapes, camera, lk, **kw)
    with pytest.raises(TypeError, match="Look"):
        render.image_paths([cpu], cam, "water")
    with pytest.raises(TypeError, match="Camera"):
        render.image_paths([cpu], None, look)
    with pytest.raises(TypeError, match="PathResult"):
        render.resolve(None)
    listed = render._shapes([cpu], device=False)
    assert render.plan_paths(listed, cam, look) == (1.0, 4.0, 0.05, 60, 0.2, 60, 60)
    assert render.plan_paths(listed, cam, L(look.materials, None, bias=0.0, shadow_steps=7, inside_steps=9), 0.1)[4:] == (0.0, 7, 9)
    assert render.plan_paths(listed, render.Camera((0, 0, 3), (0, 0, 0), width=4096, height=8, near=1.0, far=4.0),
                             L(look.materials, None, samples=4))[3] == 60  # 16384 sub-pixel columns: the limit itself
    with pytest.raises(ValueError, match="water"):
        render.simulation_look(("liquid", "solid"), "wine")
    assert render.simulation_look(("solid", "liquid"), "water").materials[1].is_liquid


def test_the_slab_classes_take_the_keyword_and_still_do_not_render():
    import notebook_sim as NSIM
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        inst = cls.__new__(cls)
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.render(None, look="water")


# --------------------------------------------------------------------------------------------------------- C ABI ----
def test_new_symbols_are_exported_and_typed(lib):
    import os
    from mfs import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mfs.h")).read()
    assert all(name + "(" in header for name in NEW) and lib.mfs_abi_version() == 3


def test_the_new_entry_points_refuse_bad_arguments_before_any_launch(lib):
    from mfs import _lib
    err = lambda: lib.mfs_last_error()  # noqa: E731
    p = C.c_void_p(64)                                                   # never dereferenced: every call below returns first
    e = _lib.i64x
    assert lib.mfs_render_bricks_max3d(None, 1, e((4, 4, 4)), p, None) == -1 and b"null" in err()
    assert lib.mfs_render_bricks_max3d(p, 5, e((4, 4, 4)), p, None) == -1 and b"dtype" in err()
    assert lib.mfs_render_bricks_max3d(p, 1, e((4, 1, 4)), p, None) == -1 and b"extents" in err()
    assert lib.mfs_render_resolve3d(None, 4, 4, 1, p, None) == -1 and b"null" in err()
    assert lib.mfs_render_resolve3d(p, 4, 4, 0, p, None) == -1 and b"samples" in err()
    assert lib.mfs_render_resolve3d(p, 4, 4, 5, p, None) == -1 and b"samples" in err()
    assert lib.mfs_render_resolve3d(p, 8192, 4, 4, p, None) == -1 and b"extents" in err()
    camera = [0, 0, 3, 0, 0, -1, 1, 0, 0, 0, 1, 0, 0.5, 0.5]

    def paths(mat=(1, 0.1, 0.2, 0.3, 1.33, 1, 1, 1), bias=0.1, ks=10, ki=10, skip=0, out=(p, p, p, p), bg=(255, 255, 255),
              light=(0, 1, 0), grids=None, tops=None, W=4):
        ptr = (C.c_void_p * 1)(64)
        return lib.mfs_render_paths3d(_lib.f64x(camera), 0, W, 4, 1.0, 0.1, 10, 1, ptr, (C.c_int * 1)(1), e((4, 4, 4)),
                                      _lib.f64x((0, 0, 0)), _lib.f64x((0.1,)), _lib.f64x((1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0)),
                                      grids, tops, skip, None if mat is None else _lib.f64x(mat),
                                      None if light is None else _lib.f64x(light), (C.c_int * 3)(*bg), 1, bias, ks, ki, *out, None, None)

    for kw, word in ((dict(mat=None), b"null"), (dict(mat=(2, 0, 0, 0, 1.33, 0, 0, 0)), b"kind"), (dict(mat=(1, 0, 0, 0, 1.0, 0, 0, 0)), b"ior"),
                     (dict(mat=(1, 0, 0, 0, 4.5, 0, 0, 0)), b"ior"), (dict(mat=(1, 0, 0, 0, 1.33, 0, -1, 0)), b"absorb"),
                     (dict(mat=(0, float("nan"), 0, 0, 0, 0, 0, 0)), b"albedo"), (dict(bias=-1.0), b"bias"), (dict(bias=float("nan")), b"bias"),
                     (dict(ks=0), b"steps"), (dict(ki=65537), b"steps"), (dict(skip=1), b"brick"), (dict(out=(p, None, p, p)), b"null output"),
                     (dict(bg=(0, 256, 0)), b"background"), (dict(light=(0, float("inf"), 0)), b"light"), (dict(W=16385), b"extents")):
        assert paths(**kw) == -1 and word in err(), (kw, err())
    one = (C.c_void_p * 1)(64)
    none = (C.c_void_p * 1)(None)
    assert paths(skip=1, grids=one, tops=none) == -1 and b"brick" in err()    # a liquid needs its maxima
