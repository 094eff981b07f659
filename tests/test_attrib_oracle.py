"""mfs.attrib without a GPU: the oracle (tests/attrib_numpy.py) against closed forms; the float32 restatement of the
kernel inside the derived bound on every case the GPU tests use, the band empty there, and two mutants outside the bound
(so the bound is neither violated by correct code nor vacuous); the colormap, `hit_points` against the oracle's rays, and
every argument error that needs no device.

Measured here when the tests were written (printed by every run): on the cloud the restatement reaches 0.20 of the bound
at worst (median 0.012), 0.17 on the other cases; the bound is 7e-6 of |A| at the median; the t^2 mutant exceeds it at
93 % of the covered queries, the dropped bin at 42 %."""
import functools
import os

import numpy as np
import pytest
import torch

import attrib_numpy as A
import render_numpy as RN

U32 = A.U32


@functools.lru_cache(maxsize=None)
def reference(name):
    px, vals, q, R, box = A.CASES[name]()
    ref = A.gather(px, vals, q, R, box)
    for a in (px, vals, q, ref["A"], ref["K"], ref["W"], ref["bound"]):
        a.setflags(write=False)
    return px, vals, q, R, box, ref


# ------------------------------------------------------------------------------------------------- closed forms ----
def test_one_particle_gives_its_value_everywhere_inside_R():
    rng = np.random.default_rng(0)
    x = np.array([[0.3, -0.2, 0.7]])
    d = rng.standard_normal((200, 3))
    d *= (rng.random(200) * 1.4 / np.sqrt((d * d).sum(axis=1)))[:, None]
    ref = A.gather(x, np.array([[2.5, -1.0]]), x + 0.2 * d, 0.2)
    inside = (d * d).sum(axis=1) < 1.0 - 1e-9
    assert inside.sum() > 50 and (~inside).sum() > 50
    np.testing.assert_array_equal(ref["K"], inside.astype(int))
    np.testing.assert_allclose(ref["A"][inside], np.tile([2.5, -1.0], (inside.sum(), 1)), rtol=1e-15)
    assert np.isnan(ref["A"][~inside]).all() and (ref["W"][~inside] == 0).all()
    assert (A.gather(x, [[2.5]], x + 0.2 * d, 0.2, fill=-7.0)["A"][~inside] == -7.0).all()


def test_two_particles_give_the_mean_at_the_midpoint():
    x = np.array([[0.0, 0.0, 0.0], [0.25, 0.5, 0.125]])
    ref = A.gather(x, np.array([1.0, 4.0]), x.mean(axis=0)[None], 0.5)
    assert ref["K"][0] == 2 and ref["A"][0, 0] == 2.5


def test_linear_values_on_a_point_symmetric_cluster_give_the_linear_value_at_the_centre():
    rng = np.random.default_rng(1)
    half = 0.1 * rng.standard_normal((40, 3))
    c = np.array([1.0, 2.0, 0.5])
    x = np.concatenate([c + half, c - half])
    vals = np.round((3.0 * x[:, 0] - 2.0 * x[:, 1] + 0.5 * x[:, 2] + 1.0) * 2 ** 20) / 2 ** 20   # float32 holds these exactly
    ref = A.gather(x, vals, c[None], 0.3)
    assert ref["K"][0] > 40
    assert abs(ref["A"][0, 0] - (3.0 * c[0] - 2.0 * c[1] + 0.5 * c[2] + 1.0)) < 2e-6


def test_a_constant_is_reproduced_by_the_float32_restatement():
    px, _, q, R, box, ref = reference("cloud")
    got, W = A.gather32(px, np.ones(len(px)), q, R, box)
    cov = ref["K"] > 0
    assert cov.sum() > 1000 and ((W > 0) == cov).all()
    assert (np.abs(got[cov, 0].astype(np.float64) - 1.0) <= 2.0 * (ref["K"][cov] + 1) * U32).all()


def test_a_particle_exactly_R_away_does_not_contribute():
    px, vals, q, R, box, ref = reference("exactly_R")
    np.testing.assert_array_equal(ref["K"], [0, 1, 2, 0, 0, 1])
    np.testing.assert_array_equal(ref["A"][1], vals[0])
    np.testing.assert_array_equal(ref["A"][2], 0.5 * (vals[1] + vals[2]))
    np.testing.assert_array_equal(ref["A"][5], vals[3])
    got, W = A.gather32(px, vals, q, R, box)                             # dyadic: float32 is exact here
    np.testing.assert_array_equal(W > 0, ref["K"] > 0)
    np.testing.assert_array_equal(got[ref["K"] > 0], ref["A"][ref["K"] > 0])


def test_non_finite_particles_queries_and_values():
    px, vals, q, R, box, ref = reference("non_finite")
    assert (ref["K"][[3, 8, 11]] == 0).all() and np.isnan(ref["A"][[3, 8, 11]]).all()
    t = ref["t"]
    assert (t[:, [5, 17, 900]] == -np.inf).all()                        # particles that are not finite add nothing
    hit = np.flatnonzero(t[:, 100] > 0)
    assert len(hit) and np.isnan(ref["A"][hit, 0]).all() and np.isfinite(ref["A"][hit, 3]).all()
    miss = (t[:, 100] <= 0) & (ref["K"] > 0)
    assert np.isfinite(ref["A"][miss, 0]).all()                          # a NaN out of reach does not propagate
    assert np.isinf(ref["A"][t[:, 200] > 0, 1]).all()


def test_lattice_rule():
    o, m = A.lattice(([1.0, 2.0, 0.5], [1.0, 2.0, 0.5]), 0.125)
    assert m == (3, 3, 3) and (o == [0.875, 1.875, 0.375]).all()
    o, m = A.lattice(([0.0, 0.0, 0.0], [1.0, 0.99, 0.26]), 0.25)
    assert m == (7, 6, 4)
    from mfs import attrib
    assert attrib.lattice(([0.0, 0.0, 0.0], [1.0, 0.99, 0.26]), 0.25) == ((-0.25, -0.25, -0.25), (7, 6, 4))


# --------------------------------------------------------------------------- the bound, the band and the mutants ----
@pytest.mark.parametrize("name", sorted(A.CASES))
def test_the_float32_restatement_stays_inside_the_bound_and_the_band_is_empty(name):
    px, vals, q, R, box, ref = reference(name)
    if name != "exactly_R":                                              # t == 0 there on purpose; float32 is exact on it
        assert not ref["band"].any(), (name, int(ref["band"].sum()), ref["eps"])
    for C in (1, 3, 4):
        got, W = A.gather32(px, vals[:, :C], q, R, box)
        np.testing.assert_array_equal(W > 0, ref["K"] > 0)
        ex = A.excess(got, dict(ref, A=ref["A"][:, :C], bound=ref["bound"][:, :C]))
        cov = ref["K"] > 0
        print(f"{name} C={C}: {cov.sum()} of {len(q)} covered, K up to {ref['K'].max()}, error / bound max {ex.max():.3f} "
              f"median {np.median(ex[cov]) if cov.any() else 0:.3f}")
        assert ex.max() <= 1.0
        assert np.isnan(got[~cov]).all()
        rel = W[cov].astype(np.float64) / ref["W"][cov] - 1.0
        assert (np.abs(rel) <= (ref["K"][cov] + 64) * U32 + 60 * U32 * (np.where(ref["t"][cov] > 0, ref["t"][cov] ** 2, 0).sum(axis=1)
                                                                      / ref["W"][cov])).all()


@pytest.mark.parametrize("mutant,least", [("t2", 0.5), ("drop_bin", 0.1)])
def test_the_mutants_exceed_the_bound(mutant, least):
    px, vals, q, R, box, ref = reference("cloud")
    got, W = A.gather32(px, vals, q, R, box, mutant=mutant)
    cov = ref["K"] > 0
    over = (A.excess(got, ref)[cov] > 1.0).any(axis=1) | ~(W[cov] > 0)
    print(f"{mutant}: beyond the bound at {over.mean():.1%} of {cov.sum()} covered queries")
    assert over.mean() >= least


def test_the_bound_is_small():
    _, _, _, _, _, ref = reference("cloud")
    cov = ref["K"] > 0
    rel = ref["bound"][cov, 0] / np.abs(ref["A"][cov, 0])
    print(f"bound / |A|, channel 0: median {np.median(rel):.2e}, max {rel.max():.2e}; K up to {ref['K'].max()}")
    assert np.median(rel) < 1e-5 and ref["K"].max() >= 70


# ---------------------------------------------------------------------------------------------------- colormap ----
def test_colormap_at_and_between_stops_clamps_and_keeps_nan():
    from mfs import render
    cm = render.Colormap([(0.0, (0, 0, 0)), (0.5, (255, 0, 51)), (1.0, (255, 255, 51))])
    v = torch.tensor([2.0, 3.0, 4.0, 2.5, 3.5, 1.0, 9.0, float("nan")], dtype=torch.float32)
    c = cm.apply(v, 2.0, 4.0).numpy()
    assert c.dtype == np.float32 and c.shape == (8, 3)
    f = lambda *a: np.asarray(a, np.float32) / np.float32(255)  # noqa: E731
    np.testing.assert_array_equal(c[0], f(0, 0, 0))
    np.testing.assert_array_equal(c[1], f(255, 0, 51))
    np.testing.assert_array_equal(c[2], f(255, 255, 51))
    np.testing.assert_allclose(c[3], f(127.5, 0, 25.5), rtol=2e-7)
    np.testing.assert_allclose(c[4], f(255, 127.5, 51), rtol=2e-7)
    np.testing.assert_array_equal(c[5], c[0])                            # clamped below
    np.testing.assert_array_equal(c[6], c[2])                            # and above
    assert np.isnan(c[7]).all()
    grey = render.Colormap("speed", nan_color=(10, 20, 30)).apply(v.reshape(2, 4), 0.0, 1.0).numpy()
    assert grey.shape == (2, 4, 3)
    np.testing.assert_array_equal(grey[1, 3], f(10, 20, 30))
    assert cm.slope() == 2.0
    speed = render.Colormap("speed")
    assert speed.colors[0] == tuple(float(v) for v in render.LIQUID_COLOR) and speed.colors[-1] == (255.0, 255.0, 255.0)
    for name in ("speed", "heat", "diverging"):
        out = render.Colormap(name).apply(torch.linspace(-0.5, 1.5, 41), 0.0, 1.0)
        assert bool(((out >= 0) & (out <= 1)).all())


def test_colormap_argument_errors():
    from mfs import render
    for bad in ("rainbow", [(0.0, (0, 0, 0))], [(0.1, (0, 0, 0)), (1.0, (1, 1, 1))], [(0.0, (0, 0, 0)), (0.0, (1, 1, 1)), (1.0, (2, 2, 2))],
                [(0.0, (0, 0, 0)), (1.0, (256, 0, 0))], [(0.0, (0, 0)), (1.0, (1, 1))]):
        with pytest.raises(ValueError, match="colormap"):
            render.Colormap(bad)
    with pytest.raises(ValueError, match="nan_color"):
        render.Colormap("heat", nan_color=(0, 0, 300))
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="range"):
            render.Colormap("heat").apply(torch.zeros(3), lo, hi)
    with pytest.raises(TypeError, match="tensor"):
        render.Colormap("heat").apply(np.zeros(3), 0.0, 1.0)


# -------------------------------------------------------------------------------------------------- hit points ----
@pytest.mark.parametrize("ortho", [False, True])
def test_hit_points_follow_the_oracles_rays(ortho):
    from mfs import render
    W, H = 13, 9
    kw = dict(ortho_height=1.3) if ortho else dict(fov=35.0)
    cam = render.Camera((0.9, 0.8, 1.1), (0.1, 0.3, -0.2), width=W, height=H, **kw)
    rng = np.random.default_rng(3)
    depth = 0.5 + rng.random((H, W))
    steps = rng.integers(-1, 3, (H, W)).astype(np.int32)
    depth[steps < 0] = np.inf
    res = render.RenderResult(torch.tensor(depth), torch.zeros((H, W, 3), dtype=torch.float32), torch.tensor(np.minimum(steps, 0)),
                              torch.tensor(steps), 0.0, 1.0, 0.1, 10, 1)
    pts = render.hit_points(res, cam).numpy()
    assert pts.shape == (H, W, 3) and pts.dtype == np.float64
    o, d = RN.rays(RN.basis(cam.eye, cam.target, cam.up, cam.fov, cam.ortho_height, W, H), W, H)
    want = (o + np.where(steps < 0, 0.0, depth).reshape(-1, 1) * d).reshape(H, W, 3)
    hit = steps >= 0
    assert hit.any() and (~hit).any()
    np.testing.assert_array_equal(pts[hit], want[hit])
    assert np.isnan(pts[~hit]).all()
    with pytest.raises(ValueError, match="camera is"):
        render.hit_points(res, render.Camera((0.9, 0.8, 1.1), (0.1, 0.3, -0.2), width=W + 1, height=H))
    with pytest.raises(TypeError, match="RenderResult"):
        render.hit_points(None, cam)


# --------------------------------------------------------------------------------------------- argument errors ----
def test_gather_argument_errors_need_no_device():
    from mfs import attrib
    px, q = torch.zeros((5, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float32)
    vals = torch.zeros(5)
    for kw, match in ((dict(influence=0.0), "influence"), (dict(influence=float("nan")), "influence"),
                      (dict(influence=float("inf")), "influence"), (dict(influence=None), "influence"),
                      (dict(box=((0, 0, 0), (1, float("inf"), 1))), "box"), (dict(box=((0, 0, 0), (1, -1, 1))), "box"),
                      (dict(box=(0, 1, 2)), "box"),
                      (dict(box=((0, 0, 0), (1e4, 1e4, 1e4)), influence=1.0), "2\\^31 - 2"),
                      (dict(px=torch.zeros((5, 2))), "px"), (dict(px=torch.zeros((5, 3), dtype=torch.float16)), "px"),
                      (dict(px=torch.zeros((3, 5), dtype=torch.float64).T), "px"),
                      (dict(points=torch.zeros(4)), "points"), (dict(points=torch.zeros((4, 3), dtype=torch.int32)), "points"),
                      (dict(values=torch.zeros(4)), "values"), (dict(values=torch.zeros((5, 5))), "channels"),
                      (dict(values=torch.zeros((5, 0))), "channels"), (dict(values=torch.zeros((5, 2, 1))), "values"),
                      (dict(values=torch.zeros(5, dtype=torch.int64)), "values")):
        args = dict(dict(points=q, px=px, values=vals, influence=0.1), **kw)
        with pytest.raises(ValueError, match=match):
            attrib.gather(**args)
    for kw in (dict(points=np.zeros((4, 3))), dict(px=np.zeros((5, 3))), dict(values=np.zeros(5))):
        with pytest.raises(TypeError, match="torch tensor"):
            attrib.gather(**dict(dict(points=q, px=px, values=vals, influence=0.1), **kw))
    with pytest.raises(TypeError, match="no CPU fallback"):             # everything else is fine: the device is refused last
        attrib.gather(q, px, vals, 0.1)
    with pytest.raises(TypeError, match="no CPU fallback"):
        attrib.bins(px, 0.1, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="2\\^31 - 2"):
        attrib.bins(px, 1e-4, ((0, 0, 0), (1, 1, 1)))
    with pytest.raises(ValueError, match="influence"):
        attrib.bins(px, -1.0, ((0, 0, 0), (1, 1, 1)))


def test_the_c_entry_points_refuse_before_any_launch():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    lib = _lib.load()
    g, o, one = _lib.i64x((3, 3, 3)), _lib.f64x((0.0, 0.0, 0.0)), 1
    assert lib.mfs_attrib_bins3d(g) == 27 and lib.mfs_attrib_bins3d(None) == 0
    assert lib.mfs_attrib_bins3d(_lib.i64x((0, 3, 3))) == 0 and lib.mfs_attrib_bins3d(_lib.i64x((2048, 2048, 512))) == 0
    assert lib.mfs_attrib_bins3d(_lib.i64x((2 ** 31 - 2, 1, 1))) == 2 ** 31 - 2
    refusals = [
        (lib.mfs_attrib_keys3d, (None, o, 0.1, None, one, 1, 4, one, None), b"null"),
        (lib.mfs_attrib_keys3d, (g, o, 0.1, None, None, 1, 4, one, None), b"null"),
        (lib.mfs_attrib_keys3d, (g, o, 0.1, None, one, 1, 4, None, None), b"null"),
        (lib.mfs_attrib_keys3d, (g, o, 0.0, None, one, 1, 4, one, None), b"influence"),
        (lib.mfs_attrib_keys3d, (g, o, float("inf"), None, one, 1, 4, one, None), b"influence"),
        (lib.mfs_attrib_keys3d, (g, o, float("nan"), None, one, 1, 4, one, None), b"influence"),
        (lib.mfs_attrib_keys3d, (_lib.i64x((2048, 2048, 512)), o, 0.1, None, one, 1, 4, one, None), b"2^31 - 2"),
        (lib.mfs_attrib_keys3d, (_lib.i64x((3, 0, 3)), o, 0.1, None, one, 1, 4, one, None), b"bins per axis"),
        (lib.mfs_attrib_keys3d, (g, o, 0.1, None, one, 1, 2 ** 31, one, None), b"2^31"),
        (lib.mfs_attrib_keys3d, (g, o, 0.1, None, one, 7, 4, one, None), b"dtype"),
        (lib.mfs_attrib_keys3d, (g, o, 0.1, _lib.f64x((0, 0, 0, 1, float("nan"), 1)), one, 1, 4, one, None), b"box"),
    ]
    ok = (g, o, 0.1, 1, 0.0, one, 1, one, 1, 4, one, one, 1, one, 4, one, 1, one, one, None, None)

    def but(**kw):
        names = ["shape", "origin", "influence", "channels", "fill", "ps", "pdt", "vs", "vdt", "P", "starts", "qs", "qdt", "rows",
                 "Q", "items", "n", "values", "weight", "tested", "stream"]
        return tuple(kw.get(n, v) for n, v in zip(names, ok))
    refusals += [(lib.mfs_attrib_gather3d, but(**kw), msg) for kw, msg in (
        (dict(shape=None), b"null"), (dict(influence=-1.0), b"influence"), (dict(channels=0), b"channels"),
        (dict(channels=5), b"channels"), (dict(ps=None), b"null"), (dict(vs=None), b"null"), (dict(starts=None), b"null"),
        (dict(qs=None), b"null"), (dict(rows=None), b"null"), (dict(items=None), b"null"), (dict(values=None), b"null"),
        (dict(weight=None), b"null"), (dict(P=2 ** 31), b"2^31"), (dict(Q=2 ** 31), b"2^31"), (dict(n=5), b"work item"),
        (dict(n=-1), b"work item"), (dict(vdt=9), b"dtype"), (dict(shape=_lib.i64x((2 ** 20, 2 ** 20, 2))), b"2^31 - 2"))]
    cam = _lib.f64x([0, 0, 1, 0, 0, -1, 1, 0, 0, 0, 1, 0, 0.5, 0.5])
    import ctypes
    bg, pal = (ctypes.c_int * 3)(255, 255, 255), _lib.f64x((0.5, 0.5, 0.5))
    shade_ok = (cam, 0, 4, 4, one, one, 1, pal, bg, None, one, 0, one, None)
    for k, v, msg in ((4, None, b"null"), (5, None, b"null"), (10, None, b"null"), (12, None, b"null"), (11, 1, b"albedo_id"),
                      (11, -1, b"albedo_id"), (6, 17, b"colours"), (2, 0, b"extents"), (0, None, b"null")):
        refusals.append((lib.mfs_render_shade_albedo3d, shade_ok[:k] + (v,) + shade_ok[k + 1:], msg))
    for fn, args, msg in refusals:
        assert fn(*args) == -1, (fn.__name__, args)
        assert msg in lib.mfs_last_error(), (fn.__name__, msg, lib.mfs_last_error())


def test_render_keywords_are_refused_without_a_device():
    import notebook_sim as NSIM
    import notebook_sim2d as NSIM2
    sim = NSIM.NotebookSimulation.__new__(NSIM.NotebookSimulation)
    with pytest.raises(ValueError, match="color_by and look"):
        sim.render(None, color_by="speed", look="water")
    with pytest.raises(ValueError, match="liquid"):
        sim.render(None, what="solid", color_by="speed")
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        inst = cls.__new__(cls)
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.render(None, color_by="speed", color_range=(0, 1), colormap="heat")
        with pytest.raises(NotImplementedError, match="single-GPU"):
            inst.sample_particles(None, values="speed")
    flat = NSIM2.NotebookSimulation2D.__new__(NSIM2.NotebookSimulation2D)
    with pytest.raises(NotImplementedError, match="3D"):
        flat.render(None, color_by="speed")
    with pytest.raises(NotImplementedError, match="3D"):
        flat.sample_particles(None)


def test_save_obj_writes_coloured_vertices_that_read_obj_reads(tmp_path):
    from mfs import attrib, surface
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0], [0.25, 0.125, 2.0]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    colors = torch.tensor([[1.0, 0.0, 0.0], [0.0, 0.5, 0.0], [0.25, 0.25, 1.0], [float("nan"), 0.0, 0.0]])
    path = os.path.join(tmp_path, "c.obj")
    attrib.save_obj(path, surface.Mesh(v, f, None), colors)
    rv, rf = surface.read_obj(path)
    np.testing.assert_array_equal(rv, v.numpy())
    np.testing.assert_array_equal(rf, f.numpy())
    rows = [ln.split() for ln in open(path) if ln.startswith("v ")]
    assert all(len(r) == 7 for r in rows) and [float(c) for c in rows[2][4:]] == [0.25, 0.25, 1.0] and float(rows[3][4]) == 0.0
    with pytest.raises(ValueError, match="colors"):
        attrib.save_obj(path, surface.Mesh(v, f, None), colors[:3])
