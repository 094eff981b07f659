"""DensityCGSolver2D and sdf2D without a GPU: the numpy restatement (tests/density2d_numpy.py) against the goldens that
the reference's own source wrote (tests/golden/make_goldens_density2d.py), the edge cases the goldens must hold, the new
entry points in header / library / ctypes table, and the argument checks, which refuse bad calls before anything
touches a device.  Tolerances are those of tests/test_density_gpu.py / tests/test_sdf_gpu.py for the 3D twins."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import density2d_numpy as D
from conftest import REPO, golden, golden_names

DNAMES = golden_names("d2d_")
SNAMES = golden_names("sdf2d_")


def _geo(g):
    gres = tuple(int(v) for v in g["gres"])
    return gres, np.asarray(g["bound_size"], np.float64) / np.asarray(gres, np.float64)


def test_goldens_exist():
    assert DNAMES == ["d2d_a_44", "d2d_b_40x28_f32", "d2d_c_33x21_maxiter6"]
    assert SNAMES == ["sdf2d_a_f64", "sdf2d_b_f32"]
    for n in DNAMES + SNAMES:
        assert os.path.getsize(os.path.join(REPO, "tests", "golden", n + ".npz")) <= 257457, n


@pytest.mark.parametrize("name", DNAMES)
def test_numpy_kernels_match_golden(name):
    g = golden(name)
    gres, cs = _geo(g)
    fx, fy = (gres[0] + 1, gres[1]), (gres[0], gres[1] + 1)
    wx, wy = np.full(fx, 7.0), np.full(fy, 7.0)
    D.solid_frac(gres, g["sphi"], wx, wy)
    # compute_solid_frac writes cells x < Nx-1, y < Ny-1 (both faces per axis); everything else keeps the prefill here
    # and the constructor's 0 in the golden
    mx, my = np.zeros(fx, bool), np.zeros(fy, bool)
    mx[:gres[0], :gres[1] - 1], my[:gres[0] - 1, :gres[1]] = True, True
    np.testing.assert_allclose(wx[mx], g["wx"][mx], rtol=1e-12, atol=0)
    np.testing.assert_allclose(wy[my], g["wy"][my], rtol=1e-12, atol=0)
    assert (wx[~mx] == 7.0).all() and (wy[~my] == 7.0).all() and not g["wx"][~mx].any() and not g["wy"][~my].any()
    gm = np.zeros(gres)
    D.splat(g["bound_min"], cs, gres, g["px"], g["pm"], gm)
    np.testing.assert_allclose(gm, g["gm"], rtol=0, atol=1e-11 * np.abs(g["gm"]).max())
    gvol = np.full(gres, 7.0)
    D.fix_volume(cs, gres, g["lvol"], gvol, g["sphi"], g["lphi"], g["wx"], g["wy"])
    np.testing.assert_allclose(gvol, g["gvol"], rtol=1e-13, atol=0)
    b = np.full(gres, 7.0)
    D.rhs(float(g["rho0"]), float(g["dt"]), gres, cs, g["gm"], g["gvol"], g["lphi"], g["wx"], g["wy"], b)
    np.testing.assert_allclose(b, g["b"], rtol=1e-12, atol=1e-12 * np.abs(g["b"][1:-1, 1:-1]).max())
    qr = np.full(gres, 7.0)
    D.apply(gres, g["rv"], qr, g["wx"], g["wy"], g["lphi"])
    np.testing.assert_allclose(qr, g["qr"], rtol=1e-12, atol=1e-12)
    dx, dy = np.full(fx, 7.0), np.full(fy, 7.0)
    D.displacement(gres, float(g["dt"]), cs, dx, dy, g["x"], g["lphi"])
    for a, k in ((dx, "dx"), (dy, "dy")):
        w = g[k] != 7.0
        np.testing.assert_array_equal(a == 7.0, ~w)
        np.testing.assert_allclose(a[w], g[k][w], rtol=1e-12, atol=1e-12 * np.abs(g[k][w]).max())
    # what the reference never writes kept the 7.0 prefill, in the golden and here
    for a in (g["gvol"], g["b"], g["qr"], gvol, b, qr):
        assert (a[0] == 7).all() and (a[-1] == 7).all() and (a[:, 0] == 7).all() and (a[:, -1] == 7).all()
        assert (a[1:-1, 1:-1] != 7).all()
    # displacement: [1:Nx, 1:Ny] of both arrays, the last cell included, nothing else
    Nx, Ny = gres
    for a in (g["dx"], dx):
        assert (a[0] == 7).all() and (a[Nx] == 7).all() and (a[:, 0] == 7).all() and (a[1:Nx, 1:] != 7).all()
    for a in (g["dy"], dy):
        assert (a[0] == 7).all() and (a[:, 0] == 7).all() and (a[:, Ny] == 7).all() and (a[1:, 1:Ny] != 7).all()


@pytest.mark.parametrize("name", DNAMES)
def test_numpy_gather_matches_golden(name):
    """the two gathers on the golden's displacements (zeros where the reference never writes: the solver's own arrays),
    x first, then y at the moved positions"""
    g = golden(name)
    gres, cs = _geo(g)
    dx, dy = np.where(g["dx"] == 7.0, 0.0, g["dx"]), np.where(g["dy"] == 7.0, 0.0, g["dy"])
    px = g["px"].copy()
    D.advect(px, dx, g["bound_min"], cs, (0, 0.5), 0)
    D.advect(px, dy, g["bound_min"], cs, (0.5, 0), 1)
    assert px.dtype == g["out_px"].dtype
    if px.dtype == np.float64:
        np.testing.assert_allclose(px, g["out_px"], rtol=0, atol=1e-15)
    else:
        np.testing.assert_array_equal(px, g["out_px"])
    # y-then-x order gives other positions: the order is pinned by the golden
    py = g["px"].copy()
    D.advect(py, dy, g["bound_min"], cs, (0.5, 0), 1)
    D.advect(py, dx, g["bound_min"], cs, (0, 0.5), 0)
    assert not np.array_equal(py, g["out_px"])


@pytest.mark.parametrize("name", DNAMES)
def test_numpy_solve_matches_golden(name):
    g = golden(name)
    gres, cs = _geo(g)
    px = g["px"].copy()
    out = D.solve(gres, g["bound_min"], g["bound_size"], float(g["rho0"]), float(g["dt"]), px, g["pm"], g["sphi"], g["lphi"],
                  g["lvol"], g["wx"], g["wy"], tol=float(g["tol"]), max_iter=int(g["max_iter"]))
    hg, it = g["history"], int(g["iters"])
    n = min(21, len(hg), len(out["history"]))
    np.testing.assert_allclose(out["history"][:n], hg[:n], rtol=1e-9)
    assert abs(out["iters"] - it) <= max(2, it // 10), (out["iters"], it)
    np.testing.assert_allclose(out["x"], g["x"], rtol=0, atol=1e-6 * np.abs(g["x"]).max())
    np.testing.assert_allclose(px, g["out_px"], rtol=0, atol=1e-6 * np.abs(g["out_px"] - g["px"]).max() + 1e-7)


def test_goldens_hold_their_edge_cases():
    hit = dict(lo=0, hi=0, tiny=0, theta=0)
    for name in DNAMES:
        g = golden(name)
        gres, cs = _geo(g)
        Nx, Ny = gres
        frac, tiny = D.rhs(float(g["rho0"]), float(g["dt"]), gres, cs, g["gm"], g["gvol"], g["lphi"], g["wx"], g["wy"],
                           np.zeros(gres))
        lo, hi = int((frac < 0.5).sum()), int((frac > 1.5).sum())
        assert lo > 0 and hi > 0 and tiny.sum() > 0, (name, lo, hi, int(tiny.sum()))
        st = {}
        D.apply(gres, g["rv"], np.zeros(gres), g["wx"], g["wy"], g["lphi"], stats=st)
        assert st["theta_clamped"] > 0, name
        w = np.concatenate([g["wx"].ravel(), g["wy"].ravel()])
        assert ((w > 0) & (w < 1)).any(), name                      # fractional face weights
        # scatter indices clamped at all four walls
        gi = np.floor((g["px"].astype(np.float64) - g["bound_min"]) / cs - 0.5)
        assert (gi[:, 0] < 0).any() and (gi[:, 0] + 1 > Nx - 1).any() and (gi[:, 1] < 0).any() and (gi[:, 1] + 1 > Ny - 1).any()
        hit["lo"] += lo; hit["hi"] += hi; hit["tiny"] += int(tiny.sum()); hit["theta"] += st["theta_clamped"]
    c = golden("d2d_c_33x21_maxiter6")
    assert int(c["iters"]) == int(c["max_iter"]) == 6 and c["history"][-1] >= float(c["tol"]) ** 2
    assert np.abs(c["out_px"] - c["px"]).max() > 0               # ... and the displacement was applied all the same
    assert golden("d2d_b_40x28_f32")["px"].dtype == np.float32
    b = golden("d2d_b_40x28_f32")
    assert not np.isclose(*(b["bound_size"] / b["gres"]))        # a non-square cell


@pytest.mark.parametrize("name", SNAMES)
def test_numpy_sdf_matches_golden(name):
    g = golden(name)
    sd, vel = D.sdf_evaluate(g["rb_d"], g["position"])
    np.testing.assert_allclose(sd, g["sd"], rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(vel, g["vel"])
    proj = g["position"].copy()
    D.sdf_project(g["rb_d"], proj)
    assert proj.dtype == g["projected"].dtype
    np.testing.assert_allclose(proj, g["projected"], rtol=0, atol=1e-15 if proj.dtype == np.float64 else 1.2e-7)
    # the golden's own edge cases: a moving body's velocity, zero velocity outside, the flipped box rewrote points
    assert (g["vel"][g["sd"] > 0] == 0).all() and (g["vel"] != 0).any() and (g["sd"] != 7).all()
    assert g["rb_d"].shape == (3, 8, 3) and sorted(g["rb_d"][:, 0, 0]) == [0, 2, 3]
    c = g["rb_d"][2, 1:3, 2]
    # point 4 sits at the sphere's centre: a solid sphere leaves it there (dist <= 0.0001 branch)
    np.testing.assert_allclose(g["projected"][4], c, rtol=0, atol=1e-6)


def test_scene_matches_sdf_golden_layout():
    from mfs import scenes
    sc = scenes.density_scene_2d((32, 32), 41)
    np.testing.assert_array_equal(sc["rb_d"], golden("sdf2d_a_f64")["rb_d"])
    # the scene's own sphi is what evaluate gives on the doubled grid
    X = sc["bound_min"][0] + np.arange(65) * 0.5 * sc["cell_size"][0]
    Y = sc["bound_min"][1] + np.arange(65) * 0.5 * sc["cell_size"][1]
    P = np.stack(np.meshgrid(X, Y, indexing="ij"), axis=-1)
    sd, vel = D.sdf_evaluate(sc["rb_d"], P)
    np.testing.assert_allclose(sd, sc["sphi"], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(vel, sc["sv"])


def test_module_imports_and_signatures():
    import inspect
    import solver.DensityCGSolver2D as M
    import solver.sdf2D as S
    for fn in ("initialize_density", "fix_volume", "initialize_solver", "matvecmul", "compute_displacement",
               "apply_displacement", "compute_solid_frac", "edge_in_fraction", "DensityCGSolver2D"):
        assert hasattr(M, fn), fn
    assert list(inspect.signature(M.DensityCGSolver2D.solve).parameters) == [
        "self", "rho0", "dt", "px", "pm", "pvol", "vx", "vy", "sphi", "sv", "lphi", "lvol", "wx", "wy", "tol"]
    assert list(inspect.signature(M.DensityCGSolver2D.__init__).parameters)[:5] == ["self", "buf", "gres", "bound_min",
                                                                                    "bound_size"]
    for fn in ("evaluate", "project", "generate_rb", "transform_rb", "set_vel_rb", "get_T", "get_R"):
        assert hasattr(S, fn), fn
    src = open(S.__file__).read()
    assert "matplotlib" not in src and "scipy" not in src
    np.testing.assert_array_equal(S.get_T([1.5, -2.0]), [[1, 0, 1.5], [0, 1, -2.0], [0, 0, 1]])
    r = S.get_R([0, 1], 90)
    np.testing.assert_allclose(r, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert (S.get_R([0, 1], 0) == np.identity(3)).all()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    return _lib.load()


ENTRY = ["mfs_density_splat2d", "mfs_density_fix_volume2d", "mfs_density_rhs2d", "mfs_density_apply2d",
         "mfs_density_displacement2d", "mfs_density_advect2d", "mfs_sdf_evaluate2d", "mfs_sdf_project2d",
         "mfs_pcg2d_setup_density", "mfs_pcg2d_apply"]


def test_entry_points_declared_exported_and_typed(lib):
    from mfs import _lib
    hdr = open(os.path.join(REPO, "include", "mfs.h")).read()
    for name in ENTRY:
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} not declared in include/mfs.h"
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_bad_arguments_are_refused(lib):
    from mfs import _lib
    E = -1          # MFS_E_INVALID
    g = _lib.i64x((8, 6))
    two = _lib.f64x((0.1, 0.2))
    p = [C.c_void_p(0x1000 * (k + 1)) for k in range(8)]      # never dereferenced: refused before any launch
    assert lib.mfs_density_splat2d(g, two, two, p[0], 1, p[1], 1, 0.0, 10, None, p[3], 1, None) == E
    assert b"null" in lib.mfs_last_error()
    assert lib.mfs_density_splat2d(g, two, two, None, 1, p[1], 1, 0.0, 10, p[2], p[3], 1, None) == E
    assert lib.mfs_density_splat2d(g, two, two, p[0], 1, p[1], 1, 0.0, -1, p[2], p[3], 1, None) == E
    assert lib.mfs_density_splat2d(g, two, two, p[0], 4, p[1], 1, 0.0, 10, p[2], p[3], 1, None) == E
    assert lib.mfs_density_fix_volume2d(g, two, None, 1, p[1], 1, p[2], 1, p[3], 1, p[4], p[5], 1, None) == E
    assert lib.mfs_density_fix_volume2d(g, two, p[1], 1, p[1], 1, p[2], 1, p[3], 1, p[4], p[5], 1, None) == E
    assert b"alias" in lib.mfs_last_error()
    assert lib.mfs_density_rhs2d(g, 1.0, 1.0, two, p[0], p[1], 1, p[2], 1, p[3], p[4], 1, None, 1, None) == E
    assert lib.mfs_density_apply2d(g, p[0], p[0], 1, p[1], p[2], 1, p[3], 1, None) == E
    assert lib.mfs_density_apply2d(g, p[0], p[4], 9, p[1], p[2], 1, p[3], 1, None) == E
    assert lib.mfs_density_displacement2d(g, 1.0, two, p[0], p[0], 1, p[1], 1, p[2], 1, None) == E
    assert lib.mfs_density_advect2d(p[0], 1, 10, p[1], 1, _lib.i64x((9, 6)), two, two, two, 2, None) == E
    assert lib.mfs_density_advect2d(p[0], 1, 10, p[1], 1, _lib.i64x((0, 6)), two, two, two, 0, None) == E
    for bad in ((0, 6), (8, -1), (70000, 4)):
        gb = _lib.i64x(bad)
        assert lib.mfs_density_apply2d(gb, p[0], p[4], 1, p[1], p[2], 1, p[3], 1, None) == E
        assert lib.mfs_density_rhs2d(gb, 1.0, 1.0, two, p[0], p[1], 1, p[2], 1, p[3], p[4], 1, p[5], 1, None) == E
    assert lib.mfs_sdf_evaluate2d(None, 2, p[0], 1, 10, p[1], 1, p[2], 1, None) == E
    assert lib.mfs_sdf_evaluate2d(p[3], 2, p[0], 1, 10, None, 1, p[2], 1, None) == E
    assert lib.mfs_sdf_project2d(p[3], 2, None, 1, 10, None) == E
    assert lib.mfs_sdf_project2d(p[3], 2, p[0], 3, 10, None) == E
    assert lib.mfs_pcg2d_setup_density(None, p[0], 1, p[1], p[2], 1) == E
    assert lib.mfs_pcg2d_apply(None, p[0], p[1], None) == E


def test_python_argument_checks_raise_before_any_gpu_call():
    import torch
    import solver.DensityCGSolver2D as M
    import solver.sdf2D as S
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)      # noqa: E731   (CPU tensors)
    with pytest.raises(TypeError, match="GPU"):
        M.matvecmul((4, 4), z(4, 4), z(4, 4), z(5, 4), z(4, 5), z(4, 4))
    with pytest.raises(TypeError, match="GPU"):
        M.initialize_density((0, 0), (1, 1), (4, 4), z(3, 2), z(3), 1.0, z(4, 4), z(4, 4))
    with pytest.raises(TypeError, match="GPU"):
        M.apply_displacement(z(3, 2), z(5, 4), (0, 0), (1, 1), (0, 0.5), 0)
    with pytest.raises(ValueError, match="2D"):
        M.matvecmul((4, 4, 4), z(4, 4), z(4, 4), z(5, 4), z(4, 5), z(4, 4))
    with pytest.raises(TypeError, match="GPU"):
        S.project(z(1, 8, 3), z(5, 2))
    with pytest.raises(TypeError, match="GPU"):
        S.evaluate(z(1, 8, 3), z(5), z(5, 2), z(5, 2))
    rb = S.generate_rb(None, {}, "x", ["cylinder", 1.0, 2.0], device="cpu")
    assert isinstance(rb, torch.Tensor) and tuple(rb.shape) == (0, 8, 3)       # unknown shape: the bare rb_d
    rb, m = S.generate_rb(rb, {}, "b", ["box", 1.0, 2.0], flip=True, center=[0.5, 0.25], angle=30, device="cpu")
    S.set_vel_rb(rb, 0, [0.3, -0.2])
    assert m == {"b": 0} and rb[0, 0].tolist() == [3.0, 1.0, 2.0] and rb[0, 7].tolist() == [0.3, -0.2, 0.0]
