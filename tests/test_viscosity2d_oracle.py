"""ViscosityCGSolver2D without a GPU: the numpy restatement (tests/visc2d_numpy.py) against the goldens that the
reference's own source wrote (tests/golden/make_goldens_visc2d.py), the module imports, and the C ABI's argument
checks, which refuse bad calls before anything touches a device."""
import ctypes as C

import numpy as np
import pytest

import visc2d_numpy as V
from conftest import golden, golden_names

NAMES = golden_names("v2d_")


def _scale_vol(g):
    gres = tuple(int(v) for v in g["gres"])
    cell_vol = float(np.prod(np.asarray(g["bound_size"], np.float64) / np.asarray(gres, np.float64)))
    return gres, float(g["dt"]) / cell_vol / float(g["rho"]), g["lvol"] / (cell_vol * 0.125)


def _close(a, b, tol, what):
    b = np.asarray(b, np.float64)
    np.testing.assert_allclose(np.asarray(a, np.float64), b, rtol=0, atol=tol * max(np.abs(b).max(), 1e-300),
                               err_msg=what)


def test_three_goldens_exist():
    assert NAMES == ["v2d_a_64", "v2d_b_24x40", "v2d_c_33x17_mu200"]


@pytest.mark.parametrize("name", NAMES)
def test_numpy_rhs_and_apply_match_golden(name):
    g = golden(name)
    gres, scale, vol = _scale_vol(g)
    fx, fy = (gres[0] + 1, gres[1]), (gres[0], gres[1] + 1)
    vx, vy = g["in_vx"].astype(np.float64), g["in_vy"].astype(np.float64)
    bx, by = np.full(fx, 7.0), np.full(fy, 7.0)
    V.rhs(gres, scale, float(g["mu"]), vx, vy, g["sphi"], vol, bx, by)
    qx, qy = np.full(fx, 7.0), np.full(fy, 7.0)
    V.apply(gres, scale, float(g["mu"]), vx, vy, qx, qy, g["sphi"], vol)
    for a, b, what in ((bx, g["bx"], "bx"), (by, g["by"], "by"), (qx, g["qx"], "qx"), (qy, g["qy"], "qy")):
        _close(a, b, 1e-12, what)
    # the faces the reference never writes kept the 7.0 prefill, in the golden and here
    for a in (g["bx"], g["qx"], bx, qx):
        assert (a[0] == 7).all() and (a[-1] == 7).all() and (a[:, 0] == 7).all() and (a[:, -1] == 7).all()
    for a in (g["by"], g["qy"], by, qy):
        assert (a[0] == 7).all() and (a[-1] == 7).all() and (a[:, 0] == 7).all() and (a[:, -1] == 7).all()
    assert (g["bx"][1:-1, 1:-1] != 7).all() and (g["qy"][1:-1, 1:-1] != 7).all()


@pytest.mark.parametrize("name", NAMES)
def test_numpy_solve_matches_golden(name):
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    vx, vy = g["in_vx"].copy(), g["in_vy"].copy()
    out = V.solve(gres, g["bound_size"], float(g["dt"]), float(g["mu"]), float(g["rho"]), vx, vy, g["sphi"],
                  g["lvol"], tol=float(g["tol"]))
    hg, it = g["history"], int(g["iters"])
    np.testing.assert_allclose(out["history"][:21], hg[:21], rtol=1e-9)
    assert abs(out["iters"] - it) <= max(2, it // 10), (out["iters"], it)
    for a, b, what in ((out["x_x"], g["x_x"], "x_x"), (out["x_y"], g["x_y"], "x_y"),
                       (vx, g["out_vx"], "vx"), (vy, g["out_vy"], "vy")):
        _close(a, b, 1e-6, what)
    assert vx.dtype == g["in_vx"].dtype


def test_golden_scenes_carry_the_quirks():
    """what the GPU quirk tests lean on: exact sphi zeros at face samples, partial liquid volume, nonzero velocity in
    solid faces"""
    for name in NAMES:
        g = golden(name)
        s = g["sphi"]
        assert (s[0::2, 1::2] == 0.0).any() and (s[1::2, 0::2] == 0.0).any(), name
        lv = g["lvol"]
        full = lv.max()
        assert ((lv > 0) & (lv < full)).any(), name
        assert np.abs(g["in_vx"][s[0::2, 1::2] <= 0]).max() > 0, name


def test_module_imports():
    import solver.ViscosityCGSolver2D as M
    for fn in ("initialize_solver", "matvecmul", "apply_viscosity", "ViscosityCGSolver2D"):
        assert hasattr(M, fn)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    return _lib.load()


ENTRY = ["mfs_visc_rhs2d", "mfs_visc_apply2d", "mfs_visc_writeback2d", "mfs_vcg2d_workspace_bytes", "mfs_vcg2d_dofs",
         "mfs_vcg2d_create", "mfs_vcg2d_destroy", "mfs_vcg2d_setup", "mfs_vcg2d_bind", "mfs_vcg2d_apply",
         "mfs_vcg2d_solve", "mfs_vcg2d_poll", "mfs_vcg2d_history"]


def test_entry_points_exported(lib):
    from mfs import _lib
    for name in ENTRY:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_bad_arguments_are_refused(lib):
    from mfs import _lib
    E = -1          # MFS_E_INVALID
    g = _lib.i64x((8, 6))
    p = [C.c_void_p(0x1000 * (k + 1)) for k in range(8)]      # never dereferenced: refused before any launch
    # null arrays
    assert lib.mfs_visc_rhs2d(g, 1.0, 1.0, None, p[1], 1, p[2], 1, p[3], 1, p[4], p[5], 1, None) == E
    assert b"null" in lib.mfs_last_error()
    assert lib.mfs_visc_apply2d(g, 1.0, 1.0, p[0], p[1], 1, None, p[5], 1, p[2], 1, p[3], 1, None) == E
    assert lib.mfs_visc_writeback2d(g, p[0], p[1], 1, p[2], p[3], 1, None, 1, None) == E
    # aliased arrays
    assert lib.mfs_visc_rhs2d(g, 1.0, 1.0, p[0], p[1], 1, p[2], 1, p[3], 1, p[0], p[5], 1, None) == E
    assert b"alias" in lib.mfs_last_error()
    assert lib.mfs_visc_apply2d(g, 1.0, 1.0, p[0], p[1], 1, p[4], p[4], 1, p[2], 1, p[3], 1, None) == E
    assert lib.mfs_visc_writeback2d(g, p[0], p[1], 1, p[1], p[3], 1, p[2], 1, None) == E
    # bad dtype, bad gres
    assert lib.mfs_visc_apply2d(g, 1.0, 1.0, p[0], p[1], 5, p[4], p[5], 1, p[2], 1, p[3], 1, None) == E
    for bad in ((0, 6), (8, -1), (70000, 4)):
        gb = _lib.i64x(bad)
        assert lib.mfs_visc_rhs2d(gb, 1.0, 1.0, p[0], p[1], 1, p[2], 1, p[3], 1, p[4], p[5], 1, None) == E
        assert lib.mfs_visc_apply2d(gb, 1.0, 1.0, p[0], p[1], 1, p[4], p[5], 1, p[2], 1, p[3], 1, None) == E
        assert lib.mfs_visc_writeback2d(gb, p[0], p[1], 1, p[4], p[5], 1, p[2], 1, None) == E
        assert lib.mfs_vcg2d_workspace_bytes(gb, 1) == 0
        h = C.c_void_p()
        assert lib.mfs_vcg2d_create(C.byref(h), gb, 1, p[6], 1 << 30, None) == E
    assert lib.mfs_visc_rhs2d(None, 1.0, 1.0, p[0], p[1], 1, p[2], 1, p[3], 1, p[4], p[5], 1, None) == E
    # engine: workspace size / dtype / null handle
    assert lib.mfs_vcg2d_workspace_bytes(g, 7) == 0
    assert lib.mfs_vcg2d_dofs(g) == 9 * 6 + 8 * 7
    assert lib.mfs_vcg2d_workspace_bytes(g, 0) > 0
    h = C.c_void_p()
    assert lib.mfs_vcg2d_create(C.byref(h), g, 1, p[6], 16, None) == E             # workspace too small
    assert lib.mfs_vcg2d_setup(None, 1.0, 1.0, p[0], 1, p[1], 1, None) == E
    assert lib.mfs_vcg2d_apply(None, p[0], p[1], None) == E
    assert lib.mfs_vcg2d_solve(None, 1e-4, 10, 4, None, None) == E
    assert lib.mfs_vcg2d_bind(None, p[0], p[1], p[2], p[3], p[4]) == E
