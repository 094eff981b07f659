"""CPU: the 2D pressure goldens beyond the smooth scene.  The edge cases (p2d_c, p2dt_d/e; mfs.scenes.pressure_scene_2d_edges)
must really hold the level-set edges they were made for, counted from their inputs, so that a regeneration cannot lose
one silently; the stale-boundary golden (p2dq_*) pins what the reference's CG loop does with boundary-ring values of the
shared CGSolverBuffer that it never writes itself, and the oracle's loop must reproduce it."""
import numpy as np
import pytest

from conftest import golden, golden_names
from oracle import mfs_oracle as O
from test_oracle_golden import test_pressure2d as check_pressure2d_golden   # (no test_ name: not collected twice)

# p2d_c runs in the p2d_ tests as it is; the thin grids (one interior column / row) have a prefix of their own
# because their GPU history leaves the 1e-8 window of test_pressure2d_gpu.py (test_pressure2d_oracle_gpu.py)
EDGE_CASES = ["p2d_c_33x17_edges", "p2dt_d_3x130", "p2dt_e_130x3"]


def signed_zeros(a):
    a = np.asarray(a)
    return int(((a == 0) & ~np.signbit(a)).sum()), int(((a == 0) & np.signbit(a)).sum())


def clamp_hits(gres, lphi, wx, wy):
    """(apply, update): open faces whose theta = max(0.01, ...) takes the clamp.  apply: a liquid interior cell and a
    non-liquid neighbour with phi / (phi - nphi) < 0.01 (solver/PressureCGSolver2D.py:46-100); update: a face the update
    writes (cells x >= 1, y >= 1, one side liquid) with edge_in_fraction < 0.01 (:102-120)."""
    Nx, Ny = gres
    ap = up = 0
    for x in range(Nx):
        for y in range(Ny):
            p = lphi[x, y]
            if 0 < x < Nx - 1 and 0 < y < Ny - 1 and p < 0:
                for (i, j), w in (((x + 1, y), wx[x + 1, y]), ((x - 1, y), wx[x, y]), ((x, y + 1), wy[x, y + 1]),
                                  ((x, y - 1), wy[x, y])):
                    nphi = lphi[i, j]
                    if not nphi < 0 and w > 0 and p / (p - nphi) < 0.01:
                        ap += 1
            if x >= 1 and y >= 1:
                for (i, j), w in (((x - 1, y), wx[x, y]), ((x, y - 1), wy[x, y])):
                    m = lphi[i, j]
                    if (p < 0 or m < 0) and w > 0 and float(O.edge_in_fraction(p, m)) < 0.01:
                        up += 1
    return ap, up


def test_edge_cases_are_present():
    assert golden_names("p2d_") == ["p2d_a_64", "p2d_b_24x20_sv", "p2d_c_33x17_edges"]
    assert golden_names("p2dt_") == ["p2dt_d_3x130", "p2dt_e_130x3"]
    assert golden_names("p2dq_") == ["p2dq_stale_24x20"]


@pytest.mark.parametrize("name", golden_names("p2dt_"))
def test_oracle_thin_grid_golden(name):
    """the oracle against the thin-grid goldens, exactly as test_oracle_golden.py checks the p2d_ ones"""
    check_pressure2d_golden(name)


@pytest.mark.parametrize("name", EDGE_CASES)
def test_edge_case_holds_its_edges(name):
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    Nx, Ny = gres
    assert bool(g["edges"]) and bool(g["solid_velocity"]) and np.abs(g["sv"]).max() > 0
    assert np.all(g["bound_size"] == g["gres"])                        # cell size exactly 1
    # exact and signed zeros: sphi at the corner nodes (what the fractions read), lphi at cell centres, interior too
    pz, nz = signed_zeros(g["sphi"][::2, ::2])
    assert pz > 0 and nz > 0, (pz, nz)
    pz, nz = signed_zeros(g["lphi"][1:Nx - 1, 1:Ny - 1])
    assert pz > 0 and nz > 0, (pz, nz)
    # liquid cells a hair (1e-4 cells) below the surface
    lp = g["lphi"]
    assert np.sum((lp < 0) & (lp > -1e-3)) > 0
    wx, wy = g["wx"], g["wy"]
    assert np.any((wx > 0) & (wx < 1)) or name != "p2d_c_33x17_edges"       # partial solid fractions (the diamond)
    ap, up = clamp_hits(gres, lp, wx, wy)
    assert ap >= 1 and up >= 1, (ap, up)
    # both liquid and air interior cells; the solve converged at its recorded tol
    inner = lp[1:Nx - 1, 1:Ny - 1]
    assert np.any(inner < 0) and np.any(~(inner < 0))
    assert g["history"][-1] < float(g["tol"]) ** 2


@pytest.mark.parametrize("name", golden_names("p2dq_"))
def test_oracle_stale_boundary_vs_golden(name):
    """the oracle's cg on buffers whose boundary ring holds the same stale b, q, d, r: d = r = b - q there, q keeps
    its stale value (the apply writes interior cells only), so d.q, r.r and x pick up the ring exactly as in the
    reference"""
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    Nx, Ny = gres
    wx, wy = np.zeros((Nx + 1, Ny)), np.zeros((Nx, Ny + 1))
    O.compute_solid_frac2d(gres, g["sphi"], wx, wy)
    np.testing.assert_array_equal(wx, g["wx"])
    b, q, d, r = (g["pre_" + k].copy() for k in "bqdr")
    assert all(np.count_nonzero(a) == 2 * (Nx + Ny) - 4 for a in (b, q, d, r))
    x = np.full(gres, 0.0)
    O.pressure_rhs2d(g["bound_size"] / g["gres"], gres, g["in_vx"], g["in_vy"], g["sphi"], g["sv"], g["lphi"], b,
                     wx, wy)
    hist = []
    ap = lambda V, Q: O.pressure_apply2d(gres, V[0], Q[0], wx, wy, g["lphi"])  # noqa: E731
    it, delta, alpha, beta = O.cg(ap, b, x, d, r, q, 0.0, int(g["max_iter"]), hist, raise_on_fail=False)
    assert it == int(g["iters"]) == int(g["max_iter"])
    np.testing.assert_allclose(hist, g["history"], rtol=1e-9)
    for a, k in ((b, "b"), (x, "x"), (d, "d"), (r, "r"), (q, "q")):
        np.testing.assert_allclose(a, g[k], rtol=0, atol=1e-9 * np.abs(g[k]).max(), err_msg=k)
    np.testing.assert_array_equal(q[0], g["pre_q"][0])            # the ring of q is never written
    assert np.abs(x[0]).max() > 0                                 # ... while x moves there
    assert delta == pytest.approx(float(g["delta"]), rel=1e-9) and alpha == pytest.approx(float(g["alpha"]), rel=1e-9)
    vx, vy = g["in_vx"].copy(), g["in_vy"].copy()
    O.pressure_update2d(gres, g["bound_size"] / g["gres"], vx, vy, x, wx, wy, g["sv"], g["lphi"])
    np.testing.assert_allclose(vx, g["out_vx"], rtol=0, atol=1e-9 * np.abs(g["out_vx"]).max())
    np.testing.assert_allclose(vy, g["out_vy"], rtol=0, atol=1e-9 * np.abs(g["out_vy"]).max())


@pytest.mark.parametrize("gres", [(1, 1), (1, 7), (7, 1), (2, 5), (5, 2)])
def test_oracle_grids_without_interior_cells(gres):
    """pressure_rhs2d / pressure_apply2d on a grid with no interior cell write nothing (the reference's kernels return
    for every thread); the class solve then starts and ends at delta = 0"""
    Nx, Ny = gres
    b, out = np.full(gres, 7.0), np.full(gres, 7.0)
    wx, wy = np.ones((Nx + 1, Ny)), np.ones((Nx, Ny + 1))
    O.pressure_rhs2d((1.0, 1.0), gres, np.ones((Nx + 1, Ny)), np.ones((Nx, Ny + 1)), None,
                     np.ones((2 * Nx + 1, 2 * Ny + 1, 2)), -np.ones(gres), b, wx, wy)
    O.pressure_apply2d(gres, np.ones(gres), out, wx, wy, -np.ones(gres))
    assert np.all(b == 7.0) and np.all(out == 7.0)
    s = O.PressureCGSolver2D(gres, (1.0, 1.0))
    s.solve(np.ones((Nx + 1, Ny)), np.ones((Nx, Ny + 1)), np.ones((2 * Nx + 1, 2 * Ny + 1)),
            np.zeros((2 * Nx + 1, 2 * Ny + 1, 2)), -np.ones(gres))
    assert s.iterations == 0 and s.history == [0.0] and not s.x.any()
