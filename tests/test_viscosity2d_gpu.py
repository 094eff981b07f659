"""ViscosityCGSolver2D on the MI355X: module functions and the class against the goldens the reference's own source
wrote (tests/golden/make_goldens_visc2d.py), the quirks of the 2D reference one by one, the engine's operator apply
against the direct kernel bit for bit, and production-size grids against the numpy restatement
(tests/visc2d_numpy.py).

History window of the fp64 class solve: the leading 10 iterations (21 entries) at rtol 1e-8 -- CG on this operator
amplifies rounding as the 2D pressure one does (test_pressure2d_gpu.py), and the GPU's dot products sum in another
order than cp.sum."""
import numpy as np
import pytest
import torch

import visc2d_numpy as V
from conftest import golden, golden_names

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = golden_names("v2d_")
HIST_N, HIST_RTOL = 21, 1e-8


def T(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dtype is None else t.to(dtype)


def N(t):
    return t.detach().cpu().numpy()


def close(a, b, tol, what=""):
    a = N(a) if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b, np.float64)
    np.testing.assert_allclose(a.astype(np.float64), b, rtol=0, atol=tol * max(np.abs(b).max(), 1e-300),
                               err_msg=what)


def scale_vol(gres, bound_size, dt, rho, lvol):
    cell_vol = float(np.prod(np.asarray(bound_size, np.float64) / np.asarray(gres, np.float64)))
    return dt / cell_vol / rho, lvol / (cell_vol * 0.125)


def case(name):
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    scale, vol = scale_vol(gres, g["bound_size"], float(g["dt"]), float(g["rho"]), g["lvol"])
    return g, gres, scale, vol


def sv_of(gres):
    return torch.zeros((2 * gres[0] + 1, 2 * gres[1] + 1, 2), dtype=torch.float64, device=DEV)


# ------------------------------------------------------------------------------------------ module functions ---
@pytest.mark.parametrize("name", NAMES)
def test_module_functions_vs_golden(name):
    import solver.ViscosityCGSolver2D as M
    g, gres, scale, vol = case(name)
    fx, fy = (gres[0] + 1, gres[1]), (gres[0], gres[1] + 1)
    vx, vy = T(g["in_vx"], torch.float64), T(g["in_vy"], torch.float64)
    bx, by = T(np.full(fx, 7.0)), T(np.full(fy, 7.0))
    M.initialize_solver(gres, scale, float(g["mu"]), vx, vy, T(g["sphi"]), sv_of(gres), T(vol), bx, by)
    qx, qy = T(np.full(fx, 7.0)), T(np.full(fy, 7.0))
    M.matvecmul(gres, scale, float(g["mu"]), vx, vy, qx, qy, T(g["sphi"]), T(vol))
    for a, b, what in ((bx, g["bx"], "bx"), (by, g["by"], "by"), (qx, g["qx"], "qx"), (qy, g["qy"], "qy")):
        close(a, b, 1e-12, what)
        ga = N(a)
        assert np.array_equal(ga == 7.0, np.asarray(b) == 7.0), f"{what}: untouched faces differ"


@pytest.mark.parametrize("name", NAMES)
def test_apply_viscosity_writes_exactly_the_reference_faces(name):
    import solver.ViscosityCGSolver2D as M
    g, gres, _, _ = case(name)
    Nx, Ny = gres
    rng = np.random.default_rng(5)
    ox, oy = rng.standard_normal((Nx + 1, Ny)), rng.standard_normal((Nx, Ny + 1))
    vx0, vy0 = np.full((Nx + 1, Ny), -9.0), np.full((Nx, Ny + 1), -9.0)
    vx, vy = T(vx0), T(vy0)
    M.apply_viscosity(gres, vx, vy, T(ox), T(oy), T(g["sphi"]), None)
    s = g["sphi"]
    ex, ey = vx0.copy(), vy0.copy()
    for x in range(1, Nx):
        for y in range(1, Ny):
            if s[2 * x, 2 * y + 1] > 0:
                ex[x, y] = ox[x, y]
            if s[2 * x + 1, 2 * y] > 0:
                ey[x, y] = oy[x, y]
    assert np.array_equal(N(vx), ex) and np.array_equal(N(vy), ey)
    # all samples > 0: exactly the faces of cells 1 <= x <= Nx-1, 1 <= y <= Ny-1 -- the top row of vx and the right
    # column of vy included, unlike the RHS / apply
    vx, vy = T(vx0), T(vy0)
    M.apply_viscosity(gres, vx, vy, T(ox), T(oy), T(np.ones_like(s)), None)
    ex, ey = vx0.copy(), vy0.copy()
    ex[1:Nx, 1:Ny] = ox[1:Nx, 1:Ny]
    ey[1:Nx, 1:Ny] = oy[1:Nx, 1:Ny]
    assert np.array_equal(N(vx), ex) and np.array_equal(N(vy), ey)


# ----------------------------------------------------------------------------------------------- class solve ---
def _solver(gres, g, precision="fp64", **kw):
    from solver.ViscosityCGSolver2D import ViscosityCGSolver2D
    return ViscosityCGSolver2D(gres, g["bound_size"], precision=precision, device=DEV, **kw)


def _solve(s, g, vx, vy, **kw):
    gres = tuple(int(v) for v in g["gres"])
    kw.setdefault("tol", float(g["tol"]))
    s.solve(float(g["dt"]), float(g["mu"]), float(g["rho"]), vx, vy, T(g["sphi"]), sv_of(gres), None, T(g["lvol"]),
            **kw)


@pytest.mark.parametrize("name", NAMES)
def test_class_solve_fp64_vs_golden(name):
    g, gres, _, _ = case(name)
    s = _solver(gres, g)
    vx, vy = T(g["in_vx"]), T(g["in_vy"])
    _solve(s, g, vx, vy)
    it = int(g["iters"])
    h = s.history
    np.testing.assert_allclose(h[:HIST_N], g["history"][:HIST_N], rtol=HIST_RTOL)
    assert abs(s.iterations - it) <= max(2, it // 10), (s.iterations, it)
    assert s.delta < float(g["tol"]) ** 2 and not s.history_truncated
    assert len(h) == 2 * s.iterations + 1
    for a, b, what in ((s.x_x, g["x_x"], "x_x"), (s.x_y, g["x_y"], "x_y"), (vx, g["out_vx"], "vx"),
                       (vy, g["out_vy"], "vy")):
        close(a, b, 1e-5, what)
    assert vx.dtype == T(g["in_vx"]).dtype


@pytest.mark.parametrize("name", NAMES)
def test_class_solve_fp32_state(name):
    g, gres, _, _ = case(name)
    s = _solver(gres, g, precision="fp32")
    assert s.x_x.dtype == torch.float32 and s.vol.dtype == torch.float64
    vx, vy = T(g["in_vx"]), T(g["in_vy"])
    _solve(s, g, vx, vy)
    it = int(g["iters"])
    assert 0.8 * it <= s.iterations <= 1.5 * it, (s.iterations, it)
    for a, b, what in ((s.x_x, g["x_x"], "x_x"), (s.x_y, g["x_y"], "x_y"), (vx, g["out_vx"], "vx"),
                       (vy, g["out_vy"], "vy")):
        close(a, b, 1e-4, what)


def test_attributes_keep_reference_names_and_shapes():
    g, gres, _, _ = case("v2d_b_24x40")
    s = _solver(gres, g)
    Nx, Ny = gres
    for nm in "drqxb":
        assert tuple(getattr(s, f"{nm}_x").shape) == (Nx + 1, Ny)
        assert tuple(getattr(s, f"{nm}_y").shape) == (Nx, Ny + 1)
    assert tuple(s.vol.shape) == (2 * Nx + 1, 2 * Ny + 1)
    assert s.max_iter == Nx * Ny and s.alpha == s.beta == s.delta == 0.0
    assert s.device.type == "cuda" and s.precision == torch.float64


def test_cpu_tensors_refused():
    import solver.ViscosityCGSolver2D as M
    g, gres, scale, vol = case("v2d_b_24x40")
    with pytest.raises(TypeError, match="GPU"):
        M.matvecmul(gres, scale, 1.0, torch.zeros(25, 40, dtype=torch.float64), torch.zeros(24, 41, dtype=torch.float64),
                    torch.zeros(25, 40, dtype=torch.float64), torch.zeros(24, 41, dtype=torch.float64),
                    torch.as_tensor(g["sphi"]), torch.as_tensor(vol))
    s = _solver(gres, g)
    with pytest.raises(TypeError, match="GPU"):
        s.solve(float(g["dt"]), 1.0, 1000.0, torch.as_tensor(g["in_vx"]), torch.as_tensor(g["in_vy"]),
                T(g["sphi"]), None, None, T(g["lvol"]))


# ----------------------------------------------------------------------------------------------------- quirks ---
def test_quirk1_sphi_zero_is_solid():
    import solver.ViscosityCGSolver2D as M
    g, gres, scale, vol = case("v2d_a_64")
    Nx, Ny = gres
    s = g["sphi"].copy()
    # an interior x-face whose own sample is exactly 0.0 and whose cell holds liquid
    cand = [(x, y) for x in range(1, Nx) for y in range(1, Ny - 1)
            if s[2 * x, 2 * y + 1] == 0.0 and vol[2 * x, 2 * y + 1] > 0]
    assert cand
    x, y = cand[0]
    vx, vy = T(g["in_vx"], torch.float64), T(g["in_vy"], torch.float64)

    def q_of(sp):
        qx, qy = torch.zeros((Nx + 1, Ny), dtype=torch.float64, device=DEV), torch.zeros((Nx, Ny + 1),
                                                                                          dtype=torch.float64, device=DEV)
        M.matvecmul(gres, scale, float(g["mu"]), vx, vy, qx, qy, T(sp), T(vol))
        return N(qx), N(qy)

    q0x, q0y = q_of(s)
    assert q0x[x, y] == 0.0                          # sphi == 0 -> solid -> row zeroed
    s2 = s.copy()
    s2[2 * x, 2 * y + 1] = 1e-300
    q1x, q1y = q_of(s2)
    assert q1x[x, y] != 0.0
    ex, ey = np.zeros_like(q1x), np.zeros_like(q1y)
    V.apply(gres, scale, float(g["mu"]), g["in_vx"], g["in_vy"], ex, ey, s2, vol)
    assert np.array_equal(q1x, ex) and np.array_equal(q1y, ey)


def test_quirk2_no_extrapolation_rhs_reads_raw_solid_velocities():
    import solver.ViscosityCGSolver2D as M
    g, gres, scale, vol = case("v2d_a_64")
    Nx, Ny = gres
    s = g["sphi"]
    # a solid x-face (sample <= 0) that is the +x neighbour of a non-solid interior x-face
    cand = [(x, y) for x in range(1, Nx - 1) for y in range(1, Ny - 1)
            if s[2 * x, 2 * y + 1] > 0 and s[2 * x + 2, 2 * y + 1] <= 0 and vol[2 * x + 1, 2 * y + 1] > 0]
    assert cand
    x, y = cand[0]
    vx = g["in_vx"].astype(np.float64)
    vx2 = vx.copy()
    vx2[x + 1, y] += 3.0
    out = []
    for v in (vx, vx2):
        bx = torch.zeros((Nx + 1, Ny), dtype=torch.float64, device=DEV)
        by = torch.zeros((Nx, Ny + 1), dtype=torch.float64, device=DEV)
        M.initialize_solver(gres, scale, float(g["mu"]), T(v), T(g["in_vy"], torch.float64), T(s), None, T(vol), bx, by)
        out.append(N(bx))
        ex, ey = np.zeros((Nx + 1, Ny)), np.zeros((Nx, Ny + 1))
        V.rhs(gres, scale, float(g["mu"]), v, g["in_vy"], s, vol, ex, ey)
        assert np.array_equal(N(bx), ex) and np.array_equal(N(by), ey)
    assert out[1][x, y] != out[0][x, y]
    # and the class solve does not touch solid faces before the RHS either: its b equals the direct RHS of the raw input
    sl = _solver(gres, g)
    _solve(sl, g, T(g["in_vx"]), T(g["in_vy"]))
    bx = torch.zeros((Nx + 1, Ny), dtype=torch.float64, device=DEV)
    by = torch.zeros((Nx, Ny + 1), dtype=torch.float64, device=DEV)
    M.initialize_solver(gres, scale, float(g["mu"]), T(vx), T(g["in_vy"], torch.float64), T(s), None, T(vol), bx, by)
    assert torch.equal(sl.b_x, bx) and torch.equal(sl.b_y, by)


def test_quirk3_vol_uses_the_cell_area_times_one_eighth():
    g, gres, _, vol = case("v2d_b_24x40")
    s = _solver(gres, g)
    _solve(s, g, T(g["in_vx"]), T(g["in_vy"]))
    cs = np.asarray(g["bound_size"], np.float64) / np.asarray(gres, np.float64)
    assert s.cell_vol == float(cs[0] * cs[1])
    assert torch.equal(s.vol, T(g["lvol"] / (s.cell_vol * 0.125)))
    assert float(s.vol.max()) == pytest.approx(2.0)     # a full interior node: (area / 4) / (area / 8)


def test_quirk4_sv_lphi_save_are_not_read():
    g, gres, _, _ = case("v2d_b_24x40")
    outs = []
    for sv, lphi, save in ((sv_of(gres), T(np.ones(gres)), False), (None, None, True), ("junk", object(), "yes")):
        s = _solver(gres, g)
        vx, vy = T(g["in_vx"]), T(g["in_vy"])
        s.solve(float(g["dt"]), float(g["mu"]), float(g["rho"]), vx, vy, T(g["sphi"]), sv, lphi, T(g["lvol"]),
                tol=float(g["tol"]), save=save)
        outs.append((N(vx), N(vy), s.iterations))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2] == outs[0][2]


def test_quirk5_boundary_faces_never_written_by_the_class():
    g, gres, _, _ = case("v2d_c_33x17_mu200")
    s = _solver(gres, g)
    _solve(s, g, T(g["in_vx"]), T(g["in_vy"]))
    for a in (s.b_x, s.q_x, s.r_x, s.d_x, s.b_y, s.q_y, s.r_y, s.d_y):
        a = N(a)
        assert (a[0] == 0).all() and (a[-1] == 0).all() and (a[:, 0] == 0).all() and (a[:, -1] == 0).all()
    # x keeps the input on the boundary faces (r = d = 0 there)
    xx = N(s.x_x)
    assert np.array_equal(xx[0], g["in_vx"][0]) and np.array_equal(xx[:, -1], g["in_vx"][:, -1])


def test_quirk6_start_from_v_and_raise_before_writeback():
    g, gres, scale, vol = case("v2d_c_33x17_mu200")
    # r0 = b - A v (x = v, not zero): delta0 as the numpy restatement forms it
    fx, fy = (gres[0] + 1, gres[1]), (gres[0], gres[1] + 1)
    bx, by, qx, qy = np.zeros(fx), np.zeros(fy), np.zeros(fx), np.zeros(fy)
    vx64, vy64 = g["in_vx"].astype(np.float64), g["in_vy"].astype(np.float64)
    V.rhs(gres, scale, float(g["mu"]), vx64, vy64, g["sphi"], vol, bx, by)
    V.apply(gres, scale, float(g["mu"]), vx64, vy64, qx, qy, g["sphi"], vol)
    d0 = np.sum((bx - qx) ** 2) + np.sum((by - qy) ** 2)
    s = _solver(gres, g)
    s.max_iter = 3
    vx, vy = T(g["in_vx"]), T(g["in_vy"])
    vx0, vy0 = vx.clone(), vy.clone()
    with pytest.raises(ValueError, match="Failed to converge!"):
        _solve(s, g, vx, vy)
    assert s.iterations == 3
    assert torch.equal(vx, vx0) and torch.equal(vy, vy0)
    h = s.history
    assert h[0] == pytest.approx(d0, rel=1e-12) and len(h) == 7
    np.testing.assert_allclose(h, g["history"][:7], rtol=1e-9)


def test_quirk6_already_converged_runs_zero_iterations():
    g, gres, _, _ = case("v2d_b_24x40")
    s = _solver(gres, g)
    vx = torch.zeros(g["in_vx"].shape, dtype=torch.float64, device=DEV)
    vy = torch.zeros(g["in_vy"].shape, dtype=torch.float64, device=DEV)
    _solve(s, g, vx, vy)
    assert s.iterations == 0 and list(s.history) == [0.0] and s.delta == 0.0
    assert not vx.any() and not vy.any()


def test_default_tol_is_1e_4():
    import inspect
    from solver.ViscosityCGSolver2D import ViscosityCGSolver2D
    p = inspect.signature(ViscosityCGSolver2D.solve).parameters
    assert p["tol"].default == 1e-4 and p["save"].default is False


# --------------------------------------------------------------------------- engine apply vs the direct kernel ---
GEOMS = [(1, 1), (2, 2), (1, 6), (3, 7), (5, 2), (33, 17), (64, 64), (1000, 3), (257, 130), (1024, 768)]


@pytest.mark.parametrize("gres", GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_engine_apply_equals_direct_kernel(gres, prec):
    import solver.ViscosityCGSolver2D as M
    from mfs.vcg import Vcg2dEngine
    Nx, Ny = gres
    dt = torch.float64 if prec == "fp64" else torch.float32
    rng = np.random.default_rng(Nx * 7919 + Ny)
    shp = (2 * Nx + 1, 2 * Ny + 1)
    sphi = rng.integers(-2, 4, size=shp) * 0.5                      # exact zeros among the samples
    vol = rng.uniform(0.0, 2.0, size=shp) * (rng.uniform(size=shp) < 0.9)
    scale, mu = 0.37, 12.5
    eng = Vcg2dEngine(gres, dt, DEV)
    eng.setup(scale, mu, T(sphi), T(vol))
    v, (vx, vy) = eng.new_vector()
    v.copy_(torch.as_tensor(rng.standard_normal(eng.dofs), device=DEV).to(dt))
    out_e, _ = eng.new_vector()
    out_d, (ox, oy) = eng.new_vector()
    out_e.fill_(5.0)
    out_d.fill_(5.0)
    eng.apply(v, out_e)
    M.matvecmul(gres, scale, mu, vx, vy, ox, oy, T(sphi), T(vol))
    torch.cuda.synchronize()
    assert torch.equal(out_e, out_d)
    if Nx >= 3 and Ny >= 3:
        assert (out_d != 5.0).any()


# ------------------------------------------------------------------------------------------------------- scale ---
def test_rhs_and_apply_at_1024x768_vs_numpy():
    import solver.ViscosityCGSolver2D as M
    from mfs import scenes
    gres = (1024, 768)
    sc = scenes.viscosity_scene_2d(gres, 31, mu=50.0)
    scale, vol = scale_vol(gres, sc["bound_size"], sc["dt"], sc["rho"], sc["lvol"])
    Nx, Ny = gres
    fx, fy = (Nx + 1, Ny), (Nx, Ny + 1)
    sphi, volt = T(sc["sphi"]), T(vol)
    for fn, ref in ((M.initialize_solver, V.rhs), (M.matvecmul, V.apply)):
        ox, oy = T(np.full(fx, 7.0)), T(np.full(fy, 7.0))
        ex, ey = np.full(fx, 7.0), np.full(fy, 7.0)
        if fn is M.initialize_solver:
            fn(gres, scale, sc["mu"], T(sc["vx"]), T(sc["vy"]), sphi, None, volt, ox, oy)
        else:
            fn(gres, scale, sc["mu"], T(sc["vx"]), T(sc["vy"]), ox, oy, sphi, volt)
        ref(gres, scale, sc["mu"], sc["vx"], sc["vy"], sc["sphi"], vol, ex, ey) if ref is V.rhs else \
            ref(gres, scale, sc["mu"], sc["vx"], sc["vy"], ex, ey, sc["sphi"], vol)
        close(ox, ex, 1e-12, "x")
        close(oy, ey, 1e-12, "y")


def test_solve_at_256_vs_numpy():
    from mfs import scenes
    gres = (256, 256)
    sc = scenes.viscosity_scene_2d(gres, 32, mu=5.0)
    rvx, rvy = sc["vx"].copy(), sc["vy"].copy()
    ref = V.solve(gres, sc["bound_size"], sc["dt"], sc["mu"], sc["rho"], rvx, rvy, sc["sphi"], sc["lvol"])
    from solver.ViscosityCGSolver2D import ViscosityCGSolver2D
    s = ViscosityCGSolver2D(gres, sc["bound_size"], precision="fp64", device=DEV)
    vx, vy = T(sc["vx"]), T(sc["vy"])
    s.solve(sc["dt"], sc["mu"], sc["rho"], vx, vy, T(sc["sphi"]), None, None, T(sc["lvol"]))
    it = ref["iters"]
    assert abs(s.iterations - it) <= max(2, it // 10), (s.iterations, it)
    for a, b, what in ((s.x_x, ref["x_x"], "x_x"), (s.x_y, ref["x_y"], "x_y"), (vx, rvx, "vx"), (vy, rvy, "vy")):
        close(a, b, 1e-6, what)
