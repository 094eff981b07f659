"""PressureCGSolver2D on the MI355X against the numpy oracle (oracle/mfs_oracle.py) beyond the two goldens: every dtype
code of the module functions, fp32 state, production-size grids (grid-stride apply, vector-phase tails), level-set
edges, loop control, reuse, degenerate grids and stale boundary values of the shared buffer.  The oracle computes in
fp64 on the inputs rounded to the dtype they are stored in.  No engine forms exist for the 2D solver, so nothing here
asks for the default engine: the file also runs against another build of the library (MFS_LIB).

Tolerances (stated, with their basis):
  module functions, fp64 output   1e-12 of the array maximum (same fp64 operations in the same order; FMA contraction).
  module functions, fp32 output   <= 1 fp32 ulp from the fp64 oracle value rounded to fp32 (the kernels compute in
                                  fp64 and round once at the store).
  untouched entries               the sentinel / the input, bit for bit.
  fixed-count solves              history, x, r, d, q against the oracle's cg started from the GPU's stored b, wx, wy:
                                  fp64 state 10 iterations at 1e-8 (the window of test_pressure2d_gpu.py; vectors of
                                  their maximum), fp32 state 8 iterations, history at 1e-5, vectors at VEC_F32 = 2e-4
                                  (widened from 1e-5: the 1536 x 1001 scene amplifies rounding ~1000x more than 1024^2
                                  -- fp64 r 4.1e-12 there against 3.1e-15 -- and its fp32 r measured 6.0e-5, x 1.5e-5).
                                  vx, vy = the oracle's update applied to the GPU's x at 1e-12 (fp64 velocities).
  true residual                   b - A x_gpu (oracle, fp64) against the GPU's r: fp64 state 1e-9 of max|b|; fp32
                                  state 5e-5 of max|b| (x and r are rounded to fp32 every iteration, so the recursive r
                                  drifts from the true one).  delta = sum(r^2) of the returned r to 1e-12.
  converged solves                oracle's cg from the GPU's stored b, wx, wy (in fp32 state `w < 1` and b see the
                                  rounded weights); iterations within max(2, 10 %) in fp64, -20 % .. +50 % in fp32 (as
                                  test_pressure_gpu.py: fp32 storage needs more iterations for the ABSOLUTE tol); x at
                                  1e-4 of its maximum; vx, vy = the oracle's update of the GPU's x at 1e-12.
  loop control / reuse / streams  bit for bit (the partials group identically whatever the host does).
Measured on MI355X (worst over the file): module functions fp64 2.0e-16, fp32 0 ulps; fixed-count fp64 history 7.0e-15,
vectors 4.4e-12, true residual 5.5e-15; fp32 history 1.5e-7, true residual 8.9e-6 (4096^2); converged x fp64 2.6e-6,
fp32 1.4e-6, fp32 iterations +10 .. +20 %; thin-grid goldens 6.8e-7 (THIN_*).
"""
import functools

import numpy as np
import pytest
import torch

from conftest import golden, golden_names
from mfs import scenes
from oracle import mfs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
NPDT = {F32: np.float32, F64: np.float64}
SENT = -7.25
HIST = {F64: (10, 1e-8), F32: (8, 1e-5)}       # state dtype -> (iterations compared, rtol)
VEC_F32 = 2e-4         # fp32 state, x r d q after 8 iterations (of their maximum); measured: see the module docstring
TRUE_RES_F64 = 1e-9
TRUE_RES_F32 = 5e-5
THIN_WINDOW, THIN_RTOL = 5, 1e-8                # p2dt_*: leading iterations at 1e-8, the whole history at 1e-5


def T(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def N(t):
    return t.detach().cpu().to(F64).numpy()


def rounded(a, dt):
    """the value the kernel reads from an array stored in dtype dt"""
    return np.asarray(a, np.float64).astype(NPDT[dt]).astype(np.float64)


def check_values(gpu, ref, mask, what):
    """entries in `mask`: fp64 at 1e-12 of the maximum, fp32 within one ulp of the rounded fp64 value"""
    g, ref = N(gpu)[mask], np.asarray(ref, np.float64)[mask]
    if gpu.dtype == F64:
        err = np.abs(g - ref).max(initial=0.0) / max(np.abs(ref).max(initial=0.0), 1e-300)
        note("module f64 rel", err)
        assert err <= 1e-12, f"{what}: {err:.3e}"
    else:
        r32 = ref.astype(np.float32)
        ulps = (np.abs(g - r32.astype(np.float64)) / np.spacing(np.abs(r32)).astype(np.float64)).max(initial=0.0)
        note("module f32 ulps", ulps)
        assert ulps <= 1.0, f"{what}: {ulps:.2f} fp32 ulps"


WORST = {}


def note(key, v):
    """the worst error seen per kind (printed with -s: the measured values quoted in the module docstring)"""
    if v > WORST.get(key, -1.0):
        WORST[key] = float(v)
        print(f"\n[worst] {key}: {v:.3e}")


def check_untouched(gpu, mask, value, what):
    """entries outside `mask` keep `value` (an array or a scalar) bit for bit"""
    g = gpu.detach().cpu()
    v = torch.as_tensor(np.broadcast_to(np.asarray(value), g.shape)).to(g.dtype)
    keep = torch.as_tensor(~mask)
    gi = g.view(torch.int32 if g.dtype == F32 else torch.int64)
    vi = v.contiguous().view(torch.int32 if g.dtype == F32 else torch.int64)
    assert torch.equal(gi[keep], vi[keep]), f"{what}: an entry the reference never writes changed"


def patterns(names):
    """all-fp64, all-fp32, and every one-argument-differs pattern; any two arguments differ in at least one"""
    out = [{n: F64 for n in names}, {n: F32 for n in names}]
    for n in names:
        out.append({m: (F32 if m == n else F64) for m in names})
        out.append({m: (F64 if m == n else F32) for m in names})
    for a in names:
        for b in names:
            assert a == b or any(p[a] != p[b] for p in out)
    return out


def pid(p):
    return ",".join(f"{k}{'32' if v == F32 else '64'}" for k, v in p.items())


# ------------------------------------------------------------------------------------------------ scenes ---
@functools.lru_cache(maxsize=8)
def edge_scene(gres):
    return scenes.pressure_scene_2d_edges(gres, seed=sum(gres))


@functools.lru_cache(maxsize=4)
def smooth_scene(gres):
    return scenes.pressure_scene_2d(gres, seed=gres[0] % 97, solid_velocity=True)


def interior(gres):
    m = np.zeros(gres, dtype=bool)
    m[1:gres[0] - 1, 1:gres[1] - 1] = True
    return m


def update_masks(gres, lphi):
    """faces solver/PressureCGSolver2D.py:102-120 writes: cells x >= 1, y >= 1, the face's two cells not both air"""
    Nx, Ny = gres
    liq = np.asarray(lphi) < 0
    mx, my = np.zeros((Nx + 1, Ny), bool), np.zeros((Nx, Ny + 1), bool)
    mx[1:Nx, 1:Ny] = liq[1:, 1:] | liq[:-1, 1:]
    my[1:Nx, 1:Ny] = liq[1:, 1:] | liq[1:, :-1]
    return mx, my


MODULE_SHAPES = [(33, 17), (3, 257), (257, 3), (1024, 768), (1536, 1001)]
MODULE_CASES = [("edges", s) for s in MODULE_SHAPES] + [("smooth", (1024, 768))]


def module_scene(kind, gres):
    return edge_scene(gres) if kind == "edges" else smooth_scene(gres)


# ------------------------------------------------------------------------- 1. module functions x dtype codes ---
@pytest.mark.parametrize("kind,gres", MODULE_CASES, ids=[f"{k}-{g[0]}x{g[1]}" for k, g in MODULE_CASES])
def test_module_functions_every_dtype_code(kind, gres):
    import solver.PressureCGSolver2D as P
    import solver.SolidFraction2D as S
    sc = module_scene(kind, gres)
    Nx, Ny = gres
    fx, fy = (Nx + 1, Ny), (Nx, Ny + 1)
    cs = np.asarray(sc["bound_size"], np.float64) / np.asarray(gres, np.float64)
    rng = np.random.default_rng(Nx * 7 + Ny)
    wx64, wy64 = np.zeros(fx), np.zeros(fy)
    O.compute_solid_frac2d(gres, sc["sphi"], wx64, wy64)

    # compute_solid_frac: sphi, w
    for p in patterns(["sphi", "w"]):
        wx, wy = (torch.full(s, SENT, dtype=p["w"], device=DEV) for s in (fx, fy))
        S.compute_solid_frac(gres, T(sc["sphi"], p["sphi"]), wx, wy)
        rx, ry = np.full(fx, np.nan), np.full(fy, np.nan)
        O.compute_solid_frac2d(gres, rounded(sc["sphi"], p["sphi"]), rx, ry)
        for g, r, what in ((wx, rx, "wx"), (wy, ry, "wy")):
            m = ~np.isnan(r)
            check_values(g, r, m, f"solid_frac {pid(p)} {what}")
            check_untouched(g, m, SENT, f"solid_frac {pid(p)} {what}")

    # initialize_solver: v, sv, lphi, w, b
    for p in patterns(["v", "sv", "lphi", "w", "b"]):
        args = dict(vx=rounded(sc["vx"], p["v"]), vy=rounded(sc["vy"], p["v"]), sv=rounded(sc["sv"], p["sv"]),
                    lphi=rounded(sc["lphi"], p["lphi"]), wx=rounded(wx64, p["w"]), wy=rounded(wy64, p["w"]))
        b = torch.full(gres, SENT, dtype=p["b"], device=DEV)
        P.initialize_solver(cs, gres, T(args["vx"], p["v"]), T(args["vy"], p["v"]), T(sc["sphi"]),
                            T(args["sv"], p["sv"]), T(args["lphi"], p["lphi"]), b, T(args["wx"], p["w"]),
                            T(args["wy"], p["w"]))
        rb = np.full(gres, SENT)
        O.pressure_rhs2d(cs, gres, args["vx"], args["vy"], None, args["sv"], args["lphi"], rb, args["wx"], args["wy"])
        check_values(b, rb, interior(gres), f"rhs {pid(p)}")
        check_untouched(b, interior(gres), SENT, f"rhs {pid(p)}")

    # matvecmul: v (= out), w, lphi; v random everywhere, boundary cells included
    v0 = rng.standard_normal(gres)
    for p in patterns(["v", "w", "lphi"]):
        out = torch.full(gres, SENT, dtype=p["v"], device=DEV)
        lp, wx, wy = rounded(sc["lphi"], p["lphi"]), rounded(wx64, p["w"]), rounded(wy64, p["w"])
        P.matvecmul(gres, T(v0, p["v"]), out, T(wx, p["w"]), T(wy, p["w"]), T(lp, p["lphi"]))
        ro = np.full(gres, SENT)
        O.pressure_apply2d(gres, rounded(v0, p["v"]), ro, wx, wy, lp)
        check_values(out, ro, interior(gres), f"apply {pid(p)}")
        check_untouched(out, interior(gres), SENT, f"apply {pid(p)}")

    # apply_pressure: v, pv, w, sv, lphi (velocities in place; the faces it skips keep their input bits)
    pv0 = rng.standard_normal(gres)
    mx, my = update_masks(gres, sc["lphi"])
    for p in patterns(["v", "pv", "w", "sv", "lphi"]):
        vx0, vy0 = rounded(sc["vx"], p["v"]), rounded(sc["vy"], p["v"])
        args = dict(pv=rounded(pv0, p["pv"]), wx=rounded(wx64, p["w"]), wy=rounded(wy64, p["w"]),
                    sv=rounded(sc["sv"], p["sv"]), lphi=rounded(sc["lphi"], p["lphi"]))
        vx, vy = T(vx0, p["v"]), T(vy0, p["v"])
        P.apply_pressure(gres, cs, vx, vy, T(args["pv"], p["pv"]), T(args["wx"], p["w"]), T(args["wy"], p["w"]),
                         T(args["sv"], p["sv"]), T(args["lphi"], p["lphi"]))
        rx, ry = vx0.copy(), vy0.copy()
        O.pressure_update2d(gres, cs, rx, ry, args["pv"], args["wx"], args["wy"], args["sv"], args["lphi"])
        for g, r, m, v0_, what in ((vx, rx, mx, vx0, "vx"), (vy, ry, my, vy0, "vy")):
            check_values(g, r, m, f"update {pid(p)} {what}")
            check_untouched(g, m, v0_.astype(NPDT[p["v"]]), f"update {pid(p)} {what}")


# ------------------------------------------------------------------ 2./3. fixed-count solves at production size ---
def solve_gpu(sc, prec, max_iter, tol=0.0, check_every=32, sv_dev=None):
    import solver.CGSolverBuffer as B
    import solver.PressureCGSolver2D as P
    gres = sc["gres"]
    buf = B.CGSolverBuffer(gres, precision=prec, device=DEV)
    s = P.PressureCGSolver2D(buf, gres, sc["bound_size"], check_every=check_every)
    s.max_iter = max_iter
    vx, vy = T(sc["vx"]), T(sc["vy"])
    sv = T(sc["sv"]) if sv_dev is None else sv_dev
    s.solve(vx, vy, T(sc["sphi"]), sv, T(sc["lphi"]), tol=tol)
    torch.cuda.synchronize()
    return s, buf, vx, vy


def oracle_cg(gres, b, wx, wy, lphi, tol, max_iter):
    x, d, r, q = (np.zeros(gres) for _ in range(4))
    b = b.copy()
    hist = []
    ap = lambda V, Q: O.pressure_apply2d(gres, V[0], Q[0], wx, wy, lphi)  # noqa: E731
    it, delta, _, _ = O.cg(ap, b, x, d, r, q, tol, max_iter, hist, raise_on_fail=False)
    return dict(it=it, delta=delta, hist=np.array(hist), x=x, d=d, r=r, q=q, b=b)


def true_residual(gres, b, x, wx, wy, lphi):
    ax = np.zeros(gres)
    O.pressure_apply2d(gres, x, ax, wx, wy, lphi)
    return b - ax


def check_true_residual(s, buf, wx, wy, lphi, what):
    gres = s._g
    b, r = N(buf.b), N(buf.r)
    rt = true_residual(gres, b, N(s.x), wx, wy, lphi)
    bound = (TRUE_RES_F64 if buf.r.dtype == F64 else TRUE_RES_F32) * np.abs(b).max()
    err = np.abs(r - rt).max()
    note(f"true residual {buf.r.dtype}", err / np.abs(b).max())
    assert err <= bound, f"{what}: |r - (b - A x)| = {err:.3e} > {bound:.3e}"
    rr = float(np.sum(r * r))
    assert s.delta == pytest.approx(rr, rel=1e-12, abs=1e-300), f"{what}: delta {s.delta!r} vs sum r^2 {rr!r}"
    return err / max(np.abs(b).max(), 1e-300)


@functools.lru_cache(maxsize=2)
def fixed_reference(gres, prec, n_iter):
    """the GPU's b, wx, wy (default engine) and the oracle's cg from them"""
    sc = fixed_scene(gres)
    s, buf, vx, vy = solve_gpu(sc, prec, n_iter, sv_dev=fixed_sv(gres))
    wx, wy = N(s.wx), N(s.wy)
    ref = oracle_cg(gres, N(buf.b), wx, wy, sc["lphi"], 0.0, n_iter)
    return N(buf.b), wx, wy, ref


@functools.lru_cache(maxsize=2)
def fixed_scene(gres):
    if gres == (4096, 4096):                   # the bench tool's scene (tools/visc2d_bench.py --pressure)
        return scenes.pressure_scene_2d(gres, 1)
    return smooth_scene(gres)


def fixed_sv(gres):
    if gres == (4096, 4096):                   # all zeros there: no 1 GB host-to-device copy
        return torch.zeros((2 * gres[0] + 1, 2 * gres[1] + 1, 2), dtype=F64, device=DEV)
    return None


# (gres, state, iterations, MFS_VEC_BLOCKS_PER_CU): 1 and 32 change how many grid strides each block of the apply and
# the vector phases makes and how the partials group (default 8: 2 048 blocks, every cell past 524 288 by the stride)
FIXED = [((1024, 1024), "fp64", 10, None), ((1024, 1024), "fp64", 10, "1"), ((1024, 1024), "fp64", 10, "32"),
         ((1024, 1024), "fp32", 8, None), ((1024, 1024), "fp32", 8, "1"), ((1024, 1024), "fp32", 8, "32"),
         ((1536, 1001), "fp64", 10, None), ((1536, 1001), "fp32", 8, None), ((4096, 4096), "fp32", 5, None)]


@pytest.mark.parametrize("gres,prec,n_iter,blocks_per_cu", FIXED,
                         ids=[f"{g[0]}x{g[1]}-{p}-bpc{k or 'default'}" for g, p, _, k in FIXED])
def test_fixed_count_solve_vs_oracle(gres, prec, n_iter, blocks_per_cu, monkeypatch):
    b_ref, wx, wy, ref = fixed_reference(gres, prec, n_iter)
    if blocks_per_cu is not None:
        monkeypatch.setenv("MFS_VEC_BLOCKS_PER_CU", blocks_per_cu)
    sc = fixed_scene(gres)
    s, buf, vx, vy = solve_gpu(sc, prec, n_iter, sv_dev=fixed_sv(gres))
    dt = buf.b.dtype
    assert s.iterations == n_iter and not s.converged
    assert np.array_equal(N(buf.b), b_ref)
    w, rtol = HIST[dt]
    assert n_iter <= w
    h = s.history
    assert len(h) == 2 * n_iter + 1
    note(f"fixed history {prec}", np.max(np.abs(h - ref["hist"]) / np.abs(ref["hist"])))
    np.testing.assert_allclose(h, ref["hist"], rtol=rtol)
    for name, g in (("x", s.x), ("r", buf.r), ("d", buf.d), ("q", buf.q)):
        r = ref[name]
        err = np.abs(N(g) - r).max() / np.abs(r).max()
        note(f"fixed {name} {prec}", err)
        assert err <= (rtol if dt == F64 else VEC_F32), f"{name}: {err:.3e}"
    check_true_residual(s, buf, wx, wy, sc["lphi"], f"{gres} {prec}")
    # the velocity update from the GPU's own x
    cs = np.asarray(sc["bound_size"], np.float64) / np.asarray(gres, np.float64)
    rx, ry = sc["vx"].copy(), sc["vy"].copy()
    sv = np.broadcast_to(np.zeros(()), (2 * gres[0] + 1, 2 * gres[1] + 1, 2)) if fixed_sv(gres) is not None else sc["sv"]
    O.pressure_update2d(gres, cs, rx, ry, N(s.x), wx, wy, sv, sc["lphi"])
    for g, r, what in ((vx, rx, "vx"), (vy, ry, "vy")):
        err = np.abs(N(g) - r).max()
        assert err <= 1e-12 * np.abs(r).max(), f"{what}: {err:.3e}"


# ---------------------------------------------------------------------------- 4. converged solves vs oracle ---
# tol: 190-270 oracle iterations (fp64); the x of two solves stopped at a looser tol differ by more than 1e-4
CONVERGED = [("smooth128", (128, 128), 1e-2), ("smooth200x90", (200, 90), 1e-2), ("edges65x47", (65, 47), 1e-4)]


def converged_scene(kind, gres):
    return edge_scene(gres) if kind.startswith("edges") else smooth_scene(gres)


def iterations_close(gpu, ref, dt):
    """fp64 within max(2, 10 %); fp32 storage needs more iterations to reach the ABSOLUTE tol (as in
    test_pressure_gpu.py: -20 % .. +50 %)"""
    if dt == F64:
        return abs(gpu - ref) <= max(2, ref // 10)
    return ref - max(2, ref // 5) <= gpu <= ref + max(2, ref // 2)


def check_update_from_gpu_x(sc, s, vx, vy, sv=None):
    """the velocities equal the oracle's update applied to the GPU's own x, wx, wy"""
    gres = s._g
    cs = np.asarray(sc["bound_size"], np.float64) / np.asarray(gres, np.float64)
    rx, ry = sc["vx"].copy(), sc["vy"].copy()
    O.pressure_update2d(gres, cs, rx, ry, N(s.x), N(s.wx), N(s.wy), sc["sv"] if sv is None else sv, sc["lphi"])
    for g, r, what in ((vx, rx, "vx"), (vy, ry, "vy")):
        err = np.abs(N(g) - r).max()
        assert err <= 1e-12 * np.abs(r).max(), f"{what}: {err:.3e}"


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
@pytest.mark.parametrize("kind,gres,tol", CONVERGED, ids=[c[0] for c in CONVERGED])
def test_converged_solve_vs_oracle(kind, gres, tol, prec):
    sc = converged_scene(kind, gres)
    s, buf, vx, vy = solve_gpu(sc, prec, int(np.prod(gres)), tol=tol)
    o = oracle_cg(gres, N(buf.b), N(s.wx), N(s.wy), sc["lphi"], tol, int(np.prod(gres)))
    print(f"\n[iters] {kind} {prec}: gpu {s.iterations} oracle {o['it']}")
    assert 30 <= o["it"] <= 300 and o["hist"][-1] < tol ** 2
    assert s.converged and iterations_close(s.iterations, o["it"], buf.r.dtype), (s.iterations, o["it"])
    err = np.abs(N(s.x) - o["x"]).max() / np.abs(o["x"]).max()
    note(f"converged x {prec}", err)
    assert err <= 1e-4, f"x: {err:.3e}"
    check_true_residual(s, buf, N(s.wx), N(s.wy), sc["lphi"], f"{kind} {prec}")
    check_update_from_gpu_x(sc, s, vx, vy)


# --------------------------------------------------------------------------------------- 5. loop control ---
def mid_batch_tol(hist, k):
    """a tol whose first crossing in the oracle's history is iteration k (geometric mean of the two deltas)"""
    return float(np.sqrt(np.sqrt(hist[2 * k] * hist[2 * (k - 1)])))


def test_check_every_does_not_change_anything():
    g = golden("p2d_b_24x20_sv")
    gres = tuple(int(v) for v in g["gres"])
    sc = dict(gres=gres, bound_size=tuple(g["bound_size"]), vx=g["in_vx"], vy=g["in_vy"], sphi=g["sphi"],
              sv=g["sv"], lphi=g["lphi"])
    k = 37                                      # converges mid-batch for check_every 3 and 32
    tol = mid_batch_tol(g["history"], k)
    for max_iter, tol_ in ((45, 0.0), (int(np.prod(gres)), tol)):
        runs = {}
        for ce in (1, 3, 32, 1000):
            s, buf, vx, vy = solve_gpu(sc, "fp64", max_iter, tol=tol_, check_every=ce)
            runs[ce] = (s.iterations, s.converged, s.history, N(s.x), N(buf.r), N(buf.d), N(vx), N(vy))
        it0 = runs[1][0]
        if tol_ == 0.0:
            assert it0 == max_iter and not runs[1][1]
        else:
            assert runs[1][1] and it0 % 3 != 0 and it0 % 32 != 0 and abs(it0 - k) <= 2, it0
        for ce, r in runs.items():
            assert r[0] == it0 and r[1] == runs[1][1], (ce, r[0], it0)
            for a, b_ in zip(r[2:], runs[1][2:]):
                assert np.array_equal(a, b_), f"check_every={ce} differs from check_every=1"


def test_max_iter_hit_reports_not_converged():
    sc = edge_scene((33, 17))
    for m in (1, 5, 33):
        s, _, _, _ = solve_gpu(sc, "fp32", m, tol=1e-9, check_every=4)
        assert s.iterations == m and not s.converged and len(s.history) == 2 * m + 1


# ------------------------------------------------------------------------------------ 6. restart and reuse ---
def snapshot(s, buf, vx, vy):
    return [s.iterations, s.history, N(s.x), N(buf.r), N(buf.d), N(vx), N(vy)]


def same(a, b):
    assert a[0] == b[0]
    for u, v in zip(a[1:], b[1:]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_restart_reuse_and_side_stream(prec):
    import solver.CGSolverBuffer as B
    import solver.PressureCGSolver2D as P
    gres = (97, 61)
    a = smooth_scene(gres)
    bsc = dict(a, vx=a["vx"][::-1].copy(), vy=-a["vy"], sphi=a["sphi"] + 0.02, lphi=a["lphi"] - 0.07,
               sv=a["sv"] * 0.5)
    tol = 1.0
    fresh_a = snapshot(*solve_gpu(a, prec, int(np.prod(gres)), tol=tol))
    fresh_b = snapshot(*solve_gpu(bsc, prec, int(np.prod(gres)), tol=tol))
    assert fresh_a[0] > 10 and fresh_b[0] > 10

    def run(s, buf, sc):
        vx, vy = T(sc["vx"]), T(sc["vy"])
        s.solve(vx, vy, T(sc["sphi"]), T(sc["sv"]), T(sc["lphi"]), tol=tol)
        torch.cuda.synchronize()
        return snapshot(s, buf, vx, vy)

    buf = B.CGSolverBuffer(gres, precision=prec, device=DEV)
    s = P.PressureCGSolver2D(buf, gres, a["bound_size"])
    s.x.copy_(T(np.random.default_rng(3).uniform(-1e3, 1e3, gres)))       # finite garbage: x *= 0 restarts
    same(run(s, buf, a), fresh_a)
    same(run(s, buf, bsc), fresh_b)                                         # one object, scene A then scene B
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vx, vy = T(a["vx"]), T(a["vy"])
        s.solve(vx, vy, T(a["sphi"]), T(a["sv"]), T(a["lphi"]), tol=tol)
    torch.cuda.synchronize()
    same(snapshot(s, buf, vx, vy), fresh_a)


# --------------------------------------------------------------------------- 7. degenerate and uniform scenes ---
@pytest.mark.parametrize("gres", [(1, 1), (1, 7), (2, 5), (5, 2), (3, 3)])
def test_degenerate_grids(gres):
    sc = scenes.pressure_scene_2d(gres, 5, solid_velocity=True)
    o = O.PressureCGSolver2D(gres, sc["bound_size"])
    ovx, ovy = sc["vx"].copy(), sc["vy"].copy()
    o.solve(ovx, ovy, sc["sphi"], sc["sv"], sc["lphi"], tol=1e-6)
    s, buf, vx, vy = solve_gpu(sc, "fp64", int(np.prod(gres)), tol=1e-6)
    if min(gres) < 3:                                   # no interior cell
        assert s.iterations == 0 and s.converged and list(s.history) == [0.0] and not N(s.x).any()
        assert o.iterations == 0
    else:                                               # one interior cell
        assert s.iterations == o.iterations
        np.testing.assert_allclose(s.history, o.history, rtol=1e-12, atol=1e-12 * o.history[0])
        np.testing.assert_allclose(N(s.x), o.x, rtol=1e-12)
    np.testing.assert_allclose(N(vx), ovx, rtol=0, atol=1e-12 * np.abs(ovx).max())
    np.testing.assert_allclose(N(vy), ovy, rtol=0, atol=1e-12 * np.abs(ovy).max())


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_all_air_changes_no_face(prec):
    sc = dict(smooth_scene((97, 61)))
    sc["lphi"] = np.full((97, 61), 0.25)
    s, buf, vx, vy = solve_gpu(sc, prec, 100, tol=1e-6)
    assert s.iterations == 0 and s.converged and list(s.history) == [0.0]
    assert torch.equal(vx, T(sc["vx"])) and torch.equal(vy, T(sc["vy"]))


@pytest.mark.parametrize("prec", ["fp64", "fp32"])
def test_all_fluid_vs_oracle(prec):
    gres = (40, 30)
    sc = dict(scenes.pressure_scene_2d(gres, 14, solid_velocity=True), lphi=-np.ones(gres))
    tol = 1.0
    s, buf, vx, vy = solve_gpu(sc, prec, int(np.prod(gres)), tol=tol)
    o = oracle_cg(gres, N(buf.b), N(s.wx), N(s.wy), sc["lphi"], tol, int(np.prod(gres)))
    print(f"\n[iters] all-fluid {prec}: gpu {s.iterations} oracle {o['it']}")
    assert s.converged and iterations_close(s.iterations, o["it"], buf.r.dtype), (s.iterations, o["it"])
    w, rtol = HIST[buf.r.dtype]
    np.testing.assert_allclose(s.history[:2 * w + 1], o["hist"][:2 * w + 1], rtol=rtol)
    err = np.abs(N(s.x) - o["x"]).max() / np.abs(o["x"]).max()
    note(f"all-fluid x {prec}", err)
    assert err <= 1e-4
    check_true_residual(s, buf, N(s.wx), N(s.wy), sc["lphi"], f"all-fluid {prec}")
    check_update_from_gpu_x(sc, s, vx, vy)


# --------------------------------------------------------------------------------- 8. stale boundary values ---
@pytest.mark.parametrize("name", golden_names("p2dq_"))
def test_stale_boundary_vs_golden(name):
    import solver.CGSolverBuffer as B
    import solver.PressureCGSolver2D as P
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    buf = B.CGSolverBuffer(gres, precision="fp64", device=DEV)
    for k in "bqdr":
        getattr(buf, k).copy_(T(g["pre_" + k]))
    s = P.PressureCGSolver2D(buf, gres, g["bound_size"])
    s.max_iter = int(g["max_iter"])
    vx, vy = T(g["in_vx"]), T(g["in_vy"])
    s.solve(vx, vy, T(g["sphi"]), T(g["sv"]), T(g["lphi"]), tol=0.0)
    torch.cuda.synchronize()
    assert s.iterations == int(g["iters"]) and not s.converged
    np.testing.assert_allclose(s.history[:21], g["history"][:21], rtol=1e-8)
    for a, k in ((s.x, "x"), (buf.b, "b"), (buf.d, "d"), (buf.r, "r"), (buf.q, "q"), (vx, "out_vx"), (vy, "out_vy")):
        ref = g[k]
        err = np.abs(N(a) - ref).max()
        assert err <= 1e-4 * np.abs(ref).max(), f"{k}: {err:.3e}"
    ring = ~interior(gres)
    check_untouched(buf.q, ~ring, g["pre_q"], "q ring")


# ---------------------------------------------------------------------------------- thin-grid edge goldens ---
@pytest.mark.parametrize("name", golden_names("p2dt_"))
def test_thin_grid_golden(name):
    """one interior column / row (mfs.scenes.pressure_scene_2d_edges): module functions and the class against the
    golden.  History: iterations 6-7 of these 7-iteration solves left the 1e-8 window on MI355X (measured 6.8e-7; the
    residual is 1e-4..1e-6 of its start there and the clamped faces weigh 100), so the leading THIN_WINDOW iterations
    at 1e-8 and the whole history at 1e-5."""
    import solver.CGSolverBuffer as B
    import solver.PressureCGSolver2D as P
    import solver.SolidFraction2D as S
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    Nx, Ny = gres
    wx = torch.full((Nx + 1, Ny), SENT, dtype=F64, device=DEV)
    wy = torch.full((Nx, Ny + 1), SENT, dtype=F64, device=DEV)
    S.compute_solid_frac(gres, T(g["sphi"]), wx, wy)
    mx, my = np.zeros((Nx + 1, Ny), bool), np.zeros((Nx, Ny + 1), bool)
    mx[:Nx, :Ny - 1], my[:Nx - 1, :Ny] = True, True
    check_values(wx, g["wx"], mx, "wx")
    check_values(wy, g["wy"], my, "wy")
    b = torch.full(gres, SENT, dtype=F64, device=DEV)
    P.initialize_solver(g["bound_size"] / g["gres"], gres, T(g["in_vx"]), T(g["in_vy"]), T(g["sphi"]), T(g["sv"]),
                        T(g["lphi"]), b, T(g["wx"]), T(g["wy"]))
    check_values(b, g["b"], interior(gres), "rhs")
    q = torch.full(gres, SENT, dtype=F64, device=DEV)
    P.matvecmul(gres, T(g["b"]), q, T(g["wx"]), T(g["wy"]), T(g["lphi"]))
    check_values(q, g["q1"], interior(gres), "apply")
    buf = B.CGSolverBuffer(gres, precision="fp64", device=DEV)
    s = P.PressureCGSolver2D(buf, gres, g["bound_size"])
    vx, vy = T(g["in_vx"]), T(g["in_vy"])
    s.solve(vx, vy, T(g["sphi"]), T(g["sv"]), T(g["lphi"]), tol=float(g["tol"]))
    h, hg = s.history, g["history"]
    n = 2 * THIN_WINDOW + 1
    note("thin history", np.max(np.abs(h[:len(hg)] - hg[:len(h)]) / np.abs(hg[:len(h)])))
    np.testing.assert_allclose(h[:n], hg[:n], rtol=THIN_RTOL)
    assert s.converged and abs(s.iterations - int(g["iters"])) <= max(2, int(g["iters"]) // 10)
    m = min(len(h), len(hg))
    np.testing.assert_allclose(h[:m], hg[:m], rtol=1e-5)
    for a, k in ((s.x, "x"), (vx, "out_vx"), (vy, "out_vy")):
        err = np.abs(N(a) - g[k]).max()
        assert err <= 1e-4 * np.abs(g[k]).max(), f"{k}: {err:.3e}"
