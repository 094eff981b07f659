"""The HIP kernels of the 2D time step (csrc/mfs_notebook2d.hip through notebook_kernels2d.py) on the MI355X against their
numpy restatement (tests/notebook2d_numpy.py, which tests/test_notebook2d_oracle.py pins to the 3D oracle).

Scatters (p2g, fluid volume) add with hardware fp atomics in arbitrary order.  Tolerance per node, derived as in
tests/test_particles_stress_gpu.py: a node receives K terms t_i, S = sum |t_i| (both from the restatement's `stats`); adding
them into an array of unit roundoff u (2^-24 float32, 2^-53 float64) rounds each term once on conversion and once per add:
|got - exact| <= (K + 1) u S (1 + K u); asserted: (K + 2) u S, and exactly 0.0 where K == 0.  The reference is the float64
sum in particle order.  The gather, the level set, extrapolate and the boundary condition are order-fixed: the tolerances
of their 3D twins in tests/test_particles_gpu.py and tests/test_notebook_gpu.py."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import notebook2d_numpy as R
import notebook_kernels2d as K
from mfs import _lib, scenes, tensors as TT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
NS = types.SimpleNamespace
TD = {np.float32: torch.float32, np.float64: torch.float64}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
DTYPES = [np.float32, np.float64]
ids = lambda prefix: (lambda d: prefix + ("32" if d is np.float32 else "64"))  # noqa: E731
# grid, particle count (None: the whole particle_scene_2d): odd extents that are no multiple of the wavefront in y, degenerate
# aspects, one particle, less than a wavefront, more than a block
CASES = [((12, 16), None), ((33, 21), None), ((3, 130), None), ((130, 3), None), ((33, 21), 1), ((33, 21), 63), ((33, 21), 257)]
case_id = lambda c: "%dx%d-P%s" % (c[0][0], c[0][1], "all" if c[1] is None else c[1])  # noqa: E731
_SCENES = {}


def scene(case, pdt):
    """the scene's particle arrays at the particle dtype (float32 arrays are the float64 ones rounded), built once"""
    key = (case, pdt)
    if key not in _SCENES:
        gres, P = case
        sc = dict(scenes.particle_scene_2d(gres, seed=1))
        for k in ("px", "pm", "pv", "pcx", "pcy"):
            sc[k] = sc[k][:P].astype(pdt)
        _SCENES[key] = sc
    return _SCENES[key]


def face_shape(gres, a):
    return tuple(int(v) for v in np.array(gres) + np.eye(2, dtype=int)[a])


def grid_of(sc, gdt, fill=0.0):
    def comp(a):
        return NS(bias=np.asarray(R.BIAS[a], np.float32), m=torch.full(face_shape(sc["gres"], a), fill, dtype=TD[gdt], device=DEV),
                  v=torch.full(face_shape(sc["gres"], a), fill, dtype=TD[gdt], device=DEV))
    return NS(resolution=sc["gres"], bound_min=sc["bound_min"], bound_size=sc["bound_size"], cell_size=sc["cell_size"],
              x=comp(0), y=comp(1))


def particles_of(sc):
    return NS(num_particles=len(sc["px"]), x=T(sc["px"]), m=T(sc["pm"]), v=T(sc["pv"]), cx=T(sc["pcx"]), cy=T(sc["pcy"]),
              vol=sc["pvol"])


def _within(got, want, Kn, S, u, what):
    got = np.asarray(got)
    err, bound = np.abs(got.astype(np.float64) - want), (Kn + 2) * u * S
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(ratio.argmax(), ratio.shape)
    print(f"RATIO {what}: worst err / bound {ratio.max():.4f} at {worst} (K {Kn[worst]})")
    assert ratio.max() <= 1.0, (f"{what}: worst err / bound {ratio.max():.4g} at node {worst}: got {got[worst]!r} want {want[worst]!r} "
                                f"K {Kn[worst]} S {S[worst]!r}; {int((ratio > 1).sum())} nodes over")
    assert (got[Kn == 0] == 0.0).all(), f"{what}: {int((got[Kn == 0] != 0).sum())} nodes without a contribution are not 0.0"


# ------------------------------------------------------------------------------------------------ scatters ---
@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_p2g_scatter_and_normalize(case, gdt, pdt):
    sc = scene(case, pdt)
    gres = sc["gres"]
    p, grid = particles_of(sc), grid_of(sc, gdt)
    K.p2g_scatter(p, grid)
    torch.cuda.synchronize()
    before = []
    for a, c in enumerate("xy"):
        gm, gv, st = np.zeros(face_shape(gres, a)), np.zeros(face_shape(gres, a)), {}
        R.p2g_scatter(sc["px"], sc["pm"], sc["pv"], sc["pc" + c], gm, gv, sc["bound_min"], gres, R.BIAS[a], sc["cell_size"], a,
                      stats=st)
        gc = getattr(grid, c)
        what = f"p2g {case_id(case)} grid {np.dtype(gdt).name} particles {np.dtype(pdt).name} g.{c}"
        _within(N(gc.m), gm, st["K"], st["S_m"], U[gdt], what + ".m")
        _within(N(gc.v), gv, st["K"], st["S_v"], U[gdt], what + ".mv")
        assert st["K"].sum() == 4 * p.num_particles
        before.append((N(gc.m), N(gc.v)))
    K.p2g_normalize(grid)                                      # the division, in the arrays' own precision: exact
    torch.cuda.synchronize()
    for (gm, gv), c in zip(before, "xy"):
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(gm > 0, gv / gm, gv)
        assert want.dtype == gdt
        np.testing.assert_array_equal(N(getattr(grid, c).v), want)
        np.testing.assert_array_equal(N(getattr(grid, c).m), gm)


@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fluid_volume(case, gdt, pdt):
    """the clamp min(., cell area) moves no value further from the reference's than the sums are apart"""
    sc = scene(case, pdt)
    vres, dcs = tuple(2 * v + 1 for v in sc["gres"]), sc["cell_size"] / 2
    fv = NS(resolution=vres, bound_min=sc["bound_min"], bound_size=sc["bound_size"], cell_size=dcs,
            vol=torch.full(vres, 3.0, dtype=TD[gdt], device=DEV))
    K.compute_fluid_volume(particles_of(sc), fv, sc["pvol"])
    torch.cuda.synchronize()
    want, st = np.zeros(vres), {}
    R.fluid_volume(sc["bound_min"], dcs, vres, sc["px"], sc["pvol"], want, stats=st)
    if case[1] is None:
        assert (want == dcs[0] * dcs[1]).any() and ((want > 0) & (want < dcs[0] * dcs[1])).any()      # clamped and partial nodes
    _within(N(fv.vol), want, st["K"], st["S_vol"], U[gdt], f"volume {case_id(case)} grid {np.dtype(gdt).name} particles {np.dtype(pdt).name}")
    assert N(fv.vol).max() <= gdt(dcs[0] * dcs[1])


# ---------------------------------------------------------------------------------- gather and level set ---
@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_g2p(case, gdt, pdt):
    """order-fixed: rtol 1e-12 as for the 3D gather (tests/test_particles_gpu.py); with float32 particle arrays every partial
    sum is rounded to float32 in the kernel and in the restatement alike"""
    sc = scene(case, pdt)
    gres = sc["gres"]
    rng = np.random.default_rng(3)
    fields = [rng.standard_normal(face_shape(gres, a)).astype(gdt) for a in range(2)]
    p, grid = particles_of(sc), grid_of(sc, gdt)
    p.v.fill_(7.0)
    for c, f in zip("xy", fields):
        getattr(grid, c).v.copy_(T(f))
    K.g2p(p, grid)
    torch.cuda.synchronize()
    P = p.num_particles
    pv, pc = np.full((P, 2), 7.0, pdt), [np.full((P, 2), 7.0, pdt) for _ in range(2)]
    for a in range(2):
        R.g2p_gather(sc["bound_min"], gres, R.BIAS[a], sc["cell_size"], a, sc["px"], pv, pc[a], fields[a])
    assert p.v.dtype == TD[pdt]
    np.testing.assert_allclose(N(p.v), pv, rtol=1e-12, atol=1e-13)
    for a, c in enumerate("xy"):
        np.testing.assert_allclose(N(getattr(p, "c" + c)), pc[a], rtol=1e-12, atol=1e-12 * np.abs(pc[a]).max())


@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_fluid_levelset(case, pdt):
    """an atomic min: exact up to sqrt vs pow (rtol 1e-13, as in 3D); with the default radius and with the 3D one"""
    sc = scene(case, pdt)
    gres, gdx = sc["gres"], sc["gdx"]
    ls = NS(resolution=gres, bound_min=sc["bound_min"], bound_size=sc["bound_size"], cell_size=sc["cell_size"],
            phi=torch.zeros(gres, dtype=torch.float64, device=DEV))
    for radius in (None, gdx * 0.5 * np.sqrt(3.0) * 1.02):
        K.compute_fluid_levelset(particles_of(sc), ls, gdx, radius=radius)
        torch.cuda.synchronize()
        want = np.zeros(gres)
        R.fluid_levelset(sc["px"], want, sc["bound_min"], sc["cell_size"], gdx, gres, radius=radius)
        np.testing.assert_allclose(N(ls.phi), want, rtol=1e-13, atol=1e-15)
    assert (want < 0).any()


def test_no_particles_is_a_clean_no_op():
    """P = 0: every entry returns MFS_OK without a launch and leaves the arrays as initialised"""
    sc = scene(((12, 16), None), np.float64)
    gres = sc["gres"]
    grid = grid_of(sc, np.float32, fill=5.0)
    e2 = lambda: torch.zeros((0, 2), dtype=torch.float64, device=DEV)  # noqa: E731
    p = NS(num_particles=0, x=e2(), m=torch.zeros(0, dtype=torch.float64, device=DEV), v=e2(), cx=e2(), cy=e2(), vol=1e-3)
    K.p2g_scatter(p, grid)
    K.g2p(p, grid)
    torch.cuda.synchronize()
    for c in (grid.x, grid.y):
        assert float(c.m.min()) == 5.0 == float(c.m.max()) and float(c.v.min()) == 5.0 == float(c.v.max())
    ls = NS(resolution=gres, bound_min=sc["bound_min"], cell_size=sc["cell_size"], phi=torch.zeros(gres, dtype=torch.float64, device=DEV))
    K.compute_fluid_levelset(p, ls, 0.1)
    assert float(ls.phi.min()) == float(ls.phi.max()) == 0.1 * 3                                 # the wrapper's pre-fill
    vres = tuple(2 * v + 1 for v in gres)
    fv = NS(resolution=vres, bound_min=sc["bound_min"], cell_size=sc["cell_size"] / 2, vol=torch.ones(vres, dtype=torch.float64, device=DEV))
    K.compute_fluid_volume(p, fv, 1e-3)
    assert float(fv.vol.abs().max()) == 0.0                                                      # the wrapper's zeroing
    # the entry points themselves: arrays exactly as they were
    lib = _lib.load()
    phi, vol = torch.full(gres, 2.5, dtype=torch.float64, device=DEV), torch.full(vres, 2.5, dtype=torch.float64, device=DEV)
    f2 = lambda a: _lib.f64x(TT.as_f64_list(a, 2))  # noqa: E731
    assert lib.mfs_fluid_levelset2d(_lib.i64x(gres), f2(sc["bound_min"]), f2(sc["cell_size"]), 0.1, None, _lib.MFS_F64, 0,
                                    TT.ptr(phi), _lib.MFS_F64, TT.stream()) == 0
    assert lib.mfs_fluid_volume2d(_lib.i64x(vres), f2(sc["bound_min"]), f2(sc["cell_size"] / 2), None, _lib.MFS_F64, 1e-3, 0,
                                  TT.ptr(vol), _lib.MFS_F64, TT.stream()) == 0
    torch.cuda.synchronize()
    assert float(phi.min()) == float(phi.max()) == 2.5 and float(vol.min()) == float(vol.max()) == 2.5
    with pytest.raises(ValueError, match="shape"):
        K.p2g(NS(num_particles=2, x=torch.zeros((2, 3), dtype=torch.float64, device=DEV), m=p.m, v=p.v, cx=p.cx, cy=p.cy), grid)
    assert C.sizeof(C.c_void_p) == 8


# ----------------------------------------------------------------------------------------------- grid ---
GRIDS = [(12, 16), (33, 21), (3, 130), (130, 3)]
gid = lambda g: "%dx%d" % g  # noqa: E731


def _fields(gres, seed, dt):
    """face velocities and masses: mass missing on a sprinkle of faces and on a block of up to 6 x 6 around the disc of
    `_solid` (zero averaged mass next to a solid), whose core two sweeps do not reach"""
    rng = np.random.default_rng(seed)
    Nx, Ny = gres
    out = {}
    for a, c in enumerate("xy"):
        shape = face_shape(gres, a)
        m = (rng.uniform(size=shape) > 0.15) * rng.uniform(0.2, 1.5, size=shape)
        x0, y0 = max(0, int(0.6 * Nx) - 3), max(0, int(0.4 * Ny) - 3)
        m[x0:x0 + 6, y0:y0 + 6] = 0
        out["m" + c] = m.astype(dt)
        out["v" + c] = rng.standard_normal(shape).astype(dt)
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("gres", GRIDS + [(2, 9)], ids=gid)
def test_extrapolate(gres, dt):
    """bit for bit, as the 3D kernel against its oracle; (2, 9): the y-face array (2, 10) has no interior face"""
    f = _fields(gres, 21, dt)
    got = [T(f["vx"]), T(f["vy"])]
    K.extrapolate(gres, 2, *got, T(f["mx"]), T(f["my"]))
    torch.cuda.synchronize()
    one, two = [f["vx"].copy(), f["vy"].copy()], [f["vx"].copy(), f["vy"].copy()]
    R.extrapolate(gres, 1, *one, f["mx"], f["my"])
    R.extrapolate(gres, 2, *two, f["mx"], f["my"])
    for a, c in enumerate("xy"):
        assert got[a].dtype == TD[dt]
        np.testing.assert_array_equal(N(got[a]), two[a])
        if min(two[a].shape) < 3:
            np.testing.assert_array_equal(N(got[a]), f["v" + c])                   # untouched
    if min(gres) >= 12:
        assert sum(int(((two[a] != one[a])).sum()) for a in range(2)) > 4          # the second sweep reached further
    single = [T(f["vx"]), T(f["vy"])]
    K.extrapolate(gres, 1, *single, T(f["mx"]), T(f["my"]))                        # odd sweep count: the copy back
    for a in range(2):
        np.testing.assert_array_equal(N(single[a]), one[a])


def _solid(gres, dx):
    """walls 1.2 cells thick and a disc, in units of dx, and a velocity field that is non-zero everywhere (a moving body)"""
    Nx, Ny = gres
    I = np.arange(2 * Nx + 1, dtype=np.float64)[:, None] * 0.5
    J = np.arange(2 * Ny + 1, dtype=np.float64)[None, :] * 0.5
    wall = np.minimum(np.minimum(I, Nx - I), np.minimum(J, Ny - J)) - 1.2
    disc = np.sqrt((I - 0.6 * Nx) ** 2 + (J - 0.4 * Ny) ** 2) - 0.15 * min(Nx, Ny)
    sphi = np.minimum(wall, disc) * dx
    sv = np.stack([0.3 * np.sin(0.37 * J) + 0.1 + 0 * I, -0.2 * np.cos(0.23 * I) + 0 * J], axis=-1)
    return sphi, sv


@pytest.mark.parametrize("dt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("gres", GRIDS, ids=gid)
def test_boundary_condition(gres, dt):
    """rtol 2e-7 / atol 1e-12 on dv and rtol 3e-7 / atol 1e-7 on v, as for the 3D kernel (float32 stores)"""
    dx = 0.05
    f = _fields(gres, 22, dt)
    sphi, sv = _solid(gres, dx)
    grid = NS(x=NS(v=T(f["vx"]), m=T(f["mx"]), dv=torch.full(face_shape(gres, 0), 9.0, dtype=TD[dt], device=DEV)),
              y=NS(v=T(f["vy"]), m=T(f["my"]), dv=torch.full(face_shape(gres, 1), 9.0, dtype=TD[dt], device=DEV)))
    K.apply_boundary_condition(grid, NS(phi=T(sphi), v=T(sv)), dx)
    torch.cuda.synchronize()
    gv, gm = [f["vx"], f["vy"]], [f["mx"], f["my"]]
    dv = [np.full_like(a, 9.0) for a in gv]
    R.boundary_condition(gres, gv, gm, sphi, sv, dx, dv)
    for a, c in enumerate((grid.x, grid.y)):
        got = N(c.dv)
        np.testing.assert_allclose(got, dv[a], rtol=2e-7, atol=1e-12)
        np.testing.assert_allclose(N(c.v), gv[a] + dv[a], rtol=3e-7, atol=1e-7)
        assert (got[0] == 0).all() and (got[-1] == 0).all() and (got[:, 0] == 0).all() and (got[:, -1] == 0).all()
    if min(gres) >= 12:
        far = sphi[2:-2:2, 3:-2:2] / dx >= 1                                         # x faces at least dx from the solid
        assert far.any() and (dv[0][1:-1, 1:-1][far] == 0).all() and np.count_nonzero(dv[0]) > 10 and np.count_nonzero(dv[1]) > 10
        # x faces next to the disc whose four vy taps all carry no mass: the averaged velocity is NaN, the correction 0
        msum = (f["my"][:-1, :-1] + f["my"][:-1, 1:] + f["my"][1:, :-1] + f["my"][1:, 1:])[:, 1:-1]
        empty = (msum == 0) & ~far
        assert empty.any() and (N(grid.x.dv)[1:-1, 1:-1][empty] == 0).all()
