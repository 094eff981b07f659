"""The numpy restatement of the 2D time step's kernels (tests/notebook2d_numpy.py) pinned to the 3D oracle
(oracle/mfs_oracle.py nb_*, which the executed-reference goldens pin) by dimension reduction, and the plumbing of the new
entry points -- all without a GPU.

Particles: a 3D grid (Nx, Ny, 5) with bound_min_z = 0 and dz = 2^-4; every particle at z = 2.5 dz, the centre plane of
cell layer 2 and node plane 5 of the doubled grid, exactly representable in float32.  Then the z weight is exactly 1 on
that plane and exactly 0 on the next, z displacements and z distances are exactly 0, and -- with cz = 0 and zero third
columns of cx, cy -- every z term of the 3D arithmetic is an exact 0 added or an exact 1 multiplied.  Grid kernels:
fields extruded along z over 7 layers; the middle plane sees z neighbours equal to itself.
All comparisons are BIT EQUALITY (np.testing.assert_array_equal: +0 == -0, NaN == NaN), which is stronger than the
rtol 1e-15 asked for."""
import ctypes as C

import numpy as np
import pytest

import notebook2d_numpy as R
from mfs import scenes
from oracle import mfs_oracle as O

GRIDS = [(12, 16), (33, 21)]
DZ = 2.0 ** -4
NZ = 5
BIAS3 = ((0, .5, .5), (.5, 0, .5))


def _lift(sc):
    """the scene of particle_scene_2d as a 3D one on (Nx, Ny, 5), particles on the plane z = 2.5 dz"""
    P = len(sc["px"])
    z = lambda a: np.concatenate([a, np.zeros((P, 1))], axis=1)  # noqa: E731
    px3 = np.concatenate([sc["px"], np.full((P, 1), 2.5 * DZ)], axis=1)
    assert np.float32(2.5 * DZ) == 2.5 * DZ
    return dict(gres=tuple(sc["gres"]) + (NZ,), bmin=np.concatenate([sc["bound_min"], np.zeros(1, np.float32)]),
                cs=np.concatenate([sc["cell_size"], [DZ]]), px=px3, pv=z(sc["pv"]), pc=(z(sc["pcx"]), z(sc["pcy"])))


@pytest.fixture(scope="module", params=GRIDS, ids=lambda g: "%dx%d" % g)
def pair(request):
    sc = scenes.particle_scene_2d(request.param, seed=3)
    return sc, _lift(sc)


def test_particle_scene_2d_reaches_the_clamps():
    for gres in GRIDS:
        sc = scenes.particle_scene_2d(gres, seed=3)
        again = scenes.particle_scene_2d(gres, seed=3)
        assert all(np.array_equal(sc[k], again[k]) for k in ("px", "pm", "pv", "pcx", "pcy"))
        assert sc["bound_min"].dtype == np.float32 and sc["bound_size"].dtype == np.float32 and sc["cell_size"].dtype == np.float64
        cell = np.floor((sc["px"] - sc["bound_min"].astype(np.float64)) / sc["cell_size"])
        for a in range(2):
            assert (cell[:, a] < 0).any() and (cell[:, a] >= gres[a]).any()          # outside on both sides: clamps fire
            assert (cell[:, a] == 0).any() and (cell[:, a] == gres[a] - 1).any()     # pressed against both walls
        assert (sc["px"] == sc["bound_min"].astype(np.float64)).all(axis=1).any()    # one exactly at the corner
        assert (np.diff(cell[:, 0]) < 0).sum() > len(cell) // 4                      # shuffled, not mesh order
        assert sc["px"].shape == sc["pv"].shape == sc["pcx"].shape == sc["pcy"].shape == (len(sc["pm"]), 2)
        assert 1000 < len(sc["pm"]) < 10000 or gres != (33, 21)


@pytest.mark.parametrize("axis", [0, 1])
def test_p2g_scatter_is_the_3d_scatter_on_a_plane(pair, axis):
    sc, s3 = pair
    gres = sc["gres"]
    shape = tuple(np.array(gres) + np.eye(2, dtype=int)[axis])
    gm3, gv3 = np.zeros(shape + (NZ,)), np.zeros(shape + (NZ,))
    O.nb_p2g_scatter(s3["px"], sc["pm"], s3["pv"], s3["pc"][axis], gm3, gv3, s3["bmin"], s3["gres"], BIAS3[axis], s3["cs"], axis)
    gm, gv, st = np.zeros(shape), np.zeros(shape), {}
    R.p2g_scatter(sc["px"], sc["pm"], sc["pv"], (sc["pcx"], sc["pcy"])[axis], gm, gv, sc["bound_min"], gres, R.BIAS[axis],
                  sc["cell_size"], axis, stats=st)
    np.testing.assert_array_equal(gm3[:, :, 2], gm)            # bit equality
    np.testing.assert_array_equal(gv3[:, :, 2], gv)
    assert not gm3[:, :, [0, 1, 3, 4]].any() and (gm != 0).sum() > 20          # the z weights are exactly 1 and 0
    assert st["K"].sum() == 4 * len(sc["pm"]) and st["K"].shape == shape and (st["S_m"] >= np.abs(gm) * (1 - 1e-12)).all()
    last = [slice(None)] * 2
    last[axis] = -1
    assert not st["K"][tuple(last)].any()                      # indices clamp to gres - 1, as in 3D


@pytest.mark.parametrize("axis", [0, 1])
def test_g2p_gather_is_the_3d_gather_on_a_plane(pair, axis):
    sc, s3 = pair
    gres = sc["gres"]
    shape = tuple(np.array(gres) + np.eye(2, dtype=int)[axis])
    field = np.random.default_rng(5 + axis).standard_normal(shape).astype(np.float32)
    P = len(sc["pm"])
    pv3, pc3 = np.full((P, 3), 7.0), np.full((P, 3), 7.0)
    O.nb_g2p_gather(s3["bmin"], s3["gres"], BIAS3[axis], s3["cs"], axis, s3["px"], pv3, pc3,
                    np.repeat(field[:, :, None], NZ, axis=2))
    pv, pc = np.full((P, 2), 7.0), np.full((P, 2), 7.0)
    R.g2p_gather(sc["bound_min"], gres, R.BIAS[axis], sc["cell_size"], axis, sc["px"], pv, pc, field)
    np.testing.assert_array_equal(pv3[:, axis], pv[:, axis])   # bit equality
    np.testing.assert_array_equal(pc3[:, :2], pc)
    assert (pv[:, 1 - axis] == 7.0).all() and np.abs(pc).max() > 1.0


def test_fluid_levelset_is_the_3d_level_set_on_a_plane(pair):
    sc, s3 = pair
    gres, gdx = sc["gres"], sc["gdx"]
    phi3 = np.zeros(s3["gres"])
    O.nb_fluid_levelset(s3["px"], phi3, s3["bmin"], s3["cs"], gdx, s3["gres"])
    phi = np.zeros(gres)
    R.fluid_levelset(sc["px"], phi, sc["bound_min"], sc["cell_size"], gdx, gres, radius=gdx * 0.5 * np.sqrt(3.0) * 1.02)
    np.testing.assert_array_equal(phi3[:, :, 2], phi)          # bit equality
    assert (phi < 0).any() and (phi == gdx * 3).any()
    own = np.zeros(gres)
    R.fluid_levelset(sc["px"], own, sc["bound_min"], sc["cell_size"], gdx, gres)
    assert R.default_radius(gdx) == gdx * 0.5 * np.sqrt(2.0) * 1.02
    np.testing.assert_allclose((own - phi)[phi < gdx * 2.5], gdx * 0.5 * 1.02 * (np.sqrt(3.0) - np.sqrt(2.0)), rtol=1e-12)


def test_fluid_volume_is_the_3d_volume_on_a_plane(pair):
    sc, s3 = pair
    vres, dcs = tuple(2 * np.array(sc["gres"]) + 1), sc["cell_size"] / 2
    vres3, dcs3 = tuple(2 * np.array(s3["gres"]) + 1), s3["cs"] / 2
    pvol = 1e-4 * float(np.prod(dcs3))                         # small enough for neither clamp: asserted below
    vol3 = np.zeros(vres3)
    O.nb_fluid_volume(s3["bmin"], dcs3, vres3, s3["px"], pvol, vol3)
    vol, st = np.zeros(vres), {}
    R.fluid_volume(sc["bound_min"], dcs, vres, sc["px"], pvol, vol, stats=st)
    assert st["S_vol"].max() < 0.5 * min(float(np.prod(dcs3)), R.volume_clamp(dcs))       # neither clamp is active
    np.testing.assert_array_equal(vol3[:, :, 5], vol)          # bit equality
    assert not vol3[:, :, :5].any() and not vol3[:, :, 6:].any() and (vol > 0).sum() > 50


def test_fluid_volume_clamps_to_the_cell_area(pair):
    sc, _ = pair
    vres, dcs = tuple(2 * np.array(sc["gres"]) + 1), sc["cell_size"] / 2
    assert R.volume_clamp(dcs) == dcs[0] * dcs[1]
    pvol = sc["pvol"]
    vol, tiny = np.zeros(vres), np.zeros(vres)
    R.fluid_volume(sc["bound_min"], dcs, vres, sc["px"], pvol, vol)
    R.fluid_volume(sc["bound_min"], dcs, vres, sc["px"], pvol * 2.0 ** -30, tiny)        # the same sums, scaled exactly
    assert tiny.max() < dcs[0] * dcs[1]
    np.testing.assert_array_equal(vol, np.minimum(tiny * 2.0 ** 30, dcs[0] * dcs[1]))
    assert (vol == dcs[0] * dcs[1]).any() and ((vol > 0) & (vol < dcs[0] * dcs[1])).any()


# ------------------------------------------------------------------------------------------------- grid ---
def _fields(gres, seed):
    """float32 face velocities and masses: mass missing on a sprinkle of faces and on a block of 6 x 6 (which two sweeps
    do not fill: the second sweep reaches faces the first made valid, the core stays invalid)"""
    rng = np.random.default_rng(seed)
    Nx, Ny = gres
    out = {}
    for a, c in enumerate("xy"):
        shape = tuple(np.array(gres) + np.eye(2, dtype=int)[a])
        m = (rng.uniform(size=shape) > 0.15) * rng.uniform(0.2, 1.5, size=shape)
        m[Nx // 3:Nx // 3 + 6, Ny // 3:Ny // 3 + 6] = 0
        out["m" + c] = m.astype(np.float32)
        out["v" + c] = rng.standard_normal(shape).astype(np.float32)
    return out


def _ext(a, n=7):
    return np.repeat(np.asarray(a)[:, :, None], n, axis=2).copy()


@pytest.mark.parametrize("gres", GRIDS, ids=lambda g: "%dx%d" % g)
def test_extrapolate_is_the_3d_extrapolate_on_the_middle_plane(gres):
    f = _fields(gres, 11)
    v3 = [_ext(f["vx"]), _ext(f["vy"]), np.zeros(gres + (8,), np.float32)]
    m3 = [_ext(f["mx"]), _ext(f["my"]), np.ones(gres + (8,), np.float32)]
    O.nb_extrapolate(gres + (7,), 2, *v3, *m3)
    one = [f["vx"].copy(), f["vy"].copy()]
    R.extrapolate(gres, 1, *one, f["mx"], f["my"])
    two = [f["vx"].copy(), f["vy"].copy()]
    R.extrapolate(gres, 2, *two, f["mx"], f["my"])
    for a, c in enumerate("xy"):
        np.testing.assert_array_equal(v3[a][:, :, 3], two[a])          # bit equality
        valid = f["m" + c] > 0
        assert (two[a][valid] == f["v" + c][valid]).all()              # faces with mass are never touched
        assert ((two[a] != one[a]) & ~valid).sum() > 4                 # the second sweep reached further
        core = (slice(gres[0] // 3 + 2, gres[0] // 3 + 4), slice(gres[1] // 3 + 2, gres[1] // 3 + 4))
        assert (two[a][core] == f["v" + c][core]).all()                # ... and not further than two faces
        for edge in ((0,), (-1,), (slice(None), 0), (slice(None), -1)):
            assert (two[a][edge] == f["v" + c][edge]).all()            # array-boundary faces untouched


def test_extrapolate_leaves_thin_arrays_alone():
    f = _fields((9, 2), 12)
    f["mx"][:] = 0
    f["mx"][4, 1] = 1
    v = [f["vx"].copy(), f["vy"].copy()]
    R.extrapolate((9, 2), 2, *v, f["mx"], f["my"])
    np.testing.assert_array_equal(v[0], f["vx"])               # (10, 2): no interior face


@pytest.mark.parametrize("gres", GRIDS, ids=lambda g: "%dx%d" % g)
def test_boundary_condition_is_the_3d_one_on_the_middle_plane(gres):
    sc = scenes.density_scene_2d(gres, seed=2)                 # a tank, a rotated bar that moves, a ball
    f = _fields(gres, 13)
    dx = float(min(sc["cell_size"]))
    sv3 = np.concatenate([_ext(sc["sv"][..., 0], 15)[..., None], _ext(sc["sv"][..., 1], 15)[..., None],
                          np.zeros(sc["sphi"].shape + (15, 1))], axis=-1)
    gv3 = [_ext(f["vx"]), _ext(f["vy"]), np.zeros(gres + (8,), np.float32)]
    gm3 = [_ext(f["mx"]), _ext(f["my"]), np.ones(gres + (8,), np.float32)]
    dv3 = [np.full_like(a, 9.0) for a in gv3]
    O.nb_boundary_condition(gres + (7,), gv3, gm3, _ext(sc["sphi"], 15), sv3, dx, dv3)
    gv, gm = [f["vx"], f["vy"]], [f["mx"], f["my"]]
    dv = [np.full_like(a, 9.0) for a in gv]
    R.boundary_condition(gres, gv, gm, sc["sphi"], sc["sv"], dx, dv)
    for a in range(2):
        assert dv[a].dtype == np.float32
        np.testing.assert_array_equal(dv3[a][:, :, 3], dv[a])  # bit equality
        assert np.count_nonzero(dv[a]) > 10 and (dv[a][0] == 0).all() and (dv[a][:, -1] == 0).all()
    assert np.abs(sc["sv"]).max() > 0                          # a moving body took part


# --------------------------------------------------------------------------------------------- plumbing ---
NEW = ["mfs_p2g_scatter2d", "mfs_g2p_gather2d", "mfs_fluid_levelset2d", "mfs_fluid_volume2d",
       "mfs_grid_extrapolate2d_workspace_bytes", "mfs_grid_extrapolate2d", "mfs_grid_boundary_condition2d"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mfs import _lib
    return _lib.load()


def test_new_symbols_are_exported_and_typed(lib):
    from mfs import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]


def test_entry_points_validate_before_any_launch(lib):
    """every rejection below returns before a kernel launch or any other device call: this runs on a CPU-only machine"""
    from mfs import _lib
    g, d2 = _lib.i64x((8, 9)), _lib.f64x((0.0, 0.0))
    cs = _lib.f64x((0.1, 0.1))
    buf = (C.c_double * 512)()
    a = C.cast(buf, C.c_void_p)                                # a non-null address; never dereferenced
    F = _lib.MFS_F64
    E = -1

    def scatter(axis=0, P=0, dt=F, gm=a, px=None):
        return lib.mfs_p2g_scatter2d(g, d2, cs, d2, axis, px, F, px, F, px, F, px, dt, P, gm, a, F, None)

    def gather(axis=0, P=0, dt=F, gv=a, px=None):
        return lib.mfs_g2p_gather2d(g, d2, cs, d2, axis, px, F, px, dt, px, F, P, gv, F, None)

    for fn in (scatter, gather):
        assert fn() == 0                                       # P == 0: MFS_OK without a launch
        assert fn(axis=2) == E and b"axis" in lib.mfs_last_error()
        assert fn(axis=-1) == E
        assert fn(dt=7) == E and b"dtype" in lib.mfs_last_error()
        assert fn(P=-1) == E
        assert fn(P=3) == E and b"particle" in lib.mfs_last_error()        # particles announced, arrays null
    assert scatter(gm=None) == E and b"null" in lib.mfs_last_error()
    assert gather(gv=None) == E and b"null" in lib.mfs_last_error()
    assert lib.mfs_p2g_scatter2d(_lib.i64x((0, 9)), d2, cs, d2, 0, None, F, None, F, None, F, None, F, 0, a, a, F, None) == E

    ls = lambda P=0, dt=F, phi=a: lib.mfs_fluid_levelset2d(g, d2, cs, 0.1, None, dt, P, phi, F, None)  # noqa: E731
    vol = lambda P=0, dt=F, v=a: lib.mfs_fluid_volume2d(g, d2, cs, None, dt, 1e-3, P, v, F, None)  # noqa: E731
    for fn in (ls, vol):
        assert fn() == 0
        assert fn(dt=7) == E and fn(P=-1) == E and fn(P=2) == E
    assert ls(phi=None) == E and vol(v=None) == E
    assert lib.mfs_fluid_levelset2d(g, None, cs, 0.1, None, F, 0, a, F, None) == E

    need = lib.mfs_grid_extrapolate2d_workspace_bytes(g, F)
    assert need >= (9 * 9 + 8 * 10) * (8 + 2) and lib.mfs_grid_extrapolate2d_workspace_bytes(g, 7) == 0
    assert lib.mfs_grid_extrapolate2d_workspace_bytes(None, F) == 0
    b = C.c_void_p(a.value + 8)
    ex = lambda it=2, vx=a, dt=F, ws=a, n=need: lib.mfs_grid_extrapolate2d(g, it, vx, b, dt, a, a, F, ws, n, None)  # noqa: E731
    assert ex(vx=None) == E and b"null" in lib.mfs_last_error()
    assert ex(dt=7) == E and ex(it=-1) == E and ex(n=need - 1) == E and ex(ws=None) == E
    assert ex(ws=C.c_void_p((a.value // 256 + 1) * 256 + 8)) == E and b"aligned" in lib.mfs_last_error()
    bc = lambda gvx=a, dt=F, dvx=a: lib.mfs_grid_boundary_condition2d(g, gvx, a, dt, a, a, F, a, F, a, F, 0.1, dvx, b, F, None)  # noqa: E731
    assert bc(gvx=None) == E and bc(dvx=None) == E and bc(dt=7) == E
    assert lib.mfs_grid_boundary_condition2d(None, a, a, F, a, a, F, a, F, a, F, 0.1, a, b, F, None) == E


def test_modules_import_without_a_gpu_and_refuse_cpu_tensors():
    import types

    import torch

    import notebook_kernels2d as K
    import notebook_sim2d as S
    assert callable(S.NotebookSimulation2D) and callable(S.add_box)
    for name in ("p2g", "p2g_scatter", "p2g_normalize", "g2p", "compute_fluid_levelset", "compute_fluid_volume", "extrapolate",
                 "apply_boundary_condition"):
        assert callable(getattr(K, name))
    with pytest.raises(TypeError, match="GPU"):
        K.extrapolate((4, 4), 2, torch.zeros(5, 4), torch.zeros(4, 5), torch.zeros(5, 4), torch.zeros(4, 5))
    with pytest.raises(TypeError, match="GPU"):
        K.compute_fluid_levelset(types.SimpleNamespace(x=torch.zeros((1, 2), dtype=torch.float64)),
                                 types.SimpleNamespace(resolution=(4, 4), phi=torch.zeros(4, 4)), 0.1)
    pts = S.add_box([0.5, 0.5], [0.2, 0.4], 0.05, np.random.default_rng(0))
    assert pts.shape == (4 * 8, 2)


def test_the_product_still_never_imports_the_oracle():
    from test_abi import test_product_never_imports_oracle
    test_product_never_imports_oracle()


def test_numpy_step_runs_and_moves_the_fluid():
    """two numpy time steps of a small dam break: the composition the GPU step test compares against holds together"""
    from timestep2d_scene import dam_break
    sc = dam_break((12, 16))
    s = R.make_state(sc["gres"], sc["gdx"], sc["bound_min"], sc["rb_d"], sc["px"], sc["pdx"], mu=sc["mu"])
    s.pv[...] = sc["pv"]
    x0 = s.px.copy()
    for _ in range(2):
        assert R.step(s) == pytest.approx(1.0 / 300.0)
    assert np.isfinite(s.px).all() and np.isfinite(s.pv).all() and not np.array_equal(s.px, x0)
    assert s.iters["density"] >= 0 and s.iters["viscosity"] > 0 and s.iters["pressure"] > 0
    assert s.lvol.max() <= R.volume_clamp(s.dcell_size)
