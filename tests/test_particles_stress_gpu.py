"""The particle scatters, the gather and the tile sort on the MI355X against a float64 reference of the same operation
(oracle/mfs_oracle.py nb_*, density_splat3d) on mfs.scenes.particle_stress_scene_3d: partial tiles, anisotropic cells,
clamps at all six walls, shuffled particle order (the tile sort's table overflow), float32 and float64 arrays.

Three paths per scatter:
  tiled   what runs by default at this particle count (tile-sorted, LDS-staged);
  atomic  the per-particle global atomics (TILE_MIN_PARTICLES raised);
  stale   the tiled kernels on an order computed BEFORE the particles moved up to three cells (contributions beyond
          the staged box take the global atomics).

Tolerance of a sum, per node, derived and not measured: a node receives K terms t_i, S = sum |t_i| (both from the
oracle).  A kernel that adds them into an array of unit roundoff u (2^-24 float32, 2^-53 float64) rounds each term once
on conversion and once per add, in any order: |got - exact| <= (K + 1) u S (1 + K u).  The bound asserted is
(K + 2) u S; the tiled kernels add in float64 LDS and round once per tile, they do better.  K == 0: exactly 0.0.
The float64 reference adds the same terms in particle order; for float64 arrays its own (K - 1) u S is not negligible
beside the bound in the worst case of every rounding aligned; roundings do not align like that -- the measured worst
err / bound is 0.66 over all float64 arrays, 0.53 over all float32 ones (profiles/particles_stress.txt).
Each test builds its reference on the CPU first (module-scoped, once per scene / positions / particle dtype), launches,
synchronises and compares."""
import types

import numpy as np
import pytest
import torch

import notebook_kernels as K
import solver.DensityCGSolver3D as D
from mfs import scenes
from oracle import mfs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
NS = types.SimpleNamespace
TD = {np.float32: torch.float32, np.float64: torch.float64}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
BIAS = ((0, .5, .5), (.5, 0, .5), (.5, .5, 0))
PATHS = ("tiled", "atomic", "stale")
POSITIONS = {"tiled": "fresh", "atomic": "fresh", "stale": "moved"}
DTYPES = [np.float32, np.float64]
ids = lambda prefix: (lambda d: prefix + ("32" if d is np.float32 else "64"))  # noqa: E731


def _face_shape(gres, a):
    return tuple(np.array(gres) + np.eye(3, dtype=int)[a])


class Reference:
    """the scene, the moved positions of the stale path and the float64 references, each built once"""

    def __init__(self, sc, seed=7):
        self.sc = sc
        self.gres, self.bmin, self.cs = sc["gres"], sc["bound_min"], sc["cell_size"]
        rng = np.random.default_rng(seed)
        self.pos = {"fresh": sc["px"], "moved": sc["px"] + (rng.random(sc["px"].shape) - 0.5) * 6 * self.cs}
        self._memo = {}

    def arrays(self, kind, pdt):
        """the particle arrays as the GPU gets them (float32 particle arrays are the float64 ones rounded)"""
        sc = self.sc
        return dict(px=self.pos[kind].astype(pdt), pm=sc["pm"].astype(pdt), pv=sc["pv"].astype(pdt),
                    pcx=sc["pcx"].astype(pdt), pcy=sc["pcy"].astype(pdt), pcz=sc["pcz"].astype(pdt))

    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def p2g(self, kind, pdt):
        def make():
            a, out = self.arrays(kind, pdt), []
            for ax, c in enumerate("xyz"):
                gm, gv, st = np.zeros(_face_shape(self.gres, ax)), np.zeros(_face_shape(self.gres, ax)), {}
                O.nb_p2g_scatter(a["px"], a["pm"], a["pv"], a["pc" + c], gm, gv, self.bmin, self.gres, BIAS[ax], self.cs, ax,
                                 stats=st)
                out.append(dict(gm=gm, gv=gv, **st))
            return out
        return self._once(("p2g", kind, pdt), make)

    def volume(self, kind, pdt):
        def make():
            vres = tuple(2 * np.array(self.gres) + 1)
            vol, st = np.zeros(vres), {}
            O.nb_fluid_volume(self.bmin, self.cs / 2, vres, self.arrays(kind, pdt)["px"], self.sc["pvol"], vol, stats=st)
            return dict(vol=vol, **st)
        return self._once(("vol", kind, pdt), make)

    def density(self, kind, pdt):
        def make():
            a = self.arrays(kind, pdt)
            gm, gvol, st = np.zeros(self.gres), np.zeros(self.gres), {}
            O.density_splat3d(self.bmin.astype(np.float64), self.cs, self.gres, a["px"], a["pm"], self.sc["pvol"], gm, gvol,
                              stats=st)
            return dict(gm=gm, gvol=gvol, **st)
        return self._once(("density", kind, pdt), make)

    def levelset(self, kind):
        def make():
            phi = np.zeros(self.gres)
            O.nb_fluid_levelset(self.pos[kind], phi, self.bmin, self.cs, self.sc["gdx"], self.gres)
            return phi
        return self._once(("phi", kind), make)


@pytest.fixture(scope="module")
def ref():
    return Reference(scenes.particle_stress_scene_3d())


def _particles(a):
    return NS(num_particles=len(a["px"]), x=T(a["px"]), m=T(a["pm"]), v=T(a["pv"]), cx=T(a["pcx"]), cy=T(a["pcy"]),
              cz=T(a["pcz"]))


def _grid(R, gdt, fill=0.0):
    def comp(a):
        return NS(bias=np.asarray(BIAS[a], np.float32), m=torch.full(_face_shape(R.gres, a), fill, dtype=TD[gdt], device=DEV),
                  v=torch.full(_face_shape(R.gres, a), fill, dtype=TD[gdt], device=DEV))
    return NS(resolution=R.gres, bound_min=R.bmin, bound_size=R.sc["bound_size"], cell_size=R.cs, x=comp(0), y=comp(1), z=comp(2))


class Path:
    """puts notebook_kernels on one of the three paths for the particle container it returns, and checks afterwards
    that this path is what ran"""

    def __init__(self, path, monkeypatch, R, pdt):
        self.path, self.R = path, R
        K._TILE_ORDERS.clear()                         # no order of an earlier test (allocations are reused)
        if path == "atomic":
            monkeypatch.setattr(K, "TILE_MIN_PARTICLES", 1 << 40)
        else:
            assert len(R.sc["px"]) >= K.TILE_MIN_PARTICLES          # the default threshold: nothing forced
        self.p = _particles(R.arrays("fresh", pdt))
        self.stale = None
        if path == "stale":
            assert K.tile_order(self.p, R.gres, R.bmin, R.cs) is not None
            self.stale = K._TILE_ORDERS[0]
            self.p.x.copy_(T(R.arrays("moved", pdt)["px"]))
            K._TILE_ORDERS[0] = ((self.p.x.data_ptr(), self.p.x._version) + self.stale[0][2:],) + self.stale[1:]   # pretend it is current

    def order(self):
        return K.tile_order(self.p, self.R.gres, self.R.bmin, self.R.cs)

    def check(self):
        torch.cuda.synchronize()
        if self.path == "atomic":
            assert not K._TILE_ORDERS
        else:
            assert len(K._TILE_ORDERS) == 1 and K._TILE_ORDERS[0][0][0] == self.p.x.data_ptr()      # ONE sort, shared
            if self.stale is not None:
                assert K._TILE_ORDERS[0][1] is self.stale[1]                                          # the stale order was used


def _within(got, want, Kn, S, u, what):
    got = np.asarray(got)
    err, bound = np.abs(got.astype(np.float64) - want), (Kn + 2) * u * S
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(ratio.argmax(), ratio.shape)
    print(f"RATIO {what}: worst err / bound {ratio.max():.4f} at {worst} (K {Kn[worst]})")
    assert ratio.max() <= 1.0, (f"{what}: worst err / bound {ratio.max():.4g} at node {worst}: got {got[worst]!r} want {want[worst]!r} "
                                f"K {Kn[worst]} S {S[worst]!r}; {int((ratio > 1).sum())} nodes over")
    assert (got[Kn == 0] == 0.0).all(), f"{what}: {int((got[Kn == 0] != 0).sum())} nodes without a contribution are not 0.0"


# ------------------------------------------------------------------ p2g ---------------------------------------------
@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("path", PATHS)
def test_p2g_scatter(ref, path, gdt, pdt, monkeypatch):
    want = ref.p2g(POSITIONS[path], pdt)
    run = Path(path, monkeypatch, ref, pdt)
    grid = _grid(ref, gdt)
    K.p2g_scatter(run.p, grid)
    run.check()
    for ax, c in enumerate("xyz"):
        w, gc = want[ax], getattr(grid, c)
        what = f"p2g {path} grid {np.dtype(gdt).name} particles {np.dtype(pdt).name} g.{c}"
        _within(N(gc.m), w["gm"], w["K"], w["S_m"], U[gdt], what + ".m")
        _within(N(gc.v), w["gv"], w["K"], w["S_v"], U[gdt], what + ".mv")
        last = [slice(None)] * 3
        last[ax] = -1
        assert not w["K"][tuple(last)].any() and w["K"].sum() == 8 * run.p.num_particles      # indices clamp to gres - 1


@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
def test_p2g_normalize_divides_in_the_arrays_own_precision(ref, gdt, monkeypatch):
    ref.p2g("fresh", np.float64)
    run = Path("tiled", monkeypatch, ref, np.float64)
    grid = _grid(ref, gdt)
    K.p2g_scatter(run.p, grid)
    run.check()
    before = {c: (N(getattr(grid, c).m), N(getattr(grid, c).v)) for c in "xyz"}
    K.p2g_normalize(grid)
    torch.cuda.synchronize()
    for c in "xyz":
        gm, gv = before[c]
        assert gm.dtype == gdt and (gm > 0).any() and ((gm <= 0) & (gv != 0)).any()          # negative masses: both branches
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(gm > 0, gv / gm, gv)
        assert want.dtype == gdt
        np.testing.assert_array_equal(N(getattr(grid, c).v), want)
        np.testing.assert_array_equal(N(getattr(grid, c).m), gm)


# ------------------------------------------------------------------ volume, density ---------------------------------
@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("path", PATHS)
def test_fluid_volume(ref, path, gdt, pdt, monkeypatch):
    """the clamp min(., cell volume) moves no value further from the reference's than the sums are apart"""
    want = ref.volume(POSITIONS[path], pdt)
    run = Path(path, monkeypatch, ref, pdt)
    vres = tuple(2 * np.array(ref.gres) + 1)
    fv = NS(resolution=vres, bound_min=ref.bmin, bound_size=ref.sc["bound_size"], cell_size=ref.cs / 2,
            vol=torch.full(vres, 3.0, dtype=TD[gdt], device=DEV))
    assert (run.order() is not None) == (path != "atomic")
    K.compute_fluid_volume(run.p, fv, ref.sc["pvol"])
    run.check()
    cvol = float(np.prod(ref.cs / 2))
    assert (want["vol"] == cvol).any() and ((want["vol"] > 0) & (want["vol"] < cvol)).any()      # clamped and partial nodes
    _within(N(fv.vol), want["vol"], want["K"], want["S_vol"], U[gdt],
            f"volume {path} grid {np.dtype(gdt).name} particles {np.dtype(pdt).name}")


@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("path", PATHS)
def test_density_splat(ref, path, gdt, pdt, monkeypatch):
    """solver.DensityCGSolver3D.initialize_density: on the tiled and stale paths mfs_density_splat3d_tiled"""
    want = ref.density(POSITIONS[path], pdt)
    run = Path(path, monkeypatch, ref, pdt)
    gm, gvol = (torch.zeros(ref.gres, dtype=TD[gdt], device=DEV) for _ in range(2))
    bmin64 = ref.bmin.astype(np.float64)
    assert (K.tile_order(run.p.x, ref.gres, bmin64, ref.cs) is not None) == (path != "atomic")
    D.initialize_density(bmin64, ref.cs, ref.gres, run.p.x, run.p.m, ref.sc["pvol"], gm, gvol)
    run.check()
    what = f"density {path} grid {np.dtype(gdt).name} particles {np.dtype(pdt).name}"
    _within(N(gm), want["gm"], want["K"], want["S_m"], U[gdt], what + " gm")
    _within(N(gvol), want["gvol"], want["K"], want["S_vol"], U[gdt], what + " gvol")


# ------------------------------------------------------------------ level set ---------------------------------------
def _levelset(run, R, dt):
    ls = NS(resolution=R.gres, bound_min=R.bmin, bound_size=R.sc["bound_size"], cell_size=R.cs,
            phi=torch.zeros(R.gres, dtype=TD[dt], device=DEV))
    K.compute_fluid_levelset(run.p, ls, R.sc["gdx"])
    run.check()
    return N(ls.phi)


@pytest.mark.parametrize("kind", ["fresh", "moved"])
def test_fluid_levelset(ref, kind, monkeypatch):
    """against nb_fluid_levelset, and bit for bit between the paths on the same positions (a minimum has no order)"""
    want = ref.levelset(kind)
    assert (want < 0).any() and (want == ref.sc["gdx"] * 3).any()
    tiled = _levelset(Path("tiled" if kind == "fresh" else "stale", monkeypatch, ref, np.float64), ref, np.float64)
    np.testing.assert_allclose(tiled, want, rtol=1e-13, atol=1e-15)
    run = Path("atomic", monkeypatch, ref, np.float64)
    if kind == "moved":
        run.p.x.copy_(T(ref.pos["moved"]))
    atomic = _levelset(run, ref, np.float64)
    np.testing.assert_allclose(atomic, want, rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(tiled, atomic)


@pytest.mark.parametrize("path", PATHS)
def test_fluid_levelset_float32_phi(ref, path, monkeypatch):
    """a float32 level set is the float64 one rounded: within one float32 ulp of the rounded float64 reference"""
    want = ref.levelset(POSITIONS[path]).astype(np.float32)
    got = _levelset(Path(path, monkeypatch, ref, np.float64), ref, np.float32)
    assert got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)).all()


# ------------------------------------------------------------------ g2p ---------------------------------------------
@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
def test_g2p(ref, gdt, pdt, monkeypatch):
    """float64 particle arrays: order-exact (1e-12).  float32 particle arrays: every partial sum is rounded to float32 as
    the reference's `pv[P, axis] += ...` does -- within 8 * 2^-24 * sum |terms| of the float64 gather per particle, and
    NOT the float64 gather rounded once at the end"""
    rng = np.random.default_rng(11)
    G = [(rng.standard_normal(_face_shape(ref.gres, a)) * 10.0 ** rng.uniform(-2, 1, _face_shape(ref.gres, a))).astype(gdt)
         for a in range(3)]
    a = ref.arrays("fresh", pdt)
    P = len(a["px"])
    v64, c64, st = np.zeros((P, 3)), [np.zeros((P, 3)) for _ in range(3)], [{} for _ in range(3)]
    v32, c32 = np.zeros((P, 3), np.float32), [np.zeros((P, 3), np.float32) for _ in range(3)]
    for ax in range(3):
        O.nb_g2p_gather(ref.bmin, ref.gres, BIAS[ax], ref.cs, ax, a["px"], v64, c64[ax], G[ax], stats=st[ax])
        O.nb_g2p_gather(ref.bmin, ref.gres, BIAS[ax], ref.cs, ax, a["px"], v32, c32[ax], G[ax])
    run = Path("tiled", monkeypatch, ref, pdt)
    grid = _grid(ref, gdt)
    for ax, c in enumerate("xyz"):
        getattr(grid, c).v.copy_(T(G[ax]))
    run.p.v.fill_(7.0)
    K.g2p(run.p, grid)
    torch.cuda.synchronize()
    pv, pc = N(run.p.v), [N(run.p.cx), N(run.p.cy), N(run.p.cz)]
    assert pv.dtype == pdt and pc[0].dtype == pdt
    if pdt is np.float64:
        np.testing.assert_allclose(pv, v64, rtol=1e-12, atol=1e-13)
        for ax in range(3):
            np.testing.assert_allclose(pc[ax], c64[ax], rtol=1e-12, atol=1e-12 * np.abs(c64[ax]).max())
        return
    u = 2.0 ** -24
    for ax in range(3):
        assert (np.abs(pv[:, ax].astype(np.float64) - v64[:, ax]) <= 8 * u * st[ax]["S_v"]).all(), ax
        assert (np.abs(pc[ax].astype(np.float64) - c64[ax]) <= 8 * u * st[ax]["S_c"]).all(), ax
        dv, dc = (pv[:, ax] != v64[:, ax].astype(np.float32)).mean(), (pc[ax] != c64[ax].astype(np.float32)).mean()
        ov, oc = (pv[:, ax] != v32[:, ax]).mean(), (pc[ax] != c32[ax]).mean()
        print(f"G2P grid {np.dtype(gdt).name} axis {ax}: differs from the rounded float64 gather in {dv:.3f} / {dc:.3f} of the "
              f"entries, from the oracle's float32 gather in {ov:.2e} / {oc:.2e}")
        assert dv > 0 and dc > 0, ax                     # the float32 branch was taken
        # same IEEE operations in the same order, none contracted: the oracle's float32 gather bit for bit
        assert ov == 0 and oc == 0, ax


# ------------------------------------------------------------------ tile sort ---------------------------------------
def _check_tile_order(x, gres, bmin, cs, perm, tstart):
    P = len(x)
    perm_h, ts = N(perm), N(tstart)
    assert np.array_equal(np.sort(perm_h), np.arange(P))
    assert ts[0] == 0 and ts[-1] == P and (np.diff(ts) >= 0).all()
    cell = np.floor((x.astype(np.float32) - bmin).astype(np.float64) / cs).astype(np.int64).clip(0, np.array(gres) - 1)
    nt = [(g_ + 7) // 8 for g_ in gres]
    assert len(ts) == int(np.prod(nt)) + 1
    tile = ((cell[:, 0] // 8) * nt[1] + cell[:, 1] // 8) * nt[2] + cell[:, 2] // 8
    seg = np.searchsorted(ts, np.arange(P), side="right") - 1          # tile of every slot of perm
    assert (tile[perm_h] == seg).all()
    return tile


@pytest.mark.parametrize("pdt", DTYPES, ids=ids("p"))
def test_tile_sort_on_the_stress_scene(ref, pdt, monkeypatch):
    """partial tiles, clamped particles, and workgroups (256 consecutive particles) that see more tiles than their table
    of 128 holds: the overflow path straight to memory"""
    run = Path("tiled", monkeypatch, ref, pdt)
    perm, tstart = run.order()
    run.check()
    tile = _check_tile_order(N(run.p.x), ref.gres, ref.bmin, ref.cs, perm, tstart)
    assert max(len(np.unique(tile[a:a + 256])) for a in range(0, len(tile), 256)) > 128


# ------------------------------------------------------------------ tiny grids --------------------------------------
@pytest.mark.parametrize("gdt", DTYPES, ids=ids("g"))
@pytest.mark.parametrize("gres", [(1, 1, 1), (1, 9, 1), (7, 8, 9)], ids=lambda g: "x".join(map(str, g)))
def test_tiny_grids_through_the_tiled_kernels(gres, gdt, monkeypatch):
    """a single tile, a tile larger than the grid, partial tiles only: 300 particles from one cell outside the box to one
    cell outside on the other side, every scatter forced onto the tiled kernels, against the oracle with the same bound"""
    monkeypatch.setattr(K, "TILE_MIN_PARTICLES", 1)
    K._TILE_ORDERS.clear()
    rng = np.random.default_rng(sum(gres))
    Ng = np.array(gres)
    bmin, bsz = np.asarray([-0.3, 0.0, -0.3], np.float32), (Ng * np.array([0.05, 0.03, 0.07])).astype(np.float32)
    cs = bsz / Ng.astype(np.int64)
    P = 300
    X = rng.uniform(-1.0, Ng + 1.0, size=(P, 3)) * cs + bmin.astype(np.float64)
    X[:4] = bmin
    a = dict(px=X, pm=rng.standard_normal(P), pv=rng.standard_normal((P, 3)), pcx=rng.standard_normal((P, 3)),
             pcy=rng.standard_normal((P, 3)), pcz=rng.standard_normal((P, 3)))
    R = NS(gres=gres, bmin=bmin, cs=cs, sc=dict(bound_size=bsz))
    want = []
    for ax, c in enumerate("xyz"):
        gm, gv, st = np.zeros(_face_shape(gres, ax)), np.zeros(_face_shape(gres, ax)), {}
        O.nb_p2g_scatter(a["px"], a["pm"], a["pv"], a["pc" + c], gm, gv, bmin, gres, BIAS[ax], cs, ax, stats=st)
        want.append(dict(gm=gm, gv=gv, **st))
    vres = tuple(2 * Ng + 1)
    wvol, svol = np.zeros(vres), {}
    O.nb_fluid_volume(bmin, cs / 2, vres, X, 1e-5, wvol, stats=svol)
    wdm, wdv, sden = np.zeros(gres), np.zeros(gres), {}
    O.density_splat3d(bmin.astype(np.float64), cs, gres, X, a["pm"], 1e-5, wdm, wdv, stats=sden)
    wphi = np.zeros(gres)
    gdx = float(cs.min())
    O.nb_fluid_levelset(X, wphi, bmin, cs, gdx, gres)

    p = _particles(a)
    perm, tstart = K.tile_order(p, gres, bmin, cs)
    torch.cuda.synchronize()
    _check_tile_order(X, gres, bmin, cs, perm, tstart)
    grid = _grid(R, gdt)
    K.p2g_scatter(p, grid)
    fv = NS(resolution=vres, bound_min=bmin, bound_size=bsz, cell_size=cs / 2, vol=torch.full(vres, 3.0, dtype=TD[gdt], device=DEV))
    K.compute_fluid_volume(p, fv, 1e-5)
    gm, gvol = (torch.zeros(gres, dtype=TD[gdt], device=DEV) for _ in range(2))
    D.initialize_density(bmin.astype(np.float64), cs, gres, p.x, p.m, 1e-5, gm, gvol)
    ls = NS(resolution=gres, bound_min=bmin, bound_size=bsz, cell_size=cs, phi=torch.zeros(gres, dtype=torch.float64, device=DEV))
    K.compute_fluid_levelset(p, ls, gdx)
    torch.cuda.synchronize()
    assert len(K._TILE_ORDERS) == 1                                       # every consumer took the one tile order
    what = "tiny " + "x".join(map(str, gres)) + " " + np.dtype(gdt).name
    for ax, c in enumerate("xyz"):
        w, gc = want[ax], getattr(grid, c)
        _within(N(gc.m), w["gm"], w["K"], w["S_m"], U[gdt], f"{what} g.{c}.m")
        _within(N(gc.v), w["gv"], w["K"], w["S_v"], U[gdt], f"{what} g.{c}.mv")
    _within(N(fv.vol), wvol, svol["K"], svol["S_vol"], U[gdt], what + " volume")
    _within(N(gm), wdm, sden["K"], sden["S_m"], U[gdt], what + " density gm")
    _within(N(gvol), wdv, sden["K"], sden["S_vol"], U[gdt], what + " density gvol")
    np.testing.assert_allclose(N(ls.phi), wphi, rtol=1e-13, atol=1e-15)
