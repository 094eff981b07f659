"""The particle <-> grid transfers and grid kernels of the 2D time step: `notebook_kernels.py` one dimension down.

The reference has no 2D driver; these follow the 3D notebook's functions (`p2g`, `g2p`, `compute_fluid_levelset`,
`compute_fluid_volume`, `extrapolate`, `apply_boundary_condition`) with the same names and argument lists, on containers
without `z` / `cz` and particle arrays of shape (P, 2).  PyTorch-ROCm tensors; HIP kernels behind the C ABI
(csrc/mfs_notebook2d.hip).  What they produce is what `PressureCGSolver2D`, `ViscosityCGSolver2D` and
`DensityCGSolver2D` consume.  (A tile-sorted scatter for 2D is not built: the global atomics serve every size.)"""
import math

import torch

from mfs import _lib, tensors as T


def _gres2(gres):
    g = T.as_gres(gres)
    if len(g) != 2:
        raise ValueError(f"expected a 2D grid, got {g}")
    return g


def extrapolate(gres, num_iter, vx, vy, mx, my):
    """`num_iter` Jacobi sweeps of the 4-neighbour average into faces that received no mass, in place."""
    g = _gres2(gres)
    vs = [T.dev(t, n, T.face_shape(g, a)) for a, (t, n) in enumerate(((vx, "vx"), (vy, "vy")))]
    ms = [T.dev(t, n, T.face_shape(g, a)) for a, (t, n) in enumerate(((mx, "mx"), (my, "my")))]
    if not (vs[0].dtype == vs[1].dtype and ms[0].dtype == ms[1].dtype):
        raise TypeError("velocity / mass components must share a dtype")
    lib = _lib.load()
    gi = _lib.i64x(g)
    nbytes = int(lib.mfs_grid_extrapolate2d_workspace_bytes(gi, T.code(vs[0])))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=vs[0].device)
    _lib.check(lib.mfs_grid_extrapolate2d(gi, int(num_iter), *[T.ptr(t) for t in vs], T.code(vs[0]),
                                          *[T.ptr(t) for t in ms], T.code(ms[0]), T.ptr(ws), nbytes, T.stream()),
               "mfs_grid_extrapolate2d")


def apply_boundary_condition(g, solid, dx):
    """`g`: the grid object (g.x.v, g.x.m, g.x.dv, g.y...), `solid`: the solid level set (solid.phi on the doubled grid,
    solid.v its velocity field, two components), dx the grid spacing.  Computes the free-slip corrections into g.*.dv and
    adds them to g.*.v."""
    shp = tuple(g.x.v.shape)
    if len(shp) != 2:
        raise ValueError(f"g.x.v: expected a 2D face array, got shape {shp}")
    gres = (shp[0] - 1, shp[1])
    vs = [T.dev(t, n, T.face_shape(gres, a)) for a, (t, n) in enumerate(((g.x.v, "g.x.v"), (g.y.v, "g.y.v")))]
    ms = [T.dev(t, n, T.face_shape(gres, a)) for a, (t, n) in enumerate(((g.x.m, "g.x.m"), (g.y.m, "g.y.m")))]
    dvs = [T.dev(t, n, T.face_shape(gres, a)) for a, (t, n) in enumerate(((g.x.dv, "g.x.dv"), (g.y.dv, "g.y.dv")))]
    sphi = T.dev(solid.phi, "solid.phi", T.doubled_shape(gres))
    sv = T.dev(solid.v, "solid.v", T.doubled_shape(gres) + (2,))
    for grp in (vs, ms, dvs):
        if grp[0].dtype != grp[1].dtype:
            raise TypeError("the two components of a grid field must share a dtype")
    lib = _lib.load()
    _lib.check(lib.mfs_grid_boundary_condition2d(_lib.i64x(gres), *[T.ptr(t) for t in vs], T.code(vs[0]),
                                                 *[T.ptr(t) for t in ms], T.code(ms[0]), T.ptr(sphi), T.code(sphi),
                                                 T.ptr(sv), T.code(sv), float(dx), *[T.ptr(t) for t in dvs],
                                                 T.code(dvs[0]), T.stream()), "mfs_grid_boundary_condition2d")
    g.x.v += g.x.dv
    g.y.v += g.y.dv


# ------------------------------------------------------------------ particle <-> grid
def _particles(t, name):
    t = T.dev(t, name)
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError(f"{name}: expected shape (P, 2), got {tuple(t.shape)}")
    return t


def _f2(a):
    return _lib.f64x(T.as_f64_list(a, 2))


def _components(p, g):
    return ((g.x, p.cx, 0), (g.y, p.cy, 1))


def _scatter(p, g):
    gres = _gres2(g.resolution)
    px, pv = _particles(p.x, "p.x"), _particles(p.v, "p.v")
    pm = T.dev(p.m, "p.m", (px.shape[0],))
    lib = _lib.load()
    for gc, pc, axis in _components(p, g):
        pc = _particles(pc, "p.c" + "xy"[axis])
        gm = T.dev(gc.m, "g.%s.m" % "xy"[axis], T.face_shape(gres, axis))
        gv = T.dev(gc.v, "g.%s.v" % "xy"[axis], T.face_shape(gres, axis))
        if gm.dtype != gv.dtype:
            raise TypeError("grid mass and velocity must share a dtype")
        _lib.check(lib.mfs_p2g_scatter2d(_lib.i64x(gres), _f2(g.bound_min), _f2(g.cell_size), _f2(gc.bias), axis,
                                         T.ptr(px), T.code(px), T.ptr(pm), T.code(pm), T.ptr(pv), T.code(pv), T.ptr(pc),
                                         T.code(pc), int(px.shape[0]), T.ptr(gm), T.ptr(gv), T.code(gm), T.stream()),
                   "mfs_p2g_scatter2d")


def p2g(p, g):
    """Particle -> grid: APIC scatter of mass and momentum to the two face arrays, then momentum / mass.
    `p`: num_particles, x, m, v, cx, cy.  `g`: resolution, bound_min, cell_size and per axis g.x / g.y with m, v, bias.
    The caller zeroes g.*.m and g.*.v first."""
    _scatter(p, g)
    p2g_normalize(g)


def p2g_scatter(p, g):
    """the scatter half of `p2g` alone"""
    _scatter(p, g)


def p2g_normalize(g):
    """the division half of `p2g`: momentum / mass where mass landed (the kernel is dimension-free)"""
    lib = _lib.load()
    for gc, c in ((g.x, "x"), (g.y, "y")):
        gm = T.dev(gc.m, f"g.{c}.m")
        gv = T.dev(gc.v, f"g.{c}.v", tuple(gm.shape))
        if gm.dtype != gv.dtype:
            raise TypeError("grid mass and velocity must share a dtype")
        _lib.check(lib.mfs_p2g_normalize3d(int(gm.numel()), T.ptr(gm), T.ptr(gv), T.code(gm), T.stream()),
                   "mfs_p2g_normalize3d")


def g2p(p, g):
    """Grid -> particle: p.v[:, axis] and the affine rows p.cx / p.cy from g.*.v."""
    gres = _gres2(g.resolution)
    px, pv = _particles(p.x, "p.x"), _particles(p.v, "p.v")
    lib = _lib.load()
    for gc, pc, axis in _components(p, g):
        pc = _particles(pc, "p.c" + "xy"[axis])
        gv = T.dev(gc.v, "g.%s.v" % "xy"[axis], T.face_shape(gres, axis))
        _lib.check(lib.mfs_g2p_gather2d(_lib.i64x(gres), _f2(g.bound_min), _f2(g.cell_size), _f2(gc.bias), axis,
                                        T.ptr(px), T.code(px), T.ptr(pv), T.code(pv), T.ptr(pc), T.code(pc),
                                        int(px.shape[0]), T.ptr(gv), T.code(gv), T.stream()), "mfs_g2p_gather2d")


def compute_fluid_levelset(p, ls, gdx, radius=None):
    """Particle level set on the cell grid: ls.phi = gdx * 3, then the atomic-min pass.  `radius=None`: the cell's half
    diagonal with the notebook's margin, gdx * 0.5 * sqrt(2) * 1.02 (3D: sqrt(3))."""
    gres = _gres2(ls.resolution)
    px = _particles(p.x, "p.x")
    phi = T.dev(ls.phi, "ls.phi", gres)
    r = gdx * 0.5 * math.sqrt(2.0) * 1.02 if radius is None else float(radius)
    phi.fill_(gdx * 3)
    lib = _lib.load()
    _lib.check(lib.mfs_fluid_levelset2d(_lib.i64x(gres), _f2(ls.bound_min), _f2(ls.cell_size), float(r), T.ptr(px),
                                        T.code(px), int(px.shape[0]), T.ptr(phi), T.code(phi), T.stream()),
               "mfs_fluid_levelset2d")


def compute_fluid_volume(p, fv, pvol):
    """Fluid volume (area) on the doubled grid: zero, bilinear splat of `pvol`, clamp to the node's cell area."""
    vres = _gres2(fv.resolution)
    px = _particles(p.x, "p.x")
    vol = T.dev(fv.vol, "fv.vol", vres)
    vol.zero_()
    lib = _lib.load()
    _lib.check(lib.mfs_fluid_volume2d(_lib.i64x(vres), _f2(fv.bound_min), _f2(fv.cell_size), T.ptr(px), T.code(px),
                                      float(pvol), int(px.shape[0]), T.ptr(vol), T.code(vol), T.stream()),
               "mfs_fluid_volume2d")
