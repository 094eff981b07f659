"""Drop-in for the reference's solver/DensityCGSolver2D.py on MI355X.

Same module functions, class, constructor and `solve` signature as the reference (file:line cited per item), on
PyTorch-ROCm tensors, calling the HIP kernels of libmfs_hip.so through the C ABI (include/mfs.h).  The CG loop runs on
the 2D pressure engine set up for the density operator (csrc/mfs_pressure2d.hip, mfs_pcg2d_setup_density):
device-resident scalars, no host sync per iteration.  No CPU path.

What the 2D reference does differently from its 3D twin, kept: the splat writes the mass only (`vol` is filled by
`fix_volume` from `lvol`), the loop does NOT raise when `max_iter` runs out, and the y gather samples at the positions
the x gather has already moved.
"""
import numpy as np
import torch

from mfs import _lib, tensors as T
from mfs.pcg import Pcg2dEngine
from .SolidFraction2D import compute_solid_frac, edge_in_fraction  # noqa: F401  (reference line 6)


def _faces(g, wx, wy, names=("wx", "wy")):
    wx = T.dev(wx, names[0], T.face_shape(g, 0))
    wy = T.dev(wy, names[1], T.face_shape(g, 1))
    if wx.dtype != wy.dtype:
        raise TypeError(f"{', '.join(names)} must share a dtype")
    return wx, wy


def _grid2(gres):
    g = T.as_gres(gres)
    if len(g) != 2:
        raise ValueError(f"DensityCGSolver2D needs a 2D grid, got {g}")
    return g


def _particles(px):
    px = T.dev(px, "px")
    if px.dim() != 2 or px.shape[1] != 2:
        raise ValueError(f"px: expected shape (P, 2), got {tuple(px.shape)}")
    return px


def initialize_density(bound_min, cell_size, gres, px, pm, pvol, gm, gvol, sphi=None, lphi=None):
    """Scatter particle mass to the cell centres (reference :197-202 -> kernel :8-33).  Only `gm` is written: the
    reference's volume scatter is commented out (:33).  `pvol`, `gvol`, `sphi`, `lphi` are accepted and unused."""
    g = _grid2(gres)
    px = _particles(px)
    pm = T.dev(pm, "pm", (px.shape[0],))
    gm = T.dev(gm, "gm", g)
    gvol = T.dev(gvol, "gvol", g)
    if gm.dtype != gvol.dtype:
        raise TypeError("gm and gvol must share a dtype")
    lib = _lib.load()
    _lib.check(lib.mfs_density_splat2d(_lib.i64x(g), _lib.f64x(T.as_f64_list(bound_min, 2)),
                                       _lib.f64x(T.as_f64_list(cell_size, 2)), T.ptr(px), T.code(px), T.ptr(pm),
                                       T.code(pm), 0.0 if pvol is None else float(pvol), int(px.shape[0]), T.ptr(gm),
                                       T.ptr(gvol), T.code(gm), T.stream()), "mfs_density_splat2d")


def fix_volume(cell_size, gres, lvol, gvol, sphi, lphi, wx, wy):
    """Cell fluid volume from `lvol` (reference :204-211 -> kernel :35-57); interior cells of `gvol` only."""
    g = _grid2(gres)
    lvol = T.dev(lvol, "lvol", T.doubled_shape(g))
    gvol = T.dev(gvol, "gvol", g)
    sphi = T.dev(sphi, "sphi", T.doubled_shape(g))
    lphi = T.dev(lphi, "lphi", g)
    wx, wy = _faces(g, wx, wy)
    lib = _lib.load()
    _lib.check(lib.mfs_density_fix_volume2d(_lib.i64x(g), _lib.f64x(T.as_f64_list(cell_size, 2)), T.ptr(lvol),
                                            T.code(lvol), T.ptr(gvol), T.code(gvol), T.ptr(sphi), T.code(sphi),
                                            T.ptr(lphi), T.code(lphi), T.ptr(wx), T.ptr(wy), T.code(wx), T.stream()),
               "mfs_density_fix_volume2d")


def initialize_solver(rho0, dt, gres, cell_size, gm, gvol, lphi, wx, wy, b):
    """Right-hand side (reference :213-219 -> kernel :59-83)."""
    g = _grid2(gres)
    gm, gvol = T.dev(gm, "gm", g), T.dev(gvol, "gvol", g)
    if gm.dtype != gvol.dtype:
        raise TypeError("gm and gvol must share a dtype")
    lphi = T.dev(lphi, "lphi", g)
    wx, wy = _faces(g, wx, wy)
    b = T.dev(b, "b", g)
    lib = _lib.load()
    _lib.check(lib.mfs_density_rhs2d(_lib.i64x(g), float(rho0), float(dt), _lib.f64x(T.as_f64_list(cell_size, 2)),
                                     T.ptr(gm), T.ptr(gvol), T.code(gm), T.ptr(lphi), T.code(lphi), T.ptr(wx), T.ptr(wy),
                                     T.code(wx), T.ptr(b), T.code(b), T.stream()), "mfs_density_rhs2d")


def matvecmul(gres, v, out, wx, wy, lphi):
    """out = A v, the density solver's operator (reference :221-225 -> kernel :85-139)."""
    g = _grid2(gres)
    v, out = T.dev(v, "v", g), T.dev(out, "out", g)
    if v.dtype != out.dtype:
        raise TypeError("v and out must share a dtype")
    wx, wy = _faces(g, wx, wy)
    lphi = T.dev(lphi, "lphi", g)
    lib = _lib.load()
    _lib.check(lib.mfs_density_apply2d(_lib.i64x(g), T.ptr(v), T.ptr(out), T.code(v), T.ptr(wx), T.ptr(wy), T.code(wx),
                                       T.ptr(lphi), T.code(lphi), T.stream()), "mfs_density_apply2d")


def compute_displacement(gres, dt, cell_size, dx, dy, pv, lphi):
    """Face displacements from the solved field (reference :227-231 -> kernel :141-152): entries [1:Nx, 1:Ny] of both."""
    g = _grid2(gres)
    dx, dy = _faces(g, dx, dy, ("dx", "dy"))
    pv, lphi = T.dev(pv, "pv", g), T.dev(lphi, "lphi", g)
    lib = _lib.load()
    _lib.check(lib.mfs_density_displacement2d(_lib.i64x(g), float(dt), _lib.f64x(T.as_f64_list(cell_size, 2)), T.ptr(dx),
                                              T.ptr(dy), T.code(dx), T.ptr(pv), T.code(pv), T.ptr(lphi), T.code(lphi),
                                              T.stream()), "mfs_density_displacement2d")


def apply_displacement(px, dx, bound_min, cell_size, grid_bias, axis):
    """px[:, axis] += bilinear sample of the face array (reference :233-238 -> kernel :171-195)."""
    px = _particles(px)
    dx = T.dev(dx, "dx")
    if dx.dim() != 2:
        raise ValueError("dx: expected a 2D face array")
    if int(axis) not in (0, 1):
        raise ValueError(f"axis: expected 0 or 1, got {axis}")
    lib = _lib.load()
    _lib.check(lib.mfs_density_advect2d(T.ptr(px), T.code(px), int(px.shape[0]), T.ptr(dx), T.code(dx),
                                        _lib.i64x(tuple(dx.shape)), _lib.f64x(T.as_f64_list(bound_min, 2)),
                                        _lib.f64x(T.as_f64_list(cell_size, 2)), _lib.f64x(T.as_f64_list(grid_bias, 2)),
                                        int(axis), T.stream()), "mfs_density_advect2d")


class DensityCGSolver2D:
    """Reference :240-294.  `DensityCGSolver2D(buf, gres, bound_min, bound_size)`; shares the `CGSolverBuffer` with the
    pressure solver.  `self.wx, self.wy` are what a caller hands to `PressureCGSolver2D.solve`.  Like the 2D pressure
    solver it does NOT raise when `max_iter` is exhausted (no for-else in the reference): the displacement is applied
    from whatever `x` holds.  One departure, shared with every engine of this package: a NaN / inf `delta` enters the
    loop as in the reference, but the device loop stops at its first non-finite dot product and `solve` raises
    `mfs._lib.MfsNonFinite` (a ValueError) before any displacement is applied, where the reference would run `max_iter`
    iterations and move the particles by NaN; `d.q == 0` raises `MfsZeroDivision` as the reference's division does.
    Extras that do not change reference behaviour: `iterations`, `converged`, `history`,
    `history_truncated`, `check_every`."""

    def __init__(self, buf, gres, bound_min, bound_size, check_every=32):
        self.gres = gres
        self._g = _grid2(gres)
        self.bound_min = np.array(T.as_f64_list(bound_min, 2))
        self.cell_size = np.array(T.as_f64_list(bound_size, 2)) / np.array(self._g, dtype=np.float64)
        self.bias_x = np.array([0, 0.5])
        self.bias_y = np.array([0.5, 0])
        self.buf = buf
        dt, device = buf.b.dtype, buf.b.device
        z = lambda shape: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
        self.m, self.vol, self.x = z(self._g), z(self._g), z(self._g)
        self.wx, self.wy = (z(T.face_shape(self._g, a)) for a in range(2))
        self.dx, self.dy = (z(T.face_shape(self._g, a)) for a in range(2))
        self.alpha = 0.0
        self.beta = 0.0
        self.delta = 0.0
        self.max_iter = int(np.prod(self._g))
        self.check_every = int(check_every)
        self.iterations = 0
        self.converged = False
        self._engine = Pcg2dEngine(self._g, dt, device)

    @property
    def history(self):
        return self._engine.history()

    @property
    def history_truncated(self):
        """True if the last solve ran past the history buffer (8 191 iterations); `iterations` / `delta` stay exact"""
        return self._engine.history_truncated()

    def solve(self, rho0, dt, px, pm, pvol, vx, vy, sphi, sv, lphi, lvol, wx=None, wy=None, tol=1e-3):
        """`vx`, `vy`, `sv` are accepted and never read, as in the reference; `px` is moved in place, in its dtype."""
        g, eng = self._g, self._engine
        if wx is None or wy is None:
            compute_solid_frac(self.gres, sphi, self.wx, self.wy)
            wx, wy = self.wx, self.wy
        with torch.cuda.device(self.x.device):
            self.m *= 0          # multiplies, not fills: NaN / inf survive as in the reference (:267-269)
            self.vol *= 0
            self.x *= 0
            initialize_density(self.bound_min, self.cell_size, g, px, pm, pvol, self.m, self.vol, sphi, lphi)
            fix_volume(self.cell_size, g, lvol, self.vol, sphi, lphi, wx, wy)
            initialize_solver(rho0, dt, g, self.cell_size, self.m, self.vol, lphi, wx, wy, self.buf.b)
            eng.setup_density(lphi, wx, wy)
            eng.bind(self.buf.b, self.x, self.buf.d, self.buf.r, self.buf.q)
            self.converged, self.iterations = eng.solve(tol, self.max_iter, self.check_every)
            p = eng.poll()
            self.alpha, self.beta, self.delta = p["alpha"], p["beta"], p["delta"]
            # self.x : -pressure * dt / rho / dx^2
            compute_displacement(g, dt, self.cell_size, self.dx, self.dy, self.x, lphi)
            apply_displacement(px, self.dx, self.bound_min, self.cell_size, self.bias_x, 0)
            apply_displacement(px, self.dy, self.bound_min, self.cell_size, self.bias_y, 1)
