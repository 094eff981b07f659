"""Drop-in for the reference's solver/ViscosityCGSolver2D.py on MI355X.

Same module functions (`initialize_solver`, `matvecmul`, `apply_viscosity`), class, constructor and `solve`
signature as the reference, on PyTorch-ROCm tensors, calling the HIP kernels of libmfs_hip.so through the C ABI
(include/mfs.h, csrc/mfs_visc2d.hip).  No CPU path.

The 2D reference differs from the 3D one, and the drop-in keeps the differences: a face sample is solid where
sphi <= 0; there is no extrapolation step; `vol = lvol / (cell_vol * 0.125)` with cell_vol the cell area; `sv`,
`lphi` and `save` are accepted and never read; boundary faces of b / out are never written; the CG starts from
x = v; the default tol is 1e-4.
"""
import numpy as np
import torch

from mfs import _lib, tensors as T
from mfs.vcg import Vcg2dEngine


def _comps(g, a, b, names):
    out = [T.dev(t, n, T.face_shape(g, ax)) for ax, (t, n) in enumerate(zip((a, b), names))]
    if out[0].dtype != out[1].dtype:
        raise TypeError(f"{names} must share a dtype")
    return out


def _g2(gres):
    g = T.as_gres(gres)
    if len(g) != 2:
        raise ValueError("the 2D viscosity solver needs a 2D grid")
    return g


def initialize_solver(gres, scale, mu, vx, vy, sphi, sv, vol, b_x, b_y):
    """viscosity RHS (reference :222-229 -> kernels :6-103).  `sv` is accepted and unused, as in the reference."""
    g = _g2(gres)
    vx, vy = _comps(g, vx, vy, ("vx", "vy"))
    b_x, b_y = _comps(g, b_x, b_y, ("b_x", "b_y"))
    sphi = T.dev(sphi, "sphi", T.doubled_shape(g))
    vol = T.dev(vol, "vol", T.doubled_shape(g))
    lib = _lib.load()
    _lib.check(lib.mfs_visc_rhs2d(_lib.i64x(g), float(scale), float(mu), T.ptr(vx), T.ptr(vy), T.code(vx),
                                  T.ptr(sphi), T.code(sphi), T.ptr(vol), T.code(vol), T.ptr(b_x), T.ptr(b_y),
                                  T.code(b_x), T.stream()), "mfs_visc_rhs2d")


def matvecmul(gres, scale, mu, vx, vy, out_x, out_y, sphi, vol):
    """the coupled 2-component viscosity operator (reference :231-238 -> kernels :105-207)."""
    g = _g2(gres)
    vx, vy = _comps(g, vx, vy, ("vx", "vy"))
    out_x, out_y = _comps(g, out_x, out_y, ("out_x", "out_y"))
    sphi = T.dev(sphi, "sphi", T.doubled_shape(g))
    vol = T.dev(vol, "vol", T.doubled_shape(g))
    lib = _lib.load()
    _lib.check(lib.mfs_visc_apply2d(_lib.i64x(g), float(scale), float(mu), T.ptr(vx), T.ptr(vy), T.code(vx),
                                    T.ptr(out_x), T.ptr(out_y), T.code(out_x), T.ptr(sphi), T.code(sphi), T.ptr(vol),
                                    T.code(vol), T.stream()), "mfs_visc_apply2d")


def apply_viscosity(gres, vx, vy, out_x, out_y, sphi, sv):
    """copy the solution into the non-solid faces of vx, vy, in place (reference :240-244 -> :209-220)."""
    g = _g2(gres)
    vx, vy = _comps(g, vx, vy, ("vx", "vy"))
    out_x, out_y = _comps(g, out_x, out_y, ("out_x", "out_y"))
    sphi = T.dev(sphi, "sphi", T.doubled_shape(g))
    lib = _lib.load()
    _lib.check(lib.mfs_visc_writeback2d(_lib.i64x(g), T.ptr(vx), T.ptr(vy), T.code(vx), T.ptr(out_x), T.ptr(out_y),
                                        T.code(out_x), T.ptr(sphi), T.code(sphi), T.stream()),
               "mfs_visc_writeback2d")


class ViscosityCGSolver2D:
    """Reference :246-317.  `ViscosityCGSolver2D(gres, bound_size)`;
    `solve(dt, mu, rho, vx, vy, sphi, sv, lphi, lvol, tol=1e-4, save=False)`.

    The ten solver-owned CG arrays keep the reference's names and shapes (`x_x`, `d_y`, ...); each is a view into
    one flat [x-faces | y-faces] allocation per vector, so the vector phases of the CG run as single launches over
    both components.  Extras: `iterations`, `history`, `history_truncated`; `precision` / MFS_PRECISION selects fp32
    state; the host looks at the device-resident loop every `check_every` iterations.
    """

    def __init__(self, gres, bound_size, precision=None, device=None, check_every=32):
        self.gres = gres
        self._g = _g2(gres)
        self.cell_size = np.array(T.as_f64_list(bound_size, 2)) / np.array(self._g, dtype=np.float64)
        self.cell_vol = float(np.prod(self.cell_size))
        self.precision = T.state_dtype(precision)
        self.device = torch.device("cuda" if device is None else device)
        self._engine = Vcg2dEngine(self._g, self.precision, self.device)
        self.vol = torch.zeros(T.doubled_shape(self._g), dtype=torch.float64, device=self.device)
        self._flat = {}
        for nm in "drqxb":
            flat, views = self._engine.new_vector()
            self._flat[nm] = flat
            for c, v in zip("xy", views):
                setattr(self, f"{nm}_{c}", v)
        self.alpha = 0.0
        self.beta = 0.0
        self.delta = 0.0
        self.max_iter = int(np.prod(self._g))
        self.check_every = int(check_every)
        self.iterations = 0

    @property
    def history(self):
        """[delta0, dq1, delta1, dq2, delta2, ...] of the last solve"""
        return self._engine.history()

    @property
    def history_truncated(self):
        """True if the last solve ran past the history buffer: `history` then holds its leading entries only;
        `iterations`, `delta`, `alpha`, `beta` are exact regardless"""
        return self._engine.history_truncated()

    def solve(self, dt, mu, rho, vx, vy, sphi, sv, lphi, lvol, tol=1e-4, save=False):
        """`sv`, `lphi` and `save` are accepted and never read (reference :266)."""
        g = self._g
        scale = dt / self.cell_vol / rho                                   # :267
        lvol = T.dev(lvol, "lvol", T.doubled_shape(g))
        sphi = T.dev(sphi, "sphi", T.doubled_shape(g))
        vx, vy = _comps(g, vx, vy, ("vx", "vy"))
        eng = self._engine
        with torch.cuda.device(self.vol.device):
            # :269 -- a true division (a host scalar divisor would make torch multiply by its reciprocal)
            torch.div(lvol, torch.tensor(self.cell_vol * 0.125, dtype=torch.float64, device=lvol.device), out=self.vol)
            self.x_x.copy_(vx)                                             # :270-271 (dtype cast)
            self.x_y.copy_(vy)
            initialize_solver(g, scale, mu, self.x_x, self.x_y, sphi, sv, self.vol, self.b_x, self.b_y)   # :273
            eng.setup(scale, mu, sphi, self.vol)
            f = self._flat
            eng.bind(f["b"], f["x"], f["d"], f["r"], f["q"])
            ok, self.iterations = eng.solve(tol, self.max_iter, self.check_every)   # :274-315
            st = eng.poll()
            self.alpha, self.beta, self.delta = st["alpha"], st["beta"], st["delta"]
            if not ok:
                raise ValueError("Failed to converge!")
            apply_viscosity(g, vx, vy, self.x_x, self.x_y, sphi, sv)     # :317
