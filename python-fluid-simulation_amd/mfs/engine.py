"""What every Python owner of a CG engine handle (include/mfs.h: mfs_pcg3d, mfs_vcg3d, mfs_pcg2d, mfs_vcg2d) shares:
the device workspace allocated with torch and kept alive, the handle's lifetime, bind / poll / solve / history.  The four
engines run on one C core (csrc/mfs_cg_core.h) and spell these entry points alike, so a subclass names its C prefix and
its grid rank and adds only the entries that are its own."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib, tensors as T


class CgEngine:
    PREFIX = None      # "mfs_pcg3d", ...
    RANK = None        # 2 | 3
    C_ENTRIES = ("workspace_bytes", "create", "destroy", "bind", "poll", "solve", "history")

    @classmethod
    def c_names(cls):
        """every C name this class forms from its prefix (tests/test_abi.py holds them against _lib.SIGNATURES)"""
        return [f"{cls.PREFIX}_{e}" for e in cls.C_ENTRIES + (("scalars",) if cls.RANK == 3 else ())]

    def _c(self, entry):
        """C entry point of this engine.  Construction only: methods call what __init__ resolved"""
        name = f"{self.PREFIX}_{entry}"
        assert name in self.c_names(), name
        return getattr(self.lib, name)

    def __init__(self, gres, dtype, device=None):
        self.lib = _lib.load()
        self.gres = T.as_gres(gres)
        if len(self.gres) != self.RANK:
            raise ValueError(f"{type(self).__name__} is {self.RANK}D")
        self.dtype = T.state_dtype(dtype)
        self.code = _lib.MFS_F32 if self.dtype == torch.float32 else _lib.MFS_F64
        self.device = torch.device("cuda" if device is None else device)
        self._c_destroy, self._c_bind, self._c_poll = self._c("destroy"), self._c("bind"), self._c("poll")
        self._c_solve, self._c_history = self._c("solve"), self._c("history")
        g = _lib.i64x(self.gres)
        nbytes = int(self._c("workspace_bytes")(g, self.code))
        if nbytes <= 0:
            raise _lib.MfsError(f"{self.PREFIX}_workspace_bytes returned 0")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(self._c("create")(C.byref(h), g, self.code, T.ptr(self.workspace), nbytes, T.stream()),
                       f"{self.PREFIX}_create")
        self.h = h
        # the engine's scalar block is the first bytes of the workspace (core_carve; all-reduced in place by mfs.dist)
        self.scalars = self.workspace[: _lib.NSCALARS * 8].view(torch.float64)
        if self.RANK == 3:      # the 2D engines have no *_scalars entry point
            assert self.scalars.data_ptr() == self._c("scalars")(self.h)
        self._bound = None

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self._c_destroy(h)
            except Exception:
                pass

    def _vector(self, t, name):
        """a CG vector of this engine: one entry per cell, unless the subclass says otherwise"""
        return T.dev(t, name, self.gres)

    def bind(self, b, x, d, r, q):
        ts = [self._vector(a, n) for a, n in ((b, "b"), (x, "x"), (d, "d"), (r, "r"), (q, "q"))]
        for t in ts:
            if t.dtype != self.dtype:
                raise TypeError(f"CG vectors must be {self.dtype}, got {t.dtype}")
        _lib.check(self._c_bind(self.h, *[T.ptr(t) for t in ts]), self._c_bind.__name__)
        self._bound = ts          # keep the tensors alive while the engine points at them

    def poll(self):
        it, done = C.c_int64(), C.c_int()
        delta, alpha, beta = C.c_double(), C.c_double(), C.c_double()
        _lib.check(self._c_poll(self.h, T.stream(), C.byref(it), C.byref(done), C.byref(delta), C.byref(alpha),
                                C.byref(beta)), self._c_poll.__name__)
        return dict(iterations=it.value, done=bool(done.value), delta=delta.value, alpha=alpha.value,
                    beta=beta.value)

    def poll_raw(self):
        """the scalar block as it stands, WITHOUT raising on the loop's error word (diagnostics after a failed solve)"""
        s = self.scalars.cpu()
        return dict(iterations=int(s[_lib.S_ITERS]), done=bool(s[_lib.S_DONE] != 0), delta=float(s[_lib.S_LASTRR]),
                    err=int(s[_lib.S_ERR]))

    def solve(self, tol, max_iter, check_every=32):
        it = C.c_int64()
        st = _lib.check(self._c_solve(self.h, float(tol), int(max_iter), int(check_every), T.stream(), C.byref(it)),
                        self._c_solve.__name__)
        return st == _lib.MFS_OK, it.value

    def history(self):
        cap = int(self.lib.mfs_pcg3d_history_capacity())
        buf = np.empty(cap, dtype=np.float64)
        n = self._c_history(self.h, buf.ctypes.data_as(C.POINTER(C.c_double)), cap, T.stream())
        _lib.check(int(n), self._c_history.__name__)
        return buf[: int(n)].copy()

    def history_truncated(self):
        """True when the solve ran past the history buffer (capacity mfs_pcg3d_history_capacity() doubles = 8 191 iterations):
        history() then holds the LEADING entries only -- `iterations`, `delta`, alpha and beta come from the engine's scalar
        block (poll()), never from the history, and stay exact"""
        cap = int(self.lib.mfs_pcg3d_history_capacity())
        return 2 * int(self.poll_raw()["iterations"]) + 1 > cap


class FaceCgEngine(CgEngine):
    """the viscosity engines: CG over flat [x-faces | y-faces (| z-faces)] vectors"""
    C_ENTRIES = CgEngine.C_ENTRIES + ("dofs", "setup", "apply")

    def __init__(self, gres, dtype, device=None):
        super().__init__(gres, dtype, device)
        self.dofs = int(self._c("dofs")(_lib.i64x(self.gres)))
        self.face_shapes = [T.face_shape(self.gres, a) for a in range(self.RANK)]
        self._c_setup, self._c_apply = self._c("setup"), self._c("apply")

    def new_vector(self):
        """flat face vector plus its component views, one per axis"""
        flat = torch.zeros(self.dofs, dtype=self.dtype, device=self.workspace.device)
        views, o = [], 0
        for shp in self.face_shapes:
            n = int(np.prod(shp))
            views.append(flat[o:o + n].view(shp))
            o += n
        return flat, views

    def setup(self, scale, mu, sphi, vol):
        sphi = T.dev(sphi, "sphi", T.doubled_shape(self.gres))
        vol = T.dev(vol, "vol", T.doubled_shape(self.gres))
        _lib.check(self._c_setup(self.h, float(scale), float(mu), T.ptr(sphi), T.code(sphi), T.ptr(vol), T.code(vol),
                                 T.stream()), self._c_setup.__name__)

    def _flat(self, t, name):
        t = T.dev(t, name, (self.dofs,))
        if t.dtype != self.dtype:
            raise TypeError(f"{name} must be {self.dtype}")
        return t

    _vector = _flat

    def apply(self, v, out):
        """out = A v (faces without an equation untouched); setup() first"""
        v, out = self._flat(v, "v"), self._flat(out, "out")
        _lib.check(self._c_apply(self.h, T.ptr(v), T.ptr(out), T.stream()), self._c_apply.__name__)
