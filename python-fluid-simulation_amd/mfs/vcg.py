"""Python owners of the viscosity engine handles `mfs_vcg3d` and `mfs_vcg2d` (include/mfs.h): CG over face vectors."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, tensors as T
from .engine import FaceCgEngine


class VcgEngine(FaceCgEngine):
    PREFIX, RANK = "mfs_vcg3d", 3

    def apply_kernel(self):
        """which kernel the CG applies take for the engine as bound: "march" | "scalar" (bit-identical).  Code 1, the
        LDS-tiled kernel, is retired: the library returns 2 or 0"""
        return {2: "march", 0: "scalar"}[int(self.lib.mfs_vcg3d_apply_kernel(self.h))]

    def begin(self, tol):
        _lib.check(self.lib.mfs_vcg3d_begin(self.h, float(tol), T.stream()), "mfs_vcg3d_begin")

    def iterate(self, n):
        _lib.check(self.lib.mfs_vcg3d_iterate(self.h, int(n), T.stream()), "mfs_vcg3d_iterate")

    def finish(self):
        """settle what the fused loop of `iterate` owes (last x update, d brought home); begin again before iterating on"""
        _lib.check(self.lib.mfs_vcg3d_finish(self.h, T.stream()), "mfs_vcg3d_finish")

    def set_compress(self, on):
        """compressed class access of the marching kernel (default on): bit-identical, fewer bytes where the liquid
        volume is 0 or 1 over whole z-vectors"""
        _lib.check(self.lib.mfs_vcg3d_set_compress(self.h, int(bool(on))), "mfs_vcg3d_set_compress")

    def class_census(self):
        """{"zero", "one", "mixed"}: z-vectors per class of the compressed class access (after setup)"""
        out = _lib.i64x([0, 0, 0])
        _lib.check(self.lib.mfs_vcg3d_class_census(self.h, out, T.stream()), "mfs_vcg3d_class_census")
        return {"zero": int(out[0]), "one": int(out[1]), "mixed": int(out[2])}

    def set_sparse(self, on):
        """single-domain solves from 2^21 unknowns: live-chunk vector phases + work list of the loop's march launches"""
        _lib.check(self.lib.mfs_vcg3d_set_sparse(self.h, int(bool(on))), "mfs_vcg3d_set_sparse")

    def sparse_info(self):
        out = _lib.i64x([0] * 4)
        _lib.check(self.lib.mfs_vcg3d_sparse_info(self.h, T.stream(), out), "mfs_vcg3d_sparse_info")
        return dict(live_chunks=int(out[0]), chunks=int(out[1]), listed_pairs=int(out[2]), pairs=int(out[3]))

    def set_fuse(self, on):
        _lib.check(self.lib.mfs_vcg3d_set_fuse(self.h, int(bool(on))), "mfs_vcg3d_set_fuse")

    def loop_info(self):
        """{"fused": iterate() runs the 2-launch loop with the direction and x updates folded into the marching kernel}"""
        b = int(self.lib.mfs_vcg3d_loop_info(self.h))
        return {"fused": bool(b & 1), "merged_vector_phases": bool(b & 2), "jacobi": bool(b & 4), "resident": bool(b & 8)}

    def set_resident(self, on):
        """small grids: the whole CG loop as one resident launch per iterate() batch (default on where the grid qualifies)"""
        _lib.check(self.lib.mfs_vcg3d_set_resident(self.h, int(bool(on))), "mfs_vcg3d_set_resident")

    def set_jacobi(self, on):
        """opt-in Jacobi preconditioning (NOT the reference's CG: fewer iterations, another residual history); takes effect
        at the next setup()"""
        _lib.check(self.lib.mfs_vcg3d_set_jacobi(self.h, int(bool(on))), "mfs_vcg3d_set_jacobi")

    def set_merged(self, on):
        """small problems: r update, r.r, bookkeeping and x / direction updates in one launch (default on)"""
        _lib.check(self.lib.mfs_vcg3d_set_merged(self.h, int(bool(on))), "mfs_vcg3d_set_merged")

    # ---- slab decomposition (mfs/dist.py:SlabVCG): the phases of one iteration
    def set_slab(self, skip_top_x):
        _lib.check(self.lib.mfs_vcg3d_set_slab(self.h, int(bool(skip_top_x))), "mfs_vcg3d_set_slab")

    def begin_local(self, tol):
        _lib.check(self.lib.mfs_vcg3d_begin_local(self.h, float(tol), T.stream()), "mfs_vcg3d_begin_local")

    def begin_finish(self):
        _lib.check(self.lib.mfs_vcg3d_begin_finish(self.h, T.stream()), "mfs_vcg3d_begin_finish")

    def phase_apply(self):
        _lib.check(self.lib.mfs_vcg3d_phase_apply(self.h, T.stream()), "mfs_vcg3d_phase_apply")

    def phase_reduce(self, which):
        _lib.check(self.lib.mfs_vcg3d_phase_reduce(self.h, int(which), T.stream()), "mfs_vcg3d_phase_reduce")

    def phase_update_xr(self):
        _lib.check(self.lib.mfs_vcg3d_phase_update_xr(self.h, T.stream()), "mfs_vcg3d_phase_update_xr")

    def phase_update_d(self):
        _lib.check(self.lib.mfs_vcg3d_phase_update_d(self.h, T.stream()), "mfs_vcg3d_phase_update_d")

    # ---- the same loop over a peer-to-peer window (mfs/p2p.py): no host-side exchange inside the loop
    def edge_plane_bytes(self):
        """bytes of the three edge planes one neighbour receives per iteration (the window's plane size)"""
        return sum(int(np.prod(shp[1:])) for shp in self.face_shapes) * torch.empty(0, dtype=self.dtype).element_size()

    def attach_p2p(self, window):
        self._window = window            # keep it alive as long as the engine may use it
        _lib.check(self.lib.mfs_vcg3d_attach_p2p(self.h, window.h if window is not None else None), "mfs_vcg3d_attach_p2p")

    def slab_begin(self, tol):
        _lib.check(self.lib.mfs_vcg3d_slab_begin(self.h, float(tol), T.stream()), "mfs_vcg3d_slab_begin")

    def slab_iterate(self, n):
        _lib.check(self.lib.mfs_vcg3d_slab_iterate(self.h, int(n), T.stream()), "mfs_vcg3d_slab_iterate")


class Vcg2dEngine(FaceCgEngine):
    """Python owner of one `mfs_vcg2d` engine handle (include/mfs.h): the 2D viscosity CG over flat
    [x-faces | y-faces] vectors."""
    PREFIX, RANK = "mfs_vcg2d", 2
