"""ctypes binding of libmfs_hip.so (the C ABI declared in include/mfs.h).

The product path has NO fallback: if the HIP library is missing or a call fails,
this module raises.  torch is imported before the library is opened so that the
library's dependency on libamdhip64.so.7 resolves to the HIP runtime PyTorch
already loaded -- one runtime per process, so torch streams / device pointers are
valid inside the kernels' launches.
"""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must precede CDLL: see module docstring)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFS_LIB") or os.path.join(_HERE, "libmfs_hip.so")   # MFS_LIB: A/B builds of the same ABI

MFS_F32, MFS_F64 = 0, 1
MFS_OK, MFS_NOT_CONVERGED = 0, 1
MFS_E_TIMEOUT, MFS_E_ZERODIV, MFS_E_NONFINITE = -4, -5, -6
ABI_VERSION = 3

# scalar slots of the CG engine's device block (include/mfs.h)
S_DQ, S_RR, S_DELTA, S_TOL2, S_DONE, S_ITERS, S_ALPHA, S_BETA, S_LASTRR = range(9)
S_ERR = 11         # != 0: the device loop stopped itself (include/mfs.h: MFS_PCG_S_ERR)
S_LANE = 13        # pressure engine, diagnostics: 1 when the solve's listed launches mask dead lanes (csrc/mfs_pcg_apply.h LMASK)
NSCALARS = 16


class MfsError(RuntimeError):
    pass


class MfsTimeout(MfsError, TimeoutError):
    """MFS_E_TIMEOUT: a peer rank did not answer (window loop: MFS_P2P_TIMEOUT_MS; collective loop:
    MFS_COLLECTIVE_TIMEOUT_S).  The solve was stopped; nothing is left spinning on the GPU."""
    status = MFS_E_TIMEOUT


class MfsZeroDivision(ZeroDivisionError):
    """MFS_E_ZERODIV: d.q == 0 inside the CG loop.  The reference's `alpha = self.delta / cp.sum(d*q).item()`
    raises ZeroDivisionError there (solver/PressureCGSolver3D.py:211); so do the drop-ins."""


class MfsNonFinite(FloatingPointError, ValueError):
    """MFS_E_NONFINITE: d.q or r.r became NaN / inf (poisoned inputs).  The reference never sees `nan < tol**2`
    come true, iterates max_iter = prod(gres) times and raises ValueError("Failed to converge!")
    (PressureCGSolver3D.py:222-223); the device loop stops at the first non-finite dot product instead.  Subclass of
    both FloatingPointError (what happened) and ValueError (what the reference's caller would have caught)."""


_p, _i, _i64, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_double, C.c_size_t
_pi64 = C.POINTER(C.c_int64)
_pd = C.POINTER(C.c_double)
_pint = C.POINTER(C.c_int)

# name -> (restype, argtypes).  Mirrors include/mfs.h one to one
# (tests/test_abi.py checks the header against this table and the built .so).
SIGNATURES = {
    "mfs_abi_version": (_i, []),
    "mfs_last_error": (C.c_char_p, []),
    "mfs_device_name": (_i, [C.c_char_p, _sz]),
    "mfs_solid_frac3d": (_i, [_pi64, _p, _i, _p, _p, _p, _i, _p]),
    "mfs_solid_frac2d": (_i, [_pi64, _p, _i, _p, _p, _i, _p]),
    "mfs_pressure_rhs3d": (_i, [_pi64, _pd, _p, _p, _p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _p]),
    "mfs_pressure_apply3d": (_i, [_pi64, _p, _p, _i, _p, _p, _p, _i, _p, _i, _p]),
    "mfs_pressure_update3d": (_i, [_pi64, _pd, _p, _p, _p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _p, _i, _p]),
    "mfs_pcg3d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_pcg3d_history_capacity": (_i64, []),
    "mfs_pcg3d_create": (_i, [C.POINTER(_p), _pi64, _i, _p, _sz, _p]),
    "mfs_pcg3d_destroy": (_i, [_p]),
    "mfs_pcg3d_setup": (_i, [_p, _p, _i, _p, _p, _p, _i, _p]),
    "mfs_pcg3d_apply": (_i, [_p, _p, _p, _i64, _i64, _p]),
    "mfs_pcg3d_bind": (_i, [_p, _p, _p, _p, _p, _p]),
    "mfs_pcg3d_begin": (_i, [_p, _d, _p]),
    "mfs_pcg3d_iterate": (_i, [_p, _i64, _p]),
    "mfs_pcg3d_native_apply": (_i, [_p, _p]),
    "mfs_pcg3d_native_finish": (_i, [_p, _p]),
    "mfs_pcg3d_poll": (_i, [_p, _p, _pi64, _pint, _pd, _pd, _pd]),
    "mfs_pcg3d_solve": (_i, [_p, _d, _i64, _i64, _p, _pi64]),
    "mfs_pcg3d_history": (_i64, [_p, _pd, _i64, _p]),
    "mfs_pcg3d_phase_apply": (_i, [_p, _i64, _i64, _i, _p]),
    "mfs_pcg3d_phase_apply2": (_i, [_p, _i64, _i64, _i64, _i64, _i, _p]),
    "mfs_pcg3d_phase_reduce": (_i, [_p, _i, _p]),
    "mfs_pcg3d_phase_update_xr": (_i, [_p, _p]),
    "mfs_pcg3d_phase_update_r": (_i, [_p, _p]),
    "mfs_pcg3d_phase_update_x": (_i, [_p, _p]),
    "mfs_pcg3d_phase_update_d": (_i, [_p, _p]),
    "mfs_pcg3d_begin_local": (_i, [_p, _d, _p]),
    "mfs_pcg3d_begin_finish": (_i, [_p, _p]),
    "mfs_pcg3d_scalars": (_p, [_p]),
    "mfs_pcg3d_tune": (_i, [_p, _i, _i, _i, _i]),
    "mfs_pcg3d_loop_info": (_i, [_p]),
    "mfs_pcg3d_set_sparse": (_i, [_p, _i]),
    "mfs_pcg3d_sparse_info": (_i, [_p, _p, _pi64]),
    "mfs_pcg3d_set_jacobi": (_i, [_p, _i]),
    "mfs_pcg3d_set_defer_x": (_i, [_p, _i]),
    "mfs_pcg3d_set_lean": (_i, [_p, _i]),
    "mfs_pcg3d_set_resident": (_i, [_p, _i]),
    "mfs_pcg3d_finish": (_i, [_p, _p]),
    "mfs_pcg3d_set_compress": (_i, [_p, _i]),
    "mfs_pcg3d_set_fuse": (_i, [_p, _i]),
    "mfs_pcg3d_set_prefetch": (_i, [_p, _i]),
    "mfs_p2p_handle_bytes": (_sz, []),
    "mfs_p2p_create": (_i, [C.POINTER(_p), _i, _i, _sz, _p]),
    "mfs_p2p_connect": (_i, [_p, _p]),
    "mfs_p2p_selftest": (_i, [_p, _i, _p, _pint, C.POINTER(C.c_uint)]),
    "mfs_p2p_info": (_i, [_p, _pint, C.POINTER(_sz)]),
    "mfs_p2p_destroy": (_i, [_p]),
    "mfs_pcg3d_attach_p2p": (_i, [_p, _p]),
    "mfs_pcg3d_slab_supported": (_i, [_p]),
    "mfs_rccl_unique_id_bytes": (_i, []),
    "mfs_rccl_unique_id": (_i, [C.c_char_p, _p]),
    "mfs_rccl_create": (_i, [C.POINTER(_p), C.c_char_p, _p, _i, _i]),
    "mfs_rccl_destroy": (_i, [_p]),
    "mfs_pcg3d_attach_rccl": (_i, [_p, _p, _p]),
    "mfs_pcg3d_slab_set_aux": (_i, [_p, _i]),
    "mfs_pcg3d_slab_begin": (_i, [_p, _d, _p]),
    "mfs_pcg3d_slab_iterate": (_i, [_p, _i64, _p]),
    "mfs_pcg3d_slab_solve": (_i, [_p, _d, _i64, _i64, _p, _pi64]),
    "mfs_visc_extrapolate3d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_visc_extrapolate3d": (_i, [_pi64, _i, _p, _p, _p, _i, _p, _i, _p, _sz, _p]),
    "mfs_visc_rhs3d": (_i, [_pi64, _d, _d, _p, _p, _p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _p]),
    "mfs_visc_apply3d": (_i, [_pi64, _d, _d, _p, _p, _p, _i, _p, _p, _p, _i, _p, _i, _p, _i, _p]),
    "mfs_visc_writeback3d": (_i, [_pi64, _p, _p, _p, _i, _p, _p, _p, _i, _p, _i, _p]),
    "mfs_vcg3d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_vcg3d_dofs": (_i64, [_pi64]),
    "mfs_vcg3d_create": (_i, [C.POINTER(_p), _pi64, _i, _p, _sz, _p]),
    "mfs_vcg3d_destroy": (_i, [_p]),
    "mfs_vcg3d_setup": (_i, [_p, _d, _d, _p, _i, _p, _i, _p]),
    "mfs_vcg3d_apply": (_i, [_p, _p, _p, _p]),
    "mfs_vcg3d_bind": (_i, [_p, _p, _p, _p, _p, _p]),
    "mfs_vcg3d_begin": (_i, [_p, _d, _p]),
    "mfs_vcg3d_iterate": (_i, [_p, _i64, _p]),
    "mfs_vcg3d_poll": (_i, [_p, _p, _pi64, _pint, _pd, _pd, _pd]),
    "mfs_vcg3d_solve": (_i, [_p, _d, _i64, _i64, _p, _pi64]),
    "mfs_vcg3d_finish": (_i, [_p, _p]),
    "mfs_vcg3d_set_fuse": (_i, [_p, _i]),
    "mfs_vcg3d_set_compress": (_i, [_p, _i]),
    "mfs_vcg3d_set_resident": (_i, [_p, _i]),
    "mfs_vcg3d_class_census": (_i, [_p, _pi64, _p]),
    "mfs_vcg3d_set_sparse": (_i, [_p, _i]),
    "mfs_vcg3d_sparse_info": (_i, [_p, _p, _pi64]),
    "mfs_vcg3d_loop_info": (_i, [_p]),
    "mfs_vcg3d_set_merged": (_i, [_p, _i]),
    "mfs_vcg3d_set_jacobi": (_i, [_p, _i]),
    "mfs_vcg3d_history": (_i64, [_p, _pd, _i64, _p]),
    "mfs_vcg3d_apply_kernel": (_i, [_p]),
    "mfs_vcg3d_set_slab": (_i, [_p, _i]),
    "mfs_vcg3d_scalars": (_p, [_p]),
    "mfs_vcg3d_begin_local": (_i, [_p, _d, _p]),
    "mfs_vcg3d_begin_finish": (_i, [_p, _p]),
    "mfs_vcg3d_phase_apply": (_i, [_p, _p]),
    "mfs_vcg3d_phase_reduce": (_i, [_p, _i, _p]),
    "mfs_vcg3d_phase_update_xr": (_i, [_p, _p]),
    "mfs_vcg3d_phase_update_d": (_i, [_p, _p]),
    "mfs_vcg3d_attach_p2p": (_i, [_p, _p]),
    "mfs_vcg3d_slab_begin": (_i, [_p, _d, _p]),
    "mfs_vcg3d_slab_iterate": (_i, [_p, _i64, _p]),
    "mfs_visc_valid3d": (_i, [_pi64, _i, _p, _i, _p, _p]),
    "mfs_visc_extrapolate_sweep3d": (_i, [_pi64, _i, _p, _p, _i, _p, _p, _p]),
    "mfs_grid_extrapolate3d": (_i, [_pi64, _i, _p, _p, _p, _i, _p, _p, _p, _i, _p, _sz, _p]),
    "mfs_grid_boundary_condition3d": (_i, [_pi64, _p, _p, _p, _i, _p, _p, _p, _i, _p, _i, _p, _i, _d, _p, _p, _p, _i, _p]),
    "mfs_pcg3d_setup_density": (_i, [_p, _p, _i, _p, _p, _p, _i, _p]),
    "mfs_density_splat3d": (_i, [_pi64, _pd, _pd, _p, _i, _p, _i, _d, _i64, _p, _p, _i, _p]),
    "mfs_density_fix_volume3d": (_i, [_pi64, _pd, _p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _p]),
    "mfs_density_rhs3d": (_i, [_pi64, _d, _d, _pd, _p, _p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _p]),
    "mfs_density_apply3d": (_i, [_pi64, _p, _p, _i, _p, _p, _p, _i, _p, _i, _p]),
    "mfs_density_displacement3d": (_i, [_pi64, _d, _pd, _p, _p, _p, _i, _p, _i, _p, _i, _p]),
    "mfs_density_advect3d": (_i, [_p, _i, _i64, _p, _i, _pi64, _pd, _pd, _pd, _i, _p]),
    "mfs_density_splat2d": (_i, [_pi64, _pd, _pd, _p, _i, _p, _i, _d, _i64, _p, _p, _i, _p]),
    "mfs_density_fix_volume2d": (_i, [_pi64, _pd, _p, _i, _p, _i, _p, _i, _p, _i, _p, _p, _i, _p]),
    "mfs_density_rhs2d": (_i, [_pi64, _d, _d, _pd, _p, _p, _i, _p, _i, _p, _p, _i, _p, _i, _p]),
    "mfs_density_apply2d": (_i, [_pi64, _p, _p, _i, _p, _p, _i, _p, _i, _p]),
    "mfs_density_displacement2d": (_i, [_pi64, _d, _pd, _p, _p, _i, _p, _i, _p, _i, _p]),
    "mfs_density_advect2d": (_i, [_p, _i, _i64, _p, _i, _pi64, _pd, _pd, _pd, _i, _p]),
    "mfs_p2g_scatter3d": (_i, [_pi64, _pd, _pd, _pd, _i, _p, _i, _p, _i, _p, _i, _p, _i, _i64, _p, _p, _i, _p]),
    "mfs_p2g_normalize3d": (_i, [_i64, _p, _p, _i, _p]),
    "mfs_particle_tiles3d": (_i64, [_pi64]),
    "mfs_particle_tile_sort3d": (_i, [_pi64, _pd, _pd, _p, _i, _i64, _p, _p, _p, _p]),
    "mfs_p2g_scatter3d_tiled": (_i, [_pi64, _pd, _pd, _pd, _i, _p, _i, _p, _i, _p, _i, _p, _i, _i64, _p, _p, _p, _p, _i, _p]),
    "mfs_fluid_levelset3d_tiled": (_i, [_pi64, _pd, _pd, _d, _p, _i, _i64, _p, _p, _p, _i, _p]),
    "mfs_density_splat3d_tiled": (_i, [_pi64, _pd, _pd, _p, _i, _p, _i, _d, _i64, _p, _p, _p, _p, _i, _p]),
    "mfs_fluid_volume3d_tiled": (_i, [_pi64, _pd, _pd, _p, _i, _d, _i64, _p, _p, _p, _i, _p]),
    "mfs_g2p_gather3d": (_i, [_pi64, _pd, _pd, _pd, _i, _p, _i, _p, _i, _p, _i, _i64, _p, _i, _p]),
    "mfs_fluid_levelset3d": (_i, [_pi64, _pd, _pd, _d, _p, _i, _i64, _p, _i, _p]),
    "mfs_fluid_volume3d": (_i, [_pi64, _pd, _pd, _p, _i, _d, _i64, _p, _i, _p]),
    "mfs_sdf_evaluate3d": (_i, [_p, _i64, _p, _i, _i64, _p, _i, _p, _i, _p]),
    "mfs_sdf_evaluate_grid3d": (_i, [_p, _i64, _p, _pi64, _pd, _pd, _pd, _p, _i, _p, _i, _p]),
    "mfs_sdf_project3d": (_i, [_p, _i64, _p, _i, _i64, _p]),
    "mfs_sdf_evaluate2d": (_i, [_p, _i64, _p, _i, _i64, _p, _i, _p, _i, _p]),
    "mfs_sdf_evaluate_grid2d": (_i, [_p, _i64, _p, _pi64, _pd, _pd, _pd, _p, _i, _p, _i, _p]),
    "mfs_sdf_project2d": (_i, [_p, _i64, _p, _i, _i64, _p]),
    "mfs_pressure_rhs2d": (_i, [_pi64, _pd, _p, _p, _i, _p, _i, _p, _i, _p, _p, _i, _p, _i, _p]),
    "mfs_pressure_apply2d": (_i, [_pi64, _p, _p, _i, _p, _p, _i, _p, _i, _p]),
    "mfs_pressure_update2d": (_i, [_pi64, _pd, _p, _p, _i, _p, _i, _p, _p, _i, _p, _i, _p, _i, _p]),
    "mfs_pcg2d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_pcg2d_create": (_i, [C.POINTER(_p), _pi64, _i, _p, _sz, _p]),
    "mfs_pcg2d_destroy": (_i, [_p]),
    "mfs_pcg2d_setup": (_i, [_p, _p, _i, _p, _p, _i]),
    "mfs_pcg2d_setup_density": (_i, [_p, _p, _i, _p, _p, _i]),
    "mfs_pcg2d_bind": (_i, [_p, _p, _p, _p, _p, _p]),
    "mfs_pcg2d_apply": (_i, [_p, _p, _p, _p]),
    "mfs_pcg2d_solve": (_i, [_p, _d, _i64, _i64, _p, _pi64]),
    "mfs_pcg2d_poll": (_i, [_p, _p, _pi64, _pint, _pd, _pd, _pd]),
    "mfs_pcg2d_history": (_i64, [_p, _pd, _i64, _p]),
    "mfs_visc_rhs2d": (_i, [_pi64, _d, _d, _p, _p, _i, _p, _i, _p, _i, _p, _p, _i, _p]),
    "mfs_visc_apply2d": (_i, [_pi64, _d, _d, _p, _p, _i, _p, _p, _i, _p, _i, _p, _i, _p]),
    "mfs_visc_writeback2d": (_i, [_pi64, _p, _p, _i, _p, _p, _i, _p, _i, _p]),
    "mfs_vcg2d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_vcg2d_dofs": (_i64, [_pi64]),
    "mfs_vcg2d_create": (_i, [C.POINTER(_p), _pi64, _i, _p, _sz, _p]),
    "mfs_vcg2d_destroy": (_i, [_p]),
    "mfs_vcg2d_setup": (_i, [_p, _d, _d, _p, _i, _p, _i, _p]),
    "mfs_vcg2d_bind": (_i, [_p, _p, _p, _p, _p, _p]),
    "mfs_vcg2d_apply": (_i, [_p, _p, _p, _p]),
    "mfs_vcg2d_solve": (_i, [_p, _d, _i64, _i64, _p, _pi64]),
    "mfs_vcg2d_poll": (_i, [_p, _p, _pi64, _pint, _pd, _pd, _pd]),
    "mfs_vcg2d_history": (_i64, [_p, _pd, _i64, _p]),
    "mfs_p2g_scatter2d": (_i, [_pi64, _pd, _pd, _pd, _i, _p, _i, _p, _i, _p, _i, _p, _i, _i64, _p, _p, _i, _p]),
    "mfs_g2p_gather2d": (_i, [_pi64, _pd, _pd, _pd, _i, _p, _i, _p, _i, _p, _i, _i64, _p, _i, _p]),
    "mfs_fluid_levelset2d": (_i, [_pi64, _pd, _pd, _d, _p, _i, _i64, _p, _i, _p]),
    "mfs_fluid_volume2d": (_i, [_pi64, _pd, _pd, _p, _i, _d, _i64, _p, _i, _p]),
    "mfs_grid_extrapolate2d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_grid_extrapolate2d": (_i, [_pi64, _i, _p, _p, _i, _p, _p, _i, _p, _sz, _p]),
    "mfs_grid_boundary_condition2d": (_i, [_pi64, _p, _p, _i, _p, _p, _i, _p, _i, _p, _i, _d, _p, _p, _i, _p]),
    "mfs_surface3d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_surface3d_count": (_i, [_pi64, _p, _i, _d, _i, _d, _p, _sz, _p]),
    "mfs_surface3d_fill": (_i, [_pi64, _p, _i, _d, _i, _d, _pd, _pd, _p, _sz, _p, _i64, _p, _i64, _p, _p]),
    "mfs_contour2d_workspace_bytes": (_sz, [_pi64, _i]),
    "mfs_contour2d_count": (_i, [_pi64, _p, _i, _d, _i, _d, _p, _sz, _p]),
    "mfs_contour2d_fill": (_i, [_pi64, _p, _i, _d, _i, _d, _pd, _pd, _p, _sz, _p, _i64, _p, _i64, _p]),
    "mfs_meshsdf_bricks3d": (_i64, [_pi64]),
    "mfs_meshsdf_distance3d": (_i, [_pi64, _pd, _d, _p, _i64, _i, _p, _p, _p]),
    "mfs_meshsdf_sign3d": (_i, [_pi64, _pd, _d, _p, _i64, _p, _p, _p]),
    "mfs_mesh_union_grid3d": (_i, [_p, _p, _i64, C.POINTER(_p), _pi64, _pd, _pd, _pi64, _pd, _pd, _pd, _p, _i, _p, _i, _p]),
    "mfs_mesh_project3d": (_i, [_p, _i64, C.POINTER(_p), _pi64, _pd, _pd, _p, _i, _i64, _p]),
    "mfs_skin_bricks3d": (_i64, [_pi64]),
    "mfs_skin_bins3d": (_i64, [_pi64]),
    "mfs_skin_keys3d": (_i, [_pi64, _pd, _d, _p, _i, _i64, _p, _p]),
    "mfs_skin_field3d": (_i, [_pi64, _pd, _d, _d, _d, _p, _i, _i64, _p, _p, _p, _p]),
    "mfs_seed_blocks3d": (_i64, [_pi64]),
    "mfs_seed_count3d": (_i, [_pi64, _pd, _d, _d, C.c_uint64, _i64, _i64, C.POINTER(_p), _pint, _pi64, _pd, _pd, _pd, _d,
                              _p, _p, _p]),
    "mfs_seed_fill3d": (_i, [_pi64, _pd, _d, _d, C.c_uint64, _p, _p, _p, _i, _p, _i64, _p]),
    "mfs_render_brick_count3d": (_i64, [_pi64]),
    "mfs_render_bricks3d": (_i, [_p, _i, _pi64, _p, _p]),
    "mfs_render_march3d": (_i, [_pd, _i, _i64, _i64, _d, _d, _i64, _i64, C.POINTER(_p), _pint, _pi64, _pd, _pd, _pd,
                                C.POINTER(_p), _i, _p, _p, _p, _p, _p, _p]),
    "mfs_render_shade3d": (_i, [_pd, _i, _i64, _i64, _p, _p, _i64, _pd, _pint, _pd, _p, _p]),
    "mfs_render_bricks_max3d": (_i, [_p, _i, _pi64, _p, _p]),
    "mfs_render_paths3d": (_i, [_pd, _i, _i64, _i64, _d, _d, _i64, _i64, C.POINTER(_p), _pint, _pi64, _pd, _pd, _pd,
                                C.POINTER(_p), C.POINTER(_p), _i, _pd, _pd, _pint, _i, _d, _i64, _i64, _p, _p, _p, _p, _p,
                                _p]),
    "mfs_render_resolve3d": (_i, [_p, _i64, _i64, _i, _p, _p]),
    "mfs_attrib_bins3d": (_i64, [_pi64]),
    "mfs_attrib_keys3d": (_i, [_pi64, _pd, _d, _pd, _p, _i, _i64, _p, _p]),
    "mfs_attrib_gather3d": (_i, [_pi64, _pd, _d, _i, _d, _p, _i, _p, _i, _i64, _p, _p, _i, _p, _i64, _p, _i64, _p, _p, _p,
                                 _p]),
    "mfs_render_shade_albedo3d": (_i, [_pd, _i, _i64, _i64, _p, _p, _i64, _pd, _pint, _pd, _p, _i64, _p, _p]),
}

_lib = None


def load():
    """Open libmfs_hip.so (once) and type every entry point.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the MI355X HIP kernels are not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C python-fluid-simulation_amd/csrc`). "
            "There is no CPU fallback for the solver path.")
    lib = C.CDLL(LIB_PATH)
    lib.mfs_abi_version.restype = _i
    lib.mfs_abi_version.argtypes = []
    v = lib.mfs_abi_version()
    # an older A/B build (tools/ab_libs.sh) may be loaded through MFS_LIB, but only on request: MFS_LIB_ALLOW_OLD_ABI=1
    # skips the version check and leaves entry points the build lacks untyped (calling one raises AttributeError)
    allow_old = bool(os.environ.get("MFS_LIB")) and os.environ.get("MFS_LIB_ALLOW_OLD_ABI") == "1"
    if v != ABI_VERSION and not allow_old:
        raise ImportError(f"{LIB_PATH}: ABI {v} != binding ABI {ABI_VERSION}; rebuild (`make -C python-fluid-simulation_amd/csrc`)"
                          + ("; MFS_LIB points at a stale build (MFS_LIB_ALLOW_OLD_ABI=1 loads it anyway, for A/B tools)"
                             if os.environ.get("MFS_LIB") else ""))
    missing = [name for name in SIGNATURES if not hasattr(lib, name)]
    if missing and not allow_old:
        raise ImportError(f"{LIB_PATH} lacks {len(missing)} declared entry points ({', '.join(missing[:4])}, ...); rebuild")
    for name, (res, args) in SIGNATURES.items():
        if name in missing:
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(status, what=""):
    """Raise MfsError for negative statuses; returns the status otherwise."""
    if status < 0:
        msg = load().mfs_last_error().decode(errors="replace")
        if status == MFS_E_ZERODIV:
            raise MfsZeroDivision(f"float division by zero ({what}: {msg})")
        if status == MFS_E_NONFINITE:
            raise MfsNonFinite(f"Failed to converge! ({what}: {msg})")
        cls = MfsTimeout if status == MFS_E_TIMEOUT else MfsError
        raise cls(f"{what or 'libmfs_hip'} failed with status {status}: {msg}")
    return status


def i64x(vals):
    return (C.c_int64 * len(vals))(*[int(v) for v in vals])


def f64x(vals):
    return (C.c_double * len(vals))(*[float(v) for v in vals])
