"""Lists of level-set volumes on their way to the C ABI (csrc/mfs_volume.h): the checks of `mfs.seed` and `mfs.render`, and
the packing into host arrays they share with `solver.sdf3D`.  A shape is an `mfs.seed.Shape`: .volume (.phi / .origin /
.spacing), .R (3, 3) and .T (3,) in float64."""
import ctypes
import math

import numpy as np
import torch

from . import _lib, tensors as T


def check_shapes(shapes, names):
    """everything about a list of shapes that can be refused without a device; names[k]: what to call shape k"""
    for s, name in zip(shapes, names):
        phi = s.volume.phi
        if not isinstance(phi, torch.Tensor):
            raise TypeError(f"{name}.phi: expected a torch tensor on the GPU, got {type(phi).__name__}")
        if phi.dim() != 3 or min(phi.shape) < 2 or phi.numel() > 2 ** 31 - 1:
            raise ValueError(f"{name}.phi: expected a volume (n0, n1, n2), every extent >= 2, fewer than 2^31 nodes, got "
                             f"{tuple(phi.shape)}")
        if phi.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{name}.phi: dtype {phi.dtype} unsupported (float32 / float64)")
        if not phi.is_contiguous():
            raise ValueError(f"{name}.phi: tensor must be C-contiguous")
        h = float(s.volume.spacing)
        if not (math.isfinite(h) and h > 0):
            raise ValueError(f"{name}.spacing must be positive, got {h}")
        if not (all(math.isfinite(v) for v in T.as_f64_list(s.volume.origin, 3)) and np.isfinite(s.T).all()
                and np.isfinite(s.R).all()):
            raise ValueError(f"{name}: origin and pose must be finite")


def check_one_gpu(shapes, activity):
    """every volume on the GPU, and on the same one; activity: "seeding", "rendering" """
    for k, s in enumerate(shapes):
        phi = s.volume.phi
        if not phi.is_cuda:
            raise TypeError(f"shape {k}: volume is on {phi.device}; {activity} runs on the GPU only (no CPU fallback)")
        if phi.device != shapes[0].volume.phi.device:
            raise ValueError(f"shape {k}: volume is on {phi.device}, shape 0 on {shapes[0].volume.phi.device}; all volumes "
                             "must be on one device")


def pack(volumes, dtypes=True, poses=None):
    """The host arrays of m volumes, given as (phi, origin, spacing), in the order of the C entry points: volumes_host,
    dtypes_host (dtypes=True), extents_host, origins_host, spacings_host and, with poses = [(R, T), ...], poses_host.
    m = 0 gives arrays of one unused element."""
    m = len(volumes)
    ptrs = (ctypes.c_void_p * max(m, 1))()
    codes, ext, org, sp = [], [], [], []
    for i, (phi, origin, spacing) in enumerate(volumes):
        ptrs[i] = phi.data_ptr()
        codes.append(T.code(phi))
        ext += [int(v) for v in phi.shape]
        org += T.as_f64_list(origin, 3)
        sp.append(float(spacing))
    out = [ptrs] + ([(ctypes.c_int * max(m, 1))(*codes)] if dtypes else [])
    out += [_lib.i64x(ext or [0]), _lib.f64x(org or [0.0]), _lib.f64x(sp or [0.0])]
    return out if poses is None else out + [_lib.f64x([v for R, Tr in poses for v in (*np.reshape(R, -1), *Tr)] or [0.0])]


def pack_shapes(shapes):
    """`pack` of a list of shapes, dtypes and poses included: the six arrays of mfs_seed_count3d / mfs_render_march3d"""
    return pack([(s.volume.phi, s.volume.origin, s.volume.spacing) for s in shapes], poses=[(s.R, s.T) for s in shapes])
