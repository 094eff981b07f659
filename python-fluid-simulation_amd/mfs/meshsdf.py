"""Signed distance volume of a closed triangle mesh on the GPU (csrc/mfs_meshsdf.hip; DESIGN.md "Triangle-mesh solids"):
`build(mesh, spacing)` -> `MeshSDF`, the one-time step that turns a user's geometry (`mfs.surface.load_obj`, or the mesh
`sim.surface()` wrote) into what `solver.sdf3D.MeshBody` poses in a scene.

Distance: exact, the minimum over all triangles in fp32, culled per brick of nodes without changing a bit (`cull=False`
runs the same kernel with the skip disabled).  Sign: parity of ray crossings along array axis 0 with half-open
tie-breaks; a mesh that is not closed is refused, not guessed at.  No atomics: two builds are bitwise identical.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib
from . import tensors as T

INT32_MAX = 2 ** 31 - 1


class MeshSDF(NamedTuple):
    """phi (n0,n1,n2) float32 on the GPU, negative inside; node (0,0,0) sits at `origin` (float64 triple) in the mesh's own
    frame, neighbours `spacing` apart; radius: the largest vertex distance from that frame's origin."""
    phi: torch.Tensor
    origin: Tuple[float, float, float]
    spacing: float
    radius: float


def lattice(vertices, spacing, padding):
    """(shape, origin) of the bounding box of `vertices` (host array) grown by `padding` nodes on every side: the fewest
    cells that cover the box, centred on it"""
    lo, hi = vertices.min(axis=0).astype(np.float64), vertices.max(axis=0).astype(np.float64)
    cells = np.maximum(np.ceil((hi - lo) / spacing - 1e-9), 1).astype(np.int64)
    shape = tuple(int(c) + 1 + 2 * padding for c in cells)
    origin = tuple(float(v) for v in (lo + hi) / 2 - (cells / 2 + padding) * spacing)
    return shape, origin


def check_sizes(shape):
    """node count, after the check that needs no device: it must stay below 2^31 (32-bit node indices in the kernels)"""
    nodes = math.prod(int(v) for v in shape)
    if nodes > INT32_MAX:
        raise ValueError(f"mesh lattice {tuple(shape)}: {nodes} nodes do not fit the 32-bit indices of the mesh kernels; "
                         "use a larger spacing")
    return nodes


def build(mesh, spacing, padding=3, cull=True, stats=None):
    """mesh: `mfs.surface.Mesh` (or any object with .vertices (V,3) float and .faces (F,3) int, GPU tensors) of a CLOSED
    surface with the solid inside.  stats: an optional dict that receives `surviving_fraction`, the share of
    (brick, triangle) pairs that reached the distance kernel's inner loop."""
    verts = T.dev(mesh.vertices, "mesh.vertices")
    faces = mesh.faces
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.shape[0] < 3:
        raise ValueError(f"mesh.vertices: expected (V >= 3, 3), got {tuple(verts.shape)}")
    if not isinstance(faces, torch.Tensor) or faces.device != verts.device or faces.dim() != 2 or faces.shape[1] != 3 \
            or faces.shape[0] < 1 or faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("mesh.faces: expected an int32 / int64 tensor (F >= 1, 3) on the vertices' device")
    spacing, padding = float(spacing), int(padding)
    if not (math.isfinite(spacing) and spacing > 0) or padding < 1:
        raise ValueError(f"spacing must be positive and padding >= 1, got {spacing}, {padding}")
    verts = verts.to(torch.float32)
    vh = verts.detach().cpu().numpy()
    if not np.isfinite(vh).all():
        raise ValueError("mesh.vertices: not finite")
    fl = faces.to(torch.int64)
    if int(fl.min()) < 0 or int(fl.max()) >= verts.shape[0]:
        raise ValueError("mesh.faces: vertex index out of range")
    if fl.shape[0] > INT32_MAX // 9:
        raise ValueError(f"mesh.faces: {fl.shape[0]} triangles are more than the mesh kernels index")
    shape, origin = lattice(vh, spacing, padding)
    check_sizes(shape)                                                     # before any launch
    dev = verts.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        tri = verts[fl.reshape(-1)].reshape(-1, 9).contiguous()
        phi = torch.empty(shape, dtype=torch.float32, device=dev)
        odd = torch.empty(shape[1:], dtype=torch.int32, device=dev)
        g, org = _lib.i64x(shape), _lib.f64x(origin)
        surv = None
        if stats is not None:
            surv = torch.empty(int(lib.mfs_meshsdf_bricks3d(g)), dtype=torch.int32, device=dev)
        _lib.check(lib.mfs_meshsdf_distance3d(g, org, spacing, T.ptr(tri), int(tri.shape[0]), int(bool(cull)), T.ptr(phi),
                                              None if surv is None else T.ptr(surv), T.stream()), "mfs_meshsdf_distance3d")
        _lib.check(lib.mfs_meshsdf_sign3d(g, org, spacing, T.ptr(tri), int(tri.shape[0]), T.ptr(phi), T.ptr(odd),
                                          T.stream()), "mfs_meshsdf_sign3d")
        n_odd = int(odd.sum().item())                                      # counted on the device; the one host sync
        if surv is not None:
            stats["surviving_fraction"] = float(surv.sum(dtype=torch.int64).item()) / (surv.numel() * tri.shape[0])
    if n_odd:
        raise ValueError(f"mesh is not closed: {n_odd} of {odd.numel()} lattice columns cross the surface an odd number "
                         "of times; no sign is guessed")
    return MeshSDF(phi, origin, spacing, float(np.sqrt((vh.astype(np.float64) ** 2).sum(axis=1).max())))
