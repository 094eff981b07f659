"""Surface extraction on the GPU: `isosurface` (marching tetrahedra over the Kuhn cut of every lattice cube) and `contour`
(the same one dimension down) behind mfs_surface3d_* / mfs_contour2d_* of the C ABI (csrc/mfs_surface.hip).

The contract -- which node is inside, which lattice edge carries which vertex, in what order, how faces are oriented,
what `closed` means -- is stated in DESIGN.md "Surface extraction".  No atomics anywhere: two calls on the same field
return bitwise identical tensors.  Both calls run on the current stream and sync the host once, to read the two totals
the count pass leaves on the device.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from . import tensors as T

INT32_MAX = 2 ** 31 - 1
_TILE = 1024                      # nodes per block of csrc/mfs_surface.hip: the last tile's indices stay below 2^31


class Mesh(NamedTuple):
    """vertices (V,3) float32, faces (F,3) int32 (right-hand normal from inside to outside), normals (V,3) float32 or
    None -- all on the device of the field they came from."""
    vertices: torch.Tensor
    faces: torch.Tensor
    normals: Optional[torch.Tensor] = None

    def save_obj(self, path):
        """plain-text Wavefront OBJ from host copies: `v` lines, `vn` lines when normals are present, 1-based `f` lines"""
        v = self.vertices.detach().cpu().numpy()
        f = self.faces.detach().cpu().numpy().astype(np.int64) + 1
        n = None if self.normals is None else self.normals.detach().cpu().numpy()
        with open(path, "w") as fh:
            fh.write(f"# {len(v)} vertices, {len(f)} faces\n")
            for x in v:
                fh.write("v %.9g %.9g %.9g\n" % tuple(float(c) for c in x))
            if n is not None:
                for x in n:
                    fh.write("vn %.9g %.9g %.9g\n" % tuple(float(c) for c in x))
                for a, b, c in f:
                    fh.write(f"f {a}//{a} {b}//{b} {c}//{c}\n")
            else:
                for a, b, c in f:
                    fh.write(f"f {a} {b} {c}\n")


def read_obj(path):
    """Wavefront OBJ -> (vertices float32 (V,3), faces int32 (F,3)), on the host.  `v` and `f` records only; corners in
    the forms i, i/t, i//n, i/t/n, 1-based or negative (relative to the vertices read so far); polygons are
    fan-triangulated about their first corner (orientation kept); every other record and comments are ignored.
    ValueError with the line number on a malformed face or an index out of range."""
    verts, faces, lines = [], [], []
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            rec = line.split("#", 1)[0].split()
            if not rec:
                continue
            if rec[0] == "v":
                try:
                    verts.append([float(c) for c in rec[1:4]])
                    if len(verts[-1]) != 3:
                        raise ValueError
                except ValueError:
                    raise ValueError(f"{path}:{ln}: malformed vertex {line.strip()!r}") from None
            elif rec[0] == "f":
                if len(rec) < 4:
                    raise ValueError(f"{path}:{ln}: a face needs at least three corners, got {line.strip()!r}")
                idx = []
                for corner in rec[1:]:
                    try:
                        i = int(corner.split("/")[0])
                    except ValueError:
                        raise ValueError(f"{path}:{ln}: malformed face corner {corner!r}") from None
                    j = i - 1 if i > 0 else len(verts) + i          # negative: relative to the vertices read so far
                    if i == 0 or j < 0:
                        raise ValueError(f"{path}:{ln}: vertex index {i} out of range ({len(verts)} vertices so far)")
                    idx.append(j)
                faces.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
                lines.extend([ln] * (len(idx) - 2))
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    bad = np.nonzero((faces >= len(verts)).any(axis=1))[0]    # a positive index may point ahead: checked against the file
    if len(bad):
        raise ValueError(f"{path}:{lines[bad[0]]}: vertex index {int(faces[bad[0]].max()) + 1} out of range "
                         f"({len(verts)} vertices)")
    return np.asarray(verts, np.float32).reshape(-1, 3), faces.astype(np.int32)


def load_obj(path, device="cuda"):
    """`read_obj` as a `Mesh` of GPU tensors; normals is None"""
    v, f = read_obj(path)
    return Mesh(torch.as_tensor(v, device=device), torch.as_tensor(f, device=device), None)


class Contour(NamedTuple):
    """vertices (V,2) float32, segments (S,2) int32: the inside lies on the left of every segment (u, v)"""
    vertices: torch.Tensor
    segments: torch.Tensor


def check_sizes(shape, closed=False):
    """Node count of the (extended) lattice, after the checks that need no device: every extent >= 2, and the node count
    small enough that every node index of the last 1024-node tile fits int32 (the vertex total and 3 x the face total are
    checked after the count pass, before anything is filled)."""
    shape = tuple(int(v) for v in shape)
    if any(v < 2 for v in shape):
        raise ValueError(f"phi: every dimension must be >= 2, got {shape}")
    nodes = math.prod(v + (2 if closed else 0) for v in shape)
    if nodes > INT32_MAX - _TILE:
        raise ValueError(f"phi: {nodes} lattice nodes do not fit the 32-bit indices of the extraction kernels")
    return nodes


_workspaces = {}


def _workspace(kind, shape, closed, device, nbytes):
    """one workspace per (kind, shape, closed, device), kept: a simulation asks for the same surface every frame"""
    key = (kind, shape, bool(closed), device.index if device.index is not None else torch.cuda.current_device())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        with torch.cuda.device(device):
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _arguments(phi, dim, level, origin, spacing, closed, outside):
    phi = T.dev(phi, "phi")
    if phi.dim() != dim:
        raise ValueError(f"phi: expected a {dim}D array, got shape {tuple(phi.shape)}")
    shape = tuple(int(v) for v in phi.shape)
    level = float(level)
    if not math.isfinite(level):
        raise ValueError(f"level must be finite, got {level}")
    sp = T.as_f64_list(spacing, dim)
    if not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f"spacing must be positive, got {sp}")
    org = T.as_f64_list(origin, dim)
    if closed:
        if outside is None:
            raise ValueError("closed=True needs `outside`, the value of the virtual layer of samples")
        outside = float(outside)
        if not outside > level:
            raise ValueError(f"outside ({outside}) must be > level ({level})")
    else:
        outside = 0.0
    check_sizes(shape, closed)
    return phi, shape, level, org, sp, bool(closed), outside


def _extract(kind, phi, dim, level, origin, spacing, closed, outside, normals):
    phi, shape, level, org, sp, closed, outside = _arguments(phi, dim, level, origin, spacing, closed, outside)
    lib = _lib.load()
    ws_bytes, count, fill = (getattr(lib, f"mfs_{kind}_{part}") for part in ("workspace_bytes", "count", "fill"))
    g = _lib.i64x(shape)
    nbytes = int(ws_bytes(g, int(closed)))
    if nbytes == 0:
        raise ValueError(f"phi: shape {shape} is outside the range of mfs_{kind}")
    dev = phi.device
    ws = _workspace(kind, shape, closed, dev, nbytes)
    with torch.cuda.device(dev):
        common = (g, T.ptr(phi), T.code(phi), level, int(closed), outside)
        _lib.check(count(*common, T.ptr(ws), nbytes, T.stream()), f"mfs_{kind}_count")
        nv, nf = (int(v) for v in ws[:16].view(torch.int64).tolist())          # the one host sync
        if nv > INT32_MAX or nf * dim > INT32_MAX:
            raise ValueError(f"{nv} vertices / {nf} faces do not fit int32 indices")
        verts = torch.empty((nv, dim), dtype=torch.float32, device=dev)
        faces = torch.empty((nf, dim), dtype=torch.int32, device=dev)
        nrm = torch.empty((nv, dim), dtype=torch.float32, device=dev) if normals else None
        if nv:
            args = common + (_lib.f64x(org), _lib.f64x(sp), T.ptr(ws), nbytes, T.ptr(verts), nv, T.ptr(faces), nf)
            if dim == 3:
                args += (T.ptr(nrm) if normals else None,)
            _lib.check(fill(*args, T.stream()), f"mfs_{kind}_fill")
    return verts, faces, nrm


def isosurface(phi, level=0.0, origin=(0.0, 0.0, 0.0), spacing=1.0, closed=False, outside=None, normals=False):
    """Triangle mesh of {phi < level}.  phi: C-contiguous GPU tensor (n0,n1,n2), fp32 or fp64, every n >= 2; sample
    [i,j,k] sits at origin + (i,j,k) * spacing (scalar or triple, > 0).  closed=True surrounds the array with one virtual
    layer of samples of value `outside` (> level), so that the mesh of every inside region is watertight."""
    return Mesh(*_extract("surface3d", phi, 3, level, origin, spacing, closed, outside, normals))


def contour(phi, level=0.0, origin=(0.0, 0.0), spacing=1.0, closed=False, outside=None):
    """Line segments bounding {phi < level} of a 2D field; the rules of `isosurface` one dimension down."""
    v, s, _ = _extract("contour2d", phi, 2, level, origin, spacing, closed, outside, False)
    return Contour(v, s)


def simulation_surface(sim, which, dim, normals=False):
    """`surface()` of the two single-GPU simulation classes: the liquid level set lives at cell centres and its
    background value is 3 * GDX (notebook_kernels.compute_fluid_levelset); the solid one on the doubled node grid."""
    if which == "liquid":
        fl = sim.fluid_levelset
        cs = np.asarray(fl.cell_size, np.float64)
        org = np.asarray(fl.bound_min, np.float64) + 0.5 * cs
        args = dict(origin=org, spacing=cs, closed=True, outside=3.0 * sim.GDX)
        phi = fl.phi
    elif which == "solid":
        sl = sim.solid_levelset
        args = dict(origin=np.asarray(sl.bound_min, np.float64), spacing=np.asarray(sl.cell_size, np.float64))
        phi = sl.phi
    else:
        raise ValueError(f"which: 'liquid' or 'solid', got {which!r}")
    if dim == 3:
        return isosurface(phi, 0.0, normals=normals, **args)
    return contour(phi, 0.0, **args)
