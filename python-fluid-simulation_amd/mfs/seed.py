"""Liquid seeded from level-set volumes on the GPU (csrc/mfs_seed.hip; DESIGN.md "Seeding liquid from shapes"):
`fill(include, shape, origin, spacing, exclude=...)` walks a lattice of particle sites, keeps the sites inside the include
shapes and clear of the exclude shapes, and returns their jittered positions -- the `px` of `NotebookSimulation`.

A shape is a sampled signed distance (`mfs.meshsdf.MeshSDF`, `mfs.skin.SkinField`, or anything with .phi / .origin /
.spacing) under a rigid pose; its value at x is the volume sampled trilinearly at R^T (x - T), the rule of the mesh solids.
Site (i, j, k), with the index s = (i * n1 + j) * n2 + k, puts its particle at origin + ((idx + 0.5) + jitter * u) * spacing,
u in [-0.5, 0.5) a hash of (seed, s, axis); it is kept iff min over includes < 0 and min over excludes > clearance.  The
kernels count per workgroup, the counts are scanned, and a second pass stores the survivors in ascending s: no atomics,
no array of candidates, and two calls return the same bits.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, tensors as T, volumes as _volumes

MAX_SHAPES = 16                         # the shapes' descriptions travel by value in the launch
MAX_EXTENT = 2 ** 30                    # per axis of the site lattice
MAX_BLOCKS = 2 ** 31 - 1                # workgroups of one launch
BLOCK = 256                             # sites per workgroup


class Shape:
    """A volume under a rigid pose: `volume` has .phi (float32 / float64 (n0, n1, n2) GPU tensor, every extent >= 2,
    negative inside), .origin (position of node (0,0,0) in the volume's own frame) and .spacing; center / axis / angle
    (degrees) as `solver.sdf3D.MeshBody` and `generate_rb`.  The default pose is the identity."""

    def __init__(self, volume, center=(0, 0, 0), axis=(0, 1, 0), angle=0):
        from solver import sdf3D
        self.volume = volume
        self.T = np.asarray(T.as_f64_list(center, 3), np.float64)
        self.R = np.ascontiguousarray(sdf3D.get_R(list(T.as_f64_list(axis, 3)), float(angle))[:3, :3], dtype=np.float64)


def as_shape(s):
    """a `Shape` as it is; a `solver.sdf3D.MeshBody` (anything with .sdf and .row) by its volume and its row's pose; a bare
    volume under the identity pose"""
    if isinstance(s, Shape):
        return s
    if hasattr(s, "sdf") and hasattr(s, "row"):
        row = np.asarray(s.row, np.float64).reshape(10, 4)
        out = Shape.__new__(Shape)
        out.volume, out.T, out.R = s.sdf, row[1:4, 3].copy(), np.ascontiguousarray(row[5:8, :3])
        return out
    if all(hasattr(s, a) for a in ("phi", "origin", "spacing")):
        out = Shape.__new__(Shape)
        out.volume, out.T, out.R = s, np.zeros(3), np.eye(3)
        return out
    raise TypeError(f"expected a Shape, a MeshBody or a volume with .phi / .origin / .spacing, got {type(s).__name__}")


def _shape_list(s):
    """a shape or a list of shapes -> a list of `Shape` (a MeshSDF / SkinField is a tuple, and one shape)"""
    if s is None:
        return []
    if isinstance(s, (list, tuple)) and not all(hasattr(s, a) for a in ("phi", "origin", "spacing")):
        return [as_shape(v) for v in s]
    return [as_shape(s)]


def check_sizes(shape):
    """(sites, workgroups) of a site lattice, after the checks that need no device"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or any(v < 1 or v > MAX_EXTENT for v in shape):
        raise ValueError(f"shape: expected three extents in 1 .. 2^30 = {MAX_EXTENT}, got {shape}")
    sites = math.prod(shape)
    blocks = (sites + BLOCK - 1) // BLOCK
    if blocks > MAX_BLOCKS:
        raise ValueError(f"site lattice {shape}: {blocks} workgroups of {BLOCK} sites are more than the {MAX_BLOCKS} of one "
                         "launch; fill it in parts")
    return sites, blocks


def _arguments(include, shape, origin, spacing, exclude, clearance, jitter, seed, dtype):
    """everything that can be refused without a device, then the device checks"""
    shape = tuple(int(v) for v in shape)
    check_sizes(shape)
    spacing, clearance, jitter = float(spacing), float(clearance), float(jitter)
    if not (math.isfinite(spacing) and spacing > 0):
        raise ValueError(f"spacing must be positive, got {spacing}")
    org = tuple(T.as_f64_list(origin, 3))
    if not all(math.isfinite(v) for v in org):
        raise ValueError(f"origin must be finite, got {org}")
    if not (0.0 <= jitter <= 1.0):
        raise ValueError(f"jitter must be in [0, 1], got {jitter}")
    if math.isnan(clearance):
        raise ValueError("clearance is NaN")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not (0 <= int(seed) < 2 ** 64):
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype {dtype} unsupported (float32 / float64)")
    inc, exc = _shape_list(include), _shape_list(exclude)
    if not inc:
        raise ValueError("include: at least 1 shape")
    if len(inc) + len(exc) > MAX_SHAPES:
        raise ValueError(f"{len(inc)} include + {len(exc)} exclude shapes: at most {MAX_SHAPES} per call")
    shapes = inc + exc
    _volumes.check_shapes(shapes, [f"include[{k}]" for k in range(len(inc))] + [f"exclude[{k}]" for k in range(len(exc))])
    _volumes.check_one_gpu(shapes, "seeding")
    return shapes, len(inc), len(exc), shape, org, spacing, clearance, jitter, int(seed)


def _count(lib, a, masks_wanted):
    """launch the count pass; returns (counts int32, masks or None, the lattice's ctypes triple)"""
    shapes, n_inc, n_exc, shape, org, spacing, clearance, jitter, seed = a
    dev = shapes[0].volume.phi.device
    g, o = _lib.i64x(shape), _lib.f64x(org)
    blocks = int(lib.mfs_seed_blocks3d(g))
    counts = torch.empty(blocks, dtype=torch.int32, device=dev)
    masks = torch.empty((blocks, 4), dtype=torch.int64, device=dev) if masks_wanted else None
    _lib.check(lib.mfs_seed_count3d(g, o, spacing, jitter, seed, n_inc, n_exc, *_volumes.pack_shapes(shapes), clearance,
                                    T.ptr(counts), None if masks is None else T.ptr(masks), T.stream()), "mfs_seed_count3d")
    return counts, masks, (g, o)


def count(include, shape, origin, spacing, exclude=(), clearance=0.0, jitter=1.0, seed=0, dtype=torch.float64,
          return_sites=False, stats=None):
    """the number of particles `fill` would return for the same arguments, without the fill pass"""
    a = _arguments(include, shape, origin, spacing, exclude, clearance, jitter, seed, dtype)
    lib = _lib.load()
    with torch.cuda.device(a[0][0].volume.phi.device):
        counts, _, _ = _count(lib, a, False)
        kept = int(counts.sum(dtype=torch.int64).item())
    if stats is not None:
        stats.update(sites=math.prod(a[3]), blocks=counts.numel(), kept=kept)
    return kept


def fill(include, shape, origin, spacing, exclude=(), clearance=0.0, jitter=1.0, seed=0, dtype=torch.float64,
         return_sites=False, stats=None):
    """include / exclude: a shape or a list of shapes (`Shape`, `solver.sdf3D.MeshBody`, or a bare volume), at least one
    include and at most 16 in all, volumes on one GPU.  shape: the three extents of the site lattice; origin: its corner
    (float64 triple); spacing: the site size.  A site is kept iff min over includes < 0 and min over excludes > clearance.
    jitter in [0, 1]: the share of its site cell a particle may move in; seed: an integer in [0, 2^64).
    Returns px (P, 3) of `dtype` (float32: the float64 position rounded once), P >= 0, in ascending site index; with
    return_sites=True also those indices (P,) int64.  stats: an optional dict that receives `sites`, `blocks`, `kept`.
    One host synchronisation: the read of P."""
    a = _arguments(include, shape, origin, spacing, exclude, clearance, jitter, seed, dtype)
    shapes, _, _, shape, _, spacing, _, jitter, seed = a
    dev = shapes[0].volume.phi.device
    lib = _lib.load()
    with torch.cuda.device(dev):
        counts, masks, (g, o) = _count(lib, a, True)
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        offsets = ends - counts
        kept = int(ends[-1].item())                                        # the one host sync: sizes the output
        px = torch.empty((kept, 3), dtype=dtype, device=dev)
        sites = torch.empty(kept, dtype=torch.int64, device=dev) if return_sites else None
        if kept:
            _lib.check(lib.mfs_seed_fill3d(g, o, spacing, jitter, seed, T.ptr(masks), T.ptr(offsets), T.ptr(px), T.code(px),
                                           None if sites is None else T.ptr(sites), kept, T.stream()), "mfs_seed_fill3d")
    if stats is not None:
        stats.update(sites=math.prod(shape), blocks=counts.numel(), kept=kept)
    return (px, sites) if return_sites else px
