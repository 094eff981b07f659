"""The liquid's skin on the GPU (csrc/mfs_skin.hip; DESIGN.md "Liquid skin"): Zhu & Bridson's surface of a particle
cloud, sampled on a lattice at particle spacing -- `field(px, shape, origin, spacing)` -> `SkinField`, and `mesh(...)`,
the same followed by `mfs.surface.isosurface`.  The solver's own `fluid_levelset.phi` (a union of spheres at cell
centres) is what the pressure solve needs and stays as it is; this is what one looks at.

With d_i = x_i - x, w_i = max(1 - |d_i|^2 / R^2, 0)^3 and W = sum w_i a node x gets phi = |sum w_i d_i| / W - r, and
the background R - r where no particle is within R.  The kernel gathers per brick of 4 x 8 x 8 nodes from particles
binned by brick; the binning is a stable sort, so the order of summation -- and with it every bit of the field -- is a
function of the input alone.  No atomics.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib
from . import surface as _surface
from . import tensors as T

INT32_MAX = 2 ** 31 - 1
REACH = 4                               # influence <= REACH * spacing: the shortest edge of the kernel's brick


class SkinField(NamedTuple):
    """phi (n0,n1,n2) float32 on the particles' device, negative inside; node (0,0,0) sits at `origin` (float64 triple),
    neighbours `spacing` apart; `background`: the value (float32, as a float) of every node no particle reaches."""
    phi: torch.Tensor
    origin: Tuple[float, float, float]
    spacing: float
    radius: float
    influence: float
    background: float


def default_radius(spacing):
    """the reference's level-set radius rule, 1.02 * sqrt(3) / 2 * (cell size), at the skin's spacing"""
    return 1.02 * (math.sqrt(3.0) / 2.0) * float(spacing)


def check_sizes(shape, num_particles=0):
    """node count, after the checks that need no device: three extents >= 2, and node and particle counts below 2^31
    (32-bit indices in the kernels)"""
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or any(v < 2 for v in shape):
        raise ValueError(f"shape: expected three extents >= 2, got {shape}")
    nodes = math.prod(shape)
    if nodes > INT32_MAX:
        raise ValueError(f"skin lattice {shape}: {nodes} nodes do not fit the 32-bit indices of the skin kernels; "
                         "use a larger spacing")
    if int(num_particles) > INT32_MAX:
        raise ValueError(f"{int(num_particles)} particles do not fit the 32-bit indices of the skin kernels")
    return nodes


def _arguments(px, shape, origin, spacing, radius, influence):
    """everything that can be refused without a device, then the device check"""
    spacing = float(spacing)
    if not (math.isfinite(spacing) and spacing > 0):
        raise ValueError(f"spacing must be positive, got {spacing}")
    radius = default_radius(spacing) if radius is None else float(radius)
    if not (math.isfinite(radius) and radius > 0):
        raise ValueError(f"radius must be positive, got {radius}")
    influence = 3.0 * radius if influence is None else float(influence)
    if not (math.isfinite(influence) and influence > radius):
        raise ValueError(f"influence ({influence}) must be > radius ({radius})")
    if influence > REACH * spacing:
        raise ValueError(f"influence ({influence}) must not exceed {REACH} * spacing = {REACH * spacing}: a brick of nodes "
                         "gathers from one ring of neighbour bricks")
    org = tuple(T.as_f64_list(origin, 3))
    if not all(math.isfinite(v) for v in org):
        raise ValueError(f"origin must be finite, got {org}")
    if not isinstance(px, torch.Tensor):
        raise TypeError(f"px: expected a torch tensor on the GPU, got {type(px).__name__}")
    if px.dim() != 2 or px.shape[1] != 3:
        raise ValueError(f"px: expected (P, 3), got {tuple(px.shape)}")
    if px.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"px: dtype {px.dtype} unsupported (float32 / float64)")
    if not px.is_contiguous():
        raise ValueError("px: tensor must be C-contiguous")
    shape = tuple(int(v) for v in shape)
    check_sizes(shape, px.shape[0])
    if not px.is_cuda:
        raise TypeError(f"px: tensor is on {px.device}; the skin runs on the GPU only (no CPU fallback)")
    return px, shape, org, spacing, radius, influence


def field(px, shape, origin, spacing, radius=None, influence=None, stats=None):
    """px: (P,3) float32 / float64 GPU tensor, P >= 0, anywhere (particles farther than `influence` from every node are
    dropped at the binning).  radius: default 1.02 * sqrt(3)/2 * spacing; influence: default 3 * radius, at most
    4 * spacing.  stats: an optional dict that receives `bricks`, `bricks_entered` and `pair_tests` (survivors x 256)."""
    px, shape, org, spacing, radius, influence = _arguments(px, shape, origin, spacing, radius, influence)
    dev, n = px.device, int(px.shape[0])
    lib = _lib.load()
    g, o = _lib.i64x(shape), _lib.f64x(org)
    bins = int(lib.mfs_skin_bins3d(g))
    with torch.cuda.device(dev):
        phi = torch.empty(shape, dtype=torch.float32, device=dev)
        if n:
            keys = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(lib.mfs_skin_keys3d(g, o, spacing, T.ptr(px), T.code(px), n, T.ptr(keys), T.stream()), "mfs_skin_keys3d")
            keys, order = torch.sort(keys, stable=True)                    # inside a bin: the caller's order
            ps = px[order]
            starts = torch.searchsorted(keys, torch.arange(bins + 1, dtype=torch.int32, device=dev), out_int32=True)
        else:
            ps, starts = px, torch.zeros(bins + 1, dtype=torch.int32, device=dev)
        surv = None
        if stats is not None:
            surv = torch.empty(int(lib.mfs_skin_bricks3d(g)), dtype=torch.int32, device=dev)
        _lib.check(lib.mfs_skin_field3d(g, o, spacing, radius, influence, T.ptr(ps), T.code(ps), n, T.ptr(starts), T.ptr(phi),
                                        None if surv is None else T.ptr(surv), T.stream()), "mfs_skin_field3d")
        if surv is not None:
            stats["bricks"] = surv.numel()
            stats["bricks_entered"] = int((surv > 0).sum().item())
            stats["pair_tests"] = int(surv.sum(dtype=torch.int64).item()) * 256
    return SkinField(phi, org, spacing, radius, influence, float(np.float32(influence - radius)))


def extract(f, phi=None, normals=False):
    """the closed isosurface {phi < 0} of a `SkinField` (of `phi`, a field on the same lattice, when given)"""
    return _surface.isosurface(f.phi if phi is None else phi, 0.0, f.origin, f.spacing, closed=True, outside=f.background,
                               normals=normals)


def mesh(px, shape, origin, spacing, radius=None, influence=None, normals=False):
    """`field` followed by `mfs.surface.isosurface(phi, 0, origin, spacing, closed=True, outside=background)`"""
    return extract(field(px, shape, origin, spacing, radius, influence), normals=normals)


def simulation_skin_field(sim, clip=True, radius=None, influence=None):
    """`skin_field()` of NotebookSimulation: the skin of `sim.particle.x` on the solid level set's own lattice (origin
    bound_min, spacing GDX / 2, 2 * GRES + 1 nodes).  clip: max(phi, -solid phi), which trims the rind, `radius` thick,
    that particles projected onto a solid leave inside it."""
    sl = sim.solid_levelset
    f = field(sim.particle.x, sl.resolution, np.asarray(sl.bound_min, np.float64), 0.5 * sim.GDX, radius, influence)
    if clip:
        f = f._replace(phi=torch.maximum(f.phi, -sl.phi))
    return f
