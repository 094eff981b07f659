"""Particle data evaluated at arbitrary points on the GPU (csrc/mfs_attrib.hip; DESIGN.md "Particle data at points"):
what the particles carry -- speed, velocity, a dye, an age -- at pixel hit points, mesh vertices and probes.

Particles x_i (P, 3) carry values a_i (P,) or (P, C), C in 1 .. 4, rounded to float32 on load; queries y_q (Q, 3).  With
d = x_i - y_q, t = 1 - |d|^2 / R^2 and the skin's weight w_qi = t^3 where t > 0, otherwise 0 (strict), W_q = sum_i w_qi and

    A_q = sum_i w_qi a_i / W_q        where W_q > 0,        `fill` (default NaN) in every channel where W_q == 0.

`gather(points, px, values, influence)` returns (values (Q, C) float32, weight (Q,) float32) in the caller's query order.
A particle whose position is not finite adds nothing; a non-finite value of a contributing particle propagates; a query
that is not finite, or outside the box, is uncovered.  Particles and queries are binned into cubic bins of edge R by a
stable sort, so the order of summation -- and with it every bit of the result -- is a function of the input alone.  No
atomics.  `bins(px, influence, box)` does the particles' half once for several gathers; nothing is cached otherwise.
tests/attrib_numpy.py restates the definition and derives the error bound.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Tuple

import numpy as np
import torch

from . import _lib
from . import tensors as T

INT32_MAX = 2 ** 31 - 1
MAX_BINS = 2 ** 31 - 2                  # keys are int32 and the sentinel is one more
MAX_CHANNELS = 4
CHUNK = 256                             # queries per work item: the kernel's workgroup


class Bins(NamedTuple):
    """The particles' half of a gather, held by the user: `particles` (P, 3) sorted by bin (a stable sort: the caller's
    order inside a bin), `order` (P,) int64 with particles = px[order], `starts` (bins + 1,) int32, the first sorted
    particle of every bin; the lattice: float64 `origin`, `shape` (m0, m1, m2), bin edge `influence`; `box` (lo, hi)."""
    particles: torch.Tensor
    order: torch.Tensor
    starts: torch.Tensor
    origin: Tuple[float, float, float]
    shape: Tuple[int, int, int]
    influence: float
    box: Tuple[Tuple[float, float, float], Tuple[float, float, float]]


def check_influence(influence):
    influence = float(influence)
    if not (math.isfinite(influence) and influence > 0):
        raise ValueError(f"influence must be positive and finite, got {influence}")
    return influence


def check_box(box):
    """(lo, hi) as two float64 triples, finite, lo <= hi"""
    try:
        lo, hi = box
        lo, hi = tuple(T.as_f64_list(lo, 3)), tuple(T.as_f64_list(hi, 3))
    except (TypeError, ValueError):
        raise ValueError(f"box: expected (lo, hi), two triples, got {box!r}") from None
    if not all(math.isfinite(v) for v in lo + hi) or any(b < a for a, b in zip(lo, hi)):
        raise ValueError(f"box: expected finite lo <= hi, got {lo}, {hi}")
    return lo, hi


def lattice(box, influence):
    """(origin, shape) of the bins that serve the queries of `box`: origin = lo - R, m_a = floor((hi_a - lo_a) / R) + 3,
    one ring of bins around the queries' own.  ValueError above 2^31 - 2 bins."""
    lo, hi = check_box(box)
    R = check_influence(influence)
    origin = tuple(a - R for a in lo)
    counts = [math.floor((b - a) / R) + 3 for a, b in zip(lo, hi)]
    total = counts[0] * counts[1] * counts[2]
    if total > MAX_BINS:
        raise ValueError(f"box {lo} .. {hi} at influence {R}: {total} bins exceed the limit of 2^31 - 2 = {MAX_BINS}; "
                         "use a tighter box or a larger influence")
    return origin, tuple(int(c) for c in counts)


def _positions(a, name, device=True):
    """(N, 3) float32 / float64, C-contiguous, fewer than 2^31 rows; then (device=True) on the GPU"""
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{name}: expected a torch tensor on the GPU, got {type(a).__name__}")
    if a.dim() != 2 or a.shape[1] != 3:
        raise ValueError(f"{name}: expected (N, 3), got {tuple(a.shape)}")
    if a.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name}: dtype {a.dtype} unsupported (float32 / float64)")
    if not a.is_contiguous():
        raise ValueError(f"{name}: tensor must be C-contiguous")
    if int(a.shape[0]) > INT32_MAX:
        raise ValueError(f"{name}: {int(a.shape[0])} rows exceed the limit of 2^31 - 1 = {INT32_MAX} (32-bit indices)")
    if device and not a.is_cuda:
        raise TypeError(f"{name}: tensor is on {a.device}; the gather runs on the GPU only (no CPU fallback)")
    return a


def _values(values, num_particles):
    """values as (P, C), after the checks that need no device"""
    if not isinstance(values, torch.Tensor):
        raise TypeError(f"values: expected a torch tensor on the GPU, got {type(values).__name__}")
    if values.dim() not in (1, 2) or int(values.shape[0]) != num_particles:
        raise ValueError(f"values: expected ({num_particles},) or ({num_particles}, C), got {tuple(values.shape)}")
    if values.dim() == 2 and not (1 <= int(values.shape[1]) <= MAX_CHANNELS):
        raise ValueError(f"values: {int(values.shape[1])} channels, expected 1 .. {MAX_CHANNELS}")
    if values.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"values: dtype {values.dtype} unsupported (float32 / float64)")
    return values.reshape(num_particles, int(values.shape[1]) if values.dim() == 2 else 1)


def _keys(lib, origin, shape, influence, box, pos):
    n, dev = int(pos.shape[0]), pos.device
    keys = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(lib.mfs_attrib_keys3d(_lib.i64x(shape), _lib.f64x(origin), influence,
                                     None if box is None else _lib.f64x(tuple(box[0]) + tuple(box[1])), T.ptr(pos),
                                     T.code(pos), n, T.ptr(keys), T.stream()), "mfs_attrib_keys3d")
    return keys


def bins(px, influence, box):
    """Bin the particles `px` (P, 3) for queries inside `box` = (lo, hi): a `Bins` to pass to `gather` in place of `px`.
    It holds what `px` held when it was built."""
    influence = check_influence(influence)
    origin, shape = lattice(box, influence)
    box = check_box(box)
    px = _positions(px, "px")
    dev, n = px.device, int(px.shape[0])
    lib = _lib.load()
    count = int(lib.mfs_attrib_bins3d(_lib.i64x(shape)))
    assert count == shape[0] * shape[1] * shape[2]
    with torch.cuda.device(dev):
        if n:
            keys, order = torch.sort(_keys(lib, origin, shape, influence, None, px), stable=True)   # inside a bin: the caller's order
            ps = px[order]
            starts = torch.searchsorted(keys, torch.arange(count + 1, dtype=torch.int32, device=dev), out_int32=True)
        else:
            ps, order = px, torch.zeros(0, dtype=torch.int64, device=dev)
            starts = torch.zeros(count + 1, dtype=torch.int32, device=dev)
    return Bins(ps, order, starts, origin, shape, influence, box)


def _work_items(qkeys, count):
    """(items (n, 3) int32: key, first, count; n) from the sorted query keys: every bin's queries in chunks of 256, in
    key order.  One host read: the number of items."""
    dev = qkeys.device
    qstarts = torch.searchsorted(qkeys, torch.arange(count + 1, dtype=torch.int32, device=dev)).to(torch.int64)
    per_bin = qstarts[1:] - qstarts[:-1]
    chunks = (per_bin + (CHUNK - 1)) // CHUNK
    ends = torch.cumsum(chunks, 0)
    n = int(ends[-1].item())
    if n == 0:
        return None, 0
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    key = torch.searchsorted(ends, idx, right=True)                  # the first bin whose chunks end beyond idx
    done = CHUNK * (idx - (ends[key] - chunks[key]))                 # queries of the bin in earlier chunks
    items = torch.stack([key, qstarts[key] + done, torch.clamp(per_bin[key] - done, max=CHUNK)], dim=1)
    return items.to(torch.int32).contiguous(), n


def gather(points, px, values, influence=None, box=None, fill=float("nan"), stats=None):
    """(values (Q, C) float32, weight (Q,) float32) of the particles' `values` ((P,) or (P, C), C in 1 .. 4) at `points`
    (Q, 3), in the order of `points`; Q = 0 and P = 0 are legal.  px: the particles (P, 3), or a `Bins` built from them
    (`influence` and `box` are then the Bins').  box: (lo, hi); None: the bounding box of the finite points (one
    reduction and one host read).  A point outside the box is uncovered.  stats: an optional dict that receives
    `work_items`, `pair_tests` (particles looped over x 256 lanes) and `bins`."""
    held = px if isinstance(px, Bins) else None
    if held is not None:
        if influence is not None and float(influence) != held.influence:
            raise ValueError(f"influence {influence} differs from the Bins' {held.influence}")
        if box is not None and check_box(box) != held.box:
            raise ValueError("box differs from the Bins'")
        influence, box, num_particles = held.influence, held.box, int(held.particles.shape[0])
    else:
        if influence is None:
            raise ValueError("influence: the radius is required with particles (a Bins carries its own)")
        influence = check_influence(influence)
        if box is not None:
            box = check_box(box)
            lattice(box, influence)
        px = _positions(px, "px", device=False)
        num_particles = int(px.shape[0])
    fill = float(fill)
    points = _positions(points, "points", device=False)
    vals = _values(values, num_particles)
    for name, a in (("points", points), ("values", vals)) + (() if held is not None else (("px", px),)):
        if not a.is_cuda:
            raise TypeError(f"{name}: tensor is on {a.device}; the gather runs on the GPU only (no CPU fallback)")
    dev = points.device
    particles = held.particles if held is not None else px
    if vals.device != dev or particles.device != dev:
        raise ValueError(f"points, particles and values must share one GPU, got {dev}, {particles.device}, {vals.device}")
    Q, C = int(points.shape[0]), int(vals.shape[1])
    lib = _lib.load()
    with torch.cuda.device(dev):
        out = torch.full((Q, C), fill, dtype=torch.float32, device=dev)
        weight = torch.zeros(Q, dtype=torch.float32, device=dev)
        if stats is not None:
            stats.update(work_items=0, pair_tests=0, bins=0)
        if Q == 0 or num_particles == 0:
            return out, weight
        if box is None:
            finite = torch.isfinite(points).all(dim=1, keepdim=True)
            ends = torch.stack([torch.where(finite, points, math.inf).amin(dim=0),
                                torch.where(finite, points, -math.inf).amax(dim=0)]).to(torch.float64).cpu().numpy()
            if not np.isfinite(ends).all():                              # no finite point
                return out, weight
            box = check_box((ends[0], ends[1]))
        B = held if held is not None else bins(px, influence, box)
        count = B.shape[0] * B.shape[1] * B.shape[2]
        qkeys, rows = torch.sort(_keys(lib, B.origin, B.shape, influence, box, points), stable=True)
        items, n = _work_items(qkeys, count)
        if n == 0:
            return out, weight
        qs, vs = points[rows], vals[B.order].contiguous()
        tested = torch.empty(n, dtype=torch.int32, device=dev) if stats is not None else None
        _lib.check(lib.mfs_attrib_gather3d(_lib.i64x(B.shape), _lib.f64x(B.origin), influence, C, fill, T.ptr(B.particles),
                                           T.code(B.particles), T.ptr(vs), T.code(vs), num_particles, T.ptr(B.starts),
                                           T.ptr(qs), T.code(qs), T.ptr(rows), Q, T.ptr(items), n, T.ptr(out), T.ptr(weight),
                                           None if tested is None else T.ptr(tested), T.stream()), "mfs_attrib_gather3d")
        if stats is not None:
            stats.update(work_items=n, pair_tests=int(tested.sum(dtype=torch.int64).item()) * CHUNK, bins=count)
    return out, weight


def at_vertices(mesh, px, values, influence, box=None, fill=float("nan")):
    """`gather` at `mesh.vertices` (an `mfs.surface.Mesh`)"""
    return gather(mesh.vertices, px, values, influence, box, fill)


def save_obj(path, mesh, colors):
    """plain-text Wavefront OBJ with a colour per vertex: `v x y z r g b` lines (colors (V, 3), in 0 .. 1; a NaN is
    written as 0), `vn` lines when the mesh has normals, 1-based `f` lines.  `mfs.surface.read_obj` reads the vertices'
    first three numbers."""
    v = mesh.vertices.detach().cpu().numpy()
    c = colors.detach().cpu().numpy() if isinstance(colors, torch.Tensor) else np.asarray(colors)
    if c.shape != v.shape:
        raise ValueError(f"colors: expected {v.shape}, one (r, g, b) per vertex, got {c.shape}")
    c = np.nan_to_num(c.astype(np.float64), nan=0.0)
    f = mesh.faces.detach().cpu().numpy().astype(np.int64) + 1
    n = None if mesh.normals is None else mesh.normals.detach().cpu().numpy()
    with open(path, "w") as fh:
        fh.write(f"# {len(v)} vertices with colours, {len(f)} faces\n")
        for x, k in zip(v, c):
            fh.write("v %.9g %.9g %.9g %.6g %.6g %.6g\n" % (tuple(float(t) for t in x) + tuple(float(t) for t in k)))
        if n is not None:
            for x in n:
                fh.write("vn %.9g %.9g %.9g\n" % tuple(float(t) for t in x))
            for a, b, d in f:
                fh.write(f"f {a}//{a} {b}//{b} {d}//{d}\n")
        else:
            for a, b, d in f:
                fh.write(f"f {a} {b} {d}\n")
