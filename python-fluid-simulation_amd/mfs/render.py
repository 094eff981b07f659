"""Ray-marched images of the liquid and the solids on the GPU (csrc/mfs_render.hip; DESIGN.md "Rendering"): a node with
no display gets a frame of a run as an array of bytes, and `save_png` writes it with the standard library alone.

Everything visible is a sampled signed field under a rigid pose -- a `SkinField`, `solid_levelset.phi`, a `MeshBody`'s
`MeshSDF`: the shapes of `mfs.seed` (`Shape`, `as_shape`).  `Scene(shapes)` builds a grid of brick minima per shape;
`scene.render(camera)` walks every pixel's ray in float64 at a fixed step, stops at the first sample where the minimum
over the shapes is negative, refines it by one secant step and takes the hit shape's normal: a `RenderResult` of depth,
normal, shape id and step index.  `shade` turns that into Lambert bytes.  The bricks only save work: with skip=False the
marcher visits every sample of every shape and returns the same bits.  tests/render_numpy.py restates the contract.

`scene.trace(camera, look)` follows each ray further, under a `Look` of one `Material` per shape: an opaque surface is
shadowed by the opaque shapes between it and the light; a liquid refracts the ray in and out once, absorbs along the path
inside, and weighs what lies behind it by Fresnel's term; `look.samples`^2 rays per pixel.  It returns a `PathResult`
(float colour, step and shape id per slot of the path, length inside the liquid) and `resolve` turns that into bytes.
Opaque materials without shadows give `shade(render(...))` byte for byte.  tests/render_paths_numpy.py restates it.

    cam = render.Camera(eye=(0.9, 0.8, 1.1), target=(0, 0.3, 0), width=1920, height=1080)
    rgb = sim.render(cam)                                   # NotebookSimulation: the skin and the solid level set
    rgb = sim.render(cam, look="water")                     # the skin as water over shadowed solids, 2 x 2 rays per pixel
    render.save_png("frame.png", rgb)
"""
from __future__ import annotations

import ctypes
import math
import struct
import zlib
from typing import NamedTuple

import numpy as np
import torch

from . import _lib, seed as _seed, tensors as T, volumes as _volumes

MAX_SHAPES = 16                         # the shapes' descriptions travel by value in the launch
MAX_EXTENT = 16384                      # pixels per image axis
MAX_STEPS = 65536                       # samples per ray
TILE = 16                               # pixels per workgroup edge: four waves, each a tile of 8 x 8
BRICK = 8                               # cells per brick edge


def _unit(v):
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def check_sizes(width, height, num_steps=1):
    """(pixels, workgroups) of an image, after the checks that need no device"""
    width, height, num_steps = int(width), int(height), int(num_steps)
    if not (1 <= width <= MAX_EXTENT and 1 <= height <= MAX_EXTENT):
        raise ValueError(f"image {width} x {height}: width and height must be in 1 .. {MAX_EXTENT}")
    if not (1 <= num_steps <= MAX_STEPS):
        raise ValueError(f"{num_steps} samples per ray: expected 1 .. {MAX_STEPS}; use a larger step or a tighter near / far")
    return width * height, ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)


class Camera:
    """A pinhole (fov: the vertical field of view in degrees) or, with ortho_height (the image plane's height in world
    units), an orthographic camera at `eye` looking at `target`.  near / far: the marched interval of the ray parameter
    (distance along the ray); None: taken at each render from the shapes' posed boxes, one step wider, and reported in
    the result.  Row 0 of an image is its top."""

    def __init__(self, eye, target, up=(0.0, 1.0, 0.0), fov=40.0, ortho_height=None, width=640, height=480, near=None,
                 far=None):
        self.eye, self.target, self.up = (np.asarray(T.as_f64_list(v, 3), np.float64) for v in (eye, target, up))
        self.width, self.height = int(width), int(height)
        check_sizes(self.width, self.height)
        self.fov = float(fov)
        self.ortho_height = None if ortho_height is None else float(ortho_height)
        self.near = None if near is None else float(near)
        self.far = None if far is None else float(far)
        if not all(np.isfinite(v).all() for v in (self.eye, self.target, self.up)):
            raise ValueError("camera: eye, target and up must be finite")
        if self.ortho_height is None:
            if not (0.0 < self.fov < 180.0):
                raise ValueError(f"camera: fov must be in (0, 180) degrees, got {self.fov}")
        elif not (math.isfinite(self.ortho_height) and self.ortho_height > 0):
            raise ValueError(f"camera: ortho_height must be positive, got {self.ortho_height}")
        for name, v in (("near", self.near), ("far", self.far)):
            if v is not None and not math.isfinite(v):
                raise ValueError(f"camera: {name} must be finite, got {v}")
        if self.near is not None and self.far is not None and not self.far > self.near:
            raise ValueError(f"camera: far ({self.far}) must be > near ({self.near})")
        view = self.target - self.eye
        if not float(np.abs(view).max()) > 0:
            raise ValueError("camera: eye and target coincide")
        side = np.cross(_unit(view), self.up)
        if not float(np.sqrt((side * side).sum())) > 1e-12 * float(np.sqrt((self.up * self.up).sum())) > 0:
            raise ValueError("camera: up is zero or parallel to the view direction")
        b = self.basis()
        if not all(np.isfinite(b[k]).all() for k in ("f", "r", "u")) or not (math.isfinite(b["half_w"]) and b["half_w"] > 0
                                                                              and b["half_h"] > 0):
            raise ValueError("camera: degenerate frame")

    @property
    def ortho(self):
        return self.ortho_height is not None

    def basis(self):
        """dict(eye, f, r, u, half_w, half_h, ortho) in float64: f = normalize(target - eye), r = normalize(cross(f, up)),
        u = cross(r, f); half_h = tan(fov / 2) or ortho_height / 2, half_w = half_h * width / height.  These travel to the
        kernels by value."""
        f = _unit(self.target - self.eye)
        r = _unit(np.cross(f, self.up))
        u = np.cross(r, f)
        half_h = float(np.tan(np.deg2rad(np.float64(self.fov)) / 2.0)) if self.ortho_height is None else self.ortho_height / 2.0
        return dict(eye=self.eye.copy(), f=f, r=r, u=u, half_w=half_h * self.width / self.height, half_h=half_h,
                    ortho=self.ortho)

    def packed(self):
        b = self.basis()
        return [float(v) for k in ("eye", "f", "r", "u") for v in b[k]] + [b["half_w"], b["half_h"]]

    def range(self, shapes, step):
        """(near, far): the camera's own where given; otherwise from the corners of the shapes' posed boxes -- along the
        view axis for the near end (a ray's parameter is at least that), the distance from the eye for the far end
        (orthographic: the view axis for both) -- one step wider"""
        if self.near is not None and self.far is not None:
            return self.near, self.far
        b = self.basis()
        lo, hi = math.inf, -math.inf
        for s in shapes:
            n = np.asarray(s.volume.phi.shape, np.float64) - 1.0
            org, h = np.asarray(T.as_f64_list(s.volume.origin, 3)), float(s.volume.spacing)
            for c in np.ndindex(2, 2, 2):
                p = s.R @ (org + np.asarray(c, np.float64) * n * h) + s.T - b["eye"]
                along = float(p @ b["f"])
                lo = min(lo, along)
                hi = max(hi, along if self.ortho else float(np.sqrt(p @ p)))
        near = self.near if self.near is not None else (lo - step if self.ortho else max(lo - step, 0.0))
        far = self.far if self.far is not None else max(hi + step, near + step)
        return near, far


class RenderResult(NamedTuple):
    """depth (H, W) float64, the distance along the ray, +inf at a miss; normal (H, W, 3) float32, 0 at a miss; shape_id
    (H, W) int32, -1 at a miss; steps (H, W) int32, the index of the hit sample, -1 at a miss; near / far / step /
    num_steps: the march as it was run; num_shapes: of the scene."""
    depth: torch.Tensor
    normal: torch.Tensor
    shape_id: torch.Tensor
    steps: torch.Tensor
    near: float
    far: float
    step: float
    num_steps: int
    num_shapes: int


def _shapes(shapes, device=True):
    """a shape or a list of shapes -> a list of `mfs.seed.Shape`, after the checks that need no device, then (device=True)
    the device checks"""
    out = _seed._shape_list(shapes)
    if not (1 <= len(out) <= MAX_SHAPES):
        raise ValueError(f"{len(out)} shapes: a scene has 1 .. {MAX_SHAPES}")
    _volumes.check_shapes(out, [f"shape[{k}]" for k in range(len(out))])
    if device:
        _volumes.check_one_gpu(out, "rendering")
    return out


def plan(shapes, camera, step=None):
    """(near, far, step, num_steps) of a march of `shapes` (as `_shapes` returns them) seen by `camera`, after every
    refusal that needs no device: step defaults to half the smallest spacing, near / far to the camera's or the shapes'
    boxes, num_steps = ceil((far - near) / step) must be in 1 .. 65536"""
    if not isinstance(camera, Camera):
        raise TypeError(f"camera: expected an mfs.render.Camera, got {type(camera).__name__}")
    step = 0.5 * min(float(s.volume.spacing) for s in shapes) if step is None else float(step)
    if not (math.isfinite(step) and step > 0):
        raise ValueError(f"step must be positive, got {step}")
    near, far = camera.range(shapes, step)
    if not (math.isfinite(near) and math.isfinite(far) and far > near):
        raise ValueError(f"camera: marched interval [{near}, {far}] is empty or not finite")
    K = math.ceil((far - near) / step)
    check_sizes(camera.width, camera.height, K)
    return near, far, step, K


class Scene:
    """1 to 16 shapes (anything `mfs.seed.as_shape` accepts; float32 / float64 volumes on one GPU) and, per shape, the
    grid of brick minima the marcher skips by.  The grids are built here; call `refresh()` after a volume's contents
    changed (a volume replaced by another tensor needs a new Scene)."""

    def __init__(self, shapes):
        self.shapes = _shapes(shapes)
        self.device = self.shapes[0].volume.phi.device
        self.bricks = []
        self.bricks_max = [None] * len(self.shapes)      # brick maxima: of the shapes a `trace` has seen as a liquid
        self.refresh()

    def refresh(self):
        """rebuild every shape's brick minima (and the maxima that were built) from its volume as it is now"""
        lib = _lib.load()
        self.bricks = []
        built = [k for k, g in enumerate(self.bricks_max) if g is not None]
        self.bricks_max = [None] * len(self.shapes)
        for k in built:
            self._maxima(k)
        with torch.cuda.device(self.device):
            for s in self.shapes:
                phi = s.volume.phi
                e = _lib.i64x(phi.shape)
                grid = torch.empty(tuple((int(n) - 2) // BRICK + 1 for n in phi.shape), dtype=torch.float64, device=self.device)
                assert grid.numel() == int(lib.mfs_render_brick_count3d(e))
                _lib.check(lib.mfs_render_bricks3d(T.ptr(phi), T.code(phi), e, T.ptr(grid), T.stream()), "mfs_render_bricks3d")
                self.bricks.append(grid)
        return self

    def render(self, camera, step=None, skip=True, stats=None):
        """March every pixel of `camera` (module docstring).  step: the sample distance along the ray, default half the
        smallest spacing.  skip=False visits every sample of every shape: the same bits, more work.  stats: an optional
        dict that receives `pixels`, `hits`, `samples` (shape samples evaluated) and `num_steps` (one host sync)."""
        near, far, step, K = plan(self.shapes, camera, step)
        W, H = camera.width, camera.height
        lib = _lib.load()
        m, dev = len(self.shapes), self.device
        grids = (ctypes.c_void_p * m)(*[g.data_ptr() for g in self.bricks])
        with torch.cuda.device(dev):
            depth = torch.empty((H, W), dtype=torch.float64, device=dev)
            normal = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
            ident = torch.empty((H, W), dtype=torch.int32, device=dev)
            steps = torch.empty((H, W), dtype=torch.int32, device=dev)
            evals = torch.empty((H, W), dtype=torch.int32, device=dev) if stats is not None else None
            _lib.check(lib.mfs_render_march3d(_lib.f64x(camera.packed()), int(camera.ortho), W, H, near, step, K, m,
                                              *_volumes.pack_shapes(self.shapes), grids, int(bool(skip)), T.ptr(depth),
                                              T.ptr(normal), T.ptr(ident), T.ptr(steps),
                                              None if evals is None else T.ptr(evals), T.stream()),
                       "mfs_render_march3d")
            if stats is not None:
                stats.update(pixels=W * H, hits=int((steps >= 0).sum().item()),
                             samples=int(evals.sum(dtype=torch.int64).item()), num_steps=K)
        return RenderResult(depth, normal, ident, steps, near, far, step, K, m)

    def _maxima(self, k):
        """shape k's grid of brick maxima, built at its first use as a liquid and kept up by `refresh()`"""
        if self.bricks_max[k] is None:
            lib = _lib.load()
            phi = self.shapes[k].volume.phi
            with torch.cuda.device(self.device):
                grid = torch.empty(tuple((int(n) - 2) // BRICK + 1 for n in phi.shape), dtype=torch.float64, device=self.device)
                _lib.check(lib.mfs_render_bricks_max3d(T.ptr(phi), T.code(phi), _lib.i64x(phi.shape), T.ptr(grid), T.stream()),
                           "mfs_render_bricks_max3d")
            self.bricks_max[k] = grid
        return self.bricks_max[k]

    def trace(self, camera, look, step=None, skip=True, stats=None):
        """The path of every sub-pixel ray of `camera` under `look` (a `Look`): shadows, one refraction through a liquid,
        `look.samples`^2 rays per pixel -- a `PathResult`; `resolve` turns it into bytes.  step, skip, stats: as `render`
        (`hits` counts the rays whose first march hit).  tests/render_paths_numpy.py restates every operation."""
        near, far, step, K, bias, Ks, Ki = plan_paths(self.shapes, camera, look, step)
        s = look.samples
        W, H = s * camera.width, s * camera.height
        lib = _lib.load()
        m, dev = len(self.shapes), self.device
        grids = (ctypes.c_void_p * m)(*[g.data_ptr() for g in self.bricks])
        tops = (ctypes.c_void_p * m)(*[self._maxima(k).data_ptr() if mat.is_liquid else None
                                       for k, mat in enumerate(look.materials)])
        with torch.cuda.device(dev):
            color = torch.empty((H, W, 3), dtype=torch.float64, device=dev)
            steps = torch.empty((H, W, 4), dtype=torch.int32, device=dev)
            ident = torch.empty((H, W, 4), dtype=torch.int32, device=dev)
            length = torch.empty((H, W), dtype=torch.float64, device=dev)
            evals = torch.empty((H, W), dtype=torch.int32, device=dev) if stats is not None else None
            _lib.check(lib.mfs_render_paths3d(_lib.f64x(camera.packed()), int(camera.ortho), W, H, near, step, K, m,
                                              *_volumes.pack_shapes(self.shapes), grids, tops, int(bool(skip)),
                                              _lib.f64x(look.packed()), None if look.light is None else _lib.f64x(look.light),
                                              (ctypes.c_int * 3)(*look.background), int(look.shadows), bias, Ks, Ki,
                                              T.ptr(color), T.ptr(steps), T.ptr(ident), T.ptr(length),
                                              None if evals is None else T.ptr(evals), T.stream()),
                       "mfs_render_paths3d")
            if stats is not None:
                stats.update(pixels=W * H, hits=int((steps[..., 0] >= 0).sum().item()),
                             samples=int(evals.sum(dtype=torch.int64).item()), num_steps=K)
        return PathResult(color, steps, ident, length, near, far, step, K, m, s, bias, Ks, Ki)


class Material:
    """What a shape is made of: `Material.opaque(color)` or `Material.liquid(color, ior, absorb)`; color (r, g, b) in
    0 .. 255, ior in (1, 4], absorb (r, g, b) >= 0 per world unit (Beer-Lambert along the path inside the liquid)."""

    def __init__(self, color, ior=None, absorb=(0.0, 0.0, 0.0)):
        self.color = tuple(T.as_f64_list(color, 3))
        if not all(0.0 <= v <= 255.0 for v in self.color):
            raise ValueError(f"material: colour components must be in 0 .. 255, got {self.color}")
        self.ior = None if ior is None else float(ior)
        self.absorb = tuple(T.as_f64_list(absorb, 3))
        if self.ior is not None:
            if not (1.0 < self.ior <= 4.0):
                raise ValueError(f"material: ior must be in (1, 4], got {self.ior}")
            if not all(math.isfinite(v) and v >= 0.0 for v in self.absorb):
                raise ValueError(f"material: absorb must be finite and >= 0, got {self.absorb}")

    @classmethod
    def opaque(cls, color):
        return cls(color)

    @classmethod
    def liquid(cls, color, ior=1.33, absorb=(3.0, 1.2, 0.4)):
        return cls(color, ior, absorb)

    @property
    def is_liquid(self):
        return self.ior is not None

    def packed(self):
        return [float(self.is_liquid)] + [v / 255.0 for v in self.color] + [self.ior or 0.0] + list(self.absorb)


class Look:
    """How `Scene.trace` shades: one `Material` per shape; light: a vector towards a directional light, None: a headlight
    (l = -d of the camera's ray); background (r, g, b) in 0 .. 255; shadows: opaque shapes shadow the surface finally
    shaded (a liquid casts none); samples: s x s rays per pixel on the regular grid, 1 .. 4; bias: how far off a surface a
    secondary ray starts, default 4 steps; shadow_steps / inside_steps: samples of the shadow march and of the march
    inside the liquid, default the camera ray's.  Everything is checked here, without a device."""

    def __init__(self, materials, light, background=(255, 255, 255), shadows=True, samples=1, bias=None, shadow_steps=None,
                 inside_steps=None):
        self.materials = list(materials)
        if not (1 <= len(self.materials) <= MAX_SHAPES) or not all(isinstance(q, Material) for q in self.materials):
            raise ValueError(f"look: expected 1 .. {MAX_SHAPES} mfs.render.Material, one per shape")
        self.light = None
        if light is not None:
            light = np.asarray(T.as_f64_list(light, 3), np.float64)
            if not (np.isfinite(light).all() and float(np.abs(light).max()) > 0):
                raise ValueError("look: light must be a finite, non-zero vector towards the light")
            self.light = _unit(light)
        self.background = [int(v) for v in background]
        if len(self.background) != 3 or not all(0 <= v <= 255 for v in self.background):
            raise ValueError(f"look: background must be (r, g, b) in 0 .. 255, got {tuple(background)}")
        self.shadows = bool(shadows)
        self.samples = int(samples)
        if not (1 <= self.samples <= 4) or self.samples != samples:
            raise ValueError(f"look: samples must be an integer in 1 .. 4, got {samples}")
        self.bias = None if bias is None else float(bias)
        if self.bias is not None and not (math.isfinite(self.bias) and self.bias >= 0.0):
            raise ValueError(f"look: bias must be finite and >= 0, got {bias}")
        self.shadow_steps = None if shadow_steps is None else int(shadow_steps)
        self.inside_steps = None if inside_steps is None else int(inside_steps)
        for name, v in (("shadow_steps", self.shadow_steps), ("inside_steps", self.inside_steps)):
            if v is not None and not (1 <= v <= MAX_STEPS):
                raise ValueError(f"look: {name} must be in 1 .. {MAX_STEPS}, got {v}")

    def packed(self):
        return [v for q in self.materials for v in q.packed()]

    @classmethod
    def water(cls, count=2, liquid=0, **kw):
        """the default of `NotebookSimulation.render(look="water")`: shape `liquid` of `count` is water (ior 1.33, absorbing
        red most), the others an opaque warm grey; a light from above, shadows on, 2 x 2 rays per pixel"""
        mats = [Material.liquid(LIQUID_COLOR) if k == liquid else Material.opaque(SOLID_COLOR) for k in range(count)]
        return cls(mats, **{**dict(light=(0.3, 2.0, 0.4), samples=2), **kw})


class PathResult(NamedTuple):
    """color (sH, sW, 3) float64, the colour of every sub-pixel ray; steps and shape_id (sH, sW, 4) int32 per slot of the
    path (0 the camera's ray, 1 inside the liquid, 2 after the exit, 3 the shadow ray): the hit sample and shape, -1 at a
    miss, -2 where the slot was not run; length (sH, sW) float64, the path's length inside the liquid, 0 without one;
    near / far / step / num_steps / num_shapes as `RenderResult`; samples, bias, shadow_steps, inside_steps as run."""
    color: torch.Tensor
    steps: torch.Tensor
    shape_id: torch.Tensor
    length: torch.Tensor
    near: float
    far: float
    step: float
    num_steps: int
    num_shapes: int
    samples: int
    bias: float
    shadow_steps: int
    inside_steps: int


def plan_paths(shapes, camera, look, step=None):
    """(near, far, step, num_steps, bias, shadow_steps, inside_steps) of `Scene.trace`, after every refusal that needs no
    device: `plan`'s, one material per shape, the supersampled extents within 1 .. 16384"""
    near, far, step, K = plan(shapes, camera, step)
    if not isinstance(look, Look):
        raise TypeError(f"look: expected an mfs.render.Look, got {type(look).__name__}")
    if len(look.materials) != len(shapes):
        raise ValueError(f"look: {len(look.materials)} materials for {len(shapes)} shapes: expected one per shape")
    check_sizes(look.samples * camera.width, look.samples * camera.height, K)
    bias = 4.0 * step if look.bias is None else look.bias
    return near, far, step, K, bias, look.shadow_steps or K, look.inside_steps or K


def resolve(result):
    """(H, W, 3) uint8 on the result's device: the samples^2 colours of each pixel summed in row-major order, divided by
    samples^2, rounded floor(255 c + 0.5)"""
    if not isinstance(result, PathResult):
        raise TypeError(f"result: expected a PathResult, got {type(result).__name__}")
    if not result.color.is_cuda:
        raise TypeError(f"result is on {result.color.device}; resolving runs on the GPU only (no CPU fallback)")
    s = result.samples
    H, W = int(result.color.shape[0]) // s, int(result.color.shape[1]) // s
    lib = _lib.load()
    dev = result.color.device
    with torch.cuda.device(dev):
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.mfs_render_resolve3d(T.ptr(result.color), W, H, s, T.ptr(rgb), T.stream()), "mfs_render_resolve3d")
    return rgb


def image_paths(shapes, camera, look, step=None, skip=True):
    """`resolve(Scene(shapes).trace(camera, look, step, skip))`: (H, W, 3) uint8"""
    listed = _shapes(shapes, device=False)                                # everything a host can refuse, first
    plan_paths(listed, camera, look, step)
    return resolve(Scene(listed).trace(camera, look, step, skip))


def _palette(colors, count):
    if colors is None or len(colors) < count or len(colors) > MAX_SHAPES:
        raise ValueError(f"colors: expected one (r, g, b) in 0 .. 255 per shape ({count}), at most {MAX_SHAPES}")
    out = []
    for c in colors:
        c = T.as_f64_list(c, 3)
        if not all(0.0 <= v <= 255.0 for v in c):
            raise ValueError(f"colors: components must be in 0 .. 255, got {tuple(c)}")
        out += [v / 255.0 for v in c]
    return out


def hit_points(result, camera):
    """(H, W, 3) float64 on the result's device: origin + depth * direction of every pixel's ray, NaN at a miss.  The
    rays follow the camera's rule, operation by operation as tests/render_numpy.py's `rays` restates it."""
    if not isinstance(result, RenderResult):
        raise TypeError(f"result: expected a RenderResult, got {type(result).__name__}")
    if not isinstance(camera, Camera):
        raise TypeError(f"camera: expected an mfs.render.Camera, got {type(camera).__name__}")
    H, W = (int(v) for v in result.steps.shape)
    if (camera.width, camera.height) != (W, H):
        raise ValueError(f"camera is {camera.width} x {camera.height}, the result {W} x {H}")
    dev, b = result.depth.device, camera.basis()
    f, r, u, eye = (torch.as_tensor(b[k], dtype=torch.float64, device=dev) for k in ("f", "r", "u", "eye"))
    i = torch.arange(H, dtype=torch.float64, device=dev).reshape(H, 1, 1)
    j = torch.arange(W, dtype=torch.float64, device=dev).reshape(1, W, 1)
    sx = ((j + 0.5) * (2.0 / W) - 1.0) * b["half_w"]
    sy = (1.0 - (i + 0.5) * (2.0 / H)) * b["half_h"]
    if b["ortho"]:
        o, d = (eye + sx * r) + sy * u, f.expand(H, W, 3)
    else:
        v = (f + sx * r) + sy * u
        o, d = eye.expand(H, W, 3), v / torch.sqrt((v[..., 0] ** 2 + v[..., 1] ** 2) + v[..., 2] ** 2).unsqueeze(-1)
    hit = (result.steps >= 0).unsqueeze(-1)
    depth = torch.where(hit[..., 0], result.depth, 0.0).unsqueeze(-1)
    return torch.where(hit, o + depth * d, math.nan)


class Colormap:
    """Piecewise linear colours over stops (t, (r, g, b)), t ascending from 0 to 1, colours in 0 .. 255; or the name of a
    preset.  nan_color: the (r, g, b) a NaN value gets; None: a NaN value gives a NaN albedo, which the shading kernel
    answers with the palette's colour."""

    PRESETS = {
        "speed": [(0.0, (40, 120, 230)), (1.0, (255, 255, 255))],                     # the liquid's colour to white
        "heat": [(0.0, (0, 0, 0)), (0.4, (200, 30, 0)), (0.8, (255, 200, 0)), (1.0, (255, 255, 255))],
        "diverging": [(0.0, (40, 70, 200)), (0.5, (245, 245, 245)), (1.0, (200, 40, 40))],
    }

    def __init__(self, stops, nan_color=None):
        if isinstance(stops, str):
            if stops not in self.PRESETS:
                raise ValueError(f"colormap: expected one of {sorted(self.PRESETS)} or a list of stops, got {stops!r}")
            stops = self.PRESETS[stops]
        try:
            self.t = [float(s[0]) for s in stops]
            self.colors = [tuple(T.as_f64_list(s[1], 3)) for s in stops]
        except (TypeError, ValueError, IndexError):
            raise ValueError("colormap: expected stops (t, (r, g, b))") from None
        if len(self.t) < 2 or self.t[0] != 0.0 or self.t[-1] != 1.0 or any(b <= a for a, b in zip(self.t, self.t[1:])):
            raise ValueError(f"colormap: stops must ascend strictly from t = 0 to t = 1, got {self.t}")
        if not all(0.0 <= v <= 255.0 for c in self.colors for v in c):
            raise ValueError("colormap: colour components must be in 0 .. 255")
        self.nan_color = None if nan_color is None else tuple(T.as_f64_list(nan_color, 3))
        if self.nan_color is not None and not all(0.0 <= v <= 255.0 for v in self.nan_color):
            raise ValueError("colormap: nan_color components must be in 0 .. 255")

    def slope(self):
        """the largest |d albedo / d t| over the segments and channels"""
        return max(abs(b - a) / 255.0 / (tb - ta) for ta, tb, ca, cb in zip(self.t, self.t[1:], self.colors, self.colors[1:])
                   for a, b in zip(ca, cb))

    def apply(self, values, lo, hi):
        """float32 albedo in [0, 1], shape values.shape + (3,), on the values' device: t = clamp((v - lo) / (hi - lo), 0, 1)
        in float32, then in segment k (t_k <= t, the last one at t = 1) c = c_k + (c_{k+1} - c_k) * ((t - t_k) / (t_{k+1} -
        t_k)) with c = colour / 255 rounded to float32.  A NaN value gives NaN, or nan_color."""
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise ValueError(f"colour range: expected finite lo < hi, got ({lo}, {hi})")
        if not isinstance(values, torch.Tensor):
            raise TypeError(f"values: expected a torch tensor, got {type(values).__name__}")
        v = values.to(torch.float32)
        f32 = lambda a: torch.tensor(a, dtype=torch.float64).to(torch.float32).to(v.device)  # noqa: E731
        t = torch.clamp((v - f32(lo)) / (f32(hi) - f32(lo)), 0.0, 1.0)
        ts, cs = f32(self.t), f32(self.colors) / 255.0
        k = torch.clamp(torch.bucketize(t, ts, right=True) - 1, 0, len(self.t) - 2)      # a NaN lands in the last segment
        s = ((t - ts[k]) / (ts[k + 1] - ts[k])).unsqueeze(-1)
        c = cs[k] + (cs[k + 1] - cs[k]) * s
        if self.nan_color is not None:
            c = torch.where(torch.isnan(v).unsqueeze(-1), f32(self.nan_color) / 255.0, c)
        return c


def shade(result, camera, colors, background=(255, 255, 255), light=None, albedo=None, albedo_id=0):
    """(H, W, 3) uint8 on the result's device: albedo_id * (0.25 + 0.75 * max(0, n . l)), albedo = colour / 255, rounded
    floor(255 c + 0.5); l = -d, a headlight, or `light`, a vector towards the light; `background` at misses.
    albedo: None, or (H, W, 3) float32 in 0 .. 1 on the result's device: the pixels of shape `albedo_id` take it in
    place of that shape's colour, except where it is NaN."""
    if not isinstance(result, RenderResult):
        raise TypeError(f"result: expected a RenderResult, got {type(result).__name__}")
    if not isinstance(camera, Camera):
        raise TypeError(f"camera: expected an mfs.render.Camera, got {type(camera).__name__}")
    H, W = (int(v) for v in result.steps.shape)
    if (camera.width, camera.height) != (W, H):
        raise ValueError(f"camera is {camera.width} x {camera.height}, the result {W} x {H}")
    palette = _palette(colors, result.num_shapes)
    bg = [int(v) for v in background]
    if len(bg) != 3 or not all(0 <= v <= 255 for v in bg):
        raise ValueError(f"background: expected (r, g, b) in 0 .. 255, got {tuple(background)}")
    if light is not None:
        light = np.asarray(T.as_f64_list(light, 3), np.float64)
        if not (np.isfinite(light).all() and float(np.abs(light).max()) > 0):
            raise ValueError("light: expected a finite, non-zero vector towards the light")
        light = _unit(light)
    if albedo is not None:
        if not isinstance(albedo, torch.Tensor):
            raise TypeError(f"albedo: expected a torch tensor on the GPU, got {type(albedo).__name__}")
        if tuple(albedo.shape) != (H, W, 3) or albedo.dtype != torch.float32 or not albedo.is_contiguous():
            raise ValueError(f"albedo: expected a C-contiguous ({H}, {W}, 3) float32 tensor, got {tuple(albedo.shape)} "
                             f"{albedo.dtype}")
        if not (0 <= int(albedo_id) < result.num_shapes):
            raise ValueError(f"albedo_id {albedo_id}: the result has shapes 0 .. {result.num_shapes - 1}")
    if not result.normal.is_cuda:
        raise TypeError(f"result is on {result.normal.device}; shading runs on the GPU only (no CPU fallback)")
    lib = _lib.load()
    dev = result.normal.device
    if albedo is not None:
        if albedo.device != dev:
            raise TypeError(f"albedo is on {albedo.device}, the result on {dev}")
        with torch.cuda.device(dev):
            rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
            _lib.check(lib.mfs_render_shade_albedo3d(_lib.f64x(camera.packed()), int(camera.ortho), W, H,
                                                     T.ptr(result.normal), T.ptr(result.shape_id), len(palette) // 3,
                                                     _lib.f64x(palette), (ctypes.c_int * 3)(*bg),
                                                     None if light is None else _lib.f64x(light), T.ptr(albedo),
                                                     int(albedo_id), T.ptr(rgb), T.stream()),
                       "mfs_render_shade_albedo3d")
        return rgb
    with torch.cuda.device(dev):
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        _lib.check(lib.mfs_render_shade3d(_lib.f64x(camera.packed()), int(camera.ortho), W, H, T.ptr(result.normal),
                                          T.ptr(result.shape_id), len(palette) // 3, _lib.f64x(palette), (ctypes.c_int * 3)(*bg),
                                          None if light is None else _lib.f64x(light), T.ptr(rgb), T.stream()),
                   "mfs_render_shade3d")
    return rgb


def image(shapes, camera, colors, background=(255, 255, 255), light=None, step=None, skip=True):
    """`Scene(shapes).render(camera, step, skip)` shaded: (H, W, 3) uint8"""
    listed = _shapes(shapes, device=False)                                # everything a host can refuse, first
    plan(listed, camera, step)
    _palette(colors, len(listed))
    return shade(Scene(listed).render(camera, step, skip), camera, colors, background, light)


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def save_png(path, rgb):
    """write (H, W, 3) uint8 (a tensor on any device, or an array) as an 8-bit RGB PNG; standard library only"""
    a = rgb.detach().cpu().numpy() if isinstance(rgb, torch.Tensor) else np.asarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"rgb: expected (H, W, 3) uint8, got {a.shape} {a.dtype}")
    H, W = a.shape[:2]
    rows = np.concatenate([np.zeros((H, 1), np.uint8), np.ascontiguousarray(a).reshape(H, 3 * W)], axis=1)   # filter 0
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
                + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))


# ------------------------------------------------------------------------------------------- NotebookSimulation ----
class _Volume(NamedTuple):
    phi: torch.Tensor
    origin: tuple
    spacing: float


LIQUID_COLOR, SOLID_COLOR = (40, 120, 230), (190, 185, 175)


def simulation_shapes(sim, what=("liquid", "solid")):
    """the shapes of `NotebookSimulation.render`: "liquid" = skin_field(clip=True), "solid" = solid_levelset.phi as a bare
    volume (origin bound_min, spacing GDX / 2: the analytic and the mesh bodies united), in the order of `what`"""
    what = (what,) if isinstance(what, str) else tuple(what)
    if not what or any(w not in ("liquid", "solid") for w in what) or len(set(what)) != len(what):
        raise ValueError(f'what: expected "liquid", "solid" or both, got {what!r}')
    out = []
    for w in what:
        if w == "liquid":
            out.append(sim.skin_field(clip=True))
        else:
            sl = sim.solid_levelset
            out.append(_Volume(sl.phi, tuple(float(v) for v in np.asarray(sl.bound_min, np.float64)), 0.5 * sim.GDX))
    return what, out


def simulation_result(sim, camera, what=("liquid", "solid"), step=None):
    return Scene(simulation_shapes(sim, what)[1]).render(camera, step)


def simulation_image(sim, camera, what=("liquid", "solid"), colors=None, step=None):
    names, shapes = simulation_shapes(sim, what)
    if colors is None:
        colors = [LIQUID_COLOR if w == "liquid" else SOLID_COLOR for w in names]
    return image(shapes, camera, colors, step=step)


def simulation_look(what, look):
    """`look` of `NotebookSimulation.render` as a `Look` for the shapes named by `what`: "water" -> `Look.water` with the
    skin as the liquid"""
    names = (what,) if isinstance(what, str) else tuple(what)
    if isinstance(look, str):
        if look != "water":
            raise ValueError(f'look: expected an mfs.render.Look or "water", got {look!r}')
        return Look.water(len(names), names.index("liquid") if "liquid" in names else -1)
    if not isinstance(look, Look):
        raise TypeError(f'look: expected an mfs.render.Look or "water", got {type(look).__name__}')
    return look


def simulation_paths(sim, camera, what, look, step=None, trace=False):
    """the image of `NotebookSimulation.render(look=...)`; trace=True: (the `PathResult`, the `Look`) instead"""
    look = simulation_look(what, look)
    shapes = simulation_shapes(sim, what)[1]
    if trace:
        return Scene(shapes).trace(camera, look, step), look
    return image_paths(shapes, camera, look, step)


def simulation_box(sim):
    """the simulation's bounds as a gather's box: float64(BOUND_MIN) .. + float64(BOUND_SIZE)"""
    lo = np.asarray(sim.BOUND_MIN, np.float64)
    return tuple(float(v) for v in lo), tuple(float(v) for v in lo + np.asarray(sim.BOUND_SIZE, np.float64))


def simulation_values(sim, values):
    """`values` of `sample_particles` / `color_by` as a tensor: "speed" = |particle.v|, "velocity" = particle.v"""
    if isinstance(values, str):
        if values == "speed":
            return torch.linalg.vector_norm(sim.particle.v, dim=1)
        if values == "velocity":
            return sim.particle.v
        raise ValueError(f'values: expected "velocity", "speed" or a tensor, got {values!r}')
    return values


def simulation_colored(sim, camera, what, colors, step, color_by, color_range, colormap):
    """the image of `NotebookSimulation.render(color_by=...)`: the liquid's pixels take the particles' data, gathered at
    their hit points with the rendered skin's influence over the simulation's bounds, as their albedo"""
    from . import attrib as _attrib
    names = (what,) if isinstance(what, str) else tuple(what)
    if "liquid" not in names:
        raise ValueError(f'color_by colours the liquid: "liquid" must be in what, got {what!r}')
    if isinstance(color_by, str) and color_by != "speed":
        raise ValueError(f'color_by: expected "speed", a (P,) or a (P, 3) tensor, got {color_by!r}')
    cmap = colormap if isinstance(colormap, Colormap) else Colormap(colormap)
    if color_range is not None:
        lo, hi = (float(v) for v in color_range)
        if not (math.isfinite(lo) and math.isfinite(hi) and hi > lo):
            raise ValueError(f"color_range: expected finite (lo, hi), lo < hi, got {tuple(color_range)}")
    n = int(sim.particle.x.shape[0])
    data = simulation_values(sim, color_by)
    if not isinstance(data, torch.Tensor) or tuple(data.shape) not in ((n,), (n, 3)):
        raise ValueError(f'color_by: expected "speed", a ({n},) or a ({n}, 3) tensor, got '
                         f"{tuple(data.shape) if isinstance(data, torch.Tensor) else type(data).__name__}")
    names, shapes = simulation_shapes(sim, what)
    if colors is None:
        colors = [LIQUID_COLOR if w == "liquid" else SOLID_COLOR for w in names]
    _palette(colors, len(shapes))
    liquid = names.index("liquid")
    result = Scene(shapes).render(camera, step)
    H, W = camera.height, camera.width
    points = torch.where((result.shape_id == liquid).unsqueeze(-1), hit_points(result, camera), math.nan)
    got, _ = _attrib.gather(points.reshape(-1, 3), sim.particle.x, data, shapes[liquid].influence, simulation_box(sim))
    if data.dim() == 2:
        albedo = torch.clamp(got, 0.0, 1.0).reshape(H, W, 3)              # a dye: the albedo itself (clamp keeps a NaN)
    else:
        if color_range is None:
            lo, hi = 0.0, float(data.max().item()) if n else 0.0
            if not (math.isfinite(hi) and hi > lo):
                hi = 1.0
        albedo = cmap.apply(got.reshape(H, W), lo, hi)
    return shade(result, camera, colors, albedo=albedo.contiguous(), albedo_id=liquid)


def simulation_sample(sim, points, values="velocity"):
    """`NotebookSimulation.sample_particles`: (values (Q, C), weight (Q,)) of the particles' data at `points`, gathered
    with the skin's default influence over the simulation's bounds"""
    from . import attrib as _attrib, skin as _skin
    influence = 3.0 * _skin.default_radius(0.5 * sim.GDX)
    return _attrib.gather(points, sim.particle.x, simulation_values(sim, values), influence, simulation_box(sim))
