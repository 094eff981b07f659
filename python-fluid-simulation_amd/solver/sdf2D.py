"""Drop-in for the reference's solver/sdf2D.py on MI355X: the 2D rigid-body scene description (`generate_rb`,
`transform_rb`, `set_vel_rb`, `get_T`, `get_R` -- host side, same packed (n, 8, 3) float64 layout) and the two kernels:
`evaluate` (signed distance + body velocity at a set of points: builds `sphi` / `sv`) and `project` (push particles out
of / into the bodies, every step).  PyTorch-ROCm tensors, HIP kernels behind the C ABI; no CPU path.
"""
import numpy as np
import torch

from mfs import _lib, tensors as T


def get_T(position):
    """3x3 translation matrix (reference :207-210), float64 numpy."""
    t = np.identity(3)
    t[0:2, 2] = np.asarray(T.as_f64_list(position, 2))
    return t


def get_R(axis, angle):
    """3x3 rotation matrix by `angle` degrees (reference :212-218; `axis` is accepted and unused in 2D), float64 numpy."""
    r = np.identity(3)
    if angle:
        rad = angle * np.pi / 180
        c, s = np.cos(rad), np.sin(rad)
        r[:2, :2] = np.asarray(((c, -s), (s, c)))
    return r


def _empty(device):
    return torch.zeros((0, 8, 3), dtype=torch.float64, device=device)


def generate_rb(rb_d, rb_map, name, rbparam, flip=False, center=[0, 0], axis=[0, 1], angle=0, device=None):
    """Append one body (reference :221-252).  rbparam: ['sphere', radius] | ['box', sx, sy].  Row 0 = [type code (+1 if
    flipped), parameters], rows 1-3 translation, rows 4-6 rotation, row 7 velocity.  `rb_d` may be None / empty for the
    first body.  Returns (rb_d, rb_map) -- and, like the reference, the bare `rb_d` for an unknown shape name."""
    if rb_d is None:
        rb_d = _empty(torch.device("cuda" if device is None else device))
    rb = np.zeros((1, 8, 3))
    if rbparam[0] == 'sphere':
        rb[:, 0, 0] = 1 if flip else 0
        rb[:, 0, 1] = rbparam[1]
    elif rbparam[0] == 'box':
        rb[:, 0, 0] = 3 if flip else 2
        rb[:, 0, 1:] = np.asarray(rbparam[1:], dtype=np.float64)
    else:
        return rb_d
    rb[:, 1:4, :] = get_T(center)
    rb[:, 4:7, :] = get_R(axis, angle)
    index = rb_d.shape[0]
    rb_map[name] = index
    rbt = torch.as_tensor(rb, dtype=torch.float64, device=rb_d.device)
    rb_d = rbt if index == 0 else torch.cat([rb_d, rbt], dim=0)
    return rb_d, rb_map


def transform_rb(rb_d, index, center=None, axis=None, angle=None):
    """reference :254-258"""
    if center:
        rb_d[index, 1:4, :] = torch.as_tensor(get_T(center), dtype=rb_d.dtype, device=rb_d.device)
    if axis and angle:
        rb_d[index, 4:7, :] = torch.as_tensor(get_R(axis, angle), dtype=rb_d.dtype, device=rb_d.device)


def set_vel_rb(rb_d, index, vel):
    """reference :260-261"""
    rb_d[index, -1, :2] = torch.as_tensor(np.asarray(T.as_f64_list(vel, 2)), dtype=rb_d.dtype, device=rb_d.device)


def _bodies(rb_d):
    rb_d = T.dev(rb_d, "rb_d")
    if rb_d.dim() != 3 or tuple(rb_d.shape[1:]) != (8, 3) or rb_d.dtype != torch.float64:
        raise ValueError("rb_d: expected a float64 tensor of shape (n, 8, 3)")
    return rb_d


def evaluate(rb_d, sd, vel, position):
    """sd[...] = min over bodies of the signed distance at position[..., :]; vel[..., :] = velocity of the closest body
    where sd <= 0, else 0 (reference :185-196 -> kernel :146-169).  Any leading shape, last dimension 2."""
    rb_d = _bodies(rb_d)
    position, sd, vel = T.dev(position, "position"), T.dev(sd, "sd"), T.dev(vel, "vel")
    assert tuple(sd.shape) == tuple(position.shape[:-1])
    assert position.shape[-1] == 2
    assert vel.shape[-1] == 2
    if vel.numel() != 2 * sd.numel():
        raise ValueError(f"vel: shape {tuple(vel.shape)} does not hold one velocity per position")
    vel *= 0
    n = int(sd.numel())
    lib = _lib.load()
    _lib.check(lib.mfs_sdf_evaluate2d(T.ptr(rb_d), int(rb_d.shape[0]), T.ptr(position), T.code(position), n, T.ptr(sd),
                                      T.code(sd), T.ptr(vel), T.code(vel), T.stream()), "mfs_sdf_evaluate2d")


def evaluate_grid(rb_d, sd, vel, bound_min, cell_size, bias, rb_w=None):
    """`evaluate` on the nodes of a regular grid, for bodies that move (no reference counterpart): sd has the grid's shape,
    vel that shape + (2,); the position of index i along an axis is `grid_positions`' bound_min(f32) + (f32 i + f32 bias)
    * cell_size, made in the kernel, and every element of vel is written -- no position array, no zeroing pass.
    rb_w: float64 (n,) angular velocities in rad/s; the winning body's velocity is then v + w x (pos - centre)."""
    rb_d = _bodies(rb_d)
    sd, vel = T.dev(sd, "sd"), T.dev(vel, "vel")
    if sd.dim() != 2 or tuple(vel.shape) != tuple(sd.shape) + (2,):
        raise ValueError(f"sd / vel: expected shapes (n0, ..) and (n0, .., 2) on a 2D grid, got {tuple(sd.shape)}, {tuple(vel.shape)}")
    n = int(rb_d.shape[0])
    if rb_w is not None:
        rb_w = T.dev(rb_w, "rb_w", (n,))
        if rb_w.dtype != torch.float64:
            raise TypeError("rb_w: expected float64")
    lib = _lib.load()
    f = lambda a: _lib.f64x(T.as_f64_list(a, 2))  # noqa: E731
    _lib.check(lib.mfs_sdf_evaluate_grid2d(T.ptr(rb_d), n, None if rb_w is None or n == 0 else T.ptr(rb_w),
                                           _lib.i64x(tuple(int(v) for v in sd.shape)), f(bound_min), f(bias), f(cell_size),
                                           T.ptr(sd), T.code(sd), T.ptr(vel), T.code(vel), T.stream()),
               "mfs_sdf_evaluate_grid2d")


def project(rb_d, position):
    """In place: every body in turn moves the points it owns to its surface / into itself
    (reference :198-205 -> kernel :171-183)."""
    rb_d = _bodies(rb_d)
    position = T.dev(position, "position")
    assert position.shape[-1] == 2
    lib = _lib.load()
    _lib.check(lib.mfs_sdf_project2d(T.ptr(rb_d), int(rb_d.shape[0]), T.ptr(position), T.code(position),
                                     int(position.numel() // 2), T.stream()), "mfs_sdf_project2d")
