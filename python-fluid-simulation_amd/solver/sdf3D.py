"""Drop-in for the reference's solver/sdf3D.py on MI355X: rigid-body scene
description (`generate_rb`, `transform_rb`, `set_vel_rb`, `get_T`, `get_R` -- host side, same packed
(n, 10, 4) float64 layout) and the two kernels the notebook calls: `evaluate` (signed distance +
body velocity at a set of points; ipynb scene set-up) and `project` (push particles out of / into
the bodies; ipynb:4584, every step).  PyTorch-ROCm tensors, HIP kernels behind the C ABI; no CPU path.
"""

import numpy as np
import torch
from scipy.spatial.transform import Rotation as R

from mfs import _lib, tensors as T, volumes as _volumes


def get_T(position):
    """4x4 translation matrix (reference :264-267), float64 numpy."""
    t = np.identity(4)
    t[0:3, 3] = np.asarray(T.as_f64_list(position, 3))
    return t


def get_R(axis, angle):
    """4x4 rotation matrix about `axis` by `angle` degrees (reference :269-274), float64 numpy."""
    r = np.identity(4)
    if angle:
        ax = np.asarray(T.as_f64_list(axis, 3))
        r[:3, :3] = R.from_rotvec(ax / np.linalg.norm(ax) * angle * np.pi / 180).as_matrix()
    return r


def _empty(device):
    return torch.zeros((0, 10, 4), dtype=torch.float64, device=device)


def generate_rb(rb_d, rb_map, name, rbparam, flip=False, center=[0, 0, 0], axis=[0, 1, 0], angle=0, device=None):
    """Append one body (reference :277-305).  rbparam: ['sphere', radius] | ['box', sx, sy, sz] |
    ['cylinder', radius, height].  Row 0 = [type code (+1 if flipped), parameters], rows 1-4 translation,
    rows 5-8 rotation, row 9 velocity.  `rb_d` may be None / empty for the first body.  Returns (rb_d, rb_map)."""
    if rb_d is None:
        rb_d = _empty(torch.device("cuda" if device is None else device))
    rb = np.zeros((1, 10, 4))
    if rbparam[0] == 'sphere':
        rb[:, 0, 0] = 1 if flip else 0
        rb[:, 0, 1] = rbparam[1]
    elif rbparam[0] == 'box':
        rb[:, 0, 0] = 3 if flip else 2
        rb[:, 0, 1:] = np.asarray(rbparam[1:], dtype=np.float64)
    elif rbparam[0] == 'cylinder':
        rb[:, 0, 0] = 5 if flip else 4
        rb[:, 0, 1:3] = np.asarray(rbparam[1:], dtype=np.float64)
    else:
        return rb_d
    rb[:, 1:5, :] = get_T(center)
    rb[:, 5:9, :] = get_R(axis, angle)
    index = rb_d.shape[0]
    rb_map[name] = index
    rbt = torch.as_tensor(rb, dtype=torch.float64, device=rb_d.device)
    rb_d = rbt if index == 0 else torch.cat([rb_d, rbt], dim=0)
    return rb_d, rb_map


def transform_rb(rb_d, index, center=None, axis=None, angle=None):
    """reference :307-311"""
    if center:
        rb_d[index, 1:5, :] = torch.as_tensor(get_T(center), dtype=rb_d.dtype, device=rb_d.device)
    if axis and angle:
        rb_d[index, 5:9, :] = torch.as_tensor(get_R(axis, angle), dtype=rb_d.dtype, device=rb_d.device)


def set_vel_rb(rb_d, index, vel):
    """reference :313-314"""
    rb_d[index, -1, :3] = torch.as_tensor(np.asarray(T.as_f64_list(vel, 3)), dtype=rb_d.dtype, device=rb_d.device)


def _bodies(rb_d):
    rb_d = T.dev(rb_d, "rb_d")
    if rb_d.dim() != 3 or tuple(rb_d.shape[1:]) != (10, 4) or rb_d.dtype != torch.float64:
        raise ValueError("rb_d: expected a float64 tensor of shape (n, 10, 4)")
    return rb_d


def evaluate(rb_d, sd, vel, position):
    """sd[...] = min over bodies of the signed distance at position[..., :]; vel[..., :] = velocity of the
    closest body where sd <= 0, else 0 (reference :260-270 -> kernel :218-239)."""
    rb_d = _bodies(rb_d)
    position, sd, vel = T.dev(position, "position"), T.dev(sd, "sd"), T.dev(vel, "vel")
    assert tuple(sd.shape) == tuple(position.shape[:-1])
    assert position.shape[-1] == 3
    assert vel.shape[-1] == 3
    vel *= 0
    n = int(sd.numel())
    lib = _lib.load()
    _lib.check(lib.mfs_sdf_evaluate3d(T.ptr(rb_d), int(rb_d.shape[0]), T.ptr(position), T.code(position), n, T.ptr(sd),
                                      T.code(sd), T.ptr(vel), T.code(vel), T.stream()), "mfs_sdf_evaluate3d")


def evaluate_grid(rb_d, sd, vel, bound_min, cell_size, bias, rb_w=None):
    """`evaluate` on the nodes of a regular grid, for bodies that move (no reference counterpart): sd has the grid's shape,
    vel that shape + (3,); the position of index i along an axis is `grid_positions`' bound_min(f32) + (f32 i + f32 bias)
    * cell_size, made in the kernel, and every element of vel is written -- no position array, no zeroing pass.
    rb_w: float64 (n, 3) angular velocities in rad/s; the winning body's velocity is then v + w x (pos - centre)."""
    rb_d = _bodies(rb_d)
    sd, vel = T.dev(sd, "sd"), T.dev(vel, "vel")
    if sd.dim() != 3 or tuple(vel.shape) != tuple(sd.shape) + (3,):
        raise ValueError(f"sd / vel: expected shapes (n0, ..) and (n0, .., 3) on a 3D grid, got {tuple(sd.shape)}, {tuple(vel.shape)}")
    n = int(rb_d.shape[0])
    if rb_w is not None:
        rb_w = T.dev(rb_w, "rb_w", (n, 3))
        if rb_w.dtype != torch.float64:
            raise TypeError("rb_w: expected float64")
    lib = _lib.load()
    f = lambda a: _lib.f64x(T.as_f64_list(a, 3))  # noqa: E731
    _lib.check(lib.mfs_sdf_evaluate_grid3d(T.ptr(rb_d), n, None if rb_w is None or n == 0 else T.ptr(rb_w),
                                           _lib.i64x(tuple(int(v) for v in sd.shape)), f(bound_min), f(bias), f(cell_size),
                                           T.ptr(sd), T.code(sd), T.ptr(vel), T.code(vel), T.stream()),
               "mfs_sdf_evaluate_grid3d")


def project(rb_d, position):
    """In place: every body in turn moves the points it owns to its surface / into itself
    (reference :272-278 -> kernel :241-258)."""
    rb_d = _bodies(rb_d)
    position = T.dev(position, "position")
    assert position.shape[-1] == 3
    lib = _lib.load()
    _lib.check(lib.mfs_sdf_project3d(T.ptr(rb_d), int(rb_d.shape[0]), T.ptr(position), T.code(position),
                                     int(position.numel() // 3), T.stream()), "mfs_sdf_project3d")


# ------------------------------------------------------------------ triangle-mesh bodies (no reference counterpart) ----
MESH_TYPE_CODE = 6        # row 0 of a mesh body; unknown to evaluate / evaluate_grid / project, which leave such rows alone
MAX_MESH_BODIES = 16      # the volumes' descriptions travel by value in the launch (csrc/mfs_meshsdf.hip)


class MeshBody:
    """A closed triangle mesh as a solid: `sdf` is its `mfs.meshsdf.MeshSDF` (built once), the pose one row of the packed
    (1, 10, 4) layout -- row 0 = [6, sdf.radius, 0, 0], rows 1-4 translation, rows 5-8 rotation (`axis`, `angle` in
    degrees, as generate_rb), row 9 velocity -- so that `mfs.motion.BodyKinematics` moves it like any other body.
    motion: an optional `mfs.motion.Motion`, read by `NotebookSimulation(..., mesh_bodies=[...])`."""

    def __init__(self, sdf, center=(0, 0, 0), axis=(0, 1, 0), angle=0, velocity=(0, 0, 0), motion=None):
        phi = T.dev(sdf.phi, "sdf.phi")
        if phi.dim() != 3 or phi.dtype != torch.float32 or min(phi.shape) < 2:
            raise ValueError("sdf.phi: expected a float32 volume (n0, n1, n2), every extent >= 2")
        self.sdf, self.motion = sdf, motion
        row = np.zeros((1, 10, 4))
        row[0, 0, 0], row[0, 0, 1] = MESH_TYPE_CODE, float(sdf.radius)
        row[0, 1:5, :] = get_T(center)
        row[0, 5:9, :] = get_R(list(axis), angle)
        row[0, 9, :3] = np.asarray(T.as_f64_list(velocity, 3))
        self.row = row


def mesh_rb(bodies, device=None):
    """the (m, 10, 4) float64 table of the mesh bodies' rows, on the device of their volumes"""
    bodies = list(bodies)
    if not bodies:
        raise ValueError("mesh bodies: an empty list")
    dev = torch.device(device) if device is not None else bodies[0].sdf.phi.device
    return torch.as_tensor(np.concatenate([b.row for b in bodies], axis=0), dtype=torch.float64, device=dev)


def _mesh_volumes(rb, bodies):
    rb = _bodies(rb)
    bodies = list(bodies)
    m = len(bodies)
    if m > MAX_MESH_BODIES:
        raise ValueError(f"{m} mesh bodies: at most {MAX_MESH_BODIES} per call")
    if int(rb.shape[0]) != m:
        raise ValueError(f"mesh_rb has {int(rb.shape[0])} rows for {m} mesh bodies")
    vols = []
    for b in bodies:
        phi = T.dev(b.sdf.phi, "sdf.phi")
        if phi.dtype != torch.float32 or phi.dim() != 3 or phi.device != rb.device:
            raise ValueError("mesh body volume: expected a float32 (n0, n1, n2) tensor on mesh_rb's device")
        vols.append((phi, b.sdf.origin, b.sdf.spacing))
    return rb, m, _volumes.pack(vols, dtypes=False)                      # no poses either: the kernels read mesh_rb


def union_mesh_grid(mesh_rb, bodies, sd, vel, bound_min, cell_size, bias, rb_w=None):
    """Unite the mesh bodies with the level set `sd` / `vel` already holds on a regular grid (`evaluate_grid`'s grid and
    position rule): for every node and every body in turn, d = the body's volume sampled trilinearly at R^T (x - T) (outside
    the volume: the sample at the clamped point plus the distance to the volume's box); d < sd -> sd = d and
    vel = v + w x (x - T) where d <= 0, 0 where d > 0.  Analytic and mesh bodies compose by `evaluate_grid`, then this."""
    rb, m, vol_args = _mesh_volumes(mesh_rb, bodies)
    sd, vel = T.dev(sd, "sd"), T.dev(vel, "vel")
    if sd.dim() != 3 or tuple(vel.shape) != tuple(sd.shape) + (3,):
        raise ValueError(f"sd / vel: expected shapes (n0, ..) and (n0, .., 3) on a 3D grid, got {tuple(sd.shape)}, {tuple(vel.shape)}")
    if rb_w is not None:
        rb_w = T.dev(rb_w, "rb_w", (m, 3))
        if rb_w.dtype != torch.float64:
            raise TypeError("rb_w: expected float64")
    lib = _lib.load()
    f = lambda a: _lib.f64x(T.as_f64_list(a, 3))  # noqa: E731
    _lib.check(lib.mfs_mesh_union_grid3d(T.ptr(rb), None if rb_w is None else T.ptr(rb_w), m, *vol_args,
                                         _lib.i64x(tuple(int(v) for v in sd.shape)), f(bound_min), f(bias), f(cell_size),
                                         T.ptr(sd), T.code(sd), T.ptr(vel), T.code(vel), T.stream()),
               "mfs_mesh_union_grid3d")


def project_mesh(mesh_rb, bodies, position):
    """`project` for mesh bodies, in place: for every body in turn a particle whose sampled d < 0 moves by -d * n, n the
    normalised gradient of the trilinear interpolant rotated to the world frame (central differences of samples one
    spacing apart where it vanishes; still zero: the particle stays).  Particles with d >= 0 are not written."""
    rb, m, vol_args = _mesh_volumes(mesh_rb, bodies)
    position = T.dev(position, "position")
    assert position.shape[-1] == 3
    lib = _lib.load()
    _lib.check(lib.mfs_mesh_project3d(T.ptr(rb), m, *vol_args, T.ptr(position), T.code(position),
                                      int(position.numel() // 3), T.stream()), "mfs_mesh_project3d")
