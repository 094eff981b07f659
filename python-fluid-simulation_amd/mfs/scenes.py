"""Seeded synthetic inputs for the pressure / viscosity CG solvers.

Everything here *generates inputs*; nothing here is solver arithmetic.  The
array conventions are the reference's: C-order, axis
order [x, y, z]; cell arrays (Nx,Ny,Nz); face arrays vx (Nx+1,Ny,Nz),
vy (Nx,Ny+1,Nz), vz (Nx,Ny,Nz+1); doubled grid sphi / lvol
(2Nx+1,2Ny+1,2Nz+1) with (2x+1,2y+1,2z+1) the cell centre; sv (...,3).
`sphi < 0` is inside solid, `lphi < 0` is inside fluid
(reference: solver/PressureCGSolver3D.py:137,183, solver/SolidFraction3D.py:12-18).

Generators are written once against a tiny array-namespace adapter so that the
same formulas run in numpy (goldens, CPU tests, the oracle) and in torch on the
device (bench-size slabs that should never be built on the host).
"""
from __future__ import annotations

import math

import numpy as np


class _NP:
    float64 = np.float64

    @staticmethod
    def arange(a, b):
        return np.arange(a, b, dtype=np.float64)

    minimum = staticmethod(np.minimum)
    maximum = staticmethod(np.maximum)
    sqrt = staticmethod(np.sqrt)
    sin = staticmethod(np.sin)
    cos = staticmethod(np.cos)
    abs = staticmethod(np.abs)

    @staticmethod
    def clip(a, lo, hi):
        return np.clip(a, lo, hi)

    @staticmethod
    def full(shape, v):
        return np.full(shape, v, dtype=np.float64)

    @staticmethod
    def stack_last(arrs):
        return np.stack(arrs, axis=-1)


class _Torch:
    def __init__(self, device):
        import torch
        self.t = torch
        self.device = device
        self.float64 = torch.float64
        self.minimum = torch.minimum
        self.maximum = torch.maximum
        self.sqrt = torch.sqrt
        self.sin = torch.sin
        self.cos = torch.cos
        self.abs = torch.abs

    def arange(self, a, b):
        return self.t.arange(a, b, dtype=self.t.float64, device=self.device)

    def clip(self, a, lo, hi):
        return self.t.clamp(a, lo, hi)

    def full(self, shape, v):
        return self.t.full(shape, v, dtype=self.t.float64, device=self.device)

    def stack_last(self, arrs):
        return self.t.stack(arrs, dim=-1)


def _xp(device):
    return _NP() if device is None else _Torch(device)


def _axes(xp, lo, hi, step, origin=0.0):
    """coordinate = origin + index*step for index in [lo, hi)."""
    return origin + xp.arange(lo, hi) * step


def _b3(ax, ay, az):
    return ax[:, None, None], ay[None, :, None], az[None, None, :]


# ----------------------------------------------------------------------------
# solid level set shared by the 3D scenes: closed box walls + a sphere obstacle
# ----------------------------------------------------------------------------
def _sphi_box_sphere(xp, X, Y, Z, size, wall, sph_c, sph_r):
    """>0 in the open domain, <0 in walls (thickness `wall`) and in the sphere."""
    box = xp.minimum(xp.minimum(xp.minimum(X, size[0] - X), xp.minimum(Y, size[1] - Y)),
                     xp.minimum(Z, size[2] - Z)) - wall
    sph = xp.sqrt((X - sph_c[0]) ** 2 + (Y - sph_c[1]) ** 2 + (Z - sph_c[2]) ** 2) - sph_r
    return xp.minimum(box + 0 * sph, sph + 0 * box)


def pressure_scene_3d(gres, seed=0, *, bound_size=(1.0, 1.0, 1.0), vel_dtype=np.float32,
                      solid_velocity=False, all_fluid=False, x_range=None, device=None,
                      noise=1e-2):
    """C2 of SURVEY.md 8(d): pool with a flat-ish free surface, box walls, sphere.

    x_range=(a, b) builds only cell planes [a, b) of the global grid (and the
    matching face / doubled-grid planes): the slab a rank owns plus its ghosts.
    Returns a dict of arrays (numpy when device is None, torch otherwise).
    """
    xp = _xp(device)
    Nx, Ny, Nz = (int(g) for g in gres)
    a, b = (0, Nx) if x_range is None else x_range
    size = tuple(float(s) for s in bound_size)
    cs = (size[0] / Nx, size[1] / Ny, size[2] / Nz)
    wall = 1.5 * min(cs)
    sph_c = (0.5 * size[0], 0.3 * size[1], 0.5 * size[2])
    sph_r = 0.12 * min(size)

    # doubled grid nodes of the slab: indices [2a, 2b] inclusive
    dx = _axes(xp, 2 * a, 2 * b + 1, 0.5 * cs[0])
    dy = _axes(xp, 0, 2 * Ny + 1, 0.5 * cs[1])
    dz = _axes(xp, 0, 2 * Nz + 1, 0.5 * cs[2])
    X, Y, Z = _b3(dx, dy, dz)
    if all_fluid:
        # open interior everywhere except the outermost half-cell shell
        sphi = xp.minimum(xp.minimum(xp.minimum(X, size[0] - X), xp.minimum(Y, size[1] - Y)),
                          xp.minimum(Z, size[2] - Z)) + 0.25 * min(cs)
    else:
        sphi = _sphi_box_sphere(xp, X, Y, Z, size, wall, sph_c, sph_r)

    if solid_velocity:
        svx = 0.3 * xp.sin(2.0 * Y) + 0 * X + 0 * Z
        svy = -0.2 * xp.cos(3.0 * Z) + 0 * X + 0 * Y
        svz = 0.1 * xp.sin(X + Y) + 0 * Z
    else:
        svx = svy = svz = 0 * (X + Y + Z)
    sv = xp.stack_last([svx, svy, svz])

    # cell centres
    cx = _axes(xp, a, b, cs[0], 0.5 * cs[0])
    cy = _axes(xp, 0, Ny, cs[1], 0.5 * cs[1])
    cz = _axes(xp, 0, Nz, cs[2], 0.5 * cs[2])
    CX, CY, CZ = _b3(cx, cy, cz)
    if all_fluid:
        lphi = xp.full((b - a, Ny, Nz), -1.0)
    else:
        lphi = (CY - 0.62 * size[1]) + 0.03 * size[1] * xp.sin(2 * math.pi * CX / size[0]) \
            * xp.cos(2 * math.pi * CZ / size[2])

    # staggered velocity = gradient of a smooth potential (divergent) + noise
    two_pi = 2 * math.pi

    def pot_grad(PX, PY, PZ, axis):
        sx, sy, sz = (xp.sin(two_pi * PX / size[0]), xp.sin(two_pi * PY / size[1]),
                      xp.sin(two_pi * PZ / size[2]))
        cxx, cyy, czz = (xp.cos(two_pi * PX / size[0]), xp.cos(two_pi * PY / size[1]),
                         xp.cos(two_pi * PZ / size[2]))
        if axis == 0:
            return two_pi / size[0] * cxx * sy * sz * cs[0]
        if axis == 1:
            return two_pi / size[1] * sx * cyy * sz * cs[1]
        return two_pi / size[2] * sx * sy * czz * cs[2]

    fx = _axes(xp, a, b + 1, cs[0])
    fy = _axes(xp, 0, Ny + 1, cs[1])
    fz = _axes(xp, 0, Nz + 1, cs[2])
    vx = pot_grad(*_b3(fx, cy, cz), 0)
    vy = pot_grad(*_b3(cx, fy, cz), 1)
    vz = pot_grad(*_b3(cx, cy, fz), 2)

    out = dict(gres=(Nx, Ny, Nz), x_range=(a, b), bound_size=size, cell_size=cs,
               sphi=sphi, sv=sv, lphi=lphi)
    if device is None:
        rng = np.random.default_rng(seed)
        # noise drawn for the full grid so that a slab is a slice of the global field
        nvx = rng.standard_normal((Nx + 1, Ny, Nz))[a:b + 1]
        nvy = rng.standard_normal((Nx, Ny + 1, Nz))[a:b]
        nvz = rng.standard_normal((Nx, Ny, Nz + 1))[a:b]
        out["vx"] = (vx + noise * nvx).astype(vel_dtype)
        out["vy"] = (vy + noise * nvy).astype(vel_dtype)
        out["vz"] = (vz + noise * nvz).astype(vel_dtype)
    else:
        import torch
        g = torch.Generator(device=device)
        g.manual_seed(seed * 7919 + a)
        tdt = {np.float32: torch.float32, np.float64: torch.float64}.get(vel_dtype, vel_dtype)
        for name, arr in (("vx", vx), ("vy", vy), ("vz", vz)):
            n = torch.randn(arr.shape, generator=g, device=device, dtype=torch.float64)
            out[name] = (arr + noise * n).to(tdt)
    return out


# ----------------------------------------------------------------------------
# 2D pressure scene (config 1 of BASELINE.json; reference solver/PressureCGSolver2D.py)
# ----------------------------------------------------------------------------
def pressure_scene_2d(gres, seed=1, *, bound_size=(1.0, 1.0), vel_dtype=np.float64,
                      solid_velocity=False):
    Nx, Ny = (int(g) for g in gres)
    size = tuple(float(s) for s in bound_size)
    cs = (size[0] / Nx, size[1] / Ny)
    dx = np.arange(2 * Nx + 1) * 0.5 * cs[0]
    dy = np.arange(2 * Ny + 1) * 0.5 * cs[1]
    X, Y = dx[:, None], dy[None, :]
    sphi = np.minimum(np.minimum(X, size[0] - X), np.minimum(Y, size[1] - Y)) - 0.05 * min(size)
    if solid_velocity:
        sv = np.stack([0.3 * np.sin(2 * Y) + 0 * X, -0.2 * np.cos(3 * X) + 0 * Y], axis=-1)
    else:
        sv = np.zeros((2 * Nx + 1, 2 * Ny + 1, 2))
    cx = (np.arange(Nx) + 0.5) * cs[0]
    cy = (np.arange(Ny) + 0.5) * cs[1]
    lphi = np.sqrt((cx[:, None] - 0.5 * size[0]) ** 2 + (cy[None, :] - 0.5 * size[1]) ** 2) \
        - 0.3 * min(size)
    rng = np.random.default_rng(seed)
    vx = rng.standard_normal((Nx + 1, Ny)).astype(vel_dtype)
    vy = rng.standard_normal((Nx, Ny + 1)).astype(vel_dtype)
    return dict(gres=(Nx, Ny), bound_size=size, cell_size=cs, sphi=sphi, sv=sv, lphi=lphi,
                vx=vx, vy=vy)


def pressure_scene_2d_edges(gres, seed=3, *, vel_dtype=np.float64):
    """The level-set edges of the 2D pressure solver on exact binary-fraction geometry (cell size 1, integer offsets).

    sphi (doubled grid, value = distance in cells): walls whose surface passes through the corner nodes at x = 1,
    x = Nx - 1, y = 1, y = Ny - 1 (exact 0.0) and a diamond obstacle at an integer centre (half-integer values at the
    corner nodes: its edges are cut in half, w = 0.5).
    Every second exact zero is stored as -0.0; both are "not solid" (`< 0` is false).
    lphi (cell centres): a liquid pool along the longer axis u, cell rows v < L(u) liquid (integer depths), the
    surface row v = L(u) patterned by u mod 4:
      0: 0.0 (air at exactly zero)           1: -1e-4 just below, +1.0 at the surface (theta clamp in apply and update)
      2: -0.0 (air at a signed zero)         3: -1e-4 just below, 0.0 at the surface (theta exactly 1)
    L alternates between two depths every 4 columns, so thin grids (one interior row or column) meet every pattern
    both as a liquid and as an air interior cell.  Solid velocity is on."""
    Nx, Ny = (int(g) for g in gres)
    I = np.arange(2 * Nx + 1, dtype=np.float64)[:, None] * 0.5
    J = np.arange(2 * Ny + 1, dtype=np.float64)[None, :] * 0.5
    wall = np.minimum(np.minimum(I, Nx - I), np.minimum(J, Ny - J)) - 1.0
    diamond = np.abs(I - (Nx // 2)) + np.abs(J - (Ny // 2)) - max(1, min(Nx, Ny) // 4) - 0.5
    sphi = np.minimum(wall, diamond)
    ii, jj = np.meshgrid(np.arange(2 * Nx + 1), np.arange(2 * Ny + 1), indexing="ij")
    sphi[(sphi == 0) & ((ii + jj) // 2 % 2 == 1)] = -0.0
    sv = np.stack([0.3 * np.sin(0.37 * J) + 0 * I, -0.2 * np.cos(0.23 * I) + 0 * J], axis=-1)

    transpose = Ny > Nx                       # u: the longer axis, v: the other
    Nu, Nv = (Ny, Nx) if transpose else (Nx, Ny)
    u = np.arange(Nu)
    L = np.clip(Nv // 2 + (u // 4) % 2, 1, max(1, Nv - 1))
    f = np.arange(Nv, dtype=np.float64)[None, :] - L[:, None]          # (Nu, Nv): negative below the surface
    for k in range(Nu):
        s, pat = int(L[k]), k % 4
        if pat == 0:
            f[k, s] = 0.0
        elif pat == 1:
            f[k, s - 1], f[k, s] = -1e-4, 1.0
        elif pat == 2:
            f[k, s] = -0.0
        else:
            f[k, s - 1], f[k, s] = -1e-4, 0.0
    lphi = np.ascontiguousarray(f.T if transpose else f)
    rng = np.random.default_rng(seed)
    vx = rng.standard_normal((Nx + 1, Ny)).astype(vel_dtype)
    vy = rng.standard_normal((Nx, Ny + 1)).astype(vel_dtype)
    return dict(gres=(Nx, Ny), bound_size=(float(Nx), float(Ny)), cell_size=(1.0, 1.0), sphi=sphi, sv=sv,
                lphi=lphi, vx=vx, vy=vy)


# ----------------------------------------------------------------------------
# 2D viscosity scene (reference solver/ViscosityCGSolver2D.py)
# ----------------------------------------------------------------------------
def viscosity_scene_2d(gres, seed=4, *, bound_size=(1.0, 1.0), vel_dtype=np.float64, mu=1.0, dt=1.0 / 300.0,
                       rho=1000.0, noise=0.5):
    """Walls one cell thick and a disc obstacle (sphi, doubled grid), a rectangular liquid body whose edges cut
    sub-cells (partial `lvol`), and a shear flow plus noise on EVERY face, solid ones included.  sphi is built in
    doubled-grid index units times the half cell size: the wall's surface (index 2 from each side) and the disc's
    points at integer distance r from its integer centre are exactly 0.0 on any grid (the 2D solver treats
    sphi == 0 as solid)."""
    Nx, Ny = (int(g) for g in gres)
    size = tuple(float(s) for s in bound_size)
    cs = (size[0] / Nx, size[1] / Ny)
    h = 0.5 * min(cs)
    I = np.arange(2 * Nx + 1, dtype=np.float64)[:, None]
    J = np.arange(2 * Ny + 1, dtype=np.float64)[None, :]
    wall = np.minimum(np.minimum(I, 2 * Nx - I), np.minimum(J, 2 * Ny - J)) - 2.0
    k = max(1, int(round(0.3 * min(Nx, Ny) / 5.0)))
    ci, cj, r = float(Nx), float(int(round(0.7 * Ny))), 5.0 * k        # 3-4-5 offsets land on the circle exactly
    disc = np.sqrt((I - ci) ** 2 + (J - cj) ** 2) - r
    sphi = np.minimum(wall, disc) * h
    sv = np.zeros((2 * Nx + 1, 2 * Ny + 1, 2))

    # liquid body [lo, hi]: lvol(node) = overlap with the sub-cell box of edge 0.5 cs centred on the node
    lo = (0.13 * size[0], 0.07 * size[1])
    hi = (0.81 * size[0], 0.63 * size[1])
    X, Y = I * 0.5 * cs[0], J * 0.5 * cs[1]

    def overlap(P, l, hh, half):
        return np.clip(np.minimum(P + half, hh) - np.maximum(P - half, l), 0.0, 2 * half)

    lvol = overlap(X, lo[0], hi[0], 0.25 * cs[0]) * overlap(Y, lo[1], hi[1], 0.25 * cs[1])
    cx = (np.arange(Nx) + 0.5) * cs[0]
    cy = (np.arange(Ny) + 0.5) * cs[1]
    lphi = np.maximum(np.maximum(lo[0] - cx[:, None], cx[:, None] - hi[0]),
                      np.maximum(lo[1] - cy[None, :], cy[None, :] - hi[1]))

    rng = np.random.default_rng(seed)
    fy_x = (np.arange(Ny) + 0.5) * cs[1]
    fx_y = (np.arange(Nx) + 0.5) * cs[0]
    vx = 1.0 + np.sin(6.0 * fy_x)[None, :] + noise * rng.standard_normal((Nx + 1, Ny))
    vy = -0.5 * np.cos(5.0 * fx_y)[:, None] + noise * rng.standard_normal((Nx, Ny + 1))
    return dict(gres=(Nx, Ny), bound_size=size, cell_size=cs, sphi=sphi, sv=sv, lphi=lphi, lvol=lvol,
                vx=vx.astype(vel_dtype), vy=vy.astype(vel_dtype), dt=float(dt), mu=float(mu), rho=float(rho))


# ----------------------------------------------------------------------------
# viscosity scene (config 3): buckling-like block of viscous fluid above slabs
# ----------------------------------------------------------------------------
def _box_sdf(xp, X, Y, Z, centre, half):
    """signed distance to an axis-aligned box (negative inside); the semantics
    of the reference's box SDF (solver/sdf3D.py:86-109) for an unrotated box."""
    qx = xp.abs(X - centre[0]) - half[0]
    qy = xp.abs(Y - centre[1]) - half[1]
    qz = xp.abs(Z - centre[2]) - half[2]
    zero = 0 * (qx + qy + qz)
    outside = xp.sqrt(xp.maximum(qx, zero) ** 2 + xp.maximum(qy, zero) ** 2
                      + xp.maximum(qz, zero) ** 2)
    inside = xp.minimum(xp.maximum(xp.maximum(qx + zero, qy + zero), qz + zero), zero)
    return outside + inside


def viscosity_scene_3d(gres, seed=3, *, bound_size=(1.0, 1.0, 1.0), vel_dtype=np.float32,
                       x_range=None, device=None, noise=5e-2):
    """C3 of SURVEY.md 8(d): a container (flipped box), two obstacle slabs under a
    block of fluid; `lvol` is the analytic sub-cell coverage of the fluid block
    times the sub-cell volume (what the notebook's compute_fluid_volume produces,
    ipynb c6), velocities (-2,0,0)+noise inside the block.
    """
    xp = _xp(device)
    Nx, Ny, Nz = (int(g) for g in gres)
    a, b = (0, Nx) if x_range is None else x_range
    size = tuple(float(s) for s in bound_size)
    cs = (size[0] / Nx, size[1] / Ny, size[2] / Nz)
    dx = _axes(xp, 2 * a, 2 * b + 1, 0.5 * cs[0])
    dy = _axes(xp, 0, 2 * Ny + 1, 0.5 * cs[1])
    dz = _axes(xp, 0, 2 * Nz + 1, 0.5 * cs[2])
    X, Y, Z = _b3(dx, dy, dz)
    c = (0.5 * size[0], 0.5 * size[1], 0.5 * size[2])
    container = -_box_sdf(xp, X, Y, Z, c, (0.5 * size[0] - 1.6 * cs[0], 0.5 * size[1] - 1.6 * cs[1],
                                          0.5 * size[2] - 1.6 * cs[2]))
    slab1 = _box_sdf(xp, X, Y, Z, (0.30 * size[0], 0.33 * size[1], c[2]),
                     (0.16 * size[0], 0.04 * size[1], 0.6 * size[2]))
    slab2 = _box_sdf(xp, X, Y, Z, (0.72 * size[0], 0.30 * size[1], c[2]),
                     (0.14 * size[0], 0.05 * size[1], 0.6 * size[2]))
    sphi = xp.minimum(xp.minimum(container, slab1), slab2)
    sv = xp.stack_last([0 * sphi, 0 * sphi, 0 * sphi])

    # fluid block [lo, hi]; lvol(node) = overlap of the block with the sub-cell box
    # centred on the node, edge 0.5*cs (so interior nodes carry cell_vol/8).
    lo = (0.28 * size[0], 0.42 * size[1], 0.30 * size[2])
    hi = (0.74 * size[0], 0.80 * size[1], 0.72 * size[2])

    def overlap(P, l, h, half):
        return xp.clip(xp.minimum(P + half, 0 * P + h) - xp.maximum(P - half, 0 * P + l), 0.0, 2 * half)

    lvol = overlap(X, lo[0], hi[0], 0.25 * cs[0]) * overlap(Y, lo[1], hi[1], 0.25 * cs[1]) \
        * overlap(Z, lo[2], hi[2], 0.25 * cs[2])

    cx = _axes(xp, a, b, cs[0], 0.5 * cs[0])
    cy = _axes(xp, 0, Ny, cs[1], 0.5 * cs[1])
    cz = _axes(xp, 0, Nz, cs[2], 0.5 * cs[2])
    CX, CY, CZ = _b3(cx, cy, cz)
    blk = _box_sdf(xp, CX, CY, CZ, tuple(0.5 * (l + h) for l, h in zip(lo, hi)),
                   tuple(0.5 * (h - l) for l, h in zip(lo, hi)))
    lphi = blk + 0 * (CX + CY + CZ)

    fx = _axes(xp, a, b + 1, cs[0])
    fy = _axes(xp, 0, Ny + 1, cs[1])
    fz = _axes(xp, 0, Nz + 1, cs[2])

    def inside(PX, PY, PZ):
        s = _box_sdf(xp, PX, PY, PZ, tuple(0.5 * (l + h) for l, h in zip(lo, hi)),
                     tuple(0.5 * (h - l) + 1.5 * min(cs) for l, h in zip(lo, hi)))
        return (s < 0) * 1.0

    mx = inside(*_b3(fx, cy, cz))
    my = inside(*_b3(cx, fy, cz))
    mz = inside(*_b3(cx, cy, fz))
    shear = lambda P: 1.0 + 0.5 * xp.sin(6.0 * P)  # noqa: E731
    bx = -2.0 * mx * shear(_b3(fx, cy, cz)[1] + 0 * mx)
    by = -0.5 * my * shear(_b3(cx, fy, cz)[0] + 0 * my)
    bz = 0.3 * mz * shear(_b3(cx, cy, fz)[1] + 0 * mz)

    out = dict(gres=(Nx, Ny, Nz), x_range=(a, b), bound_size=size, cell_size=cs,
               sphi=sphi, sv=sv, lphi=lphi, lvol=lvol, dt=1.0 / 300.0, mu=1.0, rho=1000.0)
    if device is None:
        rng = np.random.default_rng(seed)
        nx = rng.standard_normal((Nx + 1, Ny, Nz))[a:b + 1]
        ny = rng.standard_normal((Nx, Ny + 1, Nz))[a:b]
        nz = rng.standard_normal((Nx, Ny, Nz + 1))[a:b]
        out["vx"] = (bx + noise * nx * mx).astype(vel_dtype)
        out["vy"] = (by + noise * ny * my).astype(vel_dtype)
        out["vz"] = (bz + noise * nz * mz).astype(vel_dtype)
    else:
        import torch
        g = torch.Generator(device=device)
        g.manual_seed(seed * 104729 + a)
        tdt = {np.float32: torch.float32, np.float64: torch.float64}.get(vel_dtype, vel_dtype)
        for name, arr, m in (("vx", bx, mx), ("vy", by, my), ("vz", bz, mz)):
            n = torch.randn(arr.shape, generator=g, device=device, dtype=torch.float64)
            out[name] = (arr + noise * n * m).to(tdt)
    return out


def density_scene_3d(gres, seed=0, *, per_cell=4, bound_min=(-0.25, 0.1, 0.0), px_dtype=np.float64, rho0=1000.0,
                     dt=1.0 / 300.0):
    """Inputs of DensityCGSolver3D.solve: the pool scene of `pressure_scene_3d`
    (shifted by `bound_min`) filled with jittered particles below the free surface; particle masses
    rho0 * pvol * (1 +- 10 %), so the density right-hand side is non-trivial.  numpy only."""
    sc = pressure_scene_3d(gres, seed)
    Nx, Ny, Nz = (int(g) for g in gres)
    size = np.asarray(sc["bound_size"], np.float64)
    cs = size / np.array([Nx, Ny, Nz], np.float64)
    rng = np.random.default_rng(seed + 1000)
    n = per_cell * Nx * Ny * Nz
    pos = rng.uniform(0.6 * cs, size - 0.6 * cs, size=(n, 3))
    ci = np.minimum((pos / cs).astype(np.int64), np.array([Nx - 1, Ny - 1, Nz - 1]))
    lphi = np.asarray(sc["lphi"])
    sphi_c = np.asarray(sc["sphi"])[1::2, 1::2, 1::2]
    keep = (lphi[ci[:, 0], ci[:, 1], ci[:, 2]] < 0) & (sphi_c[ci[:, 0], ci[:, 1], ci[:, 2]] > 0)
    pos = pos[keep]
    pvol = float(np.prod(cs)) / per_cell
    pm = rho0 * pvol * (1.0 + 0.1 * rng.standard_normal(len(pos)))
    px = (pos + np.asarray(bound_min, np.float64)).astype(px_dtype)
    lvol = np.zeros_like(np.asarray(sc["sphi"]))        # accepted and unused by the density solver (:262-269)
    return dict(gres=(Nx, Ny, Nz), bound_min=tuple(float(b) for b in bound_min), bound_size=tuple(float(v) for v in size),
                sphi=sc["sphi"], sv=sc["sv"], lphi=sc["lphi"], lvol=lvol, px=px, pm=pm, pvol=pvol, rho0=float(rho0),
                dt=float(dt))


def particle_scene_3d(gres, seed=0, *, per_cell=3, bound_min=(-0.3, 0.0, -0.3)):
    """Inputs of the notebook's particle <-> grid transfers: jittered particles in the
    lower part of a box with the notebook's origin (BOUND_MIN = (-0.3, 0, -0.3), ipynb code cell 9), a few of
    them pushed up to / beyond the walls so that the index clamps are exercised; velocities and affine rows
    random.  Cubic cells of size gdx.  numpy only."""
    Nx, Ny, Nz = (int(g) for g in gres)
    gdx = 0.05
    size = np.array([Nx, Ny, Nz], np.float64) * gdx
    rng = np.random.default_rng(seed + 2000)
    n = per_cell * Nx * Ny * Nz // 2
    pos = rng.uniform([0.8 * gdx, 0.8 * gdx, 0.8 * gdx], [size[0] - 0.8 * gdx, 0.55 * size[1], size[2] - 0.8 * gdx],
                      size=(n, 3))
    k = max(4, n // 50)                 # stragglers next to / outside the walls
    pos[:k] = rng.uniform(-0.4 * gdx, 0.7 * gdx, size=(k, 3)) + rng.integers(0, 2, size=(k, 3)) * (size - 0.3 * gdx)
    px = pos + np.asarray(bound_min, np.float64)
    pvol = gdx ** 3 / per_cell
    pm = 1000.0 * pvol * (1.0 + 0.1 * rng.standard_normal(n))
    pv = rng.standard_normal((n, 3))
    aff = [2.0 * rng.standard_normal((n, 3)) for _ in range(3)]
    return dict(gres=(Nx, Ny, Nz), bound_min=tuple(float(b) for b in bound_min), bound_size=tuple(float(v) for v in size),
                gdx=gdx, px=px, pm=pm, pv=pv, pcx=aff[0], pcy=aff[1], pcz=aff[2], pvol=float(pvol))


def particle_scene_2d(gres, seed=0, *, per_cell=4, bound_min=(-0.3, 0.0), device=None):
    """Inputs of the 2D particle <-> grid transfers (notebook_kernels2d), in the style of `particle_scene_3d`: jittered
    particles in a block in the lower part of a box of square cells of size gdx; particles pressed against each of the
    four walls (within 0.7 cell inside); a few outside the domain (up to 1.5 cells), so that the index clamps fire on both
    sides of both axes; one particle exactly at `bound_min`; a shuffled order; velocities and affine rows random.
    `bound_min` / `bound_size` are float32 arrays and `cell_size` float64, as the containers hold them.  numpy arrays, or
    torch tensors on `device` for the particle arrays when one is given."""
    Nx, Ny = (int(g) for g in gres)
    gdx = 0.05
    N = np.array([Nx, Ny], np.int64)
    bmin = np.asarray(bound_min, np.float32)
    bsz = (N * gdx).astype(np.float32)
    cs = bsz / N
    size = N * cs
    rng = np.random.default_rng(seed + 4000)
    n = max(8, per_cell * Nx * Ny // 2)
    block = rng.uniform([0.8, 0.8], [Nx - 0.8, max(1.0, 0.55 * Ny)], size=(n, 2))          # in cells
    k = max(4, n // 40)
    parts = [block]
    for a in range(2):
        for side in (0, 1):
            q = rng.uniform([0.0, 0.0], N.astype(np.float64), size=(2 * k, 2))
            d = np.concatenate([rng.uniform(0.0, 0.7, k), rng.uniform(-1.5, 0.0, k)])      # pressed against / outside
            q[:, a] = d if side == 0 else N[a] - d
            parts.append(q)
    X = np.concatenate(parts) * cs + bmin.astype(np.float64)
    X = np.concatenate([X, bmin.astype(np.float64)[None]])
    X = X[rng.permutation(len(X))]
    P = len(X)
    pvol = gdx ** 2 / per_cell
    out = dict(px=X, pm=1000.0 * pvol * (1.0 + 0.1 * rng.standard_normal(P)), pv=rng.standard_normal((P, 2)),
               pcx=2.0 * rng.standard_normal((P, 2)), pcy=2.0 * rng.standard_normal((P, 2)))
    if device is not None:
        import torch
        out = {k_: torch.as_tensor(v, device=device) for k_, v in out.items()}
    out.update(gres=(Nx, Ny), bound_min=bmin, bound_size=bsz, cell_size=cs, gdx=gdx, pvol=float(pvol),
               size=tuple(float(v) for v in size))
    return out


def particle_stress_scene_3d(gres=(100, 44, 67), seed=0, *, bulk=300000, per_wall=5000, bound_min=(-0.3, 0.0, -0.3),
                             bound_size=(1.2, 0.5, 0.9)):
    """A particle set built to reach what `particle_scene_3d` and a mesh-ordered block never do in the particle <-> grid
    transfers and their tile-sorted forms (tiles of 8^3 cells, csrc/mfs_particles.hip); tests/test_particle_stress_scene.py
    asserts each item:
      * extents that are no multiple of 8 and all different (partial tiles on every axis), three different cell sizes,
        float32 `bound_min` / `bound_size` and float64 cell sizes like the notebook's containers;
      * more particles than the tile-sort threshold, in SHUFFLED order: 256 consecutive particles lie in far more than
        the 128 tiles a workgroup's table of the sort holds;
      * at each of the six walls particles within 1.5 cells inside to 2 cells outside (low clamp of the base index, high
        clamp of the +1 / +2 neighbours), particles exactly at `bound_min`, exactly on the far walls and on interior
        cell faces (a zero weight on four of the eight corners);
      * the bulk fills y below 30 cells only: the tile layer of cells 32..39 stays empty but for ONE particle, every
        bulk tile holds several hundred (more than one pass of a 256-thread tile loop);
      * masses and velocities of both signs over three decades.
    numpy only; the same arrays for the same arguments."""
    N = np.array([int(g) for g in gres], np.int64)
    if N[1] < 42 or N[0] < 16 or N[2] < 16:
        raise ValueError("particle_stress_scene_3d needs gres[1] >= 42 (an empty tile layer above the bulk) and 16 cells elsewhere")
    bmin = np.asarray(bound_min, np.float32)
    bsz = np.asarray(bound_size, np.float32)
    cs = bsz / N                                            # float64, as float32 / int64 is in the notebook
    rng = np.random.default_rng(seed + 3000)
    b64 = bmin.astype(np.float64)
    ytop = 30.0                                             # the bulk's ceiling, in cells
    hi = np.array([N[0], ytop, N[2]], np.float64)
    parts = [rng.uniform([0.0, 0.0, 0.0], hi, size=(bulk, 3))]                 # in cells
    for a in range(3):
        for side in (0, 1):
            q = rng.uniform([0.0, 0.0, 0.0], hi if a != 1 else N.astype(np.float64), size=(per_wall, 3))
            d = rng.uniform(-2.0, 1.5, size=per_wall)       # distance into the box, cells; negative: outside
            q[:, a] = d if side == 0 else N[a] - d
            parts.append(q)
    X = np.concatenate(parts) * cs + b64
    # exact positions, float32-representable so that float32 particle arrays keep them: the corner at bound_min, one
    # coordinate at bound_min, the far walls and the faces N/2, N/4 where those are integers (k * cell_size is a float32
    # there: bound_size / 2, / 4), the others random in the bulk
    exact = [bmin.astype(np.float64)]
    for a in range(3):
        for k in (0, N[a], N[a] // 2 if N[a] % 2 == 0 else None, N[a] // 4 if N[a] % 4 == 0 else None):
            if k is None:
                continue
            for _ in range(16):
                q = (rng.uniform([0.0, 0.0, 0.0], hi, size=3) * cs + b64).astype(np.float32)
                face = np.float32(np.float32(bsz[a] * np.float32(k / N[a])) + bmin[a])
                # keep the candidate only if the kernels' own arithmetic lands on the integer
                if (np.float32(face - bmin[a]).astype(np.float64) / cs[a]) == float(k):
                    q[a] = face
                    exact.append(q.astype(np.float64))
    # the lonely particle: centre of a cell in the middle of the empty tile layer
    lone = (np.array([N[0] // 2 // 8 * 8 + 3.5, 35.5, N[2] // 2 // 8 * 8 + 3.5]) * cs + b64)
    X = np.concatenate([X, np.asarray(exact), lone[None]])
    n = len(X)
    order = rng.permutation(n)
    X = X[order]
    pvol = float(np.prod(cs)) / 8
    sgn = lambda size: np.where(rng.random(size) < 0.3, -1.0, 1.0)  # noqa: E731
    pm = 1000.0 * pvol * sgn(n) * 10.0 ** rng.uniform(-3.0, 0.0, n)
    pv = sgn((n, 3)) * 10.0 ** rng.uniform(-2.0, 1.0, (n, 3))
    aff = [2.0 * rng.standard_normal((n, 3)) for _ in range(3)]
    return dict(gres=tuple(int(v) for v in N), bound_min=bmin, bound_size=bsz, cell_size=cs, gdx=float(cs.min()),
                px=X, pm=pm, pv=pv, pcx=aff[0], pcy=aff[1], pcz=aff[2], pvol=pvol,
                lone=int(np.nonzero(order == n - 1)[0][0]))


# ----------------------------------------------------------------------------
# 2D density scene (reference solver/DensityCGSolver2D.py, solver/sdf2D.py)
# ----------------------------------------------------------------------------
def _rb2(kind, params, flip, centre, angle, vel=(0.0, 0.0)):
    """one (8,3) body block in the packed layout of solver/sdf2D.py: row 0 = [type code, parameters], rows 1-3
    translation, rows 4-6 rotation, row 7 velocity"""
    rb = np.zeros((8, 3))
    rb[0, 0] = {"sphere": 0, "box": 2}[kind] + (1 if flip else 0)
    rb[0, 1:1 + len(params)] = params
    rb[1:4] = np.identity(3)
    rb[1:3, 2] = centre
    rb[4:7] = np.identity(3)
    if angle:
        rad = angle * np.pi / 180
        c, s = np.cos(rad), np.sin(rad)
        rb[4:6, :2] = ((c, -s), (s, c))
    rb[7, :2] = vel
    return rb


def _sdf2(rb_d, X, Y):
    """signed distance to the closest body and that body's velocity where the distance is <= 0 (input generator for
    sphi / sv; sign convention of solver/sdf2D.py: a flipped body is solid OUTSIDE)"""
    sd = np.full(np.broadcast(X, Y).shape, 100.0)
    vel = np.zeros(sd.shape + (2,))
    win = np.zeros(sd.shape, dtype=np.int64)
    for i, rb in enumerate(rb_d):
        T, R = rb[1:3, 2], rb[4:6, :2]
        if rb[0, 0] // 2 == 0:
            d = np.sqrt((X - T[0]) ** 2 + (Y - T[1]) ** 2) - rb[0, 1]
        else:
            bx = R[0, 0] * (X - T[0]) + R[1, 0] * (Y - T[1])
            by = R[0, 1] * (X - T[0]) + R[1, 1] * (Y - T[1])
            ex, ey = np.abs(bx) - rb[0, 1] / 2, np.abs(by) - rb[0, 2] / 2
            d = np.sqrt(np.maximum(ex, 0) ** 2 + np.maximum(ey, 0) ** 2) + np.minimum(np.maximum(ex, ey), 0)
        if rb[0, 0] % 2:
            d = -d
        closer = d < sd
        sd = np.where(closer, d, sd)
        win = np.where(closer, i, win)
    inside = sd <= 0
    vel[inside] = np.asarray(rb_d)[win[inside], 7, :2]
    return sd, vel


def density_scene_2d(gres, seed=0, *, bound_min=(-0.2, 0.1), bound_size=(1.0, 1.0), per_cell=4, px_dtype=np.float64,
                     rho0=1000.0, dt=1.0 / 300.0, wall_particles=8):
    """Inputs of DensityCGSolver2D.solve and of sdf2D.evaluate / project.  numpy only.

    Bodies (`bodies`: what to hand to sdf2D.generate_rb / set_vel_rb; `rb_d`: the packed (3,8,3) array): a flipped box
    1.5 cells inside the bounds (the container), a box rotated by 30 degrees that moves, and a sphere.  `sphi`, `sv` are
    their signed distance / velocity on the doubled grid.  The liquid is a pool with a wavy surface: `lphi` at cell
    centres (a few surface cells sit a hair below zero, so the operator's theta clamp 0.01 is hit), `lvol` the pool's
    share of every doubled-grid node's sub-cell.  Particles: `per_cell` jittered per liquid cell, except a band of
    columns filled three times over (density fraction above its clamp 1.5) and a band left empty (fraction below 0.5
    at its edges, the `cell_mass < 1e-10` branch inside); `wall_particles` more within half a cell of each of the four
    bounds (index clamps of the scatter and the gathers)."""
    Nx, Ny = (int(g) for g in gres)
    bmin = np.asarray(bound_min, np.float64)
    size = np.asarray(bound_size, np.float64)
    cs = size / np.array([Nx, Ny], np.float64)
    ctr = bmin + 0.5 * size
    bodies = [
        dict(name="tank", rbparam=["box", float(size[0] - 3.0 * cs[0]), float(size[1] - 3.0 * cs[1])], flip=True,
             center=[float(ctr[0]), float(ctr[1])], angle=0, vel=[0.0, 0.0]),
        dict(name="bar", rbparam=["box", float(0.30 * size[0]), float(0.08 * size[1])], flip=False,
             center=[float(bmin[0] + 0.33 * size[0]), float(bmin[1] + 0.30 * size[1])], angle=30, vel=[0.3, -0.2]),
        dict(name="ball", rbparam=["sphere", float(0.11 * min(size))], flip=False,
             center=[float(bmin[0] + 0.72 * size[0]), float(bmin[1] + 0.36 * size[1])], angle=0, vel=[0.0, 0.0]),
    ]
    rb_d = np.stack([_rb2(b["rbparam"][0], b["rbparam"][1:], b["flip"], b["center"], b["angle"], b["vel"])
                     for b in bodies])
    X = (bmin[0] + np.arange(2 * Nx + 1) * 0.5 * cs[0])[:, None]
    Y = (bmin[1] + np.arange(2 * Ny + 1) * 0.5 * cs[1])[None, :]
    sphi, sv = _sdf2(rb_d, X, Y)

    def surface(x):
        return bmin[1] + size[1] * (0.58 + 0.04 * np.sin(7.0 * (x - bmin[0]) / size[0]))

    cx = bmin[0] + (np.arange(Nx) + 0.5) * cs[0]
    cy = bmin[1] + (np.arange(Ny) + 0.5) * cs[1]
    lphi = cy[None, :] - surface(cx)[:, None]
    top = np.clip((lphi < 0).sum(axis=1) - 1, 1, Ny - 2)          # topmost liquid cell of every column
    cols = np.arange(Nx)
    hair = (cols % 5 == 2) & (cols > 0) & (cols < Nx - 1)
    lphi[cols[hair], top[hair]] = -1e-4 * cs[1]
    # the pool's share of the sub-cell (0.5 cs)^2 around every doubled-grid node, none of it inside a solid
    lvol = np.clip(surface(X) - (Y - 0.25 * cs[1]), 0.0, 0.5 * cs[1]) * (0.5 * cs[0]) * (sphi > 0)

    rng = np.random.default_rng(seed + 2000)
    liquid = (lphi < 0) & (sphi[1::2, 1::2] > 0)
    full = (cols >= int(0.30 * Nx)) & (cols < int(0.30 * Nx) + 3)
    empty = (cols >= int(0.55 * Nx)) & (cols < int(0.55 * Nx) + 4)
    count = liquid * (per_cell * np.where(full, 3, 1) * ~empty)[:, None]
    ci, cj = np.nonzero(count)
    rep = count[ci, cj]
    ci, cj = np.repeat(ci, rep), np.repeat(cj, rep)
    pos = np.stack([bmin[0] + (ci + rng.uniform(0, 1, len(ci))) * cs[0],
                    bmin[1] + (cj + rng.uniform(0, 1, len(cj))) * cs[1]], axis=1)
    k = int(wall_particles)
    u, v = rng.uniform(0.02, 0.48, (4, k)), rng.uniform(0.05, 0.95, (4, k))
    walls = np.concatenate([
        np.stack([bmin[0] + u[0] * cs[0], bmin[1] + v[0] * size[1]], axis=1),
        np.stack([bmin[0] + size[0] - u[1] * cs[0], bmin[1] + v[1] * size[1]], axis=1),
        np.stack([bmin[0] + v[2] * size[0], bmin[1] + u[2] * cs[1]], axis=1),
        np.stack([bmin[0] + v[3] * size[0], bmin[1] + size[1] - u[3] * cs[1]], axis=1)])
    pos = np.concatenate([pos, walls])
    pvol = float(np.prod(cs)) / per_cell
    pm = rho0 * pvol * (1.0 + 0.1 * rng.standard_normal(len(pos)))
    return dict(gres=(Nx, Ny), bound_min=tuple(float(b) for b in bmin), bound_size=tuple(float(v) for v in size),
                cell_size=tuple(float(c) for c in cs), bodies=bodies, rb_d=rb_d, sphi=sphi, sv=sv, lphi=lphi, lvol=lvol,
                px=pos.astype(px_dtype), pm=pm, pvol=pvol, rho0=float(rho0), dt=float(dt))
