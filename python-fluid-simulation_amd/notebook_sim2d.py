"""The 2D time step: `notebook_sim.NotebookSimulation` one dimension down, on the 2D drop-ins.

The reference ships the 2D solvers (solver/PressureCGSolver2D.py, ViscosityCGSolver2D.py, DensityCGSolver2D.py,
sdf2D.py) but no 2D driver; this one follows the 3D notebook's containers (code cell 9) and loop body (code cell 11)
line for line with the z axis removed: advect, `sdf2D.project`, level set / fluid volume, density solve, p2g, gravity,
viscosity CG, pressure CG, extrapolate, boundary condition, g2p -- every stage a HIP kernel behind the C ABI.
Same container dtypes as 3D: bounds / biases float32, cell sizes float64 (float32 / int64), particle arrays float64,
grid mass and velocity float32, level sets and fluid volume float64.  Single GPU; the 2D engines have no Jacobi option
and there are no slab / sharded variants.
"""
import time
import types

import numpy as np
import torch

import notebook_kernels2d as K
from mfs import surface as _surface
from mfs.motion import BodyKinematics
from solver import sdf2D as sdf
from solver.CGSolverBuffer import CGSolverBuffer
from solver.DensityCGSolver2D import DensityCGSolver2D
from solver.PressureCGSolver2D import PressureCGSolver2D
from solver.ViscosityCGSolver2D import ViscosityCGSolver2D

NS = types.SimpleNamespace


def grid_positions(res, bound_min, cell_size, bias, device):
    """get_grid_pos of the notebook in 2D: bound_min + (float32 index + float32 bias) * cell_size, float64."""
    ax = [torch.arange(int(r), dtype=torch.float32, device=device) for r in res]
    idx = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1)
    b = torch.as_tensor(np.asarray(bias, np.float32), device=device)
    cs = torch.as_tensor(np.asarray(cell_size, np.float64), device=device)
    bm = torch.as_tensor(np.asarray(bound_min, np.float32), device=device).to(torch.float64)
    return (bm + (idx + b).to(torch.float64) * cs).contiguous()


class NotebookSimulation2D:
    """gres, gdx: cell grid (Nx, Ny) and spacing; bound_min: float32 pair; rb_d: packed rigid bodies (solver.sdf2D);
    px: (P,2) float64 particle positions; pdx: particle spacing (mass = rho * pdx^2, volume = pdx^2);
    motion: {body index: mfs.motion.Motion} -- those bodies move: `rb_d` is updated in place every step and the solid level
    set and velocity are re-evaluated at the new pose.  None: solids are static scene data."""

    def __init__(self, gres, gdx, bound_min, rb_d, px, pdx, rho=1000.0, mu=1.0, dt=1.0 / 300.0, device="cuda",
                 precision=None, motion=None, mesh_bodies=None):
        if mesh_bodies:
            raise NotImplementedError("mesh_bodies: triangle-mesh solids are 3D and single-GPU (NotebookSimulation)")
        dev = torch.device(device)
        g = tuple(int(v) for v in gres)
        if len(g) != 2:
            raise ValueError(f"NotebookSimulation2D needs a 2D grid, got {g}")
        self.GRES, self.GDX, self.PDX, self.RHO, self.MU, self.DT = g, float(gdx), float(pdx), float(rho), float(mu), float(dt)
        self.device = dev
        bmin = np.asarray(bound_min, np.float32)
        bsz = (np.asarray(g, np.float64) * gdx).astype(np.float32)         # BOUND_SIZE is a float32 array
        self.BOUND_MIN, self.BOUND_SIZE = bmin, bsz
        self.rb_d = rb_d
        px = torch.as_tensor(px, dtype=torch.float64, device=dev).contiguous()
        n = px.shape[0]
        z2 = lambda: torch.zeros((n, 2), dtype=torch.float64, device=dev)  # noqa: E731
        self.particle = NS(num_particles=n, x=px, m=torch.full((n,), rho * pdx ** 2, dtype=torch.float64, device=dev),
                           v=z2(), cx=z2(), cy=z2(), vol=pdx ** 2)
        eye = np.eye(2, dtype=np.int64)
        cs = bsz / np.asarray(g, np.int64)                                 # float32 / int64 -> float64

        def comp(a, bias):
            shape = tuple(int(v) for v in np.asarray(g) + eye[a])
            f = lambda: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
            return NS(resolution=shape, bias=np.asarray(bias, np.float32), m=f(), v=f(), dv=f())
        self.grid = NS(resolution=g, bound_size=bsz, bound_min=bmin, cell_size=cs, x=comp(0, [0, .5]), y=comp(1, [.5, 0]))
        dres = tuple(2 * v + 1 for v in g)
        dcs = bsz / (2 * np.asarray(g, np.int64))
        self.solid_levelset = NS(resolution=dres, bound_size=bsz, bound_min=bmin, cell_size=dcs,
                                 bias=np.zeros(2, np.float32),
                                 phi=torch.zeros(dres, dtype=torch.float64, device=dev),
                                 v=torch.zeros(dres + (2,), dtype=torch.float64, device=dev))
        self.solid_levelset.pos = grid_positions(dres, bmin, dcs, self.solid_levelset.bias, dev)
        sdf.evaluate(rb_d, self.solid_levelset.phi, self.solid_levelset.v, self.solid_levelset.pos)
        self.fluid_levelset = NS(resolution=g, bound_size=bsz, bound_min=bmin, cell_size=cs,
                                 phi=torch.zeros(g, dtype=torch.float64, device=dev))
        self.fluid_volume = NS(resolution=dres, bound_size=bsz, bound_min=bmin, cell_size=dcs,
                               vol=torch.zeros(dres, dtype=torch.float64, device=dev))
        self.kinematics = BodyKinematics(rb_d, motion, 2) if motion else None
        self._precision = precision
        self.CGBuf = CGSolverBuffer(g, precision=precision, device=dev)
        self.PressureSolver = PressureCGSolver2D(self.CGBuf, g, self.BOUND_SIZE)
        self.DensitySolver = DensityCGSolver2D(self.CGBuf, g, self.BOUND_MIN, self.BOUND_SIZE)
        self.ViscositySolver = ViscosityCGSolver2D(g, self.BOUND_SIZE, precision=precision, device=dev)
        self.current_time = 0.0
        self.iterations = 0

    def surface(self, which="liquid"):
        """`mfs.surface.Contour` of the liquid ({fluid_levelset.phi < 0}, closed against the array border) or of the solid
        ({solid_levelset.phi < 0} on the doubled grid): `NotebookSimulation.surface` one dimension down."""
        return _surface.simulation_surface(self, which, 2)

    def skin(self, *args, **kw):
        raise NotImplementedError("skin() is 3D (NotebookSimulation.skin, mfs.skin): the 2D class has `surface()`")

    def render(self, *args, **kw):
        raise NotImplementedError("render() is 3D (NotebookSimulation.render, mfs.render), color_by included")

    def sample_particles(self, *args, **kw):
        raise NotImplementedError("sample_particles() is 3D (NotebookSimulation.sample_particles, mfs.attrib)")

    def step(self, duration_left=float("inf"), timings=None):
        """One pass of the loop body.  Returns the dt it took."""
        p, g, sl, fl, fv = self.particle, self.grid, self.solid_levelset, self.fluid_levelset, self.fluid_volume

        def tick(name, t0):
            if timings is not None:
                torch.cuda.synchronize()
                timings[name] = timings.get(name, 0.0) + time.perf_counter() - t0
            return time.perf_counter()

        t = time.perf_counter()
        vmax = torch.sqrt((p.v ** 2).sum(dim=-1)).max().item() if p.num_particles else 0.0
        cfl_dt = self.GDX / max(1e-10, vmax)
        dt = min(self.DT, cfl_dt, duration_left)
        t0 = self.current_time
        if self.kinematics is not None:                                     # a body crosses at most one cell per step
            dt = min(dt, self.GDX / max(1e-10, self.kinematics.max_surface_speed(t0)))
        self.current_time += dt
        p.x += p.v * dt
        if self.kinematics is not None:                                     # bodies to their pose at t0 + dt
            self.kinematics.advance(t0, dt)
        sdf.project(self.rb_d, p.x)
        t = tick("advect+project", t)
        if self.kinematics is not None:                                     # solid level set and surface velocity there
            sdf.evaluate_grid(self.rb_d, sl.phi, sl.v, sl.bound_min, sl.cell_size, sl.bias, rb_w=self.kinematics.rb_w)
            t = tick("solid", t)
        K.compute_fluid_levelset(p, fl, self.GDX)
        K.compute_fluid_volume(p, fv, p.vol)
        t = tick("levelset+volume", t)
        self.DensitySolver.solve(self.RHO, dt, p.x, p.m, p.vol, g.x.v, g.y.v, sl.phi, sl.v, fl.phi, fv.vol)
        t = tick("density", t)
        K.compute_fluid_levelset(p, fl, self.GDX)
        K.compute_fluid_volume(p, fv, p.vol)
        t = tick("levelset+volume", t)
        for c in (g.x, g.y):
            c.m.zero_()
            c.v.zero_()
        K.p2g(p, g)
        g.y.v += -10 * dt                                                   # gravity
        t = tick("p2g", t)
        if self.MU > 0:
            self.ViscositySolver.solve(dt, self.MU, self.RHO, g.x.v, g.y.v, sl.phi, sl.v, fl.phi, fv.vol)
        t = tick("viscosity", t)
        ds = self.DensitySolver
        self.PressureSolver.solve(g.x.v, g.y.v, sl.phi, sl.v, fl.phi, wx=ds.wx, wy=ds.wy)
        t = tick("pressure", t)
        K.extrapolate(self.GRES, 2, g.x.v, g.y.v, g.x.m, g.y.m)
        K.apply_boundary_condition(g, sl, self.GDX)
        t = tick("extrapolate+bc", t)
        K.g2p(p, g)
        tick("g2p", t)
        self.iterations += 1
        return dt


def add_box(center, size, dx, rng, keep=None):
    """Particle seeding (`add_box` of the notebook) in 2D: a jittered lattice of spacing dx filling a box."""
    center, size = np.asarray(center, np.float64), np.asarray(size, np.float64)
    dims = (size / dx).astype(np.int64)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in dims]), axis=-1).astype(np.float32)
    pos = (center - 0.5 * size) + size * ((idx + 0.5) / dims)
    pos = pos.reshape(-1, 2)
    if keep is not None:
        pos = pos[keep(pos)]
    return pos + rng.standard_normal(pos.shape) * dx * 0.3
