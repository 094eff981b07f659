#!/usr/bin/env python3
"""Generate tests/golden/step_moving_*.npz: whole time steps with a MOVING rigid body, by executing the reference's own
source (container only) exactly as tests/golden/make_goldens_step.py does -- same scene, same loop body, same refshim
plumbing -- plus a third body: a sphere of radius 0.08 at (-0.1, 0.5, 0), overlapping the fluid block by 0.06, that moves
at v = (0.6, 0, 0.15).  The reference has no driver for moving bodies; what it has is `transform_rb`, `set_vel_rb` and
`evaluate`, so every step runs

    advect -> centre += v dt -> transform_rb, set_vel_rb, evaluate (solid.phi / solid.v at the new pose) -> project -> the rest

with the reference's functions.  The body's own bound on dt, GDX / |v| = 0.05 / 0.62, is above DT and does not bind.
Needs the reference checkout (MFS_REFERENCE, as make_goldens_step.py)."""
import os

import make_goldens_step as G                      # the project's generator: paths, refshim, notebook cells, add_box
from make_goldens_step import N, CGSolverBuffer, DensityCGSolver3D, PressureCGSolver3D, ViscosityCGSolver3D, cp, cuda, np, sdf

HERE = os.path.dirname(os.path.abspath(__file__))
SPHERE_R, SPHERE_C, SPHERE_V = 0.08, (-0.1, 0.5, 0.0), (0.6, 0.0, 0.15)


def gen(name, gres, steps, seed, mu=1.0):
    ns = G.notebook_functions()
    GDX, PDX, RHO, MU, DT, D = 0.05, 0.025, 1000, mu, 1 / 300, 3
    GRES = cp.array(np.array(gres, np.int64))
    BOUND_MIN = cp.array([-0.3, 0, -0.3], dtype=cp.float32)
    BOUND_SIZE = cp.array(np.array(gres) * GDX, dtype=cp.float32)
    size = np.array(gres) * GDX
    rb_d, rb_map = cp.zeros((0, 10, 4)), {}
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'cube', ['box', size[0] - 2 * GDX, size[1] - 2 * GDX, size[2] - 2 * GDX], flip=True,
                                   center=[0, size[1] / 2, 0], axis=np.array([0., 1, 0]), angle=0)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.05, 0.8], flip=False, center=[-0.12, 0.2, 0],
                                   axis=np.array([0., 0, 1]), angle=-35)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ball', ['sphere', SPHERE_R], flip=False, center=list(SPHERE_C),
                                   axis=np.array([0., 1, 0]), angle=0)
    ball = rb_map['ball']
    centre, vel = np.array(SPHERE_C, np.float64), np.array(SPHERE_V, np.float64)
    assert GDX / np.linalg.norm(vel) > DT
    rng = np.random.default_rng(seed)
    PX = G.add_box([0.02, 0.5, 0.0], [0.2, 0.2, 0.2], PDX, rng)
    PN = PX.shape[0]
    particle = N(num_particles=PN, x=cp.array(PX), m=cp.ones(PN) * RHO * (PDX ** D), v=cp.zeros((PN, D)),
                 cx=cp.zeros((PN, D)), cy=cp.zeros((PN, D)), cz=cp.zeros((PN, D)), vol=PDX ** D)
    particle.v[:, 0] = -0.5
    eye = np.eye(3, dtype=np.int64)

    def comp(a, bias):
        shape = tuple(np.array(gres) + eye[a])
        return N(resolution=cp.array(np.array(gres) + eye[a]), bias=cp.array(bias, dtype=cp.float32),
                 m=cp.zeros(shape, dtype=cp.float32), v=cp.zeros(shape, dtype=cp.float32), dv=cp.zeros(shape, dtype=cp.float32))
    grid = N(resolution=GRES, bound_size=BOUND_SIZE, bound_min=BOUND_MIN, cell_size=BOUND_SIZE / GRES,
             x=comp(0, [0, .5, .5]), y=comp(1, [.5, 0, .5]), z=comp(2, [.5, .5, 0]))
    SOL = 2 * GRES + 1
    dres = tuple(2 * np.array(gres) + 1)
    solid = N(resolution=SOL, bound_size=BOUND_SIZE, bound_min=BOUND_MIN, cell_size=BOUND_SIZE / (2 * GRES),
              bias=cp.array([0, 0, 0], dtype=cp.float32), phi=cp.zeros(dres), pos=cp.zeros(dres + (D,)), v=cp.zeros(dres + (D,)))
    ga = [cp.arange(r) for r in dres]
    gidx = cp.stack(cp.meshgrid(*ga, indexing='ij'), axis=-1).astype(cp.float32)
    solid.pos[:] = solid.bound_min + ((gidx + solid.bias) * solid.cell_size)       # get_grid_pos (code cell 9)
    sdf.evaluate(rb_d, solid.phi, solid.v, solid.pos)
    fl = N(resolution=GRES, bound_size=BOUND_SIZE, bound_min=BOUND_MIN, cell_size=BOUND_SIZE / GRES, phi=cp.zeros(gres))
    fv = N(resolution=SOL, bound_size=BOUND_SIZE, bound_min=BOUND_MIN, cell_size=BOUND_SIZE / (2 * GRES), vol=cp.zeros(dres))
    CGBuf = CGSolverBuffer(GRES)
    PressureSolver = PressureCGSolver3D(CGBuf, GRES, GDX)
    DensitySolver = DensityCGSolver3D(CGBuf, GRES, BOUND_MIN, BOUND_SIZE)
    ViscositySolver = ViscosityCGSolver3D(GRES, BOUND_SIZE)
    out = dict(kind="timestep_moving", gres=np.array(gres), gdx=GDX, pdx=PDX, rho=RHO, mu=MU, dt=DT, rb_d=np.asarray(rb_d).copy(),
               px0=np.array(PX), pv0=np.asarray(particle.v).copy(), sphi0=np.asarray(solid.phi).copy(), steps=steps,
               ball=ball, ball_v=vel)
    dts, moved_by_sphere = [], []
    cuda.ignore_oob = True                 # boundary_condition_* kernels store before their bounds check
    try:
        with np.errstate(all="ignore"):
            for s in range(steps):         # the loop body, ipynb:4571-4667 (solver == 'apic'), with the body's move
                cfl_dt = GDX / max(1e-10, cp.max(cp.sum(particle.v ** 2, axis=-1) ** 0.5).item())
                current_dt = min(DT, cfl_dt, 3.0)
                dts.append(current_dt)
                particle.x += particle.v * current_dt
                centre = centre + vel * current_dt
                sdf.transform_rb(rb_d, ball, center=[float(c) for c in centre])
                sdf.set_vel_rb(rb_d, ball, cp.array(vel))
                sdf.evaluate(rb_d, solid.phi, solid.v, solid.pos)
                before = np.asarray(particle.x).copy()
                sdf.project(rb_d[:ball], particle.x)                       # what the static bodies alone would move ...
                static_only = np.asarray(particle.x).copy()
                particle.x[:] = cp.array(before)
                sdf.project(rb_d, particle.x)                              # ... and the step's projection, sphere included
                moved = int((np.abs(np.asarray(particle.x) - static_only).max(axis=1) > 0).sum())
                # the first projection resolves the initial overlap (at least 50 particles); later ones move the
                # particles the sphere has caught up with since
                assert moved >= (50 if s == 0 else 1), f"step {s + 1}: project moves only {moved} particles because of the sphere"
                moved_by_sphere.append(moved)
                ns["compute_fluid_levelset"](particle, fl, GDX)
                ns["compute_fluid_volume"](particle, fv, particle.vol)
                DensitySolver.solve(RHO, current_dt, particle.x, particle.m, particle.vol, grid.x.v, grid.y.v, grid.z.v,
                                    solid.phi, solid.v, fl.phi, fv.vol)
                ns["compute_fluid_levelset"](particle, fl, GDX)
                ns["compute_fluid_volume"](particle, fv, particle.vol)
                for c in (grid.x, grid.y, grid.z):
                    c.m *= 0
                    c.v *= 0
                ns["p2g"](particle, grid)
                grid.y.v += -10 * current_dt
                if MU > 0:
                    ViscositySolver.solve(current_dt, MU, RHO, grid.x.v, grid.y.v, grid.z.v, solid.phi, solid.v, fl.phi, fv.vol)
                PressureSolver.solve(grid.x.v, grid.y.v, grid.z.v, solid.phi, solid.v, fl.phi, wx=DensitySolver.wx,
                                     wy=DensitySolver.wy, wz=DensitySolver.wz)
                ns["extrapolate"](GRES, 2, grid.x.v, grid.y.v, grid.z.v, grid.x.m, grid.y.m, grid.z.m)
                ns["apply_boundary_condition"](grid, solid, GDX)
                ns["g2p"](particle, grid)
                # the sphere's velocity reaches the solves: sv != 0 at cell-centre nodes of the doubled grid inside the fluid
                sv_c = np.asarray(solid.v)[1::2, 1::2, 1::2]
                wet = int(((np.asarray(fl.phi) < 0) & (np.abs(sv_c).max(axis=-1) > 0)).sum())
                assert wet > 0, f"step {s + 1}: sv is zero on every node where lphi < 0"
                out[f"px{s + 1}"] = np.asarray(particle.x).copy()
                out[f"pv{s + 1}"] = np.asarray(particle.v).copy()
                out[f"lphi{s + 1}"] = np.asarray(fl.phi).copy()
                out[f"gvy{s + 1}"] = np.asarray(grid.y.v).copy()
                out[f"sphi{s + 1}"] = np.asarray(solid.phi).copy()
                print(f"  {name}: step {s + 1} dt={current_dt:.5f} |v|max={np.abs(np.asarray(particle.v)).max():.4f} "
                      f"fluid cells={(np.asarray(fl.phi) < 0).sum()} moved by the sphere={moved} wet sv nodes={wet}", flush=True)
    finally:
        cuda.ignore_oob = False
    out["dts"] = np.array(dts)
    out["moved_by_sphere"] = np.array(moved_by_sphere)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print(f"  {name}: gres={gres} particles={PN} steps={steps}")


if __name__ == "__main__":
    gen("step_moving_12x16x12", (12, 16, 12), 3, 51, mu=50.0)
