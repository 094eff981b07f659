#!/usr/bin/env python3
"""Generate tests/golden/sdf_*.npz by EXECUTING THE REFERENCE'S OWN solver/sdf3D.py
(container only, tests/golden/refshim plumbing): a notebook-like scene -- a flipped container box, slanted
obstacle boxes (ipynb code cell 9), plus spheres -- built with the reference's generate_rb / set_vel_rb, then
its evaluate() and project() on random points in and around the bodies.

tests/golden/sdfcyl_*.npz hold the cylinder scenes.  The reference's cylinder_eval reads an unassigned variable for points
within a cylinder's height range (sdf3D.py:148-160), so `position_eval` keeps only points that lie outside the height range
of EVERY cylinder of the scene (computed here from the body frames, with a margin of 1e-9), plus points placed above and
below every cap, inside and outside the radius.  cylinder_project runs at any point: `position_project` (float64) and
`position_project_f32` are unrestricted.  Keys: rb_d, position_eval, sd, vel, position_project, projected,
position_project_f32, projected_f32.

Usage: make_goldens_sdf.py [name prefix ...] (default: every fixture).  Needs /root/reference."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MFS_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, "refshim"))

import numpy as np  # noqa: E402
import cupy as cp   # noqa: E402  (refshim)

import solver.sdf3D as RS  # noqa: E402  (reference module)

assert RS.__file__.startswith(REF)


def scene(kind):
    if kind == "notebook":   # the five boxes of ipynb code cell 9
        h = 0.45
        return [("cube", ['box', 0.5, 0.8, 0.5], True, [0, 0.5, 0], [0, 1, 0], 0),
                ("cube1", ['box', 0.67, 0.1, 1.0], False, [-0.34, h, 0], [0, 0, 1], -45),
                ("cube2", ['box', 0.67, 0.1, 1.0], False, [0.34, h, 0], [0, 0, 1], 45),
                ("cube3", ['box', 1.0, 0.1, 0.7], False, [0, h, -0.3], [1, 0, 0], 45),
                ("cube4", ['box', 1.0, 0.1, 0.7], False, [0, h, 0.3], [1, 0, 0], -45)]
    return [("dome", ['sphere', 0.45], True, [0.02, 0.5, -0.01], [0, 1, 0], 0),
            ("ball", ['sphere', 0.12], False, [0.1, 0.4, 0.05], [0, 1, 0], 0),
            ("slab", ['box', 0.3, 0.06, 0.25], False, [-0.1, 0.6, 0.0], [1, 2, 0.5], 30)]


def gen(name, kind, seed, n=3000, dtype=np.float64):
    rb_d, rb_map = cp.zeros((0, 10, 4)), {}
    for nm, par, flip, c, ax, ang in scene(kind):
        rb_d, rb_map = RS.generate_rb(rb_d, rb_map, nm, par, flip=flip, center=c, axis=np.array(ax, dtype=np.float64),
                                      angle=ang)
    RS.set_vel_rb(rb_d, 1, cp.array([0.3, -0.2, 0.1]))
    rng = np.random.default_rng(seed)
    pos = rng.uniform([-0.4, -0.05, -0.4], [0.4, 1.05, 0.4], size=(n, 3)).astype(dtype)
    sd, vel = cp.zeros(n), cp.zeros((n, 3))
    RS.evaluate(rb_d, sd, vel, cp.array(pos))
    proj = cp.array(pos)
    RS.project(rb_d, proj)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), kind="sdf3d", rb_d=np.asarray(rb_d), position=pos,
                        sd=np.asarray(sd), vel=np.asarray(vel), projected=np.asarray(proj))
    moved = int((np.abs(np.asarray(proj) - pos).max(axis=1) > 1e-12).sum())
    print(f"  {name}: bodies={rb_d.shape[0]} points={n} inside-solid={(np.asarray(sd) <= 0).sum()} moved={moved}")


def cyl_scene(kind):
    """(name, parameters, flip, centre, axis, angle, velocity) per body, and the box the random points are drawn from"""
    if kind == "container":   # (i) a flipped container cylinder, a tilted solid cylinder and a sphere inside it
        return [("tank", ['cylinder', 0.4, 0.9], True, [0, 0.5, 0], [0, 1, 0], 0, [0.3, -0.2, 0.1]),
                ("peg", ['cylinder', 0.08, 0.3], False, [0.1, 0.45, 0.05], [1, 0, 1], 35, [-0.1, 0.25, 0.4]),
                ("ball", ['sphere', 0.1], False, [-0.12, 0.6, 0.0], [0, 1, 0], 0, [0.05, 0.6, -0.3])], ([-0.55, -0.3, -0.55], [0.55, 1.3, 0.55])
    if kind == "overlap":     # (ii) two overlapping solid cylinders and a solid box through both: a pushed-out point lands in the next
        return [("post", ['cylinder', 0.15, 0.4], False, [0, 0.5, 0], [0, 1, 0], 0, [0.2, 0.1, -0.4]),
                ("bar", ['cylinder', 0.12, 0.5], False, [0.1, 0.55, 0.05], [1, 2, 0.5], 50, [-0.3, 0.15, 0.2]),
                ("brick", ['box', 0.3, 0.2, 0.25], False, [0.05, 0.33, -0.05], [0, 1, 1], 20, [0.12, -0.5, 0.33])], ([-0.3, 0.1, -0.3], [0.4, 0.95, 0.35])
    # (iii) a flipped cylinder with radius < half height and a solid one with radius > half height: max(sd, y-hh, -(y+hh)) is won differently
    return [("pipe", ['cylinder', 0.2, 1.0], True, [0, 0.5, 0], [1, 0, 0.3], 12, [0.07, 0.3, -0.2]),
            ("disc", ['cylinder', 0.15, 0.1], False, [0.02, 0.5, 0.01], [1, 0, 0], 25, [-0.4, 0.02, 0.09])], ([-0.35, -0.2, -0.35], [0.35, 1.2, 0.35])


def cyl_heights(rb_d, pos):
    """(cylinders, points): |height of the point in the cylinder's frame| - half height, from R^T (x - T)"""
    out = []
    for rb in rb_d:
        if rb[0, 0] // 2 == 2:
            y = (pos - rb[1:4, 3]) @ rb[5:8, 1]
            out.append(np.abs(y) - rb[0, 2] / 2)
    return np.array(out)


def cap_points(rb_d, rng, per=40):
    """points above and below every cap, inside and outside the radius (body frame -> world)"""
    out = []
    for rb in rb_d:
        if rb[0, 0] // 2 != 2:
            continue
        r, hh = rb[0, 1], rb[0, 2] / 2
        for side in (1.0, -1.0):
            for lo, hi in ((0.05, 0.95), (1.05, 2.0)):
                rho, th = rng.uniform(lo, hi, per) * r, rng.uniform(0, 2 * np.pi, per)
                body = np.stack([rho * np.cos(th), side * (hh + rng.uniform(0.01, 0.5, per)), rho * np.sin(th)], axis=1)
                out.append(body @ rb[5:8, :3].T + rb[1:4, 3])
    return np.concatenate(out)


def gen_cyl(name, kind, seed, n=3000, n32=1500):
    bodies, (lo, hi) = cyl_scene(kind)
    rb_d, rb_map = cp.zeros((0, 10, 4)), {}
    for nm, par, flip, c, ax, ang, v in bodies:
        rb_d, rb_map = RS.generate_rb(rb_d, rb_map, nm, par, flip=flip, center=c, axis=np.array(ax, dtype=np.float64), angle=ang)
    for i, b in enumerate(bodies):
        RS.set_vel_rb(rb_d, i, cp.array(b[-1]))
    rb = np.asarray(rb_d)
    rng = np.random.default_rng(seed)
    pos = rng.uniform(lo, hi, size=(n, 3))
    pos32 = rng.uniform(lo, hi, size=(n32, 3)).astype(np.float32)
    proj, proj32 = cp.array(pos), cp.array(pos32)
    RS.project(rb_d, proj)
    RS.project(rb_d, proj32)
    ev = np.concatenate([pos, cap_points(rb, rng)])
    ev = ev[(cyl_heights(rb, ev) > 1e-9).all(axis=0)]
    sd, vel = cp.zeros(len(ev)), cp.zeros((len(ev), 3))
    RS.evaluate(rb_d, sd, vel, cp.array(ev))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), kind="sdf3d_cyl", rb_d=rb, position_eval=ev, sd=np.asarray(sd),
                        vel=np.asarray(vel), position_project=pos, projected=np.asarray(proj), position_project_f32=pos32,
                        projected_f32=np.asarray(proj32))
    moved = int((np.abs(np.asarray(proj) - pos).max(axis=1) > 1e-12).sum())
    moved32 = int((np.asarray(proj32) != pos32).any(axis=1).sum())
    print(f"  {name}: bodies={rb.shape[0]} project points={n} moved={moved} (float32: {n32}, moved={moved32}) "
          f"evaluate points={len(ev)} sd<=0: {(np.asarray(sd) <= 0).sum()}")


FIXTURES = [(gen, "sdf_a_notebook", ("notebook", 41), {}), (gen, "sdf_b_spheres", ("mixed", 42), {}),
            (gen, "sdf_c_notebook_f32", ("notebook", 43), dict(n=1500, dtype=np.float32)),
            (gen_cyl, "sdfcyl_a_container", ("container", 51), {}), (gen_cyl, "sdfcyl_b_overlap", ("overlap", 52), {}),
            (gen_cyl, "sdfcyl_c_aspect", ("aspect", 53), {})]

if __name__ == "__main__":
    for fn, name, args, kw in FIXTURES:
        if len(sys.argv) == 1 or any(name.startswith(a) for a in sys.argv[1:]):
            fn(name, *args, **kw)
