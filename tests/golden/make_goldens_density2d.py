#!/usr/bin/env python3
"""Generate tests/golden/d2d_*.npz and sdf2d_*.npz by EXECUTING THE REFERENCE'S OWN SOURCE (container only).

Same method as make_goldens_visc2d.py: tests/golden/refshim/ (numpy as the array container, a sequential per-thread
launcher) ahead of the reference on sys.path, then the reference's `solver.DensityCGSolver2D` and `solver.sdf2D`
imported UNMODIFIED; their module functions and the class are called as they are.  Every arithmetic statement that
produces a fixture is the reference's.  sdf2D imports `scipy` and `matplotlib` and never uses them: where they are not
installed, empty stand-ins are supplied from here (the shim stays as it is).

d2d_* (inputs: mfs.scenes.density_scene_2d): `wx, wy` from compute_solid_frac, `gm` from the scatter (into zeros;
the volume array it is handed keeps its 7.0 prefill, asserted here), `gvol` / `b` from the module functions, `qr = A rv`
for a random `rv` and the displacements of the solved `x` -- these into arrays prefilled with 7.0, so the entries the
reference never writes are pinned --, then the class solve: the residual history
[delta0, dq1, delta1, ...] (every cp.sum the solve makes), the iteration count, `x`, `dx`, `dy`, the moved particles.
A case with `max_iter` set (assigned to `slv.max_iter`, as a caller could) pins that the 2D solve does not raise.
sdf2d_*: `rb_d` built by the reference's generate_rb / set_vel_rb, `sd`, `vel` from evaluate at scattered points (with
points exactly on a box face and at the sphere's centre), the positions after project.

Needs the reference; never runs on the GPU box.

Usage:  python tests/golden/make_goldens_density2d.py [case-prefix ...]
"""
import importlib.util
import os
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("MFS_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True          # the reference mount is read-only
sys.path.insert(0, os.path.join(REPO, "python-fluid-simulation_amd"))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.join(HERE, "refshim"))

import numpy as np  # noqa: E402
import cupy as cp   # noqa: E402  (tests/golden/refshim/cupy.py)

from mfs import scenes  # noqa: E402


def _stand_in(name, **attrs):
    """an empty module for an import the reference makes and never uses"""
    parts = name.split(".")
    for k in range(1, len(parts) + 1):
        sub = ".".join(parts[:k])
        if sub not in sys.modules and importlib.util.find_spec(parts[0]) is None:
            sys.modules[sub] = types.ModuleType(sub)
            if k > 1:
                setattr(sys.modules[".".join(parts[:k - 1])], parts[k - 1], sys.modules[sub])
    mod = sys.modules.get(name)
    if mod is not None and isinstance(mod, types.ModuleType) and getattr(mod, "__file__", None) is None:
        for a, v in attrs.items():
            setattr(mod, a, v)


_stand_in("scipy.spatial.transform", Rotation=None)
_stand_in("matplotlib.pyplot")

import solver.DensityCGSolver2D as RD2    # noqa: E402  (reference module)
import solver.sdf2D as RS2                # noqa: E402  (reference module)
from solver.CGSolverBuffer import CGSolverBuffer as RBuf    # noqa: E402

assert RD2.__file__.startswith(REF) and RS2.__file__.startswith(REF), (RD2.__file__, RS2.__file__)


class _SumLogger:
    """Proxy for the reference module's global `cp`: logs every cp.sum() result (delta0, dq1, delta1, ...)."""

    def __init__(self, real):
        self._real = real
        self.log = []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def sum(self, a, *args, **kw):
        v = self._real.sum(a, *args, **kw)
        self.log.append(float(np.asarray(v)))
        return v


def C(a, dtype=None):
    return cp.array(np.array(a, dtype=dtype, copy=True))


def ref_bodies(bodies):
    """the scene's bodies through the reference's own generate_rb / set_vel_rb"""
    rb_d, rb_map = cp.zeros((0, 8, 3)), {}
    for i, b in enumerate(bodies):
        rb_d, rb_map = RS2.generate_rb(rb_d, rb_map, b["name"], b["rbparam"], flip=b["flip"], center=b["center"],
                                       angle=b["angle"])
        RS2.set_vel_rb(rb_d, i, b["vel"])
    return rb_d, rb_map


def gen_density2d(name, gres, seed, px_dtype, bound_size=(1.0, 1.0), tol=1e-3, max_iter=None):
    sc = scenes.density_scene_2d(gres, seed, px_dtype=px_dtype, bound_size=bound_size)
    rb_d, _ = ref_bodies(sc["bodies"])
    assert np.array_equal(np.asarray(rb_d), sc["rb_d"]), "mfs.scenes packs the bodies differently from generate_rb"
    g = C(gres, np.int64)
    bmin, bsz = C(sc["bound_min"], np.float64), C(sc["bound_size"], np.float64)
    cs = bsz / g
    sphi, sv, lphi, lvol = C(sc["sphi"]), C(sc["sv"]), C(sc["lphi"]), C(sc["lvol"])
    pm = C(sc["pm"])
    fx, fy = (gres[0] + 1, gres[1]), (gres[0], gres[1] + 1)
    full = lambda shape: cp.array(np.full(shape, 7.0))      # noqa: E731

    # the class solve first (its x feeds the displacement fixture)
    buf = RBuf(g)
    slv = RD2.DensityCGSolver2D(buf, g, bmin, bsz)
    if max_iter is not None:
        slv.max_iter = int(max_iter)
    px = C(sc["px"])
    logger = _SumLogger(cp)
    RD2.cp = logger
    t0 = time.time()
    try:
        slv.solve(sc["rho0"], sc["dt"], px, pm, sc["pvol"], None, None, sphi, sv, lphi, lvol, tol=tol)
    finally:
        RD2.cp = cp
    log = np.array(logger.log)
    iters = (len(log) - 1) // 2
    wx, wy = np.asarray(slv.wx).copy(), np.asarray(slv.wy).copy()

    # module functions, outputs prefilled with 7.0
    gm, gvol_raw = cp.zeros(gres), full(gres)
    RD2.initialize_density(bmin, cs, g, C(sc["px"]), pm, sc["pvol"], gm, gvol_raw, sphi, lphi)
    assert (np.asarray(gvol_raw) == 7.0).all()          # the volume scatter is commented out in the reference (:33)
    gvol = full(gres)
    RD2.fix_volume(cs, g, lvol, gvol, sphi, lphi, C(wx), C(wy))
    b = full(gres)
    RD2.initialize_solver(sc["rho0"], sc["dt"], g, cs, slv.m, slv.vol, lphi, C(wx), C(wy), b)
    rv = np.random.default_rng(seed + 77).standard_normal(gres)
    qr = full(gres)
    RD2.matvecmul(g, C(rv), qr, C(wx), C(wy), lphi)
    dx, dy = full(fx), full(fy)
    RD2.compute_displacement(g, sc["dt"], cs, dx, dy, slv.x, lphi)
    # the solve's own m / vol are the module functions' results (vol: interior cells; its boundary stays 0)
    assert np.array_equal(np.asarray(slv.m), np.asarray(gm))
    assert np.array_equal(np.asarray(slv.vol)[1:-1, 1:-1], np.asarray(gvol)[1:-1, 1:-1])

    print(f"  {name}: gres={gres} P={len(sc['px'])} iters={iters}/{slv.max_iter} delta0={log[0]:.4e} "
          f"delta_end={log[-1]:.4e} ({time.time() - t0:.1f}s)")
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"),
        kind="density2d", gres=np.array(gres), bound_min=np.array(sc["bound_min"]), bound_size=np.array(sc["bound_size"]),
        tol=tol, seed=seed, dt=sc["dt"], rho0=sc["rho0"], pvol=sc["pvol"], max_iter=int(slv.max_iter),
        px=sc["px"], pm=sc["pm"], sphi=sc["sphi"], lphi=sc["lphi"], lvol=sc["lvol"], rb_d=sc["rb_d"],
        wx=wx, wy=wy, gm=np.asarray(gm), gvol=np.asarray(gvol), b=np.asarray(b),
        rv=rv, qr=np.asarray(qr), history=log, iters=iters,
        x=np.asarray(slv.x),
        dx=np.asarray(dx), dy=np.asarray(dy), out_px=np.asarray(px))


def gen_sdf2d(name, gres, seed, pos_dtype, n=3000):
    sc = scenes.density_scene_2d(gres, seed)
    rb_d, rb_map = ref_bodies(sc["bodies"])
    rng = np.random.default_rng(seed + 500)
    bmin, bsz = np.array(sc["bound_min"]), np.array(sc["bound_size"])
    pos = rng.uniform(bmin - 0.05 * bsz, bmin + 1.05 * bsz, size=(n, 2))
    tank, bar, ball = sc["bodies"]
    # exactly on faces of the axis-aligned container, at the sphere's centre, within 1e-4 of it, on the sphere
    half = np.array(tank["rbparam"][1:]) / 2
    c = np.array(tank["center"])
    pos[0] = (c[0] + half[0], c[1] + 0.1 * half[1])
    pos[1] = (c[0] - half[0], c[1])
    pos[2] = (c[0] + 0.3 * half[0], c[1] - half[1])
    pos[3] = c + half
    pos[4] = ball["center"]
    pos[5] = (ball["center"][0] + 5e-5, ball["center"][1])
    pos[6] = (ball["center"][0], ball["center"][1] + ball["rbparam"][1])
    pos[7] = bar["center"]
    pos = pos.astype(pos_dtype)
    sd, vel = cp.array(np.full(n, 7.0)), cp.array(np.full((n, 2), 7.0))
    RS2.evaluate(rb_d, sd, vel, C(pos))
    proj = C(pos)
    RS2.project(rb_d, proj)
    moved = int((np.asarray(proj) != pos).any(axis=1).sum())
    print(f"  {name}: bodies={rb_map} n={n} inside={int((np.asarray(sd) <= 0).sum())} moved={moved}")
    np.savez_compressed(os.path.join(HERE, name + ".npz"), kind="sdf2d", gres=np.array(gres), seed=seed,
                        rb_d=np.asarray(rb_d), position=pos, sd=np.asarray(sd), vel=np.asarray(vel),
                        projected=np.asarray(proj))


CASES = [
    ("d2d_a_44", lambda n: gen_density2d(n, (44, 44), 31, np.float64)),
    ("d2d_b_40x28_f32", lambda n: gen_density2d(n, (40, 28), 32, np.float32, bound_size=(1.0, 0.8))),
    ("d2d_c_33x21_maxiter6", lambda n: gen_density2d(n, (33, 21), 33, np.float64, bound_size=(1.2, 0.7), max_iter=6)),
    ("sdf2d_a_f64", lambda n: gen_sdf2d(n, (32, 32), 41, np.float64)),
    ("sdf2d_b_f32", lambda n: gen_sdf2d(n, (24, 40), 42, np.float32)),
]

if __name__ == "__main__":
    want = sys.argv[1:]
    for cname, fn in CASES:
        if want and not any(cname.startswith(w) for w in want):
            continue
        fn(cname)
