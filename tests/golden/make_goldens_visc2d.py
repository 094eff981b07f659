#!/usr/bin/env python3
"""Generate tests/golden/v2d_*.npz by EXECUTING THE REFERENCE'S OWN SOURCE (container only).

Same method as make_goldens.py: tests/golden/refshim/ (numpy as the array container, a sequential
per-thread launcher) ahead of the reference on sys.path, then the reference's
`solver.ViscosityCGSolver2D` imported UNMODIFIED; its module functions and its class are called as they
are.  Every arithmetic statement that produces a fixture is the reference's.

Per case the fixture holds the inputs (mfs.scenes.viscosity_scene_2d), `bx, by` from initialize_solver and
`qx, qy` from matvecmul(v) -- both into arrays prefilled with 7.0, so the faces the reference never writes are
pinned --, the residual history [delta0, dq1, delta1, ...] (cp.sum pairs summed, as the reference adds them), the
iteration count, the solver's x_x / x_y and the output velocities.

Needs the reference; never runs on the GPU box.

Usage:  python tests/golden/make_goldens_visc2d.py [case-prefix ...]
"""
import os
import sys
import time

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

import solver.ViscosityCGSolver2D as RV2    # noqa: E402  (reference module)

assert RV2.__file__.startswith(REF), RV2.__file__


class _SumLogger:
    """Proxy for the reference module's global `cp`: logs every cp.sum() result
    (2D viscosity log = [rx, ry (delta0), dqx, dqy, rx, ry, ...])."""

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


def gen_viscosity2d(name, gres, seed, vel_dtype, mu, tol=1e-4, dt=1.0 / 300.0):
    sc = scenes.viscosity_scene_2d(gres, seed, vel_dtype=vel_dtype, mu=mu, dt=dt)
    g = C(gres, np.int64)
    bsz = C(sc["bound_size"], np.float64)
    sphi, sv, lvol = C(sc["sphi"]), C(sc["sv"]), C(sc["lvol"])
    fx, fy = (gres[0] + 1, gres[1]), (gres[0], gres[1] + 1)

    # module functions on fp64 copies of the velocities (as solve() calls them), outputs prefilled with 7.0
    cell_vol = float(np.prod(np.array(sc["bound_size"]) / np.array(gres)))
    scale = sc["dt"] / cell_vol / sc["rho"]
    vol = cp.array(sc["lvol"] / (cell_vol * 0.125))
    ex, ey = C(sc["vx"], np.float64), C(sc["vy"], np.float64)
    bx, by = cp.array(np.full(fx, 7.0)), cp.array(np.full(fy, 7.0))
    RV2.initialize_solver(g, scale, sc["mu"], ex, ey, sphi, sv, vol, bx, by)
    qx, qy = cp.array(np.full(fx, 7.0)), cp.array(np.full(fy, 7.0))
    RV2.matvecmul(g, scale, sc["mu"], ex, ey, qx, qy, sphi, vol)

    slv = RV2.ViscosityCGSolver2D(g, bsz)
    vx, vy = C(sc["vx"]), C(sc["vy"])
    logger = _SumLogger(cp)
    RV2.cp = logger
    t0 = time.time()
    try:
        slv.solve(sc["dt"], sc["mu"], sc["rho"], vx, vy, sphi, sv, None, lvol, tol=tol)
    finally:
        RV2.cp = cp
    log = np.array(logger.log).reshape(-1, 2).sum(axis=1)   # pairs -> scalars, as the reference adds them
    iters = (len(log) - 1) // 2
    print(f"  {name}: gres={gres} mu={sc['mu']} iters={iters} delta0={log[0]:.4e} delta_end={log[-1]:.4e}"
          f" ({time.time() - t0:.1f}s)")
    np.savez_compressed(
        os.path.join(HERE, name + ".npz"),
        kind="viscosity2d", gres=np.array(gres), bound_size=np.array(sc["bound_size"]), tol=tol,
        seed=seed, dt=sc["dt"], mu=sc["mu"], rho=sc["rho"],
        in_vx=sc["vx"], in_vy=sc["vy"], sphi=sc["sphi"], lvol=sc["lvol"],
        bx=np.asarray(bx), by=np.asarray(by), qx=np.asarray(qx), qy=np.asarray(qy),
        history=log, iters=iters,
        x_x=np.asarray(slv.x_x), x_y=np.asarray(slv.x_y),
        out_vx=np.asarray(vx), out_vy=np.asarray(vy))


CASES = [
    ("v2d_a_64", lambda n: gen_viscosity2d(n, (64, 64), 21, np.float64, 50.0)),
    ("v2d_b_24x40", lambda n: gen_viscosity2d(n, (24, 40), 22, np.float32, 1.0)),
    ("v2d_c_33x17_mu200", lambda n: gen_viscosity2d(n, (33, 17), 23, np.float64, 200.0, dt=0.1)),
]

if __name__ == "__main__":
    want = sys.argv[1:]
    for cname, fn in CASES:
        if want and not any(cname.startswith(w) for w in want):
            continue
        fn(cname)
