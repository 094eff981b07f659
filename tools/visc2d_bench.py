"""GPU: ViscosityCGSolver2D on an N x N viscosity_scene_2d -- one JSON line.

    python tools/visc2d_bench.py N [fp32|fp64] [--mu MU] [--check-every K] [--batches B] [--pressure]

us_per_iteration   device events around engine solves of fixed length (tol 0), the difference of a 2-batch and a
                   (2 + B)-batch run divided by B * K iterations: whole check_every batches, begin cost and warm-up
                   excluded
us_per_apply       device events around 200 engine applies q = A d
apply_bytes        algorithmic bytes of one apply: cells * (4 s + 32) + 4 * cells of class words, cells = (N+1)^2
                   (v read, q written, the four fp64 vol samples of a cell, its class word; s = state element size)
apply_frac_8TBs    apply_bytes / us_per_apply as a share of 8 TB/s
iterations         of one tol-terminated solve (tol 1e-4, the reference's default)
--pressure adds PressureCGSolver2D's us per iteration on pressure_scene_2d of the same size (same difference method).
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), REPO]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mfs import scenes  # noqa: E402


def events_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int)
    ap.add_argument("precision", nargs="?", default="fp64")
    ap.add_argument("--mu", type=float, default=1.0)
    ap.add_argument("--check-every", type=int, default=32)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--pressure", action="store_true")
    a = ap.parse_args()
    from solver.ViscosityCGSolver2D import ViscosityCGSolver2D
    dev = torch.device("cuda:0")
    gres = (a.N, a.N)
    ce, B = a.check_every, a.batches
    sc = scenes.viscosity_scene_2d(gres, 1, mu=a.mu)
    t = lambda x: torch.as_tensor(x, device=dev)  # noqa: E731
    sphi, lvol, vx_in, vy_in = t(sc["sphi"]), t(sc["lvol"]), t(sc["vx"]), t(sc["vy"])
    del sc["sv"]
    s = ViscosityCGSolver2D(gres, sc["bound_size"], precision=a.precision, device=dev, check_every=ce)

    vx, vy = vx_in.clone(), vy_in.clone()
    torch.cuda.synchronize()
    try:
        s.solve(sc["dt"], sc["mu"], sc["rho"], vx, vy, sphi, None, None, lvol)
        iters, conv = s.iterations, True
    except ValueError:
        iters, conv = s.iterations, False

    eng, f = s._engine, s._flat

    def fixed(n):
        s.x_x.copy_(vx_in)
        s.x_y.copy_(vy_in)
        return events_ms(lambda: eng.solve(0.0, n, ce))

    fixed(2 * ce)                                     # warm-up
    t1 = min(fixed(2 * ce) for _ in range(2))
    t2 = min(fixed((2 + B) * ce) for _ in range(2))
    us_iter = (t2 - t1) * 1e3 / (B * ce)

    for _ in range(10):
        eng.apply(f["d"], f["q"])
    us_apply = min(events_ms(lambda: [eng.apply(f["d"], f["q"]) for _ in range(200)]) for _ in range(3)) * 1e3 / 200
    cells = (a.N + 1) ** 2
    es = 4 if s.precision == torch.float32 else 8
    nbytes = cells * (4 * es + 32) + 4 * cells
    out = {"tool": "visc2d_bench", "N": a.N, "precision": a.precision, "mu": a.mu, "check_every": ce,
           "us_per_iteration": round(us_iter, 3), "us_per_apply": round(us_apply, 3), "apply_bytes": nbytes,
           "apply_frac_8TBs": round(nbytes / (us_apply * 1e-6) / 8e12, 3), "iterations": iters, "converged": conv}

    if a.pressure:
        import solver.CGSolverBuffer as CB
        from solver.PressureCGSolver2D import PressureCGSolver2D
        ps = scenes.pressure_scene_2d(gres, 1)
        buf = CB.CGSolverBuffer(gres, precision=a.precision, device=dev)
        p = PressureCGSolver2D(buf, gres, ps["bound_size"], check_every=ce)
        args = [t(ps[k]) for k in ("sphi", "sv", "lphi")]
        pvx, pvy = t(ps["vx"]), t(ps["vy"])

        def pfixed(n):
            p.max_iter = n
            return events_ms(lambda: p.solve(pvx.clone(), pvy.clone(), *args, tol=0.0))

        pfixed(2 * ce)
        p1 = min(pfixed(2 * ce) for _ in range(2))
        p2 = min(pfixed((2 + B) * ce) for _ in range(2))
        out["pressure2d_us_per_iteration"] = round((p2 - p1) * 1e3 / (B * ce), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
