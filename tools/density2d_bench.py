"""GPU: DensityCGSolver2D on an N x N density_scene_2d, PressureCGSolver2D on the same scene beside it -- one JSON line.

    python tools/density2d_bench.py N [fp32|fp64] [--check-every K] [--batches B] [--repeats R]

us_per_iteration            device events around engine solves of fixed length (tol 0), the difference of a 2-batch
                            and a (2 + B)-batch run divided by B * K iterations (begin cost and warm-up excluded).
                            A density solve also scatters, fixes the volume, builds b and gathers inside the timed
                            span; that constant part cancels in the difference but its jitter does not, so on small
                            grids B has to make the span long (--batches 64 at 256^2)
us_per_apply                device events around 200 stand-alone density applies (mfs_density_apply2d) q = A d
pressure2d_us_per_*         the same two figures for the pressure operator on the same lphi, wx, wy
*_spread                    every figure is measured R times; the value is the median, the spread (max - min) / median.
                            The density apply stands against the pressure apply within the pressure apply's own spread
scatter_ms / gather_ms      one mfs_density_splat2d / one mfs_density_advect2d at 4 particles per liquid cell
solve_ms, iterations        one tol-terminated solve (tol 1e-3, the reference's default), scatter and gathers included
"""
import argparse
import json
import os
import statistics
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


def med_spread(vals):
    m = statistics.median(vals)
    return round(m, 3), round((max(vals) - min(vals)) / m, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", type=int)
    ap.add_argument("precision", nargs="?", default="fp64")
    ap.add_argument("--check-every", type=int, default=32)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import solver.DensityCGSolver2D as D
    import solver.PressureCGSolver2D as P
    from solver.CGSolverBuffer import CGSolverBuffer
    dev = torch.device("cuda:0")
    gres = (a.N, a.N)
    ce, B, R = a.check_every, a.batches, a.repeats
    sc = scenes.density_scene_2d(gres, 1)
    t = lambda x: torch.as_tensor(x, device=dev)  # noqa: E731
    sphi, lphi, lvol, pm = t(sc["sphi"]), t(sc["lphi"]), t(sc["lvol"]), t(sc["pm"])
    sv = torch.zeros(tuple(sc["sphi"].shape) + (2,), dtype=torch.float64, device=dev)
    px0 = t(sc["px"])
    buf = CGSolverBuffer(gres, precision=a.precision, device=dev)
    d = D.DensityCGSolver2D(buf, gres, sc["bound_min"], sc["bound_size"], check_every=ce)
    p = P.PressureCGSolver2D(buf, gres, sc["bound_size"], check_every=ce)
    cs = d.cell_size

    def dsolve(n, tol):
        d.max_iter = n
        px = px0.clone()
        return events_ms(lambda: d.solve(sc["rho0"], sc["dt"], px, pm, sc["pvol"], None, None, sphi, sv, lphi, lvol,
                                         wx=d.wx, wy=d.wy, tol=tol))

    D.compute_solid_frac(gres, sphi, d.wx, d.wy)
    solve_ms = dsolve(a.N * a.N, 1e-3)
    iters, conv = d.iterations, d.converged
    solve_ms = dsolve(a.N * a.N, 1e-3)
    vx = torch.zeros((a.N + 1, a.N), dtype=torch.float64, device=dev)
    vy = torch.zeros((a.N, a.N + 1), dtype=torch.float64, device=dev)
    rng = torch.Generator(device=dev).manual_seed(1)

    def psolve(n):
        p.max_iter = n
        vx.normal_(generator=rng)
        vy.normal_(generator=rng)
        return events_ms(lambda: p.solve(vx, vy, sphi, sv, lphi, wx=d.wx, wy=d.wy, tol=0.0))

    def per_iter(fn):
        fn(2 * ce)
        out = []
        for _ in range(R):
            t1, t2 = fn(2 * ce), fn((2 + B) * ce)
            out.append((t2 - t1) * 1e3 / (B * ce))
        return out

    it_d = per_iter(lambda n: dsolve(n, 0.0))
    it_p = per_iter(psolve)

    v, q = buf.d, buf.q
    v.normal_(generator=rng)

    def per_apply(fn):
        for _ in range(10):
            fn()
        return [events_ms(lambda: [fn() for _ in range(200)]) * 1e3 / 200 for _ in range(R)]

    # interleaved: pressure, density, pressure, ... would hide drift; here each block is repeated R times back to back and
    # the pressure block is run before AND after the density block, so drift between blocks shows in the pressure spread
    ap_p1 = per_apply(lambda: P.matvecmul(gres, v, q, d.wx, d.wy, lphi))
    ap_d = per_apply(lambda: D.matvecmul(gres, v, q, d.wx, d.wy, lphi))
    ap_p2 = per_apply(lambda: P.matvecmul(gres, v, q, d.wx, d.wy, lphi))

    gm = torch.zeros(gres, dtype=buf.b.dtype, device=dev)
    px = px0.clone()
    sc_ms = [events_ms(lambda: D.initialize_density(sc["bound_min"], cs, gres, px, pm, sc["pvol"], gm, gm)) for _ in range(R + 1)][1:]
    ga_ms = [events_ms(lambda: D.apply_displacement(px, d.dx, sc["bound_min"], cs, (0, 0.5), 0)) for _ in range(R + 1)][1:]

    out = {"tool": "density2d_bench", "N": a.N, "precision": a.precision, "check_every": ce, "particles": int(px0.shape[0]),
           "iterations": iters, "converged": conv, "solve_ms": round(solve_ms, 3)}
    for k, vals in (("us_per_iteration", it_d), ("pressure2d_us_per_iteration", it_p), ("us_per_apply", ap_d),
                    ("pressure2d_us_per_apply", ap_p1 + ap_p2), ("scatter_ms", sc_ms), ("gather_ms", ga_ms)):
        out[k], out[k + "_spread"] = med_spread(vals)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
