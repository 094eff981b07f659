#!/usr/bin/env python3
"""bench.py -- PressureCGSolver3D conjugate-gradient throughput on MI355X.

A "step" is ONE CG iteration of the pressure solve (stencil apply + 2 dot
products + the x/r/d updates: the loop solver/PressureCGSolver3D.py:207-221 of
the reference) on a synthetic 256^3-per-GPU grid with fp32 state, inputs already
resident in HBM.  value = cells x iterations / second over all GPUs (Mcells/s).

N GPUs: one process per GPU (torch.distributed, RCCL), the grid sharded into
x-slabs with a one-plane halo exchange of `d` and two scalar all-reduces per
iteration (weak scaling: 256^3 cells per GPU; 8 GPUs = 512^3, BASELINE config 4).

Prints ONE JSON line on rank 0.

A plain run (`--gpus N --steps K --warmup W`) sets up, warms up, times one block of exactly K steps, writes its outputs if
`--dump-outputs DIR` is given and prints the line (metric, value, unit, higher_is_better, dtype, ms_per_step, ...).
Everything beyond the headline -- the roofline and per-kernel legs, the parity self-checks against the C oracle, the
fp64 / config 2-5 / Jacobi side legs, the CPU baseline, the other transport's time at N > 1 and the repeated timed
blocks of short runs -- runs with `--full` only.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(REPO, "python-fluid-simulation_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)

# global grid per world size: 256^3 cells per GPU, slabs along x (axis 0)
GRIDS = {1: (256, 256, 256), 2: (512, 256, 256), 4: (512, 512, 256), 8: (512, 512, 512)}

# --dump-outputs: cells written per CG vector when the slab holds more (3 vectors x 2^21 x 8 bytes = 48 MiB in fp64 state)
DUMP_SAMPLE = 1 << 21
DUMP_SEED = 20240


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--n", "--edge", dest="n", type=int, default=0, help="override: cubic grid edge per GPU (default 256)")
    ap.add_argument("--strong", action="store_true", help="strong scaling: the 256^3 grid is split over the ranks instead of 256^3 per rank")
    ap.add_argument("--local-grid", default="", help="1 GPU experiments: Nx,Ny,Nz of the grid (e.g. 66,512,512 = one rank's slab of the 8-GPU run)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "f64"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-numpy-leg", action="store_true", help="CPU baseline: skip the 2-iteration numpy sample")
    ap.add_argument("--no-f64-line", action="store_true", help="skip the fp64-state sub-measurement (default precision of the drop-in)")
    ap.add_argument("--timed-loop-only", action="store_true",
                    help="profiling runs (tools/pmc_bench.sh): warm-up + timed loop only -- no roofline legs, no parity self-check, "
                         "no fp64 line -- so that per-kernel counter averages belong to ONE configuration")
    ap.add_argument("--dense-coefficients", action="store_true", help="timed loop with compressed coefficient access off")
    ap.add_argument("--unfused", action="store_true", help="timed loop with the direction update as its own kernel")
    ap.add_argument("--force-phases", action="store_true",
                    help="1 GPU: run the phase-by-phase multi-GPU driver loop (1-rank RCCL group) to price its host overhead")
    ap.add_argument("--transport", default="auto", choices=["auto", "p2p", "rccl"],
                    help="N>1: how halo planes and dot products travel. p2p = xGMI stores from the solver's kernels into "
                         "HIP-IPC windows (csrc/mfs_pcg_slab.h); rccl = torch.distributed collectives per iteration; "
                         "auto = p2p if its self-test and a cross-check against rccl pass, else rccl")
    ap.add_argument("--force-rccl", action="store_true",
                    help="1 GPU: run the NATIVE collective slab loop (csrc/mfs_rccl.h: RCCL between the window loop's launches) on a "
                         "1-rank communicator to price its launches and host enqueue")
    ap.add_argument("--force-p2p", action="store_true",
                    help="1 GPU: run the peer-to-peer slab loop on a 1-rank window to price its launches")
    ap.add_argument("--b2b", action="store_true", help="also time back-to-back applies (cache-warm; not the CG number)")
    ap.add_argument("--cpu-iters", type=int, default=0, help="CG iterations of the CPU baseline sample (0 = auto)")
    ap.add_argument("--repeat", type=int, default=0,
                    help="timed blocks of exactly --steps iterations each (0 = auto: 1; with --full 9 when --steps < 100); "
                         "ms_per_step is their median, min / max are reported beside it")
    ap.add_argument("--no-side-legs", action="store_true", help="headline, roofline and parity only (skip config 2 / 3 / 4 / 5 legs)")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: roofline and per-kernel legs, parity self-checks, fp64 and side legs, "
                         "CPU baseline, the other transport (N > 1), repeated blocks of short runs.  Off: the timed steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last one left to the caller (x, r, d: a fixed seeded sample of "
                         f"{DUMP_SAMPLE} cells each on larger grids; the residual history) as DIR/<name>.npy")
    return ap.parse_args()


def dump_outputs(out_dir, torch, eng, fields, rank, world):
    """--dump-outputs: the CG vectors the timed loop hands back after its last step (the solution x, the residual r, the
    direction d; state precision, float32 or float64) and the residual history of the last timed block (float64), as
    DIR/<name>.npy -- DIR/<name>_rank<k>.npy per rank when N > 1.  A vector of more than DUMP_SAMPLE cells is written as
    the same DUMP_SAMPLE flat indices on every run (numpy default_rng(DUMP_SEED), sorted): at most 48 MiB in all."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    sfx = "" if world == 1 else f"_rank{rank}"
    n = fields["x"].numel()
    idx = None
    if n > DUMP_SAMPLE:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_SAMPLE, replace=False))
        idx = torch.from_numpy(idx).to(fields["x"].device)
    for name, t in fields.items():
        flat = t.reshape(-1)
        np.save(os.path.join(out_dir, f"{name}{sfx}.npy"), (flat if idx is None else flat[idx]).cpu().numpy())
    np.save(os.path.join(out_dir, f"history{sfx}.npy"), eng.history())


def cpu_baseline(args, gres, scene_seed):
    """The oracle (CPU restatement of the reference algorithm) timed on this box's
    host cores on a bounded sample of the same workload: a few CG iterations of
    the same 256^3 problem.  Reported beside the GPU number; not a target."""
    import numpy as np
    from mfs import scenes
    try:
        from oracle import cbaseline
    except Exception:
        cbaseline = None
    from oracle import mfs_oracle as O
    sc = scenes.pressure_scene_3d(gres, seed=scene_seed)
    Nx, Ny, Nz = gres
    wx, wy, wz = np.zeros((Nx + 1, Ny, Nz)), np.zeros((Nx, Ny + 1, Nz)), np.zeros((Nx, Ny, Nz + 1))
    O.compute_solid_frac3d(gres, sc["sphi"], wx, wy, wz)
    b = np.zeros(gres)
    O.pressure_rhs3d(sc["cell_size"], gres, sc["vx"], sc["vy"], sc["vz"], sc["sphi"], sc["sv"], sc["lphi"], b, wx, wy, wz)
    cells = Nx * Ny * Nz
    if cbaseline is not None and cbaseline.available():
        nthr = min(os.cpu_count() or 1, 16)          # the box's CPU share for one GPU
        iters = args.cpu_iters
        if not iters:                                # size the sample to ~15 s of CPU work
            t_probe, _ = cbaseline.time_cg(gres, b, sc["lphi"], wx, wy, wz, 5, nthr)
            iters = int(max(10, min(400, 15.0 / (t_probe / 5))))
        dt, cores = cbaseline.time_cg(gres, b, sc["lphi"], wx, wy, wz, iters, nthr)
        sample = (f"{iters} CG iterations of the same {Nx}x{Ny}x{Nz} problem, C/OpenMP restatement "
                  f"(oracle/mfs_oracle_c.c), fp64, {cores} threads")
    else:
        iters = args.cpu_iters or 4
        x, d, r, q = (np.zeros(gres) for _ in range(4))
        ap = lambda V, Q: O.pressure_apply3d(gres, V[0], Q[0], wx, wy, wz, sc["lphi"])  # noqa: E731
        t0 = time.perf_counter()
        O.cg(ap, b, x, d, r, q, 0.0, iters, raise_on_fail=False)
        dt = time.perf_counter() - t0
        cores = 1
        sample = f"{iters} CG iterations of the same {Nx}x{Ny}x{Nz} problem, numpy restatement (oracle/mfs_oracle.py), fp64"
    out = {"value": cells * iters / dt / 1e6, "unit": "Mcells/s", "cores": cores, "kind": "port",
           "sample": sample, "iters_per_s": iters / dt, "host_cpus": os.cpu_count()}
    if cores > 1 and not args.no_numpy_leg:
        # SURVEY.md 8(d) asks for both CPU legs: the numpy restatement too (vectorised, effectively one core), 2 iterations
        n_it = 2
        x, d, r, q = (np.zeros(gres) for _ in range(4))
        ap = lambda V, Q: O.pressure_apply3d(gres, V[0], Q[0], wx, wy, wz, sc["lphi"])  # noqa: E731
        t0 = time.perf_counter()
        O.cg(ap, b, x, d, r, q, 0.0, n_it, raise_on_fail=False)
        dtn = time.perf_counter() - t0
        out["numpy_port"] = {"value": cells * n_it / dtn / 1e6, "unit": "Mcells/s", "cores": 1, "iters_per_s": n_it / dtn,
                             "sample": f"{n_it} CG iterations of the same problem, numpy restatement (oracle/mfs_oracle.py), fp64"}
    return out


def build_problem(torch, dev, tdt, lgres, ggrid, seed, x_range):
    """the bench workload on this rank's slab: weights, RHS, level set, CG vectors (all resident in HBM)"""
    from mfs import scenes
    import solver.PressureCGSolver3D as P
    import solver.SolidFraction3D as S
    sc = scenes.pressure_scene_3d(ggrid, seed=seed, x_range=x_range, device=dev)
    wx = torch.zeros((lgres[0] + 1, lgres[1], lgres[2]), dtype=tdt, device=dev)
    wy = torch.zeros((lgres[0], lgres[1] + 1, lgres[2]), dtype=tdt, device=dev)
    wz = torch.zeros((lgres[0], lgres[1], lgres[2] + 1), dtype=tdt, device=dev)
    S.compute_solid_frac(lgres, sc["sphi"], wx, wy, wz)
    stag = int(os.environ.get("MFS_BENCH_STAGGER", "-1"))
    if stag >= 0:
        # A/B knob: the five CG vectors carved out of ONE allocation, vector k starting k * stag bytes past its natural
        # place (a multiple of 16 bytes) -- does the relative placement of the streams matter?  (profiles/r02_placement_ab.txt)
        n = lgres[0] * lgres[1] * lgres[2]
        esz = torch.empty(0, dtype=tdt).element_size()
        pad = (stag // esz) if stag else 0
        big = torch.zeros(5 * (n + 4 * pad) + 64, dtype=tdt, device=dev)
        b, x, d, r, q = (big[k * (n + pad): k * (n + pad) + n].view(lgres) for k in range(5))
    else:
        b, x, d, r, q = (torch.zeros(lgres, dtype=tdt, device=dev) for _ in range(5))
    P.initialize_solver(sc["cell_size"], lgres, sc["vx"], sc["vy"], sc["vz"], sc["sphi"], sc["sv"], sc["lphi"],
                        b, wx, wy, wz)
    lphi = sc["lphi"]
    del sc
    torch.cuda.empty_cache()
    return wx, wy, wz, lphi, (b, x, d, r, q)


def parity_check(args, torch, dev, tdt, lgres, seed, iters=10, x_tol=None):
    """default engine (as timed) vs oracle/mfs_oracle_c.c on the bench workload: residual history over the first
    `iters` iterations (fp32 state: north_star's 1e-5 rel; fp64 state: 1e-9) and x after finish()"""
    import numpy as np
    from mfs.pcg import PcgEngine
    from oracle import cbaseline
    tol = 1e-5 if tdt == torch.float32 else 1e-9
    wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, tdt, lgres, lgres, seed, None)
    eng = PcgEngine(lgres, tdt, dev)
    eng.setup(lphi, wx, wy, wz)
    eng.bind(b, x, d, r, q)
    eng.begin(0.0)
    eng.iterate(iters)
    eng.finish()
    torch.cuda.synchronize()
    h = eng.history()[: 2 * iters + 1]
    form = eng.loop_info()
    host = lambda t: t.double().cpu().numpy()  # noqa: E731
    # the oracle starts from the SAME stored RHS and weights (state-precision values), and computes in fp64
    ref = cbaseline.cg(lgres, host(b), host(lphi), host(wx), host(wy), host(wz), 0.0, iters, 2 * iters + 1)
    hr = ref["history"]
    dev_h = float(np.max(np.abs(h - hr) / np.abs(hr)))
    xr = ref["x"]
    dev_x = float(np.max(np.abs(host(x) - xr)) / np.max(np.abs(xr)))
    x_tol = tol if x_tol is None else x_tol        # (the field tolerance of the parity tests is 1e-4 of its maximum for fp32 state)
    ok = bool(len(h) == len(hr) == 2 * iters + 1 and dev_h < tol and dev_x < x_tol)
    out = {"checked": "default engine as timed: " + ", ".join(k for k, v in form.items() if v), "iterations": iters,
           "window": f"first {iters} CG iterations (the history is rounding-chaotic beyond a leading window: DESIGN.md section 3)",
           "history_max_rel_dev": dev_h, "x_max_dev_rel_to_max": dev_x, "tolerance": tol, "x_tolerance": x_tol, "ok": ok,
           "oracle": "oracle/mfs_oracle_c.c (C/OpenMP restatement, fp64), outside the timed region"}
    del eng, wx, wy, wz, lphi, b, x, d, r, q
    torch.cuda.empty_cache()
    if not ok:
        raise AssertionError(f"bench parity self-check failed: {out}")
    return out


def f64_leg(args, torch, dev, lgres, seed):
    """the same workload with fp64 solver state -- the drop-in's default precision"""
    from mfs.pcg import PcgEngine
    steps, warm = max(20, args.steps // 3), max(5, args.warmup // 3)
    wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, torch.float64, lgres, lgres, seed, None)
    eng = PcgEngine(lgres, torch.float64, dev)
    eng.setup(lphi, wx, wy, wz)
    eng.bind(b, x, d, r, q)
    eng.begin(0.0)
    eng.iterate(warm)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.iterate(steps)
    eng.finish()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = eng.poll()
    assert st["iterations"] == warm + steps and st["delta"] == st["delta"], st
    cells = lgres[0] * lgres[1] * lgres[2]
    pc = parity_check(args, torch, dev, torch.float64, lgres, seed)
    out = {"dtype": "f64", "steps": steps, "warmup": warm, "ms_per_step": round(dt / steps * 1e3, 5),
           "value": round(cells * steps / dt / 1e6, 1), "unit": "Mcells/s", "iters_per_s": round(steps / dt, 2),
           "cg_iteration_hbm_gbs": round(15 * cells * 8 / (dt / steps) / 1e9, 1), "parity_check": pc}
    del eng, wx, wy, wz, lphi, b, x, d, r, q
    torch.cuda.empty_cache()
    return out


def config2_leg(args, torch, dev, seed):
    """BASELINE config 2 as written: `PressureCGSolver3D` 128^3, fp32 state (Infinity-Cache resident: the headline's 256^3 is
    the same solver beyond the cache) -- time per CG iteration and the same 10-iteration oracle check"""
    from mfs.pcg import PcgEngine
    gres, tdt = (128, 128, 128), torch.float32
    wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, tdt, gres, gres, seed, None)
    eng = PcgEngine(gres, tdt, dev)
    eng.setup(lphi, wx, wy, wz)
    eng.bind(b, x, d, r, q)
    eng.begin(0.0)
    eng.iterate(50)
    torch.cuda.synchronize()
    n = 1000
    t0 = time.perf_counter()
    eng.iterate(n)
    eng.finish()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = eng.poll()
    assert st["iterations"] == n + 50 and st["delta"] == st["delta"], st
    pc = parity_check(args, torch, dev, tdt, gres, seed, x_tol=1e-4)     # history 1e-5 (north_star); field: the tests' 1e-4 of its maximum
    cells = gres[0] * gres[1] * gres[2]
    return {"workload": "PressureCGSolver3D 128x128x128 synthetic pool scene, fp32 state", "us_per_iteration": round(dt / n * 1e6, 2),
            "value": round(cells * n / dt / 1e6, 1), "unit": "Mcells/s", "iters_per_s": round(n / dt, 1),
            "loop": ", ".join(k for k, v in eng.loop_info().items() if v), "parity_check": pc}


def notebook_grid_leg(torch, dev):
    """the reference's OWN grid (3D_viscous_fluid_sim.ipynb: 48 x 80 x 48, the drop-in's default fp64 state): a launch-bound
    size, where the loop runs as one resident launch per batch (csrc/mfs_pcg_resident.h).  Time per CG iteration, and the
    first 10 iterations against the C oracle like every other leg."""
    from mfs.pcg import PcgEngine
    gres = (48, 80, 48)
    wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, torch.float64, gres, gres, 5, None)
    eng = PcgEngine(gres, torch.float64, dev)
    eng.setup(lphi, wx, wy, wz)
    eng.bind(b, x, d, r, q)
    eng.begin(0.0)
    eng.iterate(100)
    torch.cuda.synchronize()
    n = 2000
    t0 = time.perf_counter()
    eng.iterate(n)
    eng.finish()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = eng.poll()
    info = eng.loop_info()
    assert st["iterations"] == n + 100 and st["delta"] == st["delta"], st
    import argparse
    pc = parity_check(argparse.Namespace(), torch, dev, torch.float64, gres, 5)
    return {"grid": list(gres), "dtype": "f64", "loop": "resident" if info.get("resident") else "launch-per-phase",
            "us_per_iteration": round(dt / n * 1e6, 2), "iters_per_s": round(n / dt, 1), "parity_check": pc}


def viscosity_leg(torch, dev, n, steps, with_parity, precision="fp32", ev_over=0.0):
    """BASELINE config 3 (`ViscosityCGSolver3D`, buckling-like scene) on an n^3 grid (or the grid tuple `n`), state
    `precision`: time per CG iteration of the native loop; the operator apply (k_vcg_apply_march, csrc/mfs_vcg_march.h)
    bracketed by HIP events inside real iterations against its algorithmic bytes (13 scalars + 1 packed mask byte per cell,
    DESIGN.md section 4) -- with the default compressed class access AND with dense access; the census of the classes; and
    the first 10 iterations against the oracle's C restatement of the viscosity CG."""
    import numpy as np
    from mfs import scenes
    import solver.ViscosityCGSolver3D as V
    gres = (n, n, n) if isinstance(n, int) else tuple(n)
    esz = 4 if precision == "fp32" else 8
    sc = scenes.viscosity_scene_3d(gres, seed=3, device=dev)
    s = V.ViscosityCGSolver3D(gres, sc["bound_size"], precision=precision, device=dev)
    scale, mu = sc["dt"] / s.cell_vol / sc["rho"], sc["mu"]
    torch.div(sc["lvol"], s.cell_vol * 0.125, out=s.vol)

    def start():
        s.x_x.copy_(sc["vx"]); s.x_y.copy_(sc["vy"]); s.x_z.copy_(sc["vz"])
        V.extrapolate(gres, 3, s.x_x, s.x_y, s.x_z, sc["sphi"])
    start()
    V.initialize_solver(gres, scale, mu, s.x_x, s.x_y, s.x_z, sc["sphi"], sc["sv"], s.vol, s.b_x, s.b_y, s.b_z)
    e, f = s._engine, s._flat
    e.setup(scale, mu, sc["sphi"], s.vol)
    e.bind(f["b"], f["x"], f["d"], f["r"], f["q"])
    host = lambda t: t.double().cpu().numpy()  # noqa: E731
    info = e.loop_info()
    out = {"workload": "ViscosityCGSolver3D %s buckling-like scene, %s state" % ("x".join(map(str, gres)), precision),
           "apply_kernel": e.apply_kernel(),
           "loop": ("resident: one launch per batch (csrc/mfs_vcg_resident.h)" if info.get("resident") else
                    "fused" if info["fused"] else
                    "two launches (march | merged vector phases)" if info["merged_vector_phases"] else
                    "three launches (march | r update | direction + x update)")}
    if with_parity:
        from oracle import cbaseline
        iters, tol = 10, (1e-5 if precision == "fp32" else 1e-9)
        x0, b = host(f["x"]), host(f["b"])
        vol = s.vol.to(f["x"].dtype).double().cpu().numpy()          # the state precision's class samples: same values
        e.begin(0.0)
        e.iterate(iters)
        e.finish()
        torch.cuda.synchronize()
        h = e.history()[: 2 * iters + 1]
        ref = cbaseline.visc_cg(gres, scale, mu, b, x0, host(sc["sphi"]), vol, 0.0, iters, 2 * iters + 1)
        dev_h = float(np.max(np.abs(h - ref["history"]) / np.abs(ref["history"])))
        dev_x = float(np.max(np.abs(host(f["x"]) - ref["x"])) / np.max(np.abs(ref["x"])))
        ok = bool(len(h) == len(ref["history"]) == 2 * iters + 1 and dev_h < tol and dev_x < tol)
        out["parity_check"] = {"iterations": iters, "history_max_rel_dev": dev_h, "x_max_dev_rel_to_max": dev_x,
                               "tolerance": tol, "ok": ok, "oracle": "oracle/mfs_oracle_c.c (viscosity operator + CG loop, fp64)"}
        del ref, x0, b, vol
        if not ok:
            raise AssertionError(f"bench viscosity parity self-check failed: {out}")
        start()
    e.begin(0.0)
    e.iterate(10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e.iterate(steps)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    st = e.poll()
    assert st["iterations"] == 10 + steps and st["delta"] == st["delta"], st
    cells = gres[0] * gres[1] * gres[2]
    out.update({"us_per_iteration": round(dt / steps * 1e6, 2), "Mcells_per_s": round(cells * steps / dt / 1e6, 1)})
    if e.apply_kernel() == "march":
        out["class_census"] = e.class_census()
    sp = e.sparse_info()
    if sp["chunks"]:
        # the same loop with the solve's sparse lists off (same process): what they are worth on this scene
        e.set_sparse(False)
        e.begin(0.0)
        e.iterate(10)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        e.iterate(steps)
        torch.cuda.synchronize()
        out["sparse_lists"] = dict(sp, us_per_iteration_lists_off=round((time.perf_counter() - t1) / steps * 1e6, 2),
                                   note="live 32-unknown chunks for the r and d / x updates, busy (tile, plane) pairs for the loop's march "
                                        "launches; the `apply` legs below time the stand-alone launch, which visits every pair")
        e.set_sparse(True)
        e.begin(0.0)
        e.iterate(2)
    if cells >= 64 ** 3:
        # the apply launch inside real iterations (phase form of the same kernels: the events bracket one launch each)
        reps = 24
        ab = cells * (13 * esz + 1)

        def bracketed():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            for a, b_ in ev:
                a.record()
                e.phase_apply()
                b_.record()
                e.phase_reduce(0)
                e.phase_update_xr()
                e.phase_reduce(1)
                e.phase_update_d()
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b_) for a, b_ in ev)
            return ts[len(ts) // 2]

        def back_to_back():
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e.phase_apply()
            a.record()
            for _ in range(reps):
                e.phase_apply()
            b_.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b_) / reps

        def figures(label):
            ms, ms_b2b = bracketed(), back_to_back()
            return {"kernel": label, "algorithmic_bytes": ab, "kernel_ms": round(ms, 5), "kernel_ms_is": "median of %d bracketed launches" % reps,
                    "kernel_ms_minus_event_pair": round(ms - ev_over, 5),
                    "achieved": round(ab / (ms * 1e-3) / 1e9, 1), "frac": round(ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "unit": "GB/s",
                    "kernel_ms_back_to_back": round(ms_b2b, 5),
                    "frac_back_to_back": round(ab / (ms_b2b * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        tname = "float, 4" if precision == "fp32" else "double, 2"
        out["apply"] = figures("k_vcg_apply_march<%s, ..., COMP=true> (q = A d, three coupled components, d.q partials; class arrays "
                               "read only for z-vectors that are neither all air nor all bulk liquid)" % tname)
        out["apply"]["frac_is"] = ("EFFECTIVE rate on this scene (algorithmic bytes / kernel time / peak): with compressed class access "
                                   "the kernel moves fewer bytes than the algorithmic count; `apply_dense` is the scene-independent figure")
        e.set_compress(False)
        out["apply_dense"] = figures("k_vcg_apply_march<%s, ..., COMP=false> (every class array read in full)" % tname)
        e.set_compress(True)
    del s, e, f, sc
    torch.cuda.empty_cache()
    return out


def config4_rank_share_leg(args, torch, dev, seed, ev_over=0.0):
    """One rank's share of BASELINE config 4 (`PressureCGSolver3D` 512^3 on 8 GPUs): the slab of rank 3 of 8 -- 64 owned
    planes + 2 ghost planes of 512 x 512, fp32 state -- through the WINDOW slab loop on a 1-rank window (the launches, the
    edge / interior split and the in-launch all-reduce of the multi-GPU path, no peer).  This is the per-rank cost the
    >= 6x claim rests on; the first 10 iterations are checked against the C oracle on the same slab."""
    import numpy as np
    import torch.distributed as dist
    from mfs import dist as mdist
    from mfs.p2p import P2PWindow
    from mfs.pcg import PcgEngine
    from oracle import cbaseline
    tdt = torch.float32
    ggrid = GRIDS[8]
    lo, hi = mdist.SlabPartition(ggrid[0], 8, 3).local_range
    lgres = (hi - lo, ggrid[1], ggrid[2])
    own = not dist.is_initialized()
    if own:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29534")
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev, timeout=mdist.pg_timeout())
    out = {"workload": f"PressureCGSolver3D slab {lgres[0]}x{lgres[1]}x{lgres[2]} (planes {lo}..{hi} of the 512^3 pool scene: rank 3 of 8), fp32 state"}
    win = None
    try:
        wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, tdt, lgres, ggrid, seed, (lo, hi))
        eng = PcgEngine(lgres, tdt, dev)
        eng.setup(lphi, wx, wy, wz)
        eng.bind(b, x, d, r, q)
        part = mdist.SlabPartition(lgres[0], 1, 0)
        win = P2PWindow(dist, lgres[1] * lgres[2] * 4, dev)
        out["p2p_selftest"] = "ok" if win.ok else win.why
        cg = mdist.SlabCG(eng, part, d, dist, force_multi=True, window=win if win.ok else None)
        # parity first: 10 iterations through this very loop against the C oracle
        iters = 10
        cg.begin(0.0)
        cg.iterate(iters)
        cg.finish()
        torch.cuda.synchronize()
        out["transport"] = cg.mode
        h = eng.history()[: 2 * iters + 1]
        host = lambda t: t.double().cpu().numpy()  # noqa: E731
        ref = cbaseline.cg(lgres, host(b), host(lphi), host(wx), host(wy), host(wz), 0.0, iters, 2 * iters + 1)
        dev_h = float(np.max(np.abs(h - ref["history"]) / np.abs(ref["history"])))
        dev_x = float(np.max(np.abs(host(x) - ref["x"])) / np.max(np.abs(ref["x"])))
        ok = bool(len(h) == 2 * iters + 1 and dev_h < 1e-5 and dev_x < 1e-4)
        out["parity_check"] = {"iterations": iters, "history_max_rel_dev": dev_h, "x_max_dev_rel_to_max": dev_x, "tolerance": 1e-5,
                               "x_tolerance": 1e-4, "ok": ok, "oracle": "oracle/mfs_oracle_c.c on the same slab (ghost planes as boundary planes)"}
        del ref
        if not ok:
            raise AssertionError(f"config4_rank_share parity self-check failed: {out}")
        n = max(50, min(args.steps, 200))
        cg.begin(0.0)
        cg.iterate(10)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cg.iterate(n)
        t_enq = time.perf_counter() - t0
        cg.finish()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        cells = (lgres[0] - 2) * lgres[1] * lgres[2]           # owned planes
        out.update({"us_per_iteration": round(dt / n * 1e6, 2), "host_enqueue_us_per_iteration": round(t_enq / n * 1e6, 2),
                    "owned_Mcells_per_s": round(cells * n / dt / 1e6, 1), "iterations_timed": n,
                    "eight_ranks_at_this_rate_Mcells_per_s": round(8 * cells * n / dt / 1e6, 1),
                    "note": "1-rank window: every launch, the edge / interior split and the in-launch reductions of the multi-GPU "
                            "loop, no xGMI traffic -- an upper bound on what 8 ranks can reach, not a measurement of them"})
        del eng, cg, wx, wy, wz, lphi, b, x, d, r, q
    finally:
        if win is not None:
            win.close()
        if own:
            dist.destroy_process_group()
        torch.cuda.empty_cache()
    return out


def timestep_leg(torch, dev, N=128, steps=3):
    """BASELINE config 5's pipeline on ONE GPU at N^3 (tools/bench_timestep.py's scene: flipped container, four slanted plates,
    a fluid block of (N/2)^3 cells at 8 particles per cell, mu = 1, fp64 state): per-stage wall clock of whole time steps --
    and the pressure solve of the LAST step, inputs captured as it ran, first 10 iterations against the C oracle."""
    import numpy as np
    import notebook_sim as NSIM
    import solver.sdf3D as sdf
    import solver.PressureCGSolver3D as P
    from mfs.pcg import PcgEngine
    from oracle import cbaseline
    gdx = 1.0 / N
    rb_d, rb_map = sdf.generate_rb(None, {}, 'cube', ['box', 1 - 4 * gdx, 1 - 4 * gdx, 1 - 4 * gdx], flip=True, center=[0, 0.5, 0], device=dev)
    h = 0.35
    for nm, par, c, ax, ang in (("p1", ['box', 0.67, 0.05, 1.2], [-0.42, h, 0], [0, 0, 1], -45), ("p2", ['box', 0.67, 0.05, 1.2], [0.42, h, 0], [0, 0, 1], 45),
                                ("p3", ['box', 1.2, 0.05, 0.67], [0, h, -0.42], [1, 0, 0], 45), ("p4", ['box', 1.2, 0.05, 0.67], [0, h, 0.42], [1, 0, 0], -45)):
        rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, nm, par, flip=False, center=c, axis=ax, angle=ang)
    px = NSIM.add_box([0.0, 0.7, 0.0], [0.5, 0.5, 0.5], gdx / 2, np.random.default_rng(0))
    sim = NSIM.NotebookSimulation((N, N, N), gdx, [-0.5, 0.0, -0.5], rb_d, px, gdx / 2, mu=1.0, device=dev)
    sim.particle.v[:, 0] = -2.0
    sim.step()                                   # warm-up step (allocations, first launches)
    cap = {}
    solve0 = sim.PressureSolver.solve

    def spy(vx, vy, vz, sphi, sv, lphi, wx=None, wy=None, wz=None, **kw):
        cap.update(vx=vx.clone(), vy=vy.clone(), vz=vz.clone(), sphi=sphi, sv=sv, lphi=lphi.clone(), wx=wx.clone(), wy=wy.clone(), wz=wz.clone())
        return solve0(vx, vy, vz, sphi, sv, lphi, wx=wx, wy=wy, wz=wz, **kw)
    tim, its = {}, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        if k == steps - 1:
            sim.PressureSolver.solve = spy
        sim.step(timings=tim)
        its.append((sim.DensitySolver.iterations, sim.ViscositySolver.iterations, sim.PressureSolver.iterations))
    torch.cuda.synchronize()
    t_all = time.perf_counter() - t0
    out = {"workload": f"notebook time step {N}^3, {sim.particle.num_particles} particles, mu=1, fp64 state, 1 GPU", "steps": steps,
           "s_per_step": round(t_all / steps, 4), "stage_ms_per_step": {k: round(v / steps * 1e3, 2) for k, v in tim.items()},
           "cg_iterations(density,viscosity,pressure)": its}
    # the captured pressure solve against the C oracle
    g = (N, N, N)
    tdt = torch.float64
    b, x, d, r, q = (torch.zeros(g, dtype=tdt, device=dev) for _ in range(5))
    P.initialize_solver(sim.PressureSolver.cell_size, g, cap["vx"], cap["vy"], cap["vz"], cap["sphi"], cap["sv"], cap["lphi"], b, cap["wx"], cap["wy"], cap["wz"])
    eng = PcgEngine(g, tdt, dev)
    eng.setup(cap["lphi"], cap["wx"], cap["wy"], cap["wz"])
    eng.bind(b, x, d, r, q)
    iters = 10
    eng.begin(0.0)
    eng.iterate(iters)
    eng.finish()
    torch.cuda.synchronize()
    hh = eng.history()[: 2 * iters + 1]
    host = lambda t: t.double().cpu().numpy()  # noqa: E731
    ref = cbaseline.cg(g, host(b), host(cap["lphi"]), host(cap["wx"]), host(cap["wy"]), host(cap["wz"]), 0.0, iters, 2 * iters + 1)
    dev_h = float(np.max(np.abs(hh - ref["history"]) / np.abs(ref["history"])))
    dev_x = float(np.max(np.abs(host(x) - ref["x"])) / np.max(np.abs(ref["x"])))
    ok = bool(len(hh) == 2 * iters + 1 and dev_h < 1e-9 and dev_x < 1e-9)
    out["parity_check"] = {"what": "the pressure solve of the last timed step (inputs captured as it ran: post-viscosity velocities, the "
                                   "density solve's face weights), default engine, first 10 CG iterations", "iterations": iters,
                           "history_max_rel_dev": dev_h, "x_max_dev_rel_to_max": dev_x, "tolerance": 1e-9, "ok": ok,
                           "oracle": "oracle/mfs_oracle_c.c"}
    if not ok:
        raise AssertionError(f"timestep parity self-check failed: {out}")
    sim.PressureSolver.solve = solve0
    del sim, eng, cap, b, x, d, r, q
    torch.cuda.empty_cache()
    return out


def viscosity_jacobi_leg(torch, dev, n):
    """the OPT-IN Jacobi-preconditioned viscosity loop on BASELINE config 3's scene (fp32 state, the reference's default
    tol = 1e-3): iterations and time of a whole solve() against the reference's unpreconditioned CG"""
    from mfs import scenes
    import solver.ViscosityCGSolver3D as V
    gres = (n, n, n)
    sc = scenes.viscosity_scene_3d(gres, seed=3, device=dev)
    out = {"workload": f"ViscosityCGSolver3D {n}^3 buckling-like scene, fp32 state, tol 1e-3, mu {sc['mu']}"}
    for jac in (False, True):
        s = V.ViscosityCGSolver3D(gres, sc["bound_size"], precision="fp32", device=dev, jacobi=jac)
        for rep in range(2):          # first solve: allocations / first launches
            vx, vy, vz = sc["vx"].clone(), sc["vy"].clone(), sc["vz"].clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.solve(sc["dt"], sc["mu"], sc["rho"], vx, vy, vz, sc["sphi"], sc["sv"], sc["lphi"], sc["lvol"], tol=1e-3)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
        out["jacobi" if jac else "reference_cg"] = {"iterations": int(s.iterations), "solve_ms": round(ms, 2)}
        del s
    out["note"] = ("opt-in (jacobi=True / MFS_VISC_JACOBI=1), off by default: not the reference's residual history; stopped by the "
                   "same rule, its iterate is CLOSER to the exact solution than the reference's (tests/test_viscosity_jacobi_gpu.py)")
    torch.cuda.empty_cache()
    return out


def jacobi_leg(args, torch, dev, tdt, lgres, seed):
    """the OPT-IN Jacobi-preconditioned loop (north_star: "Jacobi-precondition fused"; NOT the reference's iteration) on the
    bench workload: time per iteration of the fused two-launch form, and what it buys -- iterations and time of a whole
    solve at the reference's default tol = 1e-3 against the reference's CG on the same engine."""
    from mfs.pcg import PcgEngine
    wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, tdt, lgres, lgres, seed, None)
    eng = PcgEngine(lgres, tdt, dev)
    eng.setup(lphi, wx, wy, wz)
    eng.bind(b, x, d, r, q)
    out = {}
    cap = lgres[0] * lgres[1] * lgres[2]
    for jac in (False, True):
        eng.set_jacobi(jac)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok, it = eng.solve(1e-3, cap, 32)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert ok, "the bench problem did not converge at tol 1e-3"
        out["jacobi" if jac else "reference_cg"] = {"iterations": int(it), "solve_ms": round(ms, 2)}
    steps = max(50, min(args.steps, 200))
    eng.begin(0.0)
    eng.iterate(20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.iterate(steps)
    eng.finish()
    torch.cuda.synchronize()
    info = eng.loop_info()
    out["jacobi"].update({"us_per_iteration": round((time.perf_counter() - t0) / steps * 1e6, 2),
                          "loop": "fused: stencil launch forms d = z + beta d (z = r / diag stored by the r update), 2 launches"
                                  if info["fused_direction_update"] else "three launches"})
    out["note"] = "opt-in (jacobi=True / MFS_JACOBI=1), off by default: not the reference's residual history, same solution to tol"
    del eng, wx, wy, wz, lphi, b, x, d, r, q
    torch.cuda.empty_cache()
    return out


def spawn_ranks(args):
    """`python bench.py --gpus N` (N > 1) started WITHOUT torch.distributed.run: start the N ranks as child processes
    (one per GPU, `python -m torch.distributed.run`), relay their output -- rank 0 prints the JSON line -- and return
    their exit code.  Done before anything in this process touches the GPU (never an exec of a process that has)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL and the HIP-IPC windows need it on this pool
    return subprocess.run(cmd, env=env).returncode


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        args.gpus = world
    # MFS_BENCH_SHARED_GPU=1: REHEARSAL of the N > 1 flow on a one-GPU box -- every rank on cuda:0, gloo instead
    # of RCCL (which refuses two ranks on one device).  The numbers mean nothing; the code path is the real one.
    shared = os.environ.get("MFS_BENCH_SHARED_GPU", "0") == "1"
    if shared:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1 or args.force_phases or args.force_p2p or args.force_rccl:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        from mfs.dist import pg_timeout       # bounded: a lost rank must end the run, not hang it
        if shared:
            dist.init_process_group("gloo", rank=rank, world_size=world, timeout=pg_timeout())
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev, timeout=pg_timeout())

    from mfs import _lib
    from mfs.pcg import PcgEngine
    from mfs import dist as mdist

    _lib.load()
    tdt = torch.float32 if args.dtype == "f32" else torch.float64
    esz = 4 if args.dtype == "f32" else 8
    if args.n:
        n = args.n
        ggrid = {1: (n, n, n), 2: (2 * n, n, n), 4: (2 * n, 2 * n, n), 8: (2 * n, 2 * n, 2 * n)}.get(world, (n * world, n, n))
    else:
        ggrid = GRIDS.get(world, (256 * world, 256, 256))      # other world sizes: 256 planes of 256^2 per rank
    if args.strong:
        n = args.n or 256
        ggrid = (n, n, n)
    if args.local_grid and world == 1:
        ggrid = tuple(int(v) for v in args.local_grid.split(","))
    seed = 0

    # ---- this rank's slab (global planes [a-1, b+1) incl. one ghost/boundary plane each side)
    part = mdist.SlabPartition(ggrid[0], world, rank)
    lo, hi = part.local_range            # cell planes held locally
    lgres = (hi - lo, ggrid[1], ggrid[2])
    wx, wy, wz, lphi, (b, x, d, r, q) = build_problem(torch, dev, tdt, lgres, ggrid, seed, (lo, hi))
    eng = PcgEngine(lgres, tdt, dev)
    eng.setup(lphi, wx, wy, wz)
    eng.bind(b, x, d, r, q)
    if args.dense_coefficients:
        eng.set_compress(False)
    if args.unfused:
        eng.set_fuse(False)
    multi = world > 1 or args.force_phases or args.force_p2p or args.force_rccl
    cg_rccl = mdist.SlabCG(eng, part, d, dist if multi else None, force_multi=args.force_phases or args.force_p2p or args.force_rccl)
    cg, transport, tinfo = cg_rccl, ("rccl" if multi else "single"), {}
    native_rccl = False

    def sync():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def agree(flag):
        """True only if every rank says so (the ranks must take the same path)."""
        if world == 1:
            return bool(flag)
        t = torch.tensor([1 if flag else 0], dtype=torch.int32, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    # ---- the collective transport, native form (round 3): the window loop's launches with RCCL between them, enqueued from
    # C.  Needs a real RCCL group (not the gloo rehearsal); trusted only after it reproduces the phase-by-phase loop's history.
    if multi and not shared and not args.force_phases and not args.force_p2p and args.transport in ("auto", "rccl"):
        ok, why = False, ""
        try:
            from mfs.rccl import RcclComm
            comm = RcclComm(dist, dev)
            cg_native = mdist.SlabCG(eng, part, d, dist, force_multi=True, rccl=comm)
            V = 6
            cg_rccl.begin(0.0)
            cg_rccl.iterate(V)
            h_py = eng.history()[: 2 * V + 1]
            cg_native.begin(0.0)
            cg_native.iterate(V)
            cg_native.finish()
            h_nat = eng.history()[: 2 * V + 1]
            ok = cg_native.mode == "rccl" and len(h_nat) == len(h_py) == 2 * V + 1 and bool(max(abs(h_nat - h_py) / abs(h_py)) < 1e-9)
            if not ok:
                why = f"history differs from the phase-by-phase loop's (mode {cg_native.mode})"
        except Exception as exc:      # noqa: BLE001
            why = repr(exc)[:300]
        ok = agree(ok)
        tinfo["rccl_loop"] = ("native: window-loop launches, ncclSend/Recv of the edge planes on a second stream, one ncclAllReduce per "
                              "dot product, enqueued from C (csrc/mfs_rccl.h)") if ok else ("phase-by-phase (torch.distributed); native loop not used: " + why)
        if ok:
            cg_rccl_phases, cg_rccl, native_rccl = cg_rccl, cg_native, True
            if transport == "rccl":
                cg = cg_rccl

    window = None
    if multi and not args.force_phases and not args.force_rccl and args.transport in ("auto", "p2p"):
        from mfs.p2p import P2PWindow
        window = P2PWindow(dist, lgres[1] * lgres[2] * esz, dev)
        tinfo["p2p_selftest"] = "ok" if window.ok else window.why
        tinfo["p2p_window_memory"] = window.alloc_kind
        if window.ok:
            cg_p2p = mdist.SlabCG(eng, part, d, dist, window=window)
            # cross-check before trusting it for the timed run: the same V iterations from the same
            # start through both transports must give the same residual history (they differ only
            # in the order the dot products' partial sums are added)
            V, dev_rel, ok = 6, float("nan"), False
            try:
                cg_rccl.begin(0.0)
                cg_rccl.iterate(V)
                h_r = eng.history()[: 2 * V + 1]
                cg_p2p.begin(0.0)
                cg_p2p.iterate(V)
                h_p = eng.history()[: 2 * V + 1]
                cg_p2p.begin(0.0)                 # ... and once more: the window loop must reproduce itself bit for bit
                cg_p2p.iterate(V)
                h_p2 = eng.history()[: 2 * V + 1]
                tinfo["p2p_reproducible"] = bool(len(h_p2) == len(h_p) and (h_p2 == h_p).all())
                dev_rel = float(abs(h_p - h_r).max() / abs(h_r).max()) if len(h_p) == len(h_r) == 2 * V + 1 else float("nan")
                # both loops do the same arithmetic per cell and differ only in the order of the dot products' partial
                # sums: 1e-16 .. 1e-15 in either state precision; anything visibly larger is a transport fault
                ok = dev_rel == dev_rel and max(abs(h_p - h_r) / abs(h_r)) < 1e-9 and tinfo["p2p_reproducible"]
            except _lib.MfsError as exc:
                tinfo["p2p_error"] = str(exc)[:300]
            ok = agree(ok)
            tinfo["p2p_vs_rccl_history_dev"] = dev_rel
            tinfo["p2p_crosscheck"] = "ok" if ok else "FAILED -> rccl"
            if ok and args.transport == "auto":
                # calibration (part of the warm-up, outside the timed region): the same C iterations through both
                # transports; the timed run uses the faster one and both times are reported
                C = 20

                def probe(c):
                    c.begin(0.0)
                    c.iterate(5)
                    sync()
                    t1 = time.perf_counter()
                    c.iterate(C)
                    sync()
                    tt_ = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
                    if world > 1:
                        dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
                    return tt_.item() / C
                def poll_ok():
                    """collective: True only if NO rank saw a peer-to-peer wait time out"""
                    try:
                        eng.poll()
                        good = True
                    except _lib.MfsError as exc:
                        tinfo["p2p_error"] = str(exc)[:300]
                        good = False
                    return agree(good)
                t_p2p = t_p2p_aux = float("inf")
                eng.slab_set_aux(False)
                t = probe(cg_p2p)
                if poll_ok():
                    t_p2p = t
                    eng.slab_set_aux(True)                 # edge-plane sends from a second stream
                    t = probe(cg_p2p)
                    if poll_ok():
                        t_p2p_aux = t
                t_rccl = probe(cg_rccl)
                r5 = lambda v: round(v * 1e3, 5) if v != float("inf") else None  # noqa: E731
                tinfo["calibration_ms_per_step"] = {"p2p": r5(t_p2p), "p2p_aux_stream": r5(t_p2p_aux), "rccl": r5(t_rccl)}
                eng.slab_set_aux(t_p2p_aux < t_p2p)
                tinfo["p2p_aux_stream"] = bool(t_p2p_aux < t_p2p)
                if min(t_p2p, t_p2p_aux) <= t_rccl:
                    cg, transport = cg_p2p, "p2p"
                else:
                    tinfo["p2p_slower_than_rccl"] = True
            elif ok:
                cg, transport = cg_p2p, "p2p"

    def timed_block(warm):
        """W untimed warm-up steps, then EXACTLY args.steps steps bracketed by barrier + synchronize; max over the ranks"""
        cg.begin(0.0)                      # tol = 0: never "converged", every step does full work
        cg.iterate(warm)
        sync()
        t0_ = time.perf_counter()
        cg.iterate(args.steps)
        t_enq_ = time.perf_counter() - t0_   # host time to enqueue the steps (no sync inside)
        if transport in ("single", "p2p") or (transport == "rccl" and native_rccl):
            eng.finish()                   # the one solution update the fused loop still owes (inside the timed region)
        sync()
        dt_ = time.perf_counter() - t0_
        if world > 1:
            tt_ = torch.tensor([dt_], dtype=torch.float64, device=dev)
            dist.all_reduce(tt_, op=dist.ReduceOp.MAX)
            dt_ = tt_.item()
        st_ = eng.poll()
        assert st_["iterations"] == warm + args.steps, st_
        assert st_["delta"] == st_["delta"], "NaN residual"
        return dt_, t_enq_

    # With --full a short run (the driver's --steps 20 is a 2.6 ms region) is repeated: 9 blocks of exactly --steps steps
    # each, the MEDIAN is the reported time, min / max beside it (`steps` stays what was asked for).  A plain run: one block
    n_blocks = args.repeat if args.repeat > 0 else (9 if args.full and args.steps < 100 else 1)
    blocks = [timed_block(args.warmup) for _ in range(n_blocks)]
    if args.dump_outputs:              # before anything below iterates the engine again
        dump_outputs(args.dump_outputs, torch, eng, {"x": x, "r": r, "d": d}, rank, world)
    dts = sorted(b_[0] for b_ in blocks)
    dt = dts[len(dts) // 2]
    t_enq = sorted(b_[1] for b_ in blocks)[len(blocks) // 2]
    block_info = {"blocks": n_blocks, "steps_per_block": args.steps, "ms_per_step_median": round(dt / args.steps * 1e3, 5),
                  "ms_per_step_min": round(dts[0] / args.steps * 1e3, 5), "ms_per_step_max": round(dts[-1] / args.steps * 1e3, 5),
                  "ms_per_step_first_block": round(blocks[0][0] / args.steps * 1e3, 5),
                  "reported": "median" if n_blocks > 1 else "the one block"}

    # the other transport on the same problem, outside the timed region (diagnostic only)
    if args.full and world > 1 and transport == "p2p":
        k_alt = max(10, min(args.steps, 100))
        cg_rccl.begin(0.0)
        cg_rccl.iterate(10)
        sync()
        t1 = time.perf_counter()
        cg_rccl.iterate(k_alt)
        sync()
        ta = torch.tensor([time.perf_counter() - t1], dtype=torch.float64, device=dev)
        dist.all_reduce(ta, op=dist.ReduceOp.MAX)
        tinfo["rccl_transport_ms_per_step"] = round(ta.item() / k_alt * 1e3, 5)

    owned_cells = part.global_cells(ggrid)
    value = owned_cells * args.steps / dt / 1e6

    # ---- roofline of the dominant kernel (stencil apply), measured with HIP events
    rf = None
    parity = None
    f64_line = None
    nb_line = None
    visc_line = None
    jac_line = None
    cfg2_line = None
    cfg4_line = None
    ts_line = None
    sparse_line = None
    ev_over = 0.0
    if rank == 0 and args.full and not args.timed_loop_only:
        Nx, Ny, Nz = lgres
        cells_l = Nx * Ny * Nz
        reps = max(20, min(args.steps, 200))
        reps_leg = 32          # the side legs stay short: they share kernel templates with the timed loop (rocprof averages)

        cal = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
        for s_ev, e_ev in cal:
            s_ev.record()
            e_ev.record()
        torch.cuda.synchronize()
        ev_over = sorted(a.elapsed_time(b_) for a, b_ in cal)[len(cal) // 2]
        # NOT subtracted: an empty pair (~9 us) over-states what two records cost around a running kernel
        # (rocprofv3 gives 63.2 us for the kernel whose bracketed time is 66.5 us); the bracketed time is the
        # conservative figure and is what `achieved` uses.
        def time_apply(engine, n, robust=False):
            """average duration of the stencil launch inside real CG iterations: HIP events (on the stream the kernel is
            launched on) bracket each apply launch of n native iterations"""
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for s_ev, e_ev in ev:
                s_ev.record()
                engine.native_apply()       # the stencil launch of one native iteration
                e_ev.record()
                engine.native_finish()
            torch.cuda.synchronize()
            ts = sorted(a.elapsed_time(b_) for a, b_ in ev)
            if robust:       # side legs (few launches): the median -- one hiccup among 24 launches moves a mean by 30 %
                return ts[len(ts) // 2]
            return sum(ts) / n

        def alg_bytes_of(form, fused):
            # SURVEY.md 8(d)'s stencil figure (6N^3+3N^2 scalars: v, 4 coefficient arrays in, out); with the direction
            # update folded in: + r in, d_new out, d_old in the place of v = 8N^3+3N^2; with the previous iteration's
            # x update deferred into the launch as well: + x in, x out = 10N^3+3N^2
            per = 6 if not fused else (10 if form["deferred_x_update"] else 8)
            return (per * cells_l + 3 * Ny * Nz) * esz

        def leg(engine, fused, label):
            engine.set_fuse(fused)
            engine.begin(0.0)
            engine.iterate(2)
            form = engine.loop_info()
            ms = time_apply(engine, reps_leg, robust=True)
            ab = alg_bytes_of(form, fused)
            return {"kernel": label, "algorithmic_bytes": ab, "kernel_ms": round(ms, 5), "kernel_ms_is": "median of %d launches" % reps_leg,
                    "kernel_ms_minus_event_pair": round(ms - ev_over, 5),
                    "achieved": round(ab / (ms * 1e-3) / 1e9, 1), "frac": round(ab / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}

        form = eng.loop_info()
        alg_bytes = alg_bytes_of(form, True)
        if transport != "single":          # leave the slab loops' state behind: plain single-domain iterations
            eng.begin(0.0)
            eng.iterate(2)
        ms_cg = time_apply(eng, reps)
        # round 3: the fused launches of a single-domain solve visit only the (tile, plane) pairs of the march that hold a live
        # z-vector (mfs_pcg3d_sparse_info).  The roofline prices the launch on the cells it PROCESSES (listed pairs); the rate
        # over all cells of the grid is reported beside it as `effective`, and the same loop with the lists off is timed below.
        sp = eng.sparse_info()
        listed_frac = (sp["listed_pairs"] / sp["pairs"]) if sp["pairs"] else 1.0
        alg_bytes_all = alg_bytes
        alg_bytes = int(alg_bytes_all * listed_frac)
        ms_b2b = None
        if args.b2b:   # back-to-back applies (Infinity-Cache-warm; NOT what the CG loop sees)
            s_ev, e_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            eng.apply(d, q)
            s_ev.record()
            for _ in range(reps):
                eng.apply(d, q)
            e_ev.record()
            torch.cuda.synchronize()
            ms_b2b = s_ev.elapsed_time(e_ev) / reps
        achieved = alg_bytes / (ms_cg * 1e-3) / 1e9
        # the launch the timed loop runs: since round 2 it also closes the previous iteration (folds the r.r partials, takes
        # the convergence decision; template flag BOOK) -- native_apply / native_finish are the two halves of exactly that loop
        kname = ("k_pcg_apply_march<..., FUSE=true, XDEF=true, BOOK=true> (stencil apply + d = r + beta d + x += alpha d_old "
                 "+ bookkeeping of the previous iteration)"
                 if form["deferred_x_update"] else "k_pcg_apply_march<..., FUSE=true, BOOK=true> (stencil apply + d = r + beta d "
                 "+ bookkeeping of the previous iteration)")
        # HBM bytes per launch from PMC counters: collected by tools/pmc_bench.sh on this same command in a SEPARATE
        # run (rocprofv3 --pmc passes cannot ride in a timed run) and committed under profiles/ -- evidence, not a
        # measurement of this run; valid for the default workload only.  traffic_frac = those bytes / this run's kernel
        # time / peak: the fraction of the HBM roofline the kernel's real traffic amounts to.
        traffic, traffic_src, dense_traffic = None, None, None
        for name in ("r03_pmc_apply.json", "r02_pmc_apply.json", "r01_pmc_apply.json"):
            pj = os.path.join(REPO, "profiles", name)
            if os.path.exists(pj) and transport == "single":
                try:
                    pm = json.load(open(pj))
                    if pm.get("workload") == f"{Nx}x{Ny}x{Nz} {args.dtype}":
                        traffic = pm.get("hbm_bytes_per_launch")
                        dense_traffic = pm.get("dense_hbm_bytes_per_launch")
                        traffic_src = {"file": "profiles/" + name, "collected": pm.get("collected"),
                                       "commit": pm.get("commit"), "how": "separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE "
                                       "passes over this command (tools/pmc_bench.sh), FETCH_SIZE x2 (gfx950), not this run"}
                        break
                except Exception:
                    pass
        rf = {"bound": "hbm", "kernel": kname, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
              "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
              "frac_is": "EFFECTIVE rate: algorithmic bytes / kernel time / peak.  With compressed coefficient access "
                         "(default) the kernel moves fewer bytes than the algorithmic count on this scene, so this is "
                         "not an HBM-utilisation figure -- traffic_frac and the `dense` legs are",
              "traffic": traffic,
              "traffic_frac": (round(traffic / (ms_cg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if traffic else None),
              "traffic_source": traffic_src,
              "algorithmic_bytes": alg_bytes, "algorithmic_bytes_is": "SURVEY 8(d) bytes per cell x the cells of the (tile, plane) "
              "pairs the launch visits (%d of %d pairs)" % (sp["listed_pairs"], sp["pairs"]) if sp["pairs"] else "SURVEY 8(d) bytes per cell x all cells",
              "effective_all_cells": {"algorithmic_bytes": alg_bytes_all, "achieved": round(alg_bytes_all / (ms_cg * 1e-3) / 1e9, 1),
                                      "frac": round(alg_bytes_all / (ms_cg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                      "note": "the same kernel time priced on every cell of the grid (what a dense sweep would move)"},
              "kernel_ms": round(ms_cg, 5),
              "kernel_ms_minus_event_pair": round(ms_cg - ev_over, 5),
              "event_pair_overhead_ms": round(ev_over, 5),
              "event_pair_note": "an empty record pair; NOT subtracted in `achieved` / `frac` (it over-states what two records cost "
                                 "around a running kernel): kernel_ms_minus_event_pair is the lower bracket, rocprofv3's kernel-only "
                                 "average (profiles/) lies between the two"}
        # the timed loop with the sparse lists off (same process, same box): what the lists are worth on this scene
        if sp["pairs"] or sp["chunks"]:
            eng.set_sparse(False)
            eng.begin(0.0)
            eng.iterate(10)
            torch.cuda.synchronize()
            t1_ = time.perf_counter()
            eng.iterate(100)
            eng.finish()
            torch.cuda.synchronize()
            ms_dense_loop = (time.perf_counter() - t1_) / 100 * 1e3
            ms_dense_apply = time_apply(eng, reps_leg, robust=True)
            eng.set_sparse(True)
            sparse_line = dict(sp, ms_per_step_lists_off=round(ms_dense_loop, 5), stencil_launch_ms_lists_off=round(ms_dense_apply, 5),
                               note="single-domain solves from 2^21 cells: live 32-cell chunks for the r update, listed (tile, plane) "
                                    "pairs for the fused stencil launches; dead cells keep q = r = d = 0 and x as the dense loop leaves them")
        # the PLAIN stencil apply (6N^3 + 3N^2 scalars -- the figure BASELINE.md's 60 % target is
        # stated on), inside the three-kernel form of the loop (direction update unfused)
        rf["plain_stencil_apply"] = leg(eng, False, "k_pcg_apply_march<..., FUSE=false> (6N^3+3N^2 scalars, SURVEY.md 8(d)), "
                                                    "compressed coefficient access")
        # DENSE coefficient access (every coefficient array read in full: what the kernel does on a scene without
        # regular regions) -- the honest HBM figure: measured traffic ~ algorithmic bytes here
        eng.set_compress(False)
        rf["dense"] = {"plain_stencil_apply": leg(eng, False, "k_pcg_apply_march<..., FUSE=false, COMP=false>"),
                       "fused": leg(eng, True, "k_pcg_apply_march<..., FUSE=true, COMP=false>"),
                       "note": "set_compress(False): the 60 % target of BASELINE.json is judged on dense.plain_stencil_apply"}
        if dense_traffic:
            rf["dense"]["traffic_plain"] = dense_traffic
        eng.set_compress(True)
        eng.set_fuse(True)
        # an ALL-MIXED scene: every face weight a random quarter, every cell fluid -- no vector is ZERO or REGULAR, the
        # compressed access reads everything (plus the class bytes): the figure is then no property of the pool scene
        gen = torch.Generator(device=dev).manual_seed(1)
        rq = lambda shape: (torch.randint(1, 5, shape, generator=gen, device=dev).to(tdt) * 0.25)  # noqa: E731
        wxm, wym, wzm = rq(tuple(wx.shape)), rq(tuple(wy.shape)), rq(tuple(wz.shape))
        eng.setup(-torch.ones(lgres, dtype=tdt, device=dev), wxm, wym, wzm)
        b.normal_(generator=gen)
        rf["all_mixed_scene"] = {"plain_stencil_apply": leg(eng, False, "compressed access, every vector MIXED"),
                                 "fused": leg(eng, True, "compressed access, every vector MIXED"),
                                 "scene": "lphi = -1 everywhere, face weights uniform in {0.25, 0.5, 0.75, 1}"}
        del wxm, wym, wzm
        if ms_b2b:
            rf["kernel_ms_back_to_back"] = round(ms_b2b, 5)
            rf["achieved_back_to_back"] = round(alg_bytes / (ms_b2b * 1e-3) / 1e9, 1)

        # ---- parity self-check OUTSIDE the timed region: the engine exactly as timed (auto nontemporal / compressed /
        # fused / deferred-x forms) on the bench workload, first 10 iterations' residual history and x after finish()
        # against the oracle's C restatement (the checker; never the thing measured)
        if world == 1 and transport == "single":
            parity = parity_check(args, torch, dev, tdt, lgres, seed)

        # ---- the drop-in's DEFAULT precision (fp64 state, like the reference): same workload, shorter timed loop
        if world == 1 and transport == "single" and args.dtype == "f32" and not args.no_f64_line:
            f64_line = f64_leg(args, torch, dev, lgres, seed)
        # ---- the reference's own grid (launch-bound size): resident loop
        if world == 1 and transport == "single" and not args.no_f64_line:
            nb_line = notebook_grid_leg(torch, dev)
        # ---- BASELINE config 3 (viscosity CG 128^3, with its own oracle check) and the same solver beyond the Infinity
        # Cache; the opt-in Jacobi loop on the bench workload
        if world == 1 and transport == "single" and args.dtype == "f32" and not args.no_f64_line and not args.local_grid:
            def soft(fn, *a):
                """a side leg must not take the headline down with it: its failure is reported in its place (and on stderr)"""
                try:
                    return fn(*a)
                except Exception as exc:      # noqa: BLE001
                    print(f"bench side leg {fn.__name__} failed: {exc!r}", file=sys.stderr, flush=True)
                    torch.cuda.empty_cache()
                    return {"error": repr(exc)[:400]}
            if not args.no_side_legs:
                cfg2_line = soft(config2_leg, args, torch, dev, seed)
                visc_line = {"config3_128": soft(viscosity_leg, torch, dev, 128, 200, True, "fp32", ev_over),
                             "n256": soft(viscosity_leg, torch, dev, 256, 60, False, "fp32", ev_over),
                             # the drop-in's DEFAULT precision at the size beyond the Infinity Cache, with its own oracle check
                             "f64_state": soft(viscosity_leg, torch, dev, 256, 40, True, "fp64", ev_over),
                             # the reference's OWN grid (3D_viscous_fluid_sim.ipynb:651-656): the resident small-grid loop
                             "notebook_grid": soft(viscosity_leg, torch, dev, (48, 80, 48), 2000, True, "fp64", ev_over)}
                jac_line = soft(jacobi_leg, args, torch, dev, tdt, lgres, seed)
                jac_line["viscosity"] = soft(viscosity_jacobi_leg, torch, dev, 128)
                cfg4_line = soft(config4_rank_share_leg, args, torch, dev, seed, ev_over)
                ts_line = soft(timestep_leg, torch, dev, 128, 3)
    if world > 1:
        dist.barrier()

    if rank == 0:
        cb = None
        if world == 1 and args.full and not args.no_cpu_baseline:
            del eng, cg, cg_rccl, b, x, d, r, q, wx, wy, wz, lphi
            torch.cuda.empty_cache()
            cb = cpu_baseline(args, ggrid, seed)
        iter_bytes = 15 * lgres[0] * lgres[1] * lgres[2] * esz
        out = {
            "metric": "PressureCGSolver3D CG throughput (cells x iterations / s)",
            "value": round(value, 1), "unit": "Mcells/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 5), "higher_is_better": True,
            "scaling": "strong" if args.strong else "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": f"PressureCGSolver3D {ggrid[0]}x{ggrid[1]}x{ggrid[2]} synthetic pool scene, "
                                   f"fp32 state" if args.dtype == "f32" else
                                   f"PressureCGSolver3D {ggrid[0]}x{ggrid[1]}x{ggrid[2]} synthetic pool scene, fp64 state",
                       "grid": list(ggrid), "cells_per_gpu": lgres[0] * lgres[1] * lgres[2],
                       "decomposition": f"x-slabs x{world}" if world > 1 else "single domain",
                       "transport": transport,
                       "step": "one CG iteration (apply + 2 dots + x/r/d updates)"},
            "iters_per_s": round(args.steps / dt, 2),
            "timed_blocks": block_info,
            "host_enqueue_ms_per_step": round(t_enq / args.steps * 1e3, 5),
            "cg_iteration_hbm_gbs": round(iter_bytes / (dt / args.steps) / 1e9, 1),
            "roofline": rf,
            "residual_parity": ("checked over a window: CG on this operator is chaotic in rounding (the oracle departs from "
                                "its own history by > 1e-2 after ~30 iterations when only its summation order changes, "
                                "tests/test_oracle_sensitivity.py), so north_star's 1e-5 rel residual match is asserted on "
                                "the first 10 iterations at the bench size (parity_check) and 8-10 on the goldens; over the WHOLE "
                                "history the HIP solvers stay inside the rounding envelope of the oracle itself -- dev_k <= 4 E_k + 1e-9 "
                                "for every entry k, E_k from 80 rounding variants of the C oracle (tests/test_history_envelope.py, "
                                "tests/golden/envelope_*.npz)"),
        }
        if not args.full:              # a plain run times the steps and checks nothing beyond them
            del out["roofline"], out["residual_parity"]
        if sparse_line is not None:
            out["sparse_lists"] = sparse_line
        if parity is not None:
            out["parity_check"] = parity
        if f64_line is not None:
            out["f64_state"] = f64_line
        if nb_line is not None:
            out["notebook_grid"] = nb_line
        if cfg2_line is not None:
            out["config2_128"] = cfg2_line
        if visc_line is not None:
            out["viscosity"] = visc_line
        if jac_line is not None:
            out["jacobi_preconditioned"] = jac_line
        if cfg4_line is not None:
            out["config4_rank_share"] = cfg4_line
        if ts_line is not None:
            out["timestep_128"] = ts_line
        if shared:
            out["rehearsal"] = "all ranks share cuda:0 over gloo (MFS_BENCH_SHARED_GPU=1): code-path check, not a measurement"
        if tinfo:
            out["transport_info"] = tinfo
        if cb is not None:
            out["cpu_baseline"] = cb
        print(json.dumps(out), flush=True)
    if window is not None:
        window.close()
    elif world > 1:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
