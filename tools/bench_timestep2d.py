"""GPU: whole 2D time steps (notebook_sim2d.NotebookSimulation2D) on ONE MI355X: a dam break on an N x N grid -- flipped
sdf2D container box, one ramp, a liquid block of (0.4 N) x (0.5 N) cells at 4 particles per cell against the left wall --
per-stage wall-clock (synchronised) in milliseconds per step, CG iteration counts.
usage: python tools/bench_timestep2d.py N [fp32|fp64] [steps]"""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), REPO]
import numpy as np, torch
import notebook_sim2d as NSIM
import solver.sdf2D as sdf
N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
precision = sys.argv[2] if len(sys.argv) > 2 else "fp64"
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = "cuda:0"
torch.cuda.set_device(dev)
gdx = 1.0 / N
bmin = [-0.5, 0.0]
rb_d, rb_map = sdf.generate_rb(None, {}, 'tank', ['box', 1 - 4 * gdx, 1 - 4 * gdx], flip=True, center=[0, 0.5], device=dev)
rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.04], flip=False, center=[0.05, 0.2], angle=-35)
rng = np.random.default_rng(0)
t0 = time.perf_counter()
px = NSIM.add_box([-0.5 + 2 * gdx + 0.2, 0.6], [0.4, 0.5], gdx / 2, rng)
sim = NSIM.NotebookSimulation2D((N, N), gdx, bmin, rb_d, px, gdx / 2, device=dev, precision=precision)
sim.particle.v[:, 0] = 1.0 + torch.sin(6.0 * sim.particle.x[:, 1])          # a sheared start: the viscosity solve has work
torch.cuda.synchronize()
t_setup = time.perf_counter() - t0
sim.step()                                  # warm-up step (allocations, first launches)
tim, its = {}, []
t0 = time.perf_counter()
for _ in range(steps):
    sim.step(timings=tim)
    its.append((sim.DensitySolver.iterations, sim.ViscositySolver.iterations, sim.PressureSolver.iterations))
torch.cuda.synchronize()
t_all = time.perf_counter() - t0
print(json.dumps({"workload": f"2D time step {N}x{N}, {sim.particle.num_particles} particles, mu={sim.MU}", "state_precision": precision,
                  "steps": steps, "ms_per_step": round(t_all / steps * 1e3, 2), "setup_s": round(t_setup, 2),
                  "stage_ms_per_step": {k: round(v / steps * 1e3, 3) for k, v in tim.items()},
                  "cg_iterations(density,viscosity,pressure)": its}))
