"""GPU: time of mfs.render on the scene of tools/bench_skin.py -- the skin of a dam-break-like column of liquid (8 particles
per cell of an N^3 grid) on the (2N+1)^3 lattice of spacing GDX / 2 -- over a solid level set on the same lattice (a floor
slab and a tilted ramp, `notebook_sim.solid_volume`), 1920 x 1080, perspective (fov 40 degrees), step = half the lattice
spacing, near / far from the shapes' boxes.
Between device events, median of REPEATS after a warm-up call, spread = (max - min) / median:
  bricks_ms       `Scene.refresh()`: the brick minima of both volumes
  march_ms        the whole `Scene.render` call with the skips (allocation of the four outputs included)
  march_full_ms   the same with skip=False: every sample of every shape up to the hit
  shade_ms        `mfs.render.shade`
`samples` = shape samples evaluated (one trilinear gather of 8 nodes each), with and without the skips; rays_per_s and
samples_per_s over the march times.  The outputs of the two marches are checked to be the same bits.
usage: python tools/bench_render.py N [fp32|fp64]   -- the particles' dtype; one JSON line"""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), REPO]
import numpy as np, torch
from mfs import render, skin, tensors as T
from solver import sdf3D as sdf
import notebook_sim as NSIM
REPEATS = 5
W, H = 1920, 1080
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_render.py measures on the GPU; there is no CPU path"
torch.cuda.set_device(dev)


def cloud(N, dtype):
    """tools/bench_skin.py's column: cell-centred sub-lattice of spacing PDX, jittered by 0.25 PDX, shuffled"""
    pdx = 0.5 / N
    gen = torch.Generator(device=dev).manual_seed(0)
    n = [int(round(f * 2 * N)) for f in (0.4, 0.6, 1.0)]
    ax = [(torch.arange(k, dtype=torch.float64, device=dev) + 0.5) * pdx for k in n]
    x = torch.stack(torch.meshgrid(*ax, indexing="ij"), dim=-1).reshape(-1, 3)
    x = x + 0.25 * pdx * (2 * torch.rand(x.shape, dtype=torch.float64, device=dev, generator=gen) - 1)
    x = x[torch.randperm(x.shape[0], device=dev, generator=gen)]
    return (x + torch.tensor([-0.5, 0.0, -0.5], dtype=torch.float64, device=dev)).to(dtype).contiguous()


def solid(N):
    rb_d, rb_map = sdf.generate_rb(None, {}, 'floor', ['box', 1.2, 0.1, 1.2], center=[0, 0.0, 0], device=dev)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.7, 0.06, 1.2], center=[0.15, 0.3, 0], axis=[0., 0, 1], angle=-35)
    return NSIM.solid_volume((N, N, N), 1.0 / N, [-0.5, 0.0, -0.5], rb_d, None, dev)


def timed(fn, repeats=REPEATS):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    v = np.asarray(out)
    return round(float(np.median(v)), 4), round(float((v.max() - v.min()) / np.median(v)), 3)


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    dtype = T.state_dtype(sys.argv[2] if len(sys.argv) > 2 else "fp64")
    px = cloud(N, dtype)
    shape, origin, h = (2 * N + 1,) * 3, (-0.5, 0.0, -0.5), 0.5 / N
    liquid, ground = skin.field(px, shape, origin, h), solid(N)
    del px
    assert tuple(ground.phi.shape) == shape
    scene = render.Scene([liquid, ground])
    cam = render.Camera((1.3, 1.1, 1.7), (0.0, 0.35, 0.0), fov=40.0, width=W, height=H)
    st, full = {}, {}
    res = scene.render(cam, stats=st)
    plain = scene.render(cam, skip=False, stats=full)
    same = all(torch.equal(a, b) for a, b in zip(res[:4], plain[:4]))
    del plain
    bricks_ms, bricks_sp = timed(scene.refresh)
    march_ms, march_sp = timed(lambda: scene.render(cam))
    full_ms, full_sp = timed(lambda: scene.render(cam, skip=False), 3)
    colors = [render.LIQUID_COLOR, render.SOLID_COLOR]
    rgb = render.shade(res, cam, colors)
    shade_ms, shade_sp = timed(lambda: render.shade(res, cam, colors))
    if len(sys.argv) > 3:
        render.save_png(sys.argv[3], rgb)
    ids = res.shape_id
    print(json.dumps(dict(N=N, dtype=str(dtype).replace("torch.", ""), lattice=shape, volumes=[str(s.volume.phi.dtype).replace("torch.", "") for s in scene.shapes],
                          bricks=[int(b.numel()) for b in scene.bricks], image=[W, H], near=round(res.near, 5), far=round(res.far, 5),
                          step=res.step, num_steps=res.num_steps, hits=st["hits"], liquid_pixels=int((ids == 0).sum()),
                          solid_pixels=int((ids == 1).sum()), samples=st["samples"], samples_full=full["samples"], same_bits=same,
                          bricks_ms=bricks_ms, bricks_spread=bricks_sp, march_ms=march_ms, march_spread=march_sp,
                          march_full_ms=full_ms, march_full_spread=full_sp, shade_ms=shade_ms, shade_spread=shade_sp,
                          rays_per_s=float(f"{W * H / (march_ms * 1e-3):.4g}"), samples_per_s=float(f"{st['samples'] / (march_ms * 1e-3):.4g}"),
                          samples_per_s_full=float(f"{full['samples'] / (full_ms * 1e-3):.4g}"), repeats=REPEATS,
                          device=torch.cuda.get_device_name(0))), flush=True)
