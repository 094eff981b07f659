"""GPU: time of mfs.render's paths (Scene.trace / resolve) on the scene of tools/bench_render.py -- the skin of a column of
liquid over a floor slab and a ramp on (2N+1)^3 lattices, 1920 x 1080, perspective, step = half the lattice spacing --
beside the primary-only march of `Scene.render`, measured in the same process.
Between device events, median of REPEATS after a warm-up call, spread = (max - min) / median; per variant `ms`, `spread`,
`samples` (shape samples evaluated) and `ratio` = ms / march_ms:
  march          `Scene.render` with the skips: the comparison
  shadows        `trace`, both shapes opaque, shadows on: slots 0 and 3
  water          `trace`, the skin a liquid (ior 1.33), shadows on: up to four marches per ray
  water_2x2      the same with samples=2: four rays per pixel
  *_full         the same with skip=False (3 repeats)
  maxima_ms      the brick maxima of the liquid's volume
  resolve_ms     `mfs.render.resolve` of the 2 x 2 trace
The outputs with and without the skips are checked to be the same bits.
usage: python tools/bench_render_paths.py N [fp32|fp64] [out.png]   -- one JSON line"""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), REPO, os.path.join(REPO, "tools")]
import torch
from mfs import render, skin, tensors as T
import bench_render as BR
W, H, REPEATS = BR.W, BR.H, BR.REPEATS

if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    dtype = T.state_dtype(sys.argv[2] if len(sys.argv) > 2 else "fp64")
    px = BR.cloud(N, dtype)
    shape, origin, h = (2 * N + 1,) * 3, (-0.5, 0.0, -0.5), 0.5 / N
    liquid, ground = skin.field(px, shape, origin, h), BR.solid(N)
    del px
    scene = render.Scene([liquid, ground])
    cam = render.Camera((1.3, 1.1, 1.7), (0.0, 0.35, 0.0), fov=40.0, width=W, height=H)
    M = render.Material
    light = (0.3, 2.0, 0.4)
    opaque = [M.opaque(render.LIQUID_COLOR), M.opaque(render.SOLID_COLOR)]
    water = [M.liquid(render.LIQUID_COLOR), M.opaque(render.SOLID_COLOR)]
    looks = dict(shadows=render.Look(opaque, light), water=render.Look(water, light), water_2x2=render.Look(water, light, samples=2))
    out = {}
    st = {}
    scene.render(cam, stats=st)
    ms, sp = BR.timed(lambda: scene.render(cam))
    out["march"] = dict(ms=ms, spread=sp, samples=st["samples"])
    st = {}
    scene.render(cam, skip=False, stats=st)
    ms, sp = BR.timed(lambda: scene.render(cam, skip=False), 3)
    out["march_full"] = dict(ms=ms, spread=sp, samples=st["samples"])
    same = True
    for name, look in looks.items():
        st, full = {}, {}
        res = scene.trace(cam, look, stats=st)
        if name != "water_2x2":                                          # the 2 x 2 trace without skips: four times `water_full`
            plain = scene.trace(cam, look, skip=False, stats=full)
            same = same and all(torch.equal(a, b) for a, b in zip(res[:4], plain[:4]))
            del plain
            ms, sp = BR.timed(lambda: scene.trace(cam, look, skip=False), 3)
            out[name + "_full"] = dict(ms=ms, spread=sp, samples=full["samples"])
        ms, sp = BR.timed(lambda: scene.trace(cam, look))
        ids = res.shape_id
        out[name] = dict(ms=ms, spread=sp, samples=st["samples"], rays=int(ids[..., 0].numel()),
                         marches=[int((ids[..., q] != -2).sum()) for q in range(4)])
    for v in out.values():
        v["ratio"] = round(v["ms"] / out["march"]["ms"], 3)

    def maxima():
        scene.bricks_max[0] = None
        scene._maxima(0)
    maxima_ms, maxima_sp = BR.timed(maxima)
    resolve_ms, resolve_sp = BR.timed(lambda: render.resolve(res))
    if len(sys.argv) > 3:
        render.save_png(sys.argv[3], render.resolve(res))
    print(json.dumps(dict(N=N, dtype=str(dtype).replace("torch.", ""), lattice=shape, image=[W, H], step=res.step, num_steps=res.num_steps,
                          same_bits=same, variants=out, maxima_ms=maxima_ms, maxima_spread=maxima_sp, resolve_ms=resolve_ms,
                          resolve_spread=resolve_sp, repeats=REPEATS, device=torch.cuda.get_device_name(0))), flush=True)
