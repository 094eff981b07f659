"""GPU: time of mfs.attrib on the scene of tools/bench_render.py -- the skin of a column of liquid (8 particles per cell of
an N^3 grid) over a floor and a ramp, 1920 x 1080, perspective -- with a swirl as the particles' velocity: their speed
gathered at every liquid pixel's hit point and at the skin mesh's vertices, with the skin's influence over the unit box.
Between device events, median of REPEATS after a warm-up call, spread = (max - min) / median:
  bins_ms           `attrib.bins`: keys, stable sort, gather of the sorted particles, bin starts
  gather_ms         the whole `attrib.gather` on held bins (query keys, sort, work list with its host read, the kernel)
  kernel_ms         mfs_attrib_gather3d alone on the plumbing's output
  vertices_*        the same at the mesh's vertices
  plain_ms          `render.simulation_image`: skin field, Scene, march, shade -- what `sim.render(camera)` runs
  colored_ms        `render.simulation_colored`: the same plus hit points, binning, gather, colormap, the albedo shading
                    -- what `sim.render(camera, color_by="speed")` runs
`pair_tests` = particles looped over x 256 lanes, `pair_tests_per_s` over kernel_ms (tools/bench_skin.py reports the skin
kernel's, the yardstick).
usage: python tools/bench_attrib.py N [fp32|fp64]   -- the particles' dtype; one JSON line"""
import json, os, sys
from types import SimpleNamespace as NS
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), REPO, os.path.join(REPO, "tools")]
import numpy as np, torch
from mfs import _lib, attrib, render, skin, tensors as T
from bench_render import cloud, solid, timed, W, H, REPEATS, dev


class Stand:
    """what `render.simulation_image` / `simulation_colored` read of a NotebookSimulation"""

    def __init__(self, N, px):
        self.GDX, self.BOUND_MIN, self.BOUND_SIZE = 1.0 / N, np.array([-0.5, 0.0, -0.5], np.float32), np.ones(3, np.float32)
        x = px.to(torch.float64)
        v = torch.stack([-x[:, 2], 0.3 + 0.0 * x[:, 1], x[:, 0]], dim=1) * (1.0 + x[:, 1:2])
        self.particle = NS(x=px, v=v.contiguous())
        ground = solid(N)
        self.solid_levelset = NS(phi=ground.phi, bound_min=self.BOUND_MIN, resolution=tuple(ground.phi.shape))
        self.shape, self.h = (2 * N + 1,) * 3, 0.5 / N

    def skin_field(self, clip=True):
        f = skin.field(self.particle.x, self.shape, (-0.5, 0.0, -0.5), self.h)
        return f._replace(phi=torch.maximum(f.phi, -self.solid_levelset.phi)) if clip else f


def gather_times(points, B, values, tag):
    """(dict of the timings of one set of query points, stats)"""
    st = {}
    out = attrib.gather(points, B, values, stats=st)
    whole = timed(lambda: attrib.gather(points, B, values))
    lib = _lib.load()
    count = int(np.prod(B.shape))
    qkeys, rows = torch.sort(attrib._keys(lib, B.origin, B.shape, B.influence, B.box, points), stable=True)
    items, n = attrib._work_items(qkeys, count)
    qs, vs = points[rows], values.reshape(len(values), -1)[B.order].contiguous()
    val = torch.full((points.shape[0], 1), float("nan"), dtype=torch.float32, device=dev)
    wgt = torch.zeros(points.shape[0], dtype=torch.float32, device=dev)
    kernel = lambda: _lib.check(lib.mfs_attrib_gather3d(  # noqa: E731
        _lib.i64x(B.shape), _lib.f64x(B.origin), B.influence, 1, float("nan"), T.ptr(B.particles), T.code(B.particles), T.ptr(vs),
        T.code(vs), B.particles.shape[0], T.ptr(B.starts), T.ptr(qs), T.code(qs), T.ptr(rows), points.shape[0], T.ptr(items), n,
        T.ptr(val), T.ptr(wgt), None, T.stream()), "gather")
    k = timed(kernel)
    assert torch.equal(val.view(torch.int32), out[0].view(torch.int32))
    return {f"{tag}_points": int(points.shape[0]), f"{tag}_covered": int((out[1] > 0).sum()), f"{tag}_work_items": st["work_items"],
            f"{tag}_pair_tests": st["pair_tests"], f"{tag}_gather_ms": whole[0], f"{tag}_gather_spread": whole[1],
            f"{tag}_kernel_ms": k[0], f"{tag}_kernel_spread": k[1],
            f"{tag}_pair_tests_per_s": float(f"{st['pair_tests'] / (k[0] * 1e-3):.4g}")}


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    dtype = T.state_dtype(sys.argv[2] if len(sys.argv) > 2 else "fp64")
    sim = Stand(N, cloud(N, dtype))
    cam = render.Camera((1.3, 1.1, 1.7), (0.0, 0.35, 0.0), fov=40.0, width=W, height=H)
    names, shapes = render.simulation_shapes(sim)
    R, box = shapes[0].influence, render.simulation_box(sim)
    res = render.Scene(shapes).render(cam)
    points = torch.where((res.shape_id == 0).unsqueeze(-1), render.hit_points(res, cam), float("nan")).reshape(-1, 3).contiguous()
    speed = render.simulation_values(sim, "speed")
    B = attrib.bins(sim.particle.x, R, box)
    bins_ms, bins_sp = timed(lambda: attrib.bins(sim.particle.x, R, box))
    out = dict(N=N, particles=int(sim.particle.x.shape[0]), dtype=str(dtype).replace("torch.", ""), image=[W, H],
               influence_h=round(R / sim.h, 4), bins=list(B.shape), bins_ms=bins_ms, bins_spread=bins_sp)
    out.update(gather_times(points, B, speed, "pixels"))
    mesh = skin.extract(shapes[0])
    out.update(gather_times(mesh.vertices.contiguous(), B, speed, "vertices"))
    del B, points, mesh, res, shapes
    plain = render.simulation_image(sim, cam)
    plain_ms, plain_sp = timed(lambda: render.simulation_image(sim, cam))
    colored = render.simulation_colored(sim, cam, ("liquid", "solid"), None, None, "speed", None, "speed")
    colored_ms, colored_sp = timed(lambda: render.simulation_colored(sim, cam, ("liquid", "solid"), None, None, "speed", None, "speed"))
    liquid = (colored != plain).any(dim=-1)
    if len(sys.argv) > 3:
        render.save_png(sys.argv[3], colored)
    out.update(plain_ms=plain_ms, plain_spread=plain_sp, colored_ms=colored_ms, colored_spread=colored_sp,
               colored_over_plain=round(colored_ms / plain_ms, 3), recoloured_pixels=int(liquid.sum()), repeats=REPEATS,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out), flush=True)
