"""GPU: time of mfs.meshsdf.build on two generated closed meshes -- an icosphere at subdivision 6 (81 920 triangles) and the
closed liquid surface of a dam-break-like frame (a collapsing column over a shallow pool, extracted by
mfs.surface.isosurface) -- onto an N^3 lattice, with the per-brick culling on and off, and of sdf.union_mesh_grid /
sdf.project_mesh for the icosphere body on the 513^3 solid grid (the two extremes: the body wins every node / no node)
and 16.8 M particles (arrays are reset outside the timed region).
Per figure: median and spread = (max - min) / median of REPEATS timings after a warm-up call, each between two device
events (`distance_ms`: the distance kernel alone; `build_ms`: the whole build() call including the triangle gather, the
sign pass and the host sync that reads the odd-column count).  `surviving` = share of (brick, triangle) pairs that reached
the distance kernel's inner loop; `cull_gain` = distance_ms without culling / with.
usage: python tools/bench_meshsdf.py N   -- one JSON line per figure"""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), os.path.join(REPO, "tests"), REPO]
import numpy as np, torch
from mfs import _lib, meshsdf, surface, tensors as T
from solver import sdf3D as sdf
import meshsdf_numpy as M                                    # the mesh generators of the tests
REPEATS, PAD = 5, 3
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_meshsdf.py measures on the GPU; there is no CPU path"
torch.cuda.set_device(dev)


def timed(fn, repeats=REPEATS, reset=None):
    """reset (optional) runs before every call, OUTSIDE the timed region, and is drained before the first event"""
    if reset:
        reset()
    fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if reset:
            reset()
            torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    med = float(np.median(out))
    return round(med, 4), round((max(out) - min(out)) / med, 3)


def dam_break_mesh(n=128):
    """a column that has begun to collapse (it widens towards its foot) over a shallow rippled pool, on n^3 cell centres"""
    h = 1.0 / n
    ax = [(-0.5 + h / 2) + h * torch.arange(n, dtype=torch.float64, device=dev).reshape([-1 if a == d else 1 for a in range(3)])
          for d in range(3)]
    x, y, z = ax[0], ax[1] + 0.5, ax[2]
    col = torch.maximum(torch.maximum(x.abs() - 0.15 - 0.1 * (1 - y).clamp(0, 1) ** 3, y - 0.62), z.abs() - 0.18 - 0.05 * (1 - y).clamp(0, 1) ** 2)
    pool = y - (0.08 + 0.015 * torch.sin(11 * x) * torch.cos(9 * z))
    phi = torch.minimum(col, pool + 0 * z).clamp(max=3 * h).contiguous()
    return surface.isosurface(phi, 0.0, origin=(-0.5 + h / 2, h / 2, -0.5 + h / 2), spacing=h, closed=True, outside=3 * h)


def bench_build(name, mesh, N):
    v = mesh.vertices.detach().cpu().numpy()
    spacing = float((v.max(axis=0) - v.min(axis=0)).max()) / (N - 1 - 2 * PAD)
    shape, origin = meshsdf.lattice(v, spacing, PAD)
    lib = _lib.load()
    tri = mesh.vertices.to(torch.float32)[mesh.faces.to(torch.int64).reshape(-1)].reshape(-1, 9).contiguous()
    phi = torch.empty(shape, dtype=torch.float32, device=dev)
    g, org = _lib.i64x(shape), _lib.f64x(origin)
    row = dict(mesh=name, N=N, lattice=list(shape), triangles=int(tri.shape[0]))
    for cull in (1, 0):
        def kernel():
            _lib.check(lib.mfs_meshsdf_distance3d(g, org, spacing, T.ptr(tri), int(tri.shape[0]), cull, T.ptr(phi), None, T.stream()))
        reps = REPEATS if cull else 3
        tag = "cull" if cull else "nocull"
        row[f"distance_ms_{tag}"], row[f"distance_spread_{tag}"] = timed(kernel, reps)
        row[f"build_ms_{tag}"], row[f"build_spread_{tag}"] = timed(lambda: meshsdf.build(mesh, spacing, PAD, cull=bool(cull)), reps)
    stats = {}
    out = meshsdf.build(mesh, spacing, PAD, cull=True, stats=stats)
    row["surviving"] = round(stats["surviving_fraction"], 5)
    row["cull_gain"] = round(row["distance_ms_nocull"] / row["distance_ms_cull"], 2)
    print(json.dumps(row), flush=True)
    return out


def bench_bodies(msdf):
    body = sdf.MeshBody(msdf, center=(0.05, 0.45, -0.03), axis=(1, 2, 3), angle=37, velocity=(0.1, 0, 0))
    rb = sdf.mesh_rb([body])
    w = torch.tensor([[0.0, 1.0, 0.5]], dtype=torch.float64, device=dev)
    res, h = (513, 513, 513), 1.0 / 512
    for name, dt in (("fp64", torch.float64), ("fp32", torch.float32)):
        sd = torch.full(res, 100.0, dtype=dt, device=dev)
        vel = torch.zeros(res + (3,), dtype=dt, device=dev)
        union = lambda: sdf.union_mesh_grid(rb, [body], sd, vel, (-0.5, 0.0, -0.5), (h, h, h), (0, 0, 0), rb_w=w)  # noqa: E731

        # sd = 100 everywhere before every timed call: the body wins EVERY node, sd and vel are written everywhere
        ms_all, spread_all = timed(union, reset=lambda: sd.fill_(100.0))
        union()
        ms_none, spread_none = timed(union)     # sd holds the body already: no node is won, nothing is written
        print(json.dumps(dict(op="union_mesh_grid", grid=list(res), dtype=name, ms_every_node_won=ms_all,
                              spread_every=spread_all, ms_no_node_won=ms_none, spread_none=spread_none,
                              inside=int((sd < 0).sum().item()))), flush=True)
        del sd, vel
    P = 256 ** 3
    x0 = torch.rand((P, 3), dtype=torch.float64, device=dev) - torch.tensor([0.5, 0.0, 0.5], dtype=torch.float64, device=dev)
    x = x0.clone()

    # every timed call starts from the same positions; the copy that restores them is outside the timed region
    ms, spread = timed(lambda: sdf.project_mesh(rb, [body], x), reset=lambda: x.copy_(x0))
    print(json.dumps(dict(op="project_mesh", particles=P, dtype="fp64", ms=ms, spread=spread,
                          moved=int((x != x0).any(dim=1).sum().item()))), flush=True)


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), N=N, repeats=REPEATS)), flush=True)
    v, f = M.icosphere(6, 0.3)
    ico = bench_build("icosphere6", surface.Mesh(torch.as_tensor(v, device=dev), torch.as_tensor(f, device=dev)), N)
    try:
        bench_build("dam_break_surface", dam_break_mesh(), N)
    except ValueError as e:                                  # build() refuses a surface it finds open: report, go on
        print(json.dumps(dict(mesh="dam_break_surface", error=str(e))), flush=True)
    bench_bodies(ico)
