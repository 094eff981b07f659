"""GPU: time of mfs.surface.isosurface on the two fields a NotebookSimulation user extracts -- a pool-like liquid level set
on the N^3 cell grid (closed, background 3 * GDX, as `sim.surface("liquid")` calls it) and a solid level set on the
(2N+1)^3 doubled grid (a container, a slanted plate and a ball; open, as `sim.surface("solid")`).
The count pass and the fill pass are timed apart with device events: REPEATS windows, each of at least WINDOW_S seconds
of back-to-back calls after a warm-up; reported per pass: median and spread = (max - min) / median over the windows.
`call_ms` is the whole `isosurface()` call on the host clock (count, the host sync that reads the totals, allocation,
fill), median of REPEATS; `phi_GBps` = bytes of phi / call time.
usage: python tools/bench_surface.py N [fp32|fp64]   -- one JSON line per field"""
import json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "python-fluid-simulation_amd"), REPO]
import numpy as np, torch
from mfs import _lib, surface, tensors as T
REPEATS, WINDOW_S = 7, 0.2
dev = "cuda:0"
assert torch.cuda.is_available(), "bench_surface.py measures on the GPU; there is no CPU path"
torch.cuda.set_device(dev)


def axes(res, lo, h):
    return [lo[d] + h * torch.arange(res[d], dtype=torch.float64, device=dev).reshape([-1 if a == d else 1 for a in range(3)])
            for d in range(3)]


def liquid_field(N, dtype):
    """a pool filling the lower 40 % of the unit box with a rippled top, two drops above it; clipped at 3 GDX like the
    level set of the time step.  Cell centres."""
    gdx = 1.0 / N
    x, y, z = axes((N,) * 3, (-0.5 + gdx / 2, gdx / 2, -0.5 + gdx / 2), gdx)
    pool = y - (0.4 + 0.03 * torch.sin(9 * x) * torch.cos(7 * z))
    drop = lambda c, r: torch.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2) - r  # noqa: E731
    phi = torch.minimum(pool, torch.minimum(drop((0.1, 0.7, -0.2), 0.08), drop((-0.25, 0.6, 0.2), 0.05)))
    return torch.clamp(phi, max=3 * gdx).to(dtype).contiguous(), dict(origin=(-0.5 + gdx / 2, gdx / 2, -0.5 + gdx / 2), spacing=gdx,
                                                                      closed=True, outside=3 * gdx)


def solid_field(N, dtype):
    """the container (outside of a box two cells inside the bounds), a plate slanted by 35 degrees, a ball.  Doubled nodes."""
    gdx = 1.0 / N
    x, y, z = axes((2 * N + 1,) * 3, (-0.5, 0.0, -0.5), gdx / 2)
    hx = 0.5 - 2 * gdx
    qx, qy, qz = x.abs() - hx, (y - 0.5).abs() - hx, z.abs() - hx
    box = torch.sqrt(qx.clamp(min=0) ** 2 + qy.clamp(min=0) ** 2 + qz.clamp(min=0) ** 2) + torch.maximum(qx, torch.maximum(qy, qz)).clamp(max=0)
    c, s = np.cos(np.radians(35)), np.sin(np.radians(35))
    u, v = c * (x + 0.1) + s * (y - 0.25), -s * (x + 0.1) + c * (y - 0.25)
    px, py, pz = u.abs() - 0.25, v.abs() - 0.025, z.abs() - 0.4
    plate = torch.sqrt(px.clamp(min=0) ** 2 + py.clamp(min=0) ** 2 + pz.clamp(min=0) ** 2) + torch.maximum(px, torch.maximum(py, pz)).clamp(max=0)
    ball = torch.sqrt((x - 0.2) ** 2 + (y - 0.55) ** 2 + z ** 2) - 0.12
    phi = torch.minimum(-box, torch.minimum(plate, ball))
    return phi.to(dtype).contiguous(), dict(origin=(-0.5, 0.0, -0.5), spacing=gdx / 2)


def windows(fn):
    """per-call ms of fn over REPEATS windows of back-to-back calls between two device events"""
    fn(); fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    k = max(3, int(np.ceil(WINDOW_S / max(time.perf_counter() - t0, 1e-6))))
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / k)
    return out


def stats(v):
    v = np.asarray(v)
    return round(float(np.median(v)), 4), round(float((v.max() - v.min()) / np.median(v)), 3)


def case(name, phi, kw):
    lib = _lib.load()
    shape = tuple(phi.shape)
    closed, outside = int(kw.get("closed", False)), float(kw.get("outside") or 0.0)
    g = _lib.i64x(shape)
    nbytes = int(lib.mfs_surface3d_workspace_bytes(g, closed))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    common = (g, T.ptr(phi), T.code(phi), 0.0, closed, outside)
    count = lambda: _lib.check(lib.mfs_surface3d_count(*common, T.ptr(ws), nbytes, T.stream()), "count")  # noqa: E731
    count()
    nv, nf = (int(v) for v in ws[:16].view(torch.int64).tolist())
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    faces = torch.empty((nf, 3), dtype=torch.int32, device=dev)
    org, sp = _lib.f64x(T.as_f64_list(kw["origin"], 3)), _lib.f64x(T.as_f64_list(kw["spacing"], 3))
    fill = lambda: _lib.check(lib.mfs_surface3d_fill(*common, org, sp, T.ptr(ws), nbytes, T.ptr(verts), nv, T.ptr(faces), nf,  # noqa: E731
                                                     None, T.stream()), "fill")
    c_ms, c_sp = stats(windows(count))
    f_ms, f_sp = stats(windows(fill))
    calls = []
    for r in range(REPEATS + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = surface.isosurface(phi, 0.0, **kw)
        torch.cuda.synchronize()
        calls.append((time.perf_counter() - t0) * 1e3)
    call_ms, call_sp = stats(calls[2:])
    assert m.vertices.shape[0] == nv and m.faces.shape[0] == nf and torch.equal(m.vertices, verts) and torch.equal(m.faces, faces)
    pb = phi.numel() * phi.element_size()
    print(json.dumps(dict(field=name, shape=shape, dtype=str(phi.dtype).replace("torch.", ""), closed=bool(closed), V=nv, F=nf,
                          count_ms=c_ms, count_spread=c_sp, fill_ms=f_ms, fill_spread=f_sp, call_ms=call_ms, call_spread=call_sp,
                          phi_GBps=round(pb / (call_ms * 1e-3) / 1e9, 1), workspace_MiB=round(nbytes / 2 ** 20, 1),
                          device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    dtype = T.state_dtype(sys.argv[2] if len(sys.argv) > 2 else "fp64")
    for name, make in (("liquid", liquid_field), ("solid", solid_field)):
        phi, kw = make(N, dtype)
        case(name, phi, kw)
        del phi
