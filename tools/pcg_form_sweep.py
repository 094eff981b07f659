"""Fingerprint of the pressure engine across its march and loop forms, for A/B runs of two builds of the library that must
compute the same bits (MFS_LIB selects the build; run once per build, diff the outputs).

One line per configuration: its name, mfs_pcg3d_loop_info, the iteration count and a SHA-256 over the bytes of the history
and of x, d, r, q.  Group `solve`: mfs_pcg3d_solve.  Group `iter`: begin / iterate / finish.  Group `apply`: the stencil
launch alone (aligned operands, and a view one element off a 16-byte boundary: the scalar path).

Ball-in-a-box problems on the smallest grids at which the march can still go wrong: (12, 40, 32) -- several tiles per plane,
the last one partial --, the golden grid (24, 20, 16), and (12, 40, 33), where Nz is no multiple of the vector width.  Lists
are forced with MFS_SPARSE_MIN=0 and a look every 4 iterations, so that the lane-mask form is taken after the first look.

usage: [MFS_LIB=path/to/libmfs_hip.so] python tools/pcg_form_sweep.py > out.txt"""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "python-fluid-simulation_amd"))
from mfs import _lib  # noqa: E402
from mfs.pcg import PcgEngine  # noqa: E402

DEV = torch.device("cuda:0")
G_TILES, G_GOLDEN, G_SCALAR = (12, 40, 32), (24, 20, 16), (12, 40, 33)
DTS = {"f32": torch.float32, "f64": torch.float64}
TOL = {"f32": 1e-3, "f64": 1e-6}
# (fuse, lean, defer_x): the launch-per-phase loop forms
LOOPS = {"plain": (False, False, False), "fused": (True, False, False), "fused+xdef": (True, False, True),
         "lean": (True, True, False), "lean+xdef": (True, True, True)}


def blob_problem(gres, seed):
    """a ball of liquid in an otherwise empty box: lphi, unit weights with a few quarter weights, a random right-hand side in
    the liquid (fp64; cast per configuration)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ax = [torch.arange(n, device=DEV, dtype=torch.float64) + 0.5 for n in gres]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    c, radius = [n / 2.0 for n in gres], 0.38 * min(gres)
    lphi = torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - radius

    def w(shape):
        q = torch.randint(1, 5, shape, generator=g, device=DEV).double() * 0.25
        return torch.where(torch.rand(shape, generator=g, device=DEV) < 0.9, torch.ones(shape, dtype=torch.float64, device=DEV), q)
    wx, wy, wz = w((gres[0] + 1, gres[1], gres[2])), w((gres[0], gres[1] + 1, gres[2])), w((gres[0], gres[1], gres[2] + 1))
    b = torch.randn(gres, generator=g, device=DEV, dtype=torch.float64) * (lphi < 0)
    b[0] = 0; b[-1] = 0; b[:, 0] = 0; b[:, -1] = 0; b[:, :, 0] = 0; b[:, :, -1] = 0
    return lphi, wx, wy, wz, b


_problems = {}


def problem(gres):
    if gres not in _problems:
        _problems[gres] = blob_problem(gres, 1 + len(_problems))
    return _problems[gres]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


def engine(gres, dtn, op, variant=2, nt=0, compress=True, pd=1, loop="fused", jacobi=False, resident=False):
    dt = DTS[dtn]
    lphi, wx, wy, wz, b = problem(gres)
    eng = PcgEngine(gres, dt, DEV)
    (eng.setup_density if op == "density" else eng.setup)(lphi.to(dt), wx.to(dt), wy.to(dt), wz.to(dt))
    eng.tune(variant=variant, nontemporal=nt)
    eng.set_compress(compress)
    eng.set_prefetch(pd)
    fuse, lean, defer = LOOPS[loop]
    eng.set_fuse(fuse)
    eng.set_lean(lean)
    eng.set_defer_x(defer)
    eng.set_jacobi(jacobi)
    eng.set_resident(resident)
    x, d, r, q = (torch.zeros(gres, dtype=dt, device=DEV) for _ in range(4))
    q[1:-1, 1:-1, 1:-1] = 5.0                  # stale q: begin must overwrite every computed cell
    eng.bind(b.to(dt), x, d, r, q)
    return eng, (x, d, r, q)


def report(group, name, eng, it, vecs, extra=""):
    torch.cuda.synchronize()
    bits = int(eng.lib.mfs_pcg3d_loop_info(eng.h))
    print(f"{group} {name} loop_info={bits} iters={it} {extra}sha256={digest(eng.history(), *vecs)}", flush=True)


def name_of(gres, dtn, op, **kw):
    return "x".join(map(str, gres)) + f" {dtn} {op} " + " ".join(f"{k}={v}" for k, v in kw.items())


def run_solve(gres, dtn, op, max_iter=2000, check_every=16, solves=1, lists=False, **kw):
    eng, vecs = engine(gres, dtn, op, **kw)
    for s in range(solves):
        if s:
            for v in vecs:
                v.zero_()
        ok, it = eng.solve(TOL[dtn], max_iter, check_every)
        extra = ""
        if lists:      # the lane-mask decision of this solve's lists, as tests/test_pressure_gpu.py asserts it
            info = eng.sparse_info()
            assert info["listed_pairs"] > 0 and info["live_chunks"] > 0, info
            assert float(eng.scalars[_lib.S_LANE]) == 1.0
            extra = f"listed={info['listed_pairs']}/{info['pairs']} "
        report("solve", name_of(gres, dtn, op, max_iter=max_iter, every=check_every, solve=s, **kw), eng, it, vecs,
               f"converged={int(ok)} " + extra)


def run_iter(gres, dtn, op, native=False, **kw):
    eng, vecs = engine(gres, dtn, op, **kw)
    eng.begin(TOL[dtn])
    if native:
        for _ in range(6):
            eng.native_apply()
            eng.native_finish()
    else:
        eng.iterate(5)
        eng.iterate(3)
    eng.finish()
    report("iter", name_of(gres, dtn, op, native=int(native), **kw), eng, eng.poll()["iterations"], vecs)


def run_apply(gres, dtn, op, misaligned, xr=None, **kw):
    eng, _ = engine(gres, dtn, op, **kw)
    dt, n = DTS[dtn], int(np.prod(gres))
    g = torch.Generator(device=DEV).manual_seed(7)
    off = 1 if misaligned else 0
    v = torch.randn(n + off, generator=g, device=DEV, dtype=torch.float64).to(dt)[off:].view(gres)
    out = torch.full((n + off,), 7.0, dtype=dt, device=DEV)[off:].view(gres)
    eng.apply(v, out, *(xr or (None, None)))
    torch.cuda.synchronize()
    print(f"apply {name_of(gres, dtn, op, misaligned=int(misaligned), range=xr, **kw)} sha256={digest(out)}", flush=True)


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"# library: {os.path.basename(_lib.LIB_PATH)}", file=sys.stderr)
    ops, dts = ("pressure", "density"), ("f32", "f64")
    # -- solve: every launch-per-phase loop x nt x compress x prefetch at the LDS march; the marches without LDS; partial nt masks
    for op, dtn in itertools.product(ops, dts):
        for loop, nt, comp, pd in itertools.product(LOOPS, (0, 7), (True, False), (1, 2)):
            run_solve(G_TILES, dtn, op, loop=loop, nt=nt, compress=comp, pd=pd)
        for variant, nt in itertools.product((0, 1), (0, 7)):
            run_solve(G_TILES, dtn, op, loop="plain", variant=variant, nt=nt)
        for nt in (1, 3, 5):
            run_solve(G_TILES, dtn, op, loop="plain", nt=nt, compress=False)
        for loop in LOOPS:
            run_solve(G_GOLDEN, dtn, op, loop=loop)
            run_solve(G_TILES, dtn, op, loop=loop, max_iter=7, check_every=4)      # stops on max_iter
        for loop, jac in (("plain", True), ("fused", True), ("fused+xdef", True)):
            run_solve(G_TILES, dtn, op, loop=loop, jacobi=jac)
        # the scalar path (Nz no multiple of the vector width): every loop request ends in the three-launch loop
        for variant, nt, pd in itertools.product((0, 1, 2), (0, 7), (1, 2)):
            run_solve(G_SCALAR, dtn, op, loop="lean", variant=variant, nt=nt, pd=pd)
        for nt in (1, 3, 5):
            run_solve(G_SCALAR, dtn, op, loop="plain", nt=nt)
        run_solve(G_SCALAR, dtn, op, loop="plain", jacobi=True)
    # -- the resident loop: one configuration each for the plain and the Jacobi iteration
    run_solve(G_GOLDEN, "f64", "pressure", loop="lean", resident=True)
    run_solve(G_GOLDEN, "f64", "pressure", loop="fused", jacobi=True, resident=True)
    # -- forced lists, a look every 4 iterations: the listed launches take the lane-mask form after the first look; a second solve
    # through the same engine starts with it (and with the first batch sized by the first solve)
    os.environ["MFS_SPARSE_MIN"] = "0"
    for op, dtn in itertools.product(ops, dts):
        for loop, nt in itertools.product(("fused", "fused+xdef", "lean", "lean+xdef"), (0, 7)):
            run_solve(G_TILES, dtn, op, loop=loop, nt=nt, check_every=4, solves=2, lists=True)
        for loop in ("fused", "fused+xdef"):
            run_solve(G_TILES, dtn, op, loop=loop, jacobi=True, check_every=4, solves=2, lists=True)
        run_solve(G_GOLDEN, dtn, op, loop="lean+xdef", check_every=4, solves=2, lists=True)
    del os.environ["MFS_SPARSE_MIN"]
    # -- begin / iterate / finish
    for op, dtn in itertools.product(ops, dts):
        for loop in LOOPS:
            run_iter(G_TILES, dtn, op, loop=loop)
            run_iter(G_TILES, dtn, op, loop=loop, native=True)
        for loop in ("plain", "fused", "fused+xdef"):
            run_iter(G_TILES, dtn, op, loop=loop, jacobi=True)
        run_iter(G_TILES, dtn, op, loop="fused", pd=2)
        run_iter(G_SCALAR, dtn, op, loop="lean+xdef")
    run_iter(G_GOLDEN, "f64", "pressure", loop="lean", resident=True)
    run_iter(G_GOLDEN, "f64", "pressure", loop="fused", jacobi=True, resident=True)
    # -- the stencil launch alone
    for op, dtn, mis in itertools.product(ops, dts, (False, True)):
        for variant, nt, comp, pd in itertools.product((0, 1, 2), (0, 1, 3, 5, 7), (True, False), (1, 2)):
            run_apply(G_TILES, dtn, op, mis, variant=variant, nt=nt, compress=comp, pd=pd)
        run_apply(G_TILES, dtn, op, mis, xr=(3, 7))
        run_apply(G_GOLDEN, dtn, op, mis)
        run_apply(G_SCALAR, dtn, op, mis)


if __name__ == "__main__":
    main()
