"""Fingerprint of the viscosity engine across its stencil-launch and loop forms, for A/B runs of two builds of the library
that must compute the same bits (MFS_LIB selects the build; run once per build, diff the outputs).

One line per configuration: its name, mfs_vcg3d_loop_info, mfs_vcg3d_apply_kernel, the iteration count and a SHA-256 over
the bytes of the history and of x, d, r, q.  Group `solve`: mfs_vcg3d_solve.  Group `iter`: begin / iterate / finish.
Group `apply`: the stencil launch alone -- the masked stand-alone apply and the loop's unmasked launch (phase_apply) -- on
aligned operands and on a view one element off a 16-byte boundary.

mfs.scenes.viscosity_scene_3d on the smallest grids at which each form can still go wrong: (12, 40, 32) -- two fp32 / three
fp64 march tiles per plane, the last one partial --, (12, 40, 33) -- the scalar path --, (10, 14, 256) and (6, 10, 512) --
the 512-thread and 3-slot geometries --, (2, 5, 8) and (5, 2, 8) -- per-row launches --, (9, 11, 13) -- the smallest grid
tests/test_viscosity_resident_gpu.py runs resident.  The environment knobs of a configuration stay set from the engine's
creation to its last call, so a build that reads them per call and one that reads them at creation see the same values.

usage: [MFS_LIB=path/to/libmfs_hip.so] python tools/vcg_form_sweep.py > out.txt"""
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "python-fluid-simulation_amd"))
from mfs import _lib, scenes  # noqa: E402
from mfs.vcg import VcgEngine  # noqa: E402
import solver.ViscosityCGSolver3D as V  # noqa: E402

DEV = torch.device("cuda:0")
G_TILES, G_SCALAR, G_512, G_RING3 = (12, 40, 32), (12, 40, 33), (10, 14, 256), (6, 10, 512)
G_ROWS_A, G_ROWS_B, G_RESIDENT = (2, 5, 8), (5, 2, 8), (9, 11, 13)
GRIDS = (G_TILES, G_SCALAR, G_512, G_RING3, G_ROWS_A, G_ROWS_B, G_RESIDENT)
DTS = {"f32": torch.float32, "f64": torch.float64}
TOL, MU = {"f32": 1e-3, "f64": 1e-6}, 40.0
# loop -> (jacobi, fuse, split_x, resident, merged, MFS_VISC_JACOBI_Z)
LOOPS = {"plain": (0, 0, 1, 0, 0, None), "plain-nosplit": (0, 0, 0, 0, 0, None), "merged": (0, 0, 1, 0, 1, None),
         "fused": (0, 1, 1, 0, 0, None), "resident": (0, 0, 1, 1, 1, None), "jacobi-z0": (1, 0, 1, 0, 0, "0"),
         "jacobi-z1": (1, 0, 1, 0, 0, "1")}
KNOB_ENV = {"march": "MFS_VISC_MARCH", "block": "MFS_VISC_MARCH_BLOCK", "nt": "MFS_VISC_MARCH_NT", "compress": "MFS_VISC_COMPRESS"}

_problems = {}


def problem(gres):
    """the scene, the operator's scale and volume fractions, the extrapolated start and the right-hand side (fp64)"""
    if gres not in _problems:
        sc = scenes.viscosity_scene_3d(gres, seed=5, device=DEV, noise=0.3)
        cell_vol = float(np.prod(np.array(sc["bound_size"]) / np.array(gres)))
        scale = sc["dt"] / cell_vol / sc["rho"]
        vol = sc["lvol"] / (cell_vol * 0.125)
        x = [sc[k].double().clone() for k in ("vx", "vy", "vz")]
        V.extrapolate(gres, 3, *x, sc["sphi"])
        b = [torch.zeros_like(t) for t in x]
        V.initialize_solver(gres, scale, MU, *x, sc["sphi"], sc["sv"], vol, *b)
        flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])  # noqa: E731
        _problems[gres] = dict(sc=sc, scale=scale, vol=vol, x0=flat(x), b=flat(b))
    return _problems[gres]


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).tobytes())
    return h.hexdigest()


class Config:
    """the environment of one configuration, set for the engine's whole life"""

    def __init__(self, loop="plain", lists=False, **knobs):
        self.env = {KNOB_ENV[k]: str(v) for k, v in knobs.items() if v is not None}
        self.loop = LOOPS[loop]
        if self.loop[5] is not None:
            self.env["MFS_VISC_JACOBI_Z"] = self.loop[5]
        self.env["MFS_VISC_SPLIT_X"] = str(self.loop[2])
        if lists:
            self.env["MFS_VISC_SPARSE_MIN"] = "0"

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def engine(self, gres, dtn, misaligned=False):
        dt, p = DTS[dtn], problem(gres)
        eng = VcgEngine(gres, dt, DEV)
        jac, fuse, _, res, merged, _ = self.loop
        eng.set_jacobi(jac)
        eng.set_fuse(fuse)
        eng.set_resident(res)
        eng.set_merged(merged)
        eng.setup(p["scale"], MU, p["sc"]["sphi"], p["vol"])
        off = 1 if misaligned else 0
        b, x, d, r, q = (torch.zeros(eng.dofs + off, dtype=dt, device=DEV)[off:] for _ in range(5))
        b.copy_(p["b"])
        x.copy_(p["x0"])
        o = 0
        for shp in eng.face_shapes:                # stale q: begin must overwrite every computed face (the interior ones;
            n = int(np.prod(shp))                  # array-boundary faces have no equation and keep q = r = d = 0)
            q[o:o + n].view(shp)[1:-1, 1:-1, 1:-1] = 5.0
            o += n
        eng.bind(b, x, d, r, q)
        return eng, (x, d, r, q)


def name_of(gres, dtn, **kw):
    return "x".join(map(str, gres)) + f" {dtn} " + " ".join(f"{k}={v}" for k, v in kw.items())


def report(group, name, eng, it, vecs, extra=""):
    torch.cuda.synchronize()
    print(f"{group} {name} loop_info={int(eng.lib.mfs_vcg3d_loop_info(eng.h))} apply_kernel={int(eng.lib.mfs_vcg3d_apply_kernel(eng.h))} "
          f"iters={it} {extra}sha256={digest(eng.history(), *vecs)}", flush=True)


def run_solve(gres, dtn, max_iter=2000, check_every=16, **kw):
    with Config(**kw) as cfg:
        eng, vecs = cfg.engine(gres, dtn)
        try:
            ok, it = eng.solve(TOL[dtn], max_iter, check_every)
            extra = f"converged={int(ok)} "
        except (_lib.MfsNonFinite, _lib.MfsZeroDivision) as e:      # an outcome of the solve (an empty system, say): part of the fingerprint
            it, extra = eng.poll_raw()["iterations"], f"stopped={type(e).__name__} "
        if kw.get("lists"):
            info = eng.sparse_info()
            extra += f"live={info['live_chunks']}/{info['chunks']} listed={info['listed_pairs']}/{info['pairs']} "
        report("solve", name_of(gres, dtn, max_iter=max_iter, **kw), eng, it, vecs, extra)


def run_iter(gres, dtn, **kw):
    with Config(**kw) as cfg:
        eng, vecs = cfg.engine(gres, dtn)
        eng.begin(TOL[dtn])
        eng.iterate(5)
        eng.iterate(3)
        try:
            eng.finish()
            it, extra = eng.poll()["iterations"], ""
        except (_lib.MfsNonFinite, _lib.MfsZeroDivision) as e:
            it, extra = eng.poll_raw()["iterations"], f"stopped={type(e).__name__} "
        report("iter", name_of(gres, dtn, **kw), eng, it, vecs, extra)


def run_apply(gres, dtn, misaligned, **kw):
    """the masked stand-alone apply of the start vector, then the loop's unmasked launch on a direction vector (random on
    non-solid interior faces, exactly 0 elsewhere) with its d.q"""
    with Config(**kw) as cfg:
        eng, (x, d, r, q) = cfg.engine(gres, dtn, misaligned)
        eng.apply(x, r)
        sphi = problem(gres)["sc"]["sphi"]
        valid = [sphi[0::2, 1::2, 1::2] >= 0, sphi[1::2, 0::2, 1::2] >= 0, sphi[1::2, 1::2, 0::2] >= 0]
        gen, o = torch.Generator(device=DEV).manual_seed(11), 0
        for shp, m in zip(eng.face_shapes, valid):
            n = int(np.prod(shp))
            t = d[o:o + n].view(shp)
            inner = t[1:-1, 1:-1, 1:-1]
            inner.copy_(torch.randn(inner.shape, generator=gen, device=DEV, dtype=torch.float64))
            t.mul_(m)
            o += n
        kernel = int(eng.lib.mfs_vcg3d_apply_kernel(eng.h))
        eng.phase_apply()
        eng.phase_reduce(0)
        torch.cuda.synchronize()
        dq = float(eng.scalars[_lib.S_DQ])
        print(f"apply {name_of(gres, dtn, misaligned=int(misaligned), **kw)} apply_kernel={kernel} "
              f"sha256={digest(r, q, np.array([dq]))}", flush=True)


def march_knobs():
    """march on / off x block knob auto / 256 / 512 / 5123 x nontemporal -1 / 0 / 1 x compress on / off"""
    yield dict(march=0)
    for block, nt, compress in itertools.product((None, 256, 512, 5123), (-1, 0, 1), (1, 0)):
        yield dict(march=1, block=block, nt=nt, compress=compress)


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    print(f"# library: {os.path.basename(_lib.LIB_PATH)}", file=sys.stderr)
    for gres, dtn in itertools.product(GRIDS, DTS):
        # -- solve: the launch knobs under the plain loop; every loop with and without forced lists; the fused march's
        # geometries; a max_iter that stops early
        for kn in march_knobs():
            run_solve(gres, dtn, loop="plain", **kn)
        for loop, lists in itertools.product(LOOPS, (False, True)):
            run_solve(gres, dtn, loop=loop, lists=lists)
        for block, nt in itertools.product((256, 512, 5123), (0, 1)):
            run_solve(gres, dtn, loop="fused", block=block, nt=nt)
        for loop in ("plain", "merged", "fused", "resident", "jacobi-z0"):
            run_solve(gres, dtn, loop=loop, max_iter=7, check_every=4)
        run_solve(gres, dtn, loop="plain", lists=True, compress=0)
        run_solve(gres, dtn, loop="plain", lists=True, march=0)
        # -- begin / iterate / finish
        for loop, lists in itertools.product(LOOPS, (False, True)):
            run_iter(gres, dtn, loop=loop, lists=lists)
        # -- the stencil launch alone
        for mis in (False, True):
            for kn in march_knobs():
                run_apply(gres, dtn, mis, **kn)


if __name__ == "__main__":
    main()
