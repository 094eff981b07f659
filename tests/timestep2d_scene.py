"""The dam-break scene of the 2D time-step tests (numpy only, test helper): a flipped box one cell inside the bounds (the
container), one ramp box rotated by -35 degrees, and a block of liquid at about 4 jittered particles per cell (particle
spacing gdx / 2) held against the left wall above the ramp, with a sheared initial velocity `pv`.  `bodies` is what to hand to solver.sdf2D.generate_rb, `rb_d`
the same bodies in its packed (n, 8, 3) layout."""
import numpy as np

from mfs import scenes


def dam_break(gres=(24, 32), seed=0, gdx=0.05, bound_min=(-0.3, 0.0), mu=1.0):
    Nx, Ny = (int(v) for v in gres)
    bmin = np.asarray(bound_min, np.float64)
    size = np.array([Nx, Ny], np.float64) * gdx
    ctr = bmin + 0.5 * size
    bodies = [
        dict(name="tank", rbparam=["box", float(size[0] - 2 * gdx), float(size[1] - 2 * gdx)], flip=True,
             center=[float(ctr[0]), float(ctr[1])], angle=0),
        dict(name="ramp", rbparam=["box", float(0.375 * size[0]), float(gdx)], flip=False,
             center=[float(bmin[0] + 0.35 * size[0]), float(bmin[1] + 0.15 * size[1])], angle=-35),
    ]
    rb_d = np.stack([scenes._rb2(b["rbparam"][0], b["rbparam"][1:], b["flip"], b["center"], b["angle"]) for b in bodies])
    pdx = gdx / 2
    lo = bmin + np.array([1.0 * gdx, 0.40 * size[1]])            # flush with the left wall: the jitter puts some inside it
    hi = bmin + np.array([0.45 * size[0], 0.80 * size[1]])
    dims = np.floor((hi - lo) / pdx).astype(np.int64)
    ii, jj = np.meshgrid(np.arange(dims[0]), np.arange(dims[1]), indexing="ij")
    pos = lo + (np.stack([ii, jj], axis=-1).reshape(-1, 2) + 0.5) * pdx
    rng = np.random.default_rng(seed + 5000)
    px = pos + rng.standard_normal(pos.shape) * pdx * 0.3
    # a sheared start, so that the viscosity solve has work to do from the first step on
    pv = np.stack([0.5 + np.sin(6.0 * px[:, 1]), -0.3 * np.cos(5.0 * px[:, 0])], axis=1)
    return dict(gres=(Nx, Ny), gdx=float(gdx), bound_min=tuple(float(b) for b in bmin), bodies=bodies, rb_d=rb_d, px=px, pv=pv,
                pdx=float(pdx), mu=float(mu), box=(bmin + gdx, bmin + size - gdx))
