"""numpy restatement of the 2D time step's particle <-> grid transfers and grid kernels (csrc/mfs_notebook2d.hip,
notebook_kernels2d.py), test helper.

The reference has no 2D driver, so there is nothing to execute for goldens: these functions are oracle/mfs_oracle.py's
nb_* restatements of the 3D notebook cells (which the executed-reference goldens pin) with the z factor / z terms removed,
every remaining statement in the same order -- float32 position, float32 grid position, float32 weight, float64 after
that.  tests/test_notebook2d_oracle.py pins them to the 3D oracle by dimension reduction.  Scatters add in particle order
in the dtype of the target array; `stats` (a dict) receives K and S_<name> per node as oracle.mfs_oracle._scatter_stats
gives them.  `step()` composes them with the oracle's 2D pressure solve, tests/visc2d_numpy.py and tests/density2d_numpy.py
into one time step of notebook_sim2d.NotebookSimulation2D.
"""
import types

import numpy as np

import density2d_numpy as D2
import visc2d_numpy as V2
from oracle import mfs_oracle as O

F32, F64 = np.float32, np.float64


def _cell(px, bound_min, cell_size, bias, centre_offset=None):
    """float32 position, base index, float32 grid position"""
    x32 = np.asarray(px).astype(F32)
    bmin32, cs = np.asarray(bound_min, F32), np.asarray(cell_size, F64)
    t = (x32 - bmin32).astype(F64) / cs                       # float32 difference, float64 quotient
    if bias is not None:
        t = t - np.asarray(bias, F32).astype(F64)
    gi = np.floor(t).astype(np.int64)
    off = np.asarray(bias, F32).astype(F64) if centre_offset is None else centre_offset
    gx32 = ((gi + off) * cs + bmin32.astype(F64)).astype(F32)
    return x32, gi, gx32


def p2g_scatter(px, pm, pv, pca, gm, gv, bound_min, gres, grid_bias, cell_size, axis, stats=None):
    """APIC scatter of mass and momentum of component `axis` to its face array; indices clamped to gres - 1"""
    Nx, Ny = (int(g) for g in gres)
    cs = np.asarray(cell_size, F64)
    x32, gi, gx32 = _cell(px, bound_min, cs, grid_bias)
    disp = gx32 - x32                                          # float32
    w = (np.abs(disp).astype(F64) / cs).astype(F32).astype(F64)
    v32 = np.asarray(pv).astype(F32)
    m, pca = np.asarray(pm, F64), np.asarray(pca, F64)
    d64 = disp.astype(F64)
    for ix in (0, 1):
        for iy in (0, 1):
            cx = np.clip(gi[:, 0] + ix, 0, Nx - 1)
            cy = np.clip(gi[:, 1] + iy, 0, Ny - 1)
            wx = ix + ((-1) ** ix) * (1 - w[:, 0])
            wy = iy + ((-1) ** iy) * (1 - w[:, 1])
            cv = (d64[:, 0] + ix * cs[0]) * pca[:, 0] + (d64[:, 1] + iy * cs[1]) * pca[:, 1]
            weight = wx * wy
            tm, tv = weight * m, weight * m * (v32[:, axis].astype(F64) + cv)
            np.add.at(gm, (cx, cy), tm.astype(gm.dtype))
            np.add.at(gv, (cx, cy), tv.astype(gv.dtype))
            O._scatter_stats(stats, gm.shape, (cx, cy), m=tm, v=tv)


def p2g_normalize(gm, gv):
    m = gm > 0
    gv[m] = gv[m] / gm[m]


def g2p_gather(bound_min, gres, grid_bias, cell_size, axis, px, pv, pca, gv):
    """bilinear velocity into pv[:, axis] and the affine row into pca (P, 2): the 3D accumulation order on four corners,
    every partial sum in the dtype of `pv` / `pca`"""
    Nx, Ny = (int(g) for g in gres)
    cs = np.asarray(cell_size, F64)
    x32, gi, gx32 = _cell(px, bound_min, cs, grid_bias)
    w = (np.abs(gx32 - x32).astype(F64) / cs).astype(F32).astype(F64)
    pca[:, :] = 0
    vel = np.zeros(len(x32), dtype=pv.dtype)
    G = np.asarray(gv)
    for ix in (0, 1):
        for iy in (0, 1):
            cx = np.clip(gi[:, 0] + ix, 0, Nx - 1)
            cy = np.clip(gi[:, 1] + iy, 0, Ny - 1)
            wx = 1 - ix + (2 * ix - 1) * w[:, 0]
            wy = 1 - iy + (2 * iy - 1) * w[:, 1]
            g = G[cx, cy].astype(F64)
            vel = (vel + wx * wy * g).astype(pv.dtype)
            pca[:, 0] += (2 * ix - 1) * wy * g / cs[0]
            pca[:, 1] += wx * (2 * iy - 1) * g / cs[1]
    pv[:, axis] = vel


def default_radius(gdx):
    """the cell's half diagonal with the notebook's 2 % margin (3D: sqrt(3))"""
    return gdx * 0.5 * np.sqrt(2.0) * 1.02


def fluid_levelset(px, phi, bound_min, cell_size, gdx, gres, radius=None):
    """phi = gdx * 3, then min over particles within +-2 cells of |centre - x| - radius"""
    Nx, Ny = (int(g) for g in gres)
    cs = np.asarray(cell_size, F64)
    r = default_radius(gdx) if radius is None else radius
    phi[...] = gdx * 3
    x32, gi, _ = _cell(px, bound_min, cs, None, centre_offset=0.5)
    bmin = np.asarray(bound_min, F32).astype(F64)
    x64 = x32.astype(F64)
    for dx in range(-2, 3):
        for dy in range(-2, 3):
            ii = np.stack([np.clip(gi[:, 0] + dx, 0, Nx - 1), np.clip(gi[:, 1] + dy, 0, Ny - 1)], axis=1)
            gip = ((ii + 0.5) * cs + bmin - x64).astype(F32)
            n = np.zeros(len(x32))
            for d in range(2):
                n = n + (gip[:, d] * gip[:, d]).astype(F64)           # float32 product, float64 sum
            np.minimum.at(phi, (ii[:, 0], ii[:, 1]), n ** 0.5 - r)


def volume_clamp(cell_size):
    """what a node of the doubled grid can hold: its cell's area cs_x * cs_y"""
    cs = np.asarray(cell_size, F64)
    return float(cs[0] * cs[1])


def fluid_volume(bound_min, cell_size, vres, px, pvol, gvol, stats=None):
    """bilinear splat of the particle volume onto the doubled-grid nodes (shape vres, spacing cell_size), clamped to
    `volume_clamp(cell_size)`; `stats` describes the splat before the clamp"""
    Nx, Ny = (int(g) for g in vres)
    cs = np.asarray(cell_size, F64)
    gvol[...] = 0.0
    x32, gi, gx32 = _cell(px, bound_min, cs, None, centre_offset=0.0)
    w = (np.abs(gx32 - x32).astype(F64) / cs).astype(F32).astype(F64)
    for ix in (0, 1):
        for iy in (0, 1):
            cx = np.clip(gi[:, 0] + ix, 0, Nx - 1)
            cy = np.clip(gi[:, 1] + iy, 0, Ny - 1)
            weight = (ix + ((-1) ** ix) * (1 - w[:, 0])) * (iy + ((-1) ** iy) * (1 - w[:, 1]))
            t = weight * float(pvol)
            np.add.at(gvol, (cx, cy), t.astype(gvol.dtype))
            O._scatter_stats(stats, gvol.shape, (cx, cy), vol=t)
    np.minimum(gvol, gvol.dtype.type(volume_clamp(cs)), out=gvol)


def extrapolate(gres, num_iter, vx, vy, mx, my):
    """Jacobi sweeps of the 4-neighbour average (+x, -x, +y, -y) into interior faces with mass <= 0; validity grows per
    sweep; a sweep reads the previous sweep only; arrays with an extent below 3 have no interior face"""
    valids = [np.asarray(mx) > 0, np.asarray(my) > 0]
    for _ in range(num_iter):
        for v, valid in zip((vx, vy), valids):
            n = v.shape
            if min(n) < 3:
                continue
            I = (slice(1, n[0] - 1), slice(1, n[1] - 1))
            val = np.zeros(tuple(s - 2 for s in n))
            count = np.zeros(val.shape, dtype=np.int64)
            for off in ((1, 0), (-1, 0), (0, 1), (0, -1)):
                sl = tuple(slice(1 + o, s - 1 + o) for o, s in zip(off, n))
                m = valid[sl]
                val = val + np.where(m, v[sl].astype(F64), 0.0)
                count = count + m
            upd = (~valid[I]) & (count > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                v[I] = np.where(upd, val / count, v[I].astype(F64)).astype(v.dtype)
            nv = valid.copy()
            nv[I] = valid[I] | upd
            valid[...] = nv


def boundary_condition(gres, gv, gm, sphi, sv, dx, dv):
    """free-slip correction dv = -(component of the solid-relative velocity's inward normal part) * (1 - sphi/dx) on interior
    faces closer than dx to a solid, 0 elsewhere.  gv, gm, dv: (x, y) pairs of face arrays; sv (2Nx+1, 2Ny+1, 2).  The other
    component is mass-averaged over four taps -- x face: (x-ix, y+iy); y face: (x+iz, y-iy) -- with the product formed in the
    arrays' own dtype; min(0, s) is `s if s < 0 else 0` (NaN -> 0)."""
    sphi = np.asarray(sphi, F64)
    sv = np.asarray(sv, F64)
    D0 = ((0, 1), (1, 0))
    taps = {0: (1, [(-ix, iy) for ix in range(2) for iy in range(2)]),
            1: (0, [(iz, -iy) for iy in range(2) for iz in range(2)])}
    for a in range(2):
        n = gv[a].shape
        dv[a][...] = 0
        if min(n) < 3:
            continue
        cnt = tuple(s - 2 for s in n)
        I = tuple(slice(1, 1 + c) for c in cnt)

        def dg(G, off, comp=None):
            sl = tuple(slice(2 + D0[a][k] + off[k], 2 + D0[a][k] + off[k] + 2 * cnt[k], 2) for k in range(2))
            return G[sl] if comp is None else G[sl + (comp,)]

        def sh(A, off):
            return np.asarray(A)[tuple(slice(1 + off[k], 1 + off[k] + cnt[k]) for k in range(2))]

        ndist = dg(sphi, (0, 0)) / dx
        vel = [None, None]
        vel[a] = sh(gv[a], (0, 0)).astype(F64)
        with np.errstate(divide="ignore", invalid="ignore"):
            comp, offs = taps[a]
            msum = np.zeros(cnt)
            vsum = np.zeros(cnt)
            for off in offs:
                m_ = sh(gm[comp], off)
                v_ = sh(gv[comp], off)
                msum = msum + m_.astype(F64)
                vsum = vsum + (v_ * m_).astype(F64)           # product in the arrays' own dtype
            vel[comp] = vsum / msum
            rel = [vel[c] - dg(sv, (0, 0), c) for c in range(2)]
            sn = [dg(sphi, (1, 0)) - dg(sphi, (-1, 0)), dg(sphi, (0, 1)) - dg(sphi, (0, -1))]
            sn_inv = 1.0 / (sn[0] ** 2 + sn[1] ** 2)
            s = sn[0] * rel[0] + sn[1] * rel[1]
            proj = np.where(s < 0, s, 0.0) * sn[a] * sn_inv
            out = -proj * (1.0 - ndist)
        dv[a][I] = np.where(ndist >= 1, 0.0, out).astype(dv[a].dtype)


# ----------------------------------------------------------------------------------------- the time step ---
BIAS = ((0, .5), (.5, 0))


def make_state(gres, gdx, bound_min, rb_d, px, pdx, rho=1000.0, mu=1.0, dt=1.0 / 300.0):
    """the containers of notebook_sim2d.NotebookSimulation2D on numpy arrays, with its dtypes"""
    g = tuple(int(v) for v in gres)
    bmin = np.asarray(bound_min, F32)
    bsz = (np.asarray(g, F64) * gdx).astype(F32)
    cs = bsz / np.asarray(g, np.int64)
    dres = tuple(2 * v + 1 for v in g)
    dcs = bsz / (2 * np.asarray(g, np.int64))
    idx = np.stack(np.meshgrid(*[np.arange(r, dtype=F32) for r in dres], indexing="ij"), axis=-1)
    pos = bmin.astype(F64) + (idx + np.zeros(2, F32)).astype(F64) * dcs
    sphi, sv = D2.sdf_evaluate(np.asarray(rb_d), pos)
    px = np.array(px, F64)
    n = len(px)
    fx, fy = (g[0] + 1, g[1]), (g[0], g[1] + 1)
    return types.SimpleNamespace(
        gres=g, gdx=float(gdx), rho=float(rho), mu=float(mu), DT=float(dt), bound_min=bmin, bound_size=bsz, cell_size=cs,
        dcell_size=dcs, dres=dres, rb_d=np.asarray(rb_d), sphi=sphi, sv=sv, pos=pos,
        px=px, pv=np.zeros((n, 2)), pcx=np.zeros((n, 2)), pcy=np.zeros((n, 2)), pm=np.full(n, rho * pdx ** 2), pvol=pdx ** 2,
        gm=[np.zeros(fx, F32), np.zeros(fy, F32)], gv=[np.zeros(fx, F32), np.zeros(fy, F32)],
        dv=[np.zeros(fx, F32), np.zeros(fy, F32)], lphi=np.zeros(g), lvol=np.zeros(dres),
        wx=np.zeros(fx), wy=np.zeros(fy), iters={})


def _levelset_and_volume(s):
    fluid_levelset(s.px, s.lphi, s.bound_min, s.cell_size, s.gdx, s.gres)
    fluid_volume(s.bound_min, s.dcell_size, s.dres, s.px, s.pvol, s.lvol)


def step(s, duration_left=float("inf")):
    """one pass of NotebookSimulation2D.step on the state of `make_state`, in place.  Returns dt."""
    vmax = np.sqrt((s.pv ** 2).sum(axis=-1)).max() if len(s.px) else 0.0
    dt = min(s.DT, s.gdx / max(1e-10, float(vmax)), duration_left)
    s.px += s.pv * dt
    D2.sdf_project(s.rb_d, s.px)
    _levelset_and_volume(s)
    D2.solid_frac(s.gres, s.sphi, s.wx, s.wy)
    out = D2.solve(s.gres, s.bound_min.astype(F64), s.bound_size.astype(F64), s.rho, dt, s.px, s.pm, s.sphi, s.lphi, s.lvol,
                   s.wx, s.wy, tol=1e-3)
    s.iters["density"] = out["iters"]
    _levelset_and_volume(s)
    for a in range(2):
        s.gm[a][...] = 0
        s.gv[a][...] = 0
    for a, pc in enumerate((s.pcx, s.pcy)):
        p2g_scatter(s.px, s.pm, s.pv, pc, s.gm[a], s.gv[a], s.bound_min, s.gres, BIAS[a], s.cell_size, a)
    for a in range(2):
        p2g_normalize(s.gm[a], s.gv[a])
    s.gv[1] += F32(-10 * dt)                                    # gravity, in the array's float32
    if s.mu > 0:
        out = V2.solve(s.gres, s.bound_size.astype(F64), dt, s.mu, s.rho, s.gv[0], s.gv[1], s.sphi, s.lvol, tol=1e-4)
        s.iters["viscosity"] = out["iters"]
    ps = O.PressureCGSolver2D(s.gres, s.bound_size.astype(F64))
    ps.solve(s.gv[0], s.gv[1], s.sphi, s.sv, s.lphi, wx=s.wx, wy=s.wy, tol=1e-3)
    s.iters["pressure"] = ps.iterations
    extrapolate(s.gres, 2, s.gv[0], s.gv[1], s.gm[0], s.gm[1])
    boundary_condition(s.gres, s.gv, s.gm, s.sphi, s.sv, s.gdx, s.dv)
    for a in range(2):
        s.gv[a] += s.dv[a]
    for a, pc in enumerate((s.pcx, s.pcy)):
        g2p_gather(s.bound_min, s.gres, BIAS[a], s.cell_size, a, s.px, s.pv, pc, s.gv[a])
    return dt
