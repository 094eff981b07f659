"""numpy restatement of the 2D density solve and the 2D rigid-body distances (solver/DensityCGSolver2D.py and
solver/sdf2D.py of the reference), test helper.

Vectorised over cells / particles, every statement in the reference kernels' order (separate multiplies and adds,
left to right), so the kernels' fp64 results round as the HIP kernels' do.  The particle scatter adds in particle order
(np.bincount walks its input front to back, as the reference's sequential launch under the golden shim does); `order`
selects another order for the spread measurements.  The CG loop uses numpy's sums (or sums in blocks of 256,
`block=256`), so its history agrees with the reference's to rounding only.  Used by the CPU golden tests and, at sizes
the reference shim cannot reach, by the GPU tests.
"""
import numpy as np


def _cell(px, bmin, cs, bias):
    """base index and |gx - x| / cell_size weights per axis (:19-23, :182-186)"""
    x = np.asarray(px, np.float64)
    gi = np.floor((x - bmin) / cs - bias)
    gx = (gi + bias) * cs + bmin
    return gi.astype(np.int64), np.abs(gx - x) / cs


def _cw(i, w):
    return i + ((-1) ** i) * (1 - w)


def splat(bound_min, cell_size, gres, px, pm, gm, order=None):
    """initialize_density (:8-33): gm += scattered mass, particles in `order` (default: as stored).  gvol untouched.
    Returns the number of contributions per cell."""
    Nx, Ny = (int(v) for v in gres)
    bmin, cs = np.asarray(bound_min, np.float64), np.asarray(cell_size, np.float64)
    px, pm = np.asarray(px), np.asarray(pm, np.float64)
    if order is not None:
        px, pm = px[order], pm[order]
    gi, w = _cell(px, bmin, cs, 0.5)
    idx = np.empty((len(px), 4), np.int64)
    val = np.empty((len(px), 4), np.float64)
    k = 0
    for ix in (0, 1):
        for iy in (0, 1):
            cx = np.clip(gi[:, 0] + ix, 0, Nx - 1)
            cy = np.clip(gi[:, 1] + iy, 0, Ny - 1)
            idx[:, k] = cx * Ny + cy
            val[:, k] = _cw(ix, w[:, 0]) * _cw(iy, w[:, 1]) * pm
            k += 1
    add = np.bincount(idx.ravel(), weights=val.ravel(), minlength=Nx * Ny).reshape(Nx, Ny)
    gm += add.astype(gm.dtype) if gm.dtype != np.float64 else add
    return np.bincount(idx.ravel(), minlength=Nx * Ny).reshape(Nx, Ny)


def splat_abs(bound_min, cell_size, gres, px, pm):
    """sum of |contribution| per cell: the S of the per-node bound (K + 2) u S"""
    Nx, Ny = (int(v) for v in gres)
    out = np.zeros((Nx, Ny))
    splat(bound_min, cell_size, gres, px, np.abs(np.asarray(pm, np.float64)), out)
    return out


def _nonsolid(wx, wy):
    return (wx[1:-2, 1:-1] + wx[2:-1, 1:-1] + wy[1:-1, 1:-2] + wy[1:-1, 2:-1]) * 0.25


def _D(a, i0, j0, nx, ny):
    """a[2x + i0, 2y + j0] over the interior cells x = 1 .. nx, y = 1 .. ny"""
    return a[2 + i0:2 + i0 + 2 * nx:2, 2 + j0:2 + j0 + 2 * ny:2]


def fix_volume(cell_size, gres, lvol, gvol, sphi, lphi, wx, wy):
    """fix_volume (:35-57): interior cells of gvol"""
    Nx, Ny = (int(v) for v in gres)
    nx, ny = Nx - 2, Ny - 2
    if nx <= 0 or ny <= 0:
        return
    cs = np.asarray(cell_size, np.float64)
    cvol, dx = float(np.prod(cs)), float(np.min(cs))
    L = lambda a, b: _D(lvol, a, b, nx, ny)         # noqa: E731
    fluid = L(1, 1) + (1.0 / 2.0) * (L(2, 1) + L(0, 1) + L(1, 2) + L(1, 0)) \
        + (1.0 / 4.0) * (L(2, 2) + L(0, 2) + L(2, 0) + L(0, 0))
    near = _D(sphi, 1, 1, nx, ny) < dx
    f = lphi < 0
    internal = f[1:-1, 1:-1] & f[2:, 1:-1] & f[:-2, 1:-1] & f[1:-1, 2:] & f[1:-1, :-2]
    fluid = np.where(internal & ~near, cvol, fluid)
    gvol[1:-1, 1:-1] = np.minimum(fluid, cvol * _nonsolid(wx, wy))


def rhs(rho0, dt, gres, cell_size, gm, gvol, lphi, wx, wy, b):
    """initialize_solver (:59-83): interior cells of b.  Returns (density_frac before the clamp, mask of the
    cell_mass < 1e-10 branch) over the interior fluid cells, for the edge-case tests."""
    Nx, Ny = (int(v) for v in gres)
    if Nx <= 2 or Ny <= 2:
        return None, None
    cvol = float(np.prod(np.asarray(cell_size, np.float64)))
    solid_vol = (1 - _nonsolid(wx, wy)) * cvol
    solid_mass = rho0 * solid_vol
    cell_mass = np.asarray(gm, np.float64)[1:-1, 1:-1] + solid_mass
    cell_vol = np.asarray(gvol, np.float64)[1:-1, 1:-1] + solid_vol
    frac = cell_mass / np.maximum(cell_vol, 1e-10) / rho0
    tiny = cell_mass < 1e-10
    frac = np.where(tiny, 1.0, frac)
    out = (1 - np.maximum(0.5, np.minimum(1.5, frac))) / dt
    fl = lphi[1:-1, 1:-1] < 0
    b[1:-1, 1:-1] = np.where(fl, out, 0.0)
    return np.where(fl, frac, np.nan), tiny & fl


def apply(gres, v, out, wx, wy, lphi, stats=None):
    """matvecmul (:85-139): interior cells of out"""
    Nx, Ny = (int(v_) for v_ in gres)
    if Nx <= 2 or Ny <= 2:
        return
    v = np.asarray(v, np.float64)
    phi = lphi[1:-1, 1:-1]
    val = np.zeros(phi.shape)
    diag = np.zeros(phi.shape)
    clamped = 0
    for nphi, w, vn in ((lphi[2:, 1:-1], wx[2:-1, 1:-1], v[2:, 1:-1]), (lphi[:-2, 1:-1], wx[1:-2, 1:-1], v[:-2, 1:-1]),
                        (lphi[1:-1, 2:], wy[1:-1, 2:-1], v[1:-1, 2:]), (lphi[1:-1, :-2], wy[1:-1, 1:-2], v[1:-1, :-2])):
        fl = nphi < 0
        with np.errstate(divide="ignore", invalid="ignore"):
            th = phi / (phi - nphi)
            frac = np.minimum(1, np.maximum(0.01, th))
            if stats is not None:
                clamped += int(((phi < 0) & ~fl & (th < 0.01)).sum())
            val = np.where(fl, val - w * vn, val)
            diag = np.where(fl, diag + 1, diag + 1 / frac)
    val = val + diag * v[1:-1, 1:-1]
    out[1:-1, 1:-1] = np.where(phi < 0, val, 0.0)
    if stats is not None:
        stats["theta_clamped"] = clamped


def _eif(l, r):
    """edge_in_fraction (SolidFractionCommon.py)"""
    li, ri = l < 0, r < 0
    with np.errstate(divide="ignore", invalid="ignore"):
        diff = -np.abs(l - r)
        return np.where(li & ri, 1.0, np.where(~li & ~ri, 0.0, np.where(li, l / diff, r / diff)))


def displacement(gres, dt, cell_size, dx, dy, pv, lphi):
    """compute_displacement (:141-152): dx[1:Nx, 1:Ny], dy[1:Nx, 1:Ny], nothing else"""
    Nx, Ny = (int(v) for v in gres)
    if Nx < 2 or Ny < 2:
        return
    pv = np.asarray(pv, np.float64)
    c, cl, cp_ = lphi[1:, 1:], lphi[:-1, 1:], lphi[1:, :-1]
    phix = np.minimum(1, np.maximum(0.01, _eif(c, cl)))
    phiy = np.minimum(1, np.maximum(0.01, _eif(c, cp_)))
    dx[1:Nx, 1:Ny] = (pv[1:, 1:] - pv[:-1, 1:]) * dt * cell_size[0] / phix
    dy[1:Nx, 1:Ny] = (pv[1:, 1:] - pv[1:, :-1]) * dt * cell_size[1] / phiy


def advect(px, d, bound_min, cell_size, grid_bias, axis):
    """apply_displacement (:171-195), in place on px[:, axis]; each of the four terms added into the stored value"""
    bmin, cs = np.asarray(bound_min, np.float64), np.asarray(cell_size, np.float64)
    gi, w = _cell(px, bmin, cs, np.asarray(grid_bias, np.float64))
    d = np.asarray(d, np.float64)
    pos = px[:, axis].copy()
    for ix in (0, 1):
        for iy in (0, 1):
            cx = np.clip(gi[:, 0] + ix, 0, d.shape[0] - 1)
            cy = np.clip(gi[:, 1] + iy, 0, d.shape[1] - 1)
            weight = _cw(ix, w[:, 0]) * _cw(iy, w[:, 1])
            pos = (pos.astype(np.float64) + weight * d[cx, cy]).astype(px.dtype)
    px[:, axis] = pos


def _sum(a, block):
    a = np.asarray(a, np.float64).ravel()
    if not block:
        return float(np.sum(a))
    pad = (-len(a)) % block
    a = np.concatenate([a, np.zeros(pad)]).reshape(-1, block)
    return float(np.sum(np.sum(a, axis=1)))


def cg(gres, b, wx, wy, lphi, tol, max_iter, q=None, block=0):
    """the loop of solve (:274-290) from x = 0 on stored b; `q` = what the shared buffer's q held before (its boundary
    cells are never written and count in d.q).  Returns dict(history, iters, x, d, r, q)."""
    g = tuple(int(v) for v in gres)
    x = np.zeros(g)
    q = np.zeros(g) if q is None else np.array(q, np.float64)
    apply(g, x, q, wx, wy, lphi)
    d = b - q
    r = d.copy()
    delta = _sum(r ** 2, block)
    hist, iters = [delta], 0
    if not delta < tol ** 2:
        for _ in range(int(max_iter)):
            apply(g, d, q, wx, wy, lphi)
            dq = _sum(d * q, block)
            alpha = delta / dq
            x += alpha * d
            r -= alpha * q
            old = delta
            delta = _sum(r ** 2, block)
            hist += [dq, delta]
            iters += 1
            if delta < tol ** 2:
                break
            d = r + (delta / old) * d
    return dict(history=np.array(hist), iters=iters, x=x, d=d, r=r, q=q, delta=delta)


def solve(gres, bound_min, bound_size, rho0, dt, px, pm, sphi, lphi, lvol, wx, wy, tol=1e-3, max_iter=None, q=None,
          b_boundary=None, order=None, block=0):
    """DensityCGSolver2D.solve (:262-294) from given face weights, in place on px.  No error when max_iter runs out.
    `b_boundary`: what the shared buffer's b held before (only its boundary cells survive)."""
    g = tuple(int(v) for v in gres)
    cs = np.asarray(bound_size, np.float64) / np.asarray(g, np.float64)
    gm, gvol = np.zeros(g), np.zeros(g)
    splat(bound_min, cs, g, px, pm, gm, order)
    fix_volume(cs, g, lvol, gvol, sphi, lphi, wx, wy)
    b = np.zeros(g) if b_boundary is None else np.array(b_boundary, np.float64)
    rhs(rho0, dt, g, cs, gm, gvol, lphi, wx, wy, b)
    out = cg(g, b, wx, wy, lphi, tol, int(np.prod(g)) if max_iter is None else max_iter, q, block)
    dx, dy = np.zeros((g[0] + 1, g[1])), np.zeros((g[0], g[1] + 1))
    displacement(g, dt, cs, dx, dy, out["x"], lphi)
    advect(px, dx, bound_min, cs, (0, 0.5), 0)
    advect(px, dy, bound_min, cs, (0.5, 0), 1)
    out.update(gm=gm, gvol=gvol, b=b, dx=dx, dy=dy)
    return out


def solid_frac(gres, sphi, wx, wy):
    """compute_solid_frac (SolidFraction2D.py): cells x < Nx-1, y < Ny-1 write wx[x,y], wx[x+1,y]... -- here through the
    project's oracle, which the existing 2D tests pin against the reference"""
    from oracle import mfs_oracle as O
    O.compute_solid_frac2d(gres, sphi, wx, wy)


# ------------------------------------------------------------------------------------------- sdf2D ---
def _body(rb):
    return rb[0], rb[1:3, 2], rb[4:6, :2], rb[7, :2]


def _to_body(R, T, p0, p1):
    out = []
    for i in range(2):
        t2 = (0.0 - R[0, i] * T[0]) - R[1, i] * T[1]
        out.append((R[0, i] * p0 + R[1, i] * p1) + t2)
    return out


def _to_world(R, T, b0, b1):
    return [(R[i, 0] * b0 + R[i, 1] * b1) + T[i] for i in range(2)]


def sdf_evaluate(rb_d, position):
    """evaluate (:146-169, :185-196) -> (sd, vel) for position (..., 2)"""
    pos = np.asarray(position, np.float64).reshape(-1, 2)
    p0, p1 = pos[:, 0], pos[:, 1]
    sd = np.full(len(pos), 100.0)
    win = np.zeros(len(pos), np.int64)
    for i, rb in enumerate(np.asarray(rb_d)):
        par, T, R, _ = _body(rb)
        if par[0] // 2 == 0:
            d = np.sqrt((p0 - T[0]) ** 2 + (p1 - T[1]) ** 2) - par[1]
        elif par[0] // 2 == 1:
            b = _to_body(R, T, p0, p1)
            tmp = np.zeros(len(pos))
            mx = np.full(len(pos), -100.0)
            for k in range(2):
                disp = np.abs(b[k]) - par[1 + k] / 2
                tmp = np.where(disp > 0, tmp + disp ** 2, tmp)
                mx = np.where(mx < disp, disp, mx)
            d = np.sqrt(tmp)
            d = np.where(mx < 0, d + mx, d)
        else:
            continue
        if par[0] % 2:
            d = -d
        closer = d < sd
        sd = np.where(closer, d, sd)
        win = np.where(closer, i, win)
    vel = np.zeros((len(pos), 2))
    inside = sd <= 0
    if len(rb_d):
        vel[inside] = np.asarray(rb_d)[win[inside], -1, :2]
    shape = np.asarray(position).shape[:-1]
    return sd.reshape(shape), vel.reshape(shape + (2,))


def sdf_project(rb_d, position):
    """project (:171-183, :198-205) in place on position (P, 2); float32 positions round after every body"""
    pos = position
    for rb in np.asarray(rb_d):
        par, T, R, _ = _body(rb)
        p0, p1 = pos[:, 0].astype(np.float64), pos[:, 1].astype(np.float64)
        flipped = bool(par[0] % 2)
        if par[0] // 2 == 0:
            d0, d1 = p0 - T[0], p1 - T[1]
            dist = np.sqrt(d0 ** 2 + d1 ** 2)
            centre = dist <= 0.0001
            sd = dist - par[1]
            if flipped:
                sd = -sd
            with np.errstate(divide="ignore", invalid="ignore"):
                n0 = np.where(~centre & (sd < 0), d0 / dist * par[1] + T[0], p0)
                n1 = np.where(~centre & (sd < 0), d1 / dist * par[1] + T[1], p1)
            if flipped:
                n0, n1 = np.where(centre, T[0] + par[1], n0), np.where(centre, T[1], n1)
        elif par[0] // 2 == 1:
            b = _to_body(R, T, p0, p1)
            h = [par[1] / 2, par[2] / 2]
            if flipped:
                c = [np.where(b[k] < -h[k], -h[k], np.where(b[k] > h[k], h[k], b[k])) for k in range(2)]
                n0, n1 = _to_world(R, T, c[0], c[1])
            else:
                inside = (np.abs(b[0]) <= h[0]) & (np.abs(b[1]) <= h[1])
                dist = np.full(len(p0), 100.0)
                index = np.zeros(len(p0), np.int64)
                for k in range(2):
                    a = h[k] - b[k]
                    m = a < dist
                    dist, index = np.where(m, a, dist), np.where(m, 2 * k, index)
                    a = b[k] + h[k]
                    m = a < dist
                    dist, index = np.where(m, a, dist), np.where(m, 2 * k + 1, index)
                move = dist * np.where(index % 2 == 1, -1.0, 1.0)
                c = [np.where(index // 2 == k, b[k] + move, b[k]) for k in range(2)]
                w0, w1 = _to_world(R, T, c[0], c[1])
                n0, n1 = np.where(inside, w0, p0), np.where(inside, w1, p1)
        else:
            continue
        pos[:, 0] = n0.astype(pos.dtype)
        pos[:, 1] = n1.astype(pos.dtype)
