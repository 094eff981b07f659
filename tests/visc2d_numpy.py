"""numpy restatement of the 2D viscosity solve (solver/ViscosityCGSolver2D.py of the reference), test helper.

Vectorised over the interior faces, every statement in the reference kernels' order (separate multiplies and adds,
products left to right), so the RHS and the operator round as the HIP direct kernels do.  The CG loop uses numpy's
sums, so its history agrees with the reference's to rounding only.  Used by the CPU golden tests and, at sizes the
reference shim cannot reach, by the GPU tests.
"""
import numpy as np


def _S(a, i0, j0, nx, ny):
    """a[2x + i0, 2y + j0] over the nx * ny faces of the interior block (doubled grid, step 2)"""
    return a[i0:i0 + 2 * nx:2, j0:j0 + 2 * ny:2]


def _V(a, x0, y0, nx, ny):
    return a[x0:x0 + nx, y0:y0 + ny]


def _x_block(g):
    return g[0] - 1, g[1] - 2          # x-faces with an equation: 1 <= x <= Nx-1, 1 <= y <= Ny-2


def _y_block(g):
    return g[0] - 2, g[1] - 1          # y-faces: 1 <= x <= Nx-2, 1 <= y <= Ny-1


def rhs(gres, scale, mu, vx, vy, sphi, vol, b_x, b_y):
    """initialize_solver (:6-103); boundary faces of b_x, b_y untouched"""
    g = tuple(int(v) for v in gres)
    vx, vy = np.asarray(vx, np.float64), np.asarray(vy, np.float64)
    nx, ny = _x_block(g)
    if nx > 0 and ny > 0:
        S = lambda a, b: _S(sphi, 2 + a, 3 + b, nx, ny)          # noqa: E731   sphi[2x+a, 2y+1+b]
        W = lambda a, b: _S(vol, 2 + a, 3 + b, nx, ny)           # noqa: E731
        X = lambda p, q: _V(vx, 1 + p, 1 + q, nx, ny)            # noqa: E731
        Y = lambda p, q: _V(vy, 1 + p, 1 + q, nx, ny)            # noqa: E731
        vc, vr, vl, vt, vb = W(0, 0), W(1, 0), W(-1, 0), W(0, 1), W(0, -1)
        b = X(0, 0) * vc
        b = np.where(S(2, 0) <= 0, b + 2 * scale * mu * vr * X(1, 0), b)
        b = np.where(S(-2, 0) <= 0, b + 2 * scale * mu * vl * X(-1, 0), b)
        b = np.where(S(0, 2) <= 0, b + scale * mu * vt * X(0, 1), b)
        b = np.where(S(0, -2) <= 0, b + scale * mu * vb * X(0, -1), b)
        b = np.where(S(1, 1) <= 0, b + scale * mu * vt * Y(0, 1), b)
        b = np.where(S(-1, 1) <= 0, b - scale * mu * vt * Y(-1, 1), b)
        b = np.where(S(1, -1) <= 0, b - scale * mu * vb * Y(0, 0), b)
        b = np.where(S(-1, -1) <= 0, b + scale * mu * vb * Y(-1, 0), b)
        b_x[1:1 + nx, 1:1 + ny] = np.where(S(0, 0) <= 0, 0.0, b)
    nx, ny = _y_block(g)
    if nx > 0 and ny > 0:
        S = lambda a, b: _S(sphi, 3 + a, 2 + b, nx, ny)          # noqa: E731   sphi[2x+1+a, 2y+b]
        W = lambda a, b: _S(vol, 3 + a, 2 + b, nx, ny)           # noqa: E731
        X = lambda p, q: _V(vx, 1 + p, 1 + q, nx, ny)            # noqa: E731
        Y = lambda p, q: _V(vy, 1 + p, 1 + q, nx, ny)            # noqa: E731
        vc, vr, vl, vt, vb = W(0, 0), W(1, 0), W(-1, 0), W(0, 1), W(0, -1)
        b = Y(0, 0) * vc
        b = np.where(S(2, 0) <= 0, b + scale * mu * vr * Y(1, 0), b)
        b = np.where(S(-2, 0) <= 0, b + scale * mu * vl * Y(-1, 0), b)
        b = np.where(S(0, 2) <= 0, b + 2 * scale * mu * vt * Y(0, 1), b)
        b = np.where(S(0, -2) <= 0, b + 2 * scale * mu * vb * Y(0, -1), b)
        b = np.where(S(1, 1) <= 0, b + scale * mu * vr * X(1, 0), b)
        b = np.where(S(1, -1) <= 0, b - scale * mu * vr * X(1, -1), b)
        b = np.where(S(-1, 1) <= 0, b - scale * mu * vl * X(0, 0), b)
        b = np.where(S(-1, -1) <= 0, b + scale * mu * vl * X(0, -1), b)
        b_y[1:1 + nx, 1:1 + ny] = np.where(S(0, 0) <= 0, 0.0, b)


def apply(gres, scale, mu, vx, vy, out_x, out_y, sphi, vol):
    """matvecmul (:105-207); boundary faces of out_x, out_y untouched"""
    g = tuple(int(v) for v in gres)
    vx, vy = np.asarray(vx, np.float64), np.asarray(vy, np.float64)
    nx, ny = _x_block(g)
    if nx > 0 and ny > 0:
        S = lambda a, b: _S(sphi, 2 + a, 3 + b, nx, ny)          # noqa: E731
        W = lambda a, b: _S(vol, 2 + a, 3 + b, nx, ny)           # noqa: E731
        X = lambda p, q: _V(vx, 1 + p, 1 + q, nx, ny)            # noqa: E731
        Y = lambda p, q: _V(vy, 1 + p, 1 + q, nx, ny)            # noqa: E731
        vc, vr, vl, vt, vb = W(0, 0), W(1, 0), W(-1, 0), W(0, 1), W(0, -1)
        diag = vc + scale * mu * (2 * vr + 2 * vl + vt + vb)
        v = diag * X(0, 0)
        v = np.where(S(2, 0) > 0, v - 2 * scale * mu * vr * X(1, 0), v)
        v = np.where(S(-2, 0) > 0, v - 2 * scale * mu * vl * X(-1, 0), v)
        v = np.where(S(0, 2) > 0, v - scale * mu * vt * X(0, 1), v)
        v = np.where(S(0, -2) > 0, v - scale * mu * vb * X(0, -1), v)
        v = np.where(S(1, 1) > 0, v - scale * mu * vt * Y(0, 1), v)
        v = np.where(S(-1, 1) > 0, v + scale * mu * vt * Y(-1, 1), v)
        v = np.where(S(1, -1) > 0, v + scale * mu * vb * Y(0, 0), v)
        v = np.where(S(-1, -1) > 0, v - scale * mu * vb * Y(-1, 0), v)
        out_x[1:1 + nx, 1:1 + ny] = np.where(S(0, 0) <= 0, 0.0, v)
    nx, ny = _y_block(g)
    if nx > 0 and ny > 0:
        S = lambda a, b: _S(sphi, 3 + a, 2 + b, nx, ny)          # noqa: E731
        W = lambda a, b: _S(vol, 3 + a, 2 + b, nx, ny)           # noqa: E731
        X = lambda p, q: _V(vx, 1 + p, 1 + q, nx, ny)            # noqa: E731
        Y = lambda p, q: _V(vy, 1 + p, 1 + q, nx, ny)            # noqa: E731
        vc, vr, vl, vt, vb = W(0, 0), W(1, 0), W(-1, 0), W(0, 1), W(0, -1)
        diag = vc + scale * mu * (vr + vl + 2 * vt + 2 * vb)
        v = diag * Y(0, 0)
        v = np.where(S(2, 0) > 0, v - scale * mu * vr * Y(1, 0), v)
        v = np.where(S(-2, 0) > 0, v - scale * mu * vl * Y(-1, 0), v)
        v = np.where(S(0, 2) > 0, v - 2 * scale * mu * vt * Y(0, 1), v)
        v = np.where(S(0, -2) > 0, v - 2 * scale * mu * vb * Y(0, -1), v)
        v = np.where(S(1, 1) > 0, v - scale * mu * vr * X(1, 0), v)
        v = np.where(S(1, -1) > 0, v + scale * mu * vr * X(1, -1), v)
        v = np.where(S(-1, 1) > 0, v + scale * mu * vl * X(0, 0), v)
        v = np.where(S(-1, -1) > 0, v - scale * mu * vl * X(0, -1), v)
        out_y[1:1 + nx, 1:1 + ny] = np.where(S(0, 0) <= 0, 0.0, v)


def writeback(gres, vx, vy, out_x, out_y, sphi):
    """apply_viscosity (:209-220): faces of cells 1 <= x <= Nx-1, 1 <= y <= Ny-1 whose sample is > 0"""
    Nx, Ny = (int(v) for v in gres)
    if Nx < 2 or Ny < 2:
        return
    mx = sphi[2:2 * Nx:2, 3:2 * Ny + 1:2] > 0           # sphi[2x, 2y+1]
    my = sphi[3:2 * Nx + 1:2, 2:2 * Ny:2] > 0           # sphi[2x+1, 2y]
    sx, sy = (slice(1, Nx), slice(1, Ny)), (slice(1, Nx), slice(1, Ny))
    vx[sx] = np.where(mx, out_x[sx], vx[sx])
    vy[sy] = np.where(my, out_y[sy], vy[sy])


def solve(gres, bound_size, dt, mu, rho, vx, vy, sphi, lvol, tol=1e-4, max_iter=None):
    """ViscosityCGSolver2D.solve (:266-317) in place on vx, vy.  Returns dict(history=[delta0, dq1, delta1, ...],
    iters, x_x, x_y) -- iters counts every iteration, the converging one included."""
    g = tuple(int(v) for v in gres)
    cell_size = np.asarray(bound_size, np.float64) / np.asarray(g, np.float64)
    cell_vol = float(np.prod(cell_size))
    scale = dt / cell_vol / rho
    vol = np.asarray(lvol) / (cell_vol * 0.125)
    fx, fy = (g[0] + 1, g[1]), (g[0], g[1] + 1)
    xx, xy = np.array(vx, np.float64), np.array(vy, np.float64)
    bx, by, qx, qy = np.zeros(fx), np.zeros(fy), np.zeros(fx), np.zeros(fy)
    rhs(g, scale, mu, xx, xy, sphi, vol, bx, by)
    apply(g, scale, mu, xx, xy, qx, qy, sphi, vol)
    dx, dy = bx - qx, by - qy
    rx, ry = dx.copy(), dy.copy()
    delta = np.sum(rx ** 2) + np.sum(ry ** 2)
    hist, iters = [delta], 0
    max_iter = int(np.prod(g)) if max_iter is None else int(max_iter)
    if not delta < tol ** 2:
        for _ in range(max_iter):
            apply(g, scale, mu, dx, dy, qx, qy, sphi, vol)
            dq = np.sum(dx * qx) + np.sum(dy * qy)
            alpha = delta / dq
            xx += alpha * dx
            xy += alpha * dy
            rx -= alpha * qx
            ry -= alpha * qy
            old = delta
            delta = np.sum(rx ** 2) + np.sum(ry ** 2)
            hist += [dq, delta]
            iters += 1
            if delta < tol ** 2:
                break
            beta = delta / old
            dx = rx + beta * dx
            dy = ry + beta * dy
        else:
            raise ValueError("Failed to converge!")
    writeback(g, vx, vy, xx, xy, sphi)
    return dict(history=np.array(hist), iters=iters, x_x=xx, x_y=xy)
