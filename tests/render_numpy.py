"""The float64 oracle of the ray marcher (mfs/render.py, csrc/mfs_render.hip), operation by operation,
vectorised over pixels and looped over steps.  It visits every sample of every shape: no bricks, no skips.

Scene: shapes (vol, origin, spacing, R, T) as tests/seed_numpy.py.  Shape i at the world point x: xb = to_body(R, T, x),
u_a = (xb_a - origin_a) / spacing; if 0 <= u_a <= n_a - 1 on all three axes the value is seed_numpy.sample (the distance
term is 0 there), otherwise +inf.  F(x) = min_i S_i(x) taken with a strict `<` from +inf, so the id is the first shape
that attains it and a NaN sample is passed over: it never counts as negative.
Camera: `basis` restates mfs.render.Camera.basis(); pixel (i, j), row i from the top: sx = ((j + 0.5) * (2 / W) - 1) * half_w,
sy = (1 - (i + 0.5) * (2 / H)) * half_h; perspective o = eye, v = (f + sx r) + sy u, d = v / sqrt((v0^2 + v1^2) + v2^2);
orthographic o = (eye + sx r) + sy u, d = f.
March: t_k = near + k * step, x_k = o + t_k d; hit = the smallest k < K with F(x_k) < 0; with a = F(x_{k-1}), b = F(x_k):
depth = (t_k - step) + step * (a / (a - b)) if k > 0 and a is finite, else t_k.
Normal: g_a = S_id(x_hit + 0.5 h e_a) - S_id(x_hit - 0.5 h e_a) with seeding's sampler (clamp plus distance outside the box)
and h the hit shape's spacing, n = g / sqrt((g0^2 + g1^2) + g2^2), rounded to float32; -d where that length is 0 or not finite.

The band: the pixels a rounding could turn (see `render`); tests assert that it is empty before they compare pixel-wise.
"""
import numpy as np

import seed_numpy as S

EPS64 = S.EPS64
FACE_TOL = 1e-9          # node units: a sample this close to a face of a box could fall on either side of it
FLAT_TOL = 1e-6          # x spacing: a secant denominator or a gradient shorter than this is ill-conditioned
BRICK = 8                # cells per brick edge


def _unit(v):
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def basis(eye, target, up=(0.0, 1.0, 0.0), fov=40.0, ortho_height=None, width=1, height=1):
    """dict(eye, f, r, u, half_w, half_h, ortho): what mfs.render.Camera.basis() returns"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    f = _unit(target - eye)
    r = _unit(np.cross(f, up))
    u = np.cross(r, f)
    half_h = float(np.tan(np.deg2rad(np.float64(fov)) / 2.0)) if ortho_height is None else float(ortho_height) / 2.0
    return dict(eye=eye, f=f, r=r, u=u, half_w=half_h * width / height, half_h=half_h, ortho=ortho_height is not None)


def rays(cam, W, H):
    """(o, d), each (H * W, 3), pixel (i, j) at row i * W + j"""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    sx = (((j + 0.5) * (2.0 / W) - 1.0) * cam["half_w"]).reshape(-1, 1)
    sy = ((1.0 - (i + 0.5) * (2.0 / H)) * cam["half_h"]).reshape(-1, 1)
    f, r, u, eye = cam["f"], cam["r"], cam["u"], cam["eye"]
    if cam["ortho"]:
        return (eye + sx * r) + sy * u, np.broadcast_to(f, (H * W, 3)).copy()
    v = (f + sx * r) + sy * u
    return np.broadcast_to(eye, (H * W, 3)).copy(), v / np.sqrt((v[:, 0] ** 2 + v[:, 1] ** 2) + v[:, 2] ** 2)[:, None]


def value(shape, x):
    """(S_i(x) by the render rule, node coordinates u) of one shape at the points x"""
    vol, origin, h, R, T = shape
    xb = S.to_body(R, T, x)
    u = (xb - np.asarray(origin, np.float64)) / np.float64(h)
    inside = ((u >= 0.0) & (u <= np.asarray(vol.shape, np.float64) - 1.0)).all(axis=-1)
    return np.where(inside, S.sample(vol, origin, h, xb), np.inf), u


def scene(shapes, x):
    """(F, id, every shape's value (m, P), every shape's node coordinates (m, P, 3))"""
    F, ident = np.full(len(x), np.inf), np.full(len(x), -1, np.int32)
    vals, us = [], []
    for i, s in enumerate(shapes):
        v, u = value(s, x)
        with np.errstate(invalid="ignore"):
            better = v < F
        F, ident = np.where(better, v, F), np.where(better, np.int32(i), ident)
        vals.append(v)
        us.append(u)
    return F, ident, np.stack(vals), np.stack(us)


def _near_face(shapes, us):
    """pixels whose sample is within FACE_TOL node units of a face of some shape's box (and not beyond the others)"""
    out = np.zeros(us.shape[1], bool)
    for s, u in zip(shapes, us):
        hi = np.asarray(s[0].shape, np.float64) - 1.0
        within = ((u >= -FACE_TOL) & (u <= hi + FACE_TOL)).all(axis=-1)
        on = ((np.abs(u) <= FACE_TOL) | (np.abs(u - hi) <= FACE_TOL)).any(axis=-1)
        out |= within & on
    return out


def render(shapes, cam, W, H, near, step, K, touched=None):
    """dict of (H, W[, 3]) arrays: depth, normal (float32), shape_id, steps; a, b (the secant's operands; NaN where none
    was taken), secant (mask), glen (gradient length), band (mask), depth_bound, normal_bound, eps, samples (shape samples
    a marcher without skips visits).
    band: a pixel is in it if (1) a visited sample up to the hit, or the sample before it, has |F| <= eps, eps =
    band_eps(shapes, the rays' end points); (2) such a sample lies within FACE_TOL node units of a face of a box; (3) at
    the hit another shape's value is within eps of the minimum; (4) at the hit a - b or the gradient length is below
    FLAT_TOL * spacing.  touched(i, u) -> mask, optional: pixels with a visited sample of shape i at node coordinates u
    for which it is true are reported in `touched`."""
    assert 1 <= len(shapes) <= 16
    near, step = np.float64(near), np.float64(step)
    o, d = rays(cam, W, H)
    P = H * W
    eps = S.band_eps(shapes, np.concatenate([o + near * d, o + (near + np.float64(K) * step) * d]))
    depth, steps, ident = np.full(P, np.inf), np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    a, b = np.full(P, np.nan), np.full(P, np.nan)
    band, touch = np.zeros(P, bool), np.zeros(P, bool)
    prev = np.full(P, np.inf)
    live = np.arange(P)
    for k in range(K):
        if not len(live):
            break
        t = near + np.float64(k) * step
        x = o[live] + t * d[live]
        F, idk, vals, us = scene(shapes, x)
        with np.errstate(invalid="ignore"):
            band[live] |= (np.abs(F) <= eps) | _near_face(shapes, us)
            hit = F < 0
            second = np.sort(np.where(np.isnan(vals), np.inf, vals), axis=0)
            if len(shapes) > 1:
                band[live] |= hit & (second[1] - second[0] <= eps)
        if touched is not None:
            for i in range(len(shapes)):
                touch[live] |= touched(i, us[i])
        h = live[hit]
        steps[h], ident[h], b[h] = k, idk[hit], F[hit]
        sec = hit & np.isfinite(prev[live]) & (k > 0)
        hs = live[sec]
        a[hs] = prev[hs]
        with np.errstate(invalid="ignore", divide="ignore"):
            depth[h] = t
            depth[hs] = (t - step) + step * (a[hs] / (a[hs] - b[hs]))
        prev[live] = F
        live = live[~hit]
    hitm = steps >= 0
    secant = hitm & ~np.isnan(a)
    normal, glen = np.zeros((P, 3), np.float32), np.full(P, np.nan)
    spacing = np.ones(P)
    for i, s in enumerate(shapes):
        m = np.flatnonzero(ident == i)
        if not len(m):
            continue
        vol, origin, h, R, T = s
        spacing[m] = h
        xh = o[m] + depth[m][:, None] * d[m]
        hh = 0.5 * np.float64(h)
        g = np.empty((len(m), 3))
        for ax in range(3):
            xp, xm = xh.copy(), xh.copy()
            xp[:, ax], xm[:, ax] = xh[:, ax] + hh, xh[:, ax] - hh
            g[:, ax] = S.sample(vol, origin, h, S.to_body(R, T, xp)) - S.sample(vol, origin, h, S.to_body(R, T, xm))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            ok = (ln > 0) & np.isfinite(ln)
            normal[m] = np.where(ok[:, None], g / ln[:, None], -d[m]).astype(np.float32)
        glen[m] = ln
    normal[~hitm] = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        band |= secant & ((a - b) < FLAT_TOL * spacing)
        band |= hitm & ~(glen >= FLAT_TOL * spacing)
        tk = near + steps.astype(np.float64) * step
        depth_bound = np.where(secant, step * 2 * eps * (np.abs(a) + np.abs(b)) / (a - b) ** 2 + 8 * EPS64 * np.abs(tk), 0.0)
        normal_bound = np.where(hitm, 2.0 ** -24 + 8 * eps / glen, 0.0)
    samples = int(np.where(hitm, steps + 1, K).astype(np.int64).sum()) * len(shapes)
    sh = lambda v: v.reshape((H, W) + v.shape[1:])  # noqa: E731
    return dict(depth=sh(depth), normal=sh(normal), shape_id=sh(ident), steps=sh(steps), a=sh(a), b=sh(b), secant=sh(secant),
                glen=sh(glen), band=sh(band), touched=sh(touch), depth_bound=sh(depth_bound), normal_bound=sh(normal_bound),
                eps=eps, samples=samples, o=o, d=d)


def band(result):
    """the number of pixels in the band"""
    return int(result["band"].sum())


def bricks(vol):
    """float64 (ceil((n0-1)/8), ceil((n1-1)/8), ceil((n2-1)/8)): the minimum over each brick's nodes, 8 b .. min(8 b + 8,
    n - 1) along each axis; -inf for a brick that holds a NaN"""
    vol = np.asarray(vol)
    nb = [(n - 2) // BRICK + 1 for n in vol.shape]
    out = np.empty(nb, np.float64)
    for b0 in range(nb[0]):
        for b1 in range(nb[1]):
            for b2 in range(nb[2]):
                blk = vol[BRICK * b0:BRICK * b0 + BRICK + 1, BRICK * b1:BRICK * b1 + BRICK + 1,
                          BRICK * b2:BRICK * b2 + BRICK + 1].astype(np.float64)
                out[b0, b1, b2] = -np.inf if np.isnan(blk).any() else blk.min()
    return out


def shade(result, colors, background=(255, 255, 255), light=None):
    """(H, W, 3) uint8: albedo_id * (0.25 + 0.75 * max(0, n . l)), albedo = colour / 255, l = -d (the headlight) or the
    given unit vector towards the light; floor(255 c + 0.5); the background at misses"""
    H, W = result["steps"].shape
    n = result["normal"].reshape(-1, 3).astype(np.float64)
    l = -result["d"] if light is None else np.broadcast_to(np.asarray(light, np.float64), n.shape)
    lam = np.maximum(0.0, (n[:, 0] * l[:, 0] + n[:, 1] * l[:, 1]) + n[:, 2] * l[:, 2])
    ident = result["shape_id"].reshape(-1)
    albedo = np.asarray(colors, np.float64).reshape(-1, 3)[np.maximum(ident, 0)] / 255.0
    c = albedo * (0.25 + 0.75 * lam)[:, None]
    rgb = np.clip(np.floor(255.0 * c + 0.5), 0, 255).astype(np.uint8)
    rgb[ident < 0] = np.asarray(background, np.uint8)
    return rgb.reshape(H, W, 3)
