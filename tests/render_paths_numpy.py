"""The float64 oracle of the path renderer (mfs.render.Scene.trace / resolve, k_render_paths / k_render_resolve of
csrc/mfs_render.hip), operation by operation.  It builds on tests/render_numpy.py (shapes, camera, rays,
the render rule, the band's tolerances) and tests/seed_numpy.py (the sampler) and changes neither.  No bricks, no skips.

Segment march(o, d, t0, step, K, medium, include): samples x_k = o + (t0 + k * step) d, k < K; t0 = near for the camera's
ray, 0 for every later segment (0 + k * step is k * step exactly).  Shape i is sampled iff include[i].  In air (medium = -1)
S_i is render_numpy.value: the trilinear sample inside the shape's box, +inf outside.  Inside shape m (medium = m) shape m
counts negated: -S_m inside its box, -inf outside.  F = min over the included shapes taken with a strict `<` from +inf (the
first shape that attains it; a NaN is passed over); the hit is the first k with F(x_k) < 0, its id the arg min: id = m is
the exit from the liquid, another id a shape met inside it.  With a = F(x_{k-1}), b = F(x_k): depth = (t_k - step) + step *
(a / (a - b)) if k > 0, a is finite and the hit is not the medium's own -inf (leaving its box), else t_k.  Normal: the hit
shape's UN-negated central difference at x = o + depth d, exactly render_numpy's, n = g / sqrt((g0^2 + g1^2) + g2^2) kept in
float64, -d where that length is 0 or not finite.  It points outward at an exit.

Path of one ray.  Materials per shape: opaque(colour) or liquid(colour, ior, absorb per world unit); albedo = colour / 255,
bg = background / 255; l = the unit vector towards the light, or -d of the camera's ray (the headlight); ambient 0.25.
  slot 0  the camera's ray in air over all shapes, K samples.  A miss: colour = bg.
  shade(id, x, n)  of the surface finally shaded: lam = max(0, (n32_0 l_0 + n32_1 l_1) + n32_2 l_2) with n32 = n rounded to
          float32 -- the normal as mfs_render_march3d stores it, so that an all-opaque look without shadows repeats today's
          shade() bit for bit; every other use of n is float64.  vis = 1; with shadows, slot 3: an air march from x + bias n
          along l over the OPAQUE shapes only, K_shadow samples, vis = 0 if it hits.  Colour: albedo * (0.25 + 0.75 * (vis * lam)).
  refract(d, n, eta)  if (d0 n0 + d1 n1) + d2 n2 > 0 negate n (it faces the arriving ray); c = -(d . n);
          k = 1 - (eta * eta) * (1 - c * c); k < 0: total internal reflection; w = eta * c - sqrt(k); t_a = eta * d_a + w * n_a,
          t / sqrt((t0^2 + t1^2) + t2^2); the next segment starts at x - bias * n.
  An opaque hit in slot 0 is shaded.  A liquid hit: r0 = ((ior - 1) / (ior + 1))^2, m1 = 1 - c, m2 = m1 * m1,
  R = r0 + (1 - r0) * ((m2 * m2) * m1); refract with eta = 1 / ior;
  slot 1  inside the liquid (medium = its id) over all shapes, K_inside samples.  (c) a miss: behind = the liquid's albedo,
          L = K_inside * step.  (a) another shape met: behind = shade(...), L = depth.  (b) the exit: L = depth, refract with
          eta = ior; total internal reflection: behind = the liquid's albedo; otherwise
  slot 2  in air over all shapes, K samples: a miss leaves behind = bg, any hit (a second liquid surface too) is shaded.
  colour_a = R * bg_a + ((1 - R) * exp(-(absorb_a * L))) * behind_a.
Resolve: the s x s colours of a pixel summed in row-major order from the first, divided by s * s; floor(255 c + 0.5) held in
0 .. 255.

The band: a ray is in it if a segment trips one of render_numpy's four conditions -- evaluated per segment and per sample
with eps_k = band_eps(shapes, the segment's end points) + (do + |t_k| dd) * LIP, where do and dd are the propagated bounds
on the segment's origin and direction and LIP is the largest node difference per spacing of the shapes (times sqrt 3: a
trilinear gradient has three components) plus 1 for the sampler's distance term; FACE_TOL is widened by
(do + |t_k| dd) / spacing -- or a Fresnel cosine is <= 1e-9, or a refraction discriminant has |k| <= 1e-9, or the colour
bound below exceeds 1e-6.

Bounds (first order in the errors; every factor that multiplies one in the colour is <= 1 because albedo, bg, R, T and
vis * lam are in [0, 1]):
  segment  depth_bound = render_numpy's secant bound with eps_k of the hit; the hit point moves by dx = do + depth * dd +
           depth_bound + 8 eps64 |x|.  The gradient component g_a = S(x + h/2 e_a) - S(x - h/2 e_a) has the derivative
           grad S(x + h/2 e_a) - grad S(x - h/2 e_a) in x, taken here from the cells' own nodes (`sample_grad`): with
           turn = sqrt(sum_a |that|^2), g moves by turn * dx plus the two samples' rounding, 2 sqrt(3) eps over the three
           components; normalising is a projection divided by |g|: dn = (2 sqrt(3) eps + turn dx) / |g| + 4 eps64.
  refract  dc = dd + dn; dk = 2 eta^2 dc; the unnormalised t moves by eta dd + |w| dn + eta dc + dk / (2 sqrt k), and so
           does the normalised one (a projection; |t| = 1 up to rounding), + 8 eps64; the next origin by dx + bias dn.
  Schlick  |dR / dc| = 5 (1 - r0) (1 - c)^4 <= 5: dR = 5 dc + 8 eps64.
  Lambert  |d lam| <= |dn| (+ dd for the headlight); the float32 rounding of n can move a component by 2^-23 only where n - dn
           and n + dn round differently, and is counted there.
  exp      |d exp(-a L)| <= a exp(-a (L - dL)) dL per channel; the argument's rounding, eps64 a L, costs eps64 x exp(-x)
           <= eps64 / e, the library a few ulps of T <= 1: dT = max over the channels of the first + 8 eps64.
  colour   dR (of R bg) + dR (of 1 - R) + dT + 0.75 d lam + 16 eps64.
The length bound is slot 1's depth_bound.
"""
import numpy as np

import render_numpy as RN
import seed_numpy as S

EPS64 = S.EPS64
AMBIENT = 0.25
TINY = 1e-9              # a Fresnel cosine or a refraction discriminant this small could fall on either side of 0
COLOR_TOL = 1e-6         # a ray whose derived colour bound exceeds this joins the band


def opaque(color):
    return dict(liquid=False, color=tuple(float(v) for v in color), ior=0.0, absorb=(0.0, 0.0, 0.0))


def liquid(color, ior=1.33, absorb=(0.0, 0.0, 0.0)):
    return dict(liquid=True, color=tuple(float(v) for v in color), ior=float(ior), absorb=tuple(float(v) for v in absorb))


def unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def lipschitz(shapes):
    """sqrt(3) * the largest finite difference of adjacent nodes per spacing over the shapes, + 1"""
    big = 0.0
    for vol, origin, h, R, T in shapes:
        v = np.asarray(vol, np.float64)
        for ax in range(3):
            dv = np.abs(np.diff(v, axis=ax))
            dv = dv[np.isfinite(dv)]
            if dv.size:
                big = max(big, float(dv.max()) / float(h))
    return np.sqrt(3.0) * big + 1.0


def sample_grad(vol, origin, h, xb):
    """the gradient of seed_numpy.sample in the body frame: of the trilinear cell along the axes where the point is not
    clamped, plus that of the distance term (for the bounds only: the kernels never take it)"""
    vol = np.asarray(vol)
    n, h = vol.shape, np.float64(h)
    c, fr, e, free = [], [], [], []
    for k in range(3):
        t = (xb[..., k] - np.float64(origin[k])) / h
        tc = np.minimum(np.maximum(t, 0.0), np.float64(n[k] - 1))
        ci = np.minimum(np.floor(tc).astype(np.int64), n[k] - 2)
        c.append(ci)
        fr.append(tc - ci.astype(np.float64))
        e.append((t - tc) * h)
        free.append(t == tc)
    V = lambda a, b, d: vol[c[0] + a, c[1] + b, c[2] + d].astype(np.float64)  # noqa: E731
    w = [(1.0 - fr[k], fr[k]) for k in range(3)]
    out = []
    with np.errstate(invalid="ignore", divide="ignore"):
        dist = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        for k in range(3):
            tot = 0.0
            for a in range(2):
                for b in range(2):
                    for q in range(2):
                        wk = [w[0][a], w[1][b], w[2][q]]
                        wk[k] = np.float64((-1.0, 1.0)[(a, b, q)[k]])
                        tot = tot + V(a, b, q) * wk[0] * wk[1] * wk[2]
            out.append(np.where(free[k], tot / h, 0.0) + np.where(dist > 0, e[k] / dist, 0.0))
    return np.stack(out, axis=-1)


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def segment(shapes, o, d, t0, step, K, medium, include, do, dd):
    """One march of the rays (o, d) (each (P, 3)); medium (P,) int (-1: air); include: a bool per shape; do, dd (P,): bounds on
    the errors of o and d.  Returns a dict of (P,) arrays: steps, id, depth, x (P, 3), n (P, 3), a, b, secant, glen, band,
    depth_bound, dx, dn, and `samples`, the shape samples a marcher without skips visits."""
    P = len(o)
    t0, step = np.float64(t0), np.float64(step)
    inc = [i for i in range(len(shapes)) if include[i]]
    lip = lipschitz(shapes)
    ends = np.concatenate([o + t0 * d, o + (t0 + np.float64(K) * step) * d]) if P else np.zeros((0, 3))
    eps0 = S.band_eps(shapes, ends[np.isfinite(ends).all(axis=-1)])
    hmin = min(float(s[2]) for s in shapes)
    eps = np.full(P, eps0)                             # at the hit, once known
    depth, steps, ident = np.full(P, np.inf), np.full(P, -1, np.int32), np.full(P, -1, np.int32)
    a, b = np.full(P, np.nan), np.full(P, np.nan)
    band = np.zeros(P, bool)
    prev = np.full(P, np.inf)
    live = np.arange(P)
    for k in range(K if inc else 0):
        if not len(live):
            break
        t = t0 + np.float64(k) * step
        x = o[live] + t * d[live]
        moved = do[live] + abs(float(t)) * dd[live]     # how far this sample can lie from the exact path's
        epsk, fl = eps0 + moved * lip, (RN.FACE_TOL + moved / hmin)[:, None]
        F, idk = np.full(len(live), np.inf), np.full(len(live), -1, np.int32)
        vals = []
        for i in inc:
            v, u = RN.value(shapes[i], x)
            hi = np.asarray(shapes[i][0].shape, np.float64) - 1.0
            inside = ((u >= 0.0) & (u <= hi)).all(axis=-1)
            neg = medium[live] == i
            v = np.where(neg, np.where(inside, -v, -np.inf), v)
            with np.errstate(invalid="ignore"):
                better = v < F
                within = ((u >= -fl) & (u <= hi + fl)).all(axis=-1)
                on = ((np.abs(u) <= fl) | (np.abs(u - hi) <= fl)).any(axis=-1)
                band[live] |= within & on
            F, idk = np.where(better, v, F), np.where(better, np.int32(i), idk)
            vals.append(v)
        with np.errstate(invalid="ignore"):
            band[live] |= np.abs(F) <= epsk
            hit = F < 0
            if len(inc) > 1:
                second = np.sort(np.where(np.isnan(np.stack(vals)), np.inf, np.stack(vals)), axis=0)
                band[live] |= hit & (second[1] - second[0] <= epsk)
        h = live[hit]
        eps[h] = epsk[hit]
        steps[h], ident[h], b[h] = k, idk[hit], F[hit]
        sec = hit & np.isfinite(prev[live]) & (k > 0) & ~((idk == medium[live]) & np.isneginf(F))
        hs = live[sec]
        a[hs] = prev[hs]
        with np.errstate(invalid="ignore", divide="ignore"):
            depth[h] = t
            depth[hs] = (t - step) + step * (a[hs] / (a[hs] - b[hs]))
        prev[live] = F
        live = live[~hit]
    hitm = steps >= 0
    secant = hitm & ~np.isnan(a)
    n, glen, spacing, turn = -d.copy(), np.full(P, np.nan), np.ones(P), np.zeros(P)
    xh = o + np.where(hitm, depth, 0.0)[:, None] * d
    for i, s in enumerate(shapes):
        m = np.flatnonzero(ident == i)
        if not len(m):
            continue
        vol, origin, h, R, T = s
        spacing[m] = h
        hh = 0.5 * np.float64(h)
        g, j2 = np.empty((len(m), 3)), np.zeros(len(m))
        for ax in range(3):
            xp, xm = xh[m].copy(), xh[m].copy()
            xp[:, ax], xm[:, ax] = xh[m][:, ax] + hh, xh[m][:, ax] - hh
            bp, bm = S.to_body(R, T, xp), S.to_body(R, T, xm)
            g[:, ax] = S.sample(vol, origin, h, bp) - S.sample(vol, origin, h, bm)
            j2 += ((sample_grad(vol, origin, h, bp) - sample_grad(vol, origin, h, bm)) ** 2).sum(axis=-1)
        turn[m] = np.sqrt(j2)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
            ok = (ln > 0) & np.isfinite(ln)
            n[m] = np.where(ok[:, None], g / ln[:, None], -d[m])
        glen[m] = ln
    with np.errstate(invalid="ignore", divide="ignore"):
        band |= secant & ((a - b) < RN.FLAT_TOL * spacing)
        band |= hitm & ~(glen >= RN.FLAT_TOL * spacing)
        tk = t0 + steps.astype(np.float64) * step
        depth_bound = np.where(secant, step * 2 * eps * (np.abs(a) + np.abs(b)) / (a - b) ** 2 + 8 * EPS64 * np.abs(tk), 0.0)
        dx = do + np.where(hitm, depth, 0.0) * dd + depth_bound + 8 * EPS64 * np.abs(xh).max(axis=-1, initial=0.0)
        dn = np.where(hitm, (2 * np.sqrt(3.0) * eps0 + turn * dx) / glen + 4 * EPS64, 0.0)
    samples = int(np.where(hitm, steps + 1, K).astype(np.int64).sum()) * len(inc)
    return dict(steps=steps, id=ident, depth=depth, x=xh, n=n, a=a, b=b, secant=secant, glen=glen, band=band,
                depth_bound=depth_bound, dx=dx, dn=dn, samples=samples)


def refract(d, n, eta, dd, dn):
    """(t, n facing the ray, c, k, dc, dt) of the module docstring; eta (P,).  Where k < 0, t is NaN."""
    flip = _dot(d, n) > 0.0
    n = np.where(flip[:, None], -n, n)
    c = -_dot(d, n)
    k = 1.0 - (eta * eta) * (1.0 - c * c)
    with np.errstate(invalid="ignore", divide="ignore"):
        w = eta * c - np.sqrt(k)
        t = eta[:, None] * d + w[:, None] * n
        t = t / np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])[:, None]
        dc = dd + dn
        dt = (eta * dd + np.abs(w) * dn + eta * dc + (eta * eta) * dc / np.sqrt(k)) + 8 * EPS64
    return t, n, c, k, dc, dt


def trace(shapes, materials, cam, W, H, near, step, K, light=None, background=(255, 255, 255), shadows=True, bias=None,
          K_shadow=None, K_inside=None):
    """The paths of the W x H rays of `cam` (for s x s supersampling pass (s W, s H) and the same camera).  Returns a dict:
    color (H, W, 3) float64, steps and shape_id (H, W, 4) int32 (-2: slot not run, -1: a miss), length (H, W), band,
    color_bound, length_bound (H, W), samples (an int), counts (a dict of the path outcomes)."""
    assert len(materials) == len(shapes)
    near, step = np.float64(near), np.float64(step)
    bias = 4.0 * step if bias is None else np.float64(bias)
    K_shadow = K if K_shadow is None else K_shadow
    K_inside = K if K_inside is None else K_inside
    m, P = len(shapes), H * W
    is_liquid = np.array([bool(q["liquid"]) for q in materials])
    albedo = np.array([q["color"] for q in materials], np.float64).reshape(m, 3) / 255.0
    ior = np.array([q["ior"] for q in materials], np.float64)
    absorb = np.array([q["absorb"] for q in materials], np.float64).reshape(m, 3)
    bg = np.asarray(background, np.float64) / 255.0
    o, d = RN.rays(cam, W, H)
    lvec = -d if light is None else np.broadcast_to(np.asarray(light, np.float64), (P, 3)).copy()
    dl = np.full(P, 4 * EPS64) if light is None else np.zeros(P)
    everything, air = np.ones(m, bool), np.full(P, -1)
    steps, ids = np.full((P, 4), -2, np.int32), np.full((P, 4), -2, np.int32)
    band = np.zeros(P, bool)
    samples = 0
    behind = np.tile(bg, (P, 1))
    R, L, liq = np.zeros(P), np.zeros(P), np.full(P, -1)
    dR, dL = np.zeros(P), np.zeros(P)
    fin, fid = np.zeros(P, bool), np.zeros(P, np.int64)
    fx, fn, fdx, fdn = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P), np.zeros(P)
    counts = dict(liquid=0, opaque=0, exits=0, met_inside=0, shadowed=0, opaque_after_exit=0, reflected=0, inside_miss=0)

    def record(slot, rays, seg):
        nonlocal samples
        steps[rays, slot], ids[rays, slot] = seg["steps"], seg["id"]
        band[rays] |= seg["band"]
        samples += seg["samples"]

    def final(rays, seg, sub):
        fin[rays], fid[rays] = True, seg["id"][sub]
        fx[rays], fn[rays], fdx[rays], fdn[rays] = seg["x"][sub], seg["n"][sub], seg["dx"][sub], seg["dn"][sub]

    s0 = segment(shapes, o, d, near, step, K, air, everything, np.zeros(P), np.full(P, 4 * EPS64))
    record(0, np.arange(P), s0)
    hit0 = s0["steps"] >= 0
    liq0 = hit0 & is_liquid[np.maximum(s0["id"], 0)]
    q = np.flatnonzero(hit0 & ~liq0)
    final(q, s0, q)
    counts["opaque"] = len(q)
    q = np.flatnonzero(liq0)
    counts["liquid"] = len(q)
    if len(q):
        liq[q] = s0["id"][q]
        n_i = ior[liq[q]]
        t1, nf, c, k, dc, dt = refract(d[q], s0["n"][q], 1.0 / n_i, np.full(len(q), 4 * EPS64), s0["dn"][q])
        band[q] |= (c <= TINY) | (np.abs(k) <= TINY)
        r0 = ((n_i - 1.0) / (n_i + 1.0)) ** 2
        m1 = 1.0 - c
        m2 = m1 * m1
        R[q], dR[q] = r0 + (1.0 - r0) * ((m2 * m2) * m1), 5.0 * dc + 8 * EPS64
        s1 = segment(shapes, s0["x"][q] - bias * nf, t1, 0.0, step, K_inside, liq[q], everything,
                     s0["dx"][q] + bias * s0["dn"][q], dt)
        record(1, q, s1)
        hit1 = s1["steps"] >= 0
        miss = q[~hit1]
        L[miss], behind[miss] = np.float64(K_inside) * step, albedo[liq[miss]]
        counts["inside_miss"] = len(miss)
        L[q[hit1]], dL[q[hit1]] = s1["depth"][hit1], s1["depth_bound"][hit1]
        out = hit1 & (s1["id"] == liq[q])
        met = np.flatnonzero(hit1 & ~out)
        final(q[met], s1, met)
        counts["met_inside"] = len(met)
        e = np.flatnonzero(out)
        counts["exits"] = len(e)
        if len(e):
            qe = q[e]
            t2, nf2, c2, k2, dc2, dt2 = refract(t1[e], s1["n"][e], n_i[e], dt[e], s1["dn"][e])
            band[qe] |= (c2 <= TINY) | (np.abs(k2) <= TINY)
            tir = k2 < 0.0
            behind[qe[tir]] = albedo[liq[qe[tir]]]
            counts["reflected"] = int(tir.sum())
            g = np.flatnonzero(~tir)
            if len(g):
                s2 = segment(shapes, s1["x"][e][g] - bias * nf2[g], t2[g], 0.0, step, K, air[:len(g)], everything,
                             s1["dx"][e][g] + bias * s1["dn"][e][g], dt2[g])
                record(2, qe[g], s2)
                h2 = np.flatnonzero(s2["steps"] >= 0)
                final(qe[g][h2], s2, h2)
                counts["opaque_after_exit"] = int((~is_liquid[s2["id"][h2]]).sum())

    f = np.flatnonzero(fin)
    dlam = np.zeros(P)
    if len(f):
        n32 = fn[f].astype(np.float32).astype(np.float64)
        lam = np.maximum(0.0, _dot(n32, lvec[f]))
        turned = (fn[f] - fdn[f][:, None]).astype(np.float32) != (fn[f] + fdn[f][:, None]).astype(np.float32)
        dlam[f] = fdn[f] + dl[f] + np.where(turned.any(axis=-1), 3 * 2.0 ** -23, 0.0)
        vis = np.ones(len(f))
        if shadows:
            s3 = segment(shapes, fx[f] + bias * fn[f], lvec[f], 0.0, step, K_shadow, air[:len(f)], ~is_liquid,
                         fdx[f] + bias * fdn[f], dl[f])
            record(3, f, s3)
            vis = np.where(s3["steps"] >= 0, 0.0, 1.0)
            counts["shadowed"] = int((vis == 0.0).sum())
        behind[f] = albedo[fid[f]] * (0.25 + 0.75 * (vis * lam))[:, None]
    wet = liq >= 0
    li = np.maximum(liq, 0)
    color = np.where(wet[:, None], R[:, None] * bg + ((1.0 - R)[:, None] * np.exp(-(absorb[li] * L[:, None]))) * behind, behind)
    with np.errstate(invalid="ignore", over="ignore"):
        dT = (absorb[li] * np.exp(-(absorb[li] * np.maximum(L - dL, 0.0)[:, None]))).max(axis=-1) * dL + 8 * EPS64
        bound = np.where(wet, 2 * dR + dT, 0.0) + 0.75 * dlam + 16 * EPS64
        band |= ~(bound <= COLOR_TOL)
    sh = lambda v, *tail: v.reshape((H, W) + tail)  # noqa: E731
    return dict(color=sh(color, 3), steps=sh(steps, 4), shape_id=sh(ids, 4), length=sh(np.where(wet, L, 0.0)), band=sh(band),
                color_bound=sh(bound), length_bound=sh(np.where(wet, dL, 0.0)), samples=samples, counts=counts, o=o, d=d)


def band(result):
    return int(result["band"].sum())


def resolve(color, s=1):
    """(H, W, 3) uint8 from the (s H, s W, 3) colours"""
    sH, sW, _ = color.shape
    H, W = sH // s, sW // s
    total = None
    for a in range(s):
        for b in range(s):
            part = color[a::s, b::s][:H, :W]
            total = part.copy() if total is None else total + part
    with np.errstate(invalid="ignore"):
        q = np.floor(255.0 * (total / np.float64(s * s)) + 0.5)
    return np.clip(np.where(np.isnan(q), 0.0, q), 0, 255).astype(np.uint8)


def bricks_max(vol):
    """render_numpy.bricks with the maximum over each brick's nodes; +inf for a brick that holds a NaN"""
    vol = np.asarray(vol)
    nb = [(n - 2) // RN.BRICK + 1 for n in vol.shape]
    out = np.empty(nb, np.float64)
    for b0 in range(nb[0]):
        for b1 in range(nb[1]):
            for b2 in range(nb[2]):
                blk = vol[RN.BRICK * b0:RN.BRICK * b0 + RN.BRICK + 1, RN.BRICK * b1:RN.BRICK * b1 + RN.BRICK + 1,
                          RN.BRICK * b2:RN.BRICK * b2 + RN.BRICK + 1].astype(np.float64)
                out[b0, b1, b2] = np.inf if np.isnan(blk).any() else blk.max()
    return out
