"""CPU checks on the inputs and bounds of tests/test_cell_kernels3d_gpu.py (tests/cell_kernels3d_inputs.py): the designed
fields reach both branches of every tap and comparison of the nine 3D cell kernels, no compared quantity sits on its
threshold, and every planted mistake of C.MISTAKES, applied to a copy of the oracle, exceeds the GPU tests' bound a hundred
times over on every coverage grid.

What a grid must cover.  COVERAGE_GRIDS (13,9,11), (17,19,23) and THIN_GRIDS (one interior row of 68 cells, four periods of
the level-set pattern; the taps across the thin axes reach into boundary cells, which carry the pattern too): everything
below.  (3,3,3) has one interior cell: it is liquid with liquid and air neighbours, a theta of 0.01 and a theta of 1.
Solid fractions and particles do not depend on interior cells and are checked on the coverage grids and on the face shapes
of every grid.

Solid-fraction values: a face's fraction is a quarter of the number of its four triangles (two adjacent nodes and the
centre) that lie wholly inside, and three such triangles force the fourth, so w takes the values 1, 0.75, 0.5 and 0 and
never 0.25; all four are required, with 0, 1, 2, 3 and 4 nodes inside and with node sums of exactly zero."""
import numpy as np
import pytest

import cell_kernels3d_inputs as C
from oracle import mfs_oracle as O

F64 = np.float64
SIDES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


def _sh(a, g, off=(0, 0, 0)):
    return np.asarray(a, F64)[tuple(slice(1 + o, n - 1 + o) for o, n in zip(off, g))]


def _face_w(d, side):
    """the weight of the face of every interior cell on `side`, as the pressure kernels read it"""
    a = [abs(s) for s in side].index(1)
    off = tuple(max(s, 0) for s in side)
    return _sh(d["w" + "xyz"[a]], d["gres"], off)


def _neg(a):
    return np.asarray(a) < 0


# ------------------------------------------------------------------------------------------------- the pattern ---
def test_pattern_holds_every_pair_at_every_distance():
    n = len(C.PATTERN)
    liquid, air = set("eL"), set("OznA")
    for dist in (1, -1, 3, -3, 5, -5):
        pairs = {(C.PATTERN[k], C.PATTERN[(k + dist) % n]) for k in range(n)}
        assert ("e", "O") in pairs and ("L", "A") in pairs and (("e", "z") in pairs or ("e", "n") in pairs), dist
        assert any(a == "L" and b in "zn" for a, b in pairs), dist
        for first, second in ((liquid, liquid), (air, liquid), (air, air)):
            assert any(a in first and b in second for a, b in pairs), dist
    assert "z" in C.PATTERN and "n" in C.PATTERN and all(np.gcd(s, n) == 1 for s in (1, 3, 5))


# ----------------------------------------------------------------------------------------------------- coverage ---
def _lphi_coverage(d):
    g, L = d["gres"], d["lphi"]
    phi = _sh(L, g)
    liquid = phi < 0
    out = {}
    for k, side in enumerate(SIDES):
        nphi = _sh(L, g, side)
        nl = nphi < 0
        out[f"side{k} liquid neighbour"] = (liquid & nl).any()
        out[f"side{k} air neighbour"] = (liquid & ~nl).any()
        w = _face_w(d, side)
        out[f"side{k} w < 1"] = (liquid & (w < 1)).any()
        out[f"side{k} w == 1"] = (liquid & ~(w < 1)).any()
        out[f"side{k} w > 0 beside liquid"] = (liquid & nl & (w > 0)).any()
        th = O._theta(phi, nphi)
        ghost = liquid & ~nl & (w > 0)
        out[f"side{k} theta 0.01"] = (ghost & (th == 0.01)).any()
        out[f"side{k} theta 1"] = (ghost & (th == 1.0)).any()
        out[f"side{k} theta between"] = (ghost & (th > 0.01) & (th < 1.0)).any()
    return out


def _face_coverage(d):
    """update and displacement: per axis, active and inactive faces and the three thetas of edge_in_fraction"""
    g, L = d["gres"], d["lphi"]
    C_ = tuple(slice(1, n) for n in g)
    out = {}
    for a in range(3):
        M = tuple(slice(1 - (a == b), g[b] - (a == b)) for b in range(3))
        pc, pm = L[C_], L[M]
        act = (pc < 0) | (pm < 0)
        th = np.minimum(1.0, np.maximum(0.01, O.edge_in_fraction(pc, pm)))
        w = d["w" + "xyz"[a]][C_]
        out[f"axis{a} active"], out[f"axis{a} inactive"] = act.any(), (~act).any()
        for name, m in (("0.01", th == 0.01), ("1", th == 1.0), ("between", (th > 0.01) & (th < 1.0))):
            out[f"axis{a} theta {name}"] = (act & m & (w > 0)).any()
        out[f"axis{a} w 0"], out[f"axis{a} w 1"] = (act & (w == 0)).any(), (act & (w == 1)).any()
        out[f"axis{a} w between"] = (act & (w > 0) & (w < 1)).any()
    return out


def _density_quantities(d, gdt=F64, wdt=F64):
    g = d["gres"]
    nsf = O._nonsolid_frac(g, *[C.rounded(d[k], wdt) for k in ("wx", "wy", "wz")])
    solid_vol = (1 - nsf) * C.CVOL
    cell_mass = _sh(C.rounded(d["gm"], gdt), g) + C.RHO0 * solid_vol
    cell_vol = _sh(C.rounded(d["gvol"], gdt), g) + solid_vol
    frac = cell_mass / np.maximum(cell_vol, 1e-10) / C.RHO0
    return cell_mass, cell_vol, frac


def _density_coverage(d):
    g, L = d["gres"], d["lphi"]
    liquid = _sh(L, g) < 0
    internal = liquid.copy()
    for side in SIDES:
        internal &= _sh(L, g, side) < 0
    near = d["sphi"][3:2 * g[0] - 2:2, 3:2 * g[1] - 2:2, 3:2 * g[2] - 2:2] < min(C.CS)
    cell_mass, cell_vol, frac = _density_quantities(d)
    live = liquid & ~(cell_mass < 1e-10)
    return {"internal, near solid": (internal & near).any(), "internal, away from solid": (internal & ~near).any(),
            "not internal, near": (~internal & near).any(), "not internal, away": (~internal & ~near).any(),
            "zero mass": (liquid & (cell_mass < 1e-10)).any(), "volume floor": (live & (cell_vol < 1e-10)).any(),
            "fraction clamps at 0.5": (live & (frac < 0.5)).any(), "fraction clamps at 1.5": (live & (frac > 1.5)).any(),
            "fraction between": (live & (frac > 0.5) & (frac < 1.5)).any()}


@pytest.mark.parametrize("gres", C.THIN_GRIDS + C.COVERAGE_GRIDS, ids=C.gid)
def test_both_branches_of_every_tap_and_comparison(gres):
    d = C.inputs(gres)
    cov = {**_lphi_coverage(d), **_face_coverage(d), **_density_coverage(d)}
    missing = [k for k, v in cov.items() if not v]
    assert not missing, missing


def test_the_one_interior_cell_of_333():
    d = C.inputs((3, 3, 3))
    cov = _lphi_coverage(d)
    assert d["lphi"][1, 1, 1] < 0
    assert any(cov[f"side{k} liquid neighbour"] for k in range(6)) and any(cov[f"side{k} air neighbour"] for k in range(6))
    L = d["lphi"]
    th = [float(O._theta(L[1, 1, 1], L[tuple(1 + s for s in side)])) for side in SIDES if not L[tuple(1 + s for s in side)] < 0]
    assert 0.01 in th and 1.0 in th


@pytest.mark.parametrize("gres", C.INTERIOR_GRIDS, ids=C.gid)
def test_boundary_cells_carry_both_signs(gres):
    d = C.inputs(gres)
    edge = d["lphi"][~C.interior(gres)]
    assert (edge < 0).any() and (edge >= 0).any()
    zeros = d["lphi"][d["lphi"] == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()            # 0.0 and -0.0
    for c in "xyz":
        assert np.isin(d["w" + c], C.W_SET).all()


@pytest.mark.parametrize("gres", C.COVERAGE_GRIDS, ids=C.gid)
def test_solid_fraction_inputs(gres):
    d = C.inputs(gres)
    Nx, Ny, Nz = gres
    s = d["sphi"]
    n = lambda ox, oy, oz: s[ox:ox + 2 * Nx:2, oy:oy + 2 * Ny:2, oz:oz + 2 * Nz:2]  # noqa: E731
    faces = [(n(0, 2, 0), n(0, 0, 0), n(0, 2, 2), n(0, 0, 2)), (n(2, 0, 0), n(0, 0, 0), n(2, 0, 2), n(0, 0, 2)),
             (n(2, 2, 0), n(0, 2, 0), n(2, 0, 0), n(0, 0, 0))]
    w = C.solid_frac(d)
    for a in range(3):
        inside = sum(_neg(v).astype(int) for v in faces[a])
        total = faces[a][0] + faces[a][1] + faces[a][2] + faces[a][3]
        assert sorted(set(inside.ravel())) == [0, 1, 2, 3, 4], a
        assert ((total == 0) & (inside > 0)).any(), a
        vals = w[a][:Nx, :Ny, :Nz]
        assert sorted(set(vals.ravel())) == [0.0, 0.5, 0.75, 1.0], a
        assert (vals[inside == 4] == 0).all() and (vals[inside <= 1] == 1).all()
        assert set(vals[inside == 3].ravel()) == {0.5, 1.0} and set(vals[inside == 2].ravel()) == {0.75, 1.0}
        assert (w[a][tuple(slice(-1, None) if b == a else slice(None) for b in range(3))] == 7.5).all()
    centre = s[1::2, 1::2, 1::2]
    assert (centre == min(C.CS)).any() and (centre < min(C.CS)).any() and ((centre > min(C.CS)) & (centre < max(C.CS))).any()
    assert (centre == 0).any() and (centre < 0).any() and (centre > max(C.CS)).any()
    assert len({float(abs(d["sv"][..., k]).max()) // 1 for k in range(3)}) == 3
    assert abs(d["sv"][..., 0]).max() < abs(d["sv"][..., 1]).min() and abs(d["sv"][..., 1]).max() < abs(d["sv"][..., 2]).min()


@pytest.mark.parametrize("gdt", [np.float32, np.float64], ids=["g32", "g64"])
@pytest.mark.parametrize("gres", C.INTERIOR_GRIDS, ids=C.gid)
def test_threshold_margins(gres, gdt):
    """no computed quantity that a kernel compares to a constant lies within 1e-6 relative of it, at either storage dtype
    of gm / gvol and of the weights"""
    d = C.inputs(gres)
    for wdt in (np.float32, np.float64):
        cell_mass, cell_vol, frac = _density_quantities(d, gdt, wdt)
        live = ~(cell_mass < 1e-10)
        for q, t in ((cell_mass, 1e-10), (cell_vol, 1e-10), (frac[live], 0.5), (frac[live], 1.5)):
            assert (np.abs(q - t) > 1e-6 * t).all(), (t, float(np.abs(q - t).min()))


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_particles(gres):
    for axis in range(3):
        shape = C.face_shape(gres, axis)
        assert C.particles(shape, axis, 0).shape == (0, 3)
        for P in (63, 257):
            px = C.particles(shape, axis, P)
            assert px.shape == (P, 3)
            gi, w = O._particle_cell(px, C.BMIN, C.CS, C.BIAS[axis])
            for a, (low, high, free) in enumerate(C.clamps(px, shape, axis)):
                assert low.any() and high.any(), (axis, a)
                assert free.any() == (shape[a] >= 2), (axis, a)
                # on a sample point the base index comes out as the point's own or the one below: corner weights 0 and 1.
                # Along y, cell size and origin are binary fractions, so every such point is exact; along x and z
                # (0.05, 0.04) only some indices reproduce themselves, and a shape with few samples may hold none
                exact = (w[:, a] == 0) | (w[:, a] == 1)
                assert exact.any() or (a != 1 and min(gres) < 9), (axis, a)
                assert ((w[:, a] > 0) & (w[:, a] < 1)).any(), (axis, a)
        _, _, free = zip(*C.clamps(C.particles(shape, axis, 1), shape, axis))
        assert all(f.all() == (shape[a] >= 2) for a, f in enumerate(free))


# ------------------------------------------------------------------------------------------------ the mistakes ---
def _all_true(a):
    return np.ones(np.shape(a), bool)


def _excess(kernel, mistake, d):
    """worst |mistaken - oracle| / bound over all outputs (inf where the bound is 0, as for the bit-exact kernels)"""
    if kernel == "solid_frac":
        base, alt = C.solid_frac(d), C.solid_frac(d, mistake=mistake)
        return max(float(C.ratio(y, x, 0.0, 0, C.U[F64], _all_true(x)).max()) for x, y in zip(base, alt))
    if kernel == "advect":
        worst = np.inf
        for axis in range(3):
            dval = d["v" + "xyz"[axis]]
            px = C.particles(dval.shape, axis, 257)
            base, alt = C.advect(px, dval, axis), C.advect(px, dval, axis, mistake=mistake)
            worst = min(worst, float((np.abs(alt - base)[:, axis] / (C.U[F64] * np.abs(base[:, axis]))).max()))
        return worst                     # the least over the axes: the mistake shows on each of them
    want, mag = C.call(kernel, d)
    alt, _ = C.call(kernel, d, mistake=mistake)
    return max(float(C.ratio(y, x, m, C.R[kernel], C.U[F64], _all_true(x)).max()) for x, y, m in zip(want, alt, mag))


@pytest.mark.parametrize("gres", C.COVERAGE_GRIDS, ids=C.gid)
def test_planted_mistakes_exceed_the_bound(gres):
    d = C.inputs(gres)
    low = []
    for name, kernel, mistake in C.MISTAKES:
        with np.errstate(all="ignore"):              # a mistaken copy may divide by zero; ratio() counts that as inf
            e = _excess(kernel, mistake, d)
        print(f"MISTAKE {C.gid(gres)} {name}: worst excess over the bound {e:.3g}")
        if not e >= 100:
            low.append((name, e))
    assert not low, low


def test_the_mistake_table_names_what_the_issue_lists():
    names = " | ".join(n for n, _, _ in C.MISTAKES)
    for needle in ("-z tap weighted by wz[z]", "diagonal counts 1", "theta floor removed", "w <= 1", "sv components swapped",
                   "cell sizes swapped (rhs)", "cell sizes swapped (update)", "cell sizes swapped (displacement)",
                   "lphi <= 0", "max(cell_size)", "wrong axis", "wrong four nodes", "bias of another axis"):
        assert needle in names, needle


@pytest.mark.parametrize("gres", C.INTERIOR_GRIDS, ids=C.gid)
def test_an_unmistaken_copy_and_a_reordered_sum_stay_within_the_bound(gres):
    """the copy mechanism changes nothing by itself, and a correct implementation that sums the taps in another order passes"""
    d = C.inputs(gres)
    differs = 0
    for kernel, fn, old, new in (("pressure_apply", "pressure_apply3d", "for off, w in nbrs:", "for off, w in nbrs[::-1]:"),
                                 ("density_apply", "density_apply3d", "for off, w in nbrs:", "for off, w in nbrs[::-1]:"),
                                 ("pressure_rhs", "pressure_rhs3d", "for w, v, sgn, c, s in terms:", "for w, v, sgn, c, s in terms[::-1]:")):
        want, mag = C.call(kernel, d)
        same, _ = C.call(kernel, d, mistake=(fn, old, old))
        np.testing.assert_array_equal(same[0], want[0])
        alt, _ = C.call(kernel, d, mistake=(fn, old, new))
        r = C.ratio(alt[0], want[0], mag[0], C.R[kernel], C.U[F64], _all_true(want[0])).max()
        assert r <= 1.0, (kernel, r)
        differs += r > 0
    assert differs or tuple(gres) == (3, 3, 3)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_magnitude_outputs_change_no_result(gres):
    """the oracle's results are the same to the bit with and without `mag=`, and the magnitudes bound the results"""
    d = C.inputs(gres)
    w = [d["wx"], d["wy"], d["wz"]]
    V = [d["v" + c] for c in "xyz"]
    pairs = []
    for mag in (None, {}):
        kw = {} if mag is None else {"mag": mag}
        b, out, out2, gvol, b2 = (np.full(gres, 7.0) for _ in range(5))
        v = [a.copy() for a in V]
        disp = [np.full(a.shape, 7.0) for a in V]
        O.pressure_rhs3d(C.CS, gres, *V, None, d["sv"], d["lphi"], b, *w, **kw)
        O.pressure_apply3d(gres, d["v"], out, *w, d["lphi"], **kw)
        O.pressure_update3d(gres, C.CS, *v, d["pv"], *w, d["sv"], d["lphi"], **kw)
        O.density_fix_volume3d(C.CS, gres, None, gvol, d["sphi"], d["lphi"], *w, **kw)
        O.density_rhs3d(C.RHO0, C.DT, gres, C.CS, d["gm"], d["gvol"], d["lphi"], *w, b2, **kw)
        O.density_apply3d(gres, d["v"], out2, *w, d["lphi"], **kw)
        O.density_displacement3d(gres, C.DT, C.CS, *disp, d["pv"], d["lphi"], **kw)
        pairs.append([b, out, *v, gvol, b2, out2, *disp])
    for x, y in zip(*pairs):
        np.testing.assert_array_equal(x, y)
    for kernel in C.R:
        want, mag = C.call(kernel, d, sentinel=0.0)
        for x, m, where in zip(want, mag, C.written(kernel, d)):
            assert m.shape == x.shape and (m >= 0).all()
            if kernel != "density_rhs":                       # there M is an error magnitude, not a bound of |b|
                assert (np.abs(x)[where] <= m[where] * (1 + 1e-12)).all(), kernel
