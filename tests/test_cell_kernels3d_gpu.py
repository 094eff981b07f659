"""The nine stateless 3D cell kernels of csrc/mfs_pressure.hip (solid fraction, pressure rhs / apply / update) and
csrc/mfs_density.hip (fix_volume, rhs, apply, displacement, advect) on the MI355X against the numpy oracle in float64 on
the same rounded inputs, through the module functions of solver/SolidFraction3D.py, solver/PressureCGSolver3D.py and
solver/DensityCGSolver3D.py (the C ABI directly only for the refusals and for P = 0): every dtype code differing alone in
both directions, grids of extent 1, 2 and 3, one long axis in each position, odd extents whose rows cross 256-thread
blocks.  Inputs, planted mistakes and the derivation of the bounds are in tests/cell_kernels3d_inputs.py;
tests/test_cell_kernels3d_inputs.py shows on the CPU that those inputs reach both branches of every tap and comparison
and that each planted mistake exceeds the bound a hundred times over.

The solid fraction and the advect are exact (bit for bit; the advect in both position dtypes).  The other seven hold
|got - want| <= (R + 2) 2^-53 M + u_out |want| per written entry, R counted from the kernel source (C.R) and M the
oracle's magnitude output; entries that a kernel does not write are compared bit for bit with what they held, NaN
sentinels included.  Every output array is a contiguous view inside a larger flat buffer filled with PAD; the padding on
both sides is checked after every call, so a store next to an array fails the test.

Measured on the MI355X, worst err / bound over all grids and dtype patterns (the RATIO lines that the tests print):
  into float64 outputs   pressure rhs 0.0000   pressure apply 0.1424   pressure update 0.1802   fix_volume 0.0000
                         density rhs 0.0000    density apply 0.0000    displacement 0.0000
                         (0.0000: bit for bit.  Only the pressure apply and update hold an a * b + c that the compiler
                         contracts; mfs_density.hip has contraction off, and the pressure rhs divides between its
                         product and its add)
  into float32 outputs   pressure rhs 0.9984   pressure apply 0.9986   pressure update 0.9998   fix_volume 0.9681
                         density rhs 0.9829    density apply 0.9986    displacement 0.9961   (the rounding of the store
                         alone reaches u_out |want|, so these approach 1 by construction)
  solid fraction and advect: bit for bit in every case, the advect in float64 and float32 positions alike.
"""
import itertools

import numpy as np
import pytest
import torch

import cell_kernels3d_inputs as C
from mfs import _lib, tensors as TT
from solver import DensityCGSolver3D as D3, PressureCGSolver3D as P3, SolidFraction3D as S3
from test_grid_kernels3d_gpu import CODE, TD, Padded, T, note, refused, report

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
SENT = 7.5
INT = {F32: np.int32, F64: np.int64}
GROUPS = dict(pressure_rhs=("v", "sv", "lphi", "w", "b"), pressure_apply=("v", "w", "lphi"),
              pressure_update=("v", "pv", "w", "sv", "lphi"), fix_volume=("g", "sphi", "lphi", "w"),
              density_rhs=("g", "lphi", "w", "b"), density_apply=("v", "w", "lphi"), displacement=("d", "pv", "lphi"))
OUT = dict(pressure_rhs="b", pressure_apply="v", pressure_update="v", fix_volume="g", density_rhs="b", density_apply="v",
           displacement="d")
ZEROED = ("pressure_rhs", "pressure_apply", "density_rhs", "density_apply")        # non-fluid interior cells get 0.0


def patterns(names):
    """all-float64, all-float32, and every one-group-differs pattern in both directions; any two groups differ in one"""
    out = [{n: F64 for n in names}, {n: F32 for n in names}]
    for n in names:
        out.append({m: (F32 if m == n else F64) for m in names})
        out.append({m: (F64 if m == n else F32) for m in names})
    for a in names:
        for b in names:
            assert a == b or any(p[a] != p[b] for p in out)
    return out


def pid(p):
    return ",".join(f"{k}{'32' if v is F32 else '64'}" for k, v in p.items())


def bits(a):
    return np.ascontiguousarray(a).view(INT[a.dtype.type])


def _launch(kernel, d, p, sentinel):
    """runs `kernel` through its module function on the inputs at the dtypes `p`; returns (outputs as Padded, what each held)"""
    g = d["gres"]
    up = lambda key, grp: T(d[key].astype(p[grp]))  # noqa: E731
    w = [up(k, "w") for k in ("wx", "wy", "wz")] if "w" in p else None
    lphi = up("lphi", "lphi")
    odt = p[OUT[kernel]]
    if kernel in ("pressure_update",):
        init = [d["v" + c].astype(odt) for c in "xyz"]
    elif kernel == "fix_volume":
        init = [np.where(C.interior(g), d["gvol"], sentinel).astype(odt)]
    elif kernel == "displacement":
        init = [np.full(C.face_shape(g, a), sentinel, odt) for a in range(3)]
    else:
        init = [np.full(g, sentinel, odt)]
    out = [Padded(a.shape, TD[odt], a) for a in init]
    if kernel == "pressure_rhs":
        P3.initialize_solver(C.CS, g, up("vx", "v"), up("vy", "v"), up("vz", "v"), None, up("sv", "sv"), lphi, out[0].t, *w)
    elif kernel == "pressure_apply":
        P3.matvecmul(g, up("v", "v"), out[0].t, *w, lphi)
    elif kernel == "pressure_update":
        P3.apply_pressure(g, C.CS, *[o.t for o in out], up("pv", "pv"), *w, up("sv", "sv"), lphi)
    elif kernel == "fix_volume":
        D3.fix_volume(C.CS, g, None, out[0].t, up("sphi", "sphi"), lphi, *w)
    elif kernel == "density_rhs":
        D3.initialize_solver(C.RHO0, C.DT, g, C.CS, up("gm", "g"), up("gvol", "g"), lphi, *w, out[0].t)
    elif kernel == "density_apply":
        D3.matvecmul(g, up("v", "v"), out[0].t, *w, lphi)
    elif kernel == "displacement":
        D3.compute_displacement(g, C.DT, C.CS, *[o.t for o in out], up("pv", "pv"), lphi)
    return out, init


def _check_bounded(kernel, gres):
    d = C.inputs(gres)
    for k, p in enumerate(patterns(GROUPS[kernel])):
        sentinel = np.nan if k % 5 == 0 else SENT
        out, init = _launch(kernel, d, p, sentinel)
        want, mag = C.call(kernel, d, p, sentinel=sentinel)
        masks = C.written(kernel, d, p)
        odt = p[OUT[kernel]]
        for a, (o, was, wnt, M, wr) in enumerate(zip(out, init, want, mag, masks)):
            got, what = o.np(), f"{kernel} {C.gid(gres)} {pid(p)} output {a}"
            assert got.dtype == odt
            zeroed = np.zeros(wr.shape, bool)
            if kernel in ZEROED:
                zeroed = C.interior(gres) & ~wr
                assert (bits(got)[zeroed] == 0).all(), what + ": a non-fluid interior cell is not 0.0"
                assert (wnt[zeroed] == 0).all()
            keep = ~wr & ~zeroed
            assert (bits(got)[keep] == bits(was)[keep]).all(), what + ": an entry outside the kernel's range changed"
            if min(gres) < 3 and kernel not in ("pressure_update", "displacement"):
                assert keep.all()
            if kernel in ("pressure_update", "displacement") and tuple(gres) in C.WRITING_GRIDS:
                assert wr.any() and (bits(got)[wr] != bits(was)[wr]).any(), what + ": no face was written"
            if kernel == "displacement":
                assert (bits(got)[wr] != bits(was)[wr]).all(), what + ": a face in the kernel's range kept the sentinel"
            note(f"{kernel} -> {np.dtype(odt).name}", C.ratio(got, wnt, M, C.R[kernel], C.U[odt], wr), what)
    report(kernel)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_pressure_rhs(gres):
    """mfs_pressure_rhs3d at the 12 patterns of (v, sv, lphi, w, b): fluid interior cells within the bound (R = 14), non-fluid
    interior cells exactly 0.0, boundary cells and grids without an interior cell untouched, bit for bit"""
    _check_bounded("pressure_rhs", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_pressure_apply(gres):
    """mfs_pressure_apply3d at the 8 patterns of (v and out, w, lphi): as the rhs, R = 11"""
    _check_bounded("pressure_apply", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_pressure_update(gres):
    """mfs_pressure_update3d at the 12 patterns of (v, pv, w, sv, lphi), in place: active faces with x, y, z >= 1 within the
    bound (R = 8); inactive faces, the planes at index 0 and v*[N] bit for bit as given; (2,2,2) and (2,5,3) write faces"""
    _check_bounded("pressure_update", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_density_fix_volume(gres):
    """mfs_density_fix_volume3d at the 10 patterns of (gvol, sphi, lphi, w), in place: interior cells within the bound (R = 9),
    boundary cells (which hold the sentinel) untouched"""
    _check_bounded("fix_volume", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_density_rhs(gres):
    """mfs_density_rhs3d at the 10 patterns of (gm and gvol, lphi, w, b): as the pressure rhs, R = 16 with the oracle's
    amplified magnitude; cells of zero mass give exactly 0"""
    _check_bounded("density_rhs", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_density_apply(gres):
    """mfs_density_apply3d at the 8 patterns of (v and out, w, lphi): as the pressure apply, R = 11"""
    _check_bounded("density_apply", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_density_displacement(gres):
    """mfs_density_displacement3d at the 8 patterns of (d, pv, lphi): every face with x, y, z >= 1 below d*[N] within the
    bound (R = 6) and written (no sentinel left), every other face untouched; (2,2,2) and (2,5,3) write faces"""
    _check_bounded("displacement", gres)


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_solid_fraction(gres):
    """mfs_solid_frac3d for sphi x w in {float32, float64}: bit for bit the oracle's quarters on the rounded sphi; the
    planes wx[Nx], wy[:, Ny], wz[:, :, Nz] keep the sentinel (NaN for float64 sphi)"""
    d = C.inputs(gres)
    for sdt, wdt in itertools.product(DTYPES, DTYPES):
        sentinel = np.nan if sdt is F64 else SENT
        w = [Padded(C.face_shape(gres, a), TD[wdt], np.full(C.face_shape(gres, a), sentinel, wdt)) for a in range(3)]
        S3.compute_solid_frac(gres, T(d["sphi"].astype(sdt)), *[p.t for p in w])
        want = C.solid_frac(d, sdt, fill=sentinel)
        for a in range(3):
            got = w[a].np()
            assert got.dtype == wdt
            np.testing.assert_array_equal(bits(got), bits(want[a].astype(wdt)), err_msg=f"{C.gid(gres)} s{sdt.__name__} w{wdt.__name__} {a}")
            top = got[tuple(slice(-1, None) if b == a else slice(None) for b in range(3))]
            assert (bits(top) == bits(np.full(top.shape, sentinel, wdt))).all()


@pytest.mark.parametrize("gres", C.GRIDS, ids=C.gid)
def test_advect(gres):
    """mfs_density_advect3d for px x d in {float32, float64}, the three axes with their biases and face shapes, P in
    {0, 1, 63, 257}: the whole position array is bit for bit the oracle's (FMA contraction is off in mfs_density.hip and the
    kernel performs the oracle's IEEE operations in its order), so the other two columns are unchanged; P = 0 returns MFS_OK"""
    lib, d = _lib.load(), C.inputs(gres)
    for axis, P, pdt, ddt in itertools.product(range(3), C.PARTICLE_COUNTS, DTYPES, DTYPES):
        dval = d["v" + "xyz"[axis]]
        px0 = C.particles(dval.shape, axis, P).astype(pdt)
        px, dt = Padded((P, 3), TD[pdt], px0), T(dval.astype(ddt))
        if P == 0:
            assert lib.mfs_density_advect3d(px.ptr, CODE[pdt], 0, TT.ptr(dt), CODE[ddt], _lib.i64x(dval.shape), _lib.f64x(C.BMIN),
                                            _lib.f64x(C.CS), _lib.f64x(C.BIAS[axis]), axis, TT.stream()) == _lib.MFS_OK
        D3.apply_displacement(px.t, dt, C.BMIN, C.CS, C.BIAS[axis], axis)
        got, want = px.np(), C.advect(px0, dval, axis, pdt, ddt)
        what = f"advect {C.gid(gres)} axis {axis} P {P} px {pdt.__name__} d {ddt.__name__}"
        assert got.dtype == pdt and got.shape == (P, 3)
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)
        other = [c for c in range(3) if c != axis]
        assert (bits(got)[:, other] == bits(px0)[:, other]).all(), what
        assert P == 0 or (got[:, axis] != px0[:, axis]).any(), what


def test_refusals():
    """v == out in either apply, a dtype code outside the two in every position of every entry, an extent of 0 or 4097,
    dshape 4098 and axis 3: a negative status with a message before any launch; no array changes"""
    lib, g = _lib.load(), (3, 3, 3)
    gi, cs, s = _lib.i64x(g), _lib.f64x(C.CS), TT.stream()
    fx, fy, fz = (Padded(C.face_shape(g, a), torch.float64) for a in range(3))
    c1, c2, c3 = (Padded(g, torch.float64) for _ in range(3))
    dg, dg3 = Padded(C.doubled_shape(g), torch.float64), Padded(C.doubled_shape(g) + (3,), torch.float64)
    px = Padded((5, 3), torch.float64)
    f = [a.ptr for a in (fx, fy, fz)]
    entries = {   # name: (call with (gres, dtype codes...), number of codes)
        "mfs_solid_frac3d": (lambda G, a, b: lib.mfs_solid_frac3d(G, dg.ptr, a, *f, b, s), 2),
        "mfs_pressure_rhs3d": (lambda G, a, b, c, e, h: lib.mfs_pressure_rhs3d(G, cs, *f, a, dg3.ptr, b, c1.ptr, c, *f, e, c2.ptr, h, s), 5),
        "mfs_pressure_apply3d": (lambda G, a, b, c: lib.mfs_pressure_apply3d(G, c1.ptr, c2.ptr, a, *f, b, c3.ptr, c, s), 3),
        "mfs_pressure_update3d": (lambda G, a, b, c, e, h: lib.mfs_pressure_update3d(G, cs, *f, a, c1.ptr, b, *f, c, dg3.ptr, e, c2.ptr, h, s), 5),
        "mfs_density_fix_volume3d": (lambda G, a, b, c, e: lib.mfs_density_fix_volume3d(G, cs, c1.ptr, a, dg.ptr, b, c2.ptr, c, *f, e, s), 4),
        "mfs_density_rhs3d": (lambda G, a, b, c, e: lib.mfs_density_rhs3d(G, C.RHO0, C.DT, cs, c1.ptr, c2.ptr, a, c3.ptr, b, *f, c, c1.ptr, e, s), 4),
        "mfs_density_apply3d": (lambda G, a, b, c: lib.mfs_density_apply3d(G, c1.ptr, c2.ptr, a, *f, b, c3.ptr, c, s), 3),
        "mfs_density_displacement3d": (lambda G, a, b, c: lib.mfs_density_displacement3d(G, C.DT, cs, *f, a, c1.ptr, b, c2.ptr, c, s), 3),
    }
    ok = _lib.MFS_F64
    for name, (fn, ncodes) in entries.items():
        for k, bad in itertools.product(range(ncodes), (2, -1)):
            refused(fn(gi, *[bad if j == k else ok for j in range(ncodes)]), "dtype")
        for a, n in itertools.product(range(3), (0, 4097)):
            refused(fn(_lib.i64x([n if b == a else 3 for b in range(3)]), *[ok] * ncodes), "grid resolution out of range")
    refused(lib.mfs_pressure_apply3d(gi, c1.ptr, c1.ptr, ok, *f, ok, c3.ptr, ok, s), "in place")
    refused(lib.mfs_density_apply3d(gi, c1.ptr, c1.ptr, ok, *f, ok, c3.ptr, ok, s), "in place")
    bmin, bias = _lib.f64x(C.BMIN), _lib.f64x(C.BIAS[0])
    advect = lambda pc, dc, shape, axis: lib.mfs_density_advect3d(px.ptr, pc, 5, fx.ptr, dc, _lib.i64x(shape), bmin, cs, bias, axis, s)  # noqa: E731
    refused(advect(2, ok, fx.t.shape, 0), "dtype")
    refused(advect(ok, 2, fx.t.shape, 0), "dtype")
    refused(advect(ok, ok, fx.t.shape, 3), "axis")
    refused(advect(ok, ok, fx.t.shape, -1), "axis")
    for a, n in itertools.product(range(3), (0, 4098)):
        refused(advect(ok, ok, [n if b == a else 3 for b in range(3)], 0), "array shape")
    for arr in (fx, fy, fz, c1, c2, c3, dg, dg3, px):
        assert (arr.np() == 7.5).all()
