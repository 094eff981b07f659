"""The stateless 3D face-grid kernels of csrc/mfs_visc.hip on the MI355X against the numpy oracle in float64 on the same
rounded inputs: extrapolate (both validity forms, and the slab path's one-sweep entry points), the rows (rhs, apply), the
write-back and the boundary condition -- at every dtype code, on grids of extent 1, 2 and 3, with one long axis in each
position, and with odd extents whose rows cross 256-thread blocks; sweep counts 0 to 3.  Inputs, grids and the derivation
of the bounds are in tests/grid_kernels3d_inputs.py; tests/test_grid_kernels3d_inputs.py shows on the CPU that those
inputs reach every tap, sample, sweep and category of face, and that a wrong tap exceeds the bound a hundred times over.

Extrapolate, the one-sweep entry points and the write-back are exact (bit for bit).  The rows and the boundary condition
hold |got - want| <= (R + 2) 2^-53 M + u_out |want| per face, with R = 17 (rhs), 23 (apply), 25 (boundary condition)
counted from the kernel source and M the oracle's magnitude output.

Every output array is a contiguous view inside a larger flat buffer filled with PAD; the padding on both sides is checked
after every call, so a store next to an array fails the test.

Measured on the MI355X, worst err / bound over all grids and dtype codes (the RATIO lines that the tests print):
  into float64 outputs   rhs 0.1522   apply 0.1433   boundary condition 0.1404
  into float32 outputs   rhs 0.9967   apply 0.9993   boundary condition 0.9959   (the rounding of the store alone reaches
                         u_out |want|, so these approach 1 by construction)
"""
import itertools

import numpy as np
import pytest
import torch

import grid_kernels3d_inputs as G
from mfs import _lib, tensors as TT
from oracle import mfs_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
TD = {F32: torch.float32, F64: torch.float64}
CODE = {F32: _lib.MFS_F32, F64: _lib.MFS_F64}
nm = lambda *dts: "".join("s" if dt is F32 else "d" for dt in dts)  # noqa: E731
SENT, PAD, PAD_U8, NPAD = 7.5, -3.25, 165, 256      # faces that a kernel must leave alone; padding (floats, bytes) and its length
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731


class Padded:
    """an array of `shape` as a contiguous view in the middle of a flat buffer whose ends hold PAD"""

    def __init__(self, shape, dtype, fill=SENT):
        n = int(np.prod(shape))
        self.pad = PAD_U8 if dtype == torch.uint8 else PAD
        self.buf = torch.full((n + 2 * NPAD,), self.pad, dtype=dtype, device=DEV)
        self.t = self.buf[NPAD:NPAD + n].view(tuple(shape))
        assert self.t.is_contiguous() and self.t.data_ptr() % 256 == 0
        if isinstance(fill, np.ndarray):
            self.t.copy_(T(fill))
        else:
            self.t.fill_(fill)

    def np(self):
        """the array on the host, after checking that the padding still holds PAD"""
        torch.cuda.synchronize()
        b = N(self.buf)
        assert (b[:NPAD] == self.pad).all() and (b[-NPAD:] == self.pad).all(), "a store landed outside the array"
        return b[NPAD:-NPAD].reshape(tuple(self.t.shape)).copy()

    @property
    def ptr(self):
        return TT.ptr(self.t)


def padded3(arrays_or_shapes, npdt, fill=SENT):
    return [Padded(a.shape, TD[npdt], a.astype(npdt)) if isinstance(a, np.ndarray) else Padded(a, TD[npdt], fill)
            for a in arrays_or_shapes]


def shapes(gres):
    return [G.face_shape(gres, a) for a in range(3)]


def refused(status, words):
    assert status < 0
    assert words in _lib.load().mfs_last_error().decode(errors="replace")


WORST = {}


def note(kernel, r, what):
    """keeps the worst err / bound per kernel and output dtype (a float32 store alone comes close to 1: its rounding error
    reaches u_out |want|); r: ratio array of one case"""
    worst = float(r.max()) if r.size else 0.0
    WORST[kernel] = max(WORST.get(kernel, 0.0), worst)
    assert worst <= 1.0, (f"{what}: worst err / bound {worst:.4g} at face {np.unravel_index(r.argmax(), r.shape)}; "
                          f"{int((r > 1).sum())} faces over")


def report(*kernels):
    for k in sorted(WORST):
        if k.split(" -> ")[0] in kernels:
            print(f"RATIO {k}: worst err / bound so far {WORST[k]:.4f}")


# --------------------------------------------------------------------------------------------------- 1. extrapolate ---
def _oracle_extrapolate(d, form, k, vdt, xdt, valid_out=None):
    v = [d["v" + c].astype(vdt) for c in "xyz"]
    if form == "sphi":
        O.visc_extrapolate3d(d["gres"], k, *v, G.rounded(d["sphi"], xdt), valid_out=valid_out)
    else:
        O.nb_extrapolate(d["gres"], k, *v, *[d["m" + c].astype(xdt) for c in "xyz"], valid_out=valid_out)
    return v


@pytest.mark.parametrize("form", ["sphi", "mass"])
@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_extrapolate(gres, form):
    """mfs_visc_extrapolate3d (validity sphi >= 0) and mfs_grid_extrapolate3d (mass > 0): bit-equal to the oracle for
    velocities x sphi-or-mass in {float32, float64} and 0 to 3 sweeps (odd counts end in the workspace and are copied
    back); 0 sweeps and components without an interior face leave the arrays as they were; the reported workspace size is
    accepted, one byte less is refused before any write"""
    lib, gi, d = _lib.load(), _lib.i64x(gres), G.inputs(gres)
    for vdt, xdt in itertools.product(DTYPES, DTYPES):
        nbytes = int(lib.mfs_visc_extrapolate3d_workspace_bytes(gi, CODE[vdt]))
        assert nbytes > 0
        x = T(G.rounded(d["sphi"], xdt).astype(xdt)) if form == "sphi" else [T(d["m" + c].astype(xdt)) for c in "xyz"]

        def run(k, v, ws, size):
            if form == "sphi":
                return lib.mfs_visc_extrapolate3d(gi, k, *[p.ptr for p in v], CODE[vdt], TT.ptr(x), CODE[xdt], ws.ptr, size,
                                                  TT.stream())
            return lib.mfs_grid_extrapolate3d(gi, k, *[p.ptr for p in v], CODE[vdt], *[TT.ptr(m) for m in x], CODE[xdt],
                                              ws.ptr, size, TT.stream())

        v0 = [d["v" + c].astype(vdt) for c in "xyz"]
        for k in range(4):
            v, ws = padded3(v0, vdt), Padded((nbytes,), torch.uint8, 0)
            assert run(k, v, ws, nbytes) == 0, lib.mfs_last_error()
            want = _oracle_extrapolate(d, form, k, vdt, xdt)
            ws.np()
            for a in range(3):
                got = v[a].np()
                assert got.dtype == vdt
                np.testing.assert_array_equal(got, want[a], err_msg=f"{form} {nm(vdt, xdt)} k={k} component {a}")
                if k == 0 or min(got.shape) < 3:
                    np.testing.assert_array_equal(got, v0[a])
        v, ws = padded3(v0, vdt), Padded((nbytes,), torch.uint8, 5)
        refused(run(3, v, ws, nbytes - 1), "workspace too small")
        assert (ws.np() == 5).all()
        for a in range(3):
            np.testing.assert_array_equal(v[a].np(), v0[a])


# ------------------------------------------------------------------------------------- 2. the one-sweep entry points ---
@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_one_sweep_entry_points(gres):
    """mfs_visc_valid3d: the oracle's validity bytes per component and sphi dtype.  mfs_visc_extrapolate_sweep3d: values
    and validity bytes of the oracle after each of three sweeps, from both validity forms; aliased arrays are refused"""
    lib, gi, d = _lib.load(), _lib.i64x(gres), G.inputs(gres)
    for sdt in DTYPES:
        sphi = T(G.rounded(d["sphi"], sdt).astype(sdt))
        for a in range(3):
            valid = Padded(shapes(gres)[a], torch.uint8, 9)
            assert lib.mfs_visc_valid3d(gi, a, TT.ptr(sphi), CODE[sdt], valid.ptr, TT.stream()) == 0
            want = G.face_of_doubled(G.rounded(d["sphi"], sdt), a) >= 0
            np.testing.assert_array_equal(valid.np(), want.astype(np.uint8))
    for form, vdt in itertools.product(("sphi", "mass"), DTYPES):
        start = []
        _oracle_extrapolate(d, form, 0, vdt, F64, valid_out=start)
        for a in range(3):
            shp = shapes(gres)[a]
            vin, bin_ = Padded(shp, TD[vdt], d["v" + "xyz"[a]].astype(vdt)), Padded(shp, torch.uint8, start[a].astype(np.uint8))
            for k in range(1, 4):
                vout, bout = Padded(shp, TD[vdt]), Padded(shp, torch.uint8, 9)
                assert lib.mfs_visc_extrapolate_sweep3d(gi, a, vin.ptr, vout.ptr, CODE[vdt], bin_.ptr, bout.ptr, TT.stream()) == 0
                wv = []
                want = _oracle_extrapolate(d, form, k, vdt, F64, valid_out=wv)
                what = f"{form} {nm(vdt)} component {a} sweep {k}"
                np.testing.assert_array_equal(vout.np(), want[a], err_msg=what)
                np.testing.assert_array_equal(bout.np(), wv[a].astype(np.uint8), err_msg=what)
                vin, bin_ = vout, bout
            ov, ob = Padded(shp, TD[vdt]), Padded(shp, torch.uint8, 9)
            sweep = lib.mfs_visc_extrapolate_sweep3d
            refused(sweep(gi, a, vin.ptr, vin.ptr, CODE[vdt], bin_.ptr, ob.ptr, TT.stream()), "a sweep reads")
            refused(sweep(gi, a, vin.ptr, ov.ptr, CODE[vdt], bin_.ptr, bin_.ptr, TT.stream()), "a sweep reads")
            assert (ov.np() == SENT).all() and (ob.np() == 9).all()
            np.testing.assert_array_equal(vin.np(), want[a])
            np.testing.assert_array_equal(bin_.np(), wv[a].astype(np.uint8))


# ------------------------------------------------------------------------------------------------------- 3. the rows ---
@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_rows(gres):
    """mfs_visc_rhs3d and mfs_visc_apply3d at all 16 combinations of the (v, out, sphi, vol) dtype codes and two
    magnitudes of scale * mu: array-boundary faces keep SENT, solid faces are exactly 0.0, every other face is within
    (R + 2) 2^-53 S + u_out |want| (R = 17 rhs, 23 apply); apply in place is refused"""
    lib, gi, d = _lib.load(), _lib.i64x(gres), G.inputs(gres)
    inner = [G.interior(s) for s in shapes(gres)]
    for vdt, sdt, voldt in itertools.product(DTYPES, DTYPES, DTYPES):
        v = [T(d["v" + c].astype(vdt)) for c in "xyz"]
        sphi, vol = T(d["sphi"].astype(sdt)), T(d["vol"].astype(voldt))
        solid = [inner[a] & (G.face_of_doubled(G.rounded(d["sphi"], sdt), a) < 0) for a in range(3)]
        for (scale, mu), rhs in itertools.product(G.KS, (True, False)):
            want, mag = G.rows(d, scale, mu, rhs, vdt, sdt, voldt, sentinel=SENT)
            for odt in DTYPES:
                out = padded3(shapes(gres), odt)
                if rhs:
                    st = lib.mfs_visc_rhs3d(gi, scale, mu, *[TT.ptr(t) for t in v], CODE[vdt], TT.ptr(sphi), CODE[sdt],
                                            TT.ptr(vol), CODE[voldt], *[p.ptr for p in out], CODE[odt], TT.stream())
                else:
                    st = lib.mfs_visc_apply3d(gi, scale, mu, *[TT.ptr(t) for t in v], CODE[vdt], *[p.ptr for p in out],
                                              CODE[odt], TT.ptr(sphi), CODE[sdt], TT.ptr(vol), CODE[voldt], TT.stream())
                assert st == 0, lib.mfs_last_error()
                kernel = "rhs" if rhs else "apply"
                what = f"{kernel} {G.gid(gres)} {nm(vdt, odt, sdt, voldt)} scale*mu {scale * mu}"
                for a in range(3):
                    got = out[a].np()
                    assert got.dtype == odt
                    assert (got[~inner[a]] == SENT).all(), what + ": an array-boundary face was written"
                    assert (got[solid[a]] == 0.0).all(), what + ": a solid face is not 0.0"
                    assert (want[a][solid[a]] == 0.0).all() and (want[a][~inner[a]] == SENT).all()
                    note(f"{kernel} -> {np.dtype(odt).name}",
                         G.ratio(got, want[a], mag[a], G.R_RHS if rhs else G.R_APPLY, G.U[odt], inner[a] & ~solid[a]),
                         f"{what} component {a}")
    report("rhs", "apply")
    out = padded3(shapes(gres), vdt)
    for alias in range(3):
        o = [v[a] if a == alias else out[a].t for a in range(3)]
        refused(lib.mfs_visc_apply3d(gi, 1.0, 1.0, *[TT.ptr(t) for t in v], CODE[vdt], *[TT.ptr(t) for t in o], CODE[vdt],
                                     TT.ptr(sphi), CODE[sdt], TT.ptr(vol), CODE[voldt], TT.stream()), "in place")
    for a in range(3):
        assert (out[a].np() == SENT).all()
        np.testing.assert_array_equal(N(v[a]), d["v" + "xyz"[a]].astype(vdt))


# ------------------------------------------------------------------------------------------------- 4. the write-back ---
@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_writeback(gres):
    """mfs_visc_writeback3d at the 8 combinations of the (v, out, sphi) dtype codes: bit-equal to visc_writeback3d, the
    rounding of a float64 solution into float32 velocities included; faces of cells with x, y or z == 0, the last face
    plane on each component's own axis and solid faces keep their old value (which differs from the solution everywhere)"""
    lib, gi, d = _lib.load(), _lib.i64x(gres), G.inputs(gres)
    for vdt, odt, sdt in itertools.product(DTYPES, DTYPES, DTYPES):
        v0 = [d["v" + c].astype(vdt) for c in "xyz"]
        o = [d["out" + c].astype(odt) for c in "xyz"]
        sphi = G.rounded(d["sphi"], sdt)
        v, ot, st = padded3(v0, vdt), [T(a) for a in o], T(sphi.astype(sdt))
        assert lib.mfs_visc_writeback3d(gi, *[p.ptr for p in v], CODE[vdt], *[TT.ptr(t) for t in ot], CODE[odt], TT.ptr(st),
                                        CODE[sdt], TT.stream()) == 0, lib.mfs_last_error()
        want = [a.copy() for a in v0]
        O.visc_writeback3d(gres, *want, *o, sphi)
        for a in range(3):
            got, what = v[a].np(), f"writeback {G.gid(gres)} {nm(vdt, odt, sdt)} component {a}"
            np.testing.assert_array_equal(got, want[a], err_msg=what)
            keep = np.ones(got.shape, bool)
            keep[1:, 1:, 1:] = False
            keep[tuple(slice(-1, None) if k == a else slice(None) for k in range(3))] = True
            keep |= G.face_of_doubled(sphi, a) < 0
            assert (o[a].astype(vdt) != v0[a]).all()
            assert (got[keep] == v0[a][keep]).all(), what + ": a face outside the write-back's range changed"
            assert (got[~keep] == o[a].astype(vdt)[~keep]).all(), what
            np.testing.assert_array_equal(N(ot[a]), o[a])


# ----------------------------------------------------------------------------------------- 5. the boundary condition ---
def _bc_patterns():
    """all-float32, all-float64 and every single-code deviation from each, over (v, m, sphi, sv, dv): both settings of the
    float32-product rule"""
    out = []
    for base in DTYPES:
        other = F64 if base is F32 else F32
        out.append((base,) * 5)
        out += [tuple(other if k == j else base for k in range(5)) for j in range(5)]
    return out


@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_boundary_condition(gres):
    """mfs_grid_boundary_condition3d: every element of dv is overwritten; array-boundary faces, faces with sphi/dx >= 1 and
    faces with an averaged mass of zero are 0.0; every other face is within (25 + 2) 2^-53 A + u_out |want|; NaN exactly
    where the oracle has NaN (the flat patch of sphi on (17,19,23)).  Through notebook_kernels.apply_boundary_condition
    where v and dv share a dtype: v afterwards is v + dv in that dtype, bit for bit, for the dv that the kernel wrote"""
    import types

    import notebook_kernels as NK
    lib, gi, d = _lib.load(), _lib.i64x(gres), G.inputs(gres)
    NS = types.SimpleNamespace
    for vdt, mdt, sdt, svdt, dvdt in _bc_patterns():
        v0 = [d["v" + c].astype(vdt) for c in "xyz"]
        v, dv = padded3(v0, vdt), padded3(shapes(gres), dvdt, 9.0)
        m = [T(d["m" + c].astype(mdt)) for c in "xyz"]
        sphi, sv = T(d["sphi"].astype(sdt)), T(d["sv"].astype(svdt))
        if vdt is dvdt:
            grid = NS(**{c: NS(v=v[a].t, m=m[a], dv=dv[a].t) for a, c in enumerate("xyz")})
            NK.apply_boundary_condition(grid, NS(phi=sphi, v=sv), d["dx"])
        else:
            assert lib.mfs_grid_boundary_condition3d(gi, *[p.ptr for p in v], CODE[vdt], *[TT.ptr(t) for t in m], CODE[mdt],
                                                     TT.ptr(sphi), CODE[sdt], TT.ptr(sv), CODE[svdt], d["dx"],
                                                     *[p.ptr for p in dv], CODE[dvdt], TT.stream()) == 0, lib.mfs_last_error()
        want, mag = G.boundary_condition(d, vdt, mdt, sdt, svdt)
        for a in range(3):
            got, what = dv[a].np(), f"boundary condition {G.gid(gres)} {nm(vdt, mdt, sdt, svdt, dvdt)} component {a}"
            edge, far, empty, rest = G.bc_categories(d, a, mdt, sdt)
            assert got.dtype == dvdt and (got != 9.0).all(), what + ": an element of dv was not written"
            nan = np.isnan(want[a])
            np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
            assert nan.any() == (tuple(gres) == G.FLAT_GRID) and not nan[edge | far].any()
            assert (got[edge] == 0.0).all(), what + ": array-boundary faces"
            assert (got[far] == 0.0).all(), what + ": faces at least dx from the solid"
            assert (got[empty & ~nan] == 0.0).all(), what + ": faces without averaged mass"
            note(f"boundary condition -> {np.dtype(dvdt).name}", G.ratio(got, want[a], mag[a], G.R_BC, G.U[dvdt], ~nan), what)
            after = v[a].np()
            if vdt is dvdt:
                with np.errstate(invalid="ignore"):
                    np.testing.assert_array_equal(after, v0[a] + got, err_msg=what + ": v + dv")
            else:
                np.testing.assert_array_equal(after, v0[a])
    report("boundary condition")
