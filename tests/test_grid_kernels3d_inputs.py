"""CPU checks on the inputs and bounds of tests/test_grid_kernels3d_gpu.py (tests/grid_kernels3d_inputs.py): the generated
fields reach every tap, every diagonal factor, every averaged sample, every sweep and every category of face that the GPU
tests claim to pin, a wrong tap would exceed the bound a hundred times over, and a correct implementation that merely
sums in another order stays within it."""
import copy

import numpy as np
import pytest

import grid_kernels3d_inputs as G
from oracle import mfs_oracle as O

F64 = np.float64

# Taps of VISC_ROWS that a grid's inputs do not exercise (dropping the tap changes no face by more than 100 bounds), by
# row: a thin grid has no solid (rhs) or no fluid (apply) mask sample across its thin axes for them.  Everything not
# listed is exercised; the grids with three long axes leave out nothing, so neither does the union.
LEFT_OUT = {
    ((3, 3, 3), True): {0: [0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12], 1: [0, 1, 2, 4, 5, 6, 7, 8, 10, 11, 12],
                        2: [0, 1, 2, 3, 4, 6, 7, 8, 10, 11, 12, 13]},
    ((3, 3, 3), False): {0: [0, 1, 4, 9, 10, 11, 13], 1: [3, 9, 13], 2: [0, 3, 5, 6, 7, 9, 12, 13]},
    ((70, 3, 3), True): {0: [0, 2, 3, 4, 5, 6, 7, 8, 10, 11, 13], 1: [2, 4, 5, 10, 11, 12], 2: [2, 3, 4, 10, 11, 12]},
    ((3, 70, 3), True): {0: [0, 4, 10, 11, 12], 1: [0, 4, 6, 7, 10, 11, 12], 2: [0, 4, 6, 7, 8]},
    ((3, 3, 70), True): {0: [0, 2, 3, 6, 7, 8], 1: [0, 1, 2, 6, 7, 8], 2: [0, 1, 2, 3, 6, 7, 10, 11]},
}
# diagonal factors (row, index into R L T B F K) and averaged samples (axis, which of the two components, sample) that
# (3,3,3), with two interior faces per component, leaves out
LEFT_OUT_DIAG_333 = [(0, 0), (0, 4), (2, 0), (2, 3)]
LEFT_OUT_BC_333 = [(0, 1, 1), (1, 0, 1), (1, 1, 2)]


def _pairs(by_row):
    return [(a, t) for a in sorted(by_row) for t in by_row[a]]


def _row_ratio(monkeypatch, table, d, scale, mu, rhs, base, mag):
    """worst err / bound per component of the rows evaluated with VISC_ROWS replaced by `table`"""
    with monkeypatch.context() as mp:
        mp.setattr(O, "VISC_ROWS", table)
        alt, _ = G.rows(d, scale, mu, rhs)
    R = G.R_RHS if rhs else G.R_APPLY
    return [G.ratio(alt[a], base[a], mag[a], R, G.U[F64], G.interior(base[a].shape)).max() for a in range(3)]


@pytest.mark.parametrize("rhs", [True, False], ids=["rhs", "apply"])
@pytest.mark.parametrize("gres", G.INTERIOR_GRIDS, ids=G.gid)
def test_every_tap_is_exercised(monkeypatch, gres, rhs):
    d = G.inputs(gres)
    for scale, mu in G.KS:
        base, mag = G.rows(d, scale, mu, rhs)
        left_out = []
        for a in range(3):
            for t in range(14):
                table = copy.deepcopy(O.VISC_ROWS)
                del table[a]["taps"][t]
                if not _row_ratio(monkeypatch, table, d, scale, mu, rhs, base, mag)[a] > 100:
                    left_out.append((a, t))
        assert left_out == _pairs(LEFT_OUT.get((tuple(gres), rhs), {})), (scale, mu)


def test_the_grids_together_leave_out_no_tap():
    for rhs in (True, False):
        out = [set(_pairs(LEFT_OUT.get((tuple(g), rhs), {}))) for g in G.INTERIOR_GRIDS]
        assert not set.intersection(*out)
        assert all(len(O.VISC_ROWS[a]["taps"]) == 14 for a in range(3))


@pytest.mark.parametrize("gres", G.INTERIOR_GRIDS, ids=G.gid)
def test_every_diagonal_factor_is_exercised(monkeypatch, gres):
    d = G.inputs(gres)
    for scale, mu in G.KS:
        base, mag = G.rows(d, scale, mu, False)
        left_out = []
        for a in range(3):
            for t in range(6):
                table = copy.deepcopy(O.VISC_ROWS)
                table[a]["diag"] = tuple(0 if k == t else f for k, f in enumerate(table[a]["diag"]))
                if not _row_ratio(monkeypatch, table, d, scale, mu, False, base, mag)[a] > 100:
                    left_out.append((a, t))
        assert left_out == (LEFT_OUT_DIAG_333 if tuple(gres) == (3, 3, 3) else []), (scale, mu)


@pytest.mark.parametrize("gres", G.INTERIOR_GRIDS, ids=G.gid)
def test_every_averaged_sample_is_exercised(monkeypatch, gres):
    d = G.inputs(gres)
    base, mag = G.boundary_condition(d)
    left_out = []
    for a in range(3):
        for w in range(2):
            for t in range(4):
                table = copy.deepcopy(O.NB_BC_TAPS)
                del table[a][w][1][t]
                with monkeypatch.context() as mp:
                    mp.setattr(O, "NB_BC_TAPS", table)
                    alt, _ = G.boundary_condition(d)
                if not G.ratio(alt[a], base[a], mag[a], G.R_BC, G.U[F64], G.interior(base[a].shape)).max() > 100:
                    left_out.append((a, w, t))
    assert left_out == (LEFT_OUT_BC_333 if tuple(gres) == (3, 3, 3) else [])


@pytest.mark.parametrize("gres", G.INTERIOR_GRIDS, ids=G.gid)
def test_reordered_sums_stay_within_the_bounds(monkeypatch, gres):
    """a correct implementation passes: the oracle with every sum reversed is within the bounds of the GPU tests"""
    d = G.inputs(gres)
    table = copy.deepcopy(O.VISC_ROWS)
    for a in range(3):
        table[a]["taps"] = table[a]["taps"][::-1]
    differs = 0
    for rhs in (True, False):
        for scale, mu in G.KS:
            base, mag = G.rows(d, scale, mu, rhs)
            r = _row_ratio(monkeypatch, table, d, scale, mu, rhs, base, mag)
            assert max(r) <= 1.0, (rhs, scale, mu, r)
            differs += max(r) > 0
    base, mag = G.boundary_condition(d)
    alt, _ = G.boundary_condition(d, reverse=True)
    r = [G.ratio(alt[a], base[a], mag[a], G.R_BC, G.U[F64], G.interior(base[a].shape)).max() for a in range(3)]
    assert max(r) <= 1.0, r
    assert differs and max(r) > 0                # the reordering did change bits: the check is not vacuous


@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_magnitude_outputs_change_no_result(gres):
    """the oracle's results are the same to the bit with and without `mag=` / `valid_out=`"""
    d = G.inputs(gres)
    V = [d["v" + c] for c in "xyz"]
    M = [d["m" + c] for c in "xyz"]
    for rhs in (True, False):
        a, b = ([np.full(G.face_shape(gres, k), 7.0) for k in range(3)] for _ in range(2))
        if rhs:
            O.visc_rhs3d(gres, 0.5, 2.0, *V, d["sphi"], None, d["vol"], *a)
            O.visc_rhs3d(gres, 0.5, 2.0, *V, d["sphi"], None, d["vol"], *b, mag={})
        else:
            O.visc_apply3d(gres, 0.5, 2.0, *V, *a, d["sphi"], d["vol"])
            O.visc_apply3d(gres, 0.5, 2.0, *V, *b, d["sphi"], d["vol"], mag={})
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)
    a, b = ([np.full(G.face_shape(gres, k), 7.0) for k in range(3)] for _ in range(2))
    O.nb_boundary_condition(gres, V, M, d["sphi"], d["sv"], d["dx"], a)
    O.nb_boundary_condition(gres, V, M, d["sphi"], d["sv"], d["dx"], b, mag={})
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    a, b = [v.copy() for v in V], [v.copy() for v in V]
    O.visc_extrapolate3d(gres, 3, *a, d["sphi"])
    O.visc_extrapolate3d(gres, 3, *b, d["sphi"], valid_out=[])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    a, b = [v.copy() for v in V], [v.copy() for v in V]
    O.nb_extrapolate(gres, 3, *a, *M)
    O.nb_extrapolate(gres, 3, *b, *M, valid_out=[])
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def _valid_after(d, form, k):
    v, out = [d["v" + c].copy() for c in "xyz"], []
    if form == "sphi":
        O.visc_extrapolate3d(d["gres"], k, *v, d["sphi"], valid_out=out)
    else:
        O.nb_extrapolate(d["gres"], k, *v, d["mx"], d["my"], d["mz"], valid_out=out)
    return v, out


@pytest.mark.parametrize("form", ["sphi", "mass"])
@pytest.mark.parametrize("gres", G.COVERAGE_GRIDS, ids=G.gid)
def test_extrapolate_inputs_need_every_sweep(gres, form):
    """per component: each of three sweeps fills faces that the sweeps before it did not; interior faces stay unfilled after
    three (with sphi as the validity: in at least one component -- the ellipsoid of (17,19,23) is four faces deep along x
    only)"""
    d = G.inputs(gres)
    valid = [_valid_after(d, form, k)[1] for k in range(4)]
    for a in range(3):
        n = [int(valid[k][a].sum()) for k in range(4)]
        assert n[0] < n[1] < n[2] < n[3], (a, n)
    unfilled = [int((~valid[3][a] & G.interior(valid[3][a].shape)).sum()) for a in range(3)]
    assert max(unfilled) > 0 if form == "sphi" else min(unfilled) > 0, unfilled
    v0, v3 = _valid_after(d, form, 0)[0], _valid_after(d, form, 3)[0]
    for a in range(3):
        np.testing.assert_array_equal(v0[a], d["v" + "xyz"[a]])
        assert (v3[a] != v0[a]).sum() == valid[3][a].sum() - valid[0][a].sum()     # every fill changed the value


@pytest.mark.parametrize("gres", G.COVERAGE_GRIDS, ids=G.gid)
def test_boundary_condition_inputs_hold_every_category(gres):
    d = G.inputs(gres)
    dv, mag = G.boundary_condition(d)
    for a in range(3):
        edge, far, empty, rest = G.bc_categories(d, a)
        assert edge.any() and far.any() and empty.any() and rest.any(), a
        assert (edge ^ far ^ empty ^ rest).all() and (edge | far | empty | rest).all()
        assert (dv[a][edge | far] == 0).all()
        nan = np.isnan(dv[a])
        assert (dv[a][empty & ~nan] == 0).all()
        assert np.count_nonzero(dv[a][rest & ~nan]) > 10                       # both branches of min(0, s)
        assert (dv[a][rest & ~nan] == 0).sum() > 10
        assert nan.any() == (tuple(gres) == G.FLAT_GRID)


@pytest.mark.parametrize("gres", G.GRIDS, ids=G.gid)
def test_generated_fields(gres):
    d = G.inputs(gres)
    assert G.inputs(gres) is d and not d["sphi"].flags.writeable
    vol = d["vol"]
    assert vol.min() == 0.0 and vol.max() == 1.0 and ((vol > 0) & (vol < 1)).any()
    assert (d["sv"] != 0).all()
    for c in "xyz":
        assert (d["v" + c] != 0).all() and (d["out" + c] != 0).all() and (d["m" + c] >= 0).all()
    # the gradient of sphi vanishes on no interior face nearer than dx to the solid, but on the flat patch
    s = d["sphi"]
    flat = 0
    for a in range(3):
        shp = G.face_shape(gres, a)
        if min(shp) < 3:
            continue
        D0 = [0 if k == a else 1 for k in range(3)]
        cnt = [n - 2 for n in shp]
        at = lambda off: s[tuple(slice(2 + D0[k] + off[k], 2 + D0[k] + off[k] + 2 * cnt[k], 2) for k in range(3))]  # noqa: E731
        e = np.eye(3, dtype=int)
        g2 = sum((at(e[k]) - at(-e[k])) ** 2 for k in range(3))
        near = at((0, 0, 0)) / d["dx"] < 1
        if tuple(gres) == G.FLAT_GRID:
            flat += int((near & (g2 == 0)).sum())
            assert (at((0, 0, 0))[near & (g2 == 0)] == -0.75 * d["dx"]).all()
        else:
            assert (g2[near] > 0).all()
    assert (flat > 0) == (tuple(gres) == G.FLAT_GRID)
    if tuple(gres) in G.COVERAGE_GRIDS:
        for a in range(3):
            f = G.face_of_doubled(d["sphi"], a)[G.interior(G.face_shape(gres, a))]
            assert (f < 0).any() and (f >= 0).any() and (f / d["dx"] >= 1).any()
            assert (d["m" + "xyz"[a]] == 0).any() and (d["m" + "xyz"[a]] > 0).any()
