"""The three kernels of csrc/mfs_sdf.hip (k_sdf_evaluate, k_sdf_evaluate_grid, k_sdf_project) on the MI355X on every branch,
cylinders included, through solver.sdf3D (the C ABI directly only for its edges): the designed inputs of
tests/sdf3d_inputs.py against oracle/mfs_oracle.py, and the cylinder scenes against the executed reference
(tests/golden/sdfcyl_*.npz).  tests/test_sdf3d_inputs.py shows on the CPU that those inputs take both sides of every
comparison and that each planted mistake is caught by the comparisons made here.

Generic points (rotated bodies of all six type codes and a row of the mesh code in every position, no compared quantity
within 1e-6 of its threshold) hold |got - want| <= (R + 2) 2^-53 M + u_out |want|; the velocities are the winner's, bit for
bit.  Exact points (dyadic bodies and points on faces, edges, corners, surfaces, caps, rims, axes and ties) are bit-equal,
the sign of a zero included, NaN matching NaN.  float32 positions in `project` equal the oracle's per-body rounding; a point
may be one float32 ulp off, at no more than 1 % of the points.  Every output lies in a padded buffer and holds more entries
than the call is given: those and the padding keep their values.

Measured on the MI355X, worst err / bound (the RATIO, SLACK and GOLDEN lines that the tests print):
  evaluate into float64 0.0631, into float32 0.9809 (the rounding of the store alone reaches u_out |want|)
  evaluate_grid into float64 0.0000, into float32 0.8304          project float64 0.0000 (bit for bit)
  project float32: no point differs from the oracle's per-body rounding
  cylinder goldens: sd within 2.8e-17, float64 projection within 5.6e-17, float32 projection 0 ulp, vel exact."""
import functools
import itertools

import numpy as np
import pytest
import torch

import sdf3d_inputs as I
from conftest import golden, golden_names
from mfs import _lib, tensors as TT
import notebook_sim as NSIM3
import solver.sdf3D as S
import test_sdf_grid_gpu as G
from test_grid_kernels3d_gpu import DEV, N, TD, Padded, T, refused

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]
SENT, EXTRA = 7.5, 37                 # what the entries beyond the point count hold, and how many there are
WORST = {}
RB = lambda rb: T(np.array(rb, F64))  # noqa: E731  (the tables are read-only arrays)


def _note(key, r):
    w = float(np.max(r)) if np.size(r) else 0.0
    WORST[key] = max(WORST.get(key, 0.0), w)
    print(f"RATIO {key}: worst err / bound {w:.4f} (so far {WORST[key]:.4f})")
    return w


@functools.lru_cache(maxsize=None)
def want_evaluate(scene, pdt):
    rb, pts = _scene(scene)
    return I.evaluate(rb, pts, pdt)


@functools.lru_cache(maxsize=None)
def want_project(scene, pdt):
    rb, pts = _scene(scene)
    return I.project(rb, pts, pdt)


def _scene(scene):
    if scene in I.GENERIC_TABLES:
        return I.GENERIC_TABLES[scene], I.generic_points()
    if scene == "chain":
        return I.CHAIN, I.chain_points()
    return I.EXACT_SCENES[scene][:2]


def _same_bits(got, want, what):
    bad = I.bit_mismatches(got, want)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {np.argwhere(bad)[0]}: {got[bad][:3]} for {want[bad][:3]}"


def run_evaluate(rb, pts, n, pdt, sdt, vdt):
    """evaluate on the first n points; returns (sd, vel) of all n + EXTRA entries of the buffers"""
    sd, vel = Padded((n + EXTRA,), TD[sdt], SENT), Padded((n + EXTRA, 3), TD[vdt], SENT)
    S.evaluate(RB(rb), sd.t[:n], vel.t[:n], T(pts[:n].astype(pdt)))
    return sd.np(), vel.np()


# ----------------------------------------------------------------------------------------------------- evaluate ---
@pytest.mark.parametrize("pdt,sdt,vdt", list(itertools.product(DTYPES, DTYPES, DTYPES)),
                         ids=lambda d: "32" if d is F32 else "64")
def test_evaluate(pdt, sdt, vdt):
    for k, n in enumerate(I.COUNTS):
        scene = list(I.GENERIC_TABLES)[k % 3]
        rb, pts = _scene(scene)
        wsd, wvel, M = want_evaluate(scene, pdt)
        sd, vel = run_evaluate(rb, pts, n, pdt, sdt, vdt)
        what = f"evaluate generic, mesh row {scene}, {n} points, p{pdt.__name__} sd{sdt.__name__} vel{vdt.__name__}"
        assert sd.dtype == sdt and vel.dtype == vdt
        assert (sd[n:] == SENT).all() and (vel[n:] == SENT).all(), what + ": wrote beyond the point count"
        r = I.excess(sd[:n], wsd[:n], M[:n], I.r_evaluate(rb), sdt)
        assert _note(f"evaluate -> {sdt.__name__}", r) <= 1.0, f"{what}: {int((r > 1).sum())} points over, first {int(r.argmax())}"
        _same_bits(vel[:n], wvel[:n].astype(vdt), what + " vel")
        assert (vel[:n][sd[:n] > 0] == 0).all(), what
    for scene, (rb, pts, names) in I.EXACT_SCENES.items():
        wsd, wvel, _ = want_evaluate(scene, pdt)
        sd, vel = run_evaluate(rb, pts, len(pts), pdt, sdt, vdt)
        what = f"evaluate exact {scene}, p{pdt.__name__} sd{sdt.__name__} vel{vdt.__name__}"
        assert (sd[len(pts):] == SENT).all() and (vel[len(pts):] == SENT).all(), what
        _same_bits(sd[:len(pts)], wsd.astype(sdt), what + " sd")
        _same_bits(vel[:len(pts)], wvel.astype(vdt), what + " vel")
        assert (vel[:len(pts)][sd[:len(pts)] > 0] == 0).all(), what


# ------------------------------------------------------------------------------------------------------ project ---
def run_project(rb, pts, n, pdt):
    pos = Padded((n + EXTRA, 3), TD[pdt], SENT)
    pos.t[:n].copy_(T(pts[:n].astype(pdt)))
    S.project(RB(rb), pos.t[:n])
    out = pos.np()
    assert (out[n:] == SENT).all(), "project wrote beyond the point count"
    return out[:n]


@pytest.mark.parametrize("pdt", DTYPES, ids=["p32", "p64"])
def test_project(pdt):
    cases = [(list(I.GENERIC_TABLES)[k % 3], n) for k, n in enumerate(I.COUNTS)] + [("chain", I.N_CHAIN)]
    for scene, n in cases:
        rb, pts = _scene(scene)
        want, M = want_project(scene, pdt)
        got = run_project(rb, pts, n, pdt)
        what = f"project {scene}, {n} points, p{pdt.__name__}"
        assert got.dtype == pdt and (n < 255 or (np.abs(got.astype(F64) - pts[:n]).max(axis=1) > 1e-3).sum() > 20), what
        if pdt is F64:
            r = I.excess(got, want[:n], M[:n], I.r_project(rb))
            assert _note("project float64", r) <= 1.0, f"{what}: {int((r > 1).sum())} elements over"
        else:
            over, slack = I.f32_verdict(got, want[:n])
            print(f"SLACK {what}: {over} points more than one float32 ulp off, {slack:.3%} of the points differ")
            assert over == 0, what
            assert slack <= I.F32_SLACK_SHARE, what
    for scene, (rb, pts, names) in I.EXACT_SCENES.items():
        want, _ = want_project(scene, pdt)
        got = run_project(rb, pts, len(pts), pdt)
        _same_bits(got, want, f"project exact {scene}, p{pdt.__name__}")
        nan = [nm for nm, row in zip(names, got) if np.isnan(row).any()]
        assert nan == I.NAN_POINTS.get(scene, []), nan


# ------------------------------------------------------------------------------------------------ evaluate_grid ---
def run_grid(rb, bias, dtype, rb_w=None, grid=I.GRID):
    res = grid["res"]
    sd, vel = Padded(res, TD[dtype], np.nan), Padded(res + (3,), TD[dtype], np.nan)
    S.evaluate_grid(RB(rb), sd.t, vel.t, grid["bound_min"], grid["cell_size"], bias, rb_w=None if rb_w is None else T(rb_w))
    return sd.np(), vel.np()


@pytest.mark.parametrize("dtype", DTYPES, ids=["o32", "o64"])
def test_evaluate_grid_on_exact_nodes(dtype):
    rb = I.EXACT_SCENES["solids"][0]
    rng = np.random.default_rng(9)
    rb_w = np.round(rng.uniform(-3, 3, size=(len(rb), 3)) * 64) / 64
    for bias in I.GRID["biases"]:
        nodes = I.grid_nodes(bias)
        pos = NSIM3.grid_positions(I.GRID["res"], I.GRID["bound_min"], I.GRID["cell_size"], bias, DEV)
        _same_bits(N(pos), nodes, "grid positions")
        P = nodes.reshape(-1, 3)
        wsd, wvel, M = I.evaluate(rb, P)
        sd, vel = run_grid(rb, bias, dtype)
        what = f"evaluate_grid bias {bias} -> {dtype.__name__}"
        assert not np.isnan(sd).any() and not np.isnan(vel).any(), what + ": an element was not written"
        # against evaluate on the stored positions: the same device functions, bit for bit
        sd0, vel0 = torch.zeros(I.GRID["res"], dtype=TD[dtype], device=DEV), torch.zeros(I.GRID["res"] + (3,), dtype=TD[dtype], device=DEV)
        S.evaluate(RB(rb), sd0, vel0, pos)
        _same_bits(sd, N(sd0), what + " against evaluate, sd")
        _same_bits(vel, N(vel0), what + " against evaluate, vel")
        # against the oracle: within the bound everywhere, and bit for bit where every intermediate is exact (inside or on
        # the box, and along the x axis through the box and the sphere's centre)
        r = I.excess(sd.reshape(-1), wsd, M, I.r_evaluate(rb), dtype)
        assert _note(f"evaluate_grid -> {dtype.__name__}", r) <= 1.0, what
        exact = ((np.abs(P[:, 0]) <= 0.5) & (np.abs(P[:, 1]) <= 0.25) & (np.abs(P[:, 2]) <= 0.125)) | ((P[:, 1] == 0) & (P[:, 2] == 0))
        assert exact.sum() >= 20
        _same_bits(sd.reshape(-1)[exact], wsd[exact].astype(dtype), what + " exact nodes, sd")
        _same_bits(vel.reshape(-1, 3), wvel.astype(dtype), what + " vel")
        # with angular velocities: the restatement of test_sdf_grid_gpu.py, v + w x (pos - T) of the winning body
        sdw, velw = run_grid(rb, bias, dtype, rb_w=rb_w)
        want, skipped, best = G.restated(3, np.asarray(rb), rb_w, nodes, wsd <= 0)
        _same_bits(sdw, sd, what + " rb_w changes no distance")
        keep = ~skipped                                              # the coincident and the touching bodies tie: never the
        assert skipped.mean() <= 0.05 and keep[exact].all()          # winner at a node of this grid
        _same_bits(velw.reshape(-1, 3)[keep], want[keep].astype(dtype), what + " with rb_w, vel")
        assert (want[keep] != wvel[keep]).any() and (want[wsd > 0] == 0).all()


def test_evaluate_grid_leaves_the_unknown_row_alone():
    grid = dict(res=(9, 11, 7), bound_min=(-0.8, -0.2, -0.8), cell_size=(0.19, 0.13, 0.23))
    rb_w = np.random.default_rng(4).uniform(-3, 3, size=(7, 3))
    for bias in ((0, 0.5, 0.5), (0, 0, 0)):
        pos = NSIM3.grid_positions(grid["res"], grid["bound_min"], grid["cell_size"], bias, DEV)
        P = N(pos).reshape(-1, 3)
        wsd, wvel, M = I.evaluate(I.GENERIC_KNOWN, P)
        for where, rb in I.GENERIC_TABLES.items():
            sd, vel = run_grid(rb, bias, F64, grid=grid)
            r = I.excess(sd.reshape(-1), wsd, M, I.r_evaluate(rb))
            assert _note("evaluate_grid -> float64", r) <= 1.0, where
            clear = np.abs(wsd) > I.MARGIN                          # nodes are not filtered: a sign within the margin may differ
            _same_bits(vel.reshape(-1, 3)[clear], wvel[clear], f"evaluate_grid, mesh row {where}, vel")
            at = int(np.flatnonzero(rb[:, 0, 0] == I.MESH_CODE)[0])
            w = np.insert(rb_w[:6], at, [50.0, 60.0, 70.0], axis=0)     # the unknown row's angular velocity is never read either
            _, velw = run_grid(rb, bias, F64, rb_w=w, grid=grid)
            _, velk = run_grid(I.GENERIC_KNOWN, bias, F64, rb_w=rb_w[:6], grid=grid)
            _same_bits(velw, velk, f"evaluate_grid with rb_w, mesh row {where}")


# --------------------------------------------------------------------------------------------- cylinder goldens ---
@pytest.mark.parametrize("name", golden_names("sdfcyl_"))
def test_cylinders_against_the_executed_reference(name):
    g = golden(name)
    rb, pos = g["rb_d"], g["position_eval"]
    sd, vel = run_evaluate(rb, pos, len(pos), F64, F64, F64)
    np.testing.assert_allclose(sd[:len(pos)], g["sd"], rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(vel[:len(pos)], g["vel"])
    print(f"GOLDEN {name}: evaluate worst |sd - golden| {np.abs(sd[:len(pos)] - g['sd']).max():.3g}")
    got = run_project(rb, g["position_project"], len(g["position_project"]), F64)
    print(f"GOLDEN {name}: project float64 worst difference {np.abs(got - g['projected']).max():.3g}")
    np.testing.assert_allclose(got, g["projected"], rtol=0, atol=1e-15)
    got32 = run_project(rb, g["position_project_f32"], len(g["position_project_f32"]), F32)
    assert got32.dtype == np.float32 and g["projected_f32"].dtype == np.float32
    ulps = np.abs(got32.astype(F64) - g["projected_f32"].astype(F64)) / np.spacing(np.abs(g["projected_f32"])).astype(F64)
    print(f"GOLDEN {name}: project float32 worst difference {ulps.max():.3g} ulp, {(ulps > 0).any(axis=1).mean():.3%} of the points differ")
    assert (ulps <= 1).all()


# ------------------------------------------------------------------------------------------------- C ABI edges ---
def test_4096_bodies_are_accepted_and_4097_refused():
    """far-away spheres and one near box at the last index: the winner index is the largest possible"""
    lib, s, ok = _lib.load(), TT.stream(), _lib.MFS_F64
    rows = [I.body(I.SPHERE, (0.5,), (1000.0 + 2 * k, 0, 0), vel=(1.0, k, -1.0)) for k in range(4095)]
    rb = I.table(*rows, I.body(I.BOX, (1.0, 0.5, 0.25), (0, 0, 0), vel=I.V[0]))
    pts = np.array([(0.25, 0.0625, 0), (0.5, 0.1, 0), (3, 0, 0), (0, 0, 0), (1000.25, 0, 0)], F64)
    wsd, wvel, _ = I.evaluate(rb, pts)
    assert (wvel[:2] == I.V[0]).all() and (wvel[3] == I.V[0]).all() and not wvel[2].any() and (wvel[4] == (1.0, 0, -1.0)).all()
    sd, vel = run_evaluate(rb, pts, len(pts), F64, F64, F64)
    _same_bits(sd[:5], wsd, "4096 bodies, sd")
    _same_bits(vel[:5], wvel, "4096 bodies, vel")
    _same_bits(run_project(rb, pts, 5, F64), I.project(rb, pts)[0], "4096 bodies, project")
    grid = dict(res=(2, 2, 2), bound_min=(0, 0, 0), cell_size=(0.25, 0.125, 0.0625))
    gsd, gvel = run_grid(rb, (0, 0, 0), F64, grid=grid)
    assert (gsd <= 0).all() and (gvel == I.V[0]).all()
    # one more row: refused before any launch, nothing written
    big = T(np.concatenate([rb, rb[:1]]))
    assert big.shape[0] == 4097
    sdp, velp, pos = Padded((5,), torch.float64), Padded((5, 3), torch.float64), Padded((5, 3), torch.float64, pts)
    refused(lib.mfs_sdf_evaluate3d(TT.ptr(big), 4097, pos.ptr, ok, 5, sdp.ptr, ok, velp.ptr, ok, s), "rigid bodies")
    refused(lib.mfs_sdf_project3d(TT.ptr(big), 4097, pos.ptr, ok, 5, s), "rigid bodies")
    gs, gv = Padded((2, 2, 2), torch.float64), Padded((2, 2, 2, 3), torch.float64)
    refused(lib.mfs_sdf_evaluate_grid3d(TT.ptr(big), 4097, None, _lib.i64x(grid["res"]), _lib.f64x(grid["bound_min"]),
                                        _lib.f64x((0, 0, 0)), _lib.f64x(grid["cell_size"]), gs.ptr, ok, gv.ptr, ok, s), "rigid bodies")
    for p in (sdp, velp, gs, gv):
        assert (p.np() == 7.5).all()
    assert (pos.np() == pts).all()
    with pytest.raises(_lib.MfsError, match="rigid bodies"):
        S.project(big, pos.t)


def test_no_positions_with_null_arrays_is_ok():
    lib, s, ok = _lib.load(), TT.stream(), _lib.MFS_F64
    rb = RB(I.GENERIC_KNOWN)
    for code in (ok, _lib.MFS_F32):
        assert lib.mfs_sdf_evaluate3d(TT.ptr(rb), 6, None, code, 0, None, code, None, code, s) == _lib.MFS_OK
        assert lib.mfs_sdf_project3d(TT.ptr(rb), 6, None, code, 0, s) == _lib.MFS_OK
    assert lib.mfs_sdf_evaluate3d(None, 0, None, ok, 0, None, ok, None, ok, s) == _lib.MFS_OK
    assert lib.mfs_sdf_project3d(None, 0, None, ok, 0, s) == _lib.MFS_OK
    refused(lib.mfs_sdf_evaluate3d(TT.ptr(rb), 6, None, ok, 1, None, ok, None, ok, s), "position / output arrays")
    refused(lib.mfs_sdf_project3d(TT.ptr(rb), 6, None, ok, 1, s), "position array")
    refused(lib.mfs_sdf_evaluate3d(None, 1, None, ok, 0, None, ok, None, ok, s), "rigid bodies")
    torch.cuda.synchronize()
