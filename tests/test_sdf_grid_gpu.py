"""`evaluate_grid` of solver.sdf3D / solver.sdf2D on the MI355X: the solid level set and surface velocity on the nodes of a
regular grid, positions made from the index inside the kernel.

Without angular velocities it must be `evaluate` on `grid_positions(...)` bit for bit (same device functions, same
position arithmetic), for float64 and float32 outputs, with every vel element written (vel starts as NaN).  With `rb_w`
the velocity of the winning body is v + w x (pos - T); the winner (first strict minimum of the per-body distance) comes
from the oracle evaluating one body at a time, the formulas are restated here in float64 with one rounding per operation,
and the result must be bit-equal; float32 outputs are the float64 result rounded once.  Points where two bodies' distances
tie to rounding (the kernel's sqrt against the oracle's pow can then pick another winner) are skipped, at most 0.1 % of a
grid; the poses here are chosen so that there are none."""
import numpy as np
import pytest
import torch

from conftest import golden
import density2d_numpy as D2
from oracle import mfs_oracle as O
import notebook_sim as NSIM3
import notebook_sim2d as NSIM2
import solver.sdf2D as S2
import solver.sdf3D as S3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
F32, F64 = np.float32, np.float64

BMIN = {3: (-0.3, 0.013, -0.3), 2: (-0.3, 0.013)}
BIASES = {3: ((0, .5, .5), (0, 0, 0)), 2: ((0, .5), (0, 0))}
# anisotropic cell sizes that spread each grid over the bodies; no node on a symmetry plane of the notebook's ramps
GRIDS = {3: {(11, 15, 7): (0.057, 0.061, 0.083), (3, 3, 3): (0.21, 0.33, 0.23), (1, 1, 300): (0.05, 0.07, 0.0021)},
         2: {(11, 15): (0.1, 0.07), (81, 7): (0.013, 0.15), (1, 1): (0.05, 0.07)}}
MOD = {3: (S3, NSIM3), 2: (S2, NSIM2)}
TIE = 1e-12


def _with_velocities(rb_d):
    """the goldens' bodies mostly rest: give every body its own velocity, so that a wrong winner shows in vel"""
    rb = np.array(rb_d, F64)
    D = 3 if rb.shape[1] == 10 else 2
    for i in range(len(rb)):
        if not rb[i, -1, :D].any():
            rb[i, -1, :D] = np.array([0.11, -0.07, 0.05])[:D] * (i + 1)
    return rb


def bodies(name):
    if name == "empty3":
        return np.zeros((0, 10, 4))
    if name == "empty2":
        return np.zeros((0, 8, 3))
    if name == "extra3":            # a rotated flipped box and a tilted cylinder inside it
        rb_d, m = S3.generate_rb(None, {}, "tank", ['box', 0.52, 0.7, 0.47], flip=True, center=[0.01, 0.45, -0.02], axis=[1, 1, 0],
                                 angle=30, device="cpu")
        rb_d, m = S3.generate_rb(rb_d, m, "can", ['cylinder', 0.09, 0.31], center=[0.03, 0.4, 0.02], axis=[1, 0, 1], angle=35)
        return _with_velocities(rb_d.numpy())
    if name == "extra2":            # a rotated flipped box and a disc inside it
        rb_d, m = S2.generate_rb(None, {}, "tank", ['box', 0.8, 0.7], flip=True, center=[0.21, 0.52], angle=30, device="cpu")
        rb_d, m = S2.generate_rb(rb_d, m, "disc", ['sphere', 0.12], center=[0.17, 0.43])
        return _with_velocities(rb_d.numpy())
    return _with_velocities(golden(name)["rb_d"])


SETS = {3: ("sdf_b_spheres", "sdf_c_notebook_f32", "extra3", "empty3"), 2: ("sdf2d_a_f64", "extra2", "empty2")}
CASES = [(D, name, res) for D in (3, 2) for name in SETS[D] for res in GRIDS[D]]


def positions(D, res, bias):
    """get_grid_pos in numpy: bound_min(f32) + (f32 index + f32 bias) * cell_size, float64"""
    idx = np.stack(np.meshgrid(*[np.arange(r, dtype=F32) for r in res], indexing="ij"), axis=-1)
    return np.asarray(BMIN[D], F32).astype(F64) + (idx + np.asarray(bias, F32)).astype(F64) * np.asarray(GRIDS[D][res], F64)


def per_body_sd(D, rb, pos):
    """(n, points): the oracle on one body at a time"""
    P = pos.reshape(-1, D)
    out = np.zeros((len(rb), len(P)))
    for i in range(len(rb)):
        if D == 3:
            O.sdf_evaluate(rb[i:i + 1], out[i], np.zeros((len(P), 3)), P)
        else:
            out[i] = D2.sdf_evaluate(rb[i:i + 1], P)[0]
    return out


def restated(D, rb, rb_w, pos, inside):
    """winner, skipped points and vel = v + w x (pos - T) at the `inside` points, 0 elsewhere; one rounding per operation"""
    P = pos.reshape(-1, D)
    vel = np.zeros((len(P), D))
    if len(rb) == 0:
        return vel, np.zeros(len(P), bool), np.full(len(P), 100.0)
    sds = per_body_sd(D, rb, P)
    win = np.zeros(len(P), np.int64)
    best = np.full(len(P), 100.0)
    for i in range(len(rb)):                                  # first strict minimum, start value 100
        closer = sds[i] < best
        best, win = np.where(closer, sds[i], best), np.where(closer, i, win)
    others = np.where(np.arange(len(rb))[:, None] == win[None, :], np.inf, sds)
    skipped = np.abs(others - best[None, :]).min(axis=0) <= TIE if len(rb) > 1 else np.zeros(len(P), bool)
    v, w = rb[win, -1, :D], rb_w[win]
    r = [P[:, k] - rb[win, 1 + k, D] for k in range(D)]
    if D == 3:
        full = [v[:, 0] + (w[:, 1] * r[2] - w[:, 2] * r[1]), v[:, 1] + (w[:, 2] * r[0] - w[:, 0] * r[2]),
                v[:, 2] + (w[:, 0] * r[1] - w[:, 1] * r[0])]
    else:
        full = [v[:, 0] - w * r[1], v[:, 1] + w * r[0]]
    for k in range(D):
        vel[:, k] = np.where(inside, full[k], 0.0)
    return vel, skipped, best


def run_grid(D, rb, res, bias, dtype, rb_w=None):
    S = MOD[D][0]
    sd = torch.full(res, float("nan"), dtype=dtype, device=DEV)
    vel = torch.full(res + (D,), float("nan"), dtype=dtype, device=DEV)
    S.evaluate_grid(T(rb), sd, vel, BMIN[D], GRIDS[D][res], bias, rb_w=None if rb_w is None else T(rb_w))
    return N(sd), N(vel)


@pytest.mark.parametrize("D,name,res", CASES)
def test_without_rotation_it_is_evaluate_on_grid_positions(D, name, res):
    S, NSIM = MOD[D]
    rb = bodies(name)
    for bias in BIASES[D]:
        pos = NSIM.grid_positions(res, BMIN[D], GRIDS[D][res], bias, DEV)
        np.testing.assert_array_equal(N(pos), positions(D, res, bias))
        for dtype in (torch.float64, torch.float32):
            sd0 = torch.zeros(res, dtype=dtype, device=DEV)
            vel0 = torch.zeros(res + (D,), dtype=dtype, device=DEV)
            S.evaluate(T(rb), sd0, vel0, pos)
            sd, vel = run_grid(D, rb, res, bias, dtype)
            assert not np.isnan(vel).any() and not np.isnan(sd).any()          # every element written
            np.testing.assert_array_equal(sd, N(sd0))
            np.testing.assert_array_equal(vel, N(vel0))
            if len(rb) == 0:
                assert (sd == 100).all() and (vel == 0).all()
            # all-zero angular velocities: row 9 of the winner again (v + (0 - 0); no body velocity here is -0.0)
            _, velz = run_grid(D, rb, res, bias, dtype, rb_w=np.zeros((len(rb), 3) if D == 3 else (len(rb),)))
            np.testing.assert_array_equal(velz, vel)


@pytest.mark.parametrize("D,name,res", CASES)
def test_angular_velocity_against_the_restatement(D, name, res):
    rb = bodies(name)
    rng = np.random.default_rng(len(name) + sum(res))
    rb_w = rng.uniform(-3.0, 3.0, size=(len(rb), 3) if D == 3 else (len(rb),))
    bias = BIASES[D][0]
    pos = positions(D, res, bias)
    sd, vel = run_grid(D, rb, res, bias, torch.float64, rb_w=rb_w)
    want, skipped, best = restated(D, rb, rb_w, pos, sd.reshape(-1) <= 0)
    assert skipped.mean() <= 1e-3, f"{skipped.sum()} of {skipped.size} points tie: choose other poses"
    keep = ~skipped
    np.testing.assert_allclose(sd.reshape(-1)[keep], best[keep], rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(vel.reshape(-1, D)[keep], want[keep])
    if len(rb):
        inside = (sd.reshape(-1) <= 0) & keep
        assert inside.any() and (want[keep] != 0).any(), "no node inside a body: the case would not exercise the rotation term"
    sd32, vel32 = run_grid(D, rb, res, bias, torch.float32, rb_w=rb_w)
    np.testing.assert_array_equal(sd32, sd.astype(F32))                        # the float64 result rounded once
    np.testing.assert_array_equal(vel32, vel.astype(F32))


def test_misuse():
    rb = T(bodies("extra3"))
    sd = torch.zeros((3, 4, 5), dtype=torch.float64, device=DEV)
    vel = torch.zeros((3, 4, 5, 3), dtype=torch.float64, device=DEV)
    args = (BMIN[3], (0.1, 0.1, 0.1), (0, 0, 0))
    with pytest.raises(ValueError, match="sd / vel"):
        S3.evaluate_grid(rb, sd, vel[..., :2].contiguous(), *args)
    with pytest.raises(ValueError, match="rb_w"):
        S3.evaluate_grid(rb, sd, vel, *args, rb_w=torch.zeros((3, 3), dtype=torch.float64, device=DEV))
    with pytest.raises(TypeError, match="rb_w"):
        S3.evaluate_grid(rb, sd, vel, *args, rb_w=torch.zeros((2, 3), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError, match="rb_d"):
        S2.evaluate_grid(rb, sd[0], vel[0, ..., :2].contiguous(), BMIN[2], (0.1, 0.1), (0, 0))
    empty = torch.zeros((0, 4), dtype=torch.float64, device=DEV)                # zero sizes: nothing to do
    S2.evaluate_grid(T(bodies("extra2")), empty, torch.zeros((0, 4, 2), dtype=torch.float64, device=DEV), BMIN[2], (0.1, 0.1), (0, 0))
