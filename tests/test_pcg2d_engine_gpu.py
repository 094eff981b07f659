"""mfs.pcg.Pcg2dEngine, the Python owner of the `mfs_pcg2d` handle, on its own: argument checks, the agreement of its
two polls and its history after a solve, and its stencil launch in both operator modes, bit for bit against the stateless
module functions (the engine and they instantiate one kernel template, csrc/mfs_apply2d.h).  Grids: 9x7 (odd, not a
multiple of anything) and 3x3, the smallest with an interior cell."""
import numpy as np
import pytest
import torch

from mfs import scenes
from mfs.pcg import Pcg2dEngine
import solver.DensityCGSolver2D as D
import solver.PressureCGSolver2D as P
from solver.SolidFraction2D import compute_solid_frac

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
GRIDS = [(9, 7), (3, 3)]


def T(a, dt=None):
    t = torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    return t if dt is None else t.to(dt)


def scene(gres, dt):
    """pressure_scene_2d on the device, with its face fractions and the pressure right-hand side in `dt`"""
    sc = scenes.pressure_scene_2d(gres, seed=5, solid_velocity=True)
    Nx, Ny = gres
    sphi, sv, lphi = T(sc["sphi"]), T(sc["sv"]), T(sc["lphi"])
    wx, wy = torch.zeros((Nx + 1, Ny), dtype=dt, device=DEV), torch.zeros((Nx, Ny + 1), dtype=dt, device=DEV)
    compute_solid_frac(gres, sphi, wx, wy)
    b = torch.zeros(gres, dtype=dt, device=DEV)
    P.initialize_solver(sc["cell_size"], gres, T(sc["vx"], dt), T(sc["vy"], dt), sphi, sv, lphi, b, wx, wy)
    assert bool((lphi[1:-1, 1:-1] < 0).any())            # there is an equation to solve
    return lphi, wx, wy, b


def test_rank_is_checked():
    with pytest.raises(ValueError):
        Pcg2dEngine((4, 4, 4), F64, DEV)


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("gres", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_bind_solve_poll_history(gres, dt):
    lphi, wx, wy, b = scene(gres, dt)
    eng = Pcg2dEngine(gres, dt, DEV)
    x, d, r, q = (torch.zeros(gres, dtype=dt, device=DEV) for _ in range(4))
    other = F32 if dt == F64 else F64
    with pytest.raises(TypeError):
        eng.bind(b, x.to(other), d, r, q)
    eng.setup(lphi, wx, wy)
    eng.bind(b, x, d, r, q)
    converged, iters = eng.solve(1e-6, gres[0] * gres[1], 4)
    p, raw = eng.poll(), eng.poll_raw()
    assert p["iterations"] == raw["iterations"] == iters
    assert p["done"] == raw["done"] == converged and raw["err"] == 0
    assert converged and iters >= 1
    assert p["delta"] == raw["delta"]
    assert len(eng.history()) == 2 * iters + 1
    assert eng.history_truncated() is False


@pytest.mark.parametrize("dt", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("gres", GRIDS, ids=lambda g: "x".join(map(str, g)))
def test_apply_is_the_module_functions_kernel(gres, dt):
    lphi, wx, wy, _ = scene(gres, dt)
    eng = Pcg2dEngine(gres, dt, DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    v = torch.randn(gres, generator=gen, device=DEV, dtype=F64).to(dt)
    for setup, matvecmul in ((eng.setup_density, D.matvecmul), (eng.setup, P.matvecmul)):
        out, ref = (torch.full(gres, 7.0, dtype=dt, device=DEV) for _ in range(2))
        setup(lphi, wx, wy)
        eng.apply(v, out)
        matvecmul(gres, v, ref, wx, wy, lphi)
        assert bool((ref[1:-1, 1:-1] != 7.0).all())
        assert torch.equal(out[1:-1, 1:-1], ref[1:-1, 1:-1])
    with pytest.raises(TypeError):
        eng.apply(v.to(F32 if dt == F64 else F64), out)
