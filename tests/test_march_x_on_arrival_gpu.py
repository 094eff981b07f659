"""The deferred solution update inside the fused stencil march (csrc/mfs_pcg_apply.h, XDEF): each x vector is updated by
the run that owns its plane, when the d_old it needs arrives as half of the march's own operand -- the prologue for the
run's first two planes, step x for plane x+2.  The loop with the update deferred against the loop with the update in the
vector phase, bit for bit: x, d, r, q, the history and the iteration count; and, for what both loops share, the march's
stand-alone apply against the direct-load kernel.

What can go wrong is ownership (a plane updated twice or not at all where runs of 1, 2 or 3 planes meet, where `xchunk`,
a segment boundary or a work list cuts a run) and the carried z-edge weight (lane 63 of a wave that is not a row end).
A march has at least 256 workgroups to spread its (tile, plane) pairs over, so runs longer than one plane need more than
256 pairs: the "long" shapes below have 370 to 650 (thin in x, long in y, a grid edge being at most 4096; up to a million
cells), the others have a handful and exercise the one-plane run only."""
import numpy as np
import pytest
import torch

from mfs import _lib
from mfs.pcg import PcgEngine

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS = 12


def _problem(gres, seed, ball=None):
    """liquid below y = 0.7 Ny (or a ball: (centre, radius)), face weights 1 with one in ten drawn from {0, 1/4 .. 1}, a
    random right-hand side and a random warm-start vector on the liquid's interior cells"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ax = [torch.arange(n, device=DEV, dtype=torch.float64) + 0.5 for n in gres]
    X, Y, Z = torch.meshgrid(*ax, indexing="ij")
    if ball is None:
        lphi = Y - 0.7 * gres[1] + 0.25 * torch.sin(0.37 * Z + 1.3 * X)
    else:
        c, rad = ball
        lphi = torch.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - rad

    def w(shape):
        q = torch.randint(0, 5, shape, generator=g, device=DEV).double() * 0.25
        one = torch.ones(shape, dtype=torch.float64, device=DEV)
        return torch.where(torch.rand(shape, generator=g, device=DEV) < 0.9, one, q)

    wx, wy, wz = w((gres[0] + 1, gres[1], gres[2])), w((gres[0], gres[1] + 1, gres[2])), w((gres[0], gres[1], gres[2] + 1))
    inside = (lphi < 0).double()
    for a in range(3):
        idx = [slice(None)] * 3
        for e in (0, -1):
            idx[a] = e
            inside[tuple(idx)] = 0
    b = torch.randn(gres, generator=g, device=DEV, dtype=torch.float64) * inside
    x0 = torch.randn(gres, generator=g, device=DEV, dtype=torch.float64) * inside
    return dict(lphi=lphi, wx=wx, wy=wy, wz=wz, b=b, x0=x0)


def _engine(gres, dt, pb, defer, lists, xchunk=0, bpc=2, lean=None, density=False, jacobi=False, warm=False):
    eng = PcgEngine(gres, dt, DEV)
    ops = [pb[k].to(dt) for k in ("lphi", "wx", "wy", "wz")]
    (eng.setup_density if density else eng.setup)(*ops)
    eng.set_resident(False)
    eng.set_sparse(lists)
    eng.set_defer_x(defer)
    if lean is not None:
        eng.set_lean(lean)
    if jacobi:
        eng.set_jacobi(True)
    eng.tune(2, xchunk, bpc, -1)
    b = pb["b"].to(dt)
    x = pb["x0"].to(dt) if warm else torch.zeros(gres, dtype=dt, device=DEV)
    d, r, q = (torch.zeros(gres, dtype=dt, device=DEV) for _ in range(3))
    eng.bind(b, x, d, r, q)
    info = eng.loop_info()
    assert bool(info["deferred_x_update"]) == defer and info["fused_direction_update"] and not info["resident"], info
    return eng, dict(x=x, d=d, r=r, q=q)


def _iterate(gres, dt, pb, defer, lists, poll_after=0, **kw):
    eng, v = _engine(gres, dt, pb, defer, lists, **kw)
    eng.begin(0.0)
    if poll_after:                  # the lane-mask decision of a listed solve reaches the launches with a poll
        eng.iterate(poll_after)
        eng.poll()
    eng.iterate(ITERS - poll_after)
    eng.finish()
    torch.cuda.synchronize()
    assert eng.poll()["iterations"] == ITERS
    v["hist"] = eng.history()[: 2 * ITERS + 1]
    v["lane"] = float(eng.scalars[_lib.S_LANE])
    v["listed"] = eng.sparse_info()["listed_pairs"]
    return v


def _assert_same(a, b, what):
    np.testing.assert_array_equal(a["hist"], b["hist"], err_msg=str(what))
    for k in ("x", "d", "r", "q"):
        assert torch.equal(a[k], b[k]), (k, what)


# (xchunk, blocks_per_cu, lean): runs capped at 1 / 2 / 3 planes; one workgroup per CU (the longest segments a grid allows),
# the default two, and 64 (segments of one pair); the iteration closed by the next stencil launch (BOOK) or by the update's tail
KNOBS = [(0, 1, None), (1, 1, True), (2, 1, False), (3, 1, None), (0, 2, True), (3, 2, False), (0, 64, None), (2, 64, True)]

# Nz: rows of 6, 10 and 34 vectors (lane 63 of a wave is no row end: the carried edge weight is used) and 1028 (more than 256
# halo vectors: the slow halo path); fp64 adds 68 (34 vectors a row, as 136 in fp32) for the long shapes.  Every shape has a
# partial last tile.  Nx = 3 .. 6: 1 .. 4 interior planes.
SHAPES_F32 = [(3, 70, 24), (4, 45, 40), (5, 14, 136), (6, 70, 24), (5, 5, 1028),
              (6, 4000, 24), (5, 4000, 40), (4, 2410, 136), (6, 1220, 136), (5, 216, 1028)]
SHAPES_F64 = [(3, 70, 12), (4, 45, 20), (5, 45, 20), (6, 70, 12), (5, 5, 1028),
              (6, 4000, 12), (5, 4000, 20), (4, 2410, 68), (6, 1220, 68), (5, 109, 1028)]
CASES = [(torch.float32, s) for s in SHAPES_F32] + [(torch.float64, s) for s in SHAPES_F64]


@pytest.mark.parametrize("dt,gres", CASES, ids=[f"{'f32' if d == torch.float32 else 'f64'}-{'x'.join(map(str, s))}" for d, s in CASES])
def test_deferred_update_is_bit_identical(dt, gres, monkeypatch):
    monkeypatch.setenv("MFS_SPARSE_MIN", "1")          # work lists from the first cell on (read when the engine is created)
    vec = 4 if dt == torch.float32 else 2
    assert gres[2] % vec == 0 and ((gres[1] - 2) * (gres[2] // vec)) % 256 != 0
    pb = _problem(gres, seed=sum(gres))
    for lists in (True, False):
        for xchunk, bpc, lean in KNOBS:
            kw = dict(xchunk=xchunk, bpc=bpc, lean=lean)
            on = _iterate(gres, dt, pb, True, lists, **kw)
            off = _iterate(gres, dt, pb, False, lists, **kw)
            assert (on["listed"] > 0) == lists
            assert float(on["x"].abs().max()) > 0 and np.all(np.isfinite(on["hist"]))
            _assert_same(on, off, (lists, kw))


LONG = [(d, s) for d, s in CASES if s[1] > 1000 and s[2] != 1028]


@pytest.mark.parametrize("dt,gres", LONG, ids=[f"{'f32' if d == torch.float32 else 'f64'}-{'x'.join(map(str, s))}" for d, s in LONG])
def test_carried_edge_weight_against_the_direct_kernel(dt, gres):
    """A deferred loop and an undeferred one share the march, so the comparison above is blind to what both get wrong.  The
    z-edge weight of a wave's last vector is requested one step ahead and carried; past a run's first plane it is the
    carried one that is used.  The stand-alone apply on runs of several planes (rows of 6, 10 and 34 vectors: lane 63 is no
    row end) against the direct-load kernel, which reads every neighbour and weight where it uses it: bit for bit."""
    pb = _problem(gres, seed=sum(gres) + 1)
    ops = [pb[k].to(dt) for k in ("lphi", "wx", "wy", "wz")]
    v = torch.randn(gres, generator=torch.Generator(device=DEV).manual_seed(5), device=DEV, dtype=torch.float64).to(dt)
    outs = []
    for variant, xchunk, bpc, compress in ((0, 0, 2, True), (2, 0, 1, True), (2, 3, 1, True), (2, 0, 2, False), (1, 0, 1, True)):
        eng = PcgEngine(gres, dt, DEV)
        eng.setup(*ops)
        eng.set_compress(compress)
        eng.tune(variant, xchunk, bpc, -1)
        out = torch.full(gres, 7.0, dtype=dt, device=DEV)
        eng.apply(v, out)
        outs.append(out)
    torch.cuda.synchronize()
    assert float((outs[0] - 7.0).abs().max()) > 0
    for k, o in enumerate(outs[1:]):
        assert torch.equal(outs[0], o), k + 1


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_lane_masked_march(dt, monkeypatch):
    """a ball of liquid in a box: most lanes of a listed pair are air, so the listed launches mask dead lanes.  ~900 listed
    pairs over 256 workgroups: runs of up to four planes."""
    monkeypatch.setenv("MFS_SPARSE_MIN", "1")
    gres = (100, 160, 128)
    pb = _problem(gres, seed=7, ball=((50.0, 80.0, 64.0), 45.0))
    kw = dict(bpc=1, poll_after=4)
    on = _iterate(gres, dt, pb, True, True, **kw)
    off = _iterate(gres, dt, pb, False, True, **kw)
    assert on["lane"] == 1.0 and off["lane"] == 1.0 and on["listed"] > 512
    _assert_same(on, off, "lane mask")
    dense = _iterate(gres, dt, pb, True, False, **kw)
    assert dense["lane"] == 0.0 and dense["listed"] == 0
    air = dense["x"] == 0
    assert torch.equal(on["x"][air], dense["x"][air])          # nothing leaks into the air


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("lean", [True, False], ids=["book", "tailed"])
def test_stop_inside_a_batch(dt, lean):
    """convergence at an iteration that is no multiple of check_every: the launches enqueued behind it return early, and the
    x update still owed is settled once"""
    gres, every = (6, 1220, 136) if dt == torch.float32 else (6, 1220, 68), 8
    pb = _problem(gres, seed=11)
    rr = _iterate(gres, dt, pb, False, False, bpc=1)["hist"][0::2]       # r.r after 0, 1, 2, ... iterations
    k = max(k for k in range(2, ITERS + 1) if k % every and rr[k] < 0.9 * rr[:k].min())
    tol = float((rr[k] * rr[:k].min()) ** 0.25)        # tol^2: the geometric mean of r.r at iteration k and the least before it
    outs = []
    for defer in (True, False):
        eng, v = _engine(gres, dt, pb, defer, False, bpc=1, lean=lean)
        ok, it = eng.solve(tol, 1000, every)
        torch.cuda.synchronize()
        assert ok and it == k and it % every != 0, (it, k)
        outs.append(dict(v, hist=eng.history()))
    _assert_same(outs[0], outs[1], "stop")


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("what", ["density", "jacobi", "warm_start"])
def test_other_operands(dt, what, monkeypatch):
    """the density operator's asymmetric -z tap, the fused Jacobi loop (z in place of r) and a non-zero x at begin"""
    monkeypatch.setenv("MFS_SPARSE_MIN", "1")
    gres = (6, 1220, 136) if dt == torch.float32 else (6, 1220, 68)
    pb = _problem(gres, seed=13)
    kw = dict(bpc=1, density=what == "density", jacobi=what == "jacobi", warm=what == "warm_start")
    for lists in (True, False):
        on = _iterate(gres, dt, pb, True, lists, **kw)
        off = _iterate(gres, dt, pb, False, lists, **kw)
        assert float(on["x"].abs().max()) > 0 and np.all(np.isfinite(on["hist"]))
        _assert_same(on, off, (what, lists))
