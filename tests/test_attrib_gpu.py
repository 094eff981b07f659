"""mfs.attrib on the MI355X against the brute-force oracle (tests/attrib_numpy.py): covered exactly where the oracle is
(the band, asserted empty first, holds the queries a rounding could turn), values within the derived per-query bound
(tests/test_attrib_oracle.py shows on the CPU that the kernel's float32 restatement stays inside it and
that two mutants do not), `fill` at the uncovered rows, the same bits from call to call and under a shuffle of the queries.

Measured on the MI355X (for the reader; printed by every run), GPU error / bound at worst: cloud 0.16 (C = 1, 3) and 0.20
(C = 4), 0.16 to 0.27 over the eight dtype pairings, shuffled particles 0.20, 600 particles in one bin 0.12, 300 queries in
one bin 0.09, one point 0.02, box faces 0.07, non-finite input 0.17, the dyadic case 0 (exact)."""
import functools

import numpy as np
import pytest
import torch

import attrib_numpy as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def reference(name):
    """(px, values, queries, R, box, oracle) -- computed once per case, never modified"""
    px, vals, q, R, box = A.CASES[name]()
    ref = A.gather(px, vals, q, R, box)
    for a in (px, vals, q, ref["A"], ref["K"], ref["W"], ref["bound"], ref["band"]):
        a.setflags(write=False)
    return px, vals, q, R, box, ref


def gpu_gather(name, C=4, dts=(F64, F64, F64), px=None, vals=None, q=None, **kw):
    from mfs import attrib
    p0, v0, q0, R, box, _ = reference(name)
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=DEV)  # noqa: E731
    v = (v0 if vals is None else vals)[:, :C]
    return attrib.gather(t(q0 if q is None else q, dts[2]), t(p0 if px is None else px, dts[0]), t(v, dts[1]), R, box, **kw)


def check(name, got, weight, C, ref=None, what=""):
    ref = reference(name)[5] if ref is None else ref
    if name != "exactly_R":                                              # t == 0 there on purpose; float32 is exact on it
        assert not ref["band"].any()                                     # first: then no query is left out below
    assert got.dtype == F32 and weight.dtype == F32 and tuple(got.shape) == (len(ref["K"]), C) and got.is_cuda
    g, w = N(got), N(weight)
    cov = ref["K"] > 0
    np.testing.assert_array_equal(w > 0, cov)
    ex = A.excess(g, dict(ref, A=ref["A"][:, :C], bound=ref["bound"][:, :C]))
    print(f"{name}{what} C={C}: {cov.sum()} of {len(cov)} covered, K up to {ref['K'].max()}, GPU error / bound max {ex.max():.3f}")
    assert ex.max() <= 1.0
    assert np.isnan(g[~cov]).all() and (w[~cov] == 0).all()
    return g, w


@pytest.mark.parametrize("C", [1, 3, 4])
def test_the_cloud_matches_the_oracle(C):
    px, _, q, _, _, ref = reference("cloud")
    assert px.shape == (1680, 3) and q.shape == (2000, 3) and ref["K"].max() >= 70 and 0.1 < (ref["K"] == 0).mean() < 0.5
    stats = {}
    got, weight = gpu_gather("cloud", C, stats=stats)
    check("cloud", got, weight, C)
    assert stats["work_items"] >= 100 and stats["pair_tests"] >= int(ref["K"].sum()) and stats["bins"] > 27
    print(stats)


@pytest.mark.parametrize("dts", [(p, v, q) for p in (F32, F64) for v in (F32, F64) for q in (F32, F64)],
                         ids=lambda d: "-".join(str(t)[-2:] for t in d))
def test_every_dtype_pairing(dts):
    """float32 particles / queries are other points than their float64 originals: the oracle is evaluated at what the GPU got"""
    px, vals, q, R, box, ref = reference("cloud")
    if dts != (F64, F64, F64):
        cast = lambda a, dt: a.astype(np.float32).astype(np.float64) if dt == F32 else a  # noqa: E731
        # (the default box is the bounding box of the queries as given: the oracle takes it from the rounded ones too)
        ref = A.gather(cast(px, dts[0]), vals, cast(q, dts[2]), R, box)
    got, weight = gpu_gather("cloud", 3, dts)
    check("cloud", got, weight, 3, ref, what=" " + "-".join(str(t)[-2:] for t in dts))


def test_fill_and_repeatability_and_query_order():
    px, vals, q, R, box, ref = reference("cloud")
    got, weight = gpu_gather("cloud", 4, fill=-3.5)
    assert (N(got)[ref["K"] == 0] == -3.5).all() and np.isfinite(N(got)).all()
    base, wbase = gpu_gather("cloud", 4)
    again, wagain = gpu_gather("cloud", 4)
    same = lambda a, b: np.array_equal(N(a).view(np.uint32), N(b).view(np.uint32))  # noqa: E731
    assert same(base, again) and same(wbase, wagain)                     # a second call: identical bits
    perm = np.random.default_rng(4).permutation(len(q))
    shuffled, wsh = gpu_gather("cloud", 4, q=q[perm])
    assert same(shuffled, base[torch.as_tensor(perm, device=DEV)])       # the order of summation is the particles' alone
    assert same(wsh, wbase[torch.as_tensor(perm, device=DEV)])


def test_shuffled_particles_stay_within_the_bound():
    px, vals, q, R, box, ref = reference("cloud")
    perm = np.random.default_rng(5).permutation(len(px))
    got, weight = gpu_gather("cloud", 4, px=px[perm], vals=vals[perm])
    check("cloud", got, weight, 4, what=" shuffled particles")


def test_a_reused_bins_equals_the_direct_call():
    from mfs import attrib
    px, vals, q, R, _, ref = reference("cloud")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    box = A.default_box(q)
    B = attrib.bins(t(px), R, box)
    assert isinstance(B, attrib.Bins) and B.shape == A.lattice(box, R)[1] and B.influence == R
    assert tuple(B.starts.shape) == (int(np.prod(B.shape)) + 1,) and int(B.starts[-1]) == len(px)
    assert torch.equal(B.particles, t(px)[B.order])
    for C in (1, 3):
        direct = attrib.gather(t(q), t(px), t(vals[:, :C]), R)
        held = attrib.gather(t(q), B, t(vals[:, :C]))
        assert torch.equal(direct[0].view(torch.int32), held[0].view(torch.int32)) and torch.equal(direct[1], held[1])
    via = attrib.at_vertices(type("M", (), {"vertices": t(q.astype(np.float32))})(), t(px), t(vals[:, 0]), R)
    assert torch.equal(via[0].view(torch.int32), attrib.gather(t(q.astype(np.float32)), t(px), t(vals[:, 0]), R)[0].view(torch.int32))
    with pytest.raises(ValueError, match="influence"):
        attrib.gather(t(q), B, t(vals), influence=2 * R)
    with pytest.raises(ValueError, match="box"):
        attrib.gather(t(q), B, t(vals), box=((0, 0, 0), (1, 1, 1)))


@pytest.mark.parametrize("name", ["crowded_bin", "crowded_queries", "one_point", "faces", "non_finite", "exactly_R"])
def test_the_shapes_where_the_kernel_can_go_wrong(name):
    px, vals, q, R, box, ref = reference(name)
    stats = {}
    got, weight = gpu_gather(name, 4, stats=stats)
    g, w = check(name, got, weight, 4)
    if name == "crowded_bin":                                            # 600 particles: batches of 256, 256 and 88
        assert ref["K"].max() == 600 and stats["pair_tests"] == 256 * 600 * stats["work_items"]
    if name == "crowded_queries":                                        # 300 queries of one bin: chunks of 256 and 44
        assert stats["work_items"] == 2 and stats["bins"] == 64       # the box is one bin wide: 1 + 3 bins per axis
    if name == "one_point":
        assert stats["work_items"] == 1 and stats["bins"] == 27
        assert (g.view(np.uint32) == g.view(np.uint32)[0]).all()
    if name == "faces":
        assert (ref["K"][:62] > 0).all() and (ref["K"][62:94] == 0).all()
    if name == "non_finite":
        hit = ref["t"][:, 100] > 0
        assert hit.any() and np.isnan(g[hit, 0]).all() and np.isfinite(g[(ref["K"] > 0) & ~hit, 0]).all()
        assert np.isinf(g[ref["t"][:, 200] > 0, 1]).all() and np.isnan(g[[3, 8, 11]]).all()
    if name == "exactly_R":
        np.testing.assert_array_equal(w > 0, [False, True, True, False, False, True])
        np.testing.assert_array_equal(g[[1, 2, 5]], ref["A"][[1, 2, 5]])


def test_one_query_no_query_no_particle():
    from mfs import attrib
    px, vals, q, R, _, ref = reference("cloud")
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    k = int(np.argmax(ref["K"]))
    one = A.gather(px, vals, q[k:k + 1], R)
    got, weight = attrib.gather(t(q[k:k + 1]), t(px), t(vals), R)
    assert tuple(got.shape) == (1, 4) and A.excess(N(got), one).max() <= 1.0 and float(weight[0]) > 0
    got, weight = attrib.gather(t(q[:0]), t(px), t(vals), R)
    assert tuple(got.shape) == (0, 4) and tuple(weight.shape) == (0,) and got.dtype == F32
    got, weight = attrib.gather(t(q), t(px[:0]), t(vals[:0, :2]), R, fill=2.0)
    assert tuple(got.shape) == (2000, 2) and bool((got == 2.0).all()) and bool((weight == 0).all())
    got, weight = attrib.gather(torch.full((3, 3), float("nan"), device=DEV), t(px), t(vals[:, 0]), R)
    assert tuple(got.shape) == (3, 1) and bool(torch.isnan(got).all()) and bool((weight == 0).all())
    B = attrib.bins(t(px[:0]), R, A.default_box(q))
    assert int(B.starts.sum()) == 0 and bool(torch.isnan(attrib.gather(t(q[:5]), B, t(vals[:0]))[0]).all())
