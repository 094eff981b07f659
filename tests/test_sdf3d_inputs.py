"""CPU checks on the inputs and bounds of tests/test_sdf3d_branches_gpu.py (tests/sdf3d_inputs.py): over the union of the
generic, exact and chain inputs every comparison of the rigid-body oracle (`trace=`) is taken on both sides; the generic
points keep MARGIN from every threshold and the exact points sit on theirs; a last-bit change of every square root stays
within the bound and within the float32 slack; and every planted mistake of I.MISTAKES is caught by the comparison that
the GPU test makes -- bits on the exact points, err / bound on the generic ones, `f32_verdict` on the float32 chain.

Unreachable comparisons: none.  Four comparisons have a neighbour that no input can tell from them (`disp >= 0`,
`max_disp <= 0`, `prb[1] >= hh`, the cap test by `>=`; reasons in I.MISTAKES): those are shown to be bit-identical on every
input here, and a catchable mistake of the same comparison stands next to each.

Measured: the smallest err / bound of a planted mistake caught on the generic points is 1.1e+13 (a flipped box clamped
only when in_out == 0; the test prints each, inf where the velocity of another body is written), so the floor is 1e12."""
import inspect
import re

import numpy as np
import pytest

import sdf3d_inputs as I
from oracle import mfs_oracle as O

F32, F64 = np.float32, np.float64
FLOOR = 1e12
TRACED = ("_sdf_eval_one", "sdf_evaluate", "sdf_project")
N_MISTAKE = 400                       # generic points that the mistakes are tried on
UNREACHABLE = {}                      # comparison name -> why one of its sides cannot be taken


def _all_inputs():
    yield "generic", I.GENERIC_TABLES["middle"], I.generic_points()
    yield "chain", I.CHAIN, I.chain_points()
    for name, (rb, pts, _) in I.EXACT_SCENES.items():
        yield name, rb, pts


def _results(mistake=None, pdt=F64, **kw):
    """{(input, what): array} of the oracle (or a mistaken copy) over every input"""
    out = {}
    for name, rb, pts in _all_inputs():
        sd, vel, _ = I.evaluate(rb, pts, pdt, mistake=mistake)
        out[name, "sd"], out[name, "vel"] = sd, vel
        out[name, "project"] = I.project(rb, pts, pdt, mistake=mistake, **kw)[0]
    return out


@pytest.fixture(scope="module")
def base():
    return {F64: _results(), F32: _results(pdt=F32)}


# ----------------------------------------------------------------------------------------------------- coverage ---
def test_every_comparison_is_taken_on_both_sides():
    names = [n for f in TRACED for n in re.findall(r'_tr\(trace, "([^"]+)"', inspect.getsource(getattr(O, f)))]
    assert len(names) == len(set(names)) == 27
    t = {}
    for _, rb, pts in _all_inputs():
        I.evaluate(rb, pts, trace=t)
        I.project(rb, pts, trace=t)
    missing = [(n, side) for n in names for side in (True, False) if not t.get((n, side), 0) and n not in UNREACHABLE]
    assert not missing, missing
    assert {k[0] for k in t if isinstance(k, tuple)} == set(names)
    # the generic points alone take both sides of every comparison that can be off its threshold on both sides
    g = {}
    I.evaluate(I.GENERIC_KNOWN, I.generic_points(), trace=g)
    I.project(I.GENERIC_KNOWN, I.generic_points(), trace=g)
    thin = [(n, side) for n in names for side in (True, False) if g.get((n, side), 0) < 2]
    assert not thin, thin


def test_trace_and_magnitudes_change_no_result(base):
    for name, rb, pts in _all_inputs():
        sd, vel = np.zeros(len(pts)), np.zeros((len(pts), 3))
        with np.errstate(all="ignore"):
            O.sdf_evaluate(rb, sd, vel, pts)
            p = pts.copy()
            O.sdf_project(rb, p)
        for what, got in (("sd", sd), ("vel", vel), ("project", p)):
            assert not I.bit_mismatches(got, base[F64][name, what]).any(), (name, what)
        _, _, M = I.evaluate(rb, pts)
        assert (M >= np.abs(sd) * (1 - 1e-12))[sd != 100].all()


def test_the_unknown_row_changes_nothing_wherever_it_sits():
    pts = I.generic_points()
    want = (I.evaluate(I.GENERIC_KNOWN, pts)[:2], I.project(I.GENERIC_KNOWN, pts)[0])
    for where, rb in I.GENERIC_TABLES.items():
        assert (rb[:, 0, 0] == I.MESH_CODE).sum() == 1 and sorted(rb[:, 0, 0]) == [0, 1, 2, 3, 4, 5, 6]
        sd, vel, _ = I.evaluate(rb, pts)
        assert not I.bit_mismatches(sd, want[0][0]).any() and not I.bit_mismatches(I.project(rb, pts)[0], want[1]).any()
        assert not I.bit_mismatches(vel, want[0][1]).any()
        assert not (vel == rb[rb[:, 0, 0] == I.MESH_CODE][0, -1, :3]).all(axis=1).any()         # its velocity is never written
    assert {"first": 0, "middle": 3, "last": 6} == {k: int(np.flatnonzero(rb[:, 0, 0] == 6)[0]) for k, rb in I.GENERIC_TABLES.items()}
    assert (np.abs(I.GENERIC_KNOWN[:, 5:8, :3] - np.identity(3)).max(axis=(1, 2)) > 0.01).sum() >= 4     # rotated


# ------------------------------------------------------------------------------------------- margins, exactness ---
@pytest.mark.parametrize("pdt", [F64, F32], ids=["p64", "p32"])
def test_generic_and_chain_points_keep_the_margin(pdt):
    for rb, pts, n in ((I.GENERIC_KNOWN, I.generic_points(), I.N_GENERIC), (I.CHAIN, I.chain_points(), I.N_CHAIN)):
        m = I._margins(rb, pts, pdt)
        assert m.shape == (n,) and (m > I.MARGIN).all(), float(m.min())
    sd, vel, _ = I.evaluate(I.GENERIC_KNOWN, I.generic_points(), pdt)
    assert 200 < (sd <= 0).sum() < I.N_GENERIC - 200                         # vel written and left alone, both often
    assert len(np.unique(vel, axis=0)) == 7                                  # every body wins somewhere, and none
    after = I.project(I.GENERIC_KNOWN, I.generic_points(), pdt)[0].astype(F64)
    moved = np.abs(after - I.generic_points().astype(pdt).astype(F64)).max(axis=1) > 1e-3      # beyond a rounding
    assert 200 < moved.sum() < I.N_GENERIC - 200


ON_THE_THRESHOLD = {
    "solids": ["box_eval disp > 0", "box_eval max_disp < disp", "box_eval max_disp < 0", "evaluate min_sd <= 0",
               "evaluate d < min_sd", "cylinder_eval y > hh", "cylinder_eval y < -hh", "cylinder_eval sd < 0",
               "cylinder_eval max is radial", "sphere_project sd < 0", "box_project prb > h", "box_project prb < -h",
               "box_project h - prb < dist", "box_project prb + h < dist", "cylinder_project y > hh",
               "cylinder_project y < -hh", "cylinder_project sd < 0", "cylinder_project mv == sd"],
    "flipped box": ["box_eval disp > 0", "box_eval max_disp < 0", "evaluate min_sd <= 0", "box_project prb > h", "box_project prb < -h"],
    "flipped sphere": ["evaluate min_sd <= 0", "sphere_project sd < 0"],
    "flipped cylinder": ["cylinder_eval sd < 0", "cylinder_eval y > hh", "cylinder_eval y < -hh", "evaluate min_sd <= 0",
                         "cylinder_project flipped sd > 0", "cylinder_project flipped sd >= 0", "cylinder_project y > hh"],
    "solid and flipped box": ["evaluate min_sd <= 0", "box_project prb > h"],
}


@pytest.mark.parametrize("scene", sorted(I.EXACT_SCENES))
def test_exact_points_sit_on_their_thresholds(scene, base):
    rb, pts, names = I.EXACT_SCENES[scene]
    assert len(set(names)) == len(names) == len(pts)
    assert (rb[:, 5:9] == np.identity(4)).all()
    for a in (rb[:, 0, 1:], rb[:, 1:4, 3], rb[:, 9, :3]):
        assert (a * 2 ** 10 == np.round(a * 2 ** 10)).all()                  # dyadic sizes, centres and velocities
    t = {}
    I.evaluate(rb, pts, trace=t)
    I.project(rb, pts, trace=t)
    off = [n for n in ON_THE_THRESHOLD[scene] if t["gaps"].get(n) != 0.0]
    assert not off, off
    sd = base[F64][scene, "sd"]
    assert (sd * 2 ** 10 == np.round(sd * 2 ** 10)).all(), "an inexact distance among the exact points"
    # and they are distances that a last-bit change of a square root would alter: the roots themselves are exact there
    alt = ("_sdf_eval_one", " ** 0.5", " ** 0.5 * (1 + 2.0 ** -52)", 4)
    assert I.bit_mismatches(I.evaluate(rb, pts, mistake=alt)[0], sd).any()
    nan = np.isnan(base[F64][scene, "project"]).all(axis=1)
    assert not np.isnan(sd).any() and not (np.isnan(base[F64][scene, "project"]).any(axis=1) & ~nan).any()
    assert [n for n, k in zip(names, nan) if k] == I.NAN_POINTS.get(scene, [])


def test_exact_results_are_what_the_reference_text_says(base):
    """a few of the exact expectations, spelled out by hand from solver/sdf3D.py rather than taken from the oracle"""
    rb, pts, names = I.EXACT_SCENES["solids"]
    at = names.index
    sd, vel, proj = (base[F64]["solids", k] for k in ("sd", "vel", "project"))
    for n in ("box face", "box edge", "box corner", "sphere surface", "fat cylinder rim", "fat cylinder side",
              "fat cylinder cap plane inside the radius", "sphere and box touch"):
        assert sd[at(n)] == 0 and not np.signbit(sd[at(n)]) and vel[at(n)].any(), n
        assert (proj[at(n)] == pts[at(n)]).all(), n
    assert (vel[at("box face")] == I.V[0]).all() and (vel[at("sphere and box touch")] == I.V[7]).all()
    assert (vel[at("coincident spheres, inside")] == I.V[5]).all()                                 # the first of the two
    assert (proj[at("box inside, +x and +y tie")] == (0.5, 0.1875, 0)).all()                       # +x before +y
    assert (proj[at("box inside, -x and -y tie")] == (-0.5, -0.1875, 0)).all()                     # -x before -y
    assert (proj[at("box inside, +y and -z tie")] == (0, 0.25, -0.0625)).all()                     # +y before -z
    assert (proj[at("cube centre, six faces tie")] == (0.25, -2, 0)).all()                         # +x before all
    assert (proj[at("fat cylinder inside, three-way tie")] == (0.625, 4, 0)).all()                 # radial first
    assert (proj[at("fat cylinder inside, radial and top tie")] == (0.625, 4.125, 0)).all()
    assert (proj[at("fat cylinder axis")] == (0, 4.25, 0)).all() and sd[at("fat cylinder axis")] == -0.25
    assert sd[at("farther than 100 from everything")] == 100 and not vel[at("farther than 100 from everything")].any()
    assert sd[at("fat cylinder cap plane outside the radius")] == 0.625 and sd[at("fat cylinder above the cap, inside")] == 0.25
    assert base[F64]["flipped box", "sd"][-1] == -499.5 and base[F64]["solid and flipped box", "sd"][0] == -498.0
    assert (base[F64]["solid and flipped box", "vel"][0] == I.V[4]).all()
    fsd = base[F64]["flipped box", "sd"]
    assert (fsd[:3] == 0).all() and np.signbit(fsd[:3]).all() and base[F64]["flipped box", "vel"][:3].all()
    rim = I.EXACT_SCENES["flipped cylinder"][1][0]
    assert (base[F64]["flipped cylinder", "project"][0] != rim).any()                              # the rescale shows in a bit


def test_grid_nodes_hold_exact_points():
    rb = I.EXACT_SCENES["solids"][0]
    nodes = I.grid_nodes(I.GRID["biases"][0]).reshape(-1, 3)
    assert (nodes * 2 ** 10 == np.round(nodes * 2 ** 10)).all()
    sd, vel, _ = I.evaluate(rb, nodes)
    on = (sd == 0).sum()
    assert on >= 20 and (sd < 0).any() and (sd > 0).any() and (nodes == (2, 0, 0)).all(axis=1).any()
    have = {tuple(p) for p in nodes}
    assert {(0.5, 0.25, 0.125), (0.5, 0.25, 0.0), (0.5, 0.0, 0.0), (0.0, 0.0, 0.0)} <= have
    assert len(np.unique(vel[sd <= 0], axis=0)) == 2                                               # the box and the sphere


# -------------------------------------------------------------------------------------------------------- chain ---
def test_the_chain_moves_points_again_and_rounding_per_body_shows():
    pts = I.chain_points()
    assert (I.CHAIN[:, 0, 0] // 2).tolist()[:3] == [0, 1, 2]
    p = [pts] + [I.project(I.CHAIN[:k], pts)[0] for k in (1, 2, 3, 4)]
    first = (p[1] != p[0]).any(axis=1)
    assert (first & (p[2] != p[1]).any(axis=1)).sum() >= 50 and (first & (p[3] != p[2]).any(axis=1)).sum() >= 50
    assert (first & (p[2] != p[1]).any(axis=1) & (p[3] != p[2]).any(axis=1)).sum() >= 10
    each, once = I.project(I.CHAIN, pts, F32)[0], I.project(I.CHAIN, pts, F32, round_each=False)[0]
    assert each.dtype == once.dtype == np.float32
    share = (each != once).any(axis=1).mean()
    print(f"CHAIN float32: rounding per body differs from rounding once at {share:.2%} of the points")
    assert share >= 0.01
    over, slack = I.f32_verdict(once, each)
    assert over > 0 and slack > I.F32_SLACK_SHARE                            # the GPU test's comparison refuses it twice over


@pytest.mark.parametrize("factor", ["(1 + 2.0 ** -52)", "(1 - 2.0 ** -53)"], ids=["up", "down"])
def test_a_last_bit_change_of_every_square_root_is_allowed(factor, base):
    """what kernel and oracle may differ by: stays within the float64 bound and within the float32 slack on these inputs"""
    ev, pr = ("_sdf_eval_one", " ** 0.5", " ** 0.5 * " + factor, 4), ("sdf_project", " ** 0.5", " ** 0.5 * " + factor, 2)
    for name, rb, pts in list(_all_inputs())[:2]:
        want, _, M = I.evaluate(rb, pts)
        got, vel, _ = I.evaluate(rb, pts, mistake=ev)
        r = I.excess(got, want, M, I.r_evaluate(rb))
        assert 0 < r.max() <= 1.0, (name, r.max())
        assert not I.bit_mismatches(vel, base[F64][name, "vel"]).any()
        want, M = I.project(rb, pts)
        r = I.excess(I.project(rb, pts, mistake=pr)[0], want, M, I.r_project(rb))
        assert 0 < r.max() <= 1.0, (name, r.max())
        over, slack = I.f32_verdict(I.project(rb, pts, F32, mistake=pr)[0], base[F32][name, "project"])
        print(f"SQRT {factor} {name}: float32 points differing {slack:.3%}, more than one ulp {over}")
        assert over == 0 and slack <= I.F32_SLACK_SHARE


# ------------------------------------------------------------------------------------------------ the mistakes ---
def _caught(mistake, base):
    """(worst err / bound on the generic points, exact arrays with other bits, float32 chain refused)"""
    rb, pts = I.GENERIC_TABLES["middle"], I.generic_points()[:N_MISTAKE]
    want, wvel, M = I.evaluate(rb, pts)
    got, vel, _ = I.evaluate(rb, pts, mistake=mistake)
    worst = float(I.excess(got, want, M, I.r_evaluate(rb)).max())
    if I.bit_mismatches(vel, wvel).any():
        worst = np.inf
    want, M = I.project(rb, pts)
    worst = max(worst, float(I.excess(I.project(rb, pts, mistake=mistake)[0], want, M, I.r_project(rb)).max()))
    alt = {}
    for name, (erb, epts, _) in I.EXACT_SCENES.items():
        alt[name, "sd"], alt[name, "vel"], _ = I.evaluate(erb, epts, mistake=mistake)
        alt[name, "project"] = I.project(erb, epts, mistake=mistake)[0]
    exact = sorted(k for k in alt if I.bit_mismatches(alt[k], base[F64][k]).any())
    over, slack = I.f32_verdict(I.project(I.CHAIN, I.chain_points(), F32, mistake=mistake)[0], base[F32]["chain", "project"])
    return worst, exact, over > 0 or slack > I.F32_SLACK_SHARE


def test_planted_mistakes_are_caught(base):
    failed, least = [], np.inf
    for name, mistake, where in I.MISTAKES:
        worst, exact, f32 = _caught(mistake, base)
        print(f"MISTAKE {name}: generic err / bound {worst:.3g}; exact arrays with other bits {exact}; float32 chain refused {f32}")
        if where == "generic":
            least = min(least, worst)
            ok = worst >= FLOOR
        elif where == "exact":
            ok = bool(exact)
        elif where == "f32":
            ok = f32
        else:
            assert where.startswith("equivalent: ")
            ok = worst == 0 and not exact and not f32
            alt = _results(mistake)
            ok = ok and not any(I.bit_mismatches(alt[k], base[F64][k]).any() for k in alt)
        if not ok:
            failed.append((name, where, worst, exact, f32))
    print(f"MISTAKE smallest err / bound among those caught on the generic points: {least:.3g}")
    assert not failed, failed
    assert least >= FLOOR


def test_the_mistake_table_names_what_the_issue_lists():
    names = " | ".join(n for n, _, _ in I.MISTAKES)
    for needle in ("d < min_sd to <=", "min_sd <= 0 to < 0", "start value 100", "R for R^T", "translation applied before",
                   "disp > 0 to >= 0", "max_disp < 0 to <= 0", "face tests of box_project swapped", "only when in_out == 0",
                   "prb[1] > hh to >=", "cap test by >=", "flip sign dropped on the cylinder", "sd >= 0 to sd > 0",
                   "answering -hh", "no float32 rounding between bodies", "radius p[2]"):
        assert needle in names, needle
    for name, _, where in I.MISTAKES:                    # every equivalent one has a catchable neighbour
        assert where in ("generic", "exact", "f32") or where.startswith("equivalent: "), name
    assert sum(w.startswith("equivalent") for _, _, w in I.MISTAKES) == 5 and len(I.MISTAKES) >= 16 + 5


def test_an_unmistaken_copy_is_the_oracle(base):
    same = ("sdf_project", "if round_each:", "if round_each:")
    alt = _results(same)
    assert not any(I.bit_mismatches(alt[k], base[F64][k]).any() for k in alt)
