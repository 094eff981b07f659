"""The particle <-> grid restatements (oracle/mfs_oracle.py nb_p2g_*, nb_g2p_*, nb_fluid_*) against goldens
produced by executing the notebook's own cells (tests/golden/make_goldens_particles.py, pt_*)."""
import numpy as np
import pytest

from conftest import golden, golden_names
from oracle import mfs_oracle as O

BIAS = {0: (0, .5, .5), 1: (.5, 0, .5), 2: (.5, .5, 0)}


def containers(g):
    gres = tuple(int(v) for v in g["gres"])
    bmin = np.asarray(g["bound_min"], np.float32)
    cs = np.asarray(g["bound_size"], np.float32) / np.asarray(gres, np.int64)          # float64, like the notebook's
    return gres, bmin, cs


@pytest.mark.parametrize("name", golden_names("pt_"))
def test_particle_transfers(name):
    g = golden(name)
    gres, bmin, cs = containers(g)
    assert cs.dtype == np.float64
    grids = {}
    for a, c in enumerate("xyz"):
        shape = tuple(np.array(gres) + np.eye(3, dtype=int)[a])
        gm, gv = np.zeros(shape, np.float32), np.zeros(shape, np.float32)
        O.nb_p2g_scatter(g["px"], g["pm"], g["pv"], g["pc" + c], gm, gv, bmin, gres, BIAS[a], cs, a)
        O.nb_p2g_normalize(gm, gv)
        # fp32 accumulation in particle order: agreement to a few ulps of the largest entry
        np.testing.assert_allclose(gm, g[f"g{c}_m"], rtol=0, atol=2e-6 * np.abs(g[f"g{c}_m"]).max())
        np.testing.assert_allclose(gv, g[f"g{c}_v"], rtol=2e-4, atol=2e-5 * np.abs(g[f"g{c}_v"]).max())
        grids[c] = g[f"g{c}_v"]
    pv = np.array(g["pv"])
    for a, c in enumerate("xyz"):
        pca = np.array(g["pc" + c])
        O.nb_g2p_gather(bmin, gres, BIAS[a], cs, a, g["px"], pv, pca, grids[c])
        np.testing.assert_allclose(pca, g["g2p_c" + c], rtol=1e-12, atol=1e-12 * np.abs(g["g2p_c" + c]).max())
    np.testing.assert_allclose(pv, g["g2p_v"], rtol=1e-12, atol=1e-13)
    phi = np.zeros(gres)
    O.nb_fluid_levelset(g["px"], phi, bmin, cs, float(g["gdx"]), gres)
    np.testing.assert_allclose(phi, g["lphi"], rtol=1e-13, atol=1e-15)
    vres = tuple(2 * np.array(gres) + 1)
    vcs = np.asarray(g["bound_size"], np.float32) / (2 * np.asarray(gres, np.int64))
    vol = np.zeros(vres)
    O.nb_fluid_volume(bmin, vcs, vres, g["px"], float(g["pvol"]), vol)
    np.testing.assert_allclose(vol, g["lvol"], rtol=1e-11, atol=1e-15 * np.abs(g["lvol"]).max())


# ------------------------------------------------------------------ float64 reference with a per-node bound ---------
# A node that receives K terms t_i, S = sum |t_i|: a sum in arrays of unit roundoff u rounds each term once on conversion
# (u S in all) and once per add (at most (K - 1) u S), so it lies within (K + 2) u S of the exact sum whatever the
# order; the float64 reference's own error is 2^-29 of that for float32 arrays.  K and S come from the oracle (`stats=`).
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}


def _within(got, ref, K, S, u, what):
    err, bound = np.abs(np.asarray(got, np.float64) - ref), (K + 2) * u * S
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    assert ratio.max() <= 1.0, f"{what}: worst err / bound {ratio.max():.3g} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    assert (np.asarray(got)[K == 0] == 0.0).all(), f"{what}: a node without contributions is not 0.0"
    return float(ratio.max())


@pytest.mark.parametrize("name", golden_names("pt_"))
def test_float64_scatter_reference_against_the_goldens(name):
    """the pt_* goldens (the notebook's own float32 atomics) lie within the per-node bound of the float64-accumulated
    oracle: mass directly; momentum as golden velocity x golden mass where the notebook divided (one more rounding, the
    division's, on top of the K - 1 adds and the conversions: still within (K + 2) u S)"""
    g = golden(name)
    gres, bmin, cs = containers(g)
    for a, c in enumerate("xyz"):
        shape = tuple(np.array(gres) + np.eye(3, dtype=int)[a])
        gm, gv, st = np.zeros(shape), np.zeros(shape), {}
        O.nb_p2g_scatter(g["px"], g["pm"], g["pv"], g["pc" + c], gm, gv, bmin, gres, BIAS[a], cs, a, stats=st)
        u = U[g[f"g{c}_m"].dtype]
        _within(g[f"g{c}_m"], gm, st["K"], st["S_m"], u, f"{name} g{c}_m")
        m32 = g[f"g{c}_m"].astype(np.float64)
        mom = np.where(m32 > 0, g[f"g{c}_v"].astype(np.float64) * m32, g[f"g{c}_v"])
        _within(mom, gv, st["K"], st["S_v"], u, f"{name} g{c}_v * g{c}_m")
        last = [slice(None)] * 3
        last[a] = -1
        assert not st["K"][tuple(last)].any()                 # indices clamp to gres - 1: the last face plane gets nothing
    vres = tuple(2 * np.array(gres) + 1)
    vcs = np.asarray(g["bound_size"], np.float32) / (2 * np.asarray(gres, np.int64))
    vol, st = np.zeros(vres), {}
    O.nb_fluid_volume(bmin, vcs, vres, g["px"], float(g["pvol"]), vol, stats=st)
    _within(g["lvol"], vol, st["K"], st["S_vol"], U[g["lvol"].dtype], f"{name} lvol")      # min(., cell volume) is 1-Lipschitz


@pytest.mark.parametrize("name", golden_names("d3d_"))
def test_float64_density_splat_against_the_goldens(name):
    g = golden(name)
    gres = tuple(int(v) for v in g["gres"])
    cs = np.asarray(g["bound_size"], np.float64) / np.asarray(gres, np.float64)
    gm, gvol, st = np.zeros(gres), np.zeros(gres), {}
    O.density_splat3d(g["bound_min"], cs, gres, g["px"], g["pm"], float(g["pvol"]), gm, gvol, stats=st)
    _within(g["gm"], gm, st["K"], st["S_m"], U[g["gm"].dtype], f"{name} gm")
    _within(g["gvol_raw"], gvol, st["K"], st["S_vol"], U[g["gvol_raw"].dtype], f"{name} gvol_raw")
    assert st["K"].sum() == 8 * len(g["px"])


@pytest.mark.parametrize("name", golden_names("pt_"))
def test_contribution_counts_are_what_scattering_ones_gives(name):
    g = golden(name)
    gres, bmin, cs = containers(g)
    x32 = np.asarray(g["px"]).astype(np.float32)
    t = (x32 - bmin).astype(np.float64) / cs
    for a, c in enumerate("xyz"):
        shape = tuple(np.array(gres) + np.eye(3, dtype=int)[a])
        st = {}
        O.nb_p2g_scatter(g["px"], g["pm"], g["pv"], g["pc" + c], np.zeros(shape), np.zeros(shape), bmin, gres, BIAS[a], cs, a,
                         stats=st)
        base = np.floor(t - np.asarray(BIAS[a], np.float32).astype(np.float64)).astype(np.int64)
        ones = np.zeros(shape, np.int64)
        for off in np.ndindex(2, 2, 2):
            idx = tuple(np.clip(base[:, d] + off[d], 0, gres[d] - 1) for d in range(3))
            np.add.at(ones, idx, 1)
        assert st["K"].dtype.kind == "i" and np.array_equal(st["K"], ones) and st["K"].sum() == 8 * len(x32)
        assert (st["S_m"][ones == 0] == 0).all() and (st["S_m"] >= 0).all() and st["S_m"].shape == shape
    vres = tuple(2 * np.array(gres) + 1)
    st = {}
    O.nb_fluid_volume(bmin, cs / 2, vres, g["px"], float(g["pvol"]), np.zeros(vres), stats=st)
    ones = np.zeros(vres, np.int64)
    base = np.floor(2 * t).astype(np.int64)
    for off in np.ndindex(2, 2, 2):
        np.add.at(ones, tuple(np.clip(base[:, d] + off[d], 0, vres[d] - 1) for d in range(3)), 1)
    assert np.array_equal(st["K"], ones)


@pytest.mark.parametrize("name", golden_names("pt_"))
@pytest.mark.parametrize("gdt", [np.float32, np.float64])
def test_float32_gather_rounds_every_partial_sum(name, gdt):
    """float32 particle arrays: pv[P, axis] += ... rounds each of the 8 partial sums to float32 -- within
    8 * 2^-24 * sum |terms| of the float64 gather per particle, and not identical to it (the rounding is modelled)"""
    g = golden(name)
    gres, bmin, cs = containers(g)
    P = len(g["px"])
    v64, v32 = np.zeros((P, 3)), np.zeros((P, 3), np.float32)
    for a, c in enumerate("xyz"):
        G = g[f"g{c}_v"].astype(gdt)
        c64, c32, st = np.zeros((P, 3)), np.zeros((P, 3), np.float32), {}
        O.nb_g2p_gather(bmin, gres, BIAS[a], cs, a, g["px"], v64, c64, G, stats=st)
        O.nb_g2p_gather(bmin, gres, BIAS[a], cs, a, g["px"], v32, c32, G)
        assert c32.dtype == np.float32 and v32.dtype == np.float32
        assert (np.abs(v32[:, a] - v64[:, a]) <= 8 * 2.0 ** -24 * st["S_v"]).all()
        assert (np.abs(c32 - c64) <= 8 * 2.0 ** -24 * st["S_c"]).all()
        # not merely the float64 result rounded once at the end
        assert (v32[:, a] != v64[:, a].astype(np.float32)).any() and (c32 != c64.astype(np.float32)).any()
        assert (st["S_v"] >= np.abs(v64[:, a]) * (1 - 1e-15)).all()
