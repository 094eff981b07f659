"""mfs.scenes.particle_stress_scene_3d carries every hazard tests/test_particles_stress_gpu.py leans on (CPU only): what
is asserted here is the CONDITION for a code path (partial tiles, the tile sort's table overflow, index clamps at all six
walls, zero weights, a multi-pass and a single-particle tile), computed with the kernels' own index arithmetic."""
import numpy as np
import pytest

from mfs import scenes
from oracle import mfs_oracle as O

TB = 8                 # tile edge of the tile-sorted scatters, cells (csrc/mfs_particles.hip kTB)
TABLE = 128            # entries of a workgroup's tile table in the sort (kTileTab); a workgroup is 256 consecutive particles


@pytest.fixture(scope="module")
def sc():
    return scenes.particle_stress_scene_3d()


def _t(sc):
    """(x32 - bound_min) / cell_size per particle and axis as the kernels form it: float32 difference, float64 quotient"""
    x32 = sc["px"].astype(np.float32)
    return (x32 - sc["bound_min"]).astype(np.float64) / sc["cell_size"]


def _tiles(sc):
    N = np.array(sc["gres"])
    cell = np.floor(_t(sc)).astype(np.int64).clip(0, N - 1)
    nt = (N + TB - 1) // TB
    return ((cell[:, 0] // TB) * nt[1] + cell[:, 1] // TB) * nt[2] + cell[:, 2] // TB, int(np.prod(nt))


def test_grid_is_awkward(sc):
    gres = sc["gres"]
    assert all(g % TB for g in gres) and len(set(gres)) == 3
    assert _tiles(sc)[1] >= 512
    cs = sc["cell_size"]
    assert cs.dtype == np.float64 and len({float(c) for c in cs}) == 3
    assert sc["bound_min"].dtype == np.float32 and sc["bound_size"].dtype == np.float32
    assert (sc["bound_min"] == np.asarray([-0.3, 0.0, -0.3], np.float32)).all()      # the notebook's BOUND_MIN


def test_default_path_is_the_tiled_one(sc):
    import notebook_kernels as K
    P = len(sc["px"])
    assert K.TILE_MIN_PARTICLES <= P <= 400000
    for k in ("pm", "pv", "pcx", "pcy", "pcz"):
        assert len(sc[k]) == P
    again = scenes.particle_stress_scene_3d()
    assert all(np.array_equal(sc[k], again[k]) for k in ("px", "pm", "pv", "pcx"))      # seeded


def test_order_is_shuffled_beyond_the_sort_table(sc):
    tile, _ = _tiles(sc)
    P = len(tile)
    distinct = [len(np.unique(tile[a:a + 256])) for a in range(0, P, 256)]
    assert max(distinct) > TABLE
    assert np.mean(np.array(distinct[:-1]) > TABLE) > 0.9           # the overflow is the normal case, not one workgroup


def test_all_six_walls_clamp(sc):
    t, N = _t(sc), np.array(sc["gres"])
    for a in range(3):
        for bias in (0.0, 0.5):                                      # face-centred and cell-centred samples of p2g / g2p
            gi = np.floor(t[:, a] - bias).astype(np.int64)
            assert (gi < 0).any() and (gi + 1 > N[a] - 1).any(), (a, bias)
        c = np.floor(t[:, a]).astype(np.int64)                       # level set: cells c - 2 .. c + 2
        assert (c + 2 > N[a] - 1).any() and (c + 1 > N[a] - 1).any() and (c - 2 < 0).any(), a
        v = np.floor(2 * t[:, a]).astype(np.int64)                   # volume: nodes of the doubled grid, 2 N + 1 of them
        assert (v < 0).any() and (v + 1 > 2 * N[a]).any(), a
        out_lo, out_hi = t[:, a] < 0, t[:, a] > N[a]
        assert out_lo.sum() >= 100 and out_hi.sum() >= 100, a
        assert t[:, a].min() >= -2.001 and t[:, a].max() <= N[a] + 2.001, a
        assert (t[:, a] < -1).any() and (t[:, a] > N[a] + 1).any(), a


def test_exact_positions(sc):
    t, N = _t(sc), np.array(sc["gres"])
    x32 = sc["px"].astype(np.float32)
    assert (x32 == sc["bound_min"]).all(axis=1).any()                 # the corner itself
    for a in range(3):
        assert (t[:, a] == 0.0).sum() >= 2, a                         # on the low wall
        assert (t[:, a] == float(N[a])).any(), a                      # on the high wall
    on_face = (t == np.round(t)) & (t > 0) & (t < N)
    assert on_face.any()                                              # an interior cell face: weight exactly 0 / 1
    assert ((sc["px"] == x32).all(axis=1) & on_face.any(axis=1)).sum() >= 8           # and float32 arrays keep them


def test_tile_occupancy(sc):
    tile, nt = _tiles(sc)
    count = np.bincount(tile, minlength=nt)
    assert (count == 0).sum() >= 50
    assert count.max() > 256
    assert (count == 1).sum() >= 1 and count[tile[sc["lone"]]] == 1


def test_signs_and_decades(sc):
    for k in ("pm", "pv"):
        a = np.abs(sc[k])
        assert (sc[k] < 0).any() and (sc[k] > 0).any() and a.max() / a.min() >= 500, k
    # ... so that the sum of absolute contributions and the absolute sum differ, and the last face plane gets nothing
    gres, cs = sc["gres"], sc["cell_size"]
    gm, gv, st = np.zeros((gres[0] + 1,) + gres[1:]), np.zeros((gres[0] + 1,) + gres[1:]), {}
    O.nb_p2g_scatter(sc["px"], sc["pm"], sc["pv"], sc["pcx"], gm, gv, sc["bound_min"], gres, (0, .5, .5), cs, 0, stats=st)
    hit = st["K"] > 0
    assert (st["S_m"][hit] > 1.5 * np.abs(gm[hit])).mean() > 0.25
    assert (gm[hit] <= 0).any() and (gm[hit] > 0).any()
    assert not hit[-1].any() and hit[-2].any()
