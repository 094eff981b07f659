"""The numpy restatement of the surface-extraction contract (tests/surface_numpy.py) on fields whose answer is known:
closed, consistently oriented meshes with the right Euler characteristic and, within the chord-sag bound, the right
volume.  No GPU: this is the checker the GPU tests compare against, checked on its own."""
import numpy as np
import pytest

import surface_numpy as S


@pytest.fixture(scope="module")
def meshes():
    out = {}
    for name in ("sphere", "torus", "two_spheres", "octahedron"):
        c = getattr(S, "case_" + name)()
        V, F, _ = S.isosurface(c["phi"], 0.0, c["origin"], c["spacing"])
        out[name] = (c, V, F)
    return out


@pytest.mark.parametrize("name", ["sphere", "torus", "two_spheres", "octahedron"])
def test_closed_oriented_and_euler(meshes, name):
    c, V, F = meshes[name]
    print(name, "V", len(V), "F", len(F), "chi", S.euler(V, F), "volume", S.signed_volume(V, F))
    assert len(F) > 0
    assert S.is_closed_manifold(F, len(V))
    assert S.all_vertices_used(V, F)
    assert S.euler(V, F) == c["chi"]
    assert S.signed_volume(V, F) > 0


def test_octahedron_volume_is_exact(meshes):
    c, V, F = meshes["octahedron"]
    assert (len(V), len(F)) == (194, 384)
    assert abs(S.signed_volume(V, F) - 36.0) <= 1e-12 * 36.0
    # a third of the vertices sit ON lattice nodes (t = 1 or t = 0): zero-area triangles are kept
    a, b, cc = V[F[:, 0]], V[F[:, 1]], V[F[:, 2]]
    assert (np.linalg.norm(np.cross(b - a, cc - a), axis=1) == 0).any()


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_volume_within_the_chord_sag_bound(meshes, name):
    """|dV| / V <= 9 h_max^2 / (8 R_min^2): a chord of length L = sqrt(3) h (the longest lattice edge) on a circle of radius
    R sags L^2 / (8 R); a shell of that thickness over a body of minimum curvature radius R is 3 sag / R of its volume"""
    c, V, F = meshes[name]
    vol = S.signed_volume(V, F)
    err = abs(vol - c["analytic"]) / c["analytic"]
    print(name, "volume", vol, "analytic", c["analytic"], "relative error", err, "cap", c["cap"])
    assert err <= c["cap"]


def test_vertex_order_is_nodes_then_slots():
    phi = np.full((2, 2, 2), 1.0)
    phi[0, 0, 0] = -1.0
    V, F, _ = S.isosurface(phi, 0.0, (10.0, 20.0, 30.0), (1.0, 2.0, 4.0))
    # node (0,0,0) owns all seven, in slot order, each at t = 1/2
    want = np.array([10.0, 20.0, 30.0]) + 0.5 * np.array(S.SLOTS3, np.float64) * np.array([1.0, 2.0, 4.0])
    np.testing.assert_allclose(V, want, rtol=0, atol=1e-15)
    assert len(F) == 6 and S.signed_volume(V - V.mean(0), F) > 0     # six corner triangles, normals away from the corner


def test_circle_is_one_closed_loop():
    c = S.case_circle()
    V, Sg = S.contour(c["phi"], 0.0, c["origin"], c["spacing"])
    assert S.is_closed_contour(Sg, len(V))
    lp = S.loops(Sg, len(V))
    assert len(lp) == 1 and len(lp[0]) == len(V)
    area = S.shoelace(V, lp[0])
    assert area > 0 and abs(area - np.pi * 0.45 ** 2) < 0.1 * np.pi * 0.45 ** 2


def test_diamond_area_is_exact():
    c = S.case_diamond()
    V, Sg = S.contour(c["phi"], 0.0, c["origin"], c["spacing"])
    assert S.is_closed_contour(Sg, len(V))
    assert abs(S.signed_area(V, Sg) - 18.0) <= 1e-12 * 18.0


def test_discs_and_annulus_loops():
    c = S.case_discs()
    V, Sg = S.contour(c["phi"], 0.0, c["origin"], c["spacing"])
    assert S.is_closed_contour(Sg, len(V))
    areas = sorted(S.shoelace(V, lp) for lp in S.loops(Sg, len(V)))
    assert len(areas) == 5 and areas[0] < 0 and all(a > 0 for a in areas[1:])      # the hole of the annulus runs clockwise


def test_closed_is_padding():
    """a block that is inside everywhere: open gives nothing, closed gives its box"""
    phi = np.full((6, 5, 7), -1.0)
    V, F, _ = S.isosurface(phi)
    assert V.shape == (0, 3) and F.shape == (0, 3)
    V, F, _ = S.isosurface(phi, closed=True, outside=1.0)
    assert S.is_closed_manifold(F, len(V)) and S.euler(V, F) == 2
    # the box reaches half a cell beyond the samples (t = 1/2 towards the virtual layer), its edges and corners cut by
    # the Kuhn diagonals: between the hull of the samples and the full box
    assert 5 * 4 * 6 < S.signed_volume(V, F) < 6 * 5 * 7
    assert V.min() == -0.5


def test_obj_writer_round_trip(tmp_path):
    import torch
    from mfs.surface import Mesh
    v = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.5, 0.0], [0.0, 0.0, 2.25]], dtype=torch.float32)
    f = torch.tensor([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=torch.int32)
    n = torch.nn.functional.normalize(v + 0.1, dim=1)
    for normals in (None, n):
        path = tmp_path / "m.obj"
        Mesh(v, f, normals).save_obj(str(path))
        rv, rn, rf = [], [], []
        for line in path.read_text().splitlines():
            tok = line.split()
            if not tok or tok[0] == "#":
                continue
            if tok[0] == "v":
                rv.append([float(x) for x in tok[1:]])
            elif tok[0] == "vn":
                rn.append([float(x) for x in tok[1:]])
            elif tok[0] == "f":
                rf.append([int(x.split("/")[0]) for x in tok[1:]])
                if normals is not None:
                    assert all(x.split("/")[2] == x.split("/")[0] for x in tok[1:])
            else:
                raise AssertionError(line)
        np.testing.assert_array_equal(np.array(rv, np.float32), v.numpy())
        np.testing.assert_array_equal(np.array(rf) - 1, f.numpy())
        if normals is None:
            assert not rn
        else:
            np.testing.assert_array_equal(np.array(rn, np.float32), n.numpy())
