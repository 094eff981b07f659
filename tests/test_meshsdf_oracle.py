"""The oracle of the triangle-mesh tests (tests/meshsdf_numpy.py) against closed forms, without a GPU."""
import numpy as np
import pytest

import meshsdf_numpy as M
from mfs.meshsdf import lattice
from mfs.surface import Mesh, read_obj


def test_generated_meshes_are_closed_manifolds():
    sizes = {"icosphere": 320, "box": 12, "octahedron": 8, "torus": 384, "l_prism": 20}
    for name, make in M.MESHES.items():
        v, f = make()
        assert v.dtype == np.float32 and f.dtype == np.int32 and len(f) == sizes[name]
        e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
        fwd = {tuple(x) for x in e}
        assert len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd), name     # every edge once in each direction
    v, f = M.icosphere(3)
    assert len(f) == 1280
    v2, f2 = M.with_split_triangle(v, f)
    e = np.concatenate([f2[:, [0, 1]], f2[:, [1, 2]], f2[:, [2, 0]]])
    fwd = {tuple(x) for x in e}
    assert len(f2) == 1282 and len(f2) % 256 and len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)


def test_box_distance_is_the_analytic_box_sdf():
    size = (1.0, 1.5, 0.75)
    v, f = M.box(size)
    p = np.random.default_rng(0).uniform(-1.5, 1.5, (4000, 3))
    ref = M.box_sdf(p, size)
    got = M.signed_distance(p, v, f)
    assert (ref < 0).sum() > 100
    assert np.abs(got - ref).max() <= 8 * np.finfo(np.float64).eps * 3.0


def test_icosphere_distance_lies_between_the_two_spheres():
    r = 0.8
    v, f = M.icosphere(3, r)
    theta = M.max_facet_half_angle(v, f)
    assert 0 < theta < 0.1
    rv = np.linalg.norm(v.astype(np.float64), axis=1)            # float32 vertices: r to one rounding
    p = np.random.default_rng(1).uniform(-1.3, 1.3, (3000, 3))
    d = M.signed_distance(p, v, f)
    x = np.linalg.norm(p, axis=1)
    assert (d >= x - rv.max() - 1e-12).all() and (d <= x - rv.min() * np.cos(theta) + 1e-12).all()


@pytest.mark.parametrize("name", sorted(M.MESHES))
def test_winding_number_is_0_or_1_away_from_the_surface(name):
    v, f = M.MESHES[name]()
    lo, hi = v.min(axis=0) - 0.3, v.max(axis=0) + 0.3
    p = np.random.default_rng(2).uniform(lo, hi, (3000, 3))
    far = M.distance(p, v, f) > 1e-3
    w = M.winding_number(p, v, f)[far]
    assert far.sum() > 2900 and (np.abs(w - np.round(w)) <= 1e-9).all()
    assert set(np.round(w).astype(int)) == {0, 1}


@pytest.mark.parametrize("name", sorted(M.MESHES))
def test_generated_meshes_survive_the_obj_round_trip_and_get_a_centred_lattice(name, tmp_path):
    import torch
    v, f = M.MESHES[name]()
    path = str(tmp_path / "m.obj")
    Mesh(torch.as_tensor(v), torch.as_tensor(f)).save_obj(path)
    v2, f2 = read_obj(path)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(f2, f)
    h, pad = 0.11, 2
    shape, origin = lattice(v2, h, pad)
    lo, hi = v.min(axis=0).astype(np.float64), v.max(axis=0).astype(np.float64)
    top = np.asarray(origin) + (np.asarray(shape) - 1) * h
    assert (np.asarray(origin) <= lo - pad * h + 1e-12).all() and (top >= hi + pad * h - 1e-12).all()     # padding nodes a side
    assert (np.asarray(origin) > lo - (pad + 1) * h).all()                                               # ... and no more
    np.testing.assert_allclose((np.asarray(origin) + top) / 2, (lo + hi) / 2, rtol=0, atol=1e-12)           # centred
