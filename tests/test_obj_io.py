"""mfs.surface.read_obj / load_obj: plain-text Wavefront OBJ on the host (no GPU): every corner form, negative indices,
fan triangulation, skipped records, the two error cases, and the round trip through what Mesh.save_obj writes."""
import numpy as np
import pytest
import torch

from mfs.surface import Mesh, read_obj

V4 = "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\n"


def write(tmp_path, text):
    p = tmp_path / "m.obj"
    p.write_text(text)
    return str(p)


@pytest.mark.parametrize("face", ["f 1 2 3", "f 1/1 2/2 3/3", "f 1//1 2//2 3//3", "f 1/4/1 2/5/2 3/6/3"])
def test_every_face_form(tmp_path, face):
    v, f = read_obj(write(tmp_path, V4 + "vt 0 0\nvn 0 0 1\n" + face + "\n"))
    assert v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (4, 3)
    np.testing.assert_array_equal(f, [[0, 1, 2]])
    np.testing.assert_array_equal(v[2], [1, 1, 0])


def test_negative_indices_are_relative_to_the_vertices_read_so_far(tmp_path):
    v, f = read_obj(write(tmp_path, V4 + "f -4 -3 -2\nv 5 5 5\nf -1 -2/1 -3//2\n"))
    np.testing.assert_array_equal(f, [[0, 1, 2], [4, 3, 2]])


def test_polygons_are_fan_triangulated_with_orientation_kept(tmp_path):
    v, f = read_obj(write(tmp_path, V4 + "v -0.5 0.5 0\nf 1 2 3 4\nf 1 2 3 4 5\n"))
    np.testing.assert_array_equal(f, [[0, 1, 2], [0, 2, 3], [0, 1, 2], [0, 2, 3], [0, 3, 4]])
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    assert (np.cross(b - a, c - a)[:, 2] > 0).all()                  # both polygons are counter-clockwise about +z


def test_comments_and_unknown_records_are_skipped(tmp_path):
    text = ("# a comment\nmtllib x.mtl\no thing\n" + V4 + "vn 0 0 1\nvt 0.5 0.5\ng grp\nusemtl m\ns off\n\n"
            "f 1 2 3 # trailing comment\nl 1 2\n")
    v, f = read_obj(write(tmp_path, text))
    assert v.shape == (4, 3)
    np.testing.assert_array_equal(f, [[0, 1, 2]])


@pytest.mark.parametrize("face, line", [("f 1 2", 5), ("f 1 x 3", 5), ("f 1 2 0", 5)])
def test_a_malformed_face_names_its_line(tmp_path, face, line):
    with pytest.raises(ValueError, match=rf":{line}:"):
        read_obj(write(tmp_path, V4 + face + "\n"))


@pytest.mark.parametrize("face", ["f 1 2 5", "f 1 2 -5"])
def test_an_index_out_of_range_names_its_line(tmp_path, face):
    with pytest.raises(ValueError, match=r":6:.*out of range"):
        read_obj(write(tmp_path, V4 + "f 1 2 3\n" + face + "\n"))


@pytest.mark.parametrize("normals", [False, True])
def test_round_trip_through_save_obj(tmp_path, normals):
    """save_obj needs tensors with .detach().cpu().numpy(): CPU tensors serve; it prints %.9g, which float32 survives"""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((7, 3)).astype(np.float32)
    f = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], np.int32)
    n = rng.standard_normal((7, 3)).astype(np.float32) if normals else None
    path = str(tmp_path / "rt.obj")
    Mesh(torch.as_tensor(v), torch.as_tensor(f), None if n is None else torch.as_tensor(n)).save_obj(path)
    v2, f2 = read_obj(path)
    np.testing.assert_array_equal(v2, v)
    np.testing.assert_array_equal(f2, f)
