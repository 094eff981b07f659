"""csrc/mfs_volume.h is the one sampler of posed level-set volumes: seeding, rendering and the mesh solids inline it.
tests/c_abi/volume_sample_check.cpp (stand-alone C++17, the header alone, no HIP) runs pose_to_body and volume_sample on the
host; here their outputs are held bit for bit against the numpy restatements the GPU tests rest on -- seed_numpy.to_body
and seed_numpy.sample for the point and the value (float32 and float64 volume), meshsdf_numpy.sample for the gradient --
and lattice_split against / and %.  Built with the host compiler, contraction off, under AddressSanitizer and UBSan (a
load outside a volume would be reported); no GPU."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import meshsdf_numpy as M
import seed_numpy as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, ORIGIN, H = (6, 5, 7), (-0.25, 0.5, -0.375), 0.125                       # dyadic: node positions are exact


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("volume_sample") / "volume_sample_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "python-fluid-simulation_amd", "csrc"),
           os.path.join(REPO, "tests", "c_abi", "volume_sample_check.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.fixture(scope="module")
def volumes():
    rng = np.random.default_rng(11)
    v64 = rng.standard_normal(N)                                            # both signs
    return v64.astype(np.float32), v64


def box_points(rng):
    """body-frame points on exact coordinates: every node (the last of each axis among them), the faces and corners of
    the box, points beyond it along one, two and three axes on either side, and cell interiors on dyadic fractions"""
    lo = np.asarray(ORIGIN)
    hi = lo + (np.asarray(N) - 1) * H
    nodes = S.nodes(N, ORIGIN, H).reshape(-1, 3)
    per_axis = [[lo[k] - 0.75, lo[k] - H / 4, lo[k], lo[k] + 1.25 * H, hi[k] - H / 8, hi[k], hi[k] + H / 2, hi[k] + 3.0]
                for k in range(3)]
    around = np.array(list(itertools.product(*per_axis)))                   # 512: in / on / out per axis, all combinations
    inner = lo + rng.integers(0, 8 * (np.asarray(N) - 1) + 1, size=(500, 3)) * (H / 8)
    return np.concatenate([nodes, around, inner])


def run(exe, tmp_path, volumes, R, T, x):
    """the program's rows for world points x: (xb, value32, value32 with all outputs, value64, grad32, inside, cell)"""
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(np.array(list(N) + [len(x)], np.int64).tobytes())
        f.write(np.array(list(ORIGIN) + [H] + list(np.reshape(R, -1)) + list(T), np.float64).tobytes())
        f.write(np.ascontiguousarray(volumes[0]).tobytes() + np.ascontiguousarray(volumes[1]).tobytes())
        f.write(np.ascontiguousarray(x, np.float64).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(x) and all(len(row) == 13 for row in rows)
    f64 = np.array([[int(w, 16) for w in row[:9]] for row in rows], np.uint64).view(np.float64)
    ints = np.array([[int(w) for w in row[9:]] for row in rows], np.int64)
    return f64[:, 0:3], f64[:, 3], f64[:, 4], f64[:, 5], f64[:, 6:9], ints[:, 0], ints[:, 1:4]


def check(exe, tmp_path, volumes, R, T, x):
    v32, v64 = volumes
    xb, plain32, full32, val64, grad, inside, cell = run(exe, tmp_path, volumes, R, T, x)
    want_xb = S.to_body(np.asarray(R, np.float64), np.asarray(T, np.float64), x)
    assert xb.tobytes() == np.ascontiguousarray(want_xb).tobytes()
    assert plain32.tobytes() == S.sample(v32, ORIGIN, H, want_xb).tobytes()
    assert val64.tobytes() == S.sample(v64, ORIGIN, H, want_xb).tobytes()
    want_value, want_grad = M.sample(v32, ORIGIN, H, want_xb, gradient=True)
    assert full32.tobytes() == want_value.tobytes() == plain32.tobytes()    # asking for more outputs changes no bit
    assert grad.tobytes() == np.ascontiguousarray(want_grad).tobytes()
    t = (want_xb - np.asarray(ORIGIN)) / np.float64(H)
    top = np.asarray(N, np.float64) - 1
    np.testing.assert_array_equal(inside, ((t >= 0) & (t <= top)).all(axis=1))
    np.testing.assert_array_equal(cell, np.minimum(np.floor(np.clip(t, 0, top)).astype(np.int64), np.asarray(N) - 2))
    return want_xb, inside


def test_the_sampler_matches_the_numpy_restatements_bit_for_bit_on_exact_points(exe, tmp_path, volumes):
    """a quarter turn about axis 2 and a dyadic translation: pose_to_body is exact, so the points land ON nodes, faces and
    corners in the body frame"""
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    T = np.array([0.5, -1.25, 2.0])
    want = box_points(np.random.default_rng(5))
    x = want @ R.T + T                                                      # x = R xb + T, exact
    xb, inside = check(exe, tmp_path, volumes, R, T, x)
    np.testing.assert_array_equal(xb, want)
    nodes = int(np.prod(N))
    assert inside[:nodes].all() and 0 < inside[nodes:nodes + 512].sum() < 512
    # at a node the sample is the node
    _, plain32, _, val64, _, _, _ = run(exe, tmp_path, volumes, R, T, x[:nodes])
    np.testing.assert_array_equal(plain32, volumes[0].reshape(-1).astype(np.float64))
    np.testing.assert_array_equal(val64, volumes[1].reshape(-1))


def test_the_sampler_matches_the_numpy_restatements_bit_for_bit_under_a_general_pose(exe, tmp_path, volumes):
    rng = np.random.default_rng(6)
    R = S.rotation((1, 2, 0.5), 33)
    T = np.array([0.02, 0.31, -0.01])
    lo = np.asarray(ORIGIN)
    size = (np.asarray(N) - 1) * H
    body = lo + (rng.random((3000, 3)) * 1.8 - 0.4) * size                  # inside, and outside along 1, 2 and 3 axes
    xb, inside = check(exe, tmp_path, volumes, R, T, body @ R.T + T)
    out_axes = ((xb < lo) | (xb > lo + size)).sum(axis=1)
    assert all((out_axes == k).sum() > 50 for k in range(4)) and inside.sum() == (out_axes == 0).sum()


def test_lattice_split_agrees_with_division_on_every_point_of_three_lattices(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines == ["lattice_split 7 x 5 x 11: 385 points, 0 wrong", "lattice_split 3 x 130 x 3: 1170 points, 0 wrong",
                     "lattice_split 2 x 3 x 300: 1800 points, 0 wrong", "ok"], r.stdout
