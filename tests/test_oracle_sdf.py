"""The rigid-body SDF restatement (oracle/mfs_oracle.py sdf_*) against goldens produced by executing the
reference's solver/sdf3D.py (tests/golden/make_goldens_sdf.py)."""
import numpy as np
import pytest

from conftest import golden, golden_names
from oracle import mfs_oracle as O


@pytest.mark.parametrize("name", golden_names("sdf_"))
def test_sdf_evaluate_and_project(name):
    g = golden(name)
    n = 600                                   # per-point Python loops: a slice is enough
    pos = g["position"][:n]
    sd, vel = np.zeros(n), np.zeros((n, 3))
    O.sdf_evaluate(g["rb_d"], sd, vel, pos)
    np.testing.assert_allclose(sd, g["sd"][:n], rtol=1e-13, atol=1e-15)
    np.testing.assert_array_equal(vel, g["vel"][:n])
    proj = pos.copy()
    O.sdf_project(g["rb_d"], proj)
    tol = 1e-15 if proj.dtype == np.float64 else 0
    np.testing.assert_allclose(proj, g["projected"][:n], rtol=0, atol=tol)
    assert (vel != 0).any() and (np.abs(proj - pos) > 1e-6).any()


@pytest.mark.parametrize("name", golden_names("sdfcyl_"))
def test_cylinders_against_the_executed_reference(name):
    """cylinder_project at any point and cylinder_eval at every point outside the height range of every cylinder of the
    scene (where the reference runs; make_goldens_sdf.py): the restatement is the executed reference to the bit."""
    g = golden(name)
    assert (g["rb_d"][:, 0, 0] // 2 == 2).sum() >= 2 and len(np.unique(g["rb_d"][:, -1, :3], axis=0)) == len(g["rb_d"])
    pos = g["position_eval"]
    sd, vel = np.zeros(len(pos)), np.ones((len(pos), 3))
    O.sdf_evaluate(g["rb_d"], sd, vel, pos)
    np.testing.assert_array_equal(sd, g["sd"])
    np.testing.assert_array_equal(vel, g["vel"])
    proj = g["position_project"].copy()
    O.sdf_project(g["rb_d"], proj)
    np.testing.assert_array_equal(proj, g["projected"])
    assert ((proj != g["position_project"]).any(axis=1)).sum() > 300
    proj32 = g["position_project_f32"].copy()
    O.sdf_project(g["rb_d"], proj32)
    assert proj32.dtype == np.float32
    np.testing.assert_array_equal(proj32, g["projected_f32"])
