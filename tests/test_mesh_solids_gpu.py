"""sdf.union_mesh_grid / sdf.project_mesh on the MI355X against their numpy restatement (tests/meshsdf_numpy.py) on the SAME
float32 volumes, which are made on the host: this tests the two kernels, not the build.

Bounds.  The kernels and the restatement evaluate the same float64 expressions in the same order (no contraction on the
device), so they differ by a few roundings of quantities of the size of the coordinates: TOL64 = 64 eps64 * scale, scale
the largest coordinate / distance in play.  Float32 outputs: one float32 spacing at the value on top of that."""
import numpy as np
import pytest
import torch

import meshsdf_numpy as M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
EPS64, EPS32 = float(np.finfo(np.float64).eps), float(np.finfo(np.float32).eps)
TOL64 = 64 * EPS64 * 2.0                                     # coordinates and distances stay below 2
TORCH = {"f32": torch.float32, "f64": torch.float64}

RES, BMIN, CS, BIAS = (21, 26, 19), (-0.5, 0.0, -0.5), (0.05, 0.05, 0.05), (0.0, 0.0, 0.0)
SPHERE_C, SPHERE_R = np.array([-0.05, 0.45, 0.0]), 0.25
MARK = 7.0                                                    # what vel holds where nothing is written


def host_volume(kind, h, pad=2):
    """(vol float32, origin, spacing, radius): the exact signed distance of a box / a sphere sampled on a lattice"""
    half = np.array([0.25, 0.3, 0.2]) if kind == "box" else np.full(3, 0.3)
    cells = np.ceil(2 * half / h - 1e-9).astype(int)
    shape = tuple(int(c) + 1 + 2 * pad for c in cells)
    origin = tuple(float(x) for x in -(cells / 2 + pad) * h)
    nodes = M.lattice_nodes(shape, origin, h)
    phi = M.box_sdf(nodes, 2 * half) if kind == "box" else np.linalg.norm(nodes, axis=-1) - 0.3
    return phi.astype(np.float32), origin, h, float(np.linalg.norm(half))


@pytest.fixture(scope="module")
def scene():
    """two overlapping posed bodies (rotation about a skew axis plus a translation) and their host-side description"""
    import solver.sdf3D as sdf
    from mfs.meshsdf import MeshSDF
    vols = [host_volume("box", 0.05), host_volume("sphere", 0.06)]
    bodies = [sdf.MeshBody(MeshSDF(torch.as_tensor(v, device=DEV), o, h, r), center=c, axis=a, angle=g, velocity=u)
              for (v, o, h, r), c, a, g, u in zip(vols, [(0.1, 0.52, -0.05), (0.3, 0.6, 0.05)], [(1, 2, 3), (-1, 0.5, 2)],
                                                  [37, 110], [(0.3, -0.2, 0.1), (-0.1, 0.4, 0.0)])]
    rb = sdf.mesh_rb(bodies)
    rows = N(rb)
    assert rows.shape == (2, 10, 4) and rows[0, 0, 0] == 6 and rows[0, 0, 1] == vols[0][3]
    pos = M.grid_positions(RES, BMIN, CS, BIAS)
    sd0 = np.linalg.norm(pos - SPHERE_C, axis=-1) - SPHERE_R
    for a in (pos, sd0):
        a.setflags(write=False)
    return dict(sdf=sdf, bodies=bodies, rb=rb, rows=rows, volumes=[(v, o, h) for v, o, h, _ in vols], pos=pos, sd0=sd0)


def close(got, ref, dtype, what):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    tol = TOL64 + (np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) if dtype == "f32" else 0.0)
    err = np.abs(got - ref)
    print(f"{what} [{dtype}]: largest deviation {err.max():.3e}, bound {np.max(tol):.3e}")
    assert (err <= tol).all(), what


@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("sd_dt, vel_dt", [("f64", "f64"), ("f32", "f32"), ("f32", "f64")])
def test_union_mesh_grid_matches_the_restatement(scene, sd_dt, vel_dt, with_w):
    sdf, rows, pos = scene["sdf"], scene["rows"], scene["pos"]
    sd = torch.as_tensor(scene["sd0"].copy(), device=DEV).to(TORCH[sd_dt]).contiguous()
    vel = torch.full(RES + (3,), MARK, dtype=TORCH[vel_dt], device=DEV)
    w = np.array([[0.5, -1.0, 2.0], [1.5, 0.25, -0.75]]) if with_w else None
    ref_sd, ref_vel, winner = M.union(rows, scene["volumes"], N(sd), N(vel), pos, w)
    sdf.union_mesh_grid(scene["rb"], scene["bodies"], sd, vel, BMIN, CS, BIAS,
                        rb_w=None if w is None else torch.as_tensor(w, device=DEV))
    # every outcome occurs: each body wins inside itself, a body wins outside itself (zeros written), the analytic sphere
    # keeps nodes inside itself, nodes where nothing is inside, nodes outside both volumes
    inside_vol = [np.all((M.to_body(r, pos) >= np.asarray(o)) & (M.to_body(r, pos) <= np.asarray(o) + (np.array(v.shape) - 1) * h), axis=-1)
                  for r, (v, o, h) in zip(rows, scene["volumes"])]
    assert all(((winner == i) & (ref_sd <= 0)).sum() > 20 for i in (0, 1))
    assert ((winner >= 0) & (ref_sd > 0)).sum() > 100 and ((winner < 0) & (scene["sd0"] <= 0)).sum() > 20
    assert ((winner < 0) & (scene["sd0"] > 0)).sum() > 100 and (~inside_vol[0] & ~inside_vol[1]).sum() > 1000
    assert ((winner >= 0) & ~inside_vol[0] & ~inside_vol[1]).sum() > 0            # won from outside the volumes: clamp + distance
    close(N(sd), ref_sd, sd_dt, "sd")
    close(N(vel), ref_vel, vel_dt, "vel")
    got_vel = N(vel)
    assert (got_vel[winner < 0] == MARK).all()                                      # not written where no body wins
    assert (got_vel[(winner >= 0) & (ref_sd > 0)] == 0).all()                       # zeros where a body wins outside itself
    if with_w:
        assert np.abs(ref_vel[(winner == 0) & (ref_sd <= 0)] - rows[0, 9, :3]).max() > 0.05   # the rotation is in vel


def test_union_order_matters_only_through_the_comparison(scene):
    """the bodies in the other order give the same level set"""
    sdf = scene["sdf"]
    a = torch.as_tensor(scene["sd0"].copy(), device=DEV)
    b = a.clone()
    va, vb = (torch.zeros(RES + (3,), dtype=torch.float64, device=DEV) for _ in range(2))
    sdf.union_mesh_grid(scene["rb"], scene["bodies"], a, va, BMIN, CS, BIAS)
    sdf.union_mesh_grid(scene["rb"].flip(0).contiguous(), scene["bodies"][::-1], b, vb, BMIN, CS, BIAS)
    assert torch.equal(a, b)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_project_mesh_matches_the_restatement(scene, dt):
    sdf, rows = scene["sdf"], scene["rows"]
    x0 = np.random.default_rng(5).uniform((-0.3, 0.1, -0.45), (0.7, 1.0, 0.45), (6000, 3)).astype(np.dtype("float" + dt[1:]))
    ref, moved = M.project(rows, scene["volumes"], x0)
    x = torch.as_tensor(x0, device=DEV).clone()
    sdf.project_mesh(scene["rb"], scene["bodies"], x)
    got = N(x)
    assert got.dtype == x0.dtype and 500 < moved.sum() < 5500
    both = (M.sample(*scene["volumes"][0], M.to_body(rows[0], x0.astype(np.float64))) < 0) & \
           (M.sample(*scene["volumes"][1], M.to_body(rows[1], x0.astype(np.float64))) < 0)
    assert both.sum() > 10                                                          # the overlap is populated
    close(got, ref, dt, "positions")
    assert (got[~moved].view(np.uint8) == x0[~moved].view(np.uint8)).all()          # d >= 0: bitwise unchanged
    assert (got[moved] != x0[moved]).any(axis=1).all()


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_where_projected_particles_end_up_in_the_box_and_sphere_volumes(scene, dt, which):
    """Without the restatement of the projection: each body alone.  A particle with sampled d0 < 0 moves by |d0| (asserted);
    along that straight move the trilinear field f changes by |d0| times an average of grad f . u, and component k of
    grad f in a cell is a convex combination of the cell's k-edge differences / h, so the volume's own values bound the
    change (meshsdf_numpy.straight_move_interval): d1 in [d0 + lo, d0 + hi].  Float32 positions: x' is rounded, which moves
    the sample by at most |grad f| sqrt(3) 2^-24 max|x| (twice: before and after are both read rounded).  In the box volume's
    linear face regions the interval is a few roundings wide -- the issue's bound; next to a crease it is a fraction of
    |d0|, which is what one gradient step can promise there."""
    sdf, row, (vol, origin, h) = scene["sdf"], scene["rows"][which], scene["volumes"][which]
    x0 = np.random.default_rng(5).uniform((-0.3, 0.1, -0.45), (0.7, 1.0, 0.45), (6000, 3)).astype(np.dtype("float" + dt[1:]))
    x = torch.as_tensor(x0, device=DEV).clone()
    sdf.project_mesh(scene["rb"][which:which + 1].contiguous(), [scene["bodies"][which]], x)
    x1 = N(x)
    b0, b1 = M.to_body(row, x0.astype(np.float64)), M.to_body(row, x1.astype(np.float64))
    d0, d1 = M.sample(vol, origin, h, b0), M.sample(vol, origin, h, b1)
    ins = d0 < 0
    assert ins.sum() > 700 and (x1[~ins].view(np.uint8) == x0[~ins].view(np.uint8)).all()
    rnd = np.sqrt(3) * 2.0 ** -24 * float(np.abs(x1).max()) if dt == "f32" else 0.0
    np.testing.assert_allclose(np.linalg.norm(b1[ins] - b0[ins], axis=1), -d0[ins], rtol=0, atol=TOL64 + 2 * rnd)
    lo, hi, G = M.straight_move_interval(vol, np.asarray(origin), h, b0[ins], b1[ins])
    pad = TOL64 + 2 * G * rnd
    assert (d1[ins] >= d0[ins] + lo - pad).all() and (d1[ins] <= d0[ins] + hi + pad).all()
    c = np.maximum(np.abs(d0[ins] + lo), np.abs(d0[ins] + hi)) / np.abs(d0[ins])       # |d1| <= c |d0| (+ pad)
    tight = c < 1e-5
    print(f"body {which} [{dt}]: {ins.sum()} inside; c < 1e-5 for {tight.sum()}, < 0.5 for {(c < 0.5).sum()}; largest |d1| "
          f"where tight {np.abs(d1[ins][tight]).max() if tight.any() else 0:.3e}, overall {np.abs(d1[ins]).max():.3e}")
    if which == 0:                                    # the box: most particles sit under a face, where the field is linear
        assert tight.sum() > 400 and np.abs(d1[ins][tight]).max() <= 1e-5 * np.abs(d0[ins]).max() + pad.max()
    else:                                             # the sphere: curved everywhere, one step still takes most of d0 away
        assert (c < 0.5).sum() > 600


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_projection_lands_on_the_surface_of_a_planar_volume(dt):
    """Volume: the float32 samples of the plane field L(x) = n.x (|n| = 1, oblique).  Each sample is off by at most
    delta = 2^-24 max|vol|, and so is the interpolant; the gradient's direction is off by theta <= 2 sqrt(3) delta / h.  A
    particle with sampled d0 = L(x) + e0 moves to x' = x - d0 n': L(x') = -e0 + d0 (1 - n.n') and the sample there adds e1:
    |d(x')| <= 2 delta + |d0| theta^2 -- plus, for float32 positions, the rounding of x', sqrt(3) 2^-24 max|x|, and the
    float64 roundings TOL64.  The bound is made from the volume's values below."""
    import solver.sdf3D as sdf
    from mfs.meshsdf import MeshSDF
    h, n = 0.05, np.array([2.0, -1.0, 2.0]) / 3.0
    shape, origin = (12, 13, 11), (-0.275, -0.3, -0.25)
    vol = (M.lattice_nodes(shape, origin, h) @ n).astype(np.float32)
    body = sdf.MeshBody(MeshSDF(torch.as_tensor(vol, device=DEV), origin, h, 0.5), center=(0.2, 0.4, -0.1), axis=(3, 1, -2), angle=64)
    rb = sdf.mesh_rb([body])
    row = N(rb)[0]
    xb = np.random.default_rng(7).uniform(-0.08, 0.08, (4000, 3))                   # the move stays inside the volume
    x0 = (xb @ row[5:8, :3].T + row[1:4, 3]).astype(np.dtype("float" + dt[1:]))
    d0 = M.sample(vol, origin, h, M.to_body(row, x0.astype(np.float64)))
    x = torch.as_tensor(x0, device=DEV).clone()
    sdf.project_mesh(rb, [body], x)
    got = N(x)
    d1 = M.sample(vol, origin, h, M.to_body(row, got.astype(np.float64)))
    delta = 2.0 ** -24 * float(np.abs(vol).max())
    theta = 2 * np.sqrt(3) * delta / h
    bound = 2 * delta + np.abs(d0).max() * theta ** 2 + TOL64 + (np.sqrt(3) * 2.0 ** -24 * np.abs(got).max() if dt == "f32" else 0.0)
    inside = d0 < 0
    print(f"[{dt}] {inside.sum()} inside; largest |d| after {np.abs(d1[inside]).max():.3e}, bound {bound:.3e}")
    assert 1000 < inside.sum() < 3000 and (np.abs(d1[inside]) <= bound).all()
    assert (got[~inside].view(np.uint8) == x0[~inside].view(np.uint8)).all()


def test_vanishing_gradient_falls_back_to_central_differences_or_stays():
    import solver.sdf3D as sdf
    from mfs.meshsdf import MeshSDF
    prof = np.array([0.3, 0.1, -0.1, -0.2, -0.2, 0.0, 0.2, 0.4], np.float32)          # a plateau between nodes 3 and 4 of axis 0
    plateau = np.broadcast_to(prof[:, None, None], (8, 6, 6)).copy()
    flat = np.full((6, 6, 6), -1.0, np.float32)
    h = 0.1
    bodies = [sdf.MeshBody(MeshSDF(torch.as_tensor(v, device=DEV), (0.0, 0.0, 0.0), h, 1.0), center=c)
              for v, c in ((plateau, (0, 0, 0)), (flat, (2.0, 0, 0)))]
    rb = sdf.mesh_rb(bodies)
    x0 = np.array([[0.33, 0.25, 0.25], [0.36, 0.21, 0.3], [2.25, 0.25, 0.25], [0.62, 0.2, 0.2]])
    ref, moved = M.project(N(rb), [(plateau, (0, 0, 0), h), (flat, (0, 0, 0), h)], x0)
    assert list(moved) == [True, True, False, False] and (ref[:2, 0] != x0[:2, 0]).all() and (ref[:, 1:] == x0[:, 1:]).all()
    x = torch.as_tensor(x0, device=DEV).clone()
    sdf.project_mesh(rb, bodies, x)
    close(N(x), ref, "f64", "plateau")
    assert (N(x)[2:] == x0[2:]).all()


def test_a_box_mesh_body_against_the_analytic_box():
    """through the whole chain: build -> MeshBody -> union_mesh_grid on an empty table, against generate_rb's 'box' at the
    same pose through evaluate_grid.  Compared where the analytic closest point lies on a face more than two volume
    spacings from any edge (and the node lies inside the volume): the field is linear there and trilinear sampling exact,
    so what is left is the build's distance error, within 4 E32 (E32 as in tests/test_meshsdf_gpu.py, on this lattice)."""
    import solver.sdf3D as sdf
    from mfs import meshsdf
    from mfs.surface import Mesh
    size, h, pad = (0.5, 0.6, 0.4), 0.05, 3
    v, f = M.box(size)
    msdf = meshsdf.build(Mesh(torch.as_tensor(v, device=DEV), torch.as_tensor(f, device=DEV)), h, padding=pad)
    nodes = M.lattice_nodes(tuple(msdf.phi.shape), msdf.origin, h)
    e32 = float(np.abs(M.distance(nodes, v, f, np.float32).astype(np.float64) - M.distance(nodes, v, f)).max())
    pose = dict(center=(0.1, 0.52, -0.05), axis=(1, 2, 3), angle=37)
    body = sdf.MeshBody(msdf, **pose)
    rb = sdf.mesh_rb([body])
    empty = torch.zeros((0, 10, 4), dtype=torch.float64, device=DEV)
    sd, vel = torch.empty(RES, dtype=torch.float64, device=DEV), torch.empty(RES + (3,), dtype=torch.float64, device=DEV)
    sdf.evaluate_grid(empty, sd, vel, BMIN, CS, BIAS)
    assert bool((sd == 100).all())
    sdf.union_mesh_grid(rb, [body], sd, vel, BMIN, CS, BIAS)
    rb_a, _ = sdf.generate_rb(None, {}, "b", ["box", *size], device=DEV, center=list(pose["center"]), axis=list(pose["axis"]),
                              angle=pose["angle"])
    sd_a, vel_a = torch.empty_like(sd), torch.empty_like(vel)
    sdf.evaluate_grid(rb_a, sd_a, vel_a, BMIN, CS, BIAS)
    q = np.abs(M.to_body(N(rb)[0], M.grid_positions(RES, BMIN, CS, BIAS))) - np.asarray(size) / 2
    k = q.argmax(axis=-1)
    qk = np.take_along_axis(q, k[..., None], axis=-1)[..., 0]
    others = np.where(np.arange(3) == k[..., None], -np.inf, q).max(axis=-1)
    on_face = (others < -2 * h) & (others < qk - 2 * np.sqrt(3) * h) & (np.abs(qk) <= (pad - 1) * h)
    err = np.abs(N(sd) - N(sd_a))[on_face]
    print(f"{on_face.sum()} nodes on faces, {int((N(sd_a)[on_face] < 0).sum())} of them inside; largest deviation {err.max():.3e}, "
          f"E32 {e32:.3e}, bound {4 * e32:.3e}")
    assert on_face.sum() > 200 and (N(sd_a)[on_face] < 0).sum() > 20 and err.max() <= 4 * e32


def test_more_than_sixteen_bodies_and_bad_arguments_are_refused(scene):
    from mfs import _lib
    sdf = scene["sdf"]
    sd, vel = torch.zeros(RES, dtype=torch.float64, device=DEV), torch.zeros(RES + (3,), dtype=torch.float64, device=DEV)
    many = [scene["bodies"][0]] * 17
    with pytest.raises(ValueError, match="at most 16"):
        sdf.union_mesh_grid(sdf.mesh_rb(many), many, sd, vel, BMIN, CS, BIAS)
    lib = _lib.load()
    st = lib.mfs_mesh_project3d(None, 17, None, None, None, None, None, 1, 0, None)
    assert st == -1 and b"at most 16" in lib.mfs_last_error()
    st = lib.mfs_mesh_project3d(None, 1, None, None, None, None, None, 1, 0, None)
    assert st == -1 and b"null" in lib.mfs_last_error()
