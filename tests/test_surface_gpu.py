"""mfs.surface.isosurface / contour and the simulations' surface() on the MI355X against the numpy restatement of the
contract (tests/surface_numpy.py).

Tolerances are derived, not measured.  Counts and (canonicalised) faces are equal: topology is integer work.  Both sides
compute vertex positions in fp64 and differ by FMA contraction (~1e-16 relative) before the GPU's one rounding to fp32, so
positions, compared in order, agree within one fp32 spacing at the largest coordinate.  Normals take two roundings
(normalise, store): 4 * 2^-24.  The 130^3 case is too slow for the Python loops and is checked by invariants only."""
import numpy as np
import pytest
import torch

import surface_numpy as S
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = lambda t: t.detach().cpu().numpy()  # noqa: E731
NORMAL_TOL = 4 * 2.0 ** -24


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV).to(dtype or torch.float64).contiguous()


def check_mesh(mesh, ref, normals=False):
    Vr, Fr, Nr = ref
    V, F = N(mesh.vertices), N(mesh.faces)
    assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
    assert V.shape == Vr.shape and F.shape == Fr.shape, (V.shape, Vr.shape, F.shape, Fr.shape)
    np.testing.assert_array_equal(S.canonical_faces(F), S.canonical_faces(Fr))
    if len(Vr):
        tol = float(np.spacing(np.float32(np.abs(Vr).max())))
        err = np.abs(V.astype(np.float64) - Vr).max()
        print("vertex error", err, "tolerance", tol)
        assert err <= tol
    if normals:
        Ng = N(mesh.normals).astype(np.float64)
        assert Ng.shape == Nr.shape
        print("normal error", np.abs(Ng - Nr).max(), "tolerance", NORMAL_TOL)
        assert np.abs(Ng - Nr).max() <= NORMAL_TOL
        assert np.abs(np.linalg.norm(Ng, axis=1) - 1.0).max() <= NORMAL_TOL
    else:
        assert mesh.normals is None
    return V, F


def check_contour(c, ref):
    Vr, Sr = ref
    V, Sg = N(c.vertices), N(c.segments)
    assert c.vertices.dtype == torch.float32 and c.segments.dtype == torch.int32
    assert V.shape == Vr.shape and Sg.shape == Sr.shape, (V.shape, Vr.shape, Sg.shape, Sr.shape)
    np.testing.assert_array_equal(S.canonical_segments(Sg), S.canonical_segments(Sr))
    if len(Vr):
        assert np.abs(V.astype(np.float64) - Vr).max() <= float(np.spacing(np.float32(np.abs(Vr).max())))
    return V, Sg


@pytest.fixture(scope="module")
def surf():
    from mfs import surface
    return surface


# ---------------------------------------------------------------- against the oracle, 3D ----
@pytest.fixture(scope="module")
def refs():
    """name -> (case, {dtype: oracle mesh}); computed once, never modified"""
    out = {}
    for name in ("sphere", "octahedron"):
        c = getattr(S, "case_" + name)()
        per = {}
        for dt in (np.float64, np.float32):
            per[dt] = S.isosurface(c["phi"].astype(dt), 0.0, c["origin"], c["spacing"], normals=(name == "sphere" and dt == np.float64))
        out[name] = (c, per)
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["sphere", "octahedron"])
def test_matches_oracle(surf, refs, name, dtype):
    c, per = refs[name]
    phi = dev(c["phi"].astype(dtype), torch.float32 if dtype == np.float32 else torch.float64)
    mesh = surf.isosurface(phi, 0.0, c["origin"], c["spacing"])
    V, F = check_mesh(mesh, per[dtype][:2] + (None,))
    assert S.is_closed_manifold(F, len(V)) and S.euler(V, F) == c["chi"] and S.signed_volume(V, F) > 0
    if name == "octahedron":
        # fp32 vertex rounding is <= 1e-6 absolute over a surface of area ~62: a few 1e-6 of the volume
        assert abs(S.signed_volume(V, F) - 36.0) <= 1e-5 * 36.0


def test_normals_on_the_sphere(surf, refs):
    c, per = refs["sphere"]
    mesh = surf.isosurface(dev(c["phi"]), 0.0, c["origin"], c["spacing"], normals=True)
    check_mesh(mesh, per[np.float64], normals=True)


@pytest.mark.parametrize("shape", [(2, 2, 2), (2, 5, 3)])
def test_minimum_sizes(surf, shape):
    rng = np.random.default_rng(7)
    phi = rng.standard_normal(shape)
    for closed in (False, True):
        kw = dict(closed=closed, outside=4.0) if closed else {}
        mesh = surf.isosurface(dev(phi), 0.1, (1.0, -2.0, 0.5), (0.5, 0.25, 2.0), **kw)
        V, F = check_mesh(mesh, S.isosurface(phi, 0.1, (1.0, -2.0, 0.5), (0.5, 0.25, 2.0), **kw))
        assert len(F) > 0
        if closed:
            assert S.is_closed_manifold(F, len(V))


def test_several_scan_blocks(surf):
    """47 520 nodes = 47 tiles of 1024: the prefixes cross block and tile borders; chi is the sum of the parts"""
    c = S.case_union()
    mesh = surf.isosurface(dev(c["phi"]), 0.0, c["origin"], c["spacing"])
    V, F = check_mesh(mesh, S.isosurface(c["phi"], 0.0, c["origin"], c["spacing"]))
    assert S.is_closed_manifold(F, len(V)) and S.all_vertices_used(V, F)
    assert S.euler(V, F) == 0 + 2 + 2


def test_closed_all_inside_block(surf):
    phi = np.full((6, 5, 7), -1.0)
    mesh = surf.isosurface(dev(phi), closed=True, outside=1.0)
    V, F = check_mesh(mesh, S.isosurface(phi, closed=True, outside=1.0))
    assert S.is_closed_manifold(F, len(V)) and S.euler(V, F) == 2 and S.signed_volume(V, F) > 0


def test_closed_sphere_on_the_array_face(surf):
    sp = np.array([0.5, 0.4, 0.3])
    X = S.grid_points((9, 12, 15), 0.0, sp)
    phi = S.sphere_sdf(X, (0.0, 2.3, 2.0), 1.6)                       # centre ON the face i = 0
    ref_open = S.isosurface(phi, 0.0, 0.0, sp)
    assert not S.is_closed_manifold(ref_open[1], len(ref_open[0]))   # open: cut by the border
    mesh = surf.isosurface(dev(phi), 0.0, 0.0, sp, closed=True, outside=3.0, normals=True)
    V, F = check_mesh(mesh, S.isosurface(phi, 0.0, 0.0, sp, closed=True, outside=3.0, normals=True), normals=True)
    assert S.is_closed_manifold(F, len(V)) and S.euler(V, F) == 2 and S.signed_volume(V, F) > 0
    check_mesh(surf.isosurface(dev(phi), 0.0, 0.0, sp), ref_open)


def test_empty_results(surf):
    for phi, kw in ((np.full((4, 3, 5), 2.0), {}), (np.full((4, 3, 5), 2.0), dict(closed=True, outside=5.0)),
                    (np.full((4, 3, 5), -2.0), {})):
        mesh = surf.isosurface(dev(phi), normals=True, **kw)
        assert tuple(mesh.vertices.shape) == (0, 3) and tuple(mesh.faces.shape) == (0, 3) and tuple(mesh.normals.shape) == (0, 3)
        assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32 and mesh.vertices.is_cuda
    c = surf.contour(dev(np.full((4, 3), 2.0)))
    assert tuple(c.vertices.shape) == (0, 2) and tuple(c.segments.shape) == (0, 2)


def test_nan_is_never_inside_and_level_is_outside(surf):
    phi = np.full((3, 3, 3), 1.0)
    phi[1, 1, 1] = -1.0
    phi[0, 1, 1] = np.nan
    phi[1, 0, 1] = 0.0                                                # equal to the level: outside
    mesh = surf.isosurface(dev(phi))
    F = N(mesh.faces)
    Fr = S.isosurface(phi)[1]
    np.testing.assert_array_equal(S.canonical_faces(F), S.canonical_faces(Fr))
    assert S.is_closed_manifold(F, mesh.vertices.shape[0]) and S.euler(mesh.vertices.shape[0], F) == 2


# --------------------------------------------------------- large case: invariants only ----
def test_large_sphere_invariants(surf):
    n, R = 130, 50.0
    ax = torch.arange(n, dtype=torch.float64, device=DEV) - 64.3
    phi = torch.sqrt(ax[:, None, None] ** 2 + (ax[None, :, None] + 0.2) ** 2 + (ax[None, None, :] - 0.4) ** 2) - R
    a = surf.isosurface(phi.contiguous(), normals=True)
    b = surf.isosurface(phi.contiguous(), normals=True)
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.normals, b.normals)
    V, F = N(a.vertices).astype(np.float64), N(a.faces)
    assert 0 <= F.min() and F.max() < len(V)
    assert S.is_closed_manifold(F, len(V)) and S.all_vertices_used(V, F)
    assert S.euler(V, F) == 2
    analytic = 4.0 / 3.0 * np.pi * R ** 3
    err = abs(S.signed_volume(V - V.mean(0), F) - analytic) / analytic
    print("V", len(V), "F", len(F), "relative volume error", err, "cap", 9 / (8 * R * R))
    assert err <= 9 * 1.0 ** 2 / (8 * R ** 2)                         # chord-sag cap: 4.5e-4


# ------------------------------------------------------------------------- errors ----
def test_argument_errors(surf):
    good = torch.zeros((4, 4, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError, match="GPU"):
        surf.isosurface(torch.zeros((4, 4, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        surf.isosurface(torch.zeros((4, 4, 8), dtype=torch.float64, device=DEV)[:, :, ::2])
    with pytest.raises(TypeError, match="dtype"):
        surf.isosurface(torch.zeros((4, 4, 4), dtype=torch.float16, device=DEV))
    with pytest.raises(TypeError, match="dtype"):
        surf.isosurface(torch.zeros((4, 4, 4), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=">= 2"):
        surf.isosurface(torch.zeros((4, 1, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="3D"):
        surf.isosurface(torch.zeros((4, 4), dtype=torch.float64, device=DEV))
    for level in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="level"):
            surf.isosurface(good, level)
    for sp in (0.0, -1.0, (1.0, 0.0, 1.0)):
        with pytest.raises(ValueError, match="spacing"):
            surf.isosurface(good, spacing=sp)
    with pytest.raises(ValueError, match="outside"):
        surf.isosurface(good, closed=True)
    with pytest.raises(ValueError, match="outside"):
        surf.isosurface(good, 0.5, closed=True, outside=0.5)
    g2 = torch.zeros((4, 4), dtype=torch.float64, device=DEV)
    with pytest.raises(TypeError, match="GPU"):
        surf.contour(torch.zeros((4, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match=">= 2"):
        surf.contour(torch.zeros((1, 4), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="spacing"):
        surf.contour(g2, spacing=(1.0, -1.0))
    with pytest.raises(ValueError, match="outside"):
        surf.contour(g2, closed=True, outside=-1.0)


def test_int32_guard_from_the_shape_alone(surf):
    assert surf.check_sizes((1290, 1290, 1290)) == 1290 ** 3            # 2.1467e9: fits
    with pytest.raises(ValueError, match="32-bit"):
        surf.check_sizes((1290, 1290, 1290), closed=True)               # 1292^3 = 2.1567e9 does not
    with pytest.raises(ValueError, match="32-bit"):
        surf.check_sizes((2048, 2048, 512))
    with pytest.raises(ValueError, match="32-bit"):
        surf.check_sizes((65536, 32768))


# --------------------------------------------------------------------- simulation, 3D ----
def build(g, **kw):
    """tests/test_timestep_gpu.py::build"""
    import notebook_sim as NSIM
    import solver.sdf3D as sdf
    gres = tuple(int(v) for v in g["gres"])
    gdx = float(g["gdx"])
    size = np.array(gres) * gdx
    rb_d, rb_map = sdf.generate_rb(None, {}, 'cube', ['box', size[0] - 2 * gdx, size[1] - 2 * gdx, size[2] - 2 * gdx], flip=True,
                                   center=[0, size[1] / 2, 0], axis=[0., 1, 0], angle=0, device=DEV)
    rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, 'ramp', ['box', 0.45, 0.05, 0.8], flip=False, center=[-0.12, 0.2, 0],
                                   axis=[0., 0, 1], angle=-35)
    sim = NSIM.NotebookSimulation(gres, gdx, [-0.3, 0, -0.3], rb_d, g["px0"], float(g["pdx"]), rho=float(g["rho"]),
                                  mu=float(g["mu"]), dt=float(g["dt"]), device=DEV, **kw)
    sim.particle.v.copy_(torch.as_tensor(g["pv0"], device=DEV))
    return sim


def test_simulation_surfaces_3d():
    sim = build(golden("step_a_12x16x12"))
    sim.step()
    cs = np.asarray(sim.grid.cell_size, np.float64)
    bmin = np.asarray(sim.grid.bound_min, np.float64)
    lphi = N(sim.fluid_levelset.phi)
    assert lphi.shape == (12, 16, 12) and (lphi < 0).any()
    ref = S.isosurface(lphi, 0.0, bmin + cs / 2, cs, closed=True, outside=3 * sim.GDX)
    V, F = check_mesh(sim.surface("liquid"), ref)
    assert len(F) > 0 and S.is_closed_manifold(F, len(V)) and S.signed_volume(V, F) > 0
    sphi = N(sim.solid_levelset.phi)
    assert sphi.shape == (25, 33, 25)
    ref = S.isosurface(sphi, 0.0, bmin, cs / 2, normals=True)
    V, F = check_mesh(sim.surface("solid", normals=True), ref, normals=True)
    assert len(F) > 0
    with pytest.raises(ValueError, match="which"):
        sim.surface("gas")


def test_multi_gpu_classes_raise():
    import notebook_sim as NSIM
    for cls in (NSIM.SlabNotebookSimulation, NSIM.ShardedNotebookSimulation):
        with pytest.raises(NotImplementedError):
            cls.surface(None)


# ----------------------------------------------------------------------------- 2D ----
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", ["circle", "diamond"])
def test_contour_matches_oracle(surf, name, dtype):
    c = getattr(S, "case_" + name)()
    phi = c["phi"].astype(dtype)
    con = surf.contour(dev(phi, torch.float32 if dtype == np.float32 else torch.float64), 0.0, c["origin"], c["spacing"])
    V, Sg = check_contour(con, S.contour(phi, 0.0, c["origin"], c["spacing"]))
    assert S.is_closed_contour(Sg, len(V))
    lp = S.loops(Sg, len(V))
    assert len(lp) == 1 and S.shoelace(V, lp[0]) > 0
    if name == "diamond":
        assert abs(S.signed_area(V.astype(np.float64), Sg) - 18.0) <= 1e-5 * 18.0


def test_contour_discs_and_annulus(surf):
    c = S.case_discs()
    con = surf.contour(dev(c["phi"]), 0.0, c["origin"], c["spacing"])
    V, Sg = check_contour(con, S.contour(c["phi"], 0.0, c["origin"], c["spacing"]))
    assert S.is_closed_contour(Sg, len(V))
    lps = S.loops(Sg, len(V))
    assert len(lps) == 5
    # every loop is counter-clockwise for ITS inside: phi just left of each segment's midpoint is negative
    X = V.astype(np.float64)
    mid = 0.5 * (X[Sg[:, 0]] + X[Sg[:, 1]])
    d = X[Sg[:, 1]] - X[Sg[:, 0]]
    keep = np.linalg.norm(d, axis=1) > 1e-3
    left = mid[keep] + 0.05 * np.stack([-d[keep, 1], d[keep, 0]], axis=1) / np.linalg.norm(d[keep], axis=1, keepdims=True)
    ring = np.abs(S.sphere_sdf(left, (200.3, 120.6), 50.0)) - 14.0
    phi_left = np.minimum.reduce([S.sphere_sdf(left, (50.2, 50.7), 30.0), S.sphere_sdf(left, (60.4, 150.1), 25.0),
                                  S.sphere_sdf(left, (200.3, 120.6), 18.0), ring])
    assert (phi_left < 0).mean() > 0.99
    areas = sorted(S.shoelace(X, lp) for lp in lps)
    assert areas[0] < 0 and all(a > 0 for a in areas[1:])              # only the annulus' hole runs clockwise


def test_contour_closed_disc_cut_by_the_border(surf):
    sp = np.array([0.2, 0.3])
    X = S.grid_points((21, 17), (-1.0, 0.5), sp)
    phi = S.sphere_sdf(X, (-1.0, 3.0), 1.7)                            # centre on the border i = 0
    ref_open = S.contour(phi, 0.0, (-1.0, 0.5), sp)
    assert not S.is_closed_contour(ref_open[1], len(ref_open[0]))
    check_contour(surf.contour(dev(phi), 0.0, (-1.0, 0.5), sp), ref_open)
    con = surf.contour(dev(phi), 0.0, (-1.0, 0.5), sp, closed=True, outside=2.0)
    V, Sg = check_contour(con, S.contour(phi, 0.0, (-1.0, 0.5), sp, closed=True, outside=2.0))
    assert S.is_closed_contour(Sg, len(V))
    lp = S.loops(Sg, len(V))
    assert len(lp) == 1 and S.shoelace(V, lp[0]) > 0


def test_simulation_surface_2d():
    import notebook_sim2d as NSIM
    import solver.sdf2D as sdf
    from timestep2d_scene import dam_break
    sc = dam_break((24, 32))
    rb_d, rb_map = None, {}
    for b in sc["bodies"]:
        rb_d, rb_map = sdf.generate_rb(rb_d, rb_map, b["name"], b["rbparam"], flip=b["flip"], center=b["center"], angle=b["angle"],
                                       device=DEV)
    sim = NSIM.NotebookSimulation2D(sc["gres"], sc["gdx"], sc["bound_min"], rb_d, sc["px"], sc["pdx"], mu=sc["mu"], device=DEV)
    sim.particle.v.copy_(torch.as_tensor(sc["pv"], device=DEV))
    sim.step()
    cs = np.asarray(sim.grid.cell_size, np.float64)
    bmin = np.asarray(sim.grid.bound_min, np.float64)
    lphi = N(sim.fluid_levelset.phi)
    ref = S.contour(lphi, 0.0, bmin + cs / 2, cs, closed=True, outside=3 * sim.GDX)
    V, Sg = check_contour(sim.surface("liquid"), ref)
    assert len(Sg) > 0 and S.is_closed_contour(Sg, len(V)) and S.signed_area(V.astype(np.float64), Sg) > 0
    check_contour(sim.surface("solid"), S.contour(N(sim.solid_levelset.phi), 0.0, bmin, cs / 2))
