"""MeshBody without a GPU: STL io, validation, pseudonormals, maps, the ABI's argument checks, the checker's own pins,
and the library's bin structure (through its host evaluator) against the brute-force checker."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
import mesh_shapes as MS  # noqa: E402

from waterlily_amd import _lib, body as B, mesh  # noqa: E402
from waterlily_amd.mesh import MeshBody  # noqa: E402

EPS52 = 2.0 ** -52


def tol_d(L):
    """Float64 bound on a distance computed two ways from operands of size <= L (a few dozen operations)"""
    return 64 * EPS52 * L


def off_lattice_map(scale=1.3, w=0.05):
    return B.scaled(B.rotation3d((23.37, 24.91, 21.13), (1.0, 2.0, 0.5), w, th0=0.4), scale)


# ---------------------------------------------------------------------------------------------------- STL
def test_stl_fixtures_round_trip_and_weld(tmp_path):
    v, t = MS.cube((1.0, 2.0, 3.0), 2.0)
    for path in (MS.CUBE_STL_BIN, MS.CUBE_STL_ASCII):
        vr, tr = mesh.read_stl(path)
        assert vr.shape == (8, 3) and tr.shape == (12, 3)                      # 36 corners welded to 8 vertices
        assert np.array_equal(np.sort(vr.view("f8,f8,f8"), axis=0), np.sort(v.view("f8,f8,f8"), axis=0))
        assert np.array_equal(vr[tr], v[t])                                     # same triangles, same corner order
        assert MeshBody.from_stl(path).volume == pytest.approx(8.0, abs=1e-12)
    v2, t2 = MS.icosphere((0.3, -0.2, 0.1), 1.7, 2)
    p = tmp_path / "ico.stl"
    mesh.write_stl(p, v2, t2)
    vr, tr = mesh.read_stl(p)
    assert len(vr) == len(v2) and np.array_equal(vr[tr], v2[t2].astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match="neither a binary STL"):
        (tmp_path / "bad.stl").write_bytes(b"solid nothing\nendsolid\n" + b" " * 80)
        mesh.read_stl(tmp_path / "bad.stl")


def test_fixtures_are_what_the_helper_writes(tmp_path, monkeypatch):
    monkeypatch.setattr(MS, "CUBE_STL_BIN", str(tmp_path / "b.stl"))
    monkeypatch.setattr(MS, "CUBE_STL_ASCII", str(tmp_path / "a.stl"))
    MS.write_fixtures()
    import mesh_shapes
    import os
    assert open(tmp_path / "b.stl", "rb").read() == open(os.path.join(mesh_shapes.GOLDEN, "mesh_cube_bin.stl"), "rb").read()
    assert open(tmp_path / "a.stl").read() == open(os.path.join(mesh_shapes.GOLDEN, "mesh_cube_ascii.stl")).read()


# ---------------------------------------------------------------------------------------------------- validation
def test_validation_names_the_defect():
    v, t = MS.cube()
    with pytest.raises(ValueError, match="not closed"):
        MeshBody(v, t[:-1])
    bad = t.copy()
    bad[0] = bad[0][::-1]
    with pytest.raises(ValueError, match="inconsistently oriented"):
        MeshBody(v, bad)
    with pytest.raises(ValueError, match="inside-out.*flip=True"):
        MeshBody(v, t[:, ::-1])
    assert MeshBody(v, t[:, ::-1], flip=True).volume == pytest.approx(1.0)
    with pytest.raises(ValueError, match="out of range"):
        MeshBody(v[:-1], t)
    vn = v.copy()
    vn[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        MeshBody(vn, t)
    # a zero-area triangle: split edge 0-1 of the cube at its midpoint and add the flat triangle (0, m, 1) twice oriented
    vd = np.vstack([v, (v[0] + v[1]) / 2])
    td = np.vstack([t, [[0, 8, 1]], [[1, 8, 0]]])
    with pytest.raises(ValueError, match="degenerate"):
        MeshBody(vd, td)
    with pytest.raises(TypeError, match="AffineMap"):
        MeshBody(v, t, map=lambda x, tt: x)
    with pytest.raises(TypeError, match="concatenate"):
        MeshBody(v, t) + MeshBody(v, t)
    with pytest.raises(TypeError):
        B.Bodies([MeshBody(v, t), B.Sphere(0.0, 1.0, 3)])


def test_scale_and_volume_and_centroid():
    v, t = MS.lprism((3.0, 4.0, 5.0), a=2.0, height=3.0)
    m = MeshBody(v, t, scale=2.0)
    assert m.volume == pytest.approx(3 * 4.0 * 3.0 * 8.0, rel=1e-13)             # three a x a squares x height, x scale^3
    v2, t2 = MS.torus((0, 0, 0), 10.0, 3.0, 96, 48)
    assert MeshBody(v2, t2).volume == pytest.approx(2 * np.pi ** 2 * 10 * 9, rel=5e-3)
    assert np.allclose(MeshBody(*MS.cube((1.0, 2.0, 3.0), 2.0)).centroid, (1.0, 2.0, 3.0), atol=1e-13)


# ---------------------------------------------------------------------------------------------------- maps
def test_rotation3d_derivative_inverse_and_closure():
    import torch
    m = B.rotation3d((23.37, 24.91, 21.13), (1.0, 2.0, 0.5), 0.37, th0=0.4)
    t, h = 1.7, 1e-5
    A, b, dA, db = m.coeffs(t)
    Ap, bp, _, _ = m.coeffs(t + h)
    Am, bm, _, _ = m.coeffs(t - h)
    assert np.max(np.abs((Ap - Am) / (2 * h) - dA)) < 1e-9 and np.max(np.abs((bp - bm) / (2 * h) - db)) < 1e-7
    assert np.max(np.abs(A @ m.inverse(t) - np.eye(3))) < 1e-15
    assert np.max(np.abs(A @ A.T - np.eye(3))) < 1e-15 and np.linalg.det(A) == pytest.approx(1.0)
    k = np.array([1.0, 2.0, 0.5]) / np.linalg.norm([1.0, 2.0, 0.5])
    assert np.allclose(A @ k, k, atol=1e-15)                                   # the axis is fixed
    x = np.random.default_rng(0).normal(size=(3, 7)) * 10
    assert np.allclose(m(torch.from_numpy(x), torch.tensor(t, dtype=torch.float64)).numpy(), A @ x + b[:, None], atol=1e-12)
    # a quarter turn about z carries the body's +x axis to +y: xi = R (x - c) maps x = c + e_y onto e_x
    q = B.rotation3d(0.0, (0, 0, 1), 1.0, th0=np.pi / 2)
    assert np.allclose(q.coeffs(0.0)[0] @ np.array([0.0, 1.0, 0.0]), (1.0, 0.0, 0.0), atol=1e-15)
    # it is just another AffineMap: a parametric 3-D body takes it
    d = B.Sphere(0.0, 4.0, 3, map=m).native_desc(t, 3)
    assert np.allclose(np.array(d[0].A[:]).reshape(3, 3), A) and np.allclose(np.array(d[0].Ainv[:]).reshape(3, 3), A.T)


def test_similarity_check():
    v, t = MS.cube((0, 0, 0), 6.0)
    mb = MeshBody(v, t, map=off_lattice_map(1.3))
    A, b, dA, db, Ai, s = mb.coeffs(0.8)
    assert s == pytest.approx(1.3, rel=1e-14) and np.max(np.abs(A @ Ai - np.eye(3))) < 1e-15
    shear = B.AffineMap(lambda tt: (np.array([[1.0, 0.2, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), np.zeros(3), np.zeros((3, 3)), np.zeros(3)))
    with pytest.raises(ValueError, match="not a similarity"):
        MeshBody(v, t, map=shear).coeffs(0.0)
    stretch = B.AffineMap(lambda tt: (np.diag([1.0, 1.0, 1.1]), np.zeros(3), np.zeros((3, 3)), np.zeros(3)))
    with pytest.raises(ValueError, match="not a similarity"):
        MeshBody(v, t, map=stretch).pose(0.0)
    # the library checks again on its own
    L = _lib.lib()
    p = _lib.MeshPose()
    p.A[:] = [1, 0.2, 0, 0, 1, 0, 0, 0, 1]
    h = MeshBody(v, t).handle(4.0)
    x = np.zeros(3)
    assert L.wl_mesh_eval_host(h, C.byref(p), x.ctypes.data_as(C.c_void_p), 1, 1.0, x.ctypes.data_as(C.c_void_p), None, None) == _lib.WL_E_ARG
    assert b"not a similarity" in L.wl_last_error()


# ---------------------------------------------------------------------------------------------------- pseudonormals
def test_cube_pseudonormals_closed_form():
    v, t = MS.cube((0, 0, 0), 2.0)
    ref = mesh_ref.Ref(v, t)
    mb = MeshBody(v, t)
    pts = np.array([[0.2, -0.3, 1.5], [1.5, 1.5, 0.1], [-1.4, 0.3, -1.6], [1.5, 1.6, 1.7], [-1.5, 1.5, -1.5]])
    want = np.array([[0, 0, 1], [1, 1, 0], [-1, 0, -1], [1, 1, 1], [-1, 1, -1]], dtype=np.float64)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    q = ref.query(pts)
    assert list(q["kind"]) == [mesh_ref.FACE, mesh_ref.EDGE, mesh_ref.EDGE, mesh_ref.VERTEX, mesh_ref.VERTEX]
    assert np.max(np.abs(q["pn"] - want)) < 1e-15
    # the library: on the surface itself (|d| < 1e-9) the normal IS the pseudonormal
    on = np.array([[0.2, -0.3, 1.0], [1.0, 1.0, 0.1], [-1.0, 0.3, -1.0], [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0]])
    d, n, _ = mb.eval_host(on)
    assert np.max(np.abs(d)) < 1e-15 and np.max(np.abs(n - want)) < 1e-15


# ---------------------------------------------------------------------------------------------------- the checker's pins
def box_sdf(x, c, a):
    q = np.abs(x - c) - a / 2
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(np.max(q, axis=1), 0)


def test_mesh_ref_cube_is_the_exact_box_distance():
    c, a = np.array([3.0, -2.0, 5.0]), 4.0
    ref = mesh_ref.Ref(*MS.cube(c, a))
    rng = np.random.default_rng(1)
    x = np.vstack([c + rng.uniform(-5, 5, size=(4000, 3)),
                   c + np.array([[2, 2, 2], [3, 3, 3], [2, 2, 0], [3, 0, 3], [0, 0, 0], [1, 1, 1], [1.5, 1.5, 0], [2, 0, 0], [2.5, 2.5, 1.0]])])
    q = ref.query(x)
    assert np.max(np.abs(q["d"] - box_sdf(x, c, a))) <= 8 * EPS52 * 10


def test_mesh_ref_icosphere_within_its_faceting_bound():
    c, r = np.array([1.0, 2.0, 3.0]), 8.0
    v, t = MS.icosphere(c, r, 3)
    bound = MS.facet_bound(v, t, c, r)
    assert 0 < bound < 0.1 * r
    x = c + np.random.default_rng(2).uniform(-14, 14, size=(3000, 3))
    d = mesh_ref.Ref(v, t).query(x)["d"]
    e = d - (np.linalg.norm(x - c, axis=1) - r)
    assert np.all(e >= -1e-12) and np.max(e) <= bound + 1e-12       # an inscribed mesh: never closer than the sphere says


# ---------------------------------------------------------------------------------------------------- bins against brute force
SHAPES = {
    "cube": lambda: MS.cube((0.0, 0.0, 0.0), 9.0),
    "icosphere": lambda: MS.icosphere((0.0, 0.0, 0.0), 7.0, 2),
    "torus": lambda: MS.torus((0.0, 0.0, 0.0), 8.0, 2.6, 24, 12),
    "lprism": lambda: MS.lprism((0.0, 0.0, 0.0), 6.0, 7.0),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("posed", [False, True])
def test_library_distance_equals_brute_force(shape, posed):
    """Random points through and around the body: exact zone within tol_d of the checker (normals within tol_d/|d| off the
    medial axis), far zone the checker's sign and magnitude >= R; V exact."""
    v, t = SHAPES[shape]()
    eps, tt = 1.0, 0.8
    if posed:
        mb = MeshBody(v, t, map=off_lattice_map(1.3))
    else:
        mb = MeshBody(v + np.array([23.0, 24.0, 21.0]), t)
    ref = mesh_ref.Ref(mb.vertices, mb.triangles)
    pose = mb.coeffs(tt)
    rng = np.random.default_rng(3)
    lo, hi = mb.vertices.min(axis=0) - 7.0, mb.vertices.max(axis=0) + 7.0       # around the body in xi, carried back to x
    x = (rng.uniform(lo, hi, size=(6000, 3)) - pose[1]) @ pose[4].T
    x = np.vstack([x, np.floor(x[:2000]) + 0.5, np.floor(x[:2000]) + [0.0, 0.5, 0.5]])     # cell centres and faces as well
    d, n, V = mb.eval_host(x, t=tt, eps=eps)
    dr, nr, Vr, gap = mesh_ref.measure(ref, pose, x)
    R = mb._R / pose[5]
    assert R >= 3 + eps
    L = max(np.max(np.abs(x @ pose[0].T + pose[1])), np.max(np.abs(mb.vertices)))
    td = tol_d(L)
    exact = np.abs(dr) < R - td
    far = np.abs(dr) >= R + td
    assert exact.sum() > 1000 and far.sum() > 200 and (dr < -1).sum() > 20
    assert np.max(np.abs(d[exact] - dr[exact])) <= td
    assert np.all(np.sign(d[far]) == np.sign(dr[far])) and np.all(np.abs(d[far]) >= R - td)
    smooth = exact & (gap > 1e-9) & (np.abs(dr) > 1e-6)
    if posed:       # off the lattice the medial axis is met by accident only: at most 0.1 % of the points are left out
        assert (exact & ~smooth).sum() <= 1e-3 * exact.sum()
    assert np.max(np.abs(n[smooth] - nr[smooth]) * np.abs(dr[smooth, None])) <= td
    assert np.max(np.abs(V[exact] - Vr[exact])) <= 64 * EPS52 * max(1.0, np.max(np.abs(Vr)))
    if posed:
        assert np.max(np.abs(Vr)) > 0.1


def test_bins_are_bounded_and_info_reports_them():
    v, t = MS.icosphere((0, 0, 0), 16.0, 4)
    mb = MeshBody(v, t)
    t0 = time.perf_counter()
    mb.handle(4.0)
    assert time.perf_counter() - t0 < 20
    i = mb.info()
    assert i["nt"] == 5120 and i["nv"] == 2562 and i["bins"] > 0 and 0 < i["max_per_bin"] < i["nt"] // 8
    assert i["crossed_bins"] > 0 and i["entries"] >= i["nonempty_bins"] >= i["crossed_bins"] and i["device_bytes"] > 5120 * 240
    h0 = mb._h
    mb.handle(3.9)
    assert mb._h is h0                                                         # a smaller need keeps the handle
    mb.handle(6.0)
    assert mb._R == 6.0 * (1 + 1e-6)                                                        # a larger one rebuilds


def test_a_spinning_map_never_rebuilds_or_is_refused():
    """The scale factor of a rotating (and scaled) map is recomputed in floating point at every measure!, here and in the
    library, and wanders by an ulp: the handle built at the first time must serve every later one, and the library must
    accept it (exact radius against (2 + eps + 1) s)."""
    v, t = MS.cube((0, 0, 0), 6.0)
    rng = np.random.default_rng(7)
    x = np.zeros((1, 3))
    for case in range(40):
        m = B.rotation3d(rng.uniform(10, 30, 3), rng.normal(size=3), rng.uniform(0.01, 0.5), th0=rng.uniform(0, 6))
        if case % 2:
            m = B.scaled(m, rng.uniform(0.8, 2.5))
        mb = MeshBody(v, t, map=m)
        mb.eval_host(x, t=0.0, eps=1.0)
        h0 = mb._h.value
        for k in range(1, 200):
            mb.eval_host(x, t=0.37 * k, eps=1.0)           # WlError if the library refuses the pose
            assert mb._h.value == h0, (case, k)


# ---------------------------------------------------------------------------------------------------- ABI
def test_mesh_entry_points_validate_without_gpu():
    L = _lib.lib()
    v, t = MS.cube((0, 0, 0), 4.0)
    t = np.ascontiguousarray(t, dtype=np.int32)
    vp, tp = v.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert L.wl_mesh_create(None, vp, 8, tp, 12, 4.0) == _lib.WL_E_ARG
    assert L.wl_mesh_create(C.byref(h), None, 8, tp, 12, 4.0) == _lib.WL_E_ARG and b"null" in L.wl_last_error()
    assert L.wl_mesh_create(C.byref(h), vp, 8, tp, 0, 4.0) == _lib.WL_E_ARG and b"nt == 0" in L.wl_last_error()
    assert L.wl_mesh_create(C.byref(h), vp, 8, tp, 12, 2.5) == _lib.WL_E_ARG and b"exact_radius too small" in L.wl_last_error()
    assert L.wl_mesh_create(C.byref(h), vp, 7, tp, 12, 4.0) == _lib.WL_E_ARG and b"out of range" in L.wl_last_error()
    assert L.wl_mesh_create(C.byref(h), vp, 8, tp, 11, 4.0) == _lib.WL_E_ARG and b"not closed" in L.wl_last_error()
    bad = t.copy()
    bad[0] = bad[0][::-1]
    assert L.wl_mesh_create(C.byref(h), vp, 8, bad.ctypes.data_as(C.c_void_p), 12, 4.0) == _lib.WL_E_ARG and b"oriented" in L.wl_last_error()
    vn = v.copy()
    vn[0, 0] = np.inf
    assert L.wl_mesh_create(C.byref(h), vn.ctypes.data_as(C.c_void_p), 8, tp, 12, 4.0) == _lib.WL_E_ARG and b"finite" in L.wl_last_error()
    assert h.value is None
    assert L.wl_mesh_create(C.byref(h), vp, 8, tp, 12, 4.0) == 0 and h.value
    out = (C.c_int64 * 8)()
    assert L.wl_mesh_info(h, out) == 0 and out[0] == 12 and out[1] == 8
    assert L.wl_mesh_info(None, out) == _lib.WL_E_ARG and L.wl_mesh_info(h, None) == _lib.WL_E_ARG
    p = _lib.MeshPose()
    p.identity_map = 1
    nb = C.c_int64()
    assert L.wl_measure_rows_mesh(None, h, C.byref(p), 1.0, C.byref(nb)) == _lib.WL_E_ARG      # null flow
    assert L.wl_measure_fill_mesh(None, h, C.byref(p), 1.0, None) == _lib.WL_E_ARG
    g = _lib.Grid()
    g.D = 2
    g.n[:] = [8, 8, 1]
    g.s[:] = [1, 8, 64]
    g.sc = 64
    assert L.wl_body_nds_mesh(C.byref(g), h, C.byref(p), None, 4, None) == _lib.WL_E_ARG and b"D == 3" in L.wl_last_error()
    g.D = 3
    g.n[:] = [8, 8, 8]
    g.sc = 512
    assert L.wl_body_nds_mesh(C.byref(g), None, C.byref(p), None, 4, None) == _lib.WL_E_ARG
    assert L.wl_body_nds_mesh(C.byref(g), h, None, None, 4, None) == _lib.WL_E_ARG
    assert L.wl_body_nds_mesh(C.byref(g), h, C.byref(p), None, 4, None) == _lib.WL_E_ARG and b"null buffer" in L.wl_last_error()
    assert L.wl_mesh_destroy(h) == 0 and L.wl_mesh_destroy(None) == 0


def test_simulation_refuses_host_geometry_and_2d():
    from waterlily_amd import sim as S
    mb = MeshBody(*MS.cube((8.0, 8.0, 8.0), 4.0))

    class FakeFlow:
        D, N = 2, (18, 18)
    with pytest.raises(ValueError, match="3-D grid"):
        S.measure_flow(FakeFlow(), mb, geometry="device")
    FakeFlow.D, FakeFlow.N = 3, (18, 18, 18)
    with pytest.raises(ValueError, match='geometry="device"'):
        S.measure_flow(FakeFlow(), mb, geometry="host")
