"""SurfaceLoads without a GPU: the argument checks of wl_surface_sample / wl_surface_totals, the identities the reference
(tests/surface_ref.py) must obey on every test shape, the .vtp writer, and the refusal of a body that is no mesh.

Also the cases and the DERIVED bounds that tests/test_surface_gpu.py shares.  With EPS = 2^-52, L the largest coordinate met
(xi or x space) and td = tol_d(L) = 64 EPS L the Float64 bound of test_mesh_cpu on a position computed two ways:
  * an edge vector is off by <= 2 td per component, so |dS| <= 2 sqrt(3) td e_max and the unit normal by
    err_n = 16 td / alt_min (alt = 2 |S| / e_max the triangle's smallest altitude; 8 sqrt(3) < 16);
  * the sample point x_c + delta n is off by pos = td + delta err_n per component;
  * one interp of a field stored as T with |field| <= F: the stored corners are within ulp_T(F) of the exact field (storage),
    and the 8-term double sum adds <= 16 EPS F: e_s(T, F) = ulp_T(F) + 16 EPS F;
  * tau_i = -nu sum_j (G_ij + G_ji) n_j reads 12 samples with |n_j| <= 1.
"""
import ctypes as C
import os
import sys
import types
import xml.etree.ElementTree as ET

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_shapes as MS  # noqa: E402
import surface_ref as SR  # noqa: E402
from test_mesh_cpu import SHAPES, tol_d  # noqa: E402

from waterlily_amd import _lib, body as B, surface  # noqa: E402
from waterlily_amd.mesh import MeshBody  # noqa: E402

EPS = 2.0 ** -52
DIMS = (40, 32, 24)                                   # the issue's grid: three different extents, so a stride mix-up shows
CENTRE = np.array([23.37, 24.91, 21.19])              # test_mesh_gpu's off-lattice centre of the identity poses
MAP_CENTRE = np.array([23.37, 24.91, 21.13])          # off_lattice_map's centre of rotation
# "stated": the issue's centre and map.  In a 24-cell z extent that centre leaves 0.81 cells between a body and the last plane a
# sample at delta = 1.5 may read, so the shapes are scaled to 0.08 of SHAPES' sizes (the issue leaves the sizes open and asks
# that the body stay inside the domain).  "mid": SHAPES' own sizes with the same off-lattice fractions moved by whole cells to
# the middle of the domain, so that the samples spread over hundreds of cells.
PLACES = {"stated": (np.zeros(3), 0.08), "mid": (np.array([-4.0, -9.0, -10.0]), 1.0)}
G_LIN, C_LIN = np.array([0.75, -0.5, 0.3]), 2.0
M_LIN = np.array([[0.11, -0.23, 0.07], [0.31, 0.05, -0.13], [-0.17, 0.19, -0.29]])
CU_LIN = np.array([1.0, -0.4, 0.25])
NU = 0.37


def ulp(T, v):
    return float(np.spacing(np.abs(np.asarray(v)).astype(T)).astype(np.float64))


def place_map(place, scale=1.3, w=0.05):
    """off_lattice_map(1.3) of test_mesh_cpu, its centre moved by the placement's whole cells"""
    return B.scaled(B.rotation3d(tuple(MAP_CENTRE + PLACES[place][0]), (1.0, 2.0, 0.5), w, th0=0.4), scale)


def body_of(shape, posed, place):
    v, t = SHAPES[shape]()
    shift, k = PLACES[place]
    return MeshBody(v * k, t, map=place_map(place)) if posed else MeshBody(v * k + CENTRE + shift, t)


def pose_of(mb, posed):
    """(pose tuple for surface_ref or None, time)"""
    return (mb.coeffs(0.8), 0.8) if posed else (None, 0.0)


def scales(mb, geo):
    """(L, td, err_n, e_max) of a case"""
    L = max(np.abs(geo["xv"]).max(), np.abs(mb.vertices).max()) + 4.0
    xv = geo["xv"]
    e = np.stack([np.linalg.norm(xv[:, (k + 1) % 3] - xv[:, k], axis=1) for k in range(3)], 1).max(1)
    td = tol_d(L)
    return L, td, 16 * td / float(np.min(2 * geo["area"] / e)), float(e.max())


def e_sample(T, F):
    return ulp(T, F) + 16 * EPS * F


def tol_linear(T, mb, geo, delta, p, u):
    """bounds of the exact identities on linear fields: (tau per entry, Fp per component, Fv per component)"""
    L, td, err_n, _ = scales(mb, geo)
    Fp, Fu = float(np.abs(p).max()), float(np.abs(u).max())
    msym = float(np.abs(M_LIN + M_LIN.T).max())
    tau = NU * (12 * e_sample(T, Fu) + 6 * msym * err_n)
    sa = float(geo["area"].sum())
    nt = len(geo["area"])
    pos = td + delta * err_n
    ep = e_sample(T, Fp) + np.abs(G_LIN).sum() * pos
    dS = err_n * sa                                                  # sum |dS| <= err_n sum |S|
    fp = sa * ep + Fp * dS + nt * EPS * Fp * sa
    fv = sa * tau + NU * 3 * msym * (dS + nt * EPS * sa)
    return tau, fp, fv


# ---------------------------------------------------------------------------------------------------- argument checks
def _grid3():
    g = _lib.Grid()
    g.D = 3
    g.n[:] = [8, 8, 8]
    g.s[:] = [1, 8, 64]
    g.sc = 512
    return g


def test_entry_points_reject_bad_calls_before_the_device():
    L = _lib.lib()
    mb = MeshBody(*MS.cube((4.0, 4.0, 4.0), 2.0))
    h = mb.handle(4.0)
    pose, _ = mb.pose(0.0)
    g = _grid3()
    buf = (C.c_double * 64)()
    f = C.cast(buf, C.c_void_p)
    call = lambda **k: L.wl_surface_sample(k.get("t", _lib.WL_F64), C.byref(k.get("g", g)), f, f, k.get("h", h), k.get("pose", C.byref(pose)),
                                           k.get("delta", 1.0), k.get("nu", 0.1), k.get("rows", f), None, None, 1.0, 0)
    for kw, msg in (({"h": None}, b"null mesh or pose"), ({"pose": None}, b"null mesh or pose"), ({"rows": None}, b"null output rows"),
                    ({"delta": -0.5}, b"delta must be finite and >= 0"), ({"delta": float("nan")}, b"delta must be finite"),
                    ({"delta": float("inf")}, b"delta must be finite"), ({"nu": float("nan")}, b"nu must be finite"),
                    ({"nu": float("-inf")}, b"nu must be finite")):
        assert call(**kw) == _lib.WL_E_ARG and msg in L.wl_last_error(), (kw, L.wl_last_error())
    g2 = _lib.Grid()
    g2.D = 2
    g2.n[:] = [8, 8, 1]
    g2.s[:] = [1, 8, 64]
    g2.sc = 64
    assert call(g=g2) == _lib.WL_E_ARG and b"D == 3" in L.wl_last_error()
    shear, _ = mb.pose(0.0)
    shear.identity_map = 0
    shear.A[1] = 0.5
    assert call(pose=C.byref(shear)) == _lib.WL_E_ARG and b"similarity" in L.wl_last_error()
    x0 = _lib.d3((0.0, 0.0, 0.0))
    for args in ((None, f, 4, x0, f), (f, None, 4, x0, f), (f, f, 4, None, f), (f, f, 4, x0, None)):
        assert L.wl_surface_totals(*args) == _lib.WL_E_ARG and b"null rows, geometry, x0 or output" in L.wl_last_error()
    assert L.wl_surface_totals(f, f, 0, x0, f) == _lib.WL_E_ARG and b"nt must be positive" in L.wl_last_error()


# ---------------------------------------------------------------------------------------------------- the reference's identities
@pytest.mark.parametrize("posed", [False, True], ids=["identity", "posed"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_reference_obeys_the_identities(shape, posed):
    """Linear fields: Fp = g Vol_x at delta = 0 (divergence theorem, exact for centroid quadrature on flat triangles), per
    triangle tau = -nu (M + M^T) n at any delta, Fv = 0 (a closed surface: sum S = 0)."""
    v, t = SHAPES[shape]()
    mb = MeshBody(v, t, map=B.scaled(B.rotation3d(tuple(MAP_CENTRE), (1.0, 2.0, 0.5), 0.05, th0=0.4), 1.3)) if posed else MeshBody(v + CENTRE, t)
    pose, _ = pose_of(mb, posed)
    geo = SR.geometry(mb.vertices, mb.triangles, pose)
    p, u = SR.linear_fields((50, 46, 42), G_LIN, C_LIN, M_LIN, CU_LIN, np.float64)
    s = 1.0 if pose is None else pose[5]
    want_tau = -NU * geo["n"] @ (M_LIN + M_LIN.T).T
    for delta in (0.0, 1.5):
        pt, tau, G = SR.sample(geo, p, u, delta, NU)
        assert np.all(np.isfinite(pt)) and np.all(np.isfinite(tau))
        ttau, tfp, tfv = tol_linear(np.float64, mb, geo, delta, p, u)
        assert np.abs(G - M_LIN).max() <= 2 * e_sample(np.float64, np.abs(u).max())
        assert np.abs(tau - want_tau).max() <= ttau
        Fp, Fv, _, _ = SR.totals(geo, pt, tau, (0.0, 0.0, 0.0))
        assert np.abs(Fv).max() <= tfv
        if delta == 0.0:
            assert np.abs(Fp - G_LIN * mb.volume / s ** 3).max() <= tfp, (Fp, G_LIN * mb.volume / s ** 3)
    # moments: a uniform pressure on a closed surface has no moment, about any point
    one = np.ones(len(geo["area"]))
    _, _, Mp, _ = SR.totals(geo, one, np.zeros((len(one), 3)), (3.0, -2.0, 7.0))
    assert np.abs(Mp).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------- the surface file
def _stub(mean):
    v, t = MS.icosphere((0.0, 0.0, 0.0), 2.0, 1)
    mb = MeshBody(v, t, map=B.scaled(B.rotation3d((5.3, 4.1, 6.2), (1.0, 2.0, 0.5), 0.05, th0=0.4), 1.3))
    rng = np.random.default_rng(8)
    nt = len(t)
    rows, geom = rng.standard_normal((nt, 4)), rng.standard_normal((nt, 9))
    return types.SimpleNamespace(body=mb, nt=nt, slab=None, time=0.8, rows=torch.from_numpy(rows), geom=torch.from_numpy(geom),
                                 mean=torch.from_numpy(rows * 0.5) if mean else None), rows, geom


def _array(node):
    a = np.array(node.text.split(), dtype=np.float64 if node.get("type") == "Float64" else np.int64)
    nc = int(node.get("NumberOfComponents"))
    return a if nc == 1 else a.reshape(-1, nc)


@pytest.mark.parametrize("mean", [False, True])
def test_write_vtp_round_trips(tmp_path, mean):
    sl, rows, geom = _stub(mean)
    path = tmp_path / "s.vtp"
    surface.write_vtp(path, sl)
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "PolyData"
    piece = root.find("PolyData/Piece")
    nt, nv = len(sl.body.triangles), len(sl.body.vertices)
    assert int(piece.get("NumberOfPolys")) == nt and int(piece.get("NumberOfPoints")) == nv
    pts = _array(piece.find("Points/DataArray"))
    A, b, _, _, Ai, _ = sl.body.coeffs(0.8)
    assert np.array_equal(pts, (sl.body.vertices - b) @ Ai.T)                   # %.17g round-trips a double
    assert np.abs(pts @ A.T + b - sl.body.vertices).max() < 1e-13
    polys = {d.get("Name"): _array(d) for d in piece.findall("Polys/DataArray")}
    assert np.array_equal(polys["connectivity"].reshape(-1, 3), sl.body.triangles)
    assert np.array_equal(polys["offsets"], 3 * np.arange(1, nt + 1))
    cd = {d.get("Name"): _array(d) for d in piece.findall("CellData/DataArray")}
    want = {"p": rows[:, 0], "traction": rows[:, 1:4], "area_vector": geom[:, 3:6], "body_velocity": geom[:, 6:9]}
    if mean:
        want.update(mean_p=0.5 * rows[:, 0], mean_traction=0.5 * rows[:, 1:4])
    assert sorted(cd) == sorted(want)
    for k, w in want.items():
        assert np.array_equal(cd[k], w), k


def test_surfaceloads_refuses_a_body_that_is_no_mesh():
    for body in (B.NoBody(), B.Sphere((8.0, 8.0, 8.0), 3.0, 3), None):
        with pytest.raises(TypeError, match="must be a MeshBody"):
            surface.SurfaceLoads(types.SimpleNamespace(body=body, eps=1, flow=None))
    assert surface.columns(None) == ("Fp_x", "Fp_y", "Fp_z", "Fv_x", "Fv_y", "Fv_z", "Mp_x", "Mp_y", "Mp_z", "Mv_x", "Mv_y", "Mv_z")


# ---------------------------------------------------------------------------------------------------- shared with the GPU tests
def make_sim(mb, T, padded=True, t=0.0, dims=DIMS, slab=None):
    """what SurfaceLoads reads of a Simulation -- flow, body, eps -- around a bare Flow whose clock shows t (no Poisson solver)"""
    from waterlily_amd import sim as S
    flow = S.Flow(dims, (0.0, 0.0, 0.0), nu=NU, T=T, padded=padded, slab=slab)
    if t:
        flow.dt = [float(t), flow.dt[0]]
    return types.SimpleNamespace(flow=flow, body=mb, eps=1, slab=slab)


def upload_global(a, host):
    """copy the planes of the undecomposed host array that the (possibly z-slab) device field holds, halo planes included"""
    from waterlily_amd import sim as S
    sl = getattr(a, "_wl_slab", None)
    if sl is None:
        S.upload(a, host)
        return
    h = np.zeros(tuple(a.shape), dtype=host.dtype)
    for l in range(h.shape[2]):
        if 0 <= sl.kz0 + l < host.shape[2]:
            h[:, :, l] = host[:, :, sl.kz0 + l]
    S.upload(a, h)


def random_fields(seed, T, dims=DIMS):
    rng = np.random.default_rng(seed)
    Ng = tuple(n + 2 for n in dims)
    return np.asfortranarray(rng.standard_normal(Ng).astype(T)), np.asfortranarray(rng.standard_normal(Ng + (3,)).astype(T))


def neighbour_diff(a):
    """largest difference of two neighbouring entries along any grid direction (per component)"""
    return float(max(np.abs(np.diff(a.astype(np.float64), axis=d)).max() for d in range(3)))


def tol_sampled(mb, geo, delta, p, u):
    """bounds of device against surface_ref on the SAME stored fields (no storage term): the positions differ by pos per
    component, the interpolant moves by at most the neighbour difference per cell and direction, the 8-term sums by 16 EPS F:
    (p, tau per entry, centroid, S, Vb per entry)"""
    L, td, err_n, emax = scales(mb, geo)
    pos = td + delta * err_n
    Fp, Fu = float(np.abs(p).max()), float(np.abs(u).max())
    e2 = lambda a, F: 3 * pos * neighbour_diff(a) + 16 * EPS * F
    tp = e2(p, Fp)
    ttau = NU * (12 * e2(u, Fu) + 6 * 2 * Fu * err_n)
    if mb.amap is None:
        tV = 0.0
    else:
        _, _, dA, db, Ai, _ = mb.coeffs(0.8)
        tV = 64 * EPS * np.abs(Ai).sum(1).max() * (np.abs(dA).sum(1).max() * L + np.abs(db).max())
    return tp, ttau, td, 4 * td * emax, tV
