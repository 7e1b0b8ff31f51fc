"""oracle/geometry.py (sdf, measure through the measured fields, nds_band) against the independent extended-precision
reference tests/xref_body.py, on the bodies of xref_body.CASES that the oracle has closed forms for:
|oracle - ref| <= ulp_T(ref)/2 + K * eps_64 * M (both evaluate in Float64 and round once to T).  From the reference's branch
distances alone every case asserts that no compared cell is nearer to a branch than its error bound; control: the body
moved by 64 K eps_T of its size fails."""
import numpy as np
import pytest

import xref_body as XB
from oracle import geometry as G

TYPES = [np.float32, np.float64]
WORST = {}
ORACLE_CASES = ["seam-3d", "seam-3d-moving", "seam-2d", "seam-2d-moving", "torus", "cylinder", "plate-2d", "composite"]


def oracle_body(name):
    dims, _, leaves = XB.CASES[name]
    out = []
    for fam, p, m, op in leaves:
        shape = {"sphere": lambda: G.Sphere(p[0], p[1]), "cylinder": lambda: G.Cylinder(p[0], p[1], p[2]),
                 "torus": lambda: G.Torus(p[0], p[1], p[2]), "plate": lambda: G.Plate(p[0], p[1])}[fam]()
        mp = None if m is None else (G.Translate(v=m[1], s0=m[2]) if m[0] == "translate" else G.Rotate2D(m[1], m[2], m[3]))
        out.append(G.Body(shape, mp))
    return out[0] if len(out) == 1 else G.Bodies(out, [l[3] for l in leaves[1:]])


def branch_margin(key, T, scale):
    """how near a branch a compared point may lie.  The band test is made on sigma rounded to T: sigma_T^2 is within
    3 ulp_T of d^2 = (2+eps)^2 = 9, so 16 eps_T * 9.  Every other branch is decided in Float64 on quantities within
    K eps_64 M of the reference, M of the order of the coordinates (`scale`): 1024 K eps_64 scale."""
    f64 = 1024 * XB.K * float(np.finfo(np.float64).eps) * scale
    return f64 + (16 * 9 * float(np.finfo(T).eps) if key == "band" else 0.0)


def assert_clear(br, T, scale, keys):
    for k in keys:
        assert float(np.min(br[k])) > branch_margin(k, T, scale), (k, float(np.min(br[k])))


def record(key, T, r):
    k = f"{key} {np.dtype(T).name}"
    WORST[k] = max(WORST.get(k, 0.0), r)
    assert r <= 1, f"{k}: |got-ref| = {r:.3g} of its bound"


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_measured_fields_and_nds_oracle_vs_xref(T, name):
    dims, times, _ = XB.CASES[name]
    D = len(dims)
    idx = XB.inside_cells(dims)
    Ng = tuple(n + 2 for n in dims)
    ob = oracle_body(name)
    for t in times:
        ref, br = XB.fields(XB.body_at(name, t), idx, 1.0, T)
        assert_clear(br, T, max(Ng), ("band", "tie", "fast", "clamp", "plate"))
        assert not np.isnan(ref["mu1"][0]).any()                          # (no face on the plate's rho = 0 line)
        m0, m1, V, d = G.measure_fields(ob, dims, t=t, eps=1.0, T=T)
        cell = tuple(idx)
        record("sigma", T, XB.ratio(d[cell], *ref["sigma"], T))
        assert ref["band"].sum() > 100
        for c in range(D):
            record("mu0", T, XB.ratio(m0[cell + (c,)], ref["mu0"][0][c], ref["mu0"][1][c], T))
            record("V", T, XB.ratio(V[cell + (c,)], ref["V"][0][c], ref["V"][1][c], T))
            for j in range(D):
                record("mu1", T, XB.ratio(m1[cell + (c, j)], ref["mu1"][0][c + D * j], ref["mu1"][1][c + D * j], T))
        (nv, nM), brn = XB.nds(XB.body_at(name, t), idx)
        assert_clear(brn, np.float64, max(Ng), ("nds", "fast", "tie", "plate"))
        keep = (nv != 0).any(0)
        lin, nds = G.nds_band(ob, dims, t=t)
        assert np.array_equal(lin, np.ravel_multi_index(tuple(idx[:, keep]), Ng, order="F"))
        record("nds", np.float64, XB.ratio(nds.T, nv[:, keep], nM[:, keep], np.float64))
        XB.controls(name, t, idx, T, D, Ng, dict(sigma=d[cell], mu0=m0, mu1=m1.reshape(Ng + (D * D,), order="F"), V=V), lin, nds.T, keep)


@pytest.mark.parametrize("mk", [lambda t: XB.rotate3d(XB.C3, (0.3, -0.5, 0.8), 0.21, t, 0.4), lambda t: XB.rotate2d(12.3, 0.21, t, 0.4),
                                lambda t: XB.scale(XB.translate(3, t, v=(0.11, 0.0, 0.07)), 2.0)])
def test_map_builders_in_their_own_terms(mk):
    """The affine-map builders of the reference, checked without any other implementation: dA/dt and db/dt are the central
    differences of A(t) and b(t) (h = 2^-17: truncation 6e-11, rounding 3e-11 of entries of order 10); a rotation is
    orthogonal with determinant +1, is the identity at angle 0, keeps its axis and maps its centre to 0; it turns the BODY by
    +theta: the body point that starts at c + r sits at c + Rot(+theta) r, i.e. xi(c + Rot(theta) r) = xi_0(c + r)."""
    t, h = 7.37, 2.0 ** -17
    A, b, dA, db = mk(t)
    (Ap, bp, _, _), (Am, bm, _, _) = mk(t + h), mk(t - h)
    assert np.max(np.abs((Ap - Am) / (2 * h) - dA)) < 1e-9 and np.max(np.abs((bp - bm) / (2 * h) - db)) < 1e-9
    D = A.shape[0]
    s = np.cbrt(np.linalg.det(A)) if D == 3 else np.sqrt(np.linalg.det(A))
    assert np.allclose(A @ A.T, s * s * np.eye(D), atol=1e-14) and np.linalg.det(A) > 0


def test_rotation_conventions():
    th = 0.21 * 7.37
    k = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    c = np.array(XB.C3)
    A, b, _, _ = XB.rotate3d(XB.C3, (0.3, -0.5, 0.8), 0.21, 7.37)
    A0, b0, _, _ = XB.rotate3d(XB.C3, (0.3, -0.5, 0.8), 0.21, 0.0)
    assert np.allclose(A0, np.eye(3), atol=1e-15) and np.allclose(A @ k, k, atol=1e-15) and np.allclose(A @ c + b, 0, atol=1e-13)
    r = np.cross(k, [1.0, 0.0, 0.0])                                   # a vector across the axis, turned by +th about k
    rt = r * np.cos(th) + np.cross(k, r) * np.sin(th) + k * (k @ r) * (1 - np.cos(th))
    assert np.allclose(A @ (c + rt) + b, A0 @ (c + r) + b0, atol=1e-13)
    A2, b2, _, _ = XB.rotate2d(12.3, 0.21, 7.37)
    r2 = np.array([1.0, 0.0])
    rt2 = np.array([np.cos(th), np.sin(th)])                            # counter-clockwise by +th
    assert np.allclose(A2 @ (12.3 + rt2) + b2, r2, atol=1e-13) and np.allclose(A2 @ np.full(2, 12.3) + b2, 0, atol=1e-13)


def test_worst_ratios_are_recorded():
    """(prints the largest |oracle-ref| as a share of ulp_T/2 + K eps_64 M per quantity: -s shows it)"""
    print("\nworst oracle vs xref_body:", {k: round(v, 3) for k, v in sorted(WORST.items())})
