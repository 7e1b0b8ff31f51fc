"""Forces without a GPU: the three entry points are declared, bound and refuse bad calls before the device is touched; the
extended-precision restatement (forces_ref) agrees with xref_metrics on the three quantities they share and holds its own
closed forms; the rule by which series() combines the ranks of a z-slab run; the column names; the recorder's refusals."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forces_ref as R  # noqa: E402
import xref_metrics as XM  # noqa: E402
from xref_inputs import field  # noqa: E402

from waterlily_amd import _lib  # noqa: E402

NAMES = ("wl_body_loads", "wl_body_loads_mesh", "wl_band_loads")


def test_entry_points_declared_and_bound():
    for n, nargs in zip(NAMES, (10, 11, 10)):
        assert n in _lib.declared_symbols()
        fn = getattr(_lib.lib(), n)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int
    assert _lib.lib().wl_abi_version() == 6


def test_module_exposes_the_interface_and_columns():
    import waterlily_amd
    from waterlily_amd import forces as F
    assert waterlily_amd.forces is F
    for name in ("Forces", "record", "series", "columns", "reset", "loads", "coefficients", "combine"):
        assert callable(getattr(F, name)), name
    assert F.columns() == ("Fp_x", "Fp_y", "Fp_z", "Fv_x", "Fv_y", "Fv_z", "Mp_x", "Mp_y", "Mp_z", "Mv_x", "Mv_y", "Mv_z",
                           "Wp", "Wv", "ncells", "area")
    assert F.columns() == R.COLUMNS and len(F.columns()) == F.NV == R.NV == 16
    with pytest.raises(ValueError):
        F._x0((1.0, 2.0), 3)
    assert F._x0(None, 2) == (0.0, 0.0)
    # 2 F / (U^2 A)
    assert np.array_equal(F.coefficients(np.array([1.0, -3.0]), 2.0, 8.0), np.array([1.0, -3.0]) / 16.0)


def _grid(D=3):
    g = _lib.Grid()
    g.D = D
    g.n[:] = [10, 6, 5] if D == 3 else [10, 6, 1]
    g.s[:] = [1, 10, 60]
    g.sc = 300 if D == 3 else 60
    return g


def test_bad_calls_refused_without_device():
    L = _lib.lib()
    fake, x0 = C.c_void_p(0x1000), _lib.d3((0, 0, 0))      # never dereferenced: every call below fails validation first
    E = _lib.WL_E_ARG
    bd = (_lib.BodyDesc * 2)()
    bd[0].family, bd[0].count = _lib.WL_BODY_SPHERE, 1
    pose = _lib.MeshPose()
    pose.identity_map = 1
    g = _grid()
    calls = {
        "wl_body_loads": lambda g=g, p=fake, u=fake, lst=fake, n=4, x=x0, rows=fake, body=bd:
            L.wl_body_loads(0, None if g is None else C.byref(g), p, u, 0.1, body, lst, n, x, rows),
        "wl_body_loads_mesh": lambda g=g, p=fake, u=fake, lst=fake, n=4, x=x0, rows=fake, mesh=fake:
            L.wl_body_loads_mesh(0, None if g is None else C.byref(g), p, u, 0.1, mesh, C.byref(pose), lst, n, x, rows),
        "wl_band_loads": lambda g=g, p=fake, u=fake, lst=fake, n=4, x=x0, rows=fake, nds=fake:
            L.wl_band_loads(0, None if g is None else C.byref(g), p, u, 0.1, lst, nds, n, x, rows),
    }
    for name, call in calls.items():
        for kw in (dict(g=None), dict(p=None), dict(u=None), dict(x=None), dict(rows=None), dict(lst=None)):
            assert call(**kw) == E and b"null" in L.wl_last_error() and name.encode() in L.wl_last_error(), (name, kw)
        assert call(n=-1) == E and b"n < 0" in L.wl_last_error()
        for D in (1, 4):
            gd = _grid()
            gd.D = D
            assert call(g=gd) == E and b"D must be 2 or 3" in L.wl_last_error()
    assert calls["wl_body_loads"](body=None) == E and b"null body" in L.wl_last_error()
    bd[0].count = _lib.WL_BODY_MAXLEAF + 1
    assert calls["wl_body_loads"]() == E and b"WL_BODY_MAXLEAF" in L.wl_last_error()
    bd[0].count, bd[0].family = 1, 9
    assert calls["wl_body_loads"]() == E and b"family" in L.wl_last_error()
    assert calls["wl_body_loads_mesh"](g=_grid(2)) == E and b"D == 3" in L.wl_last_error()
    assert calls["wl_body_loads_mesh"](mesh=None) == E and b"null mesh" in L.wl_last_error()
    assert calls["wl_band_loads"](nds=None) == E and b"null nds" in L.wl_last_error()
    # a z-slab whose owned interior plane has no halo plane below it
    gs = _grid()
    gs.nzg, gs.kz0, gs.own_lo, gs.own_hi = 12, 3, 0, 3
    assert calls["wl_band_loads"](g=gs) == E and b"halo plane" in L.wl_last_error()


@pytest.mark.parametrize("T", [np.float32, np.float64])
@pytest.mark.parametrize("Ng", [(11, 9, 7), (13, 11)])
def test_restatement_agrees_with_xref_metrics(T, Ng):
    """Fp, Fv, Mp of forces_ref are xref_metrics' band sums (ratio 0 <= 1, values and bounds alike); cells with a zero nds
    vector are not counted; the leaf rows partition the total; the new columns hold their closed forms"""
    D = len(Ng)
    n = 300
    idx, nds = XM.synthetic_band(Ng, n, 7)
    nds[5] = 0.0
    nds[17] = 0.0
    p, u = field(Ng, T, "random", 41), field(Ng + (D,), T, "random", 42)
    nu, x0 = float(T(0.37)), XM.X0[:D]
    rng = np.random.default_rng(3)
    V = rng.standard_normal((n, D))
    leaf = rng.integers(0, 3, n)
    v, M, cnt = R.rows(p, u, nu, x0, idx, nds, V=V, leaf=leaf, nleaf=3)
    assert v.shape == M.shape == (4, 16) and cnt[-1] == n - 2 == cnt[:3].sum() and np.array_equal(v[:, 14], cnt)
    keep = (nds != 0).any(1)
    for name, cols, ref in (("pforce", slice(0, D), XM.pressure_force(p, idx[keep], nds[keep])),
                            ("vforce", slice(3, 3 + D), XM.viscous_force(u, nu, idx[keep], nds[keep])),
                            ("pmoment", slice(6, 9) if D == 3 else slice(8, 9), XM.pressure_moment(p, x0, idx[keep], nds[keep]))):
        rv, rM = (ref[0][:1], ref[1][:1]) if (name == "pmoment" and D == 2) else ref
        assert XM.band_ratio(name, v[-1, cols], rv, rM, n, T) <= 1
        assert XM.band_ratio(name, rv, v[-1, cols], M[-1, cols], n, T) <= 1
        assert np.array_equal(M[-1, cols], rM)
    r = R.ratios(v[-1], v[-1], M[-1], cnt[-1], T)
    assert r.max() == 0.0
    # the leaf rows add up to the total within a rounding of each
    assert np.allclose(v[:3].sum(0), v[-1], rtol=1e-13, atol=1e-13 * np.abs(M[-1]).max())
    if D == 2:
        assert not v[:, [2, 5, 6, 7, 9, 10]].any() and not M[:, [2, 5, 6, 7, 9, 10]].any()
    # closed forms: V constant -> Wp = Fp . V, Wv = Fv . V; A = sum |nds|
    Vc = np.broadcast_to(np.array([0.5, -0.25, 2.0][:D]), (n, D))
    v2, M2, _ = R.rows(p, u, nu, x0, idx, nds, V=Vc)
    assert abs(v2[-1, 12] - v2[-1, 0:D] @ Vc[0]) <= 4 * np.finfo(np.float64).eps * M2[-1, 12]
    assert abs(v2[-1, 13] - v2[-1, 3:3 + D] @ Vc[0]) <= 4 * np.finfo(np.float64).eps * M2[-1, 13]
    assert np.isclose(v2[-1, 15], np.linalg.norm(nds, axis=1).sum(), rtol=1e-14)
    # a stored band has no V: NaN, which only a NaN meets
    v3, M3, _ = R.rows(p, u, nu, x0, idx, nds)
    assert np.isnan(v3[:, 12:14]).all()
    got = v3[-1].copy()
    assert R.ratios(got, v3[-1], M3[-1], n, T).max() == 0.0
    got[12] = 0.0
    assert R.ratios(got, v3[-1], M3[-1], n, T)[12] == np.inf
    # controls: a moment about another point and a shifted list leave their bounds
    vs, Ms, _ = R.rows(p, u, nu, tuple(reversed(x0)), idx, nds, V=V)
    assert R.ratios(vs[-1], v2[-1], M2[-1], n, T)[9 if D == 3 else 11] > 1
    vr, _, _ = R.rows(p, u, nu, x0, np.roll(idx, 1), nds, V=Vc)
    rr = R.ratios(vr[-1], v2[-1], M2[-1], n, T)
    assert rr[0] > 1 and rr[3] > 1 and rr[12] > 1 and rr[13] > 1 and rr[14] == 0 and rr[15] == 0


def test_geometry_from_xref_body():
    """nds, V and the active leaf of a two-leaf union: each cell belongs to the nearer sphere, V is the leaf's own"""
    import xref_body as XB
    body = [XB.leaf("sphere", ((6.3, 6.2, 5.1), 3.0), XB.translate(3, 0.0, v=(0.5, 0.0, -0.25))),
            XB.leaf("sphere", ((15.3, 6.2, 5.1), 3.0), None, "+")]
    idx = XB.inside_cells((20, 11, 9))
    nds, V, act = R.geometry(body, idx)
    on = (nds != 0).any(1)
    assert on.sum() > 100 and set(act[on]) == {0, 1}
    assert np.array_equal(act[on] == 0, idx[0][on] < 11)
    assert np.allclose(V[on & (act == 0)], (0.5, 0.0, -0.25)) and not V[on & (act == 1)].any()


def test_slab_combination_rule():
    """series(): every column by addition in rank order (pure host code); NaN stays NaN"""
    from waterlily_amd import forces as F
    rng = np.random.default_rng(5)
    parts = [rng.standard_normal((7, 3, 16)) for _ in range(3)]
    v = F.combine(parts)
    assert np.array_equal(v, (parts[0] + parts[1]) + parts[2])
    assert np.array_equal(F.combine(parts[:1]), parts[0]) and F.combine(parts[:1]) is not parts[0]
    assert np.array_equal(F.combine([parts[0], np.zeros((7, 3, 16))]), parts[0])
    q = [np.ones((1, 2, 16)), np.ones((1, 2, 16))]
    q[1][0, :, 12:14] = np.nan
    w = F.combine(q)
    assert np.isnan(w[0, :, 12:14]).all() and np.array_equal(np.delete(w[0], [12, 13], axis=1), np.full((2, 14), 2.0))
    assert F.combine([np.zeros((0, 2, 16)), np.zeros((0, 2, 16))]).shape == (0, 2, 16)


def _fake_sim(D, slab=None):
    from waterlily_amd import body as B
    flow = types.SimpleNamespace(D=D, layout=types.SimpleNamespace(slab=slab), device="cpu", _band_cells=None)
    return types.SimpleNamespace(flow=flow, body=B.NoBody(), geometry="device", _band=None)


def test_recorder_refuses_another_dimension_or_slab():
    from waterlily_amd import forces as F
    slab = object()
    fr = F.Forces(_fake_sim(3, slab), x0=(1.0, 2.0, 3.0), capacity=4)
    assert tuple(fr.buf.shape) == (4, 2, 16) and fr.nleaf == 1 and fr.t == []
    with pytest.raises(ValueError, match="dimension or slab"):
        F.record(fr, _fake_sim(2, slab))
    with pytest.raises(ValueError, match="dimension or slab"):
        F.record(fr, _fake_sim(3, None))
    with pytest.raises(ValueError, match="dimension or slab"):
        F.record(fr, _fake_sim(3, object()))
    with pytest.raises(ValueError, match="capacity"):
        F.Forces(_fake_sim(2), capacity=0)
    with pytest.raises(ValueError, match="x0 must have 2"):
        F.Forces(_fake_sim(2), x0=(0.0, 0.0, 0.0))
    assert fr.t == []
