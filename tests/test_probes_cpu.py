"""CPU checks of the point-probe feature: the numpy restatement of interp against the reference's own answers
(test/maintests.jl:58-64) and against exact arithmetic, the Heun step against its closed form on a solid-body rotation, and
argument validation of wl_interp / wl_tracer_advance without a device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probes_ref as R  # noqa: E402

from waterlily_amd import _lib  # noqa: E402


def maintests_arrays():
    """a = zeros(5,5,2); b = zeros(5,5); apply!((i,x)->x[i]+1.5, a); apply!(x->x[1]+1.5, b)"""
    a = R.fill_faces((5, 5), lambda i, x: x[i] + 1.5)
    b = R.fill_centres((5, 5), lambda x: x[0] + 1.5)
    return a, b


def test_restatement_reproduces_maintests():
    a, b = maintests_arrays()
    assert np.array_equal(R.interp_vec((2.5, 1), a), [2.5, 1.0])
    assert np.array_equal(R.interp_vec((3.5, 3), a), [3.5, 3.0])
    assert R.interp((2.5, 1), b) == 2.5
    assert R.interp((3.5, 3), b) == 3.5
    # the 3-D analogue of the same fill
    a3 = R.fill_faces((5, 5, 4), lambda i, x: x[i] + 1.5)
    assert np.array_equal(R.interp_vec((2.5, 1, 2.25), a3), [2.5, 1.0, 2.25])


def test_restatement_range_rule():
    """x_d == n_d reads no corner beyond the array; one step further, or below 1, is NaN; a zero-weight corner outside is
    never read"""
    b = R.fill_centres((5, 4), lambda x: 2 * x[0] - x[1])
    assert R.interp((5.0, 4.0), b) == b[4, 3]
    assert R.interp((1.0, 1.0), b) == b[0, 0]
    for bad in ((5.0 + 2 ** -50, 2.0), (0.999, 2.0), (2.0, 4.5), (float("nan"), 2.0), (1e300, 2.0)):
        assert np.isnan(R.interp(bad, b)), bad
    u = R.fill_faces((5, 4), lambda i, x: x[0] + 0 * x[1])
    assert not np.isnan(R.interp_vec((4.5, 3.0), u)).any()           # x component at 5.0: upper corner weight 0
    assert np.isnan(R.interp_vec((4.5, 4.0), u)[1])                  # y component at 4.5: weighted corner 5 > 4
    assert np.isnan(R.interp_vec((4.75, 2.0), u)[0])


def test_restatement_agrees_with_exact():
    rng = np.random.default_rng(5)
    for D, shape in ((2, (7, 6)), (3, (5, 6, 4))):
        a = rng.integers(-4, 5, size=shape).astype(np.float64) / 8 + rng.standard_normal(shape) * (rng.random(shape) < 0.5)
        for _ in range(200):
            x = rng.uniform(1, np.array(shape), size=D)
            k = rng.random(D) < 0.3
            x[k] = np.floor(x[k])                                           # integer coordinates
            got = R.interp(x, a)
            want, bound = R.exact(x, a)
            assert abs(got - want) <= (2 ** D + D + 2) * np.finfo(np.float64).eps * bound, (x, got, want)


def _rotation(shape, om, cen):
    """u = om * (-(y - cy), x - cx, 0): linear, so interpolation reproduces it"""
    def f(i, x):
        if i == 0:
            return -om * (x[1] - cen[1])
        if i == 1:
            return om * (x[0] - cen[0])
        return 0 * x[0]
    return R.fill_faces(shape, f)


@pytest.mark.parametrize("D", [2, 3])
def test_heun_rotation_closed_form(D):
    """one Heun step of a solid-body rotation multiplies the radius by sqrt(1 + (om dt)^4 / 4)"""
    shape = (34, 34) if D == 2 else (34, 34, 6)
    om, dt = 0.05, 0.7
    cen = (16.0, 16.0)
    u = _rotation(shape, om, cen)
    x0 = np.array([[cen[0] + 1.5 + r * np.cos(th), cen[1] + 1.5 + r * np.sin(th)] + [3.25] * (D - 2)
                   for r, th in ((5.0, 0.3), (9.5, 2.0), (12.0, 4.4))])
    x = x0
    g = np.sqrt(1 + (om * dt) ** 4 / 4)
    for n in range(1, 6):
        x = R.heun(x, u, dt)
        r0 = np.hypot(x0[:, 0] - cen[0] - 1.5, x0[:, 1] - cen[1] - 1.5)
        r = np.hypot(x[:, 0] - cen[0] - 1.5, x[:, 1] - cen[1] - 1.5)
        np.testing.assert_allclose(r / r0, g ** n, rtol=1e-13, atol=0)
        if D == 3:
            assert np.all(x[:, 2] == 3.25)


def test_heun_wrap_and_death():
    """x periodic (N = 8: positions wrap into [1.5, 9.5)), y not (alive in [1.5, 7.5], the end included)"""
    u = R.fill_faces((10, 8), lambda i, x: 0 * x[0] + (1.0 if i == 0 else -0.5))
    X = np.array([[9.0, 4.0], [3.0, 2.0], [5.0, 1.75]])
    Y = R.heun(X, u, 1.0, perdir=(0,))
    assert np.array_equal(Y[0], [2.0, 3.5])
    assert np.array_equal(Y[1], [4.0, 1.5])
    assert np.isnan(Y[2]).all()
    Z = R.heun(Y, u, 1.0, perdir=(0,))
    assert np.array_equal(Z[0], [3.0, 3.0]) and np.isnan(Z[1]).all() and np.isnan(Z[2]).all()


def _grid3(nzg=0):
    g = _lib.Grid()
    g.D = 3
    g.n[:] = [8, 8, 8]
    g.s[:] = [1, 8, 64]
    g.sc = 512
    if nzg:
        g.nzg, g.kz0, g.own_lo, g.own_hi = nzg, -1, 1, 5
    return g


def test_entry_points_validate_without_gpu():
    L = _lib.lib()
    g = _grid3()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    E = _lib.WL_E_ARG

    def err(rc, text):
        assert rc == E and text in L.wl_last_error(), (rc, L.wl_last_error())

    err(L.wl_interp(7, C.byref(g), p, 0, p, 1, p, 1), b"dtype")
    bad = _grid3()
    bad.D = 4
    err(L.wl_interp(_lib.WL_F32, C.byref(bad), p, 0, p, 1, p, 1), b"grid.D")
    err(L.wl_interp(_lib.WL_F32, None, p, 0, p, 1, p, 1), b"null grid")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), None, 0, p, 1, p, 1), b"null")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), p, 0, None, 1, p, 1), b"null")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), p, 0, p, 1, None, 1), b"null")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), p, 2, p, 1, p, 3), b"ncomp")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), p, -3, p, 1, p, 3), b"ncomp")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), p, 0, p, -1, p, 1), b"negative")
    err(L.wl_interp(_lib.WL_F32, C.byref(g), p, 3, p, 1, p, 2), b"ldo")
    err(L.wl_interp(_lib.WL_F64, C.byref(g), p, 0, p, 1, p, 0), b"ldo")
    assert L.wl_interp(_lib.WL_F64, C.byref(g), p, 3, p, 0, p, 4) == 0          # m == 0: nothing launched
    sl = _grid3(14)
    assert L.wl_interp(_lib.WL_F32, C.byref(sl), p, 3, p, 0, p, 3) == 0          # slabs are interpolated

    err(L.wl_tracer_advance(5, C.byref(g), p, p, 1, 0.1, 0), b"dtype")
    err(L.wl_tracer_advance(_lib.WL_F32, C.byref(bad), p, p, 1, 0.1, 0), b"grid.D")
    err(L.wl_tracer_advance(_lib.WL_F32, C.byref(g), None, p, 1, 0.1, 0), b"null")
    err(L.wl_tracer_advance(_lib.WL_F32, C.byref(g), p, None, 1, 0.1, 0), b"null")
    err(L.wl_tracer_advance(_lib.WL_F32, C.byref(g), p, p, -2, 0.1, 0), b"negative")
    for dt in (float("nan"), float("inf"), -0.5):
        err(L.wl_tracer_advance(_lib.WL_F32, C.byref(g), p, p, 1, dt, 0), b"dt")
    err(L.wl_tracer_advance(_lib.WL_F32, C.byref(g), p, p, 1, 0.1, 8), b"perdir_mask")
    err(L.wl_tracer_advance(_lib.WL_F32, C.byref(g), p, p, 1, 0.1, -1), b"perdir_mask")
    assert L.wl_tracer_advance(_lib.WL_F32, C.byref(sl), p, p, 1, 0.1, 0) == _lib.WL_E_STATE
    assert b"z-slab" in L.wl_last_error()
    assert L.wl_tracer_advance(_lib.WL_F64, C.byref(g), p, p, 0, 0.0, 7) == 0      # m == 0: nothing launched
