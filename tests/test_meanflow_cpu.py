"""MeanFlow without a GPU: the entry point is exported and bound, bad calls are refused before the device is touched, the
host-side eps schedule, and why the covariance (not <uu>) is stored -- on the numpy restatement of the rule (meanflow_ref)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meanflow_ref as R  # noqa: E402

from waterlily_amd import _lib  # noqa: E402

# relative error of the stored Float32 covariance on the signal of meanflow_ref.cancellation_signal: 1.4e-7 measured with the
# numpy restatement (2000 updates, uneven dt); the bound leaves a factor of ~70 (the GPU test holds the kernel to it too)
ROBUST_BOUND = 1e-5


def test_entry_point_exported_and_bound():
    L = _lib.lib()
    assert "wl_meanflow_update" in _lib.declared_symbols()
    fn = L.wl_meanflow_update
    assert fn.argtypes is not None and len(fn.argtypes) == 12 and fn.restype is C.c_int


def _grid(D=3, n=(10, 6, 5), sy=None):
    g = _lib.Grid()
    g.D = D
    n = tuple(n[:D]) + (1,) * (3 - D)
    sy = n[0] if sy is None else sy
    g.n[:] = list(n)
    g.s[:] = [1, sy, sy * n[1]]
    g.sc = sy * n[1] * n[2]
    return g


def test_bad_calls_refused_without_device():
    L = _lib.lib()
    F32, F64, E = _lib.WL_F32, _lib.WL_F64, _lib.WL_E_ARG
    fake = C.c_void_p(0x1000)                     # never dereferenced: every call below fails validation first

    def call(tf=F32, ta=F32, g=None, ga=None, U=fake, P=fake, eps=0.5, first=0):
        g = _grid() if g is None else g
        ga = _grid() if ga is None else ga
        return L.wl_meanflow_update(tf, ta, C.byref(g), fake, fake, C.byref(ga), U, P, None, None, eps, first)

    bad = _grid()
    bad.D = 4
    assert call(g=bad) == E and b"grid.D" in L.wl_last_error()
    assert call(tf=F64, ta=F32) == E and b"Float32 accumulators" in L.wl_last_error()
    assert call(U=None) == E and b"null" in L.wl_last_error()
    assert call(P=None) == E and b"null" in L.wl_last_error()
    assert call(ga=_grid(n=(10, 6, 6))) == E and b"extents" in L.wl_last_error()
    ga = _grid()
    ga.nzg, ga.kz0, ga.own_lo, ga.own_hi = 8, 0, 1, 3
    assert call(ga=ga) == E and b"slab" in L.wl_last_error()
    for eps in (0.0, -0.5, 1.0 + 1e-12, float("nan")):
        assert call(eps=eps) == E and b"eps" in L.wl_last_error(), eps
    assert call(tf=7) == E and b"dtype" in L.wl_last_error()


def test_eps_schedule():
    from waterlily_amd.stats import weight
    for fn in (weight, R.eps_schedule):
        ts = [0.5]
        assert fn(ts, 0.75) == 1.0                            # first update of a window: exactly 1
        assert fn([0.5, 0.75], 0.75) is None                   # dt == 0: nothing to do
        with pytest.raises(ValueError):
            fn([0.5, 0.75], 0.7)                               # time went back
        # uneven dt: eps_n = dt_n / (t_n - t_0), in Float64
        t, seen = 0.0, [0.0]
        for dt in (0.3, 0.1, 0.25, 0.05):
            t += dt
            e = fn(seen, t)
            assert e == (t - seen[-1]) / (t - seen[0]) and (len(seen) > 1 or e == 1.0)
            seen.append(t)
    # the weights reproduce the dt-weighted mean exactly in exact arithmetic: check in Float64 on a short series
    xs, dts = np.array([1.0, 4.0, 2.0, 8.0]), np.array([0.3, 0.1, 0.25, 0.05])
    m, seen, t = 0.0, [0.0], 0.0
    for x, dt in zip(xs, dts):
        t += dt
        e = weight(seen, t)
        m = m + e * (x - m)
        seen.append(t)
    assert abs(m - (xs * dts).sum() / dts.sum()) < 1e-15


def test_meanflow_python_api_refuses_bad_dtypes():
    from waterlily_amd import stats

    class FakeFlow:                     # MeanFlow checks the dtype pair before it allocates anything
        D, T = 3, np.dtype(np.float64)
    with pytest.raises(ValueError, match="Float32 accumulators"):
        stats.MeanFlow(FakeFlow(), dtype=np.float32)
    with pytest.raises(ValueError, match="float32 or float64"):
        stats.MeanFlow(FakeFlow(), dtype=np.float16)


def test_covariance_not_cancellation():
    """u = a + b s_n, a / b = 1e3, 2000 updates with uneven dt: the stored Float32 covariance stays within ROBUST_BOUND of the
    dt-weighted variance, the naive Float32 <uu> - <u><u> misses by more than 100 % (> 10x the bound and then some)."""
    xs, dts = R.cancellation_signal()
    ex = R.exact_variance(xs, dts)
    robust = abs(R.robust_variance(xs, dts) - ex) / ex
    naive = abs(R.naive_variance(xs, dts) - ex) / ex
    assert robust < ROBUST_BOUND, robust
    assert naive > 1.0 and naive > 10 * ROBUST_BOUND, naive
    # in Float64 both forms are fine: it is the Float32 storage that the naive form cannot survive
    ex64 = R.exact_variance(xs, dts, np.float64)
    assert abs(R.naive_variance(xs, dts, np.float64) - ex64) / ex64 < 1e-6
    # the array form of the restatement is the same rule as its one-element form
    ref = R.RefMean(1, np.float32, 0.0, uu=True, pp=True)
    t = 0.0
    for x, dt in zip(xs, dts):
        t += dt
        ref.update(np.full((2, 1), np.float32(x)), np.full((2,), np.float32(x)), t)
    assert float(ref.UU[0, 0]) == R.robust_variance(xs, dts) and float(ref.pp[0]) == R.robust_variance(xs, dts)
