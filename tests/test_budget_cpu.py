"""Budget without a GPU: the numpy restatement of its two rules (budget_ref) against direct long-double moments and against
analytic cases, its degenerate inputs, and the argument checks of wl_budget_update / wl_budget_terms through ctypes (fake
pointers: every call fails validation before anything is dereferenced)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget_ref as B  # noqa: E402

from waterlily_amd import _lib  # noqa: E402

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("D", [2, 3])
def test_restatement_matches_direct_moments(D):
    """n = 25 updates of random fields with uneven dt, A = Float64: the incremental rule reproduces the time-weighted two-pass
    central moments (long double) within 8 n 2^-53 on the scale of each moment"""
    n = 25
    N = (9, 8) if D == 2 else (7, 6, 5)
    rng = np.random.default_rng(11 + D)
    ref = B.RefBudget(D, F64, 0.0)
    us, ps, dts, t = [], [], [], 0.0
    for _ in range(n):
        u = rng.standard_normal(N + (D,)) * 0.3 + 1.0
        p = rng.standard_normal(N)
        dt = 0.1 + 0.4 * rng.random()
        t += dt
        ref.update(u, p, t)
        us.append(u), ps.append(p), dts.append(dt)
    # the weights of the rule are the differences of the times it saw, not the dt that were added up
    want = B.direct_moments(us, ps, np.diff(np.asarray(ref.t, dtype=np.longdouble)))
    I = tuple(slice(1, m - 1) for m in N)
    for name, got in (("U", ref.mean.U), ("P", ref.mean.P), ("R", ref.R[I]), ("PU", ref.PU[I]), ("GG", ref.GG[I]), ("T3", ref.T3[I])):
        w = want[name]
        err = float(np.max(np.abs(got.astype(np.longdouble) - w)))
        bound = 8 * n * 2.0 ** -53 * max(1.0, float(np.max(np.abs(w))))
        print(name, err, bound)
        assert err <= bound, (name, err, bound)
    assert float(np.max(np.abs(want["T3"]))) > 1e-3                      # the third moments are not trivially zero


def _whole_periods(field, D, N, A=F64, periods=3, per=16):
    """a RefBudget fed field(t) at t = dt, 2 dt, ... over whole periods of omega = 2 pi"""
    ref = B.RefBudget(D, A, 0.0)
    dt = 1.0 / per
    for n in range(1, periods * per + 1):
        u, p = field(2.0 * np.pi * n * dt)
        ref.update(u, p, n * dt)
    return ref


def shear_field(N, S, a, b):
    y = np.broadcast_to(np.arange(N[1], dtype=np.float64)[None, :], N)

    def field(wt):
        u = np.zeros(N + (2,))
        u[..., 0] = S * y + a * np.cos(wt)
        u[..., 1] = b * np.cos(wt)
        return u, np.zeros(N)
    return field


def check_shear_terms(T, S, a, b, tol=1e-12):
    """analytic case A on the cells the terms are formed on: production -abS/2, k (a^2+b^2)/4, everything else 0"""
    J = tuple(slice(2, m - 2) for m in T.shape[:-1])
    T = np.asarray(T, dtype=np.float64)[J]
    want = {"k": (a * a + b * b) / 4, "production": -a * b * S / 2, "residual": -a * b * S / 2}
    for c, name in enumerate(B.COLUMNS):
        err = float(np.max(np.abs(T[..., c] - want.get(name, 0.0))))
        print(name, err)
        assert err <= tol, (name, err)


def test_production_in_uniform_shear():
    N, S, a, b = (10, 9), 0.25, 0.5, -0.75
    ref = _whole_periods(shear_field(N, S, a, b), 2, N)
    check_shear_terms(ref.terms(0.01), S, a, b)


def test_dissipation_of_a_standing_wave():
    """analytic case B: u_x' = a cos(wt) sin(kappa y) gives GG = (a^2/2) cos^2(kappa y) sin^2(kappa), exact for the discrete
    gradient; dissipation is nu times that"""
    N, a, kap, nu = (8, 12), 0.5, 0.4, 0.02
    j = np.arange(N[1], dtype=np.float64)

    def field(wt):
        u = np.zeros(N + (2,))
        u[..., 0] = a * np.cos(wt) * np.sin(kap * j)[None, :]
        return u, np.zeros(N)
    ref = _whole_periods(field, 2, N)
    want = np.broadcast_to((a * a / 2 * np.cos(kap * j) ** 2 * np.sin(kap) ** 2)[None, :], N)
    I = tuple(slice(1, m - 1) for m in N)
    assert float(np.max(np.abs(ref.GG[I] - want[I]))) <= 1e-12
    J = tuple(slice(2, m - 2) for m in N)
    T = ref.terms(nu)
    assert float(np.max(np.abs(T[J + (2,)] - nu * want[J]))) <= 1e-12
    assert np.all(T[J + (2,)] >= 0) and float(np.max(T[J + (2,)])) > 1e-4


@pytest.mark.parametrize("A", [F32, F64])
def test_degenerate_inputs(A):
    N = (7, 6, 5)
    rng = np.random.default_rng(5)
    u, p = rng.standard_normal(N + (3,)).astype(A), rng.standard_normal(N).astype(A)
    ref = B.RefBudget(3, A, 0.0)
    # `first` reads no accumulator: NaN-filled ones do not survive the first update
    ref.R, ref.PU = np.full(N + (6,), np.nan, dtype=A), np.full(N + (3,), np.nan, dtype=A)
    ref.GG, ref.T3 = np.full(N, np.nan, dtype=A), np.full(N + (3,), np.nan, dtype=A)
    for n in range(1, 6):                                              # a constant field: every moment stays exactly zero
        ref.update(u, p, 0.3 * n)
        for x in (ref.R, ref.PU, ref.GG, ref.T3):
            assert x.dtype == np.dtype(A) and not x.any()
    assert ref.update(u, p, 1.5) is None and len(ref.t) == 6           # dt == 0: nothing happens
    assert not ref.terms(0.1).any()
    with pytest.raises(ValueError):
        ref.update(u, p, 1.0)                                          # time going backwards


def test_update_refuses_time_going_backwards():
    """budget.update asks stats.weight before it touches the library: a flow whose time lies before the last one seen raises"""
    from waterlily_amd import budget
    bg = object.__new__(budget.Budget)
    bg.mean = types.SimpleNamespace(t=[0.0, 1.0])
    with pytest.raises(ValueError, match="went back"):
        budget.update(bg, types.SimpleNamespace(dt=[0.5, 0.25]))       # time(flow) = 0.5
    assert budget.update(bg, types.SimpleNamespace(dt=[1.0, 0.25])) is None and bg.mean.t == [0.0, 1.0]     # dt == 0: a no-op
    assert budget.columns() == B.COLUMNS and len(budget.columns()) == 8


def test_integrate_sums_columns_in_float64():
    import torch
    from waterlily_amd import budget
    rng = np.random.default_rng(2)
    h = rng.standard_normal((6, 5, 4, 8)).astype(F32)
    t = torch.from_numpy(h)
    got = budget.integrate(t)
    assert got.dtype == torch.float64 and tuple(got.shape) == (8,)
    assert np.allclose(got.numpy(), h.astype(F64).sum(axis=(0, 1, 2)), rtol=0, atol=1e-12)
    got = budget.integrate(t, box=((1, 2, 0), (4, 5, 3)))
    assert np.allclose(got.numpy(), h[1:4, 2:5, 0:3].astype(F64).sum(axis=(0, 1, 2)), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        budget.integrate(t, box=((1, 2), (4, 5)))


# --------------------------------------------------------------------------- argument checks through ctypes

E = _lib.WL_E_ARG
FAKE = C.c_void_p(0x1000)


def grid(n=(8, 8, 8)):
    g = _lib.Grid()
    g.D = 3
    g.n[:] = list(n)
    g.s[:] = [1, n[0], n[0] * n[1]]
    g.sc = n[0] * n[1] * n[2]
    return g


def _update(L, tf=0, ta=0, g=None, ga=None, ptrs=None, eps=0.5, first=0):
    g, ga = g or grid(), ga or grid()
    ptrs = ptrs or [FAKE] * 8
    return L.wl_budget_update(tf, ta, C.byref(g) if g is not None else None, ptrs[0], ptrs[1], C.byref(ga), *ptrs[2:], eps, first)


def _refused(L, rc, word):
    assert rc == E and word in L.wl_last_error(), (rc, L.wl_last_error())


def test_update_argument_checks():
    L = _lib.lib()
    for k in range(8):                                                 # u, p, Uf, Pm, R, PU, GG, T3
        ptrs = [FAKE] * 8
        ptrs[k] = None
        _refused(L, _update(L, ptrs=ptrs), b"null")
    for eps in (0.0, -0.1, 1.0 + 2.0 ** -52, float("nan"), float("inf")):
        _refused(L, _update(L, eps=eps), b"eps")
    _refused(L, _update(L, tf=_lib.WL_F64, ta=_lib.WL_F32), b"Float32 accumulators on a Float64 flow")
    _refused(L, _update(L, tf=7), b"dtype")
    _refused(L, _update(L, ta=7), b"dtype")
    _refused(L, _update(L, ga=grid((8, 8, 9))), b"extents")
    slab = grid((8, 8, 6))
    slab.nzg, slab.kz0, slab.own_lo, slab.own_hi = 10, 0, 2, 3
    other = grid((8, 8, 6))
    other.nzg, other.kz0, other.own_lo, other.own_hi = 10, 4, 2, 3
    _refused(L, _update(L, g=slab, ga=other), b"slab")
    g2 = grid()
    g2.D = 1
    _refused(L, _update(L, g=g2, ga=g2), b"D must be 2 or 3")
    # a slab whose owned interior planes have no halo plane below them
    bare = grid((8, 8, 4))
    bare.nzg, bare.kz0, bare.own_lo, bare.own_hi = 10, 4, 0, 3
    _refused(L, _update(L, g=bare, ga=bare), b"halo plane")


def test_terms_argument_checks():
    L = _lib.lib()
    g = grid()
    call = lambda t=0, ptrs=None, nu=0.1: L.wl_budget_terms(t, C.byref(g), *(ptrs or [FAKE] * 6)[:5], nu, (ptrs or [FAKE] * 6)[5])
    for k in range(6):                                                 # Uf, R, PU, GG, T3, out
        ptrs = [FAKE] * 6
        ptrs[k] = None
        _refused(L, call(ptrs=ptrs), b"null")
    _refused(L, call(t=7), b"dtype")
    _refused(L, call(nu=float("nan")), b"nu")
    assert L.wl_abi_version() == 6
