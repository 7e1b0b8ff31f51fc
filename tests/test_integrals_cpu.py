"""Integrals without a GPU: the entry point is declared, bound and refuses bad calls before the device is touched; the numpy
restatement (integrals_ref) holds its closed forms exactly and agrees with the oracle's per-cell metrics; the rule by which
series() combines the ranks of a z-slab run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import integrals_ref as R  # noqa: E402
from xref_inputs import field  # noqa: E402

from waterlily_amd import _lib  # noqa: E402


def test_entry_point_declared_and_bound():
    assert "wl_flow_integrals" in _lib.declared_symbols()
    fn = _lib.lib().wl_flow_integrals
    assert fn.argtypes is not None and len(fn.argtypes) == 5 and fn.restype is C.c_int
    assert _lib.lib().wl_abi_version() == 6


def test_module_exposes_the_interface():
    from waterlily_amd import integrals as I
    for name in ("Integrals", "record", "series", "columns", "reset", "integrals", "combine"):
        assert callable(getattr(I, name)), name
    assert I._names(2) == R.names(2) and I._names(3) == R.names(3)
    assert I._names(3) == ("E", "Z", "S", "div2", "divmax", "umax", "P1", "P2", "P3")
    with pytest.raises(ValueError):
        I._background((1.0, 2.0), 3)


def test_bad_calls_refused_without_device():
    L = _lib.lib()
    fake, U = C.c_void_p(0x1000), _lib.d3((0, 0, 0))      # never dereferenced: every call below fails validation first
    g = _lib.Grid()
    g.D = 3
    g.n[:] = [10, 6, 5]
    g.s[:] = [1, 10, 60]
    g.sc = 300
    E = _lib.WL_E_ARG
    assert L.wl_flow_integrals(0, C.byref(g), None, U, fake) == E and b"null" in L.wl_last_error()
    assert L.wl_flow_integrals(0, C.byref(g), fake, None, fake) == E and b"null" in L.wl_last_error()
    assert L.wl_flow_integrals(0, C.byref(g), fake, U, None) == E and b"null" in L.wl_last_error()
    assert L.wl_flow_integrals(0, None, fake, U, fake) == E and b"null" in L.wl_last_error()
    for D in (1, 4):
        g.D = D
        assert L.wl_flow_integrals(0, C.byref(g), fake, U, fake) == E and b"D must be 2 or 3" in L.wl_last_error()


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_restatement_closed_forms_exact(D, T):
    """uniform flow, E with U = U0, solid rotations, plane shear, pure strain: exact, with S = div2 = 0 to the bit for the
    rotations"""
    for label, Ng, f, U, spec in R.pins(D):
        row, bound, n = R.integrals(R.index_field(Ng, f, T), U)
        assert n == int(np.prod([m - 2 for m in Ng]))
        R.check_pin(row, spec, Ng, label)


def test_restatement_maxima_and_nan():
    u = np.zeros((6, 5, 2))
    u[2, 2, 0], u[4, 3, 1] = -7.0, 2.0
    u[0, 0, 0] = 99.0                                         # a ghost cell: outside inside(p), not seen by umax
    row, bound, n = R.integrals(u)
    assert float(row[5]) == 7.0 and float(row[4]) == 7.0 and float(bound[4]) == 7.0
    u[3, 3, 1] = np.nan
    row, _, _ = R.integrals(u)
    assert np.isnan(np.asarray(row[:4], dtype=np.float64)).all() and float(row[5]) == 7.0 and not np.isnan(float(row[4]))


def test_restatement_against_oracle_metrics():
    """sum over the oracle's ke and omega_mag^2 / 2 fields (Float64: the oracle rounds every cell to T): within the summation
    bound, plus 4 ulp per cell for the square root of omega_mag"""
    from oracle import wl_oracle as O
    for Ng, seed in (((9, 8, 7), 1), ((14, 5, 6), 2)):
        u = field(Ng + (3,), np.float64, "random", seed)
        U = (0.25, -0.5, 0.125)
        row, bound, n = R.integrals(u, U)
        tol = R.tolerance(bound, n)
        ke = O.metric(O.zeros(Ng, np.float64), "ke", u, par=U)
        om = O.metric(O.zeros(Ng, np.float64), "omega_mag", u)
        ins = tuple(slice(1, m - 1) for m in Ng)
        E = ke[ins].astype(np.longdouble).sum()
        Z = (om[ins].astype(np.longdouble) ** 2 / 2).sum()
        assert abs(float(E - row[0])) <= tol[0]
        assert abs(float(Z - row[1])) <= tol[1] + 4 * 2.0 ** -52 * float(bound[1])
        assert float(row[0]) > 0 and float(row[1]) > 0
    u2 = field((11, 9, 2), np.float64, "random", 3)
    row, bound, n = R.integrals(u2, (0.5, 0.0))
    ke = O.metric(O.zeros((11, 9), np.float64), "ke", u2, par=(0.5, 0.0))
    assert abs(float(ke[1:-1, 1:-1].astype(np.longdouble).sum() - row[0])) <= R.tolerance(bound, n)[0]


def test_slab_combination_rule():
    """series(): sums by addition in rank order, columns 4 and 5 by maximum (pure host code)"""
    from waterlily_amd import integrals as I
    rng = np.random.default_rng(5)
    parts = [rng.standard_normal((7, 9)) for _ in range(3)]
    for p in parts:
        p[:, 4:6] = np.abs(p[:, 4:6])
    v = I.combine(parts)
    for c in range(9):
        if c in (4, 5):
            assert np.array_equal(v[:, c], np.maximum(np.maximum(parts[0][:, c], parts[1][:, c]), parts[2][:, c]))
        else:
            assert np.array_equal(v[:, c], (parts[0][:, c] + parts[1][:, c]) + parts[2][:, c])
    assert np.array_equal(I.combine(parts[:1]), parts[0]) and I.combine(parts[:1]) is not parts[0]
    # a rank that owns no interior plane contributes zeros: nothing changes
    assert np.array_equal(I.combine([parts[0], np.zeros((7, 9))]), parts[0])
    # NaN in a sum surfaces, the maxima keep the number
    q = [np.ones((1, 8)), np.full((1, 8), np.nan)]
    w = I.combine(q)
    assert np.isnan(w[0, [0, 1, 2, 3, 6, 7]]).all() and np.array_equal(w[0, 4:6], [1.0, 1.0])
    assert I.combine([np.zeros((0, 8)), np.zeros((0, 8))]).shape == (0, 8)
