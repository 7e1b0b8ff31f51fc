"""TwoPoint without a GPU: the argument checks of wl_twopoint / wl_twopoint_scratch, which refuse a bad call before they touch
the device; the scratch bytes, which are host arithmetic; what one reads off a table (waterlily_amd.twopoint.covariance,
coefficient, structure, skewness, flatness, zero_crossing, integral_scale, spectrum, on torch CPU tensors) on analytic tables;
combine; and the two evaluations of tests/twopoint_ref.py -- the contract's order in double, and an order-free one in
np.longdouble -- against each other on the inputs of the GPU tests."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twopoint_ref as TR  # noqa: E402

from waterlily_amd import _lib, render, twopoint  # noqa: E402

F32, F64 = np.float32, np.float64
U = 2.0 ** -53


def test_symbols_are_exported_and_bound():
    for n, nargs in (("wl_twopoint", 13), ("wl_twopoint_scratch", 6)):
        assert n in _lib.declared_symbols()
        fn = getattr(_lib.lib(), n)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs and fn.restype is C.c_int
    assert _lib.lib().wl_abi_version() == 6
    import waterlily_amd
    assert waterlily_amd.twopoint is twopoint and waterlily_amd.TwoPoint is twopoint.TwoPoint and waterlily_amd.Value is twopoint.Value
    assert "#define WL_TP_MAX_LINE 1024" in open(_lib.HEADER).read() and twopoint.MAX_LINE == 1024
    assert C.sizeof(_lib.TpValue) == 8 + 4 + 4 + 24 + 24


# --------------------------------------------------------------------------- refusals before the device is touched

def grid(D=3, n=(10, 11, 14)):
    g = _lib.Grid()
    g.D = D
    n = tuple(n[:D]) + (1,) * (3 - D)
    g.n[:] = list(n)
    g.s[:] = [1, n[0], n[0] * n[1]]
    g.sc = n[0] * n[1] * n[2]
    return g


def slab_grid():
    g = grid(3, (10, 11, 9))                                                 # rank 0 of 2 over 12 interior planes: 14 global planes
    g.nzg, g.kz0, g.own_lo, g.own_hi, g.zring = 14, 0, 1, 6, 0
    return g


def i3(*v):
    return (C.c_int32 * 3)(*v)


BUF = (C.c_double * 4)()                                                     # never reached
PTR = C.cast(BUF, C.c_void_p)
OM, CURL, FACE = render.R_METRIC + 2, render.R_METRIC + 1, 3
BIG = 1 << 40


def value(f=PTR, kind=0, ipar=0):
    a = _lib.TpValue()
    a.f, a.kind, a.ipar = f, kind, ipar
    return a


def test_twopoint_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    g3, g2 = grid(3), grid(2)

    def refused(word, g=g3, a=value(), b=None, axis=0, nsep=4, lo=None, hi=None, scratch=PTR, nbytes=BIG, out=PTR, t=_lib.WL_F32):
        rc = L.wl_twopoint(t, None if g is None else C.byref(g), None if a is None else C.byref(a), None if b is None else C.byref(b), axis, nsep, 0,
                           lo, hi, 0, scratch, nbytes, out)
        assert rc == _lib.WL_E_ARG, (word, rc)
        assert word in L.wl_last_error(), (word, L.wl_last_error())

    refused(b"null", g=None)
    refused(b"null", a=None)
    refused(b"null", a=value(f=None))
    refused(b"null", out=None)
    refused(b"null", b=value(f=None))
    refused(b"scratch", scratch=None)
    refused(b"dtype", t=7)
    for kind in (-1, 4, 15, render.R_METRIC + 5, 99):
        refused(b"kind", a=value(kind=kind))
        refused(b"kind", b=value(kind=kind))
    refused(b"kind", a=value(kind=FACE))                                     # WL_R_FACE is Downsample's alone
    refused(b"kind", b=value(kind=FACE))
    refused(b"kind", a=value(kind=1, ipar=3))
    refused(b"kind", b=value(kind=2, ipar=-1))
    refused(b"kind", g=g2, a=value(kind=2, ipar=2))
    refused(b"kind", g=g2, a=value(kind=OM))                                 # omega_mag needs D == 3
    refused(b"kind", a=value(kind=CURL, ipar=3))
    for axis in (-1, 3):
        refused(b"axis", axis=axis)
    refused(b"axis", g=g2, axis=2)
    for axis, n in ((0, 8), (1, 9), (2, 12)):                                # inside() of (10, 11, 14)
        refused(b"nsep", axis=axis, nsep=0)
        refused(b"nsep", axis=axis, nsep=-1)
        refused(b"nsep", axis=axis, nsep=n + 1)
    refused(b"nsep", nsep=4, lo=i3(2, 1, 1), hi=i3(5, 4, 4))                 # the box's extent, not the grid's
    refused(b"WL_TP_MAX_LINE", g=grid(2, (1030, 6)), nsep=4)                 # n = 1028
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"only one", hi=i3(2, 2, 2))
    refused(b"box", lo=i3(-1, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(5, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(4, 1, 1), hi=i3(4, 4, 4))                          # an empty extent
    refused(b"box", lo=i3(1, 1, 1), hi=i3(10, 4, 4))                         # hi <= n - 1
    refused(b"box", lo=i3(1, 1, 1), hi=i3(5, 4, 14))
    refused(b"inside", a=value(kind=OM), lo=i3(0, 1, 1), hi=i3(4, 4, 4))     # a metric box outside inside(), of either value
    refused(b"inside", b=value(kind=OM), lo=i3(1, 1, 0), hi=i3(5, 4, 4))
    need = C.c_int64()
    assert L.wl_twopoint_scratch(C.byref(g3), 0, 4, None, None, C.byref(need)) == 0
    refused(b"scratch", nbytes=need.value - 1)
    refused(b"scratch", nbytes=0)
    refused(b"axis 2", g=slab_grid(), axis=2)                                # the lines cross ranks
    gs = slab_grid()
    assert L.wl_twopoint_scratch(C.byref(gs), 2, 4, None, None, C.byref(need)) == _lib.WL_E_ARG and b"axis 2" in L.wl_last_error()
    assert L.wl_twopoint_scratch(C.byref(gs), 1, 4, None, None, C.byref(need)) == 0


def test_scratch_is_host_arithmetic():
    L = _lib.lib()
    nb = C.c_int64(-1)

    def scratch(g, axis, nsep, lo=None, hi=None):
        assert L.wl_twopoint_scratch(C.byref(g), axis, nsep, lo, hi, C.byref(nb)) == 0, L.wl_last_error()
        return nb.value

    def want(nlines, n, nsep):
        return 4 * TR.launch(nlines, n)[2] * 9 * nsep * 8

    g3 = grid(3)                                                             # inside(): 8 x 9 x 12
    assert scratch(g3, 0, 8) == want(9 * 12, 8, 8) == 4 * 7 * 9 * 8 * 8
    assert scratch(g3, 1, 3) == want(8 * 12, 9, 3) and scratch(g3, 2, 12) == want(8 * 9, 12, 12)
    assert scratch(g3, 0, 2, i3(3, 2, 1), i3(9, 10, 13)) == want(8 * 12, 6, 2)
    big = grid(3, (514, 514, 514))                                           # 512^3: L = 4, the cap of 512 workgroups
    assert scratch(big, 2, 256) == 2048 * 9 * 256 * 8 and TR.launch(512 * 512, 512) == (4, 65536, 512)
    g2 = grid(2, (300, 40))                                                  # n = 298: L = 8
    assert scratch(g2, 0, 298) == want(38, 298, 298) == 4 * 5 * 9 * 298 * 8
    assert scratch(slab_grid(), 0, 8) == want(9 * 6, 8, 8)                   # a rank's own planes (global 1..6)
    assert L.wl_twopoint_scratch(None, 0, 4, None, None, C.byref(nb)) == _lib.WL_E_ARG and b"null" in L.wl_last_error()
    assert L.wl_twopoint_scratch(C.byref(g3), 0, 4, None, None, None) == _lib.WL_E_ARG and b"null" in L.wl_last_error()
    assert L.wl_twopoint_scratch(C.byref(g3), 3, 4, None, None, C.byref(nb)) == _lib.WL_E_ARG and b"axis" in L.wl_last_error()
    assert L.wl_twopoint_scratch(C.byref(g3), 0, 9, None, None, C.byref(nb)) == _lib.WL_E_ARG and b"nsep" in L.wl_last_error()


# --------------------------------------------------------------------------- what one reads off a table (torch, CPU)

def cosine_table(n, m, lines=3):
    """the periodic auto table, nsep = n, of `lines` equal lines cos(2 pi m i / n), by the ref"""
    A = np.tile(TR.cosine(n, m), (lines, 1))
    return torch.from_numpy(TR.twopoint(A, A, n, True))


cosine_tol = TR.cosine_tol


def test_cosine_line_gives_its_covariance_spectrum_and_integral_scale():
    n, m = 64, 2
    tab = cosine_table(n, m)
    r = torch.arange(n, dtype=torch.float64)
    tol = cosine_tol(n, m)
    cov = twopoint.covariance(tab)
    assert cov.dtype == torch.float64 and cov.shape == (n,) and float((cov - 0.5 * torch.cos(2 * math.pi * m * r / n)).abs().max()) <= tol
    rho = twopoint.coefficient(tab)
    assert float((rho - torch.cos(2 * math.pi * m * r / n)).abs().max()) <= 4 * tol and abs(float(rho[0]) - 1.0) <= 4 * tol      # C over 1/2 (+- tol)
    # the spectrum: every P[k] is a mean of C(r) cos(..), so it moves by at most the largest error of C, and the FFT's own error is
    # a few log2(n) u times the root-mean-square of its input (Higham 24.1): below 8 log2(n) u here.  One-sided doubles both.
    E = twopoint.spectrum(tab, n)
    etol = 2.0 * (tol + 8.0 * math.log2(n) * U)
    want = torch.zeros(n // 2 + 1, dtype=torch.float64)
    want[m] = 0.5
    assert E.shape == (n // 2 + 1,) and float((E - want).abs().max()) <= etol
    assert abs(float(E.sum()) - float(cov[0])) <= (n // 2 + 1) * 2.0 * 8.0 * math.log2(n) * U        # the inverse transform at r = 0
    # rho first reaches zero at r = n / (4 m) = 8; the chord's crossing moves by the error of rho over the slope |rho(7)| = sin(2 pi m / n)
    slope = math.sin(2 * math.pi * m / n)
    assert abs(float(twopoint.zero_crossing(tab)) - n / (4 * m)) <= 2 * 4 * tol / slope
    # the trapezoid rule of cos(k theta), k = 0 .. K with K theta = pi / 2, is cot(theta / 2) / 2: K + 1 values, each off by 4 tol
    theta = 2 * math.pi * m / n
    Lint = float(twopoint.integral_scale(tab))
    assert abs(Lint - 0.5 / math.tan(theta / 2)) <= (n / (4 * m) + 2) * 4 * tol
    assert abs(Lint - n / (2 * math.pi * m)) <= n / (2 * math.pi * m) * theta ** 2 / 12 * 1.01       # ... which is the integral to O(theta^2)
    # odd n: no Nyquist mode; the variance is still all in mode m
    n, m = 45, 3
    tab = cosine_table(n, m, lines=1)
    E = twopoint.spectrum(tab, n)
    assert E.shape == (23,) and abs(float(E[m]) - 0.5) <= 2.0 * (cosine_tol(n, m) + 8.0 * math.log2(n) * U) and float(E.abs().sum() - E[m].abs()) <= 23 * 2.0 * (cosine_tol(n, m) + 8.0 * math.log2(n) * U)


def test_spectrum_refuses_what_is_not_the_periodic_auto_covariance_of_the_whole_line():
    tab = cosine_table(16, 1, lines=1)
    with pytest.raises(ValueError):
        twopoint.spectrum(tab)                                               # a plain table does not say what n is
    with pytest.raises(ValueError):
        twopoint.spectrum(tab[:8], 16)                                       # nsep != n
    for attr in ("tp_periodic", "tp_auto"):
        t = tab.clone()
        t.tp_n, t.tp_periodic, t.tp_auto = 16, True, True
        assert twopoint.spectrum(t).shape == (9,)
        setattr(t, attr, False)
        with pytest.raises(ValueError):
            twopoint.spectrum(t)


def test_uncorrelated_table_has_no_coefficient_beyond_zero():
    # N = 8 pairs at every r, both means 1/2, both variances 1/4; <ab> = 1/2 at r = 0 and 1/4 = <a><b> beyond: all exact in double
    tab = torch.zeros(5, 10, dtype=torch.float64)
    tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3], tab[:, 4], tab[:, 5] = 8.0, 4.0, 4.0, 4.0, 4.0, 2.0
    tab[0, 5] = 4.0
    assert twopoint.covariance(tab).tolist() == [0.25, 0.0, 0.0, 0.0, 0.0]
    assert twopoint.coefficient(tab).tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert float(twopoint.zero_crossing(tab)) == 1.0 and float(twopoint.integral_scale(tab)) == 0.5      # the triangle under the first chord
    pos = tab.clone()
    pos[:, 5] = torch.tensor([4.0, 3.0, 3.0, 2.5, 2.5])                     # rho = 1, 1/2, 1/2, 1/4, 1/4: never zero
    assert twopoint.coefficient(pos).tolist() == [1.0, 0.5, 0.5, 0.25, 0.25]
    assert float(twopoint.zero_crossing(pos)) == 4.0 and float(twopoint.integral_scale(pos)) == 0.75 + 0.5 + 0.375 + 0.25


def test_structure_skewness_flatness_on_a_hand_made_table():
    tab = torch.zeros(2, 10, dtype=torch.float64)
    tab[:, 0] = 4.0
    tab[1, 6:] = torch.tensor([16.0, -8.0, 256.0, 40.0])                    # <d^2> = 4, <d^3> = -2, <d^4> = 64, <|d|^3> = 10
    assert twopoint.structure(tab, 2).tolist() == [0.0, 4.0] and twopoint.structure(tab, 3).tolist() == [0.0, -2.0]
    assert twopoint.structure(tab, 4).tolist() == [0.0, 64.0] and twopoint.structure(tab, "abs3").tolist() == [0.0, 10.0]
    assert float(twopoint.skewness(tab)[1]) == -0.25 and float(twopoint.flatness(tab)[1]) == 4.0
    assert math.isnan(float(twopoint.skewness(tab)[0])) and math.isnan(float(twopoint.flatness(tab)[0]))
    with pytest.raises(ValueError):
        twopoint.structure(tab, 5)


def test_combine_adds_in_rank_order():
    parts = [np.array([[1.0, 2.0 ** 53]]), np.array([[2.0, 1.0]]), np.array([[3.0, -(2.0 ** 53)]])]
    assert twopoint.combine(parts).tolist() == [[6.0, 0.0]]                  # (2^53 + 1) rounds to 2^53: the order shows
    assert twopoint.combine(parts[::-1]).tolist() == [[6.0, 1.0]]
    assert parts[0].tolist() == [[1.0, 2.0 ** 53]]                           # the parts are left alone
    one = torch.tensor([[5.0, 6.0]], dtype=torch.float64)
    assert twopoint.gather(one).tolist() == [[5.0, 6.0]] and twopoint.gather(one, None).dtype == F64


def test_value_and_kinds():
    v = twopoint.Value("lambda2")
    assert v.kind == render.R_METRIC + 4 and twopoint.Value().kind == 0 and twopoint.Value("centre", i=2).i == 2
    with pytest.raises(KeyError):
        twopoint.Value("face")


# --------------------------------------------------------------------------- the ref's two evaluations

def test_pair_rule_and_columns_by_hand():
    A = np.array([[1.0, 2.0, 4.0]])
    B = np.array([[0.5, 1.0, -1.0]])
    t = TR.twopoint(A, B, 3, False)
    assert t[:, 0].tolist() == [3.0, 2.0, 1.0]
    assert t[1].tolist() == [2.0, 3.0, 0.0, 5.0, 2.0, -1.0, 9.0, -27.0, 81.0, 27.0]      # pairs (1, 1), (2, -1): d = 0, -3
    assert t[2].tolist() == [1.0, 1.0, -1.0, 1.0, 1.0, -1.0, 4.0, -8.0, 16.0, 8.0]       # the pair (1, -1)
    t = TR.twopoint(A, B, 3, True)
    assert t[:, 0].tolist() == [3.0, 3.0, 3.0]
    assert t[2, 1:6].tolist() == [7.0, 0.5, 21.0, 2.25, -1.0 + 1.0 + 4.0]                # pairs (1, -1), (2, 0.5), (4, 1): the wrap
    assert TR.launch(64, 72) == (16, 4, 4) and TR.launch(16632, 8) == (16, 1040, 512) and TR.launch(10, 300)[0] == 8 and TR.launch(10, 512)[0] == 4
    w = TR.wave_lines(38, 8)                                                 # 3 rounds, 3 workgroups; the last round is short
    assert w.shape == (12, 4) and w[0].tolist() == [0, 4, 8, 12] and w[11].tolist() == [35, -1, -1, -1] and w[8].tolist() == [32, 36, -1, -1]
    assert sorted(q for q in w.reshape(-1) if q >= 0) == list(range(38))
    assert TR.wave_lines(34, 8)[10:].tolist() == [[-1] * 4] * 2              # wavefronts without a line: their sums are +0
    w = TR.wave_lines(16 * 512 + 20, 8)                                      # more rounds than workgroups: workgroup 0 takes rounds 0 and 512
    assert w.shape[0] == 2048 and w[1].tolist() == [1, 5, 9, 13, 8193, 8197, 8201, 8205] and w[4].tolist()[:5] == [16, 20, 24, 28, 8208]


@pytest.mark.parametrize("shape", [(72, 8, 8), (8, 72, 8), (8, 8, 72), (40, 24), (72, 8)], ids=lambda s: "x".join(map(str, s)))
def test_ordered_and_order_free_evaluations_agree(shape):
    """|ordered - exact| <= N * 2^-53 * sum |term| for every entry: the bound holds for ANY order of adding N doubles."""
    D = len(shape)
    p, u = TR.fields(shape, F32)[:2]
    lo, hi = (1,) * D, tuple(n + 1 for n in shape)
    axis = int(np.argmax(shape))
    A = TR.lines(TR.values(p, "scalar", 0, lo, hi), axis)
    B = TR.lines(TR.values(u, "centre", 0, lo, hi), axis)
    for periodic in (False, True):
        for a, b in ((A, A), (A, B)):
            t = TR.twopoint(a, b, shape[axis], periodic)
            ex, mag = TR.exact(a, b, shape[axis], periodic)
            assert np.array_equal(t[:, 0], ex[:, 0].astype(F64)) and (np.abs(t.astype(TR.LD) - ex) <= TR.bound(ex, mag)).all()
            assert (mag[1:, 1:] > 0).all() and (mag[0, 1:6] > 0).all()              # (r = 0 of an auto table: every increment is 0)
