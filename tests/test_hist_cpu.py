"""Histogram without a GPU: the numpy restatement tests/hist_ref.py against np.histogram / np.histogramdd and the rules of the
contract by hand, what one reads off a count (waterlily_amd.hist.pdf, cdf, quantile, marginal, conditional, fraction, on torch
CPU tensors), and the argument checks of wl_histogram / wl_field_range / wl_field_range_scratch, which refuse a bad call before
they touch the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_ref as HR  # noqa: E402

from waterlily_amd import _lib, hist, render  # noqa: E402

F32, F64 = np.float32, np.float64
nan, inf = np.nan, np.inf


# --------------------------------------------------------------------------- the restatement against numpy

@pytest.mark.parametrize("T", [F32, F64])
def test_edges_mode_equals_np_histogram(T):
    rng = np.random.default_rng(17)
    v = rng.standard_normal(7400).astype(T)
    for e in (np.linspace(-2.0, 2.0, 17), np.sort(rng.standard_normal(33)), np.array([-0.3, 0.9]), np.array([-10.0, -1.0, -0.999, 0.0, 5.0])):
        vis, nn, t = HR.histogram(v, {"edges": e})
        assert vis == v.size and nn == 0 and t.shape == (e.size + 1,)
        assert np.array_equal(t[1:-1], np.histogram(v.astype(F64), bins=e)[0])
        assert t[0] == (v < e[0]).sum() and t[-1] == (v > e[-1]).sum() and t.sum() == v.size
    # the edges themselves as data: e_k opens bin k + 1, the last one closes bin n
    e = np.array([-1.0, 0.0, 0.5, 2.0])
    assert HR.bins_edges(e, e).tolist() == [1, 2, 3, 3]
    assert HR.bins_edges(np.nextafter(e, -inf), e).tolist() == [0, 1, 2, 3] and HR.bins_edges(np.nextafter(e, inf), e).tolist() == [1, 2, 3, 4]


@pytest.mark.parametrize("T", [F32, F64])
def test_uniform_mode_equals_np_histogram_on_dyadic_data(T):
    rng = np.random.default_rng(17)
    v = (np.round(rng.standard_normal(7400) * 8.0) / 8.0).astype(T)         # multiples of 1/8: every (v - lo) * scale is exact
    vis, nn, t = HR.histogram(v, {"n": 16, "lo": -2.0, "hi": 2.0})
    assert np.array_equal(t[1:-1], np.histogram(v.astype(F64), bins=16, range=(-2, 2))[0])
    assert t[0] == (v < -2).sum() > 0 and t[-1] == (v > 2).sum() > 0 and t.sum() == v.size == vis and nn == 0
    assert ((v == -2).sum() > 0) and ((v == 2).sum() > 0)                    # values on both ends of the range are among them


def test_joint_equals_np_histogramdd():
    rng = np.random.default_rng(3)
    va, vb = rng.standard_normal(5000), rng.standard_normal(5000) * 2.0
    ea, eb = np.linspace(-2, 2, 9), np.sort(rng.standard_normal(6))
    vis, nn, t = HR.histogram(va, {"edges": ea}, vb, {"edges": eb})
    H = np.histogramdd((va, vb), bins=(ea, eb))[0]
    assert t.shape == (7, 10) and np.array_equal(t[1:-1, 1:-1], H.T.astype(np.int64)) and t.sum() == 5000
    assert np.array_equal(t.sum(0), HR.histogram(va, {"edges": ea})[2]) and np.array_equal(t.sum(1), HR.histogram(vb, {"edges": eb})[2])


def test_values_on_the_range_and_on_interior_edges():
    ax = {"n": 4, "lo": -1.0, "hi": 1.0}
    v = np.array([-1.0, -0.5, 0.0, 0.5, 1.0, np.nextafter(-1.0, -inf), np.nextafter(1.0, inf), 0.4375])
    assert HR.bins_uniform(v, -1.0, 1.0, 4).tolist() == [1, 2, 3, 4, 4, 0, 5, 3]
    assert HR.histogram(v, ax)[2].tolist() == [1, 1, 1, 2, 2, 1]
    # the difference v - lo is rounded before it is scaled: the double below 0.5 is 1.5 away from -1 after rounding, and in bin 4
    assert HR.bins_uniform(np.array([np.nextafter(0.5, -inf)]), -1.0, 1.0, 4)[0] == 4
    # a scale that rounds: the bin is the truncated PRODUCT, whatever the exact quotient would be
    lo, hi, n = 0.1, 0.7, 3
    scale = F64(n) / (F64(hi) - F64(lo))
    for x in (0.3, 0.5, np.nextafter(0.3, 0), np.nextafter(0.5, 1)):
        assert HR.bins_uniform(np.array([x]), lo, hi, n)[0] == 1 + min(n - 1, int((F64(x) - F64(lo)) * scale))


def test_zero_inf_and_nan_rules():
    ax = {"n": 2, "lo": 0.0, "hi": 1.0}
    assert HR.bins_uniform(np.array([-0.0, 0.0, inf, -inf]), 0.0, 1.0, 2).tolist() == [1, 1, 3, 0]       # -0 == +0 == lo: not below it
    assert HR.bins_edges(np.array([-0.0, 0.0, inf, -inf]), [0.0, 0.5, 1.0]).tolist() == [1, 1, 3, 0]
    vis, nn, t = HR.histogram(np.array([0.25, nan, 0.75, nan]), ax)
    assert (vis, nn, t.tolist()) == (4, 2, [0, 1, 1, 0])
    va, vb = np.array([0.25, nan, 0.75, nan, 0.25]), np.array([0.25, 0.25, nan, nan, 0.75])
    vis, nn, t = HR.histogram(va, ax, vb, ax)                               # NaN in one value, in the other, in both: dropped once each
    assert (vis, nn) == (5, 3) and t.sum() == 2 and t[1, 1] == 1 and t[2, 1] == 1
    # an infinite device range: (v - lo) * 0 is 0 for finite v and NaN for v = hi = inf, which takes the last bin
    assert HR.bins_uniform(np.array([1.0, 5.0, inf]), 1.0, inf, 4).tolist() == [1, 1, 4]
    # wl_field_range
    assert HR.field_range(np.array([nan, nan]))[2:].tolist() == [0.0, 2.0] and np.isnan(HR.field_range(np.array([nan, nan]))[:2]).all()
    r = HR.field_range(np.array([0.0, -0.0, nan]))
    assert np.signbit(r[0]) and not np.signbit(r[1]) and r[0] == 0 and r[1] == 0 and r[2:].tolist() == [2.0, 1.0]
    r = HR.field_range(np.array([-0.0, -0.0]))
    assert np.signbit(r[0]) and np.signbit(r[1])
    assert HR.field_range(np.array([1.0, -inf, inf, nan]))[:].tolist() == [-inf, inf, 3.0, 1.0]


def test_degenerate_device_ranges():
    v = np.array([-1.0, 2.0, 2.0, 3.0, inf])
    assert HR.bins_uniform(v, 2.0, 2.0, 8).tolist() == [0, 1, 1, 9, 9]      # hi == lo: the value itself is in bin 1
    assert HR.bins_uniform(v, nan, nan, 8).tolist() == [9] * 5              # a NaN range: every non-NaN cell overflows
    assert HR.bins_uniform(np.array([7.0] * 5), 7.0, 7.0, 3).tolist() == [1] * 5
    vis, nn, t = HR.histogram(np.array([1.0, nan, 2.0]), {"n": 3, "lo": nan, "hi": nan})
    assert (vis, nn, t.tolist()) == (3, 1, [0, 0, 0, 0, 2])


def test_invariant_visited_is_nan_plus_bins():
    rng = np.random.default_rng(9)
    v = rng.standard_normal(3000)
    v[rng.integers(0, 3000, 100)] = nan
    w = rng.standard_normal(3000)
    w[rng.integers(0, 3000, 100)] = nan
    for a, b in (({"n": 7, "lo": -1.0, "hi": 0.5}, None), ({"n": 7, "lo": -1.0, "hi": 0.5}, {"edges": [-1.0, 0.0, 3.0]})):
        vis, nn, t = HR.histogram(v, a, w if b else None, b)
        assert vis == 3000 == nn + t.sum() and nn > 50


# --------------------------------------------------------------------------- what one reads off a count (torch, CPU)

def test_pdf_cdf_fraction_on_hand_made_counts():
    c = torch.tensor([2, 1, 3, 0, 4, 10], dtype=torch.int64)                # underflow 2, four bins, overflow 10
    e = torch.tensor([0.0, 1.0, 1.5, 3.5, 4.0], dtype=torch.float64)
    p = hist.pdf(c, e)
    assert p.dtype == torch.float64 and p.tolist() == [1 / 20, 3 / (20 * 0.5), 0.0, 4 / (20 * 0.5)]
    assert abs(float((p * (e[1:] - e[:-1])).sum()) - 8 / 20) <= 2.0 ** -50   # integrates to the in-range share (4 roundings of <= 2^-54)
    assert hist.cdf(c).tolist() == [0.1, 0.15, 0.3, 0.3, 0.5, 1.0]
    assert float(hist.fraction(c, 1, 2)) == 0.2 and float(hist.fraction(c, 0, 5)) == 1.0 and float(hist.fraction(c, 3, 3)) == 0.0


def test_quantile_on_hand_made_counts():
    c = torch.tensor([2, 1, 3, 0, 4, 10], dtype=torch.int64)
    e = [0.0, 1.0, 1.5, 3.5, 4.0]
    qs = [0.0, 0.05, 0.1, 0.125, 0.15, 0.3, 0.4, 0.5, 0.75, 1.0]
    got = hist.quantile(c, torch.tensor(e, dtype=torch.float64), qs)
    assert got.dtype == torch.float64 and got.tolist() == [HR.quantile(c.tolist(), e, q) for q in qs]
    # by hand: N = 20.  q <= 0.1: inside the underflow -> e_0; 0.125: target 2.5, bin 1 (before 2, count 1): half of it; 0.3: the top
    # of bin 2; 0.4: target 8, bin 4 (before 6, count 4): half; 0.5: the top of bin 4; beyond: inside the overflow -> e_n
    assert got.tolist() == [0.0, 0.0, 0.0, 0.5, 1.0, 1.5, 3.75, 4.0, 4.0, 4.0]
    assert float(hist.quantile(c, torch.tensor(e, dtype=torch.float64), 0.4)) == 3.75                   # a plain number for q
    # no underflow, no overflow: q = 0 is e_0, q = 1 the top of the last bin that holds a cell
    c2 = torch.tensor([0, 5, 5, 0, 0], dtype=torch.int64)
    assert hist.quantile(c2, torch.tensor([0.0, 1.0, 2.0, 3.0]), [0.0, 0.5, 0.75, 1.0]).tolist() == [0.0, 1.0, 1.5, 2.0]


def test_quantile_of_a_sample_brackets_numpy():
    rng = np.random.default_rng(1)
    v = rng.standard_normal(20000)
    e = np.linspace(-5, 5, 401)
    t = HR.histogram(v, {"edges": e})[2]
    for q in (0.01, 0.5, 0.99):
        got = float(hist.quantile(torch.from_numpy(t), torch.from_numpy(e), q))
        assert abs(got - np.quantile(v, q)) <= e[1] - e[0]                   # within one bin width of the sample's quantile


def test_marginal_and_conditional():
    t = torch.arange(12, dtype=torch.int64).view(3, 4)                       # [B, A]
    assert hist.marginal(t, "a").tolist() == [12, 15, 18, 21] and hist.marginal(t, "b").tolist() == [6, 22, 38]
    assert hist.conditional(t, 1).tolist() == [4, 5, 6, 7]
    # one interior B-bin: row 1 is the count of A over the cells with blo <= B <= bhi
    rng = np.random.default_rng(4)
    va, vb = rng.standard_normal(2000), rng.standard_normal(2000)
    a = {"n": 8, "lo": -2.0, "hi": 2.0}
    joint = HR.histogram(va, a, vb, {"edges": [-0.5, 0.25]})[2]
    keep = (vb >= -0.5) & (vb <= 0.25)
    assert np.array_equal(joint[1], HR.histogram(va[keep], a)[2]) and keep.sum() > 100


def test_gather_adds_the_ranks_parts():
    parts = [np.array([[1, 2], [3, 4]], dtype=np.int64), np.array([[10, 0], [0, 5]], dtype=np.int64), np.array([[0, 0], [7, 0]], dtype=np.int64)]
    assert hist.combine(parts).tolist() == [[11, 2], [10, 9]] and hist.combine(parts).dtype == np.int64
    assert hist.combine(parts[::-1]).tolist() == hist.combine(parts).tolist()
    assert parts[0].tolist() == [[1, 2], [3, 4]]                             # the parts are left alone
    one = torch.tensor([5, 6, 7], dtype=torch.int64)
    assert hist.gather(one).tolist() == [5, 6, 7] and hist.gather(one, None).dtype == np.int64


def test_axis_refuses_bad_bins():
    for e in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, nan, 1.0], [0.0, inf], [1.0], np.arange(1026.0)):
        with pytest.raises(ValueError):
            hist.Axis(edges=e)
    for r in ((1.0, 1.0), (2.0, 1.0), (0.0, inf), (nan, 1.0)):
        with pytest.raises(ValueError):
            hist.Axis(range=r)
    with pytest.raises(ValueError):
        hist.Axis(bins=0)
    with pytest.raises(ValueError):
        hist.Axis(range=(0, 1), edges=[0.0, 1.0])
    a = hist.Axis("lambda2", edges=np.arange(1025.0))
    assert a.bins == 1024 and a.kind == render.R_METRIC + 4 and not a.auto and hist.Axis().auto and hist.Axis().bins == 256


# --------------------------------------------------------------------------- refusals before the device is touched

def grid(D=3, n=(10, 11, 14)):
    g = _lib.Grid()
    g.D = D
    n = tuple(n[:D]) + (1,) * (3 - D)
    g.n[:] = list(n)
    g.s[:] = [1, n[0], n[0] * n[1]]
    g.sc = n[0] * n[1] * n[2]
    return g


def i3(*v):
    return (C.c_int32 * 3)(*v)


BUF = (C.c_double * 4)()                                                     # never reached
PTR = C.cast(BUF, C.c_void_p)
OM, CURL, FACE = render.R_METRIC + 2, render.R_METRIC + 1, 3


def axis(f=PTR, kind=0, ipar=0, nbins=8, lo=0.0, hi=1.0, range_dev=None, edges_dev=None):
    a = _lib.HistAxis()
    a.f, a.kind, a.ipar, a.nbins, a.lo, a.hi = f, kind, ipar, nbins, lo, hi
    a.range_dev, a.edges_dev = range_dev, edges_dev
    return a


def test_histogram_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    g3, g2 = grid(3), grid(2)

    def refused(word, g=g3, a=axis(), b=None, lo=None, hi=None, cnt=PTR, t=_lib.WL_F32):
        rc = L.wl_histogram(t, None if g is None else C.byref(g), None if a is None else C.byref(a), None if b is None else C.byref(b), lo, hi, 0, cnt)
        assert rc == _lib.WL_E_ARG, (word, rc)
        assert word in L.wl_last_error(), (word, L.wl_last_error())

    refused(b"null", g=None)
    refused(b"null", a=None)
    refused(b"null", a=axis(f=None))
    refused(b"null", cnt=None)
    refused(b"null", b=axis(f=None))
    refused(b"dtype", t=7)
    for kind in (-1, 4, 15, render.R_METRIC + 5, 99):
        refused(b"kind", a=axis(kind=kind))
        refused(b"kind", b=axis(kind=kind))
    refused(b"kind", a=axis(kind=FACE))                                      # WL_R_FACE is Downsample's alone
    refused(b"kind", a=axis(kind=1, ipar=3))
    refused(b"kind", b=axis(kind=2, ipar=-1))
    refused(b"kind", g=g2, a=axis(kind=2, ipar=2))
    refused(b"kind", g=g2, a=axis(kind=OM))                                  # omega_mag needs D == 3
    refused(b"kind", a=axis(kind=CURL, ipar=3))
    refused(b"nbins", a=axis(nbins=0))
    refused(b"nbins", b=axis(nbins=-3))
    refused(b"8192", a=axis(nbins=8191))                                     # A = 8193
    refused(b"8192", a=axis(nbins=126), b=axis(nbins=63))                    # 128 * 65 = 8320
    refused(b"1024", a=axis(nbins=1025, edges_dev=PTR))
    refused(b"both", a=axis(range_dev=PTR, edges_dev=PTR))
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (0.0, inf), (-inf, 0.0), (nan, 1.0), (0.0, nan)):
        refused(b"host range", a=axis(lo=lo, hi=hi))
        refused(b"host range", b=axis(lo=lo, hi=hi))
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"only one", hi=i3(2, 2, 2))
    refused(b"box", lo=i3(-1, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(5, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(4, 1, 1), hi=i3(4, 4, 4))                          # an empty extent
    refused(b"box", lo=i3(1, 1, 1), hi=i3(10, 4, 4))                         # hi <= n - 1
    refused(b"box", lo=i3(1, 1, 1), hi=i3(4, 4, 14))
    refused(b"inside", a=axis(kind=OM), lo=i3(0, 1, 1), hi=i3(4, 4, 4))      # a metric box outside inside(), on either axis
    refused(b"inside", b=axis(kind=OM), lo=i3(1, 1, 0), hi=i3(4, 4, 4))


def test_field_range_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    g3, g2 = grid(3), grid(2)
    nb = C.c_int64(-1)
    assert L.wl_field_range_scratch(C.byref(g3), C.byref(nb)) == 0 and nb.value > 0
    assert L.wl_field_range_scratch(None, C.byref(nb)) == _lib.WL_E_ARG and b"null" in L.wl_last_error()
    assert L.wl_field_range_scratch(C.byref(g3), None) == _lib.WL_E_ARG and b"null" in L.wl_last_error()
    bad = grid(3)
    bad.D = 4
    assert L.wl_field_range_scratch(C.byref(bad), C.byref(nb)) != 0 and b"grid.D" in L.wl_last_error()
    need = nb.value

    def refused(word, g=g3, f=PTR, kind=0, ipar=0, lo=None, hi=None, scratch=PTR, nbytes=need, out=PTR, t=_lib.WL_F64):
        rc = L.wl_field_range(t, None if g is None else C.byref(g), f, kind, ipar, None, None, 0, lo, hi, scratch, nbytes, out)
        assert rc == _lib.WL_E_ARG, (word, rc)
        assert word in L.wl_last_error(), (word, L.wl_last_error())

    refused(b"null", g=None)
    refused(b"null", f=None)
    refused(b"null", out=None)
    refused(b"dtype", t=2)
    refused(b"kind", kind=FACE)
    refused(b"kind", kind=1, ipar=3)
    refused(b"kind", g=g2, kind=OM)
    refused(b"scratch", scratch=None)
    refused(b"scratch", nbytes=need - 1)
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"box", lo=i3(4, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(1, 1, 1), hi=i3(4, 4, 14))
    refused(b"inside", kind=OM, lo=i3(0, 1, 1), hi=i3(4, 4, 4))
