"""TwoPoint on the GPU (waterlily_amd.twopoint: wl_twopoint) against the numpy restatement tests/twopoint_ref.py: all ten columns
equal as uint64 views, in the contract's order, and within the order-free bound N * 2^-53 * sum |term| of a np.longdouble sum.

Interior shapes: (72, 8, 8), (8, 72, 8), (8, 8, 72) -- a line of 64 + 8 cells along each axis, so that with nsep = 72 the second
group of 64 separations is partial; the 2-D (40, 24) and (72, 8); MANY = (8, 132, 126), see test_more_rounds_than_workgroups;
and the 2-D lines of 264, 520 and 1024 cells at which a round has 8 and 4 lines and the staged lines lose their pad.  Float32
and Float64, padded and dense; fields are seeded standard_normal, ghost cells included, and a copy rounded to multiples of 1/8.
Every shape runs on inside() and on a box that starts at (3, 2, 1), every axis, periodic and not.  A table of nsep rows is the
first nsep rows of the table of n rows (a separation's sums do not depend on the others), so one reference of n rows serves
nsep = 1, 5, 64, 65 and n.

Why equality: every term is a fixed sequence of IEEE double operations, each rounded on its own (the library is built without
contraction), and the order of every sum is in the contract.  The metric kinds call the device function wl_metric's kernel
calls, so the yardstick for them is the host copy of what wl_metric stored for the same u.  The two-rank run through a worker
is left out: starting the ranks takes longer than a test may here; test_slab_rule_with_two_ranks_emulated_in_one_process holds
the slab rule instead.
"""
import ctypes as C
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import twopoint_ref as TR  # noqa: E402

from waterlily_amd import _lib, twopoint, sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402
from waterlily_amd.dist import Slab  # noqa: E402
from waterlily_amd.twopoint import TwoPoint, Value  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [(72, 8, 8), (8, 72, 8), (8, 8, 72), (40, 24), (72, 8)]
CASES = [(sh, T, pad) for sh in SHAPES for T in (F32, F64) for pad in (True, False)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for sh, T, pad in CASES]
MANY = (8, 132, 126)
NSEPS = (1, 5, 64, 65)


def make(shape, T, padded, dyadic=False):
    flow = S.Flow(shape, (0.0,) * len(shape), T=T, padded=padded)
    p, u, p8, u8 = TR.fields(shape, T)
    p, u = (p8, u8) if dyadic else (p, u)
    S.upload(flow.p, p)
    S.upload(flow.u, u)
    return flow, p, u


def host(x):
    return x.cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F64)).view(np.uint64)


def boxes(D):
    return [None, (3, 2, 1)[:D]]


def lohi(start, shape):
    return ((1,) * len(shape) if start is None else tuple(start)), tuple(n + 1 for n in shape)


def box_of(start, shape):
    return None if start is None else lohi(start, shape)


@functools.lru_cache(maxsize=None)
def ref_lines(shape, T, dyadic, kind, c, start, axis):
    p, u, p8, u8 = TR.fields(shape, T)
    f = (p8 if dyadic else p) if kind == "scalar" else (u8 if dyadic else u)
    lo, hi = lohi(start, shape)
    return TR.lines(TR.values(f, kind, c, lo, hi), axis)


@functools.lru_cache(maxsize=None)
def ref_ordered(shape, T, ka, kb, start, axis, periodic):
    """the table of n rows in the contract's order, normal data; ka, kb: (kind, c)"""
    A, B = ref_lines(shape, T, False, ka[0], ka[1], start, axis), ref_lines(shape, T, False, kb[0], kb[1], start, axis)
    t = TR.twopoint(A, B, A.shape[1], periodic)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def ref_exact(shape, T, dyadic, ka, kb, start, axis, periodic):
    A, B = ref_lines(shape, T, dyadic, ka[0], ka[1], start, axis), ref_lines(shape, T, dyadic, kb[0], kb[1], start, axis)
    return TR.exact(A, B, A.shape[1], periodic)


@functools.lru_cache(maxsize=None)
def ref_dyadic(shape, T, ka, start, axis, periodic):
    A = ref_lines(shape, T, True, ka[0], ka[1], start, axis)
    return TR.dyadic(A, A, A.shape[1], periodic)


def within_bound(got, ex, mag):
    return bool((np.abs(got.astype(TR.LD) - ex[:got.shape[0]]) <= TR.bound(ex, mag)[:got.shape[0]]).all())


def kinds(D):
    return [("scalar", 0)] + [(k, c) for k in ("ucomp", "centre") for c in range(D)]


def field_of(flow, kind):
    return flow.p if kind == "scalar" else flow.u


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_dyadic_data_plain_kinds_every_column_exact(shape, T, padded):
    """Multiples of 1/8 (1/16 for centre) bounded by about 5: a term is at most 10^4 < 2^14 with 16 fractional bits and there are
    at most 72 * 64 < 2^13 of them, so every term and every partial sum is exact in double, in any order: 46 bits at most
    (TR.dyadic forms the same sums in int64 and checks the size).  This holds the pair sets, the wrap, N(r) and the formulas,
    whatever the order."""
    D = len(shape)
    flow, p, u = make(shape, T, padded, dyadic=True)
    n_calls = 0
    for start in boxes(D):
        lo, hi = lohi(start, shape)
        for axis in range(D):
            n = hi[axis] - lo[axis]
            for periodic in (False, True):
                for kind, c in kinds(D):
                    ex = ref_dyadic(shape, T, (kind, c), start, axis, periodic)
                    tp = TwoPoint(flow, Value(kind, i=c), axis=axis, periodic=periodic, box=box_of(start, shape))
                    assert tp.nsep == tp.n == n
                    got = host(twopoint.measure(tp, field_of(flow, kind)))
                    assert got.shape == (n, 10) and got.dtype == F64
                    assert np.array_equal(bits(got), bits(ex)), (kind, c, start, axis, periodic)
                    n_calls += 1
                for nsep in [s for s in NSEPS if s < n]:
                    ex = ref_dyadic(shape, T, ("scalar", 0), start, axis, periodic)
                    got = host(twopoint.measure(TwoPoint(flow, Value(), axis=axis, nsep=nsep, periodic=periodic, box=box_of(start, shape)), flow.p))
                    assert got.shape == (nsep, 10) and np.array_equal(bits(got), bits(ex[:nsep])), (nsep, start, axis, periodic)
    assert n_calls == 2 * D * 2 * (1 + 2 * D)


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_normal_data_equals_the_ordered_ref_and_lies_within_the_order_free_bound(shape, T, padded):
    D = len(shape)
    flow, p, u = make(shape, T, padded)
    for start in boxes(D):
        lo, hi = lohi(start, shape)
        for axis in range(D):
            n = hi[axis] - lo[axis]
            for periodic in (False, True):
                for ka in (("scalar", 0), ("centre", axis), ("ucomp", (axis + 1) % D)):
                    want = ref_ordered(shape, T, ka, ka, start, axis, periodic)
                    ex, mag = ref_exact(shape, T, False, ka, ka, start, axis, periodic)
                    for nsep in [s for s in NSEPS if s < n] + [n] if ka[0] == "scalar" else [n]:
                        tp = TwoPoint(flow, Value(ka[0], i=ka[1]), axis=axis, nsep=nsep, periodic=periodic, box=box_of(start, shape))
                        got = host(twopoint.measure(tp, field_of(flow, ka[0])))
                        assert np.array_equal(bits(got), bits(want[:nsep])), (ka, start, axis, periodic, nsep)
                        assert within_bound(got, ex, mag), (ka, start, axis, periodic, nsep)


@pytest.mark.parametrize("shape,T,padded", CASES[::3], ids=IDS[::3])
def test_metric_kinds_equal_wl_metric(shape, T, padded):
    D = len(shape)
    flow, p, u = make(shape, T, padded)
    scratch = S.like(flow.p)
    for kind, c in ((("omega_mag", 0), ("lambda2", 0)) if D == 3 else (("curl", 2),)):
        scratch.zero_()
        m = S.to_host(S.metric(scratch, kind, flow.u, c))     # what the existing wl_metric stores
        assert np.isfinite(m).all() and m[(slice(1, -1),) * D].std() > 0
        for start in boxes(D):
            lo, hi = lohi(start, shape)
            for axis in range(D):
                A = TR.lines(TR.values(m, "scalar", 0, lo, hi), axis)
                P = TR.lines(TR.values(p, "scalar", 0, lo, hi), axis)
                for periodic in (False, True):
                    tp = TwoPoint(flow, Value(kind, i=c), axis=axis, periodic=periodic, box=box_of(start, shape))
                    assert np.array_equal(bits(host(twopoint.measure(tp, flow.u))), bits(TR.twopoint(A, A, A.shape[1], periodic))), (kind, start, axis, periodic)
                # metric x plain and plain x metric: the second staged value
                tp = TwoPoint(flow, Value(kind, i=c), Value("scalar"), axis=axis, nsep=5, box=box_of(start, shape))
                assert np.array_equal(bits(host(twopoint.measure(tp, flow.u, flow.p))), bits(TR.twopoint(A, P, 5, False))), (kind, start, axis)
                tp = TwoPoint(flow, Value("scalar"), Value(kind, i=c), axis=axis, nsep=5, periodic=True, box=box_of(start, shape))
                assert np.array_equal(bits(host(twopoint.measure(tp, flow.p, flow.u))), bits(TR.twopoint(P, A, 5, True))), (kind, start, axis)
    if D == 3:                                                 # metric x metric
        lo, hi = lohi(None, shape)
        mo, ml = (S.to_host(S.metric(scratch, k, flow.u)) for k in ("omega_mag", "lambda2"))
        A, B = TR.lines(TR.values(ml, "scalar", 0, lo, hi), 1), TR.lines(TR.values(mo, "scalar", 0, lo, hi), 1)
        tp = TwoPoint(flow, Value("lambda2"), Value("omega_mag"), axis=1)
        assert np.array_equal(bits(host(twopoint.measure(tp, flow.u))), bits(TR.twopoint(A, B, A.shape[1], False)))


@pytest.mark.parametrize("shape,T,padded", CASES[1::4], ids=IDS[1::4])
def test_a_second_value(shape, T, padded):
    D = len(shape)
    flow, p, u = make(shape, T, padded)
    ka, kb = ("scalar", 0), ("centre", 0)
    for start in boxes(D):
        for axis in range(D):
            for periodic in (False, True):
                want = ref_ordered(shape, T, ka, kb, start, axis, periodic)
                assert all(not np.array_equal(want[:, 1 + q], want[:, 2 + q]) for q in (0, 2)) and not np.array_equal(want[:, 5], want[:, 3])
                tp = TwoPoint(flow, Value(), Value("centre", i=0), axis=axis, periodic=periodic, box=box_of(start, shape))
                got = host(twopoint.measure(tp, flow.p, flow.u))
                assert np.array_equal(bits(got), bits(want)), (start, axis, periodic)                   # columns 1..5 tell a from b
                assert within_bound(got, *ref_exact(shape, T, False, ka, kb, start, axis, periodic))
                # b == NULL gives the bits of b = a passed explicitly
                one = host(twopoint.measure(TwoPoint(flow, Value("centre", i=0), axis=axis, periodic=periodic, box=box_of(start, shape)), flow.u))
                two = host(twopoint.measure(TwoPoint(flow, Value("centre", i=0), Value("centre", i=0), axis=axis, periodic=periodic, box=box_of(start, shape)), flow.u, flow.u))
                assert np.array_equal(bits(one), bits(two)) and np.array_equal(bits(one), bits(ref_ordered(shape, T, kb, kb, start, axis, periodic)))
    with pytest.raises(ValueError):
        twopoint.measure(TwoPoint(flow, Value()), flow.p, flow.u)             # a second field without a second Value
    with pytest.raises(ValueError):
        twopoint.measure(TwoPoint(flow, Value("ucomp")), flow.p)              # a component of a scalar field
    with pytest.raises(ValueError):
        TwoPoint(flow, Value(), axis=D)
    with pytest.raises(ValueError):
        TwoPoint(flow, Value(), axis=0, nsep=shape[0] + 1)


@pytest.mark.parametrize("T", [F32, F64])
def test_accumulate_adds_once_and_a_plain_call_overwrites(T):
    shape = (72, 8, 8)
    flow, p, u = make(shape, T, True)
    p8 = TR.fields(shape, T)[2]
    other = S.like(flow.p)
    S.upload(other, np.asarray(p8) * T(3) + np.asarray(p))
    for axis, periodic in ((0, False), (2, True)):
        tp = TwoPoint(flow, Value(), axis=axis, periodic=periodic)
        new = host(twopoint.measure(tp, other))
        old = host(twopoint.measure(tp, flow.p))
        assert not np.array_equal(old, new)
        got = host(twopoint.measure(tp, other, accumulate=True))
        assert np.array_equal(bits(got), bits(old + new)) and np.array_equal(got[:, 0], 2 * old[:, 0])
        got = host(twopoint.measure(tp, other, accumulate=True))
        assert np.array_equal(bits(got), bits((old + new) + new))
        assert np.array_equal(bits(host(twopoint.measure(tp, flow.p))), bits(old))      # overwrites


def test_one_nan_cell_reaches_the_rows_and_columns_that_read_it():
    shape, T = (72, 8, 8), F64
    flow, p, u = make(shape, T, True)
    pn = np.array(p)
    pn[11, 4, 3] = np.nan                                      # cell 10 of its line along x
    S.upload(flow.p, pn)
    lo, hi = lohi(None, shape)
    A = TR.lines(TR.values(pn, "scalar", 0, lo, hi), 0)
    a_cols, b_cols, both = [1, 3, 5, 6, 7, 8, 9], [2, 4, 5, 6, 7, 8, 9], list(range(1, 10))
    for periodic in (False, True):
        got = host(twopoint.measure(TwoPoint(flow, Value(), axis=0, periodic=periodic), flow.p))
        want = TR.twopoint(A, A, 72, periodic)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(bits(got[~np.isnan(got)]), bits(want[~np.isnan(want)]))
        assert np.array_equal(got[:, 0], TR.count(64, 72, 72, periodic))                # N(r) is untouched
        for r in range(72):
            as_a, as_b = periodic or 10 + r < 72, periodic or r <= 10                    # the pair (10, 10 + r); the pair (10 - r, 10)
            cols = both if (as_a and as_b) else (a_cols if as_a else (b_cols if as_b else []))
            assert np.flatnonzero(np.isnan(got[r])).tolist() == cols, (periodic, r)
    got = host(twopoint.measure(TwoPoint(flow, Value(), axis=1), flow.p))  # along y the cell is in ONE line of 8: every row that has a pair with it
    assert np.array_equal(np.isnan(got), np.isnan(TR.twopoint(TR.lines(TR.values(pn, "scalar", 0, lo, hi), 1), TR.lines(TR.values(pn, "scalar", 0, lo, hi), 1), 8, False)))
    assert np.isnan(got[:5, 1]).all() and not np.isnan(got[5:, 1]).any()               # cell 3 of 8 is an `a` for r <= 4


@pytest.mark.parametrize("T", [F32, F64])
def test_two_calls_give_equal_bits(T):
    flow, p, u = make((8, 72, 8), T, True)
    for tp, fields in ((TwoPoint(flow, Value("lambda2"), axis=1, periodic=True), (flow.u,)),
                       (TwoPoint(flow, Value(), Value("centre", i=2), axis=2), (flow.p, flow.u))):
        one = host(twopoint.measure(tp, *fields))
        tp._tab.tensor(torch.float64, flow.device).fill_(-1.0)
        tp._scratch.tensor(torch.float64, flow.device).fill_(-1.0)
        two = host(twopoint.measure(tp, *fields))
        assert np.array_equal(bits(one), bits(two)) and np.isfinite(one).all()


@pytest.mark.parametrize("shape,axis,m", [((72, 8, 8), 0, 3), ((8, 8, 72), 2, 6), ((40, 24), 1, 2)], ids=["x", "z", "y-2d"])
def test_cosine_along_the_axis_through_measure_and_the_host_functions_on_the_device(shape, axis, m):
    D, n = len(shape), shape[axis]
    flow = S.Flow(shape, (0.0,) * D, T=F64)
    line = TR.cosine(n, m)
    full = np.zeros(tuple(s + 2 for s in shape))
    sl = [None] * D
    sl[axis] = slice(None)
    full[(slice(1, -1),) * D] = line[tuple(sl)]
    S.upload(flow.p, np.asfortranarray(full))
    tab = twopoint.measure(TwoPoint(flow, Value(), axis=axis, periodic=True), flow.p)
    assert tab.is_cuda and tab.shape == (n, 10) and tab.tp_n == n
    lo, hi = lohi(None, shape)
    A = TR.lines(TR.values(full, "scalar", 0, lo, hi), axis)
    assert within_bound(host(tab), *TR.exact(A, A, n, True))
    tol = TR.cosine_tol(n, m)                                  # (holds for ANY order of the sums, so for N lines as for one)
    r = np.arange(n)
    cov = twopoint.covariance(tab)
    assert cov.is_cuda and np.abs(host(cov) - 0.5 * np.cos(2 * np.pi * m * r / n)).max() <= tol
    E = twopoint.spectrum(tab)
    etol = 2.0 * (tol + 8.0 * math.log2(n) * 2.0 ** -53)       # (tests/test_twopoint_cpu.py derives it)
    want = np.zeros(n // 2 + 1)
    want[m] = 0.5
    assert E.is_cuda and E.shape == (n // 2 + 1,) and np.abs(host(E) - want).max() <= etol
    assert abs(float(E.sum()) - float(cov[0])) <= (n // 2 + 1) * 2.0 * 8.0 * math.log2(n) * 2.0 ** -53
    slope = math.sin(2 * math.pi * m / n)                      # |rho| one cell before the crossing at n / (4 m)
    assert abs(float(twopoint.zero_crossing(tab)) - n / (4 * m)) <= 2 * 4 * tol / slope and n % (4 * m) == 0
    with pytest.raises(ValueError):
        twopoint.spectrum(twopoint.measure(TwoPoint(flow, Value(), axis=axis), flow.p))                 # not periodic
    with pytest.raises(ValueError):
        twopoint.spectrum(twopoint.measure(TwoPoint(flow, Value(), axis=axis, nsep=n - 1, periodic=True), flow.p))


@pytest.mark.parametrize("T", [F32, F64])
def test_more_rounds_than_workgroups(T):
    """The launch is capped at 512 workgroups of 4 wavefronts (TP_WG in csrc/wl_twopoint.h) and a round is 16 lines of up to 255
    cells.  Along x MANY has 132 * 126 = 16632 lines, 1040 rounds: more than twice 512 * 16 lines, so every workgroup takes two
    or three rounds and every wavefront 8 to 12 lines, with its sums at rest in the scratch in between."""
    flow, p, u = make(MANY, T, True)
    lo, hi = lohi(None, MANY)
    assert TR.launch(132 * 126, 8) == (16, 1040, 512) and 132 * 126 > 2 * 512 * 16
    A = TR.lines(TR.values(p, "scalar", 0, lo, hi), 0)
    B = TR.lines(TR.values(u, "centre", 1, lo, hi), 0)
    for periodic in (False, True):
        got = host(twopoint.measure(TwoPoint(flow, Value(), axis=0, periodic=periodic), flow.p))
        assert np.array_equal(bits(got), bits(TR.twopoint(A, A, 8, periodic))) and within_bound(got, *TR.exact(A, A, 8, periodic))
    got = host(twopoint.measure(TwoPoint(flow, Value(), Value("centre", i=1), axis=0, nsep=5), flow.p, flow.u))
    assert np.array_equal(bits(got), bits(TR.twopoint(A, B, 5, False)))
    scratch = S.like(flow.p)
    Lm = TR.lines(TR.values(S.to_host(S.metric(scratch, "lambda2", flow.u)), "scalar", 0, lo, hi), 0)
    got = host(twopoint.measure(TwoPoint(flow, Value("lambda2"), axis=0, periodic=True), flow.u))
    assert np.array_equal(bits(got), bits(TR.twopoint(Lm, Lm, 8, True)))


@pytest.mark.parametrize("shape,T", [((264, 6), F32), ((520, 5), F64), ((1024, 3), F32)], ids=["264-8-lines", "520-4-lines", "1024-no-pad"])
def test_long_lines_take_rounds_of_8_and_of_4_lines(shape, T):
    """n = 264: 8 lines a round; 520: 4; 1024 = WL_TP_MAX_LINE: 4 lines without the pad, and with a second value the whole 64 KB."""
    flow, p, u = make(shape, T, True)
    n = shape[0]
    lo, hi = lohi(None, shape)
    assert TR.launch(shape[1], n)[0] == (8 if n == 264 else 4)
    A = TR.lines(TR.values(p, "scalar", 0, lo, hi), 0)
    B = TR.lines(TR.values(u, "centre", 1, lo, hi), 0)
    got = host(twopoint.measure(TwoPoint(flow, Value(), Value("centre", i=1), axis=0, periodic=True), flow.p, flow.u))
    assert got.shape == (n, 10) and np.array_equal(bits(got), bits(TR.twopoint(A, B, n, True)))
    got = host(twopoint.measure(TwoPoint(flow, Value(), axis=0, nsep=n - 3), flow.p))
    assert np.array_equal(bits(got), bits(TR.twopoint(A, A, n - 3, False)))
    with pytest.raises(ValueError):
        TwoPoint(S.Flow((1025, 3), (0.0, 0.0), T=T), Value(), axis=0)


@pytest.mark.parametrize("T", [F32, F64])
def test_slab_rule_with_two_ranks_emulated_in_one_process(T):
    """wl_twopoint on the z-slab descriptors of 2 ranks, each pointed at its planes of ONE undecomposed array: along x and y a rank
    sums the lines in the planes it owns -- the ref restricted to those planes, bit for bit -- the N(r) add up to the
    undecomposed ones, and axis 2 is refused."""
    shape = (40, 6, 8)
    flow, p, u = make(shape, T, True)
    L = _lib.lib()
    i3 = lambda v: (C.c_int32 * 3)(*v)
    for start, zhi in ((None, 9), ((3, 2, 1), 8), ((1, 1, 6), 9)):
        lo, hi = lohi(start, shape)
        hi = hi[:2] + (zhi,)
        for axis in (0, 1, 2):
            n = hi[axis] - lo[axis]
            total = np.zeros(n)
            for rank in range(2):
                sl = Slab(rank, 2, shape[2])
                g = flow.layout.grid()
                off = sl.kz0 * g.s[2] * flow.p.element_size()  # local plane 0 is global plane kz0 (rank 0: below the array, never read)
                g.n[2], g.nzg, g.kz0, g.own_lo, g.own_hi, g.zring = sl.n2l, sl.nzg, sl.kz0, sl.own_lo, sl.own_hi, 0
                a, b = _lib.TpValue(), _lib.TpValue()
                a.f, a.kind = flow.p.data_ptr() + off, 0
                b.f, b.kind, b.ipar = flow.u.data_ptr() + off, 2, 2          # centre along z: reads the plane above
                nb = C.c_int64()
                rc = L.wl_twopoint_scratch(C.byref(g), axis, n, i3(lo), i3(hi), C.byref(nb))
                if axis == 2:
                    assert rc == _lib.WL_E_ARG and b"axis 2" in L.wl_last_error()
                    out = torch.zeros(10 * n, dtype=torch.float64, device=flow.device)
                    assert L.wl_twopoint(S._WLT[np.dtype(T)], C.byref(g), C.byref(a), C.byref(b), axis, n, 0, i3(lo), i3(hi), 0, C.c_void_p(out.data_ptr()),
                                         1 << 40, C.c_void_p(out.data_ptr())) == _lib.WL_E_ARG and b"axis 2" in L.wl_last_error()
                    continue
                assert rc == 0, L.wl_last_error()
                scratch = torch.zeros(max(1, nb.value // 8), dtype=torch.float64, device=flow.device)
                out = torch.full((n, 10), -1.0, dtype=torch.float64, device=flow.device)
                assert L.wl_twopoint(S._WLT[np.dtype(T)], C.byref(g), C.byref(a), C.byref(b), axis, n, 1, i3(lo), i3(hi), 0, C.c_void_p(scratch.data_ptr()),
                                     nb.value, C.c_void_p(out.data_ptr())) == 0, L.wl_last_error()
                part = host(out)
                zl, zh = (lo[2], min(hi[2], 5)) if rank == 0 else (max(lo[2], 5), hi[2])                # rank 0 owns the planes 0..4
                if zh > zl:
                    olo, ohi = lo[:2] + (zl,), hi[:2] + (zh,)
                    A = TR.lines(TR.values(p, "scalar", 0, olo, ohi), axis)
                    B = TR.lines(TR.values(u, "centre", 2, olo, ohi), axis)
                    assert np.array_equal(bits(part), bits(TR.twopoint(A, B, n, True))), (start, axis, rank)
                else:
                    assert not part.any(), (start, axis, rank)                                           # a rank without a plane in the box
                total += part[:, 0]
            if axis != 2:
                lines = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2]) // n
                assert np.array_equal(total, TR.count(lines, n, n, True)), (start, axis)


def test_accumulating_curl_over_a_stepping_flow():
    body = AutoBody(lambda x, t: norm2(x - 16.0) - 4.0)
    sim = S.Simulation((64, 32), (1.0, 0.0), 8.0, nu=8.0 / 250, body=body, T=F64)
    tp = TwoPoint(sim.flow, Value("curl", i=2), axis=1)
    scratch = S.like(sim.flow.p)
    lo, hi = (1, 1), (65, 33)
    want, snaps = None, []
    for k in range(3):
        S.sim_step(sim)
        tab = twopoint.measure(tp, sim.flow.u, accumulate=k > 0)
        m = S.to_host(S.metric(scratch, "curl", sim.flow.u, 2))
        A = TR.lines(TR.values(m, "scalar", 0, lo, hi), 1)
        t = TR.twopoint(A, A, 32, False)
        snaps.append(t)
        want = t if want is None else want + t
    assert np.array_equal(bits(host(tab)), bits(want)) and np.array_equal(host(tab)[:, 0], 3 * TR.count(64, 32, 32, False))
    assert not np.array_equal(snaps[0], snaps[2]) and np.abs(snaps[2][:, 6]).max() > 0                  # the flow moved, and has vorticity
    S2 = twopoint.structure(tab, 2)
    assert S2.is_cuda and float(S2[0]) == 0.0 and float(S2[1:].min()) > 0.0
