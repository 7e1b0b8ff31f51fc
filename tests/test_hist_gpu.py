"""Histogram on the GPU (waterlily_amd.hist: wl_histogram, wl_field_range) against the numpy restatement tests/hist_ref.py: every
int64 equal, and the four doubles of a range equal as uint64 views.

Interior shapes: (72, 8, 8) -- a row of 64 + 8 cells: a second, short piece of the row; the 2-D (40, 24) and (72, 8); and
MANY = (8, 132, 126), see test_more_rows_than_wavefronts.  Float32 and Float64, padded and dense; fields are seeded
standard_normal, ghost cells included, and a copy rounded to multiples of 1/8, on which every product of the uniform rule is
exact and many values sit on bin edges.  Every shape runs on inside() and on an interior box that starts at (3, 2, 1).

Why equality: a bin is found by comparisons and by one subtraction, one division and one multiplication in IEEE double, each
rounded on its own (the library is built without contraction), and counts are integers.  The metric kinds call the device
function wl_metric's kernel calls, so the yardstick for them is the host copy of what wl_metric stored for the same u.
The two-rank run through a worker is left out: starting the ranks takes longer than a test may here.  The slab rule is held by
test_slab_rule_with_two_ranks_emulated_in_one_process instead, and gather()'s sum by tests/test_hist_cpu.py.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hist_ref as HR  # noqa: E402

from waterlily_amd import _lib, hist, sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402
from waterlily_amd.dist import Slab  # noqa: E402
from waterlily_amd.hist import Axis, Histogram  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [(72, 8, 8), (40, 24), (72, 8)]
CASES = [(sh, T, pad) for sh in SHAPES for T in (F32, F64) for pad in (True, False)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for sh, T, pad in CASES]
CASES3 = [c for c in CASES if len(c[0]) == 3]
IDS3 = [i for c, i in zip(CASES, IDS) if len(c[0]) == 3]
MANY = (8, 132, 126)


@functools.lru_cache(maxsize=None)
def fields(shape, T):
    """(p, u, p8, u8) host arrays with ghosts, seeded (read-only); p8, u8: rounded to multiples of 1/8"""
    Ng = tuple(n + 2 for n in shape)
    rng = np.random.default_rng(17)
    p = np.asfortranarray(rng.standard_normal(Ng).astype(T))
    u = np.asfortranarray(rng.standard_normal(Ng + (len(shape),)).astype(T))
    return p, u, np.asfortranarray((np.round(p * 8) / 8).astype(T)), np.asfortranarray((np.round(u * 8) / 8).astype(T))


def make(shape, T, padded, dyadic=False):
    flow = S.Flow(shape, (0.0,) * len(shape), T=T, padded=padded)
    p, u, p8, u8 = fields(shape, T)
    p, u = (p8, u8) if dyadic else (p, u)
    S.upload(flow.p, p)
    S.upload(flow.u, u)
    return flow, p, u


def host(x):
    return x.cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F64)).view(np.uint64)


def boxes(Ng):
    return [None, (tuple([3, 2, 1][:len(Ng)]), tuple(n - 1 for n in Ng))]


def lohi(box, Ng):
    return ((1,) * len(Ng), tuple(n - 1 for n in Ng)) if box is None else box


def agrees(c, want):
    vis, nn, table = want
    got = host(c)
    return got.dtype == np.int64 and got.shape == table.shape and np.array_equal(got, table) and int(c.visited) == vis and int(c.nan) == nn


def kinds(D):
    return [("scalar", 0)] + [(k, c) for k in ("ucomp", "centre") for c in range(D)]


EDGES = np.sort(np.random.default_rng(5).standard_normal(13))


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_plain_kinds_with_each_way_of_giving_bins(shape, T, padded):
    D = len(shape)
    flow, p, u = make(shape, T, padded)
    p8, u8 = fields(shape, T)[2:]
    fp8, fu8 = S.like(flow.p), S.like(flow.u)
    S.upload(fp8, p8)
    S.upload(fu8, u8)
    n = 0
    for box in boxes(p.shape):
        lo, hi = lohi(box, p.shape)
        for kind, c in kinds(D):
            f, hf, f8, hf8 = (flow.p, p, fp8, p8) if kind == "scalar" else (flow.u, u, fu8, u8)
            # uniform, host range, dyadic data: values on lo, on hi and on interior edges
            v8 = HR.values(hf8, kind, c, lo, hi)
            assert kind == "centre" or (np.abs(v8) == 2).any()
            h = Histogram(flow, Axis(kind, i=c, bins=16, range=(-2, 2)), box=box)
            assert agrees(hist.count(h, f8), HR.histogram(v8, {"n": 16, "lo": -2.0, "hi": 2.0})), (kind, c, box, "host range")
            # uniform, device range
            v = HR.values(hf, kind, c, lo, hi)
            h = Histogram(flow, Axis(kind, i=c, bins=32), box=box)
            cnt = hist.count(h, f)
            r = HR.field_range(v)
            assert np.array_equal(bits(host(hist.range(h, f))), bits(r)), (kind, c, box, "range")
            assert agrees(cnt, HR.histogram(v, {"n": 32, "lo": r[0], "hi": r[1]})), (kind, c, box, "device range")
            assert host(cnt)[0] == 0 and host(cnt)[-1] == 0 and host(cnt)[1] >= 1 and host(cnt)[-2] >= 1      # the extremes are in range
            want_e = r[0] + np.arange(33, dtype=F64) * ((r[1] - r[0]) / 32)
            assert np.array_equal(bits(host(hist.edges(h))), bits(want_e))
            # edges
            h = Histogram(flow, Axis(kind, i=c, edges=EDGES), box=box)
            assert agrees(hist.count(h, f), HR.histogram(v, {"edges": EDGES})), (kind, c, box, "edges")
            assert np.array_equal(bits(host(hist.edges(h))), bits(EDGES))
            n += 1
    assert n == 2 * (1 + 2 * D)


@pytest.mark.parametrize("shape,T,padded", CASES[::3], ids=IDS[::3])
def test_abs_and_joint(shape, T, padded):
    D = len(shape)
    flow, p, u = make(shape, T, padded)
    for box in boxes(p.shape):
        lo, hi = lohi(box, p.shape)
        vp, vc = HR.values(p, "scalar", 0, lo, hi), HR.values(u, "centre", D - 1, lo, hi)
        h = Histogram(flow, Axis("scalar", bins=10, range=(0.25, 1.5), abs=True), box=box)
        assert agrees(hist.count(h, flow.p), HR.histogram(np.abs(vp), {"n": 10, "lo": 0.25, "hi": 1.5}))
        h = Histogram(flow, Axis("scalar", bins=9, abs=True), box=box)
        r = HR.field_range(np.abs(vp))
        assert agrees(hist.count(h, flow.p), HR.histogram(np.abs(vp), {"n": 9, "lo": r[0], "hi": r[1]})) and r[0] >= 0
        assert np.array_equal(bits(host(hist.range(h, flow.p))), bits(r))
        # joint p x centre(u) at 8 x 8, every way of giving bins mixed
        a, b = {"n": 8, "lo": -1.5, "hi": 1.5}, {"n": 8, "lo": -1.0, "hi": 2.0}
        h = Histogram(flow, Axis("scalar", bins=8, range=(-1.5, 1.5)), Axis("centre", i=D - 1, bins=8, range=(-1.0, 2.0)), box=box)
        c = hist.count(h, flow.p, flow.u)
        assert c.shape == (10, 10) and agrees(c, HR.histogram(vp, a, vc, b))
        assert np.array_equal(host(hist.marginal(c, "a")), HR.histogram(vp, a)[2]) and np.array_equal(host(hist.marginal(c, "b")), HR.histogram(vc, b)[2])
        rb = HR.field_range(vc)
        h = Histogram(flow, Axis("scalar", edges=EDGES), Axis("centre", i=D - 1, bins=5), box=box)
        assert agrees(hist.count(h, flow.p, flow.u), HR.histogram(vp, {"edges": EDGES}, vc, {"n": 5, "lo": rb[0], "hi": rb[1]}))
        # one interior B-bin: row 1 is the count of p over the cells where -0.5 <= centre(u) <= 0.25
        h = Histogram(flow, Axis("scalar", bins=8, range=(-1.5, 1.5)), Axis("centre", i=D - 1, edges=(-0.5, 0.25)), box=box)
        c = hist.count(h, flow.p, flow.u)
        keep = (vc >= -0.5) & (vc <= 0.25)
        assert c.shape == (3, 10) and keep.sum() > 20 and np.array_equal(host(hist.conditional(c, 1)), HR.histogram(vp[keep], a)[2])
        assert float(hist.fraction(hist.marginal(c, "b"), 1, 1)) == keep.sum() / keep.size


@pytest.mark.parametrize("shape,T,padded", CASES3, ids=IDS3)
def test_metric_kinds_equal_wl_metric(shape, T, padded):
    flow, p, u = make(shape, T, padded)
    scratch = S.like(flow.p)
    m = {}
    for kind in ("omega_mag", "lambda2"):
        scratch.zero_()
        m[kind] = S.to_host(S.metric(scratch, kind, flow.u))   # what the existing wl_metric stores
        assert np.isfinite(m[kind]).all() and m[kind][1:-1, 1:-1, 1:-1].std() > 0
    for box in boxes(p.shape):
        lo, hi = lohi(box, p.shape)
        vo, vl, vp = (HR.values(m["omega_mag"], "scalar", 0, lo, hi), HR.values(m["lambda2"], "scalar", 0, lo, hi), HR.values(p, "scalar", 0, lo, hi))
        for kind, v in (("omega_mag", vo), ("lambda2", vl)):
            h = Histogram(flow, Axis(kind, bins=24, range=(-1.0, 2.0)), box=box)
            assert agrees(hist.count(h, flow.u), HR.histogram(v, {"n": 24, "lo": -1.0, "hi": 2.0})), (kind, box)
            h = Histogram(flow, Axis(kind, bins=24), box=box)
            cnt, r = hist.count(h, flow.u), HR.field_range(v)
            assert np.array_equal(bits(host(hist.range(h, flow.u))), bits(r)), (kind, box)
            assert agrees(cnt, HR.histogram(v, {"n": 24, "lo": r[0], "hi": r[1]})), (kind, box, "auto")
        a, b, bp = {"n": 6, "lo": -2.0, "hi": 1.0}, {"n": 7, "lo": 0.0, "hi": 3.0}, {"n": 5, "lo": -1.0, "hi": 1.0}
        h = Histogram(flow, Axis("lambda2", bins=6, range=(-2.0, 1.0)), Axis("omega_mag", bins=7, range=(0.0, 3.0)), box=box)      # metric x metric
        assert agrees(hist.count(h, flow.u, flow.u), HR.histogram(vl, a, vo, b)), box
        h = Histogram(flow, Axis("lambda2", bins=6, range=(-2.0, 1.0)), Axis("scalar", bins=5, range=(-1.0, 1.0)), box=box)         # metric x plain
        assert agrees(hist.count(h, flow.u, flow.p), HR.histogram(vl, a, vp, bp)), box
        h = Histogram(flow, Axis("scalar", bins=5, range=(-1.0, 1.0)), Axis("omega_mag", bins=7, range=(0.0, 3.0)), box=box)        # plain x metric
        assert agrees(hist.count(h, flow.p, flow.u), HR.histogram(vp, bp, vo, b)), box


@pytest.mark.parametrize("T", [F32, F64])
def test_constant_field_one_bin_holds_every_cell(T):
    flow, p, u = make((72, 8, 8), T, True)
    flow.p.fill_(0.375)
    ncell = 72 * 8 * 8
    for ax, k in ((Axis(bins=16, range=(0.0, 1.0)), 7), (Axis(bins=16), 1), (Axis(edges=(0.0, 0.375, 1.0)), 2), (Axis(bins=4, range=(1.0, 2.0)), 0)):
        c = hist.count(Histogram(flow, ax), flow.p)
        got = host(c)
        assert got[k] == ncell and got.sum() == ncell and int(c.visited) == ncell and int(c.nan) == 0, (k, got)
    h = Histogram(flow, Axis(bins=16))
    assert host(hist.range(h, flow.p)).tolist() == [0.375, 0.375, float(ncell), 0.0]


def test_nan_inf_and_signed_zero():
    shape, T = (72, 8, 8), F64
    flow, p, u = make(shape, T, True)
    rng = np.random.default_rng(23)
    pn, un = p.copy(), u.copy()
    pn[rng.random(p.shape) < 0.05] = np.nan
    un[rng.random(u.shape) < 0.05] = np.nan
    pn[5, 4, 3], pn[70, 2, 2] = np.inf, -np.inf
    S.upload(flow.p, pn)
    S.upload(flow.u, un)
    lo, hi = lohi(None, p.shape)
    vp, vc = HR.values(pn, "scalar", 0, lo, hi), HR.values(un, "centre", 0, lo, hi)
    assert np.isnan(vp).sum() > 50 and (np.isnan(vp) & np.isnan(vc)).sum() > 0 and (np.isnan(vp) ^ np.isnan(vc)).sum() > 50
    a = {"n": 12, "lo": -2.0, "hi": 2.0}
    c = hist.count(Histogram(flow, Axis(bins=12, range=(-2, 2))), flow.p)
    assert agrees(c, HR.histogram(vp, a)) and int(c.visited) == int(c.nan) + int(c.sum())
    h = Histogram(flow, Axis(bins=12))                         # +-inf take part in the range
    c, r = hist.count(h, flow.p), HR.field_range(vp)
    assert r[:2].tolist() == [-np.inf, np.inf] and np.array_equal(bits(host(hist.range(h, flow.p))), bits(r))
    assert agrees(c, HR.histogram(vp, {"n": 12, "lo": -np.inf, "hi": np.inf}))
    c = hist.count(Histogram(flow, Axis(bins=12, range=(-2, 2)), Axis("centre", bins=6, range=(-1, 1))), flow.p, flow.u)
    assert agrees(c, HR.histogram(vp, a, vc, {"n": 6, "lo": -1.0, "hi": 1.0})) and int(c.visited) == int(c.nan) + int(c.sum())
    # nothing but NaN: a NaN range, every cell dropped
    flow.p.fill_(float("nan"))
    h = Histogram(flow, Axis(bins=4))
    c = hist.count(h, flow.p)
    r = host(hist.range(h, flow.p))
    assert np.isnan(r[:2]).all() and r[2:].tolist() == [0.0, 4608.0] and host(c).sum() == 0 and int(c.nan) == 4608 == int(c.visited)
    # a NaN range under cells that are not NaN: all of them overflow
    flow.p.fill_(1.0)
    c = hist.count(h, flow.p, accumulate=True)                 # (accumulate: the range is not found again)
    assert host(c).tolist() == [0, 0, 0, 0, 0, 4608] and int(c.nan) == 4608 and int(c.visited) == 2 * 4608
    # -0 and +0: the minimum is -0, the maximum +0, wherever they sit
    z = np.zeros(p.shape)
    z[3::7] = -0.0
    S.upload(flow.p, z)
    r = host(hist.range(h, flow.p))
    assert np.array_equal(bits(r), bits([-0.0, 0.0, 4608.0, 0.0]))
    assert host(hist.count(h, flow.p)).tolist() == [0, 4608, 0, 0, 0, 0]       # -0 == +0: hi == lo, bin 1


def test_accumulate_adds_and_a_plain_count_overwrites():
    flow, p, u = make((72, 8, 8), F32, True)
    h = Histogram(flow, Axis(bins=20, range=(-2, 2)), Axis("ucomp", i=1, bins=3, range=(-1, 1)))
    one = host(hist.count(h, flow.p, flow.u))
    c = hist.count(h, flow.p, flow.u, accumulate=True)
    assert np.array_equal(host(c), 2 * one) and int(c.visited) == 2 * 4608 and one.sum() == 4608
    c = hist.count(h, flow.p, flow.u)
    assert np.array_equal(host(c), one) and int(c.visited) == 4608


def test_largest_table_and_most_edges():
    flow, p, u = make((72, 8, 8), F64, True)
    lo, hi = lohi(None, p.shape)
    vp, vu = HR.values(p, "scalar", 0, lo, hi), HR.values(u, "ucomp", 2, lo, hi)
    h = Histogram(flow, Axis(bins=126, range=(-3, 3)), Axis("ucomp", i=2, bins=62, range=(-3, 3)))           # 128 * 64 = 8192
    assert agrees(hist.count(h, flow.p, flow.u), HR.histogram(vp, {"n": 126, "lo": -3.0, "hi": 3.0}, vu, {"n": 62, "lo": -3.0, "hi": 3.0}))
    h = Histogram(flow, Axis(bins=8190, range=(-3, 3)))
    assert agrees(hist.count(h, flow.p), HR.histogram(vp, {"n": 8190, "lo": -3.0, "hi": 3.0}))
    e = np.linspace(-2.5, 2.5, 1025) ** 3                      # 1024 bins of very different widths
    want = np.concatenate([[(vp < e[0]).sum()], np.histogram(vp, bins=e)[0], [(vp > e[-1]).sum()]])
    c = hist.count(Histogram(flow, Axis(edges=e), Axis("ucomp", i=2, edges=(-0.5, 0.0, 0.5, 1.0))), flow.p, flow.u)        # 1026 * 6
    assert np.array_equal(host(hist.marginal(c, "a")), want) and np.array_equal(host(hist.marginal(c, "b")), HR.histogram(vu, {"edges": [-0.5, 0.0, 0.5, 1.0]})[2])
    with pytest.raises(ValueError):
        Histogram(flow, Axis(bins=8191))
    with pytest.raises(ValueError):
        hist.count(h, flow.p, flow.u)                          # a 1-D histogram takes one field
    with pytest.raises(ValueError):
        hist.count(Histogram(flow, Axis("ucomp")), flow.p)     # a component of a scalar field


@pytest.mark.parametrize("T", [F32, F64])
def test_more_rows_than_wavefronts(T):
    """The launch is capped at 2048 workgroups of 4 wavefronts (HIST_WG in csrc/wl_hist.h) and the x-rows of the box are dealt
    round-robin to the 8192 wavefronts.  MANY has 132 * 126 = 16632 rows, more than twice 8192: every wavefront takes two or
    three rows, and all 2048 workgroups flush into the same few bins."""
    flow, p, u = make(MANY, T, True)
    lo, hi = lohi(None, p.shape)
    assert (hi[1] - lo[1]) * (hi[2] - lo[2]) > 2 * 8192
    vp, vc = HR.values(p, "scalar", 0, lo, hi), HR.values(u, "centre", 1, lo, hi)
    h = Histogram(flow, Axis(bins=6))
    c, r = hist.count(h, flow.p), HR.field_range(vp)
    assert np.array_equal(bits(host(hist.range(h, flow.p))), bits(r)) and agrees(c, HR.histogram(vp, {"n": 6, "lo": r[0], "hi": r[1]}))
    h = Histogram(flow, Axis(bins=5, range=(-1, 1)), Axis("centre", i=1, bins=4, range=(-1, 1)))
    assert agrees(hist.count(h, flow.p, flow.u), HR.histogram(vp, {"n": 5, "lo": -1.0, "hi": 1.0}, vc, {"n": 4, "lo": -1.0, "hi": 1.0}))
    scratch = S.like(flow.p)
    vl = HR.values(S.to_host(S.metric(scratch, "lambda2", flow.u)), "scalar", 0, lo, hi)
    assert agrees(hist.count(Histogram(flow, Axis("lambda2", bins=9, range=(-2, 1))), flow.u), HR.histogram(vl, {"n": 9, "lo": -2.0, "hi": 1.0}))


def test_record_and_series_of_a_stepping_flow():
    body = AutoBody(lambda x, t: norm2(x - 16.0) - 4.0)
    sim = S.Simulation((64, 32), (1.0, 0.0), 8.0, nu=8.0 / 250, body=body, T=F64)
    h = Histogram(sim.flow, Axis("curl", i=2, bins=16, range=(-1, 1)), Axis("scalar", bins=4, range=(-0.5, 0.5)))
    hs = hist.HistSeries(h, capacity=2)                        # the third record grows the buffer
    direct = []
    for _ in range(3):
        S.sim_step(sim)
        hist.record(hs, sim, sim.flow.u, sim.flow.p)
        c = hist.count(h, sim.flow.u, sim.flow.p)
        direct.append(np.concatenate([[int(c.visited), int(c.nan)], host(c).reshape(-1)]))
    t, rows = hist.series(hs)
    assert t.shape == (3,) and t[0] < t[1] < t[2] and rows.shape == (3, 2 + 18 * 6) and rows.dtype == F64
    for k in range(3):
        assert np.array_equal(rows[k], direct[k].astype(F64)) and rows[k, 0] == 64 * 32 == rows[k, 2:].sum()
    assert not np.array_equal(rows[0], rows[2])                # the flow moved


@pytest.mark.parametrize("T", [F32, F64])
def test_slab_rule_with_two_ranks_emulated_in_one_process(T):
    """wl_histogram on the z-slab descriptors of 2 ranks, each pointed at its planes of ONE undecomposed array: a rank counts the
    cells of the box in the planes it owns, and the two tables add up to the undecomposed one."""
    shape = (40, 6, 8)
    flow, p, u = make(shape, T, True)
    L = _lib.lib()
    cnt = torch.zeros(2 + 12 * 5, dtype=torch.int64, device=flow.device)
    for box in (None, ((3, 2, 1), (41, 7, 8)), ((1, 1, 6), (41, 7, 9))):
        lo, hi = lohi(box, p.shape)
        want = HR.histogram(HR.values(p, "scalar", 0, lo, hi), {"n": 10, "lo": -2.0, "hi": 2.0}, HR.values(u, "centre", 2, lo, hi), {"n": 3, "lo": -1.0, "hi": 1.0})
        total, planes = np.zeros(2 + 60, dtype=np.int64), []
        for rank in range(2):
            sl = Slab(rank, 2, shape[2])
            g = flow.layout.grid()
            off = sl.kz0 * g.s[2] * flow.p.element_size()      # local plane 0 is global plane kz0 (rank 0: below the array, never read)
            g.n[2], g.nzg, g.kz0, g.own_lo, g.own_hi, g.zring = sl.n2l, sl.nzg, sl.kz0, sl.own_lo, sl.own_hi, 0
            a, b = _lib.HistAxis(), _lib.HistAxis()
            a.f, a.kind, a.nbins, a.lo, a.hi = flow.p.data_ptr() + off, 0, 10, -2.0, 2.0
            b.f, b.kind, b.ipar, b.nbins, b.lo, b.hi = flow.u.data_ptr() + off, 2, 2, 3, -1.0, 1.0
            i3 = lambda v: (C.c_int32 * 3)(*v)
            assert L.wl_histogram(S._WLT[np.dtype(T)], C.byref(g), C.byref(a), C.byref(b), None if box is None else i3(lo), None if box is None else i3(hi), 0,
                                  C.c_void_p(cnt.data_ptr())) == 0, L.wl_last_error()
            part = host(cnt)
            planes.append(int(part[0]) // ((hi[0] - lo[0]) * (hi[1] - lo[1])))
            assert part[0] == part[1] + part[2:].sum()
            total += part
        own = [len([z for z in range(lo[2], hi[2]) if (z <= 4) == (rank == 0)]) for rank in range(2)]          # rank 0 owns the planes 0..4
        assert planes == own, (box, planes, own)
        assert total[0] == want[0] and total[1] == want[1] and np.array_equal(total[2:].reshape(5, 12), want[2]), box
