"""Regions on the GPU (waterlily_amd.regions: wl_regions) against the breadth-first fill of tests/regions_ref.py: the label volume
and the 13 columns equal as integers, the two extremes equal as uint64 views, the four counts equal.

Interior shapes: (72, 8, 8) -- a row of 64 + 8 cells: a second, short piece; (130, 5, 3) -- two seams in one row; the 2-D (40, 24)
and (72, 8); MANY = (8, 132, 126) -- more rows than the launch has wavefronts.  Float32 and Float64, padded and dense; inside()
and an interior box that starts at (3, 2, 1); BELOW and ABOVE.  Noise fields are seeded standard_normal rounded to multiples of
1/8, so that many values sit exactly on the level, thresholded at 10 %, near the face-connectivity percolation point (31 % in
3-D, 59 % in 2-D) and at 80 %: many specks, tortuous critical clusters, one giant region.  The built shapes -- serpentines, a
spiral, combs joined at the high end of each axis, a checkerboard -- are the ones a directional sweep gets wrong.

Why equality: the set is two strict IEEE comparisons of a double the host forms by the same single operations, and everything
after it is integers.  The metric kinds call the device function wl_metric's kernel calls, so their yardstick is the host copy
of what wl_metric stored for the same u.  Every call also holds visited == the cells of the box and sum(cells) == IN cells.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as RR  # noqa: E402

from waterlily_amd import _lib, hist, regions, sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402
from waterlily_amd.hist import Axis, Histogram  # noqa: E402
from waterlily_amd.regions import Regions, Value  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [(72, 8, 8), (130, 5, 3), (40, 24), (72, 8)]
CASES = [(sh, T, pad) for sh in SHAPES for T in (F32, F64) for pad in (True, False)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for sh, T, pad in CASES]
MANY = (8, 132, 126)
PERCOLATION = {3: 0.31, 2: 0.59}


@functools.lru_cache(maxsize=None)
def fields(shape, T):
    """(p, u) host arrays with ghosts, seeded, rounded to multiples of 1/8 (read-only)"""
    Ng = tuple(n + 2 for n in shape)
    rng = np.random.default_rng(29)
    p = np.asfortranarray((np.round(rng.standard_normal(Ng) * 8) / 8).astype(T))
    u = np.asfortranarray((np.round(rng.standard_normal(Ng + (len(shape),)) * 8) / 8).astype(T))
    p.setflags(write=False)
    u.setflags(write=False)
    return p, u


def make(shape, T, padded, p=None):
    flow = S.Flow(shape, (0.0,) * len(shape), T=T, padded=padded)
    hp, hu = fields(shape, T)
    hp = hp if p is None else np.asfortranarray(p.astype(T))
    S.upload(flow.p, hp)
    S.upload(flow.u, hu)
    return flow, hp, hu


def host(x):
    return x.cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F64)).view(np.uint64)


def boxes(Ng):
    return [None, (tuple([3, 2, 1][:len(Ng)]), tuple(n - 1 for n in Ng))]


def lohi(box, Ng):
    return ((1,) * len(Ng), tuple(n - 1 for n in Ng)) if box is None else box


def level(v, occupancy, above=False):
    """a multiple of 1/8 near the level that puts `occupancy` of the values in the set"""
    q = np.quantile(v[~np.isnan(v)], 1.0 - occupancy if above else occupancy)
    return float(np.round(q * 8) / 8)


def agree(res, want, what=""):
    lab, tab, ext, n = want
    got_n = [int(res.count), int(res.cells), int(res.nan), int(res.visited)]
    assert got_n == n.tolist(), (what, got_n, n.tolist())
    gl = host(res.lab)
    assert gl.dtype == np.int32 and gl.shape == lab.shape and np.array_equal(gl, lab), (what, "labels", int((gl != lab).sum()))
    gt, ge = host(res.tab), host(res.ext)
    assert gt.dtype == np.int64 and gt.shape == tab.shape and np.array_equal(gt, tab), (what, "table", np.argwhere(gt != tab)[:5].tolist())
    assert ge.shape == ext.shape and np.array_equal(bits(ge), bits(ext)), (what, "extremes")
    assert n[3] == lab.size and tab[:, 1].sum() == n[1]       # the invariants, on the yardstick and so on the device
    return int(n[0])


def check(flow, value, field, hfield, kind, comp, box, c, above=False, periodic=(), absval=False, capacity=4096):
    lo, hi = lohi(box, hfield.shape[:flow.D])
    v = RR.box_values(hfield, kind, comp, lo, hi, absval)
    rg = Regions(flow, value, box=box, periodic=periodic, capacity=capacity, **({"above": c} if above else {"below": c}))
    return agree(regions.table(rg, field), RR.regions(v, c, above=above, periodic=periodic, lo=lo), (kind, comp, box, c, above, periodic))


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_noise_at_three_occupancies(shape, T, padded):
    D = len(shape)
    flow, p, u = make(shape, T, padded)
    counts = []
    for box in boxes(p.shape):
        lo, hi = lohi(box, p.shape)
        v = RR.box_values(p, "scalar", 0, lo, hi)
        for occ in (0.10, PERCOLATION[D], 0.80):
            for above in (False, True):
                c = level(v, occ, above)
                assert (v == c).sum() > 0                      # values sit exactly on the level: they are out
                counts.append(check(flow, Value("scalar"), flow.p, p, "scalar", 0, box, c, above))
        for kind, comp in (("ucomp", 1), ("centre", D - 1)):
            c = level(RR.box_values(u, kind, comp, lo, hi), PERCOLATION[D])
            check(flow, Value(kind, i=comp), flow.u, u, kind, comp, box, c)
        c = level(np.abs(v), 0.4)
        check(flow, Value("scalar", absval=True), flow.p, p, "scalar", 0, box, c, absval=True)
    assert max(counts) > 20, counts                            # many specks at 10 %


@pytest.mark.parametrize("T", [F32, F64])
def test_more_rows_than_wavefronts(T):
    """MANY has 132 * 126 = 16632 x-rows of 8 cells; near the percolation point it holds thousands of regions: the table grows
    past its first capacity and the rows come out in ascending root order all the same."""
    flow, p, u = make(MANY, T, True)
    lo, hi = lohi(None, p.shape)
    v = RR.box_values(p, "scalar", 0, lo, hi)
    R = check(flow, Value("scalar"), flow.p, p, "scalar", 0, None, level(v, PERCOLATION[3]))
    assert R > 4096


# --------------------------------------------------------------------------- built shapes that defeat directional sweeps

def serpentine(n):
    """one region that winds through the whole box: full x-rows at even j, joined by one cell at alternating x-ends at odd j; in
    3-D that plane at even k, joined through one cell at odd k, alternately the winding's first and its last cell"""
    m = np.zeros(n, dtype=bool)
    plane = np.zeros(n[:2], dtype=bool)
    plane[:, ::2] = True
    for j in range(1, n[1], 2):
        plane[n[0] - 1 if (j // 2) % 2 == 0 else 0, j] = True
    if len(n) == 2:
        return plane
    last_j = (n[1] - 1) // 2 * 2
    ends = [(0, 0), (0 if (last_j // 2) % 2 == 0 else n[0] - 1, last_j)]
    for k in range(n[2]):
        if k % 2 == 0:
            m[:, :, k] = plane
        else:
            m[ends[(k // 2) % 2] + (k,)] = True
    return m


def spiral(n):
    """a 2-D spiral corridor, one cell wide, walls one cell wide, from the corner to the middle"""
    m = np.zeros(n, dtype=bool)
    x, y, dx, dy = 0, 0, 1, 0
    m[0, 0] = True

    def free(x, y, dx, dy):
        a, b = x + dx, y + dy
        if not (0 <= a < n[0] and 0 <= b < n[1]) or m[a, b]:
            return False
        a2, b2 = a + dx, b + dy
        return not (0 <= a2 < n[0] and 0 <= b2 < n[1]) or not m[a2, b2]

    while True:
        if not free(x, y, dx, dy):
            dx, dy = -dy, dx
            if not free(x, y, dx, dy):
                return m
        x, y = x + dx, y + dy
        m[x, y] = True


def comb(n, axis):
    """teeth along `axis` at every second position of the other axes, joined only by a plate at the high end of `axis`"""
    m = np.zeros(n, dtype=bool)
    teeth = [slice(None, None, 2)] * len(n)
    teeth[axis] = slice(None)
    m[tuple(teeth)] = True
    plate = [slice(None)] * len(n)
    plate[axis] = n[axis] - 1
    m[tuple(plate)] = True
    return m


def checkerboard(n):
    return np.indices(n).sum(axis=0) % 2 == 0


def painted(shape, T, m, outside=1.0):
    """a scalar field with ghosts: -1 where m (over inside()), +1 elsewhere in inside(), `outside` in the ghost layer"""
    p = np.full(tuple(s + 2 for s in shape), outside, dtype=T)
    inner = (slice(1, -1),) * len(shape)
    p[inner] = np.where(m, -1.0, 1.0)
    return p


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_built_shapes(shape):
    D = len(shape)
    shapes = {"serpentine": (serpentine(shape), 1), "checkerboard": (checkerboard(shape), (int(np.prod(shape)) + 1) // 2),
              "all": (np.ones(shape, dtype=bool), 1), "none": (np.zeros(shape, dtype=bool), 0)}
    for axis in range(D):
        shapes[f"comb{axis}"] = (comb(shape, axis), 1)
    if D == 2:
        shapes["spiral"] = (spiral(shape), 1)
    flow = None
    for name, (m, R) in shapes.items():
        hp = painted(shape, F32, m)
        if flow is None:
            flow, _, _ = make(shape, F32, True, p=hp)
        else:
            S.upload(flow.p, np.asfortranarray(hp))
        assert check(flow, Value("scalar"), flow.p, hp, "scalar", 0, None, 0.0) == R, name
        if name in ("serpentine", "comb0", "spiral"):
            check(flow, Value("scalar"), flow.p, hp, "scalar", 0, boxes(hp.shape)[1], 0.0)       # the interior box cuts it up
            check(flow, Value("scalar"), flow.p, hp, "scalar", 0, None, 0.0, above=True)        # the walls between the windings
    assert spiral((40, 24)).sum() > 400 and serpentine((72, 8, 8)).sum() > 72 * 4 * 4


# --------------------------------------------------------------------------- special values, isolation, wrap

def test_nan_inf_and_signed_zero():
    shape, T = (72, 8, 8), F64
    p0 = fields(shape, T)[0]
    rng = np.random.default_rng(31)
    pn = p0.copy()
    pn[rng.random(p0.shape) < 0.08] = np.nan                   # inside regions and on their rims
    pn[5, 4, 3], pn[6, 4, 3], pn[70, 2, 2], pn[40, 5, 5] = np.inf, np.inf, -np.inf, -np.inf
    flow, hp, _ = make(shape, T, True, p=pn)
    v = RR.box_values(hp, "scalar", 0, *lohi(None, hp.shape))
    assert np.isnan(v).sum() > 200
    for box in boxes(hp.shape):
        for above in (False, True):
            check(flow, Value("scalar"), flow.p, hp, "scalar", 0, box, 0.25, above)         # +-inf with a finite level
        check(flow, Value("scalar"), flow.p, hp, "scalar", 0, box, np.inf)                  # all but NaN and +inf
        check(flow, Value("scalar"), flow.p, hp, "scalar", 0, box, -np.inf, above=True)
        assert check(flow, Value("scalar"), flow.p, hp, "scalar", 0, box, -np.inf) == 0       # nothing is below -inf
    z = np.zeros(hp.shape)
    z[3::7] = -0.0
    z[1, 1, 1] = 0.0
    S.upload(flow.p, np.asfortranarray(z))
    rg = Regions(flow, Value("scalar"), below=1.0)
    res = regions.table(rg, flow.p)
    agree(res, RR.regions(RR.box_values(z, "scalar", 0, *lohi(None, z.shape)), 1.0))
    assert int(res.count) == 1 and np.array_equal(bits(host(res.ext)[0]), bits([-0.0, 0.0])) and host(res.tab)[0, 11:].tolist() == [2, 0]
    flow.p.fill_(float("nan"))
    res = regions.table(rg, flow.p)
    assert [int(res.count), int(res.cells), int(res.nan), int(res.visited)] == [0, 0, 4608, 4608] and (host(res.lab) == -1).all()


@pytest.mark.parametrize("shape", [(72, 8, 8), (40, 24)], ids=["72x8x8", "40x24"])
def test_cells_outside_the_box_join_nothing(shape):
    """the ghost layer (inside()) and the cells just outside the interior box are IN: blobs on the box's faces would join
    through them if the kernels looked outside"""
    p0 = fields(shape, F32)[0]
    for box in boxes(p0.shape):
        lo, hi = lohi(box, p0.shape)
        inner = tuple(slice(l, h) for l, h in zip(lo, hi))
        hp = np.full(p0.shape, -10.0, dtype=F32)
        hp[inner] = p0[inner]
        flow, hp, _ = make(shape, F32, True, p=hp)
        c = level(hp[inner].astype(F64), 0.2)
        R = check(flow, Value("scalar"), flow.p, hp, "scalar", 0, box, c)
        hq = np.full(p0.shape, 10.0, dtype=F32)
        hq[inner] = p0[inner]
        S.upload(flow.p, np.asfortranarray(hq))
        assert check(flow, Value("scalar"), flow.p, hq, "scalar", 0, box, c) == R > 10


@pytest.mark.parametrize("shape", [(72, 8, 8), (130, 5, 3), (40, 24)], ids=["72x8x8", "130x5x3", "40x24"])
def test_wrap_on_each_axis_and_on_all(shape):
    D = len(shape)
    flow, p, u = make(shape, F64, False)
    for box in boxes(p.shape):
        lo, hi = lohi(box, p.shape)
        c = level(RR.box_values(p, "scalar", 0, lo, hi), 0.2)
        plain = check(flow, Value("scalar"), flow.p, p, "scalar", 0, box, c)
        single = [check(flow, Value("scalar"), flow.p, p, "scalar", 0, box, c, periodic=(d,)) for d in range(D)]
        every = check(flow, Value("scalar"), flow.p, p, "scalar", 0, box, c, periodic=tuple(range(D)))
        assert every <= min(single) < plain and max(single) <= plain, (plain, single, every)      # the wrap merged regions
    hp = painted(shape, F64, comb(shape, 0))                   # the teeth's free ends reach the plate through the x wrap too
    S.upload(flow.p, np.asfortranarray(hp))
    assert check(flow, Value("scalar"), flow.p, hp, "scalar", 0, None, 0.0, periodic=tuple(range(D))) == 1


# --------------------------------------------------------------------------- capacity, repeatability

def test_capacity_smaller_than_the_regions_and_none_at_all():
    shape = (72, 8, 8)
    flow, p, u = make(shape, F32, True)
    lo, hi = lohi(None, p.shape)
    c = level(RR.box_values(p, "scalar", 0, lo, hi), 0.15)
    lab, tab, ext, n = RR.regions(RR.box_values(p, "scalar", 0, lo, hi), c, lo=lo)
    R = int(n[0])
    assert R > 40
    L = _lib.lib()
    rv = _lib.RgValue()
    rv.f, rv.kind = flow.p.data_ptr(), 0
    g = flow.layout.grid()

    def raw(rg, cap, tab, ext):
        assert L.wl_regions(S._WLT[np.dtype(F32)], C.byref(g), C.byref(rv), 0, c, 0, None, None, C.c_void_p(rg._lab.ptr), cap, tab, ext,
                            C.c_void_p(rg._n.ptr), C.c_void_p(rg._scratch.ptr), rg._scratch.nbytes) == 0, L.wl_last_error()

    rg = Regions(flow, Value("scalar"), below=c, capacity=20)
    rg._tab.tensor(torch.int64, flow.device).fill_(-77)
    rg._ext.tensor(torch.float64, flow.device).fill_(-77.0)
    raw(rg, 7, C.c_void_p(rg._tab.ptr), C.c_void_p(rg._ext.ptr))                                       # a table of 7 rows in a buffer of 20
    res = regions._view(rg, 20)
    assert int(res.count) == R and np.array_equal(host(res.lab), lab)                                    # the true R, the labels complete
    assert np.array_equal(host(res.tab)[:7], tab[:7]) and np.array_equal(bits(host(res.ext)[:7]), bits(ext[:7]))
    assert (host(res.tab)[7:] == -77).all() and (host(res.ext)[7:] == -77.0).all()                      # nothing past the table
    rg = Regions(flow, Value("scalar"), below=c, capacity=7)
    res = regions.label(rg, flow.p)
    assert res.tab.shape == (7, 13) and int(res.count) == R and np.array_equal(host(res.tab), tab[:7])
    agree(regions.table(rg, flow.p), (lab, tab, ext, n), "grown")
    assert rg.capacity == R
    rg = Regions(flow, Value("scalar"), below=c, capacity=0)   # NULL table and extremes: labels and counts only
    res = regions.label(rg, flow.p)
    assert res.tab.shape == (0, 13) and np.array_equal(host(res.lab), lab)
    assert [int(res.count), int(res.cells), int(res.nan), int(res.visited)] == n.tolist()
    rg._lab.tensor(torch.int32, flow.device).fill_(-5)
    raw(rg, 0, None, None)
    assert np.array_equal(host(regions._view(rg, 0).lab), lab)


def test_the_same_call_twice_gives_the_same_bits():
    flow, p, u = make((72, 8, 8), F64, True)
    c = level(RR.box_values(u, "centre", 2, *lohi(None, p.shape)), PERCOLATION[3])
    rg = Regions(flow, Value("centre", i=2), below=c, periodic=(1,))
    first = regions.table(rg, flow.u)
    a = (host(first.lab), host(first.tab), bits(host(first.ext)), int(first.count))
    second = regions.table(rg, flow.u)
    b = (host(second.lab), host(second.tab), bits(host(second.ext)), int(second.count))
    assert a[3] == b[3] > 10 and all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))


# --------------------------------------------------------------------------- metric kinds, series

@functools.lru_cache(maxsize=None)
def sphere():
    """a small 3-D sphere, stepped: (sim, host lambda2, host omega_mag) as wl_metric stores them"""
    m = 32
    sim = S.Simulation((m, m, m), (1.0, 0.0, 0.0), m / 4, nu=m / 4 / 3700, body=AutoBody(lambda x, t: norm2(x - (m / 2 - 1)) - m / 8), T=F32)
    for _ in range(3):
        S.sim_step(sim, remeasure=False)
    scratch = S.like(sim.flow.p)
    out = {}
    for kind in ("lambda2", "omega_mag"):
        scratch.zero_()
        out[kind] = S.to_host(S.metric(scratch, kind, sim.flow.u))
    return sim, out["lambda2"], out["omega_mag"]


@pytest.mark.parametrize("kind,above,q", [("omega_mag", True, 0.95), ("lambda2", False, 0.05)])
def test_metric_kinds_on_a_stepped_sphere(kind, above, q):
    sim, l2, om = sphere()
    m = l2 if kind == "lambda2" else om
    h = Histogram(sim.flow, Axis(kind, bins=512))
    c = float(hist.quantile(hist.count(h, sim.flow.u), hist.edges(h), q))      # the level, picked on the device
    for box in boxes(m.shape):
        lo, hi = lohi(box, m.shape)
        v = RR.box_values(m, "scalar", 0, lo, hi)
        rg = Regions(sim.flow, Value(kind), box=box, **({"above": c} if above else {"below": c}))
        res = regions.table(rg, sim.flow.u)
        R = agree(res, RR.regions(v, c, above=above, lo=lo), (kind, box))
        assert R >= 1 and 0 < int(res.cells) < v.size
    if kind == "lambda2":
        rg = Regions(sim.flow, Value("lambda2"), below=c)
        agree(regions.lambda2(rg, sim), RR.regions(RR.box_values(l2, "scalar", 0, *lohi(None, l2.shape)), c), "lambda2()")
        with pytest.raises(ValueError):
            Regions(sim.flow, Value("lambda2"), below=c, box=((0, 1, 1), (8, 8, 8)))      # a metric box must lie in inside()


def test_record_and_series_of_a_stepping_flow():
    body = AutoBody(lambda x, t: norm2(x - 16.0) - 4.0)
    sim = S.Simulation((64, 32), (1.0, 0.0), 8.0, nu=8.0 / 250, body=body, T=F64)
    rg = Regions(sim.flow, Value("curl", i=2, absval=True), above=0.05, capacity=1024)
    rs = regions.RegionSeries(rg, m=3, capacity=2)             # the third record grows the buffer
    direct = []
    for _ in range(3):
        S.sim_step(sim)
        regions.record(rs, sim, sim.flow.u)
        res = regions.table(rg, sim.flow.u)
        tab, ext = host(res.tab), host(res.ext)
        order = sorted(range(len(tab)), key=lambda r: (-tab[r, 1], r))[:3]
        rows = np.full((3, 15), np.nan)
        for k, r in enumerate(order):
            rows[k] = np.concatenate([tab[r].astype(F64), ext[r]])
        direct.append(np.concatenate([[int(res.count), int(res.cells), int(res.nan), int(res.visited)], rows.reshape(-1)]))
    t, rows = regions.series(rs)
    assert t.shape == (3,) and t[0] < t[1] < t[2] and rows.shape == (3, 4 + 45) and rows.dtype == F64
    for k in range(3):
        assert np.array_equal(bits(rows[k]), bits(direct[k])) and rows[k, 3] == 64 * 32 and 1 <= rows[k, 0] <= 1024
    assert not np.array_equal(bits(rows[0]), bits(rows[2]))     # the flow moved
