"""Region sums on the GPU (waterlily_amd.regions.sums: wl_region_sums) against the integer restatement tests/region_sums_ref.py:
limbs, counts of non-finite terms, scales, overflow counts and the rounded doubles BIT-EQUAL, no tolerance.

Boxes: 2-D with nx = 63, 64, 65 (around the 64-cell seam of a piece) and 130 (two whole pieces and a short one), six rows; 3-D
70 x 9 x 5: 45 x-rows, so several wavefronts and workgroups hold shares of one region.  Float32 and Float64.  Label patterns are
written into the label volume by the test (the kernel reads numbers, not connectivity): one region filling the box; stripes of
alternating 1-cell and 3-cell runs, a new region each, so that one piece holds many regions; bands (whole rows, three regions in
turn: a wavefront meets a new region at every row); a mix in one row; nothing at all (R = 0); and the labelling wl_regions itself
makes with periodic joins.  Values are normal noise times 2^k, k uniform in -100..40 (Float64) or -60..40 (Float32): more than
the 74 bits a limb set holds below the largest term, so truncation toward zero happens in both signs; a third of the adjacent
cell pairs of p are exact negatives of each other.

Why equality: a term is one or two IEEE double multiplications of a double the host forms by the same single operations (the
metric kinds: the host copy of what wl_metric stored), and everything after it is integers.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_sums_ref as SR  # noqa: E402
import regions_ref as RR  # noqa: E402

from waterlily_amd import regions, sim as S  # noqa: E402
from waterlily_amd.regions import Regions, Value, Weight  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [(63, 6), (64, 6), (65, 6), (130, 6), (70, 9, 5)]
CASES = [(sh, T) for sh in SHAPES for T in (F32, F64)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}" for sh, T in CASES]
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def fields(shape, T):
    """(p, u) host arrays with ghosts (read-only): noise times 2^k; a third of the x-neighbour pairs of p are +-pairs"""
    Ng = tuple(n + 2 for n in shape)
    rng = np.random.default_rng(41)
    klo = -100 if T == F64 else -60
    p = rng.standard_normal(Ng) * np.exp2(rng.integers(klo, 41, size=Ng).astype(F64))
    u = rng.standard_normal(Ng + (len(shape),)) * np.exp2(rng.integers(klo, 41, size=Ng + (len(shape),)).astype(F64))
    pair = rng.random((Ng[0] // 2,) + Ng[1:]) < 1 / 3
    lowx = p[0:2 * (Ng[0] // 2):2]
    p[1:2 * (Ng[0] // 2):2] = np.where(pair, -lowx, p[1:2 * (Ng[0] // 2):2])
    p, u = np.asfortranarray(p.astype(T)), np.asfortranarray(u.astype(T))
    assert np.isfinite(p).all() and np.isfinite(u).all()
    p.setflags(write=False)
    u.setflags(write=False)
    return p, u


def make(shape, T, p=None):
    flow = S.Flow(shape, (0.0,) * len(shape), T=T)
    hp, hu = fields(shape, T)
    hp = hp if p is None else np.asfortranarray(p.astype(T))
    S.upload(flow.p, hp)
    S.upload(flow.u, hu)
    return flow, hp, hu


def host(x):
    return x.cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F64)).view(np.uint64)


def patterns(n):
    """label volumes [nx, ny(, nz)] int32 by name"""
    nx = n[0]
    rows = int(np.prod(n[1:]))
    out = {"one": np.zeros(n, dtype=np.int32), "none": np.full(n, -1, dtype=np.int32)}
    runs = []                                                  # 1 IN, 1 out, 3 IN, 1 out, ... along x, a new region per run
    x, k = 0, 0
    line = np.full(nx, -1, dtype=np.int32)
    while x < nx:
        w = 1 if k % 2 == 0 else 3
        line[x:x + w] = k
        runs.append(k)
        x, k = x + w + 1, k + 1
    per = len(runs)
    stripes = np.empty((nx, rows), dtype=np.int32)
    for r in range(rows):
        stripes[:, r] = np.where(line >= 0, line + per * r, -1)
    out["stripes"] = stripes.reshape(n, order="F")
    bands = np.empty((nx, rows), dtype=np.int32)
    for r in range(rows):
        bands[:, r] = r % 3
    bands[5::11, :] = -1                                       # holes do not end a region's share
    out["bands"] = bands.reshape(n, order="F")
    mix = stripes.copy()
    head = 64 if nx >= 96 else nx // 2                         # nx = 130: the first piece is one region, the rest stripes
    mix[:head, :] = per * rows                                 # one region across the rows, then the stripes of each row
    mix[head, :] = -1
    out["mix"] = mix.reshape(n, order="F")
    return out


def set_labels(rg, lab, R=None):
    """write a label volume and its count into the Regions object's buffers, as wl_regions would have left them"""
    dev = rg.flow.device
    R = int(lab.max()) + 1 if R is None else R
    rg._lab.tensor(torch.int32, dev)[:rg.ncell].copy_(torch.from_numpy(np.ascontiguousarray(lab.reshape(-1, order="F"))))
    n = torch.tensor([R, int((lab >= 0).sum()), 0, lab.size], dtype=torch.int64)
    rg._n.tensor(torch.int64, dev).copy_(n)
    return regions._view(rg, min(R, rg.capacity))


def metric_host(flow, kind, i=0):
    return S.to_host(S.metric(S.like(flow.p), kind, flow.u, i=i))


def columns(flow, hp, hu):
    """eight columns of one call, as (Weight, the host array its value is formed from, ref kind, component, absval): powers 1 and
    2, every moment axis, absval, scalar / ucomp / centre / one metric kind, two fields, and columns 0, 1, 2 sharing one value"""
    D = flow.D
    mk, mi = ("omega_mag", 0) if D == 3 else ("curl", 2)
    hm = metric_host(flow, mk, mi)
    return [
        (Weight(Value("scalar"), field=flow.p), hp, "scalar", 0, False, 1, None),
        (Weight(Value("scalar"), power=2, field=flow.p), hp, "scalar", 0, False, 2, None),
        (Weight(Value("scalar"), moment=0, field=flow.p), hp, "scalar", 0, False, 1, 0),
        (Weight(Value("ucomp", i=1), moment=1), hu, "ucomp", 1, False, 1, 1),
        (Weight(Value("centre", i=D - 1, absval=True)), hu, "centre", D - 1, True, 1, None),
        (Weight(Value(mk, i=mi), power=2), hm, "scalar", 0, False, 2, None),
        (Weight(Value(mk, i=mi), moment=D - 1), hm, "scalar", 0, False, 1, D - 1),
        (Weight(Value("scalar", absval=True), power=2, moment=D - 1, field=flow.p), hp, "scalar", 0, True, 2, D - 1),
    ]


def ref_cols(cols, lo, hi):
    return [(RR.box_values(h, kind, comp, lo, hi, absval), power, moment) for _, h, kind, comp, absval, power, moment in cols]


def agree(sm, want, what=""):
    acc, val, Es, over = want
    ga, gv = host(sm.acc), host(sm.value)
    assert host(sm.scale).tolist() == Es.tolist(), (what, "scale", host(sm.scale).tolist(), Es.tolist())
    assert host(sm.over).tolist() == over.tolist(), (what, "over", host(sm.over).tolist(), over.tolist())
    assert ga.dtype == np.int64 and ga.shape == acc.shape and np.array_equal(ga, acc), (what, "limbs", np.argwhere(ga != acc)[:5].tolist())
    assert gv.shape == val.shape and np.array_equal(bits(gv), bits(val)), (what, "doubles", np.argwhere(bits(gv) != bits(val))[:5].tolist())


def inside(flow):
    return (1,) * flow.D, tuple(n - 1 for n in flow.N)


@pytest.mark.parametrize("shape,T", CASES, ids=IDS)
def test_every_pattern_with_eight_columns(shape, T):
    flow, hp, hu = make(shape, T)
    lo, hi = inside(flow)
    cols = columns(flow, hp, hu)
    rc = ref_cols(cols, lo, hi)
    rg = Regions(flow, Value("scalar"), below=0.0, periodic=tuple(range(flow.D)), capacity=2048)
    for name, lab in patterns(shape).items():
        res = set_labels(rg, lab)
        sm = regions.sums(rg, res, [c[0] for c in cols], flow.u)
        want = SR.sums(lab, rc, lo)
        agree(sm, want, name)
        assert sm.value.shape == (int(lab.max()) + 1, 8)
        if name == "one":                                     # truncation really happened: the terms span more than a limb set
            assert want[2][0] - np.log2(np.abs(rc[0][0][rc[0][0] != 0]).min()) > 74
    res = regions.table(rg, flow.p)                            # wl_regions' own labelling, joined through the periodic wrap
    lab, tab, ext, n = RR.regions(rc[0][0], 0.0, periodic=tuple(range(flow.D)), lo=lo)
    assert np.array_equal(host(res.lab), lab) and 1 < int(res.count) < int(RR.regions(rc[0][0], 0.0, lo=lo)[3][0])
    agree(regions.sums(rg, res, [c[0] for c in cols], flow.u), SR.sums(lab, rc, lo), "wl_regions, periodic")


def test_rows_beyond_the_capacity_and_beyond_the_regions_stay_untouched():
    shape, T = (65, 6), F64
    flow, hp, hu = make(shape, T)
    lo, hi = inside(flow)
    lab = patterns(shape)["stripes"]
    R = int(lab.max()) + 1
    ws = [Weight(Value("scalar")), Weight(Value("scalar"), power=2, moment=1)]
    rc = [(RR.box_values(hp, "scalar", 0, lo, hi), 1, None), (RR.box_values(hp, "scalar", 0, lo, hi), 2, 1)]
    full = SR.sums(lab, rc, lo)
    for cap in (7, R + 9):
        rg = Regions(flow, Value("scalar"), below=0.0, capacity=cap)
        res = set_labels(rg, lab)
        regions.sums(rg, res, ws, flow.p)                      # makes the buffers
        b = rg._sums[0]
        acc_all, val_all = b.acc.tensor(torch.int64, flow.device), b.val.tensor(torch.float64, flow.device)
        acc_all.fill_(SENTINEL)
        val_all.fill_(float(SENTINEL))
        sm = regions.sums(rg, res, ws, flow.p)
        rows = min(R, cap)
        want = SR.sums(lab, rc, lo, cap=cap)
        assert want[0].shape[0] == rows and np.array_equal(want[0], full[0][:rows]) and want[2].tolist() == full[2].tolist()
        agree(sm, want, cap)                                   # the scale is that of the whole box whatever the capacity
        assert (host(acc_all)[rows * 2 * 5:] == SENTINEL).all() and (host(val_all)[rows * 2:] == float(SENTINEL)).all()
    res = set_labels(rg, patterns(shape)["none"], R=0)         # nothing IN: no row is written, the scales are the clamp
    acc_all.fill_(SENTINEL)
    val_all.fill_(float(SENTINEL))
    sm = regions.sums(rg, res, ws, flow.p)
    assert sm.value.shape == (0, 2) and host(sm.scale).tolist() == [SR.EMIN] * 2 and host(sm.over).tolist() == [0, 0]
    assert (host(acc_all) == SENTINEL).all() and (host(val_all) == float(SENTINEL)).all()


@pytest.mark.parametrize("T", [F32, F64])
def test_a_nan_and_an_inf_spoil_their_own_regions_only(T):
    shape = (70, 9, 5)
    p0 = fields(shape, T)[0]
    lab = patterns(shape)["bands"]
    p = p0.copy()
    p[1 + 3, 1 + 0, 1 + 0], p[1 + 8, 1 + 1, 1 + 2] = np.nan, np.inf      # box cells (3, 0, 0): region 0; (8, 1, 2): row 19, region 1
    assert lab[3, 0, 0] == 0 and lab[8, 1, 2] == 1
    flow, hp, hu = make(shape, T, p=p)
    lo, hi = inside(flow)
    rg = Regions(flow, Value("scalar"), below=0.0, capacity=16)
    res = set_labels(rg, lab)
    ws = [Weight(Value("scalar")), Weight(Value("ucomp", i=0), field=flow.u), Weight(Value("scalar"), power=2, moment=2)]
    rc = [(RR.box_values(hp, "scalar", 0, lo, hi), 1, None), (RR.box_values(hu, "ucomp", 0, lo, hi), 1, None), (RR.box_values(hp, "scalar", 0, lo, hi), 2, 2)]
    sm = regions.sums(rg, res, ws, flow.p)
    agree(sm, SR.sums(lab, rc, lo), "nan, inf")
    v, a = host(sm.value), host(sm.acc)
    assert np.isnan(v[:2, 0]).all() and np.isnan(v[:2, 2]).all() and np.isfinite(v[2]).all() and np.isfinite(v[:, 1]).all()
    assert a[:, :, 4].tolist() == [[1, 0, 1], [1, 0, 1], [0, 0, 0]]
    clean = make(shape, T)[0]                                  # the field without them, the same scales: the third region's bits
    rg2 = Regions(clean, Value("scalar"), below=0.0, capacity=16)
    sm2 = regions.sums(rg2, set_labels(rg2, lab), ws[:1] + [Weight(Value("ucomp", i=0), field=clean.u)] + ws[2:], clean.p, scale=host(sm.scale).tolist())
    assert np.array_equal(host(sm2.acc)[2], a[2]) and np.array_equal(host(sm2.acc)[:, 1], a[:, 1])


@pytest.mark.parametrize("shape,T", [((130, 6), F32), ((70, 9, 5), F64)], ids=["130x6-float32", "70x9x5-float64"])
def test_given_scales_overflow_counts_and_halves_that_combine(shape, T):
    flow, hp, hu = make(shape, T)
    lo, hi = inside(flow)
    cols = columns(flow, hp, hu)
    ws, rc = [c[0] for c in cols], ref_cols(cols, lo, hi)
    rg = Regions(flow, Value("scalar"), below=0.0, capacity=2048)
    for name in ("mix", "bands"):
        lab = patterns(shape)[name]
        res = set_labels(rg, lab)
        found = regions.sums(rg, res, ws, flow.u)
        want = SR.sums(lab, rc, lo)
        agree(found, want, name)
        E = host(found.scale).copy()
        acc0, val0 = host(found.acc), host(found.value)
        given = regions.sums(rg, res, ws, flow.u, scale=E.tolist())                  # the found scale, given: the same bits
        agree(given, want, name + " given")
        assert np.array_equal(host(given.acc), acc0) and np.array_equal(bits(host(given.value)), bits(val0))
        Elow = E.copy()
        Elow[::2] -= 3                                         # every other column three below: its largest terms do not fit
        low = regions.sums(rg, res, ws, flow.u, scale=torch.from_numpy(Elow))
        wlow = SR.sums(lab, rc, lo, scale=Elow.tolist())
        assert (wlow[3][::2] > 0).all() and (wlow[3][1::2] == 0).all()
        agree(low, wlow, name + " low")                        # the counts, and the columns without overflow bit for bit ...
        assert np.array_equal(host(low.acc)[:, 1::2], acc0[:, 1::2]) and np.array_equal(bits(host(low.value)[:, 1::2]), bits(val0[:, 1::2]))      # ... unchanged
    # two calls on the two halves of the box along the last axis, the labels of the whole: combine gives the whole box's bits
    lab = patterns(shape)["bands"]
    whole = regions.sums(rg, set_labels(rg, lab), ws, flow.u)
    E = host(whole.scale).tolist()
    wacc, wval = host(whole.acc), host(whole.value)
    d = flow.D - 1
    cut = shape[d] // 2
    halves = []
    for a, b in ((0, cut), (cut, shape[d])):
        blo, bhi = list(lo), list(hi)
        blo[d], bhi[d] = lo[d] + a, lo[d] + b
        part = lab[(slice(None),) * d + (slice(a, b),)]
        rh = Regions(flow, Value("scalar"), below=0.0, box=(tuple(blo), tuple(bhi)), capacity=1024)
        sm = regions.sums(rh, set_labels(rh, part, R=3), ws, flow.u, scale=E)
        agree(sm, SR.sums(part, ref_cols(cols, blo, bhi), blo, R=3, scale=E), ("half", a))
        halves.append(regions.Sums(sm.value.clone(), sm.acc.clone(), sm.scale.clone(), sm.over.clone()))
    got = regions.combine(halves[0], halves[1])
    assert np.array_equal(host(halves[0].acc + halves[1].acc), wacc) and np.array_equal(bits(host(got)), bits(wval))


def test_the_same_call_twice_gives_the_same_bits_and_nine_weights_take_two_calls():
    shape, T = (70, 9, 5), F32
    flow, hp, hu = make(shape, T)
    lo, hi = inside(flow)
    cols = columns(flow, hp, hu)
    ws, rc = [c[0] for c in cols], ref_cols(cols, lo, hi)
    rg = Regions(flow, Value("scalar"), below=0.0, capacity=64)
    res = set_labels(rg, patterns(shape)["bands"])
    first = regions.sums(rg, res, ws, flow.u)
    a = (host(first.acc), bits(host(first.value)), host(first.scale), host(first.over))
    second = regions.sums(rg, res, ws, flow.u)
    b = (host(second.acc), bits(host(second.value)), host(second.scale), host(second.over))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    nine = regions.sums(rg, res, ws + [Weight(Value("ucomp", i=2), power=2)], flow.u)
    want = SR.sums(patterns(shape)["bands"], rc + [(RR.box_values(hu, "ucomp", 2, lo, hi), 2, None)], lo)
    assert nine.value.shape == (3, 9) and nine.acc.shape == (3, 9, 5) and nine.scale.shape == (9,)
    agree(nine, want, "nine")


def test_circulation_of_a_patch_of_constant_curl():
    """u_y(i, j) = w * (the cells of the disc in row j up to i), u_x = 0: curl_z = u_y(i) - u_y(i - 1) = w inside the disc, 0
    outside, exactly.  With w a power of two every sum is exact: circulation = cells * w, enstrophy = cells * w^2, and the
    curl-weighted centroid is the centroid."""
    shape, T, w = (96, 40), F32, 0.125
    flow = S.Flow(shape, (0.0, 0.0), T=T)
    I, J = np.indices(flow.N)
    disc = (I - 50.0) ** 2 + (J - 21.0) ** 2 < 15.0 ** 2
    disc[:1], disc[-1:], disc[:, :1], disc[:, -1:] = False, False, False, False
    u = np.zeros(flow.N + (2,), dtype=T)
    u[..., 1] = w * np.cumsum(disc, axis=0)
    S.upload(flow.u, np.asfortranarray(u))
    cells = int(disc.sum())
    rg = Regions(flow, Value("curl", i=2), above=w / 2)
    res = regions.table(rg, flow.u)
    assert int(res.count) == 1 and host(regions.volume(res)).tolist() == [cells] and cells > 600
    assert host(regions.circulation(rg, res, flow.u)).tolist() == [[cells * w]]
    assert host(regions.enstrophy(rg, res, flow.u)).tolist() == [cells * w * w]
    sm = regions.sums(rg, res, [Value("curl", i=2)], flow.u)
    assert host(regions.mean(sm, res)).tolist() == [[w]] and host(sm.scale).tolist() == [-3] and host(sm.over).tolist() == [0]
    assert np.array_equal(host(regions.weighted_centroid(rg, res, Value("curl", i=2), flow.u)), host(regions.centroid(res)))
    ke = host(regions.kinetic_energy(rg, res, flow.u))
    hk = RR.box_values(S.to_host(S.metric(S.like(flow.p), "ke", flow.u)), "scalar", 0, *inside(flow))
    assert np.array_equal(bits(ke), bits(SR.sums(host(res.lab), [(hk, 1, None)], (1, 1))[1][:, 0]))
    flow.u.zero_()                                             # no weight at all: the centroid is NaN, not a division by zero
    rz = Regions(flow, Value("scalar"), below=1.0)
    assert np.isnan(host(regions.weighted_centroid(rz, regions.table(rz, flow.p), Value("curl", i=2), flow.u))).all()


def test_region_series_with_and_without_weights():
    shape, T = (65, 6), F64
    flow, hp, hu = make(shape, T)
    lo, hi = inside(flow)
    rg = Regions(flow, Value("scalar"), below=0.0, capacity=256)
    plain = regions.RegionSeries(rg, m=3, capacity=2)
    ws = (Weight(Value("scalar")), Weight(Value("ucomp", i=1), power=2, moment=0, field=flow.u))
    heavy = regions.RegionSeries(rg, m=3, capacity=2, weights=ws)
    regions.record(plain, flow, flow.p)
    regions.record(heavy, flow, flow.p)
    res = regions.table(rg, flow.p)
    tab, ext = host(res.tab), host(res.ext)
    order = sorted(range(len(tab)), key=lambda r: (-tab[r, 1], r))[:3]
    rows = np.stack([np.concatenate([tab[r].astype(F64), ext[r]]) for r in order])
    direct = np.concatenate([[int(res.count), int(res.cells), int(res.nan), int(res.visited)], rows.reshape(-1)])
    t, got = regions.series(plain)                             # without weights: the row the recorder always wrote
    assert t.shape == (1,) and got.shape == (1, 4 + 45) and np.array_equal(bits(got[0]), bits(direct))
    t, got = regions.series(heavy)
    v = RR.box_values(hp, "scalar", 0, lo, hi)
    want = SR.sums(RR.regions(v, 0.0, lo=lo)[0], [(v, 1, None), (RR.box_values(hu, "ucomp", 1, lo, hi), 2, 0)], lo)[1]
    assert got.shape == (1, 4 + 45 + 6) and np.array_equal(bits(got[0, :49]), bits(direct))
    assert np.array_equal(bits(got[0, 49:].reshape(3, 2)), bits(want[order]))
    few = regions.RegionSeries(Regions(flow, Value("scalar"), below=-1e300, capacity=4), m=2, weights=ws[:1])
    regions.record(few, flow, flow.p)                          # no region at all: NaN rows, sums included
    assert np.isnan(regions.series(few)[1][0, 4:]).all()
