"""Isosurface on the GPU (waterlily_amd.iso: wl_isosurface) against the numpy restatement tests/iso_ref.py and closed forms.

Shapes (interior cells): (70, 9, 7) a row longer than one 64-cube chunk and no multiple of it, (33, 12, 10), (64, 5, 5) exactly
one chunk plus ghosts; Float32 and Float64, padded and dense.  Random fields are seeded standard_normal, the level is
0.1 + 2^-30 and equals no field value (asserted).

Bounds (EPS = 2^-52): count, order and the edge of every vertex are exact.  Positions: t is within 3 ulp of a correctly rounded
quotient in [0, 1] and one add at magnitude <= n_d follows: 8 EPS max(n_d).  Colours: 8 EPS max |b|.  The plane's bounds are
test_iso_cpu's; a linear colour is g_b.x + c_b within 16 EPS sum |g_b,d| n_d plus one ulp_T of storage.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_ref as IR  # noqa: E402
from test_iso_cpu import EPS, LEVEL, SHAPES, check_plane, linear_field, random_field  # noqa: E402

from waterlily_amd import _lib, iso, sim as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
CASES = [(sh, T, pad) for sh in SHAPES for T in (F32, F64) for pad in (True, False)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for sh, T, pad in CASES]


def make(shape, T, padded, capacity=1 << 16):
    flow = S.Flow(shape, (0.0, 0.0, 0.0), T=T, padded=padded)
    return flow, iso.Isosurface(flow, capacity=capacity)


def field_on(flow, host):
    a = S.like(flow.p)
    S.upload(a, host)
    return a


@functools.lru_cache(maxsize=None)
def colour_field(shape, T):
    return random_field(shape, T, seed=11)


@functools.lru_cache(maxsize=None)
def ref_random(shape, T):
    """iso_ref on the seeded random field with the random colour (computed once per shape and type, read-only)"""
    return IR.extract(random_field(shape, T), LEVEL, b=colour_field(shape, T))


def host(x):
    return None if x is None else x.cpu().numpy().copy()


def compare(tri, val, ref, nmax, bmax=None):
    rt, rv, redge, _ = ref
    assert tri.shape == rt.shape                                                    # the count
    assert np.array_equal(IR.edges_of(tri), redge)                                 # the order and every vertex's edge
    d = np.abs(tri - rt).max(initial=0.0)
    print(f"\n{len(rt)} triangles, max |x - ref| = {d:.3e} (bound {8 * EPS * nmax:.3e})")
    assert d <= 8 * EPS * nmax
    if bmax is not None:
        assert np.array_equal(np.isnan(val), np.isnan(rv))
        k = ~np.isnan(rv)
        dv = np.abs(val[k] - rv[k]).max(initial=0.0)
        print(f"max |val - ref| = {dv:.3e} (bound {8 * EPS * bmax:.3e})")
        assert dv <= 8 * EPS * bmax


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_random_fields_against_the_reference(shape, T, padded):
    flow, isf = make(shape, T, padded)
    a, b = random_field(shape, T), colour_field(shape, T)
    tri, val = iso.extract(isf, field_on(flow, a), LEVEL, color=field_on(flow, b))
    ref = ref_random(shape, T)
    assert len(ref[0]) > 1000
    compare(host(tri), host(val), ref, max(shape) + 2, float(np.abs(b).max()))
    tri2, val2 = iso.extract(isf, field_on(flow, a), LEVEL)                         # without a colour: the same triangles
    assert val2 is None and np.array_equal(host(tri2), host(tri))


@pytest.mark.parametrize("shape,T,padded", [c for c in CASES if c[2]], ids=[i for i, c in zip(IDS, CASES) if c[2]])
def test_closed_by_bits(shape, T, padded):
    """the outermost interior layer set to 5 (outside): the surface closes inside the box, and every directed edge is matched
    exactly once by its reverse, compared by bits"""
    a = random_field(shape, T).copy()
    inner = np.full(a.shape, 5.0, dtype=T)
    inner[2:-2, 2:-2, 2:-2] = a[2:-2, 2:-2, 2:-2]
    flow, isf = make(shape, T, padded)
    tri, _ = iso.extract(isf, field_on(flow, inner), LEVEL)
    assert len(tri) > 100 and IR.closed(host(tri))
    assert float(iso.enclosed_volume(tri)) > 0


@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("padded", [True, False])
def test_oblique_plane_on_the_device(T, padded):
    shape = (70, 9, 7)
    Ng = tuple(n + 2 for n in shape)
    g, c = np.array([1 / 32, -0.25, 1.5]), 5.1 + 2.0 ** -30                         # exact in Float32 on half-integer x
    gb, cb = np.array([0.3, -0.2, 0.7]), 1.5
    a, b = linear_field(Ng, g, 0.0, T), linear_field(Ng, gb, cb, T)
    assert np.array_equal(a.astype(F64), linear_field(Ng, g)) and not (a.astype(F64) == c).any()
    flow, isf = make(shape, T, padded)
    tri, val = iso.extract(isf, field_on(flow, a), c, color=field_on(flow, b))
    tri, val = host(tri), host(val)
    check_plane(tri, Ng, g=g, c=c)
    tol = 16 * EPS * float(np.sum(np.abs(gb) * np.array(Ng))) + float(np.spacing(T(np.abs(b).max())))
    d = np.abs(val - (tri @ gb + cb)).max()
    print(f"colour: max |val - (g_b.x + c_b)| = {d:.3e} (bound {tol:.3e})")
    assert d <= tol


@pytest.mark.parametrize("T", [F32, F64])
def test_nan_rule(T):
    shape = (33, 12, 10)
    a, b = random_field(shape, T), colour_field(shape, T)
    at = (17, 6, 5)
    rt, rv, redge, rcube = ref_random(shape, T)
    flow, isf = make(shape, T, True)
    # a NaN corner removes exactly the triangles of its 8 cubes
    an = a.copy()
    an[at] = np.nan
    tri, val = iso.extract(isf, field_on(flow, an), LEVEL, color=field_on(flow, b))
    gone = np.all((rcube <= np.array(at)) & (rcube >= np.array(at) - 1), axis=1)
    assert 0 < gone.sum() <= 8 * 12
    ref_nan = IR.extract(an, LEVEL, b=b)
    assert np.array_equal(ref_nan[0], rt[~gone]) and np.array_equal(ref_nan[2], redge[~gone])
    compare(host(tri), host(val), ref_nan, max(shape) + 2, float(np.abs(b).max()))
    # a NaN in b only: NaN in the values of the vertices whose edge ends there and nowhere else
    bn = b.copy()
    bn[at] = np.nan
    tri, val = iso.extract(isf, field_on(flow, a), LEVEL, color=field_on(flow, bn))
    tri, val = host(tri), host(val)
    touches = np.any(np.all(redge == np.array(at), axis=-1), axis=-1)                # [nt, 3]
    assert touches.sum() > 0 and np.array_equal(np.isnan(val), touches)
    assert np.array_equal(IR.edges_of(tri), redge) and np.abs(tri - rt).max() <= 8 * EPS * (max(shape) + 2)


def raw(flow, a, c, cap, tri, cnt, lo=None, hi=None):
    g = S._grid_of(a, 3)
    i3 = lambda v: None if v is None else (C.c_int32 * 3)(*v)
    _lib.check(_lib.lib().wl_isosurface(S._WLT[S._T(a)], C.byref(g), S._ptr(a), None, float(c), i3(lo), i3(hi),
                                        None if tri is None else S._ptr(tri), None, int(cap), S._ptr(cnt)))
    return [int(x) for x in cnt.cpu()]


def test_capacity():
    shape, T = (70, 9, 7), F32
    flow, isf = make(shape, T, True)
    a = field_on(flow, random_field(shape, T))
    full, _ = iso.extract(isf, a, LEVEL)
    full = host(full)
    total = len(full)
    cap = total // 2
    SENT = -12345.0
    buf = torch.full((total, 3, 3), SENT, dtype=torch.float64, device=flow.device)
    cnt = torch.zeros(2, dtype=torch.int64, device=flow.device)
    assert raw(flow, a, LEVEL, cap, buf, cnt) == [total, cap]
    got = host(buf)
    assert np.array_equal(got[:cap], full[:cap]) and np.all(got[cap:] == SENT)
    assert raw(flow, a, LEVEL, 0, None, cnt) == [total, 0]                          # a pure count
    assert iso.count(isf, a, LEVEL) == total
    small = iso.Isosurface(flow, capacity=7)                                        # too small: extract grows and returns it all
    tri, _ = iso.extract(small, a, LEVEL)
    assert small.capacity == total and np.array_equal(host(tri), full)


def test_boxes():
    shape, T = (33, 12, 10), F64
    flow, isf = make(shape, T, False)
    a = field_on(flow, random_field(shape, T))
    S.perBC(a, (0, 1, 2))                                                           # current ghosts
    h = S.to_host(a)
    Ng = h.shape
    for lo, hi in (((5, 2, 3), (30, 9, 4)), ((0, 0, 0), tuple(n - 1 for n in Ng)), ((0, 3, 0), (Ng[0] - 1, 4, Ng[2] - 1))):
        tri, _ = iso.extract(isf, a, LEVEL, box=(lo, hi))
        ref = IR.extract(h, LEVEL, lo=lo, hi=hi)
        assert len(ref[0]) > 0
        compare(host(tri), None, ref, max(Ng))
    SENT = 777.0
    buf = torch.full((64, 3, 3), SENT, dtype=torch.float64, device=flow.device)
    cnt = torch.full((2,), -1, dtype=torch.int64, device=flow.device)
    for lo, hi in (((4, 4, 4), (4, 9, 9)), ((4, 4, 4), (9, 4, 9)), ((4, 4, 4), (9, 9, 4)), ((4, 4, 4), (4, 4, 4))):   # empty boxes
        assert raw(flow, a, LEVEL, 64, buf, cnt, lo, hi) == [0, 0]
    assert raw(flow, a, float(h.max()) + 1.0, 64, buf, cnt) == [0, 0]                # c above the maximum
    assert np.all(host(buf) == SENT)


def test_same_bits_and_no_allocation():
    shape, T = (70, 9, 7), F32
    flow, isf = make(shape, T, True)
    a, b = field_on(flow, random_field(shape, T)), field_on(flow, colour_field(shape, T))
    L = _lib.lib()

    def allocs():
        n, by = C.c_int64(), C.c_int64()
        assert L.wl_prof_allocs(C.byref(n), C.byref(by)) == 0
        return n.value
    tri, val = iso.extract(isf, a, LEVEL, color=b)
    t0, v0 = host(tri), host(val)
    n0 = allocs()
    for _ in range(10):
        tri, val = iso.extract(isf, a, LEVEL, color=b)
    assert allocs() == n0
    assert np.array_equal(host(tri).view(np.uint64), t0.view(np.uint64)) and np.array_equal(host(val).view(np.uint64), v0.view(np.uint64))


def test_lambda2_plumbing():
    """32^3 Taylor-Green vortex after 3 steps: lambda2() equals extract() of the metric fields the test computes itself"""
    n = 32
    k = 2 * np.pi / n

    def tgv(i, x):
        if i == 0:
            return -np.sin(k * x[0]) * np.cos(k * x[1]) * np.cos(k * x[2])
        if i == 1:
            return np.cos(k * x[0]) * np.sin(k * x[1]) * np.cos(k * x[2])
        return 0.0 * x[0]
    sim = S.Simulation((n, n, n), (0.0, 0.0, 0.0), n / (2 * np.pi), nu=0.01, ulam=tgv, T=F32)
    for _ in range(3):
        S.sim_step(sim)
    isf = iso.Isosurface(sim.flow, capacity=1 << 16)
    lam = S.metric(S.like(sim.flow.p), "lambda2", sim.flow.u)
    om = S.metric(S.like(sim.flow.p), "omega_mag", sim.flow.u)
    h = S.to_host(lam).astype(F64)
    c = float(np.quantile(h[1:-1, 1:-1, 1:-1], 0.2)) + 2.0 ** -30
    assert not (h == c).any()
    for color, b in (("omega_mag", om), ("pressure", sim.flow.p), (None, None)):
        tri, val = iso.lambda2(isf, sim, c, color=color)
        t1, v1 = host(tri), host(val)
        other = iso.Isosurface(sim.flow, capacity=1 << 16)
        tri2, val2 = iso.extract(other, lam, c, color=b)
        assert len(t1) > 100 and np.array_equal(t1, host(tri2))
        assert (v1 is None and val2 is None) if color is None else np.array_equal(v1, host(val2))
    with pytest.raises(ValueError, match="color must be"):
        iso.lambda2(isf, sim, c, color="speed")


def test_slabs():
    """2 ranks sharing the GPU (tests/iso_worker.py): the rank-ordered concatenation is the single-device surface bit for bit"""
    from test_multi_gpu import run_workers
    out = run_workers("iso_worker.py", 2, timeout=300)
    print(out)
    for T in ("float32", "float64"):
        r = out[T]
        assert r["total"] > 1000 and min(r["parts"]) > 0 and sum(r["parts"]) == r["total"]
        assert r["tri_equal"] and r["val_equal"] and r["counts"] == r["parts"]
