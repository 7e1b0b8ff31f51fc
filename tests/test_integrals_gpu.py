"""Integrals on the MI355X (waterlily_amd.integrals: wl_flow_integrals) against the longdouble restatement of
tests/integrals_ref.py: parity at the dispatch-edge shapes, exact closed forms, determinism, NaN, untouched inputs, the
recorder in live runs, and a 2-rank z-slab run.

Tolerance (derived, integrals_ref.tolerance): a summed column over n cells within (n + 48) 2^-53 sum|term|, divmax within
8 * 2^-53 * sum_i (|u[I+d_i,i]| + |u[I,i]|) at the maximising cell, umax exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import integrals_ref as R  # noqa: E402
from xref_inputs import field  # noqa: E402

from waterlily_amd import _lib  # noqa: E402
from waterlily_amd import integrals as I  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SENTINEL = -12345.678
WORST = {}


def V(T):
    return 4 if np.dtype(T) == np.float32 else 2


def shapes3(T):
    """the dispatch-edge shapes of tests/test_xref_gpu.py (interior extents)"""
    v = V(T)
    return [(v - 1, 5, 1), (v, 4, 2), (v + 1, 9, 3), (63 * v, 8, 5), (64 * v, 3, 6), (65 * v, 5, 5)]


def dev(h, D, padded):
    """a device field holding the dense host array, its row padding poisoned"""
    lay = S.Layout(h.shape[:D], h.dtype, padded)
    a = lay.alloc(h.shape[D:], "cuda:0")
    span = 1 + sum((n - 1) * s for n, s in zip(a.shape, a.stride()))
    torch.as_strided(a, (span + lay.align,), (1,), a.storage_offset() - lay.lead).fill_(1e30)
    S.upload(a, h)
    return a


def raw(a, D, U=None, pad=8):
    """wl_flow_integrals on a device vector field: (row[6+D], the sentinel-filled buffer around it)"""
    buf = torch.full((pad + 6 + D + pad,), SENTINEL, dtype=torch.float64, device=a.device)
    g = S._grid_of(a, D)
    row = buf[pad:pad + 6 + D]
    _lib.check(_lib.lib().wl_flow_integrals(S._WLT[S._T(a)], C.byref(g), S._ptr(a), _lib.d3((0,) * 3 if U is None else U),
                                            S._ptr(row)))
    h = buf.cpu().numpy()
    return h[pad:pad + 6 + D].copy(), h


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("padded", [True, False], ids=["pitched", "dense"])
def test_parity_with_restatement(D, T, padded):
    """random / tie-rich / scaled fields at the edge shapes (rows shorter than a wavefront, one past a multiple of 64, fewer
    than four rows, one interior plane), a shape with several marching chunks of several planes, and (2-D) more tiles than
    the grid cap; a non-zero background velocity"""
    if D == 3:
        shapes = shapes3(T) + [(130, 200, 40)]
    else:
        shapes = [s[:2] for s in shapes3(T)] + [(1, 1), (130, 3), (1024, 1028)]
    kinds = ["random", "ties", "scaled-up", "random", "scaled-down", "random", "random", "ties", "random"]
    U = (0.25, -0.5, 0.125)[:D]
    for q, s in enumerate(shapes):
        Ng = tuple(n + 2 for n in s)
        kind = kinds[q % len(kinds)]
        h = field(Ng + (D,), T, kind, 900 + 10 * q + D)
        scale = float(np.abs(h).max())
        Uq = tuple(scale * x for x in U)
        got, _ = raw(dev(h, D, padded), D, Uq)
        w = R.check(got, h, Uq)
        key = f"{D}D-{np.dtype(T).name}"
        WORST[key] = max(WORST.get(key, 0.0), w)
        print(f"  {key} {'pitched' if padded else 'dense'} {s} {kind}: worst |got-ref|/tol = {w:.3g}")
        assert got[0] > 0 and got[1] > 0 and got[2] > 0 and got[5] > 0
    # negative control: the restatement of a field shifted by one cell along x must fail the same check
    h2 = np.roll(h, 1, axis=0)
    with pytest.raises(AssertionError):
        R.check(got, h2, Uq)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("T", [F32, F64])
def test_closed_forms_bit_for_bit(D, T):
    for label, Ng, f, U, spec in R.pins(D):
        h = R.index_field(Ng, f, T)
        for padded in (True, False):
            got, _ = raw(dev(h, D, padded), D, U)
            R.check_pin(got, spec, Ng, label)
            ref, _, _ = R.integrals(h, U)
            assert np.array_equal(got, np.asarray(ref, dtype=np.float64)), (label, got, ref)   # small integers: every operation exact


@pytest.mark.parametrize("T", [F32, F64])
def test_deterministic_and_nan(T):
    Ng = (200, 37, 21)
    h = field(Ng + (3,), T, "random", 77)
    a = dev(h, 3, True)
    r1, _ = raw(a, 3)
    r2, _ = raw(a, 3)
    assert r1.tobytes() == r2.tobytes()
    b = dev(h, 3, True)                                       # another allocation, same values
    assert raw(b, 3)[0].tobytes() == r1.tobytes()
    h[77, 20, 9, 1] = np.nan
    got, _ = raw(dev(h, 3, True), 3)
    assert np.isnan(got[:4]).all(), got
    assert not np.isnan(got[4:6]).any()                       # the maxima skip NaN (RED_MAX's comparison)
    ref, _, _ = R.integrals(h)
    assert got[5] == float(ref[5])
    h2 = field((30, 9, 2), T, "random", 78)
    h2[5, 4, 0] = np.nan
    got2, _ = raw(dev(h2, 2, False), 2)
    assert np.isnan(got2[:4]).all(), got2


@pytest.mark.parametrize("D", [2, 3])
def test_inputs_untouched_and_row_only(D):
    Ng = (70, 11, 6)[:D] if D == 3 else (70, 11)
    h = field(Ng + (D,), F32, "random", 5)
    a = dev(h, D, True)
    span = 1 + sum((n - 1) * s for n, s in zip(a.shape, a.stride()))
    whole = torch.as_strided(a, (span,), (1,), a.storage_offset())
    before = whole.clone()
    got, buf = raw(a, D, (0.5,) * D)
    assert torch.equal(whole, before)
    assert np.all(buf[:8] == SENTINEL) and np.all(buf[8 + 6 + D:] == SENTINEL) and not np.any(got == SENTINEL)
    R.check(got, h, (0.5,) * D)


def _sphere(T=F32, m=32):
    Rr, c = m / 8, m / 2 - 1
    return S.Simulation((m, m, m), (1.0, 0.0, 0.0), 2 * Rr, nu=2 * Rr / 3700, body=AutoBody(lambda x, t: norm2(x - c) - Rr), T=T)


def _tgv2(T=F64, Lg=64):
    k = 2 * np.pi / Lg

    def tgv(i, xy):
        x, y = xy[0] * k, xy[1] * k
        return -np.sin(x) * np.cos(y) if i == 0 else np.cos(x) * np.sin(y)
    return S.Simulation((Lg, Lg), (0.0, 0.0), Lg, U=1, ulam=tgv, nu=1 / (k * 100.0), T=T, perdir=(0, 1))


@pytest.mark.parametrize("case", ["tgv-2d-f64", "sphere-3d-f32"])
def test_recorder_in_a_live_run(case):
    """12 steps with record after each, capacity 4 (the buffer grows twice): every row equals the restatement on that step's
    host copy of u, t equals time(flow), reset empties the series, the one-off integrals() equals the last row, and u, p and
    the time steps are bitwise those of the same run without a recorder"""
    make = _tgv2 if case.startswith("tgv") else _sphere
    sim, bare = make(), make()
    D = sim.flow.D
    U = (0.0, 0.0) if D == 2 else (1.0, 0.0, 0.0)
    ig = I.Integrals(sim.flow, U=U, capacity=4)
    assert I.columns(ig) == R.names(D)
    fields, times = [], []
    for _ in range(12):
        S.sim_step(sim, remeasure=False)
        S.sim_step(bare, remeasure=False)
        I.record(ig, sim.flow)
        times.append(S.time(sim.flow))
        fields.append(S.to_host(sim.flow.u))
    assert ig.buf.shape[0] == 16
    t, v = I.series(ig)
    assert v.shape == (12, 6 + D) and v.dtype == np.float64 and t.tolist() == times
    for k in range(12):
        w = R.check(v[k], fields[k], U)
        print(f"  {case} step {k}: E={v[k, 0]:.9g} Z={v[k, 1]:.9g} S={v[k, 2]:.9g} divmax={v[k, 4]:.3g} umax={v[k, 5]:.6g} worst={w:.3g}")
    assert v[-1, 0] > 0 and v[-1, 1] > 0 and len(set(v[:, 1].tolist())) == 12          # a flow is seen, and it evolves
    if D == 2:
        assert np.all(np.diff(v[:, 0]) < 0)                                              # viscous decay of the vortex
    one = I.integrals(sim.flow, U=U)
    assert tuple(one) == R.names(D) and np.array_equal(np.array(list(one.values())), v[-1])
    assert sim.flow.dt == bare.flow.dt and sim.pois.n == bare.pois.n
    assert np.array_equal(S.to_host(sim.flow.u), S.to_host(bare.flow.u))
    assert np.array_equal(S.to_host(sim.flow.p), S.to_host(bare.flow.p))
    I.reset(ig)
    assert len(I.series(ig)[0]) == 0 and I.series(ig)[1].shape == (0, 6 + D)
    I.record(ig, sim.flow)
    t1, v1 = I.series(ig)
    assert t1.tolist() == [S.time(sim.flow)] and np.array_equal(v1[0], v[-1])
    with pytest.raises(ValueError):
        I.record(ig, S.Flow((8, 8) if D == 3 else (8, 8, 8), (0.0,) * (5 - D)))


def test_slabs():
    """2 ranks sharing the GPU (tests/integrals_worker.py)"""
    from test_multi_gpu import run_workers
    out = run_workers("integrals_worker.py", 2, timeout=300)
    assert out["t_equal"] and out["rows"] == 4, out
    assert out["within_bound"] and out["worst"] <= 1.0, out
    assert out["one_off_equal"] and out["local_rows_differ"], out
    assert out["ring_within_bound"], out


def test_worst_ratios_are_recorded():
    """(prints the largest |got - ref| / tolerance seen in this module: -s shows it)"""
    print("\nworst |got-ref|/tol:", {k: round(v, 4) for k, v in sorted(WORST.items())})
