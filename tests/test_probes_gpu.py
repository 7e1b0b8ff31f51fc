"""Point probes and tracers on the MI355X (waterlily_amd.probes: wl_interp, wl_tracer_advance) against the restatement and
the exact evaluator of tests/probes_ref.py, closed forms, and an undecomposed / 2-rank slab pair."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probes_ref as R  # noqa: E402

from waterlily_amd import probes as P  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS = np.finfo(np.float64).eps


def field(host, T, padded=True, vector=False):
    """a device field (the library's layout) holding the dense host array"""
    D = host.ndim - (1 if vector else 0)
    lay = S.Layout(host.shape[:D], T, padded=padded)
    a = lay.alloc((D,) if vector else (), "cuda:0")
    S.upload(a, host)
    return a


@pytest.mark.parametrize("T", [F32, F64])
def test_maintests_answers(T):
    """test/maintests.jl:58-64 on the device"""
    a = field(R.fill_faces((5, 5), lambda i, x: x[i] + 1.5, T), T, vector=True)
    b = field(R.fill_centres((5, 5), lambda x: x[0] + 1.5, T), T)
    assert np.array_equal(P.interp((2.5, 1), a), [2.5, 1.0])
    assert np.array_equal(P.interp((3.5, 3), a), [3.5, 3.0])
    assert P.interp((2.5, 1), b) == 2.5 and P.interp((3.5, 3), b) == 3.5
    v = P.interp(np.array([[2.5, 1], [3.5, 3]]), a)
    assert v.shape == (2, 2) and v.dtype == np.float64 and np.array_equal(v, [[2.5, 1.0], [3.5, 3.0]])
    assert P.interp(np.array([[2.5, 1], [3.5, 3]]), b).shape == (2,)


def _points(shape, rng, n=160):
    """random points over the whole array and beyond it, integer coordinates, x_d == n_d, ghost cells, just outside"""
    D = len(shape)
    hi = np.array(shape, dtype=np.float64)
    X = [rng.uniform(0.75, hi + 0.6, size=D) for _ in range(n)]
    for _ in range(n // 4):
        x = rng.uniform(1, hi, size=D)
        k = rng.random(D) < 0.5
        x[k] = np.floor(x[k])
        X.append(x)
    for d in range(D):
        for v in (1.0, 1.25, hi[d] - 0.5, hi[d], hi[d] + 2 ** -40, 1.0 - 2 ** -40, hi[d] - 1.0):
            x = rng.uniform(1.5, hi - 0.5, size=D)
            x[d] = v
            X.append(x)
    return np.array(X)


def _field_values(shape, rng):
    """tie-rich: multiples of 1/8 in [-4, 4] mixed with normals and a few large values"""
    a = rng.integers(-32, 33, size=shape) / 8.0
    k = rng.random(shape) < 0.4
    a[k] = rng.standard_normal(int(k.sum())) * 3
    a[rng.random(shape) < 0.02] = 1e4
    return a


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("padded", [True, False], ids=["pitched", "dense"])
def test_random_fields_exact_and_restatement(D, T, padded):
    rng = np.random.default_rng(100 * D + (T == F32) + 2 * padded)
    shape = (13, 9) if D == 2 else (11, 7, 6)
    a_h = _field_values(shape, rng).astype(T)
    u_h = _field_values(shape + (D,), rng).astype(T)
    a, u = field(a_h, T, padded), field(u_h, T, padded, vector=True)
    X = _points(shape, rng)
    ga, gu = P.interp(X, a), P.interp(X, u)
    assert ga.shape == (len(X),) and gu.shape == (len(X), D)
    K = (2 ** D + D + 2) * EPS
    nan_seen = 0
    for q, x in enumerate(X):
        for c, got in [(None, ga[q])] + [(c, gu[q, c]) for c in range(D)]:
            want, bound = R.exact(x, a_h if c is None else u_h, c)
            if np.isnan(want):
                assert np.isnan(got), (x, c, got)
                nan_seen += 1
            else:
                assert abs(got - want) <= K * bound, (x, c, got, want, bound)
    assert nan_seen > 20
    # the restatement in the kernel's order: bitwise (checked within 2 ulp of the scale)
    ra, ru = R.interp_many(X, a_h, False), R.interp_many(X, u_h, True)
    scale = float(np.nanmax(np.abs(a_h)))
    for got, want in ((ga, ra), (gu, ru)):
        assert np.array_equal(np.isnan(got), np.isnan(want))
        k = ~np.isnan(want)
        assert np.max(np.abs(got[k] - want[k])) <= 2 * EPS * scale
    # negative control: the restatement without the stagger shift disagrees
    drop = np.array([[R.interp(x, u_h[..., c]) for c in range(D)] for x in X])
    k = ~np.isnan(drop) & ~np.isnan(gu)
    assert np.max(np.abs(gu[k] - drop[k])) > 1e3 * EPS * scale


@pytest.mark.parametrize("T", [F32, F64])
def test_linear_fields_reproduced(T):
    """a linear field (dyadic coefficients: exact in Float32) is reproduced to rounding, at cell centres and at faces"""
    shape = (12, 10, 7)
    lin = lambda x: 0.25 * x[0] - 0.5 * x[1] + 0.125 * x[2] + 3.0
    a = field(R.fill_centres(shape, lin, T), T)
    u = field(R.fill_faces(shape, lambda i, x: lin(x) * (i + 1), T), T, vector=True)
    rng = np.random.default_rng(4)
    X = rng.uniform(1.5, np.array(shape) - 0.5, size=(300, 3))
    want = lin(X.T - 1.5)
    assert np.max(np.abs(P.interp(X, a) - want)) <= 1e-14 * 10
    gu = P.interp(X, u)
    for c in range(3):
        assert np.max(np.abs(gu[:, c] - want * (c + 1))) <= 1e-14 * 30


def _sphere(T=F32, m=32):
    Rr, c = m / 8, m / 2 - 1
    return S.Simulation((m, m, m), (1.0, 0.0, 0.0), 2 * Rr, nu=2 * Rr / 3700, body=AutoBody(lambda x, t: norm2(x - c) - Rr), T=T)


def test_probes_on_sphere():
    """10 steps of the 32^3 sphere: every record equals interp of that step's host copies of u and p; the run is bit-identical
    to one without probes; growth of the buffer keeps earlier rows; reset clears the series"""
    rng = np.random.default_rng(9)
    sim, bare = _sphere(), _sphere()
    X = np.concatenate([rng.uniform(1.5, 33.5, size=(24, 3)), [[17.5, 15.5, 15.5], [1.0, 1.0, 1.0], [34.0, 34.0, 34.0],
                                                                [34.5, 10.0, 10.0]]])
    pr = P.Probes(sim.flow, X, capacity=3)
    want, times = [], []
    for _ in range(10):
        S.sim_step(sim, remeasure=False)
        S.sim_step(bare, remeasure=False)
        P.record(pr, sim.flow)
        times.append(S.time(sim.flow))
        u, p = S.to_host(sim.flow.u), S.to_host(sim.flow.p)
        want.append(np.concatenate([R.interp_many(X, u, True), R.interp_many(X, p, False)[:, None]], axis=1))
    assert pr.buf.shape[0] == 12
    t, v = P.series(pr)
    want = np.array(want)
    assert v.shape == (10, len(X), 4) and t.tolist() == times
    assert np.array_equal(np.isnan(v), np.isnan(want)) and np.isnan(v[:, -1]).all() and not np.isnan(v[:, :-2]).any()
    scale = float(np.nanmax(np.abs(want)))
    assert np.nanmax(np.abs(v - want)) <= 2 * EPS * scale
    assert np.nanmax(np.abs(v[-1, :, 3])) > 0 and np.nanmax(np.abs(v[-1, :, 0] - 1)) > 1e-3    # a flow is seen, not a constant
    assert sim.flow.dt == bare.flow.dt and sim.pois.n == bare.pois.n
    assert np.array_equal(S.to_host(sim.flow.u), S.to_host(bare.flow.u))
    assert np.array_equal(S.to_host(sim.flow.p), S.to_host(bare.flow.p))
    P.reset(pr)
    assert len(P.series(pr)[0]) == 0
    P.record(pr, sim.flow)
    t1, v1 = P.series(pr)
    assert t1.tolist() == [S.time(sim.flow)] and np.array_equal(v1[0], v[-1], equal_nan=True)


def _uniform_flow(N, U, T=F64, perdir=()):
    flow = S.Flow(N, U, T=T, perdir=perdir)
    h = np.zeros(tuple(flow.u.shape))
    for c, v in enumerate(U):
        h[..., c] = v
    S.upload(flow.u, h)
    return flow


def test_tracers_uniform_flow_translates():
    U = (0.5, -0.25, 0.125)
    flow = _uniform_flow((16, 12, 8), U, T=F32)
    rng = np.random.default_rng(1)
    x0 = rng.integers(64, 128, size=(1000, 3)) / 16.0                # dyadic: every weight and sum is exact
    tr = P.Tracers(flow, x0)
    for _ in range(4):
        P.advance(tr, flow, dt=0.75)
    assert np.array_equal(P.positions(tr), x0 + 4 * 0.75 * np.array(U)) and P.alive(tr) == 1000


@pytest.mark.parametrize("D", [2, 3])
def test_tracers_rotation_radius(D):
    """solid-body rotation (linear, so interpolated exactly): each Heun step grows the radius by sqrt(1 + (om dt)^4 / 4)"""
    N = (32, 32) if D == 2 else (32, 32, 4)
    om, dt, cen = 0.04, 0.9, (16.0, 16.0)

    def f(i, x):
        return -om * (x[1] - cen[1]) if i == 0 else (om * (x[0] - cen[0]) if i == 1 else 0 * x[0])
    flow = S.Flow(N, (0.0,) * D, T=F64)
    S.upload(flow.u, R.fill_faces(tuple(n + 2 for n in N), f))
    th = np.linspace(0, 2 * np.pi, 64, endpoint=False)
    r0 = np.linspace(2, 12, 64)
    x0 = np.stack([cen[0] + 1.5 + r0 * np.cos(th), cen[1] + 1.5 + r0 * np.sin(th)] + [np.full(64, 2.75)] * (D - 2), axis=1)
    tr = P.Tracers(flow, x0)
    g = np.sqrt(1 + (om * dt) ** 4 / 4)
    for n in range(1, 9):
        P.advance(tr, flow, dt=dt)
        x = P.positions(tr)
        r = np.hypot(x[:, 0] - cen[0] - 1.5, x[:, 1] - cen[1] - 1.5)
        np.testing.assert_allclose(r / r0, g ** n, rtol=1e-13, atol=0)
        np.testing.assert_array_equal(x, R.heun(x0 if n == 1 else xp, S.to_host(flow.u), dt))
        xp = x


def test_tracers_wrap_death_and_dead_stay_dead():
    flow = _uniform_flow((8, 6), (1.0, -0.5), perdir=(0,))
    X = np.array([[9.0, 4.0], [3.0, 2.0], [5.0, 1.75], [8.75, 7.0]])
    tr = P.Tracers(flow, X)
    u = S.to_host(flow.u)
    want = X
    for _ in range(3):
        P.advance(tr, flow, dt=1.0)
        want = R.heun(want, u, 1.0, perdir=(0,))
        np.testing.assert_array_equal(P.positions(tr), want)
    assert np.array_equal(want[0], [4.0, 2.5]) and np.isnan(want[1:3]).all() and P.alive(tr) == 2


def test_tracers_in_sphere_flow_match_numpy_and_sorting_keeps_trajectories():
    sim = _sphere()
    for _ in range(3):
        S.sim_step(sim, remeasure=False)
    rng = np.random.default_rng(12)
    x0 = rng.uniform(1.5, 33.5, size=(600, 3))
    x0[:40, 0] = rng.uniform(33.0, 33.5, size=40)             # near the exit: some leave
    tr, ts = P.Tracers(sim.flow, x0), P.Tracers(sim.flow, x0, sort_every=1)
    want = x0
    for _ in range(3):
        S.sim_step(sim, remeasure=False)
        P.advance(tr, sim.flow)
        P.advance(ts, sim.flow)
        want = R.heun(want, S.to_host(sim.flow.u), sim.flow.dt[-2])
        got = P.positions(tr)
        assert np.array_equal(np.isnan(got), np.isnan(want))
        k = ~np.isnan(want)
        assert np.max(np.abs(got[k] - want[k])) <= 2 * EPS * 34
        np.testing.assert_array_equal(P.positions(ts), got)
    assert 0 < P.alive(tr) < 600 and P.alive(ts) == P.alive(tr)
    assert not np.array_equal(ts.id.cpu().numpy(), np.arange(600))       # the sorted set was reordered


def test_slabs():
    """2 ranks sharing the GPU (tests/probes_worker.py)"""
    from test_multi_gpu import run_workers
    out = run_workers("probes_worker.py", 2, timeout=300)
    assert out["t_equal"] and out["bitwise_own"] and out["d_own"] == 0.0, out
    assert out["nan_rows"] == 4, out                          # z = 0.75, 34.25; u_z beyond the top at z = 33.75, 34.0
    tol = 2e-5                                                # the slab tests' tolerance for u (as meanflow_worker.py)
    assert out["d_u_ref"] < tol and out["d_p_ref"] < 20 * tol, out
    assert out["ring_bitwise"] and out["ring_d"] == 0.0 and out["ring_ghost_values"] == 4, out
    assert out["tracers_refused"], out
