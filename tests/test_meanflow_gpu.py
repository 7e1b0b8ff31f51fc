"""MeanFlow on the MI355X (waterlily_amd.stats, wl_meanflow_update) against the numpy restatement of its rule (meanflow_ref)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import meanflow_ref as R  # noqa: E402

from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd import stats as M  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64


def _advance(flow, dt):
    """move time(flow) = sum(dt[:-1]) on by dt without a step"""
    flow.dt.insert(len(flow.dt) - 1, float(dt))


def _close(got, want, n, A, what):
    """the kernel and the restatement round the same double operations (hipcc is run with -ffp-contract=off); a bound of
    4 ulp of the accumulator type per update, on the scale of the field, leaves room for contraction should it ever differ"""
    scale = max(1.0, float(np.max(np.abs(want))))
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    assert err <= 4 * n * np.finfo(A).eps * scale, (what, err, scale)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("pair", [(F32, F32), (F32, F64), (F64, F64)], ids=["f32f32", "f32f64", "f64f64"])
@pytest.mark.parametrize("padded", [True, False], ids=["pitched", "dense"])
def test_parity_random_fields(D, pair, padded):
    """~20 updates of random u, p with uneven dt, every statistic on; row lengths leave a tail after the last 16-B vector"""
    T, A = pair
    N = (37, 21) if D == 2 else (29, 14, 9)
    flow = S.Flow(N, (1.0,) * D, T=T, padded=padded)
    mf = M.MeanFlow(flow, uu_stats=True, pp_stats=True, dtype=A)
    ref = R.RefMean(D, A, S.time(flow))
    rng = np.random.default_rng(7 + D)
    n = 0
    for k in range(20):
        u = rng.standard_normal(tuple(flow.u.shape)) * 0.3 + 1.0
        p = rng.standard_normal(tuple(flow.p.shape))
        S.upload(flow.u, u)
        S.upload(flow.p, p)
        _advance(flow, 0.1 + 0.4 * rng.random())
        M.update(mf, flow)
        ref.update(S.to_host(flow.u), S.to_host(flow.p), S.time(flow))
        n += 1
    assert mf.t == ref.t and len(mf.t) == 21
    for k in ("U", "P", "UU", "pp"):
        got = S.to_host(getattr(mf, k))
        assert got.dtype == np.dtype(A)
        _close(got, getattr(ref, k), n, A, k)


@pytest.mark.parametrize("padded", [True, False], ids=["pitched", "dense"])
def test_constant_field_exact_and_padding_untouched(padded):
    D, T = 3, F32
    flow = S.Flow((30, 10, 6), (1.0, 0.0, 0.0), T=T, padded=padded)
    rng = np.random.default_rng(3)
    S.upload(flow.u, rng.standard_normal(tuple(flow.u.shape)))
    S.upload(flow.p, rng.standard_normal(tuple(flow.p.shape)))
    u0, p0 = S.to_host(flow.u), S.to_host(flow.p)
    mf = M.MeanFlow(flow, uu_stats=True, pp_stats=True)
    sentinel = -7.25e30
    flats, masks = [], []
    for a in (mf.U, mf.P, mf.UU, mf.pp):
        n = a.untyped_storage().nbytes() // a.element_size()
        flat = a.as_strided((n,), (1,), 0)
        flat.fill_(sentinel)                                   # valid elements too: the first update must not read them
        idx = torch.zeros(n, dtype=torch.bool)
        off = a.storage_offset() + sum(torch.arange(s).reshape([-1 if e == d else 1 for e in range(a.ndim)]) * st
                                       for d, (s, st) in enumerate(zip(a.shape, a.stride())))
        idx[off.flatten()] = True
        flats.append(flat)
        masks.append(idx)
    for _ in range(7):
        _advance(flow, 0.2)
        M.update(mf, flow)
    torch.cuda.synchronize()
    assert np.array_equal(S.to_host(mf.U), u0) and np.array_equal(S.to_host(mf.P), p0)
    assert not S.to_host(mf.UU).any() and not S.to_host(mf.pp).any()
    for flat, idx in zip(flats, masks):
        h = flat.cpu()
        assert bool((h[~idx] == sentinel).all()), "an update wrote outside the array's elements (pitch padding)"
        assert not bool((h[idx] == sentinel).any())
    assert np.array_equal(S.to_host(flow.u), u0) and np.array_equal(S.to_host(flow.p), p0)


def test_cancellation_covariance_on_device():
    """the synthetic signal of test_meanflow_cpu.test_covariance_not_cancellation through the kernel: Float32 accumulators hold
    the covariance to the bound derived there; the naive Float32 form of the same samples misses by more than 100 %"""
    from test_meanflow_cpu import ROBUST_BOUND
    xs, dts = R.cancellation_signal()
    flow = S.Flow((8, 8), (1.0, 0.0), T=F32)
    flow.dt = [0.0]
    mf = M.MeanFlow(flow, uu_stats=True, pp_stats=True)
    for x, dt in zip(xs, dts):
        flow.u.fill_(float(np.float32(x)))
        flow.p.fill_(float(np.float32(x)))
        _advance(flow, dt)
        M.update(mf, flow)
    ex = R.exact_variance(xs, dts)
    uu, pp = S.to_host(mf.UU), S.to_host(mf.pp)
    for got in (uu[..., 0], uu[..., 1], uu[..., 2], pp):
        assert np.all(np.abs(got.astype(np.float64) - ex) / ex < ROBUST_BOUND), float(np.max(np.abs(got - ex) / ex))
    assert np.all(S.to_host(mf.UU)[..., 2] == S.to_host(mf.UU)[..., 0])          # xy of identical components = xx
    assert abs(R.naive_variance(xs, dts) - ex) / ex > 1.0


def _sphere(T=F32):
    from waterlily_amd.body import AutoBody, norm2
    m = 32
    R_, c = m / 8, m / 2 - 1
    return S.Simulation((2 * m, m, m), (1.0, 0.0, 0.0), 2 * R_, nu=2 * R_ / 3700, body=AutoBody(lambda x, t: norm2(x - c) - R_), T=T)


def test_simulation_reset_noop_vtk_and_no_disturbance(tmp_path):
    from waterlily_amd import vtk
    sim = _sphere()
    mf = M.MeanFlow(sim.flow, uu_stats=True, pp_stats=True)
    ref = R.RefMean(3, F32, S.time(sim.flow))
    for k in range(30):
        S.sim_step(sim, remeasure=False)
        if k == 14:                                         # a new window midway
            M.reset(mf)
            ref.reset()
            assert M.time(mf) == 0.0
        M.update(mf, sim.flow)
        n_t = len(mf.t)
        M.update(mf, sim.flow)                              # no step in between: dt == 0, nothing happens
        assert len(mf.t) == n_t
        ref.update(S.to_host(sim.flow.u), S.to_host(sim.flow.p), S.time(sim.flow))
    assert mf.t == ref.t and M.time(mf) == ref.t[-1] - ref.t[0] and len(mf.t) == 17
    for k in ("U", "P", "UU", "pp"):
        _close(S.to_host(getattr(mf, k)), getattr(ref, k), 16, F32, k)
    assert np.abs(S.to_host(mf.UU)[..., 0]).max() > 0
    # VTK: the averages read back bitwise
    w = vtk.vtkWriter(str(tmp_path / "mean"), attrib=M.mean_attrib(mf), dir=str(tmp_path / "d"))
    vtk.write(w, sim)
    vtk.close(w)
    got = vtk.read_vti(vtk.read_pvd(str(tmp_path / "mean.pvd"))[-1][1])
    U, UU = S.to_host(mf.U), S.to_host(mf.UU)
    assert np.array_equal(got["MeanPressure"], S.to_host(mf.P)) and np.array_equal(got["PressureVariance"], S.to_host(mf.pp))
    assert all(np.array_equal(got["MeanVelocity"][c], U[..., c]) for c in range(3))
    assert got["ReynoldsStress"].shape[0] == 6 and all(np.array_equal(got["ReynoldsStress"][c], UU[..., c]) for c in range(6))
    # averaging disturbs nothing: a second run without MeanFlow takes the same steps bit for bit
    again = _sphere()
    for _ in range(30):
        S.sim_step(again, remeasure=False)
    assert again.flow.dt == sim.flow.dt and again.pois.n == sim.pois.n
    assert np.array_equal(S.to_host(again.flow.u), S.to_host(sim.flow.u))
    assert np.array_equal(S.to_host(again.flow.p), S.to_host(sim.flow.p))
    # Float64 averages of a Float32 flow cannot go to vtk.write (it packs with the flow's T)
    with pytest.raises(TypeError, match="mean_attrib"):
        M.mean_attrib(M.MeanFlow(sim.flow, dtype=F64))


def test_slabs_match_undecomposed(tmp_path):
    """2 ranks sharing the GPU (tests/meanflow_worker.py): gathered owned planes of the slab run's averages against the
    undecomposed run's, and a two-piece VTK file of mean_attrib against the one-device file (the shared plane of the pieces
    is rank 0's halo copy: it checks that the halo planes are averaged too)"""
    from test_multi_gpu import run_workers
    out = run_workers("meanflow_worker.py", 2, WL_TMP=str(tmp_path), timeout=300)
    tol = 2e-5                                      # the slab tests' tolerance for u (test_multi_gpu.check, Float32)
    assert out["n_ref"] == out["n_slab"] and out["t_ref"] == out["t_slab"], out
    for k in ("U", "UU", "vtk_MeanVelocity", "vtk_ReynoldsStress"):
        assert out["d_" + k] < tol, (k, out)
    for k in ("P", "pp", "vtk_MeanPressure", "vtk_PressureVariance"):
        assert out["d_" + k] < 20 * tol, (k, out)      # (p: 20x, as there)
    assert out["pieces"] == 2 and out["shared_plane_checked"]
