"""Budget on the MI355X (waterlily_amd.budget, wl_budget_update / wl_budget_terms) against the numpy restatement of its rules
(budget_ref)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import budget_ref as R  # noqa: E402
from test_budget_cpu import check_shear_terms, shear_field  # noqa: E402
from test_meanflow_gpu import _advance, _close, _sphere  # noqa: E402

from waterlily_amd import budget as B  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
MOMENTS = ("R", "PU", "GG", "T3")


def _check_moments(bg, ref, n, A):
    for k in MOMENTS:
        got = S.to_host(getattr(bg, k))
        assert got.dtype == np.dtype(A)
        _close(got, getattr(ref, k), n, A, k)
    _close(S.to_host(bg.mean.U), ref.mean.U, n, A, "U")
    _close(S.to_host(bg.mean.P), ref.mean.P, n, A, "P")


def _check_terms(bg, ref, nu, A):
    """the device's terms against the restatement fed the DEVICE's moments and mean: one rounding apart at most"""
    got = S.to_host(B.terms(bg, nu))
    want = ref.terms(nu, *(S.to_host(getattr(bg, k)) for k in MOMENTS), U=S.to_host(bg.mean.U))
    assert got.dtype == np.dtype(A) and got.shape == want.shape
    for c, name in enumerate(R.COLUMNS):
        _close(got[..., c], want[..., c], 1, A, name)
    return got


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("pair", [(F32, F32), (F32, F64), (F64, F64)], ids=["f32f32", "f32f64", "f64f64"])
@pytest.mark.parametrize("padded", [True, False], ids=["pitched", "dense"])
def test_parity_random_fields(D, pair, padded):
    """20 updates of random u, p with uneven dt; row lengths leave a tail after the last 16-B vector"""
    T, A = pair
    N = (37, 21) if D == 2 else (29, 14, 9)
    flow = S.Flow(N, (1.0,) * D, T=T, padded=padded)
    bg = B.Budget(flow, dtype=A)
    ref = R.RefBudget(D, A, S.time(flow))
    rng = np.random.default_rng(17 + D)
    n = 20
    for k in range(n):
        S.upload(flow.u, rng.standard_normal(tuple(flow.u.shape)) * 0.3 + 1.0)
        S.upload(flow.p, rng.standard_normal(tuple(flow.p.shape)))
        _advance(flow, 0.1 + 0.4 * rng.random())
        B.update(bg, flow)
        ref.update(S.to_host(flow.u), S.to_host(flow.p), S.time(flow))
    assert bg.t == ref.t and len(bg.t) == n + 1 and B.time(bg) == ref.t[-1] - ref.t[0]
    _check_moments(bg, ref, n, A)
    assert float(np.abs(S.to_host(bg.T3)).max()) > 1e-4
    got = _check_terms(bg, ref, 0.37, A)
    assert float(np.abs(got[..., 7]).max()) > 0


def _storage(a, value):
    """fill every element of a's storage (pitch padding included); returns the flat view and the mask of a's own elements"""
    n = a.untyped_storage().nbytes() // a.element_size()
    flat = a.as_strided((n,), (1,), 0)
    flat.fill_(value)
    idx = torch.zeros(n, dtype=torch.bool)
    off = a.storage_offset() + sum(torch.arange(s).reshape([-1 if e == d else 1 for e in range(a.ndim)]) * st
                                   for d, (s, st) in enumerate(zip(a.shape, a.stride())))
    idx[off.flatten()] = True
    return flat, idx


@pytest.mark.parametrize("padded", [True, False], ids=["pitched", "dense"])
def test_only_inside_is_written_and_first_reads_nothing(padded):
    """NaN in every element of the moments' storage: after the updates the cells of inside() hold numbers (the first update
    read no accumulator: 0 * NaN would have stayed) and every other element, pitch padding included, still holds NaN; the same
    for the result of terms; flow.u and flow.p are unchanged"""
    D, T = 3, F32
    flow = S.Flow((30, 10, 6), (1.0, 0.0, 0.0), T=T, padded=padded)
    rng = np.random.default_rng(3)
    bg = B.Budget(flow)
    out = bg.layout.alloc((8,), flow.device)
    fields = [bg.R, bg.PU, bg.GG, bg.T3, out]
    views = [_storage(a, float("nan")) for a in fields]
    _storage(bg.mean.U, float("nan")), _storage(bg.mean.P, float("nan"))
    for _ in range(5):
        S.upload(flow.u, rng.standard_normal(tuple(flow.u.shape)))
        S.upload(flow.p, rng.standard_normal(tuple(flow.p.shape)))
        u0, p0 = S.to_host(flow.u), S.to_host(flow.p)
        _advance(flow, 0.2)
        B.update(bg, flow)
    assert B.terms(bg, 0.1, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(S.to_host(flow.u), u0) and np.array_equal(S.to_host(flow.p), p0)
    inside = tuple(slice(1, n - 1) for n in flow.p.shape)
    for a, (flat, idx) in zip(fields, views):
        h = S.to_host(a)
        own = np.zeros(h.shape, dtype=bool)
        own[inside] = True
        assert not np.isnan(h[own]).any(), "a cell of inside() was not written, or an accumulator was read on the first update"
        assert np.isnan(h[~own]).all(), "a kernel wrote outside inside()"
        assert bool(torch.isnan(flat.cpu()[~idx]).all()), "a kernel wrote into the pitch padding"
    T8 = S.to_host(out)[inside]
    rim = np.ones(T8.shape[:-1], dtype=bool)
    rim[tuple(slice(1, n - 1) for n in rim.shape)] = False
    assert not T8[rim].any() and np.abs(T8[~rim][:, 0]).min() > 0      # zeros on the rim of inside(), k > 0 within
    assert not np.isnan(S.to_host(bg.mean.U)).any() and not np.isnan(S.to_host(bg.mean.P)).any()


def test_production_in_uniform_shear_on_device():
    """analytic case A (test_budget_cpu) through the kernels, Float64"""
    N, Sh, a, b = (10, 9), 0.25, 0.5, -0.75
    flow = S.Flow((N[0] - 2, N[1] - 2), (1.0, 0.0), T=F64)
    assert tuple(flow.p.shape) == N
    flow.dt = [0.0]
    bg = B.Budget(flow)
    field = shear_field(N, Sh, a, b)
    per, periods = 16, 3
    for n in range(1, periods * per + 1):
        u, p = field(2.0 * np.pi * n / per)
        S.upload(flow.u, u)
        S.upload(flow.p, p)
        flow.dt = [1.0 / per] * n + [0.0]                       # time(flow) = n / per
        B.update(bg, flow)
    assert len(bg.t) == periods * per + 1
    check_shear_terms(S.to_host(B.terms(bg, 0.01)), Sh, a, b)


def test_simulation_reset_noop_vtk_and_no_disturbance(tmp_path):
    from waterlily_amd import vtk
    sim = _sphere()
    bg = B.Budget(sim.flow)
    ref = R.RefBudget(3, F32, S.time(sim.flow))
    for k in range(30):
        S.sim_step(sim, remeasure=False)
        if k == 14:                                         # a new window midway
            B.reset(bg)
            ref.reset()
            assert B.time(bg) == 0.0
        B.update(bg, sim.flow)
        n_t = len(bg.t)
        B.update(bg, sim.flow)                              # no step in between: dt == 0, nothing happens
        assert len(bg.t) == n_t
        ref.update(S.to_host(sim.flow.u), S.to_host(sim.flow.p), S.time(sim.flow))
    assert bg.t == ref.t and len(bg.t) == 17
    _check_moments(bg, ref, 16, F32)
    T8 = _check_terms(bg, ref, sim.flow.nu, F32)
    assert T8[..., 0].max() > 0 and T8[..., 0].min() >= 0 and T8[..., 2].min() >= 0      # k > 0 somewhere; k, dissipation >= 0
    col = B.integrate(B.terms(bg, sim.flow.nu))
    # two Float64 sums of the same numbers in different orders: each within (number of terms) 2^-53 of the sum of magnitudes
    T64 = T8.astype(F64)
    bound = 2 * T64[..., 0].size * 2.0 ** -53 * np.abs(T64).sum(axis=(0, 1, 2))
    assert col.dtype == torch.float64 and np.all(np.abs(col.cpu().numpy() - T64.sum(axis=(0, 1, 2))) <= bound)
    # VTK: the terms and the means read back bitwise
    w = vtk.vtkWriter(str(tmp_path / "tke"), attrib=B.attrib(bg, sim), dir=str(tmp_path / "d"))
    vtk.write(w, sim)
    vtk.close(w)
    got = vtk.read_vti(vtk.read_pvd(str(tmp_path / "tke.pvd"))[-1][1])
    U = S.to_host(bg.mean.U)
    assert got["TKEBudget"].shape[0] == 8 and all(np.array_equal(got["TKEBudget"][c], T8[..., c]) for c in range(8))
    assert np.array_equal(got["MeanPressure"], S.to_host(bg.mean.P))
    assert all(np.array_equal(got["MeanVelocity"][c], U[..., c]) for c in range(3))
    # the budget disturbs nothing: a second run without it takes the same steps bit for bit
    again = _sphere()
    for _ in range(30):
        S.sim_step(again, remeasure=False)
    assert again.flow.dt == sim.flow.dt and again.pois.n == sim.pois.n
    assert np.array_equal(S.to_host(again.flow.u), S.to_host(sim.flow.u))
    assert np.array_equal(S.to_host(again.flow.p), S.to_host(sim.flow.p))
    # Float64 moments of a Float32 flow cannot go to vtk.write (it packs with the flow's T)
    with pytest.raises(TypeError, match="attrib"):
        B.attrib(B.Budget(sim.flow, dtype=F64), sim)
    with pytest.raises(ValueError, match="Float32 accumulators"):
        B.Budget(S.Flow((8, 8), (1.0, 0.0), T=F64), dtype=F32)


def test_slabs_match_undecomposed(tmp_path):
    """2 ranks sharing the GPU (tests/budget_worker.py): gathered owned planes of the slab run's moments and terms against the
    undecomposed run's"""
    from test_multi_gpu import run_workers
    out = run_workers("budget_worker.py", 2, WL_TMP=str(tmp_path), timeout=300)
    tol = 2e-5                                      # the slab tests' tolerance for u (test_multi_gpu.check, Float32)
    assert out["n_ref"] == out["n_slab"] and out["t_ref"] == out["t_slab"], out
    for k in out["velocity_derived"]:
        assert out["d_" + k] < tol, (k, out)
    for k in out["pressure_derived"]:
        assert out["d_" + k] < 20 * tol, (k, out)      # (p: 20x, as there)
    assert set(out["velocity_derived"]) | set(out["pressure_derived"]) == {"U", "P", "R", "PU", "GG", "T3"} | set(R.COLUMNS)
    assert out["k_max"] > 0
