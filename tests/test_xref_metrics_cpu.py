"""The CPU oracle's Metrics.jl read-outs (oracle/wlo_impl.h: wlo_metric, wlo_pforce, wlo_vforce, wlo_pmoment) against the
independent extended-precision reference tests/xref_metrics.py: field metrics |oracle - ref| <= K * eps_T * M per cell,
band sums |oracle - ref| <= (K * eps_T + n * eps_64 / 2) * M.  The oracle was written beside the kernels and shares their
formulas; this file is what keeps the pair honest.  Every comparison carries a negative control that must FAIL."""
import numpy as np
import pytest

import xref as X
import xref_metrics as XM
from oracle import wl_oracle as O
from xref_inputs import field

TYPES = [np.float32, np.float64]
K = XM.K
WORST = {}
KINDS, SPECIAL, X0, inside, synthetic_band = XM.KINDS, XM.SPECIAL, XM.X0, XM.inside, XM.synthetic_band


def check(name, got, v, M, T, control=True):
    w = X.worst(got, v, M, T)
    key = f"{name} {np.dtype(T).name}"
    WORST[key] = max(WORST.get(key, 0.0), w)
    assert w <= K[name], f"{key}: |oracle-ref| = {w:.3g} eps*M > K = {K[name]}"
    assert not control or X.worst(got[:-1], v[1:], M[1:], T) > K[name], f"{key}: control (samples shifted by one) did not fail"
    return w


def metric(kind, u, Ng, **kw):
    return O.metric(O.zeros(Ng, u.dtype.type), kind, u, **kw).ravel(order="F")


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(7, 6, 5), (9, 8, 3), (10, 9)])
@pytest.mark.parametrize("kind", KINDS)
def test_field_metrics_oracle_vs_xref(T, Ng, kind):
    """ke with and without U (K = 4), every curl component the dimension has (K = 4), and in 3-D |ω| (K = 8), ω_θ about an
    oblique axis (K = 16) and λ₂ (K = 16), on the adversarial fields; control: the samples shifted by one cell fail"""
    D = len(Ng)
    u = field(Ng + (D,), T, kind, 21)
    C = X.host_cells({"u": u}, N=Ng)
    ins = inside(C, Ng)
    s = float(np.max(np.abs(u)))
    for U in (None, (0.25 * s, -0.5 * s, 0.125 * s)[:D]):
        v, M = XM.ke(C, U)
        check("ke", metric("ke", u, Ng, par=U)[ins], v[ins], M[ins], T)
    for i in (range(3) if D == 3 else (2,)):
        v, M = XM.curl(C, i)
        check("curl", metric("curl", u, Ng, i=i)[ins], v[ins], M[ins], T, control=kind != "ties")
    if D == 2:
        return
    v, M = XM.omega_mag(C)
    check("omega_mag", metric("omega_mag", u, Ng)[ins], v[ins], M[ins], T)
    z, c = (0.3, -0.5, 0.8), (2.3, 3.1, 1.7)
    v, M, n = XM.omega_theta(C, z, c)
    assert np.all(n[ins] > 0.05)                                     # no cell near the axis: far from the n <= eps(n) branch
    check("omega_theta", metric("omega_theta", u, Ng, par=z, par2=c)[ins], v[ins], M[ins], T)
    v, M = XM.lambda2(C)
    check("lambda2", metric("lambda2", u, Ng)[ins], v[ins], M[ins], T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", SPECIAL)
def test_lambda2_and_vorticity_on_special_fields_oracle_vs_xref(T, name):
    """The paths a random field never takes.  uniform: J ≡ 0, so λ₂, |ω|, ω_θ and curl are exactly 0.  diagonal: S²+Ω² is
    diagonal and λ₂ is the middle of its diagonal.  Solid rotation about a tilted axis and a tilted simple shear, clean and
    with noise of 2^-30: two (three) eigenvalues of S²+Ω² coincide.  The trigonometric closed form that the oracle and the
    kernel used before kept half the digits of Float64 there: ratios of 2.09e6 (rotation) and 6.53e5 (rotation-noise)
    eps*M against K = 16 on this grid; with Jacobi sweeps 0.095 and 0.029.  On the shear fields S²+Ω² vanishes up to rounding
    and both forms stay within the bound: 0.142 (shear) and 0.107 (shear-noise), before and after."""
    Ng = (9, 8, 7)
    u = XM.special_fields(Ng, T, 5)[name]
    C = X.host_cells({"u": u}, N=Ng)
    ins = inside(C, Ng)
    l2 = metric("lambda2", u, Ng)[ins]
    v, M = XM.lambda2(C)
    check("lambda2", l2, v[ins], M[ins], T, control=False)
    om = metric("omega_mag", u, Ng)[ins]
    vo, Mo = XM.omega_mag(C)
    check("omega_mag", om, vo[ins], Mo[ins], T, control=False)
    if name == "uniform":
        assert not l2.any() and not om.any()
        for i in range(3):
            assert not metric("curl", u, Ng, i=i)[ins].any()
        assert not metric("omega_theta", u, Ng, par=(0.3, -0.5, 0.8), par2=(2.3, 3.1, 1.7))[ins].any()
    if name == "diagonal":
        J = np.stack([XM.dudx(C, a, a)[0][ins] for a in range(3)])
        assert np.all(M[ins] > 0) and X.worst(l2, np.sort(J * J, axis=0)[1], M[ins], T) <= K["lambda2"]
    if name == "rotation":                                          # control: the rate 0.7 off by 64 K eps; and λ₂ = -|0.7 a|²
        u2 = XM.special_fields(Ng, T, 5, scale=1 + 64 * K["lambda2"] * X.eps(T))[name]
        v2, M2 = XM.lambda2(X.host_cells({"u": u2}, N=Ng))
        assert X.worst(l2, v2[ins], M2[ins], T) > K["lambda2"]
        assert np.allclose(l2, -0.49, rtol=1e-4)


@pytest.mark.parametrize("T", TYPES)
def test_omega_theta_on_the_axis_oracle_vs_xref(T):
    """ω_θ about z = e_z through (2.5, 3.5, .): the cells (3, 4, k) lie exactly on the axis, where n = 0 and the result is
    0 (Metrics.jl:76); every other cell is at least half a cell away from it"""
    Ng = (7, 8, 6)
    u = field(Ng + (3,), T, "random", 31)
    C = X.host_cells({"u": u}, N=Ng)
    ins = inside(C, Ng)
    z, c = (0.0, 0.0, 1.0), (2.5, 3.5, 1.0)
    v, M, n = XM.omega_theta(C, z, c)
    on = (C.idx[0] == 3) & (C.idx[1] == 4)
    assert np.array_equal(n == 0, on) and np.all(n[~on] >= 1)
    got = metric("omega_theta", u, Ng, par=z, par2=c)
    assert not got[on & ins].any() and (on & ins).sum() == Ng[2] - 2
    check("omega_theta", got[ins], v[ins], M[ins], T)


# ------------------------------------------------------------------------------------------------ band sums

def band_check(name, got, v, M, n, T, tag="oracle"):
    r = XM.band_ratio(name, got, v, M, n, T)
    key = f"{name} {np.dtype(T).name}"
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1, f"{key} n={n}: |{tag}-ref| = {r:.3g} of its bound"


BAND_GRIDS = [(11, 9, 7), (69, 8, 6), (132, 7), (13, 11)]
# the oracle scatters its terms into the field df like the reference, one per cell: no cell twice in its bands
BAND_CASES = sorted({(Ng, min(n, int(np.prod([m - 2 for m in Ng])))) for Ng in BAND_GRIDS for n in (0, 1, 255, 256, 257, 3000)})


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng,nband", BAND_CASES)
def test_band_sums_oracle_vs_xref(T, Ng, nband):
    """pressure_force (K = 1), viscous_force (K = 4), pressure_moment (K = 4) over synthetic bands on non-cubic grids.
    Controls: ν off by 64 K eps (on the band of one cell); on the bands of 99 to 257 cells x₀ with two components
    swapped and the list shifted by one against nds must fail."""
    D = len(Ng)
    idx, nds = synthetic_band(Ng, nband, 40 + nband)
    p, u = field(Ng, T, "random", 41), field(Ng + (D,), T, "random", 42)
    nu = float(np.dtype(T).type(0.37))
    x0 = X0[:D]
    df = O.zeros(Ng + (D,), T)
    fp = O.pressure_force_band(p, df, idx, nds)
    fv = O.viscous_force_band(u, nu, df, idx, nds)
    mp = O.pressure_moment_band(x0, p, df, idx, nds)
    band_check("pforce", fp, *XM.pressure_force(p, idx, nds), nband, T)
    band_check("vforce", fv, *XM.viscous_force(u, nu, idx, nds), nband, T)
    band_check("pmoment", mp, *XM.pressure_moment(p, x0, idx, nds), nband, T)
    if nband == 0:
        assert not fp.any() and not fv.any() and not mp.any()
    if D == 2:
        assert mp[0] == mp[1]
    if nband == 1:                                                  # (one term: no cancellation hides the factor)
        assert XM.band_ratio("vforce", fv, *XM.viscous_force(u, nu * (1 + 64 * K["vforce"] * X.eps(T)), idx, nds), nband, T) > 1
    if 99 <= nband <= 257:
        sh = np.roll(idx, 1)
        assert XM.band_ratio("pforce", fp, *XM.pressure_force(p, sh, nds), nband, T) > 1
        assert XM.band_ratio("vforce", fv, *XM.viscous_force(u, nu, sh, nds), nband, T) > 1
        assert XM.band_ratio("pmoment", mp, *XM.pressure_moment(p, x0, sh, nds), nband, T) > 1
        xs = (x0[1], x0[0]) + tuple(x0[2:])
        assert XM.band_ratio("pmoment", mp, *XM.pressure_moment(p, xs, idx, nds), nband, T) > 1


def test_worst_ratios_are_recorded():
    """(prints the largest |oracle-ref|/(eps*M) per metric and, for the band sums, the largest share of their bound: -s)"""
    print("\nworst oracle vs xref_metrics:", {k: round(v, 3) for k, v in sorted(WORST.items())})
