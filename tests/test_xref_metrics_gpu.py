"""The HIP read-outs of Metrics.jl against the independent extended-precision reference tests/xref_metrics.py, in both
types and in the padded and dense layouts (padding poisoned):
  * op_metric (ke, curl, |ω|, ω_θ, λ₂): |hip - ref| <= K * eps_T * M per cell on the dispatch-edge shapes of
    test_xref_gpu.py, on the adversarial fields and on the fields that take λ₂'s special paths;
  * k_pforce, k_vforce, k_pmoment through wl_pforce / wl_vforce / wl_pmoment on synthetic bands, decoupled from any
    geometry: |hip - ref| <= (K * eps_T + tree_adds(n) * eps_64 / 2) * M, for band lengths 0, 1, 255, 256, 257 and one past the
    launch cap, on non-cubic grids.
The references are computed once per (type, shape, input) and shared by the two layouts."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xref as X
import xref_metrics as XM
from test_xref_gpu import V, dev, shapes3
from waterlily_amd import sim as S
from xref_inputs import field

TYPES = [np.float32, np.float64]
K = XM.K
WORST = {}
KINDS, SPECIAL, X0, inside, synthetic_band = XM.KINDS, XM.SPECIAL, XM.X0, XM.inside, XM.synthetic_band
Z_OBLIQUE, C_OBLIQUE = (0.3, -0.5, 0.8), (2.3, 3.1, 1.7)
Z_AXIS, C_AXIS = (0.0, 0.0, 1.0), (0.5, 1.5, 1.0)                 # the cells (1, 2, k) lie on this axis


def check(name, got, v, M, T, control=True):
    w = X.worst(got, v, M, T)
    key = f"{name} {np.dtype(T).name}"
    WORST[key] = max(WORST.get(key, 0.0), w)
    assert w <= K[name], f"{key}: |hip-ref| = {w:.3g} eps*M > K = {K[name]}"
    assert not control or X.worst(got[:-1], v[1:], M[1:], T) > K[name], f"{key}: control (samples shifted by one) did not fail"


def metric_shapes(T):
    v = V(T)
    return [tuple(n + 2 for n in s) for s in shapes3(T)] + [(v + 3, 11), (64 * v + 2, 7)]


@functools.lru_cache(maxsize=None)
def metric_case(tn, Ng, kind):
    """(u, ins, {metric: (value, M)}) of one input: every metric the dimension has"""
    T = np.dtype(tn).type
    D = len(Ng)
    u = field(Ng + (D,), T, kind, 700 + len(kind)) if kind in KINDS else XM.special_fields(Ng, T, 5)[kind]
    C = X.host_cells({"u": u}, N=Ng)
    s = float(np.max(np.abs(u)))
    U = (0.25 * s, -0.5 * s, 0.125 * s)[:D]
    ref = {("ke", None): XM.ke(C), ("ke", U): XM.ke(C, U)}
    for i in (range(3) if D == 3 else (2,)):
        ref["curl", i] = XM.curl(C, i)
    if D == 3:
        ref["omega_mag", None] = XM.omega_mag(C)
        ref["lambda2", None] = XM.lambda2(C)
        ins = inside(C, Ng)
        for z, c in ((Z_OBLIQUE, C_OBLIQUE), (Z_AXIS, C_AXIS)):
            v, M, n = XM.omega_theta(C, z, c)
            on = (C.idx[0] == 1) & (C.idx[1] == 2) if z == Z_AXIS else np.zeros(len(C), bool)
            # the distance from the branch n <= eps(n): on the axis exactly, or nowhere near it (checked on the reference)
            assert np.array_equal(n == 0, on) and np.all(n[ins & ~on] > 0.05)
            ref["omega_theta", (z, c)] = (v, M)
    return u, inside(C, Ng), ref


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_field_metrics_hip_vs_xref(T, padded):
    """ke with and without U (K = 4), curl (K = 4), |ω| (K = 8), ω_θ about an oblique axis and about one that runs through
    a line of cell centres (K = 16; exactly 0 on that line), λ₂ (K = 16) on every edge shape, 2-D and 3-D, on random /
    tie-rich / 2^±20 (2^±60) scaled fields; control: the samples shifted by one cell fail"""
    tn = np.dtype(T).name
    for Ng in metric_shapes(T):
        D = len(Ng)
        for kind in KINDS:
            u, ins, ref = metric_case(tn, Ng, kind)
            ud, out = dev(u, D, padded), dev(np.zeros(Ng, T, order="F"), D, padded)
            for (name, par), (v, M) in ref.items():
                kw = {}
                if name == "ke":
                    kw = dict(par=par)
                elif name == "curl":
                    kw = dict(i=par)
                elif name == "omega_theta":
                    kw = dict(par=par[0], par2=par[1])
                got = S.to_host(S.metric(out, name, ud, **kw)).ravel(order="F")
                check(name, got[ins], v[ins], M[ins], T, control=not (kind == "ties" and name == "curl"))
                if name == "omega_theta" and par[0] == Z_AXIS:
                    C = X.host_cells({"u": u}, N=Ng)
                    on = ins & (C.idx[0] == 1) & (C.idx[1] == 2)
                    assert on.sum() == Ng[2] - 2 and not got[on].any()


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_lambda2_and_vorticity_on_special_fields_hip_vs_xref(T, padded):
    """λ₂ (K = 16) and |ω| (K = 8) on the fields of xref_metrics.special_fields, on every 3-D edge shape.  uniform flow: λ₂, |ω|,
    ω_θ and curl exactly 0; u_c(x_c): the diagonal path; solid rotation about a tilted axis and a tilted simple shear, clean
    and with noise of 2^-30: coinciding eigenvalues.  Control: the rotation rate off by 64 K eps fails."""
    tn = np.dtype(T).name
    for Ng in metric_shapes(T)[:6]:
        for name in SPECIAL:
            u, ins, ref = metric_case(tn, Ng, name)
            ud, out = dev(u, 3, padded), dev(np.zeros(Ng, T, order="F"), 3, padded)
            l2 = S.to_host(S.metric(out, "lambda2", ud)).ravel(order="F")[ins]
            v, M = ref["lambda2", None]
            check("lambda2", l2, v[ins], M[ins], T, control=False)
            om = S.to_host(S.metric(out, "omega_mag", ud)).ravel(order="F")[ins]
            v, M = ref["omega_mag", None]
            check("omega_mag", om, v[ins], M[ins], T, control=False)
            if name == "uniform":
                assert not l2.any() and not om.any()
                for i in range(3):
                    assert not S.to_host(S.metric(out, "curl", ud, i=i)).ravel(order="F")[ins].any()
                assert not S.to_host(S.metric(out, "omega_theta", ud, par=Z_OBLIQUE, par2=C_OBLIQUE)).ravel(order="F")[ins].any()
            if name == "rotation":
                u2 = XM.special_fields(Ng, T, 5, scale=1 + 64 * K["lambda2"] * X.eps(T))[name]
                v2, M2 = XM.lambda2(X.host_cells({"u": u2}, N=Ng))
                assert X.worst(l2, v2[ins], M2[ins], T) > K["lambda2"]


# ------------------------------------------------------------------------------------------------ band sums

# blocks of 256 threads: the launch cap `if (nb > 1024) nb = 1024` of wl_pforce and of band_reduce (wl_vforce, wl_pmoment),
# both in waterlily_amd/csrc/wl_api.hip; test_launch_cap_is_the_one_in_the_source holds this copy to the source
CAP = 1024
NBANDS = [0, 1, 255, 256, 257, CAP * 256 + 513]
BAND_GRIDS = [(11, 9, 7), (69, 8, 6), (132, 7), (13, 11)]         # interior (9,7,5), (67,6,4), (130,5), (11,9)


@functools.lru_cache(maxsize=None)
def band_case(tn, Ng, nband):
    T = np.dtype(tn).type
    D = len(Ng)
    idx, nds = synthetic_band(Ng, nband, 40 + nband % 1000)
    p, u = field(Ng, T, "random", 41), field(Ng + (D,), T, "random", 42)
    nu = float(T(0.37))
    x0 = X0[:D]
    ref = {"pforce": XM.pressure_force(p, idx, nds), "vforce": XM.viscous_force(u, nu, idx, nds),
           "pmoment": XM.pressure_moment(p, x0, idx, nds)}
    return idx, nds, p, u, nu, x0, ref


def hip_band_sums(T, D, pd, ud, bi, bn, nu, x0):
    L = S._lib.lib()
    vp = lambda t: S.C.c_void_p(t.data_ptr())
    out = (S.C.c_double * 3)()
    res = {}
    S.check(L.wl_pforce(S._WLT[np.dtype(T)], S.C.byref(S._grid_of(pd, D)), S._ptr(pd), vp(bi), vp(bn), bi.numel(), out))
    res["pforce"] = np.array(out[:D])
    S.check(L.wl_vforce(S._WLT[np.dtype(T)], S.C.byref(S._grid_of(ud, D)), S._ptr(ud), vp(bi), vp(bn), bi.numel(), nu, out))
    res["vforce"] = np.array(out[:D])
    S.check(L.wl_pmoment(S._WLT[np.dtype(T)], S.C.byref(S._grid_of(pd, D)), S._ptr(pd), vp(bi), vp(bn), bi.numel(), S.d3(x0), out))
    res["pmoment"] = np.array(out[:D])
    return res


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("Ng", BAND_GRIDS)
def test_band_sums_hip_vs_xref(T, padded, Ng):
    """wl_pforce (K = 1), wl_vforce (K = 4), wl_pmoment (K = 4) on synthetic bands: cells drawn from the inside of a
    non-cubic grid, those next to every ghost layer first, nds uniform in [-1, 1], x₀ asymmetric and off the half-integers.
    Band lengths 0 (no launch: zeros), 1, 255, 256, 257 (partial last blocks) and cap*256 + 513 (the grid-stride loop).
    Controls: ν off by 64 K eps (band of one cell), x₀ with two components swapped and the list shifted by one against nds
    (bands of 255 to 257 cells) fail."""
    tn = np.dtype(T).name
    D = len(Ng)
    for nband in NBANDS:
        idx, nds, p, u, nu, x0, ref = band_case(tn, Ng, nband)
        pd, ud = dev(p, D, padded), dev(u, D, padded)
        bi, bn = S.band_to_device(pd, idx, nds)
        got = hip_band_sums(T, D, pd, ud, bi, bn, nu, x0)
        for name in ("pforce", "vforce", "pmoment"):
            v, M = ref[name]
            r = XM.band_ratio(name, got[name], v, M, nband, T, adds=XM.tree_adds(nband, CAP))
            WORST[f"{name} {tn}"] = max(WORST.get(f"{name} {tn}", 0.0), r)
            assert r <= 1, f"{name} {tn} {Ng} n={nband}: |hip-ref| = {r:.3g} of its bound"
        if nband == 0:
            assert not any(got[k].any() for k in got)
        if D == 2:
            assert got["pmoment"][0] == got["pmoment"][1]
        if nband == 1:
            assert XM.band_ratio("vforce", got["vforce"], *XM.viscous_force(u, nu * (1 + 64 * K["vforce"] * X.eps(T)), idx, nds), nband, T) > 1
        if 255 <= nband <= 257:
            sh = np.roll(idx, 1)
            assert XM.band_ratio("pforce", got["pforce"], *XM.pressure_force(p, sh, nds), nband, T) > 1
            assert XM.band_ratio("vforce", got["vforce"], *XM.viscous_force(u, nu, sh, nds), nband, T) > 1
            assert XM.band_ratio("pmoment", got["pmoment"], *XM.pressure_moment(p, x0, sh, nds), nband, T) > 1
            xs = (x0[1], x0[0]) + tuple(x0[2:])
            assert XM.band_ratio("pmoment", got["pmoment"], *XM.pressure_moment(p, xs, idx, nds), nband, T) > 1


def test_launch_cap_is_the_one_in_the_source():
    """CAP above is what wl_api.hip caps the band launches at: the driver band_reduce and wl_pforce each hold the line"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(S.__file__), "csrc", "wl_api.hip")).read()
    caps = re.findall(r"if \(nb > (\d+)\) nb = (\d+);", src)
    assert len(caps) == 2 and all(a == b == str(CAP) for a, b in caps), caps


def test_worst_ratios_are_recorded():
    """(prints the largest |hip-ref|/(eps*M) per metric and, for the band sums, the largest share of their bound: -s)"""
    print("\nworst hip vs xref_metrics:", {k: round(v, 3) for k, v in sorted(WORST.items())})
