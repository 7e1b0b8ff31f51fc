"""The HIP kernels against the independent extended-precision reference tests/xref.py at small adversarial shapes:
|hip - ref| <= K * eps_T * M per cell with the K of test_xref_cpu.py (xref.py explains M).  The shapes sit on the
dispatch edges: interior x extents V-1, V, V+1, 63V, 64V, 65V (V = 4 Float32, 2 Float64: stencil7_ok and the x tile
seams), odd and even y extents across S7_BY*R and the conv_diff! 64x4 tile, z extents 1, 2, 3, 5, 6 (conv_diff_tiled's
n >= 5 and the split launch of three planes or fewer); padded and dense layouts.  Reductions: dot within 1 ulp (Float32) /
4 log2(n) eps sum|ab| (Float64) of the exact value, L∞ exact with its unique maximum in a ghost cell, in the last cell of
the last plane, negative."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xref as X
from waterlily_amd import sim as S
from xref_inputs import coefficients, field

TYPES = [np.float32, np.float64]
K = X.K
WORST = {}


def V(T):
    return 4 if np.dtype(T) == np.float32 else 2


def shapes3(T):
    v = V(T)
    return [(v - 1, 5, 1), (v, 4, 2), (v + 1, 9, 3), (63 * v, 8, 5), (64 * v, 3, 6), (65 * v, 5, 5)]


def dev(h, D, padded):
    lay = S.Layout(h.shape[:D], h.dtype, padded)
    a = lay.alloc(h.shape[D:], "cuda:0")
    span = 1 + sum((n - 1) * s for n, s in zip(a.shape, a.stride()))
    torch.as_strided(a, (span + lay.align,), (1,), a.storage_offset() - lay.lead).fill_(1e30)   # padding poisoned
    S.upload(a, h)
    return a


def check(name, key, got, v, M, T, control=True):
    """the comparison, and its control: the same values against the reference of the NEXT sample must fail"""
    w = X.worst(got, v, M, T)
    WORST[key] = max(WORST.get(key, 0.0), w)
    assert w <= K[name], f"{key}: |hip-ref| = {w:.3g} eps*M > K = {K[name]}"
    assert not control or X.worst(got[:-1], v[1:], M[1:], T) > K[name], f"{key}: control (samples shifted by one) did not fail"


def fails(name, got, v, M, T):
    return X.worst(got, v, M, T) > K[name]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_conv_diff_hip_vs_xref(T, padded):
    """conv_diff! (K = 8) on every edge shape, 2-D and 3-D, random / tie-rich / step fronts on the 64-cell seams /
    2^±20 (2^±60) scaled fields, walls and periodic x; control: nu off by 64K eps and samples shifted one plane fail."""
    v = V(T)
    tn = np.dtype(T).name
    cases = [(n + 2 for n in s) for s in shapes3(T)] + [(v + 3, 11), (64 * v + 2, 7)]
    nu = float(np.dtype(T).type(0.3))
    for q, Ng in enumerate(cases):
        Ng = tuple(Ng)
        D = len(Ng)
        for kind in ("random", "ties", "step", "scaled-up", "scaled-down"):
            for perdir in ((), (0,)) if kind == "random" else ((),):
                u = field(Ng + (D,), T, kind, 100 + q, seam=64)
                ud, rd = dev(u, D, padded), dev(field(Ng + (D,), T, "random", 7), D, padded)
                S.conv_diff(rd, ud, nu=nu, perdir=perdir)
                r = S.to_host(rd)
                C = X.host_cells({"u": u}, N=Ng)
                for c in range(D):
                    got = r[..., c].ravel(order="F")
                    val, M = X.conv_diff(C, c, nu, perdir)
                    check("conv_diff", f"conv_diff {tn}", got, val, M, T)
                    if kind == "random" and not perdir:
                        assert fails("conv_diff", got, *X.conv_diff(C, c, nu * (1 + 64 * K["conv_diff"] * X.eps(T)), perdir), T)
                        if Ng[-1] > 3:
                            sh = X.host_cells({"u": u}, idx=tuple(a + (d == D - 1) for d, a in enumerate(C.idx)), N=Ng)
                            m = C.idx[D - 1] < Ng[-1] - 1
                            vs, Ms = X.conv_diff(sh, c, nu, perdir)
                            assert fails("conv_diff", got[m], vs[m], Ms[m], T)


@pytest.mark.parametrize("T", TYPES)
def test_flow_pointwise_hip_vs_xref(T):
    """div (K = 4), flux_out (K = 4), BDIM! (f: K = 4, u: K = 8) on the edge shapes; control: dt off by 64K eps fails"""
    tn = np.dtype(T).name
    for q, s in enumerate(shapes3(T)[1:]):
        Ng = tuple(n + 2 for n in s)
        D = 3
        a = S.Flow(s, (1.0, 0.0, 0.0), T=T, nu=0.01)
        h = {}
        for p, k in enumerate(("u", "u0", "f", "V", "mu0", "mu1")):
            h[k] = field(tuple(getattr(a, k).shape), T, "ties" if q % 2 else "random", 200 + 10 * q + p)
            S.upload(getattr(a, k), h[k])
        C = X.host_cells(h, N=Ng)
        ins = np.all([(x >= 1) & (x <= n - 2) for x, n in zip(C.idx, Ng)], axis=0)
        z = S.like(a.p)
        S.divergence(z, a.u)
        val, M = X.div(C)
        check("div", f"div {tn}", S.to_host(z).ravel(order="F")[ins], val[ins], M[ins], T)
        a.sigma.zero_()
        dt = S.CFL(a)
        val, M = X.flux_out(C)
        check("flux_out", f"flux_out {tn}", S.to_host(a.sigma).ravel(order="F")[ins], val[ins], M[ins], T)
        smax = float(np.max(np.asarray(val[ins], np.float64)))
        assert abs(dt - min(10.0, 1 / (smax + 5 * 0.01))) <= 8 * X.eps(T) * dt
        r = S.copy_of(a.f)
        S.accelerate(r, (0.3, -0.2, 0.1))
        rh = S.to_host(r)
        Ca = X.host_cells({"r": h["f"]}, N=Ng)
        for c, g in enumerate((0.3, -0.2, 0.1)):
            check("accelerate", f"accelerate {tn}", rh[..., c].ravel(order="F"), *X.accelerate(Ca, c, g), T)
        del r
        dtb = a.dt[-1]
        S.BDIM(a)
        f, u = S.to_host(a.f), S.to_host(a.u)
        for c in range(D):
            val, M = X.bdim_f(C, c, dtb)
            check("bdim_f", f"bdim_f {tn}", f[..., c].ravel(order="F"), val, M, T)
            val, M = X.bdim_u(C, c, dtb)
            got = u[..., c].ravel(order="F")[ins]
            check("bdim_u", f"bdim_u {tn}", got, val[ins], M[ins], T)
            assert fails("bdim_u", got, *[w[ins] for w in X.bdim_u(C, c, dtb * (1 + 64 * K["bdim_u"] * X.eps(T)))], T)
        S.scale_u(a, 0.5)
        us = S.to_host(a.u)
        Cu = X.host_cells({"u": u}, N=Ng)
        for c in range(D):
            val, M = X.scale_u(Cu, c, 0.5)
            check("scale_u", f"scale_u {tn}", us[..., c].ravel(order="F")[ins], val[ins], M[ins], T)


def poisson_cases(T):
    v = V(T)
    out = [(s, "body", None) for s in shapes3(T)[1:]] + [((7, 6), "body", None)]
    for edge in ("f1", "f2", "seam", "n-2", "n-1", "y", "z"):
        out.append(((65 * v, 5, 4), "row", edge))
    return out


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_poisson_operators_hip_vs_xref(T, padded):
    """set_diag! (D: K = 4, iD: K = 8, exactly 0 on the solid cells), mult (K = 4), residual! (K = 8), Jacobi!+increment!
    (K = 8) with bodies and with rows uniform except one coefficient at each edge of k_lrow's row-constant detection"""
    tn = np.dtype(T).name
    v = V(T)
    for q, (s, Lk, edge) in enumerate(poisson_cases(T)):
        Ng = tuple(n + 2 for n in s)
        D = len(Ng)
        L = coefficients(Ng, T, 300 + q, Lk, edge, seam=64 * v)
        x, z = field(Ng, T, "random", 310 + q), field(Ng, T, "random", 320 + q)
        ph = S.Poisson(dev(x, D, padded), dev(L, D, padded), dev(z, D, padded))
        Dh, iDh = S.to_host(ph.D), S.to_host(ph.iD)
        C = X.host_cells({"L": L, "D": Dh, "iD": iDh, "x": x, "z": z}, N=Ng)
        ins = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C.idx, Ng)], axis=0)
        Dv, DM = X.diag(C)
        check("diag", f"diag {tn}", Dh.ravel(order="F")[ins], Dv[ins], DM[ins], T)
        iv, iM = X.inv_diag(Dv, DM, T)
        check("iD", f"iD {tn}", iDh.ravel(order="F")[ins], iv[ins], iM[ins], T)
        xr = field(Ng, T, "random", 330 + q)
        zz = S.to_host(S.mult(ph, dev(xr, D, padded))).ravel(order="F")
        val, M = X.mult(X.host_cells({"L": L, "D": Dh, "x": xr}, N=Ng))
        check("mult", f"mult {tn}", zz[ins], val[ins], M[ins], T)
        assert np.all(zz[~ins] == 0)
        Cm = X.host_cells({"L": L, "D": Dh, "x": xr}, N=Ng)       # control: one x-face coefficient off by 64K eps where
        Mf = np.asarray(M, np.float64)                              # it weighs most in M
        xm = np.roll(xr, 1, axis=0).ravel(order="F").astype(np.float64)
        w = np.where(ins & (Cm.idx[0] >= 2) & (Mf > 0), np.abs(xm * L[..., 0].ravel(order="F")) / np.where(Mf > 0, Mf, 1), 0)
        I = tuple(int(a[int(np.argmax(w))]) for a in Cm.idx)
        Lp = L.copy(order="F")
        Lp[I + (0,)] *= 1 + 64 * K["mult"] * X.eps(T)
        assert fails("mult", zz[ins], *[w[ins] for w in X.mult(X.host_cells({"L": Lp, "D": Dh, "x": xr}, N=Ng))], T)
        if Lk == "row":
            nu_, nr_ = S.uniform_rows(ph, 0)
            assert 0 < nu_ < nr_                                     # the row-constant path ran, and not for the odd row
        S.upload(ph.z, z)
        S.residual(ph)
        rv, rM = X.residual_local(C)
        n_in = int(ins.sum())
        sv = sum(float(w) for w in rv[ins]) / n_in
        if abs(sv) > 4 * X.eps(T):
            rv, rM = rv - X.LD(sv), rM + X.LD(sum(float(w) for w in rM[ins]) / n_in)
        r0 = S.to_host(ph.r)
        check("residual", f"residual {tn}", r0.ravel(order="F")[ins], rv[ins], rM[ins], T)
        S.Jacobi(ph)
        (ev, eM), (rv, rM), (xv, xM) = X.jacobi_increment(X.host_cells({"L": L, "D": Dh, "iD": iDh, "r": r0, "x": x}, N=Ng))
        for nm, (vv, MM) in (("eps", (ev, eM)), ("r", (rv, rM)), ("x", (xv, xM))):
            check("jacobi", f"jacobi {tn}", S.to_host(getattr(ph, nm)).ravel(order="F")[ins], vv[ins], MM[ins], T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_pcg_one_iteration_hip_vs_xref(T, padded):
    """pcg!(it=1) from x = 0: alpha (read back as x1/eps, K = 16), x1 and r1 (K = 16); the exits of Poisson.jl:127 (r = 0)
    and :132 (|alpha| > 100) leave x and r alone"""
    tn = np.dtype(T).name
    for q, s in enumerate(shapes3(T)[1:]):
        Ng = tuple(n + 2 for n in s)
        D = 3
        L = coefficients(Ng, T, 400 + q)
        r = field(Ng, T, "random", 410 + q)
        for d in range(D):
            ix = [slice(None)] * D
            ix[d] = [0, Ng[d] - 1]
            r[tuple(ix)] = 0
        zero = np.zeros(Ng, T, order="F")
        ph = S.Poisson(dev(zero, D, padded), dev(L, D, padded), dev(zero, D, padded))
        Dh, iDh = S.to_host(ph.D), S.to_host(ph.iD)
        S.upload(ph.r, r)
        (al, Ma), _, _, x1, r1, ins = X.pcg1_ref(L, Dh, iDh, r)
        assert S.pcg(ph, it=1) == 1
        xh, eh, rh = (S.to_host(getattr(ph, k)).ravel(order="F") for k in ("x", "eps", "r"))
        sel = ins & (eh != 0)
        a_hip = xh[sel].astype(np.float64) / eh[sel]
        check("alpha", f"alpha {tn}", a_hip, np.full(sel.sum(), al), np.full(sel.sum(), Ma), T, control=False)
        assert fails("alpha", a_hip, np.full(sel.sum(), al * (1 + 64 * K["alpha"] * X.eps(T) * float(Ma / abs(al)))),
                     np.full(sel.sum(), Ma), T)
        check("pcg", f"pcg x {tn}", xh[ins], x1[0][ins], x1[1][ins], T)
        check("pcg", f"pcg r {tn}", rh[ins], r1[0][ins], r1[1][ins], T)
        # exits
        S.upload(ph.r, np.zeros(Ng, T))
        xb = S.to_host(ph.x)
        assert S.pcg(ph, it=1) == 0 and np.array_equal(S.to_host(ph.x), xb)
        r2 = np.asfortranarray(np.where(iDh != 0, Dh, 0).astype(T))
        S.upload(ph.r, r2)
        assert S.pcg(ph, it=1) == 0 and np.array_equal(S.to_host(ph.x), xb) and np.array_equal(S.to_host(ph.r), r2)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_reductions_hip_vs_xref(T, padded):
    """dot (whole arrays, padding poisoned), L2 of the inside, L₂(p) = r.r and L∞(p) = max|r| exactly, the maximum unique
    and negative in a ghost cell, then in the last cell of the last plane; control: one dropped partial fails"""
    for s in shapes3(T):
        Ng = tuple(n + 2 for n in s)
        D = 3
        n = int(np.prod(Ng))
        a, b = field(Ng, T, "random", 500), field(Ng, T, "random", 501)
        ad, bd = dev(a, D, padded), dev(b, D, padded)
        got = S.dot(ad, bd)
        v, M = X.dot(a, b)
        if np.dtype(T) == np.float32:
            assert X.ulps(got, X.round_to(v, T), T) <= 1, (got, v)
        else:
            assert abs(got - v) <= 4 * np.log2(n) * X.eps(T) * M
        q = int(np.argmax(np.abs(a.astype(np.float64) * b)))
        assert abs(got - (v - float(a.ravel()[q]) * float(b.ravel()[q]))) > 4 * np.log2(n) * X.eps(T) * M
        v2, M2 = X.L2_inside(a)
        if np.dtype(T) == np.float32:
            assert X.ulps(S.L2(ad), X.round_to(v2, T), T) <= 1
            assert X.ulps(got, X.round_to(v - float(a.ravel()[q]) * float(b.ravel()[q]), T), T) > 1   # dropped partial
        else:
            assert abs(S.L2(ad) - v2) <= 4 * np.log2(n) * X.eps(T) * M2
        L = coefficients(Ng, T, 502)
        zero = np.zeros(Ng, T, order="F")
        ph = S.Poisson(dev(zero, D, padded), dev(L, D, padded), dev(zero, D, padded))
        r = field(Ng, T, "random", 503)
        for spot in ((0, Ng[1] // 2, Ng[2] - 1), tuple(k - 1 for k in Ng), (1, 1, 1)):
            rr = r.copy(order="F")
            rr[spot] = T(-2.5)
            S.upload(ph.r, rr)
            assert S.Linf(ph) == X.Linf(rr) == 2.5, spot
        for d in range(D):                                      # L₂(p): the reference relies on outside(p.r) ≡ 0 (Poisson.jl:146)
            ix = [slice(None)] * D
            ix[d] = [0, Ng[d] - 1]
            r[tuple(ix)] = 0
        S.upload(ph.r, r)
        v, M = X.dot(r, r)
        assert X.ulps(S.L2p(ph), X.round_to(v, T), T) <= 1 if np.dtype(T) == np.float32 else \
            abs(S.L2p(ph) - v) <= 4 * np.log2(n) * X.eps(T) * M


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_multilevel_transfers_hip_vs_xref(T, padded):
    """restrict! (K = 4), restrictL! (K = 4, BC! planes included), prolongate! (exact) between a level and the next"""
    tn = np.dtype(T).name
    for q, Ng in enumerate([(10, 10), (2 * 65 * V(T) // 2 + 2, 10, 8), (10, 8, 6)]):
        D = len(Ng)
        Nc = tuple(1 + n // 2 for n in Ng)
        b = field(Ng, T, "random", 600 + q)
        a = dev(np.zeros(Nc, T, order="F"), D, padded)
        S.restrict(a, dev(b, D, padded))
        C = X.host_cells({"b": b}, N=Nc, NA=Ng)
        ins = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C.idx, Nc)], axis=0)
        val, M = X.restrict(C)
        check("restrict", f"restrict {tn}", S.to_host(a).ravel(order="F")[ins], val[ins], M[ins], T)
        L = coefficients(Ng, T, 610 + q)
        aL = dev(np.zeros(Nc + (D,), T, order="F"), D, padded)
        S.restrictL(aL, dev(L, D, padded))
        aLh = S.to_host(aL)
        CL = X.host_cells({"b": L}, N=Nc, NA=Ng)
        for c in range(D):
            check("restrictL", f"restrictL {tn}", aLh[..., c].ravel(order="F"), *X.restrictL(CL, c), T)
        cx = field(Nc, T, "random", 620 + q)
        f = dev(np.zeros(Ng, T, order="F"), D, padded)
        S.prolongate(f, dev(cx, D, padded))
        Cf = X.host_cells({"b": cx}, N=Ng, NA=Nc)
        insf = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(Cf.idx, Ng)], axis=0)
        val, M = X.prolongate(Cf)
        check("prolongate", f"prolongate {tn}", S.to_host(f).ravel(order="F")[insf], val[insf], M[insf], T)


def test_worst_ratios_are_recorded():
    """(prints the largest |hip-ref|/(eps*M) per operator seen in this module: -s shows it)"""
    print("\nworst |hip-ref|/(eps_T*M):", {k: round(v, 3) for k, v in sorted(WORST.items())})
