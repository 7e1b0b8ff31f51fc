"""The CPU oracle (oracle/wlo_impl.h, scatter form, rounds like the reference) against the independent extended-precision
reference tests/xref.py (gather form, no rounding), operator by operator, on the adversarial inputs of xref_inputs.py:
|oracle - ref| <= K * eps_T * M at every cell, K stated per operator (xref.py explains M).  Each comparison also carries a
negative control: the same check against a reference with one planted error must FAIL."""
import numpy as np
import pytest

import xref as X
from oracle import wl_oracle as O
from xref_inputs import (KINDS, body_block, coefficients, field, pcg_body, pcg_cases, pcg_chains, pcg_wave, periodic_subsets,
                         project_fields, step_fields)
from xref_pcg import replay

TYPES = [np.float32, np.float64]
K = X.K
WORST = {}


def check(name, got, v, M, T, key=None, control=True):
    """the comparison, and its control: the same values against the reference of the NEXT sample must fail"""
    w = X.worst(got, v, M, T)
    WORST[key or name] = max(WORST.get(key or name, 0.0), w)
    assert w <= K[name], f"{name}: |got-ref| = {w:.3g} eps*M > K = {K[name]}"
    assert not control or X.worst(got[:-1], v[1:], M[1:], T) > K[name], f"{name}: control (samples shifted by one) did not fail"
    return w


def fails(name, got, v, M, T):
    return X.worst(got, v, M, T) > K[name]


CD_CASES = [((10, 9), ()), ((10, 9), (0,)), ((7, 6, 5), ()), ((7, 6, 5), (0, 1, 2)), ((6, 5, 3), (2,)), ((5, 4, 3), ())]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng,perdir", CD_CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_conv_diff_oracle_vs_xref(T, Ng, perdir, kind):
    """conv_diff! with the ϕuL/ϕuR boundary faces and the periodic ϕuP face, nu = 0.3 (K = 8)"""
    D = len(Ng)
    u = field(Ng + (D,), T, kind, 1, seam=3)
    nu = float(np.dtype(T).type(0.3))
    r, Phi = O.zeros(Ng + (D,), T), O.zeros(Ng, T)
    O.conv_diff(r, u, Phi, nu=nu, perdir=perdir)
    C = X.host_cells({"u": u}, N=Ng)
    for c in range(D):
        v, M = X.conv_diff(C, c, nu, perdir)
        got = r[..., c].ravel(order="F")
        check("conv_diff", got, v, M, T, f"conv_diff {np.dtype(T).name}")
        if kind == "random":                                   # negative controls
            assert fails("conv_diff", got, *X.conv_diff(C, c, nu * (1 + 64 * K["conv_diff"] * X.eps(T)), perdir), T)
            sh = X.host_cells({"u": u}, idx=tuple(a + (q == D - 1) for q, a in enumerate(C.idx)), N=Ng)
            in_ = C.idx[D - 1] < Ng[D - 1] - 1
            vs, Ms = X.conv_diff(sh, c, nu, perdir)
            assert fails("conv_diff", got[in_], vs[in_], Ms[in_], T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(10, 9), (7, 6, 5)])
@pytest.mark.parametrize("kind", KINDS)
def test_flow_pointwise_operators_oracle_vs_xref(T, Ng, kind):
    """div (K = 4), BDIM! (f: K = 4, u: K = 8), flux_out (K = 4)"""
    D = len(Ng)
    a = O.Flow(tuple(n - 2 for n in Ng), (1.0,) + (0.0,) * (D - 1), T=T, nu=0.01)
    for q, k in enumerate(("u", "u0", "f", "V", "mu0", "mu1")):
        getattr(a, k)[...] = field(getattr(a, k).shape, T, kind, 10 + q)
    h = {k: getattr(a, k).copy(order="F") for k in ("u", "u0", "f", "V", "mu0", "mu1")}
    C = X.host_cells(h, N=Ng)
    ins = np.all([(x >= 1) & (x <= n - 2) for x, n in zip(C.idx, Ng)], axis=0)
    z = O.zeros(Ng, T)
    O._fn("wlo_div", T)(O._p(z), O._p(a.u), O.C.byref(a.grid))
    v, M = X.div(C)
    check("div", z.ravel(order="F")[ins], v[ins], M[ins], T, f"div {np.dtype(T).name}")
    a.sigma[...] = 0
    O.CFL(a)
    v, M = X.flux_out(C)
    check("flux_out", a.sigma.ravel(order="F")[ins], v[ins], M[ins], T, f"flux_out {np.dtype(T).name}")
    dt = a.dt[-1]
    O.BDIM(a)
    for c in range(D):
        v, M = X.bdim_f(C, c, dt)
        check("bdim_f", a.f[..., c].ravel(order="F"), v, M, T, f"bdim_f {np.dtype(T).name}")
        v, M = X.bdim_u(C, c, dt)
        got = a.u[..., c].ravel(order="F")
        check("bdim_u", got[ins], v[ins], M[ins], T, f"bdim_u {np.dtype(T).name}")
        if kind == "random":
            assert fails("bdim_u", got[ins], *[q[ins] for q in X.bdim_u(C, c, dt * (1 + 64 * K["bdim_u"] * X.eps(T)))], T)


def poisson(Ng, T, seed, Lkind="body", edge=None, rkind="random"):
    D = len(Ng)
    L = coefficients(Ng, T, seed, Lkind, edge, seam=3)
    x = field(Ng, T, rkind, seed + 1)
    z = field(Ng, T, rkind, seed + 2)
    return O.Poisson(x.copy(order="F"), L.copy(order="F"), z.copy(order="F")), L, x, z


P_SHAPES = [(10, 9), (9, 8, 7), (6, 5, 3)]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", P_SHAPES)
@pytest.mark.parametrize("Lkind,edge", [("body", None), ("row", "f1"), ("row", "n-1"), ("row", "y")])
def test_poisson_operators_oracle_vs_xref(T, Ng, Lkind, edge):
    """set_diag! (D: K = 4, iD: K = 8, iD == 0 exactly on the solid cells), mult (K = 4), residual! (K = 8 after the
    mean shift), Jacobi!+increment! (K = 8)"""
    p, L, x, z = poisson(Ng, T, 3, Lkind, edge)
    tn = np.dtype(T).name
    C = X.host_cells({"L": L, "D": p.D, "iD": p.iD, "x": x, "z": z}, N=Ng)
    ins = np.all([(q >= 1) & (q <= n - 2) for q, n in zip(C.idx, Ng)], axis=0)
    Dv, DM = X.diag(C)
    check("diag", p.D.ravel(order="F")[ins], Dv[ins], DM[ins], T, f"diag {tn}")
    iv, iM = X.inv_diag(Dv, DM, T)
    check("iD", p.iD.ravel(order="F")[ins], iv[ins], iM[ins], T, f"iD {tn}")
    if Lkind == "body":
        assert np.any(p.iD[O.inside(p.iD)] == 0)
    # mult: z = A x (ghosts 0)
    xr = field(Ng, T, "random", 30)
    Cx = X.host_cells({"L": L, "D": p.D, "x": xr}, N=Ng)
    zz = O.mult(p, xr.copy(order="F")).ravel(order="F")
    v, M = X.mult(Cx)
    check("mult", zz[ins], v[ins], M[ins], T, f"mult {tn}")
    assert np.all(zz[~ins] == 0)
    Lp = L.copy(order="F")                                      # control: one face coefficient off by 64K eps, at the
    xm = np.roll(xr, 1, axis=0).ravel(order="F").astype(np.float64)     # cell where that face weighs most in M
    Mf = np.asarray(M, np.float64)
    w = np.where(ins & (C.idx[0] >= 2) & (Mf > 0), np.abs(xm * L[..., 0].ravel(order="F")) / np.where(Mf > 0, Mf, 1), 0)
    q = int(np.argmax(w))
    I = tuple(int(a[q]) for a in C.idx)
    Lp[I + (0,)] *= 1 + 64 * K["mult"] * X.eps(T)
    Cp = X.host_cells({"L": Lp, "D": p.D, "x": xr}, N=Ng)
    assert fails("mult", zz[ins], *[q[ins] for q in X.mult(Cp)], T)
    # residual!
    p.z[...] = z
    O.residual(p)
    rv, rM = X.residual_local(C)
    n_in = int(np.prod([n - 2 for n in Ng]))
    s = sum(float(q) for q in rv[ins]) / n_in
    sM = sum(float(q) for q in rM[ins]) / n_in
    if abs(s) > 4 * X.eps(T):
        rv, rM = rv - X.LD(s), rM + X.LD(sM)
    check("residual", p.r.ravel(order="F")[ins], rv[ins], rM[ins], T, f"residual {tn}")
    # Jacobi! + increment!
    r0, x0 = p.r.copy(order="F"), x.copy(order="F")
    Cj = X.host_cells({"L": L, "D": p.D, "iD": p.iD, "r": r0, "x": x0}, N=Ng)
    O.Jacobi(p)
    (ev, eM), (rv, rM), (xv, xM) = X.jacobi_increment(Cj)
    check("jacobi", p.eps.ravel(order="F")[ins], ev[ins], eM[ins], T, f"jacobi {tn}")
    check("jacobi", p.r.ravel(order="F")[ins], rv[ins], rM[ins], T, f"jacobi {tn}")
    check("jacobi", p.x.ravel(order="F")[ins], xv[ins], xM[ins], T, f"jacobi {tn}")


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", P_SHAPES)
def test_pcg_one_iteration_and_exits_oracle_vs_xref(T, Ng):
    """pcg!(it=1) from x = 0: alpha read back as x1/eps (K = 16), x1 and r1 = r0 - alpha*A*eps (K = 16); the exits of
    Poisson.jl:127 (|rho| < 10eps: r = 0) and :132 (|alpha| > 100: eps in the near-null space of A) change nothing."""
    p, L, x, z = poisson(Ng, T, 5)
    r = field(Ng, T, "random", 8)
    r[tuple(np.setdiff1d(np.arange(n), np.arange(1, n - 1)) for n in Ng[:1]) + (slice(None),) * (len(Ng) - 1)] = 0
    r = np.asfortranarray(r)
    for d in range(len(Ng)):                                    # ghost cells of r are 0 (outside(p.r) ≡ 0, Poisson.jl:146)
        idx = [slice(None)] * len(Ng)
        idx[d] = [0, Ng[d] - 1]
        r[tuple(idx)] = 0
    p.x[...] = 0
    p.r[...] = r
    p.eps[...] = 0
    (al, Ma), _, _, x1, r1, ins = X.pcg1_ref(L, p.D.copy(order="F"), p.iD.copy(order="F"), r)
    assert O.pcg(p, it=1) == 1
    tn = np.dtype(T).name
    e = p.eps.ravel(order="F")
    sel = ins & (np.abs(e) > 0)
    check("alpha", p.x.ravel(order="F")[sel] / e[sel].astype(np.float64), np.full(sel.sum(), al), np.full(sel.sum(), Ma), T,
          f"alpha {tn}", control=False)          # (a scalar: its control is the planted error below)
    check("pcg", p.x.ravel(order="F")[ins], x1[0][ins], x1[1][ins], T, f"pcg x {tn}")
    check("pcg", p.r.ravel(order="F")[ins], r1[0][ins], r1[1][ins], T, f"pcg r {tn}")
    assert fails("alpha", p.x.ravel(order="F")[sel] / e[sel].astype(np.float64),
                 np.full(sel.sum(), al * (1 + 64 * K["alpha"] * X.eps(T) * float(Ma / abs(al)))), np.full(sel.sum(), Ma), T)
    # exit :127 -- r = 0
    p.x[...] = x
    p.r[...] = 0
    assert O.pcg(p, it=1) == 0 and np.array_equal(p.x, x)
    # exit :132 -- r = c*D: eps = r*iD is constant up to rounding, A eps ~ 0, alpha huge
    r2 = np.where(p.iD != 0, p.D, 0).astype(T)
    p.r[...] = r2
    p.x[...] = x
    (al2, _), *_ = X.pcg1_ref(L, p.D.copy(order="F"), p.iD.copy(order="F"), np.asfortranarray(r2))
    assert abs(al2) > 1e2
    assert O.pcg(p, it=1) == 0 and np.array_equal(p.x, x) and np.array_equal(p.r, r2)


def oracle_replay(inp, T, key, kmax=6):
    """xref_pcg.replay on the CPU oracle: every run starts from inp's x0, r0 and z (eps zeroed: its ghost cells too)"""
    p = O.Poisson(inp["x0"].copy(order="F"), inp["L"].copy(order="F"), inp["z"].copy(order="F"), perdir=inp["perdir"])

    def run(k):
        p.x[...], p.r[...], p.z[...], p.eps[...] = inp["x0"], inp["r0"], inp["z"], 0
        n = O.pcg(p, it=k)
        return n, p.x.copy(order="F"), p.r.copy(order="F"), p.eps.copy(order="F")
    return replay(run, inp, p.D.copy(order="F"), p.iD.copy(order="F"), T, kmax, WORST, key)


PCG_BODY = [((10, 9), "body", None, ()), ((9, 8, 7), "body", None, ()), ((6, 5, 3), "body", None, ()),
            ((12, 7, 6), "row", "f1", ()), ((12, 7, 6), "row", "y", ()),
            ((10, 7, 6), "body", None, (0,)), ((10, 7, 6), "body", None, (1, 2)), ((10, 7, 6), "body", None, (0, 1, 2)),
            ((14, 9), "body", None, (1,))]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng,Lkind,edge,perdir", PCG_BODY)
def test_pcg_every_iteration_oracle_vs_xref(T, Ng, Lkind, edge, perdir):
    """pcg!(it=k), k = 1..6, from a random x0 with bodies, row cases and periodic directions (z uploaded with ghost values of
    order 1: the shell term of z.eps): eps_k (K = 8), x_k and r_k (K = 16) of every iteration against the replay of that
    iteration alone, n, the controls of xref_pcg.replay; no exit on these inputs"""
    out = oracle_replay(pcg_body(Ng, T, 40, Lkind, edge, seam=3, perdir=perdir), T, f"pcg6 {np.dtype(T).name} ")
    assert out["exit"] is None and out["n"] == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng,axis", [((10, 8, 5), 1), ((6, 5, 9), 2), ((9, 11), 1)])
def test_pcg_chains_leave_after_two_updates_oracle_vs_xref(T, Ng, axis):
    """the `chains` inputs: two updates, then :138 in iteration 2 for every it >= 2; x keeps the second update"""
    out = oracle_replay(pcg_chains(Ng, T, 41, axis), T, f"pcg6 {np.dtype(T).name} ")
    assert out["exit"] == (":138", 2) and out["n"] == [1, 2, 2, 2, 2, 2]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(34, 6, 5), (66, 4, 3), (34, 5)])
def test_pcg_wave_leaves_at_alpha_oracle_vs_xref(T, Ng):
    """the `wave` inputs: one update, then :132 (alpha_2 about 156) in iteration 2 for every it >= 2; eps is the new direction"""
    out = oracle_replay(pcg_wave(Ng, T), T, f"pcg6 {np.dtype(T).name} ")
    assert out["exit"] == (":132", 2) and out["n"] == [1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("q", [q for q, c in enumerate(pcg_cases(np.float32)) if c["group"] != "tall"])
def test_pcg_kernel_cases_oracle_vs_xref(q):
    """the inputs the kernels are held to (xref_inputs.pcg_cases: the dispatch-edge shapes) through the oracle: the same
    checks, and with them the branch margins and the exits of every case, on a machine without a GPU.  Float32 only, and
    without the 4096-row planes: the oracle's dot is ONE sequential double sum, and in Float64 that sum's own rounding
    grows with the number of cells (eps_k: 6.5 eps*M at 1100 cells, 8.4 at 5544), which K["pcg_eps"] does not count --
    the kernels sum in a tree; test_pcg_every_iteration_oracle_vs_xref holds the Float64 oracle at the small sizes."""
    T = np.float32
    case = pcg_cases(T)[q]
    out = oracle_replay(case["make"](), T, f"pcg6 {np.dtype(T).name} ")
    want = {"chains": ((":138", 2), [1, 2, 2, 2, 2, 2]), "wave": ((":132", 2), [1] * 6)}.get(case["group"], (None, [1, 2, 3, 4, 5, 6]))
    assert (out["exit"], out["n"]) == want


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(10, 10), (10, 8, 6)])
def test_multilevel_transfers_oracle_vs_xref(T, Ng):
    """restrict! (K = 4), restrictL! (K = 4, BC! planes included), prolongate! (exact)"""
    D = len(Ng)
    Nc = tuple(1 + n // 2 for n in Ng)
    b = field(Ng, T, "random", 40)
    a = O.zeros(Nc, T)
    O.restrict(a, b)
    C = X.host_cells({"b": b}, N=Nc, NA=Ng)
    ins = np.all([(q >= 1) & (q <= n - 2) for q, n in zip(C.idx, Nc)], axis=0)
    v, M = X.restrict(C)
    check("restrict", a.ravel(order="F")[ins], v[ins], M[ins], T, f"restrict {np.dtype(T).name}")
    L = coefficients(Ng, T, 41)
    aL = O.zeros(Nc + (D,), T)
    O.restrictL(aL, L)
    CL = X.host_cells({"b": L}, N=Nc, NA=Ng)
    for c in range(D):
        v, M = X.restrictL(CL, c)
        check("restrictL", aL[..., c].ravel(order="F"), v, M, T, f"restrictL {np.dtype(T).name}")
    cx = field(Nc, T, "random", 42)
    f = O.zeros(Ng, T)
    O.prolongate(f, cx)
    Cf = X.host_cells({"b": cx}, N=Ng, NA=Nc)
    insf = np.all([(q >= 1) & (q <= n - 2) for q, n in zip(Cf.idx, Ng)], axis=0)
    v, M = X.prolongate(Cf)
    check("prolongate", f.ravel(order="F")[insf], v[insf], M[insf], T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng,perdir", [(Ng, p) for Ng in [(10, 10), (10, 8, 6)] for p in periodic_subsets(len(Ng))])
def test_restrictL_periodic_oracle_vs_xref(T, Ng, perdir):
    """restrictL! with periodic directions (K = 4): BC!(a, 0, false, perdir) leaves periodic copies in the ghost planes
    of those directions and the normal component's plane 2 un-zeroed, applied in BC!'s (i, j) loop order; every cell of
    the coarse array, ghost cells included.  Control: the wall-case reference must fail."""
    D = len(Ng)
    Nc = tuple(1 + n // 2 for n in Ng)
    L = field(Ng + (D,), T, "random", 43, 0.2, 1.0)            # no zeroed planes: plane 2's normal face is not 0
    aL = O.zeros(Nc + (D,), T)
    O.restrictL(aL, L, perdir=perdir)
    CL = X.host_cells({"b": L}, N=Nc, NA=Ng)
    for c in range(D):
        got = aL[..., c].ravel(order="F")
        v, M = X.restrictL(CL, c, perdir=perdir)
        check("restrictL", got, v, M, T, f"restrictL periodic {np.dtype(T).name}")
        assert fails("restrictL", got, *X.restrictL(CL, c), T)      # (ghost copies, and plane 2 of c in perdir)


def _oracle_twin_step(a, b, T):
    """mom_step! of the oracle replayed from its operators (wlo_impl.h: wlo_mom_step's sequence): returns u', the
    predictor's projected velocity, which the oracle's own step overwrites"""
    D = a.D
    U = O.BCTuple(a.U, a.dt, D)
    gp, gc = O.accel_tuple(a.g, a.U, a.dt[:-1], D), O.accel_tuple(a.g, a.U, a.dt, D)
    ins = tuple(slice(1, n - 1) for n in a.N)
    a.u0[...] = a.u
    a.u[ins] *= T(0)
    O.conv_diff(a.f, a.u0, a.sigma, nu=a.nu, perdir=a.perdir)
    if gp is not None:
        O.accelerate(a.f, gp)
    O.BDIM(a)
    O.BC(a.u, U, False, a.perdir)
    O.project(a, b)
    O.BC(a.u, U, False, a.perdir)
    up = a.u.copy(order="F")
    O.conv_diff(a.f, a.u, a.sigma, nu=a.nu, perdir=a.perdir)
    if gc is not None:
        O.accelerate(a.f, gc)
    O.BDIM(a)
    a.u[ins] *= T(0.5)
    O.BC(a.u, U, False, a.perdir)
    O.project(a, b, 0.5)
    O.BC(a.u, U, False, a.perdir)
    a.dt.append(O.CFL(a))
    return up, gc


def _oracle_step_and_twin(T, dims, perdir, dt0=0.25, p0=None):
    """One mom_step! of the oracle on step_fields (a non-uniform u, a body block with V != 0, a time-dependent body force)
    and its replay from the oracle's operators, held bit-identical: (flow, solver, u', u_start, g_corr, dt)"""
    D = len(dims)
    Ng = tuple(n + 2 for n in dims)
    g = lambda i, t: 0.05 * (i + 1) * (1 + t)
    h = step_fields(Ng, T, 70, tuple(slice(2, max(3, n // 2)) for n in Ng))
    U = (1.0,) + (0.0,) * (D - 1)
    runs = []
    for _ in range(2):
        a = O.Flow(dims, U, T=T, nu=0.05, g=g, perdir=perdir, dt=dt0)
        for k in ("u", "mu0", "mu1", "V"):
            getattr(a, k)[...] = h[k]
        if p0 is not None:
            a.p[...] = p0
        O.BC(a.u, U, False, perdir)
        O.BC(a.mu0, (0.0,) * D, False, perdir)
        O.BC(a.V, (0.0,) * D, False, perdir)
        runs.append((a, O.MultiLevelPoisson(a.p, a.mu0, a.sigma, perdir=perdir)))
    (a, b), (a2, b2) = runs
    us = a.u.copy(order="F")
    dt = a.dt[-1]
    O.mom_step(a, b)
    up, gc = _oracle_twin_step(a2, b2, T)
    for k in ("u", "f", "p"):
        assert np.array_equal(getattr(a, k), getattr(a2, k)), k
    assert b.n == b2.n and a.dt == a2.dt
    assert not np.array_equal(up, us)
    return a, b, up, us, gc, dt


STEP_CASES = [((20, 12, 8), ()), ((24, 16), ()), ((24, 16), (0,))]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims,perdir", STEP_CASES)
def test_mom_step_corrector_f_oracle_vs_xref(T, dims, perdir):
    """After one mom_step! f holds the corrector's BDIM! value u_start + dt*(conv_diff(u') + g_corr) - V (Flow.jl:164-166,
    :133), K = 12 (xref.mom_f).  u' is taken from the oracle's own operators replayed in mom_step!'s order, held
    bit-identical to the oracle's step first.  Inputs: a non-uniform u, a body block with V != 0, a time-dependent body
    force.  Controls: dt off by 64K eps, the samples shifted one plane, u_start replaced by u' must fail."""
    D = len(dims)
    Ng = tuple(n + 2 for n in dims)
    tn = np.dtype(T).name
    a, b, up, us, gc, dt = _oracle_step_and_twin(T, dims, perdir)
    C = X.host_cells({"u": up, "us": us, "V": a.V}, N=Ng)
    ins = np.all([(q >= 1) & (q <= n - 2) for q, n in zip(C.idx, Ng)], axis=0)
    for c in range(D):
        got = a.f[..., c].ravel(order="F")[ins]
        v, M = X.mom_f(C, c, a.nu, dt, gc[c], perdir)
        check("mom_f", got, v[ins], M[ins], T, f"mom_step f {tn}")
        assert fails("mom_f", got, *[q[ins] for q in X.mom_f(C, c, a.nu, dt * (1 + 64 * K["mom_f"] * X.eps(T)), gc[c], perdir)], T)
        C0 = X.host_cells({"u": up, "us": up, "V": a.V}, N=Ng)
        assert fails("mom_f", got, *[q[ins] for q in X.mom_f(C0, c, a.nu, dt, gc[c], perdir)], T)
        sh = X.host_cells({"u": up, "us": us, "V": a.V}, idx=tuple(q + (d == D - 1) for d, q in enumerate(C.idx)), N=Ng)
        m = ins & (C.idx[D - 1] < Ng[D - 1] - 2)
        vs, Ms = X.mom_f(sh, c, a.nu, dt, gc[c], perdir)
        assert fails("mom_f", a.f[..., c].ravel(order="F")[m], vs[m], Ms[m], T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims", [(32, 32, 32), (64, 32), (512, 8, 8)])
def test_vcycle_coarse_invariant_oracle_vs_xref(T, dims):
    """After Vcycle!(ml, 0) level 1 satisfies r + A x = rhs, rhs = restrict! of level 0's Jacobi! residual (xref.vcycle_rhs,
    xref.coarse_defect; K = coarse_inv) -- the invariant the GPU file holds the coarse tail to; control: one face of level
    1's L off by 25 % in the reference fails."""
    Ng = tuple(n + 2 for n in dims)
    L = coefficients(Ng, T, 5)
    z = field(Ng, T, "random", 6)
    ins = tuple(slice(1, n - 1) for n in Ng)
    z[ins] -= z[ins].mean().astype(T)
    po = O.MultiLevelPoisson(np.zeros(Ng, T, order="F"), L.copy(order="F"), z.copy(order="F"))
    O.residual(po)
    h0 = {k: getattr(po.levels[0], k).copy(order="F") for k in ("L", "D", "iD", "x", "r")}
    rhs, rhsM = X.vcycle_rhs(h0, po.levels[1].shape)
    O.Vcycle(po, 0)
    h1 = {k: getattr(po.levels[1], k).copy(order="F") for k in ("L", "D", "x", "r")}
    v, M = X.coarse_defect(h1, rhs, rhsM)
    check("coarse_inv", np.zeros(len(v)), v, M, T, f"coarse r+Ax {np.dtype(T).name}", control=False)
    h1["L"][tuple(n // 2 for n in po.levels[1].shape) + (0,)] *= T(1.25)
    assert fails("coarse_inv", np.zeros(len(v)), *X.coarse_defect(h1, rhs, rhsM), T)


@pytest.mark.parametrize("T", TYPES)
def test_reductions_oracle_vs_xref(T):
    """dot over the whole arrays: Float32 within 1 ulp of the correctly rounded exact value, Float64 within
    4*log2(n)*eps*sum|ab|; control: one partial dropped fails."""
    Ng = (11, 9, 7)
    a, b = field(Ng, T, "random", 50), field(Ng, T, "random", 51)
    got = float(O._fn("wlo_dot", T)(O._p(a), O._p(b), a.size))
    v, M = X.dot(a, b)
    n = a.size
    if np.dtype(T) == np.float32:
        assert X.ulps(got, X.round_to(v, T), T) <= 1
    else:
        assert abs(got - v) <= 4 * np.log2(n) * X.eps(T) * M
    q = int(np.argmax(np.abs(a.astype(np.float64) * b).ravel(order="F")))
    drop = v - float(a.ravel(order="F")[q]) * float(b.ravel(order="F")[q])
    assert abs(got - drop) > 4 * np.log2(n) * X.eps(T) * M


# ----------------------------------------------------------------------------- the projection half of mom_step!

import xref_project as XP

# extents (ghosts included): 3 and 4 -- one and two inside cells, where planes 0, 1, n-2 and n-1 coincide or touch -- in
# every direction in turn, and non-cubic shapes
BC_SHAPES = [(3, 6), (7, 3), (4, 5), (6, 4), (9, 7), (3, 5, 6), (6, 3, 5), (5, 6, 3), (4, 7, 5), (5, 4, 7), (7, 5, 4), (8, 6, 5)]


def bc_neighbour(D, saveexit, perdir):
    """a neighbouring (saveexit, perdir) setting whose BC! must differ: the exit flag where x is not periodic (it only
    acts there), else x made a wall"""
    return (not saveexit, perdir) if 0 not in perdir else (saveexit, tuple(j for j in perdir if j != 0))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", BC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_BC_perBC_oracle_vs_xref(T, Ng):
    """BC! and perBC! against the reference's plane loops replayed in xref.BC / xref.perBC, every cell, exactly: every
    subset of periodic directions x saveexit; control: the neighbouring setting's result differs."""
    D = len(Ng)
    U = (1.0, 0.5, -0.25)[:D]
    for q, perdir in enumerate([()] + periodic_subsets(D)):
        h = field(Ng + (D,), T, "random", 2000 + q)
        for saveexit in (False, True):
            got = h.copy(order="F")
            O.BC(got, U, saveexit, perdir)
            assert np.array_equal(got, X.BC(h, U, saveexit, perdir)), (perdir, saveexit)
            assert not np.array_equal(got, X.BC(h, U, *bc_neighbour(D, saveexit, perdir)))
        if perdir:
            s = field(Ng, T, "random", 2100 + q)
            got = s.copy(order="F")
            O.perBC(got, perdir)
            assert np.array_equal(got, X.perBC(s, perdir)), perdir
            assert not np.array_equal(got, X.perBC(s, perdir[1:]))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(6, 3), (9, 10), (5, 3, 3), (7, 6, 5)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("kind", ["random", "ties", "scaled-up", "scaled-down"])
def test_exitBC_oracle_vs_xref(T, Ng, kind):
    """exitBC! against xref.exit_bc (K = 8) on one exit cell and on planes of 8 and 20, U and u0 of one scale; every other
    cell untouched.  Controls: the imbalance correction left out, dt off by 64 K eps (random u0 on a plane)."""
    D = len(Ng)
    sc = {"scaled-up": 2.0 ** (20 if T == np.float32 else 60), "scaled-down": 2.0 ** -(20 if T == np.float32 else 60)}.get(kind, 1.0)
    u0 = field(Ng + (D,), T, kind, 2200)
    h = field(Ng + (D,), T, kind, 2201)
    U1, dt = float(T(0.75 * sc)), float(T(0.3))
    got = h.copy(order="F")
    O.exitBC(got, u0, (U1, 0.0, 0.0), dt)
    n = XP.check_exit(WORST, f"exit_bc {np.dtype(T).name}", T, got, u0, U1, dt, dt_control=kind == "random" and min(Ng[1:]) > 3)
    assert n == int(np.prod([m - 2 for m in Ng[1:]]))
    got[XP.exit_cells(Ng) + (0,)] = h[XP.exit_cells(Ng) + (0,)]
    assert np.array_equal(got, h)


# (inside extents, periodic directions): both solver types (the reference builds a MultiLevelPoisson on all but the second
# and third), 2-D and 3-D, walls and periodic faces with L != 0 on them
PROJECT_CASES = [((24, 16), ()), ((18, 11), ()), ((5, 9, 3), ()), ((16, 12, 12), ()), ((16, 12, 12), (1,)), ((16, 12, 12), (0, 2)),
                 ((12, 12), (0, 1))]


def _oracle_project_run(T, dims, perdir, kind, w, dt, seed=2300):
    Ng = tuple(n + 2 for n in dims)
    h = project_fields(Ng, T, kind, seed, body_block(Ng), perdir)
    a, b = XP.oracle_flow(dims, T, h, perdir, dt)
    n = XP.oracle_project(a, b, w)
    p0 = XP.oracle_level0(b)
    assert np.array_equal(p0.L, h["mu0"])
    after = {"u": a.u.copy(order="F"), "p": a.p.copy(order="F"), "r": p0.r.copy(order="F")}
    return h, n, after, p0.D.copy(order="F"), p0.iD.copy(order="F")      # (copies: the solver's arrays go with it)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims,perdir", PROJECT_CASES)
@pytest.mark.parametrize("w", [1.0, 0.5])
def test_project_oracle_vs_xref(T, dims, perdir, w):
    """project! with dt = 0.25 on random, tie-rich and step-front velocities (xref_inputs.project_fields): the velocity
    correction (xref.correct, K = 4), the solve's invariant (xref.project_defect, K = 8 + 64 n), n <= 4 -- a condition on
    the input --, the periodic ghost cells of p; the controls of xref_project.check_project.  Then with dt = 0.3: the
    ghost cells of p in the non-periodic directions show the two scale passes alone (xref.scale_x, K = 2)."""
    tn = np.dtype(T).name
    ran = 0
    for kind in ("random", "ties", "step"):
        h, n, after, Dh, iDh = _oracle_project_run(T, dims, perdir, kind, w, 0.25)
        assert 1 <= n <= 4, n
        ran += XP.check_project(WORST, tn, T, perdir, w * 0.25, n, h, after, h["mu0"], Dh, iDh)
    assert ran >= 2
    if len(perdir) < len(dims):
        h, n, after, _, _ = _oracle_project_run(T, dims, perdir, "random", w, 0.3)
        dt = float(T(0.3))
        changed = XP.check_scale(WORST, f"scale_x {tn}", "scale_x", T, perdir, h["p"], after["p"], dt)
        assert changed > 0 or T == np.float64       # (the two roundings do move cells)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims,perdir", STEP_CASES)
def test_mom_step_u_oracle_vs_xref(T, dims, perdir):
    """After one mom_step! with dt = 0.25 the inside cells hold 0.5*(u' + μddn(μ₁,f) + V + μ₀*f) - L*∂(0.125*p)
    (xref.mom_u, K = 12: Flow.jl:166-167, :134, :142) with u' from the oracle's operators replayed in the step's order, held
    bit-identical to the step, f as stored and p the final pressure.  Controls: dt off by 64 K eps, p shifted one plane,
    u' replaced by u_start.  And BC! of the final u changes no bit of it."""
    a, b, up, us, gc, dt = _oracle_step_and_twin(T, dims, perdir)
    assert dt == 0.25 and max(b.n) <= 32
    h = {"u": up, "f": a.f, "V": a.V, "mu0": a.mu0, "mu1": a.mu1, "L": a.mu0, "p": a.p, "got": a.u}
    XP.check_mom_u(WORST, f"mom_u {np.dtype(T).name}", T, perdir, h, us, dt)
    assert np.array_equal(X.BC(a.u, O.BCTuple(a.U, a.dt[:-1], a.D), False, perdir), a.u)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims,perdir", STEP_CASES[:2])
def test_mom_step_scale_chain_oracle_vs_xref(T, dims, perdir):
    """The four scale passes of a whole step (*dt, /dt, *0.5dt, /0.5dt with dt = 0.3) on the ghost cells of p, which
    nothing else writes: within 4 roundings of the start value (xref.scale_x, K = 4); control: p*dt fails."""
    Ng = tuple(n + 2 for n in dims)
    p0 = field(Ng, T, "random", 2400)
    a, *_ = _oracle_step_and_twin(T, dims, perdir, dt0=0.3, p0=p0)
    XP.check_scale(WORST, f"scale_x4 {np.dtype(T).name}", "scale_x4", T, perdir, p0, a.p, a.dt[0])


def test_worst_ratios_are_recorded():
    """(prints the largest |oracle-ref|/(eps*M) seen per operator in this module: -s shows it)"""
    print("\nworst |oracle-ref|/(eps_T*M):", {k: round(v, 3) for k, v in sorted(WORST.items())})
