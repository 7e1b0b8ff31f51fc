"""The projection half of mom_step! (Flow.jl:159-168) held to tests/xref.py: the comparisons and their controls, shared
by test_xref_cpu.py (the oracle) and test_xref_project_gpu.py (the kernels).  Everything here works on host arrays and
records the largest ratio per key in the `worst` dictionary it is handed; the oracle is only used to run the reference's
project! on a single level (oracle_project), which the GPU file needs for the iteration counts."""
import ctypes

import numpy as np

import xref as X
from oracle import wl_oracle as O

K = X.K


def inside_mask(C, Ng):
    return np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C.idx, Ng)], axis=0)


def held(worst, key, k, got, v, M, T, control=True):
    """|got - v| <= k eps M at every cell, recorded under `key`; control: against the next sample it must fail"""
    w = X.worst(got, v, M, T)
    worst[key] = max(worst.get(key, 0.0), w)
    assert w <= k, f"{key}: |got-ref| = {w:.3g} eps*M > K = {k}"
    assert not control or X.worst(got[:-1], v[1:], M[1:], T) > k, f"{key}: control (samples shifted by one) did not fail"


# ----------------------------------------------------------------------------- the oracle's project!, any solver type

def levels_of(Ng):
    """restrictML (MultiLevelPoisson.jl:18-25,36-37): the extents of the hierarchy on a grid of extents Ng"""
    lv = [tuple(Ng)]
    while all(n % 2 == 0 and n > 4 for n in lv[-1]):
        lv.append(tuple(1 + n // 2 for n in lv[-1]))
    return lv


def oracle_flow(dims, T, h, perdir=(), dt=0.25):
    """the oracle's Flow and pressure solver (MultiLevelPoisson where the reference builds one, else Poisson) on the host
    fields h of xref_inputs.project_fields"""
    a = O.Flow(dims, h["U"], T=T, nu=0.05, perdir=perdir, dt=dt)
    for k in ("u", "mu0", "mu1", "V", "p"):
        getattr(a, k)[...] = h[k]
    ml = len(levels_of(a.N)) > 2
    return a, (O.MultiLevelPoisson if ml else O.Poisson)(a.p, a.mu0, a.sigma, perdir=perdir)


def oracle_level0(b):
    return b.levels[0] if isinstance(b, O.MultiLevelPoisson) else b


def oracle_project(a, b, w) -> int:
    """Flow.jl:137-145 on the oracle: wlo_project for a MultiLevelPoisson; for a single level the same statements from the
    oracle's div and solver!, the scale passes and the correction loop in T arithmetic as wlo_project has them"""
    if isinstance(b, O.MultiLevelPoisson):
        return O.project(a, b, w)
    dtT = a.T.type(a.dt[-1])
    dtd = w * float(dtT)
    O._fn("wlo_div", a.T)(O._p(b.z), O._p(a.u), ctypes.byref(a.grid))
    b.x[...] = b.x * dtT if w == 1.0 else (b.x.astype(np.float64) * dtd).astype(a.T)
    O.solver(b)
    ins = O.inside(b.x)
    for c in range(a.D):
        lo = tuple(slice(0, n - 2) if d == c else slice(1, n - 1) for d, n in enumerate(a.N))
        a.u[ins + (c,)] -= b.L[ins + (c,)] * (b.x[ins] - b.x[lo])
    b.x[...] = b.x / dtT if w == 1.0 else (b.x.astype(np.float64) / dtd).astype(a.T)
    return b.n[-1]


# ----------------------------------------------------------------------------- exitBC!

def exit_cells(Ng):
    """exitR of util.jl:218: x index N1 (0-based N-1), every other index inside, in column-major order"""
    rest = np.meshgrid(*[np.arange(1, n - 1) for n in Ng[1:]], indexing="ij")
    rest = [a.ravel(order="F") for a in rest]
    return (np.full(rest[0].size, Ng[0] - 1),) + tuple(rest)


def check_exit(worst, key, T, got_u, u0, U1, dt, dt_control=True):
    """exitBC! (K = 8): component 0 of the exit cells of got_u against xref.exit_bc on u0; every other cell of got_u must
    be what the caller put there (the caller checks that).  Controls: the imbalance correction left out; dt off by 64 K
    eps (where asked: it needs exit cells whose upwind difference is not small)."""
    Ng = u0.shape[:-1]
    idx = exit_cells(Ng)
    C = X.host_cells({"u0": u0}, idx=idx, N=Ng)
    got = got_u[idx + (0,)]
    v, M = X.exit_bc(C, U1, dt)
    held(worst, key, K["exit_bc"], got, v, M, T, control=len(got) > 1 and len(np.unique(got)) > 1)
    assert X.worst(got, *X.exit_bc(C, U1, dt, correction=False), T) > K["exit_bc"]
    if dt_control:
        assert X.worst(got, *X.exit_bc(C, U1, dt * (1 + 64 * K["exit_bc"] * X.eps(T))), T) > K["exit_bc"]
    return len(got)


# ----------------------------------------------------------------------------- project!

def nonperiodic_ghosts(Ng, perdir):
    """the cells with an index 0 or N-1 in a non-periodic direction: nothing between project!'s two scale passes writes
    them (perBC! copies such a cell only from another one of them)"""
    ix = np.indices(Ng)
    m = np.zeros(Ng, bool)
    for d, n in enumerate(Ng):
        if d not in perdir:
            m |= (ix[d] == 0) | (ix[d] == n - 1)
    return m


def check_project(worst, tn, T, perdir, s, n, before, after, L, D, iD):
    """One project! with s = w*dt a power of two, from host arrays: before = {"u", "p"}, after = {"u", "p", "r"}, the
    solver's L, D, iD, its iteration count n.  At every inside cell and component u_after against xref.correct with
    x = p_after*s (K = 4); r_final + A x = div(u_before) - shift (xref.project_defect, K = 8 + 64 n); the periodic ghost
    cells of p_after equal to the wrapped inside cells.  Controls: L of one face off by 64 K eps where it weighs most; x
    taken one cell to the left; one velocity of u_before off by 64 K eps M in a single cell (the defect); the next sample.
    Returns how many of the L and x controls the input allowed (a face must carry 1/16 of its cell's M; a shifted x must
    differ where L != 0): the callers assert that they ran."""
    assert X.dyadic(s)
    Ng = L.shape[:-1]
    Dn = len(Ng)
    x = (after["p"] * np.dtype(T).type(s)).astype(T)                   # exact: s is a power of two
    assert np.array_equal(x.astype(np.float64), after["p"].astype(np.float64) * s)
    assert np.array_equal(after["p"], X.perBC(after["p"], perdir))
    h = {"u": before["u"], "L": L, "x": x}
    C = X.host_cells(h, N=Ng)
    ins = inside_mask(C, Ng)
    kc = K["correct"]
    ran = 0                                                              # controls that could run on this input
    for c in range(Dn):
        got = after["u"][..., c].ravel(order="F")[ins]
        v, M = X.correct(C, c)
        # (the z component of a grid one plane thick is BC!'s constant at every inside cell: no next-sample control there)
        held(worst, f"correct {tn}", kc, got, v[ins], M[ins], T, control=len(np.unique(got)) > 1)
        # controls: one face of L, where L*(x[I]-x[I-dc]) weighs most in M
        a, b = C("x"), C("x", X.dl(c, Dn, -1))
        Mf = np.asarray(M, np.float64)
        wgt = np.where(ins & (Mf > 0), np.abs(np.asarray(C("L", (), c) * (a - b), np.float64)) / np.where(Mf > 0, Mf, 1), 0)
        q = int(np.argmax(wgt))
        if wgt[q] > 1 / 16:                                             # (64 K eps * weight > K eps)
            Lp = L.copy(order="F")
            Lp[tuple(int(w[q]) for w in C.idx) + (c,)] *= 1 + 64 * kc * X.eps(T)
            vp, Mp = X.correct(X.host_cells({**h, "L": Lp}, N=Ng), c)
            assert X.worst(got, vp[ins], Mp[ins], T) > kc, "correct: control (one face of L) did not fail"
            ran += 1
        xs = np.asfortranarray(np.roll(x, 1, axis=0))                   # x taken one cell to the left
        vs, Ms = X.correct(X.host_cells({**h, "x": xs}, N=Ng), c)
        m = ins & (C.idx[0] >= 2)
        if np.any(np.asarray(C("L", (), c), np.float64)[m] * (x != xs).ravel(order="F")[m] != 0):
            assert X.worst(after["u"][..., c].ravel(order="F")[m], vs[m], Ms[m], T) > kc, "correct: control (x shifted) did not fail"
            ran += 1
    # the solve's invariant
    kp = X.K_project(n)
    hb = {"u": before["u"], "p": before["p"], "L": L, "D": D, "iD": iD}
    Cb = X.host_cells(hb, idx=tuple(w[ins] for w in C.idx), N=Ng)
    shift, shiftM = X.project_shift(Cb, s, T)
    hd = {"u": before["u"], "p": after["p"], "r": after["r"], "L": L, "D": D, "iD": iD}
    Cd = X.host_cells(hd, idx=Cb.idx, N=Ng)
    v, M = X.project_defect(Cd, s, shift, shiftM)
    zero = np.zeros(len(v))
    held(worst, f"project_defect {tn}", kp, zero, v, M, T, control=False)
    worst[f"project_defect/K {tn}"] = max(worst.get(f"project_defect/K {tn}", 0.0), X.worst(zero, v, M, T) / kp)
    q = int(np.argmax(np.asarray(M, np.float64)))                       # control: one velocity off in one cell
    up = before["u"].copy(order="F")
    up[tuple(int(w[q]) for w in Cd.idx) + (0,)] += np.dtype(T).type(64 * kp * X.eps(T) * float(M[q]))
    vp, Mp = X.project_defect(X.host_cells({**hd, "u": up}, idx=Cb.idx, N=Ng), s, shift, shiftM)
    assert X.worst(zero, vp, Mp, T) > kp, "project_defect: control (one velocity off) did not fail"
    return ran


def check_scale(worst, key, kname, T, perdir, p_before, p_after, dt):
    """The scale passes alone (xref.scale_x): the ghost cells of p in the non-periodic directions, which the solver never
    writes, against the value they started with (K = 2 for one project!, 4 for the chain of a whole step); control: the
    same cells against p*dt must fail."""
    assert not X.dyadic(dt) and not X.dyadic(0.5 * dt)
    m = nonperiodic_ghosts(p_before.shape, perdir).ravel(order="F")
    idx = tuple(w.ravel(order="F")[m] for w in np.indices(p_before.shape))
    C = X.host_cells({"p": p_before}, idx=idx, N=p_before.shape)
    got = p_after.ravel(order="F")[m]
    v, M = X.scale_x(C)
    held(worst, key, K[kname], got, v, M, T)
    assert X.worst(got, v * X.LD(dt), M, T) > K[kname], f"{key}: control (p*dt) did not fail"
    return int(np.count_nonzero(got != p_before.ravel(order="F")[m]))


# ----------------------------------------------------------------------------- a whole step

def check_mom_u(worst, key, T, perdir, h, us, dt):
    """The final velocity of one mom_step! against xref.mom_u (K = 12) at every inside cell and component (the normal
    component's plane 1 is BC!'s): h = {"u": u', "f", "V", "mu0", "mu1", "L", "p", "got": final u}.  Controls: dt off by
    64 K eps; p shifted one plane (the last direction); u' replaced by u_start."""
    Ng = h["p"].shape
    Dn = len(Ng)
    k = K["mom_u"]
    C = X.host_cells(h, N=Ng)
    ins = inside_mask(C, Ng)
    ps = np.asfortranarray(np.roll(h["p"], 1, axis=Dn - 1))
    Cs = X.host_cells({**h, "p": ps}, N=Ng)
    C0 = X.host_cells({**h, "u": us}, N=Ng)
    for c in range(Dn):
        m = ins & ((C.idx[c] >= 2) | (c in perdir))
        got = h["got"][..., c].ravel(order="F")[m]
        v, M = X.mom_u(C, c, dt)
        held(worst, key, k, got, v[m], M[m], T)
        for Cx, d in ((C, dt * (1 + 64 * k * X.eps(T))), (Cs, dt), (C0, dt)):
            vp, Mp = X.mom_u(Cx, c, d, planted=True)
            assert X.worst(got, vp[m], Mp[m], T) > k, f"{key}: a control did not fail"
