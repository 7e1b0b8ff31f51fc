"""The kernels that only run inside a whole step or a whole V-cycle, against the extended-precision reference tests/xref.py
(the operators one by one are in test_xref_gpu.py):
- the fused conv_diff!+BDIM! kernels of mom_step! (Opt.BDIM_IN_CONVDIFF): the corrector's f after one step (xref.mom_f) at
  the 64-cell x tile seams, odd and even numbers of interior tile rows of the 8-row (Float32) and 4-row tiles, the
  smallest z extents the tiled kernel takes; and the fused step bit-identical to the separate BDIM! pass there;
- the one-workgroup bottom of the V-cycle (wl_coarse.h): tail on against the per-level launches, the invariant
  r + A x = rhs on the level below, and the whole solver! against the oracle, at 4096 cells exactly, at one cell per
  thread, where a level fits CV_MAXCELLS but not the LDS copy, and with the tail forced onto a level of more cells;
- restrictL! with periodic directions, alone and through a whole periodic hierarchy.
Every case asserts, from predicates mirrored from the C++ dispatch, which branch it reaches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xref as X
from oracle import wl_oracle as O
from waterlily_amd import sim as S
from waterlily_amd.sim import Opt
from xref_inputs import coefficients, field, periodic_subsets, step_fields
from test_xref_gpu import WORST, check, dev, fails     # one record of worst ratios for both GPU xref files

TYPES = [np.float32, np.float64]
K = X.K


# ----------------------------------------------------------------------------- mom_step!: fused conv_diff!+BDIM!

def fused_mom_step(a: S.Flow, row_flags_built: bool) -> bool:
    """wl_api.hip flow_mom_step: `turns` = BDIM_IN_CONVDIFF and BDIM_ROWFLAGS && a->rowfree && a->busy && no periodic direction && no
    convective exit && conv_diff_tiled(g, 0) (wl_ops.h: D == 3, CONVDIFF_TILED, every extent >= 5).  a->rowfree and a->busy are
    not visible from the host: both are set by flow_compact_busy, which every wl_flow_update runs (the busy list is
    allocated even when empty), so the caller passes whether wl_flow_update ran on this flow.  The tests also check the
    observable the fused path leaves: the u0 array holds u', not the copy of u_start (wl_mom_step)."""
    return (a.D == 3 and S.get_option(Opt.BDIM_IN_CONVDIFF) != 0 and S.get_option(Opt.BDIM_ROWFLAGS) != 0 and row_flags_built
            and not a.perdir and not a.exitBC and S.get_option(Opt.CONVDIFF_TILED) != 0 and all(n >= 5 for n in a.N))


def cd_tiles(Ng, T):
    """launch_convdiff3 (wl_convdiff.h) on extents Ng: x tiles, tile rows of the shared-flux kernel by height (8, 4) and
    the tile rows the shell kernel takes, planes of the shared-flux kernel"""
    ntx = (Ng[0] - 2 + 63) // 64
    nty_all = (Ng[1] + 3) // 4
    tlo, thi = 1, int((Ng[1] - 6) / 4)                     # (C division: truncates)
    klo, khi = 2, Ng[2] - 3
    use8 = np.dtype(T) == np.float32
    odd = use8 and (thi - tlo + 1) % 2 == 1 and thi > tlo
    if odd:
        thi -= 1                                           # 8-row tiles: an odd tile row goes to the shell
    assert S.get_option(Opt.CONVDIFF_SHARED_FLUX) != 0 and thi >= tlo and khi >= klo, "the shared-flux kernel must run"
    rows = (thi - tlo + 1) * 4
    n8 = rows // 8 if use8 else 0
    return dict(ntx=ntx, n8=n8, n4=(rows - 8 * n8) // 4, shell_rows=nty_all - (thi + 1), planes=khi - klo + 1,
                odd=odd)


def step_cases(T):
    """interior (x, y, z): x on the 64-cell seams; y = 8, 12, 16, 20 -> 1, 2, 3, 4 interior tile rows (Float32: the 4-row
    instance, one 8-row tile row, one 8-row + one odd row in the shell, two 8-row); z = 3 (the smallest conv_diff_tiled
    takes: one shared-flux plane) and 4"""
    ys = [8, 12, 16, 20] if np.dtype(T) == np.float32 else [8, 12]
    xs = [63, 64, 65, 128, 129]
    out = [(x, ys[q % len(ys)], 3 + q % 2) for q, x in enumerate(xs)] + [(64, y, 4) for y in ys[1:]] + [(65, ys[0], 4)]
    return list(dict.fromkeys(out))


def make_step(dims, T, padded, seed):
    """Flow + pressure solver with step_fields: a body block across the x seam at cell 64 (x from 58, at most 13 cells),
    y from 2 to mid-height (busy rows in the first tile row and interior ones, the rows above body-free), every plane"""
    Ng = tuple(n + 2 for n in dims)
    block = (slice(min(58, Ng[0] - 6), min(71, Ng[0] - 2)), slice(2, Ng[1] // 2 + 1), slice(1, Ng[2] - 1))
    h = step_fields(Ng, T, seed, block)
    U = (1.0, 0.0, 0.0)
    a = S.Flow(dims, U, T=T, nu=0.05, g=lambda i, t: 0.05 * (i + 1) * (1 + t), padded=padded)
    for k in ("u", "mu0", "mu1", "V"):
        S.upload(getattr(a, k), h[k])
    S.BC(a.u, U)
    S.flow_update(a)
    from waterlily_amd.dist import divisible
    lv = [Ng]
    while divisible(lv[-1]):
        lv.append(tuple(1 + n // 2 for n in lv[-1]))
    b = S.MultiLevelPoisson(a.p, a.mu0, a.sigma, padded=padded) if len(lv) > 2 else S.Poisson(a.p, a.mu0, a.sigma)
    return a, b, Ng


@pytest.mark.parametrize("T", TYPES)
def test_mom_step_fused_f_hip_vs_xref(T):
    """f after one mom_step! on the fused path (the default) against xref.mom_f (K = 12) at every interior cell and
    component, padded and dense layouts alternating; u_start from before the step, u' from the u0 array (where the fused
    path leaves it), V, dt, g_corr.  Controls: dt off by 64K eps, the samples shifted one plane in z, u_start replaced by
    u' must fail."""
    tn = np.dtype(T).name
    seen = set()
    for q, dims in enumerate(step_cases(T)):
        a, b, Ng = make_step(dims, T, q % 2 == 0, 800 + q)
        assert fused_mom_step(a, row_flags_built=True)      # (make_step ran wl_flow_update)
        t = cd_tiles(Ng, T)
        seen |= {("seam", (Ng[0] - 2) % 64), ("n8", t["n8"]), ("n4", t["n4"]), ("planes", t["planes"]),
                 ("odd", t["odd"])}
        us = S.to_host(a.u).copy()
        dt_list = list(a.dt)
        S.mom_step(a, b)
        gc = S.accel_tuple(a.g, a.U, dt_list, 3)
        dt = dt_list[-1]
        up, f, V = S.to_host(a.u0), S.to_host(a.f), S.to_host(a.V)
        assert not np.array_equal(up, us)                      # u0 holds u', not the copy of u_start
        C = X.host_cells({"u": up, "us": us, "V": V}, N=Ng)
        ins = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C.idx, Ng)], axis=0)
        C0 = X.host_cells({"u": up, "us": up, "V": V}, N=Ng)
        sh = X.host_cells({"u": up, "us": us, "V": V}, idx=(C.idx[0], C.idx[1], C.idx[2] + 1), N=Ng)
        m = ins & (C.idx[2] < Ng[2] - 2)
        for c in range(3):
            got = f[..., c].ravel(order="F")
            v, M = X.mom_f(C, c, a.nu, dt, gc[c])
            check("mom_f", f"mom_step f {tn}", got[ins], v[ins], M[ins], T)
            assert fails("mom_f", got[ins], *[w[ins] for w in X.mom_f(C, c, a.nu, dt * (1 + 64 * K["mom_f"] * X.eps(T)), gc[c])], T)
            assert fails("mom_f", got[ins], *[w[ins] for w in X.mom_f(C0, c, a.nu, dt, gc[c])], T)
            vs, Ms = X.mom_f(sh, c, a.nu, dt, gc[c])
            assert fails("mom_f", got[m], vs[m], Ms[m], T)
    # the edges this test is for were all reached: partial and full last x tiles; the 4-row instance, the 8-row one, an
    # odd tile row in the shell (Float32); one and two shared-flux planes
    assert {("seam", 63), ("seam", 0), ("seam", 1), ("planes", 1), ("planes", 2), ("n4", 1)} <= seen
    if np.dtype(T) == np.float32:
        assert {("n8", 1), ("n8", 2), ("odd", True)} <= seen


@pytest.mark.parametrize("T", TYPES)
def test_mom_step_fused_bit_exact_at_tile_edges(T):
    """At the shapes above, three steps with Opt.BDIM_IN_CONVDIFF on and off: u (ghost cells included), p, f, dt and the V-cycle
    counts bit-identical; the u0 array holds u' (fused) or u_start (separate)."""
    for q, dims in enumerate(step_cases(T)):
        runs = []
        for on in (1, 0):
            with S.options({Opt.BDIM_IN_CONVDIFF: on}):
                a, b, Ng = make_step(dims, T, q % 2 == 1, 900 + q)
                assert fused_mom_step(a, row_flags_built=True) == bool(on)
                for _ in range(3):
                    u_before = S.to_host(a.u).copy()
                    S.mom_step(a, b)
                runs.append((b.n[:], list(a.dt), S.to_host(a.u), S.to_host(a.p), S.to_host(a.f), S.to_host(a.u0), u_before))
        x, y = runs
        assert x[0] == y[0] and x[1] == y[1], dims
        for k in (2, 3, 4):
            assert np.array_equal(x[k], y[k]), (dims, k)
        assert np.array_equal(y[5], y[6]) and not np.array_equal(x[5], x[6])


# ----------------------------------------------------------------------------- the coarse V-cycle tail

CV_THREADS, CV_MAXLEV, CV_MAXCELLS, CV_LDS = 1024, 8, 4096, 7936    # wl_coarse.h


def interior(Ng):
    return int(np.prod([n - 2 for n in Ng]))


def tail_plan(shapes, l, opt6):
    """mg_vcycle (wl_api.hip) called on level l of a non-periodic single-device hierarchy with the fused smoothers: the
    level the one-workgroup tail starts on (None: per-level launches down to the bottom), and for every tail level the
    pcg! form k_coarse_vcycle takes: 'lds1' / 'lds4' (cv_pcg_onchip with 1 / CV_CPT cells per thread, where cv_fits_lds
    holds) or 'global' (cv_pcg)"""
    thr = CV_MAXCELLS if opt6 == 1 else opt6
    assert S.get_option(Opt.SMOOTH_FUSED) != 0
    for c in range(l + 1, len(shapes)):
        if opt6 and interior(shapes[c]) <= thr and len(shapes) - c <= CV_MAXLEV:
            kinds = []
            for Ng in shapes[c:]:
                fits = int(np.prod(Ng)) <= CV_LDS and interior(Ng) <= CV_MAXCELLS
                kinds.append(("lds1" if interior(Ng) <= CV_THREADS else "lds4") if fits else "global")
            return c, kinds
    return None, []


# (interior dims, Opt.COARSE_TAIL, level the tail must start on, pcg! form of that level)
TAIL_CASES = [
    ((32, 32, 32), 1, 1, "lds4"),        # exactly 4096 cells: 16^3
    ((128, 128), 1, 1, "lds4"),          # 64^2
    ((16, 16, 16), 1, 1, "lds1"),        # 512 cells: one per thread
    ((64, 32), 1, 1, "lds1"),
    ((512, 8, 8), 1, 1, "global"),       # 256x4x4 = 4096 cells, 258*6*6 = 9288 elements > CV_LDS: cv_pcg inside the launch
    ((32, 32, 36), 1, 2, "lds1"),        # 16x16x18 = 4608 cells just above: per-level launches, the tail one level lower
    ((64, 64, 64), 32768, 1, "global"),  # COARSE_TAIL forced: 32^3 cells in the tail
    ((256, 128), 8192, 1, "global"),     # 128x64 = 8192
]


def tail_system(dims, T, seed, padded=True):
    Ng = tuple(n + 2 for n in dims)
    D = len(Ng)
    L = coefficients(Ng, T, seed)
    z = field(Ng, T, "random", seed + 1)
    z[tuple(slice(1, n - 1) for n in Ng)] -= z[tuple(slice(1, n - 1) for n in Ng)].mean().astype(T)
    x = np.zeros(Ng, T, order="F")
    return L, z, S.MultiLevelPoisson(dev(x, D, padded), dev(L, D, padded), dev(z, D, padded))


def level_host(ph, l):
    lv = ph.levels[l]
    torch.cuda.synchronize()
    return {k: S.to_host(getattr(lv, k)) for k in ("L", "D", "iD", "x", "r", "eps", "z")}


def invariant_ratio(h1, rhs, rhsM, T):
    v, M = X.coarse_defect(h1, rhs, rhsM)
    return X.worst(np.zeros(len(v)), v, M, T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "x".join(map(str, c[0])) + f"-opt6={c[1]}")
def test_coarse_tail_hip_vs_per_level_and_xref(T, case):
    """One Vcycle!(ml, 0) with the tail (Opt.COARSE_TAIL as given) against the same V-cycle in per-level launches (COARSE_TAIL = 0):
    pcg! leaves every coarse level by the same exit, and x, r, eps, z agree within K = coarse_tail times eps_T and the
    level's scale of that array (the per-cell arithmetic is the same, the Float64 dot sums group differently: pcg!'s alpha
    and beta can round apart by an ulp of T, and the levels above inherit that through prolongate!); control: level 1's
    x and r against the next sample fail.  On level 1, from the host state before the call, r + A x = rhs
    (rhs = restrict! of the Jacobi! residual) within K = coarse_inv of |rhs| + |A||x| (eight updates of x and r: the
    smoother, prolongate!+increment!, six pcg! iterations); a face of level 1's L perturbed after update! must break it.
    Then solver! against the oracle: the same V-cycle counts, x within 10 rtol."""
    dims, opt6, start, kind = case
    tn = np.dtype(T).name
    Ng = tuple(n + 2 for n in dims)
    D = len(Ng)
    seed = 1000 + sum(dims)
    L, z, ph = tail_system(dims, T, seed)
    shapes = [tuple(lv.shape) for lv in ph.levels]
    c, kinds = tail_plan(shapes, 0, opt6)
    assert c == start and kinds[0] == kind, (shapes, c, kinds)
    assert tail_plan(shapes, 0, 0) == (None, [])
    S.residual(ph)
    h0 = level_host(ph, 0)
    rhs, rhsM = X.vcycle_rhs(h0, shapes[1])
    got = {}
    for o in (opt6, 0):
        _, _, p = tail_system(dims, T, seed)
        S.residual(p)
        # (per-level pcg! stores z' = r*iD, as the reference and the tail do)
        with S.options({Opt.COARSE_TAIL: o, Opt.PCG_RECOMPUTE_PRECOND: 1 if o else 0}):
            S.Vcycle(p, 0)
        got[o] = [level_host(p, l) for l in range(len(shapes))]
    on, off = got[opt6], got[0]
    for l in range(1, len(shapes)):
        ins = tuple(slice(1, n - 1) for n in shapes[l])
        hl = {k: a[ins] if k != "L" else a for k, a in off[l].items()}
        # the level's scales, from the per-level run: r, max of |r| + |A||x| (|A||x| = coarse_defect's bound with rhs = 0);
        # x, max |x|; eps and z (r*iD or A*eps): the r scale times max |iD| and twice the largest diagonal
        _, AxM = X.coarse_defect(off[l], 0, 0)
        sr = float(np.max(np.abs(hl["r"]).ravel(order="F") + AxM))
        se = 2 * sr * float(np.max(np.abs(hl["iD"]))) * max(1.0, float(np.max(np.abs(hl["D"]))))
        scale = {"x": float(np.max(np.abs(hl["x"]))), "r": sr, "eps": se, "z": se}
        # pcg!'s exit, read from z: r*iD (bitwise) after a rho exit, A*eps after the alpha exit or the sixth iteration
        ex = [np.array_equal(h[l]["z"][ins], (h[l]["r"] * h[l]["iD"])[ins]) for h in (on, off)]
        assert ex[0] == ex[1], f"level {l}: pcg! left by a different exit with the tail on and off"
        for k in ("x", "r", "eps", "z"):
            a, b = (h[l][k][ins].ravel(order="F").astype(np.float64) for h in (on, off))
            u = float(np.max(np.abs(a - b))) / (X.eps(T) * scale[k])
            WORST[f"coarse tail {tn}"] = max(WORST.get(f"coarse tail {tn}", 0.0), u)
            assert u <= K["coarse_tail"], (l, k, u)
            if l == 1 and k in ("x", "r"):            # control: the same values against the next sample must fail
                assert float(np.max(np.abs(a[:-1] - b[1:]))) / (X.eps(T) * scale[k]) > K["coarse_tail"], (l, k)
    for run in (on, off):
        w = invariant_ratio(run[1], rhs, rhsM, T)
        WORST[f"coarse r+Ax {tn}"] = max(WORST.get(f"coarse r+Ax {tn}", 0.0), w)
        assert w <= K["coarse_inv"], w
    # control: level 1's L with one face off by 25 % after update! (D, iD keep the old values)
    _, _, p = tail_system(dims, T, seed)
    S.residual(p)
    L1 = p.levels[1].L
    I = tuple(n // 2 for n in shapes[1])
    L1[I + (0,)] *= 1.25
    with S.options({Opt.COARSE_TAIL: opt6}):
        S.Vcycle(p, 0)
    hp = level_host(p, 1)
    hp["L"], hp["D"] = on[1]["L"], on[1]["D"]
    assert invariant_ratio(hp, rhs, rhsM, T) > K["coarse_inv"]
    # the whole solver against the oracle
    xh = np.zeros(Ng, T, order="F")
    po = O.MultiLevelPoisson(xh.copy(order="F"), L.copy(order="F"), z.copy(order="F"))
    _, _, p = tail_system(dims, T, seed)
    with S.options({Opt.COARSE_TAIL: opt6}):
        S.solver(p)
    O.solver(po)
    assert p.n == po.n
    rt = 1e-5 if np.dtype(T) == np.float32 else 1e-12
    xo = po.x.astype(np.float64)
    assert np.max(np.abs(S.to_host(p.x).astype(np.float64) - xo)) <= 10 * rt * max(1e-30, float(np.max(np.abs(xo))))


# ----------------------------------------------------------------------------- periodic restrictL!

@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_restrictL_periodic_hip_vs_xref(T, padded):
    """restrictL! (op_restrictL + coarse_L_finish's BC!) with every subset of periodic directions at the shapes of
    test_multilevel_transfers_hip_vs_xref, every cell of the coarse array (K = 4); control: the wall-case reference
    fails."""
    tn = np.dtype(T).name
    v4 = 4 if np.dtype(T) == np.float32 else 2
    for q, Ng in enumerate([(10, 10), (2 * 65 * v4 // 2 + 2, 10, 8), (10, 8, 6)]):
        D = len(Ng)
        Nc = tuple(1 + n // 2 for n in Ng)
        L = field(Ng + (D,), T, "random", 640 + q, 0.2, 1.0)
        for perdir in periodic_subsets(D):
            aL = dev(np.zeros(Nc + (D,), T, order="F"), D, padded)
            S.restrictL(aL, dev(L, D, padded), perdir=perdir)
            aLh = S.to_host(aL)
            CL = X.host_cells({"b": L}, N=Nc, NA=Ng)
            for c in range(D):
                got = aLh[..., c].ravel(order="F")
                check("restrictL", f"restrictL periodic {tn}", got, *X.restrictL(CL, c, perdir=perdir), T)
                assert fails("restrictL", got, *X.restrictL(CL, c), T)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("perdir", [(1,), (1, 2), (0, 1, 2)])
def test_periodic_hierarchy_hip_vs_xref(T, perdir):
    """A periodic MultiLevelPoisson after update!: on every level L (restrictL! of the level above, K = 4), D (K = 4) and
    iD (K = 8) against the reference; the fine L is random with a solid block and BC!(L, 0, false, perdir), as measure!
    leaves mu0.  Control: each coarse L against the wall-case reference fails."""
    tn = np.dtype(T).name
    dims = (32, 16, 16)
    Ng = tuple(n + 2 for n in dims)
    D = 3
    L = field(Ng + (D,), T, "random", 660, 0.2, 1.0)
    L[tuple(slice(n // 3, n // 3 + 3) for n in Ng)] = 0          # a solid block: D = 0, iD = 0 there
    Ld = dev(L, D, True)
    S.BC(Ld, (0.0,) * D, False, perdir)                # what measure! leaves in mu0 of a periodic run
    zero = np.zeros(Ng, T, order="F")
    ph = S.MultiLevelPoisson(dev(zero, D, True), Ld, dev(zero, D, True), perdir=perdir)
    assert len(ph.levels) >= 3
    prev = None
    for l, lv in enumerate(ph.levels):
        Lh, Dh, iDh = S.to_host(lv.L), S.to_host(lv.D), S.to_host(lv.iD)
        N = Lh.shape[:D]
        if prev is not None:
            CL = X.host_cells({"b": prev}, N=N, NA=prev.shape[:D])
            for c in range(D):
                got = Lh[..., c].ravel(order="F")
                check("restrictL", f"restrictL periodic {tn}", got, *X.restrictL(CL, c, perdir=perdir), T)
                assert fails("restrictL", got, *X.restrictL(CL, c), T)
        C = X.host_cells({"L": Lh}, N=N)
        ins = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C.idx, N)], axis=0)
        Dv, DM = X.diag(C)
        check("diag", f"diag periodic {tn}", Dh.ravel(order="F")[ins], Dv[ins], DM[ins], T)
        iv, iM = X.inv_diag(Dv, DM, T)
        check("iD", f"iD periodic {tn}", iDh.ravel(order="F")[ins], iv[ins], iM[ins], T)
        prev = Lh


def test_worst_ratios_are_recorded():
    """(prints the largest |hip-ref|/(eps*M) per check seen in this module: -s shows it)"""
    print("\nworst |hip-ref|/(eps_T*M):", {k: round(v, 3) for k, v in sorted(WORST.items())})
