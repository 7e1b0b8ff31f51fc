"""The projection half of mom_step! (Flow.jl:159-168) on the device against the extended-precision reference
tests/xref.py: BC! and perBC! exactly (the one-launch closed form k_bc_vec_all and the per-plane form), exitBC!, project!
alone (the velocity correction k_correct3 and its per-cell fallback, the solve's invariant r + A x = div(u) - shift with
the fused div-in-residual! kernel on and off), the scale passes of k_scale_flat (head, tail, chained form), and the
velocity a whole fused step leaves with its ghost cells.  The comparisons and their controls are those of
test_xref_cpu.py (xref_project.py); every case asserts, from predicates mirrored from the C++ dispatch, which branch it
reaches."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xref as X
import xref_project as XP
from waterlily_amd import sim as S
from waterlily_amd.sim import Opt
from xref_inputs import body_block, field, periodic_subsets, project_fields
from test_xref_gpu import WORST, V, dev                 # one record of worst ratios for the GPU xref files
from test_xref_step_gpu import fused_mom_step, make_step, step_cases

TYPES = [np.float32, np.float64]
K = X.K
S7_BY, WL_MAXB = 4, 16384                               # wl_stencil7.h, wl_common.h


# ----------------------------------------------------------------------------- a. BC!, perBC!

# extents (ghosts included).  3 and 4 in every direction in turn (one and two inside cells: planes 0, 1, n-2, n-1 coincide
# or touch); (20, 30, 18): boundary planes of 540, 360 and 600 cells -- three different counts, so a swapped e1/e2 decode of
# k_bc_vec_all cannot pass, one above 256 and two above 512 (pos = blockIdx.x*256 + thread crosses workgroups); 2-D
# boundary lines of 300 and 600 cells
BC_SHAPES = [(3, 6), (7, 3), (4, 5), (6, 4), (300, 7), (7, 600), (3, 5, 6), (6, 3, 5), (5, 6, 3), (4, 7, 5), (5, 4, 7), (7, 5, 4),
             (20, 30, 18)]


def bc_neighbour(saveexit, perdir):
    """a neighbouring (saveexit, perdir) setting whose BC! must differ: the exit flag where x is not periodic (it only
    acts there), else x made a wall"""
    return (not saveexit, perdir) if 0 not in perdir else (saveexit, tuple(j for j in perdir if j != 0))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("fused", [1, 0])
def test_BC_perBC_hip_vs_xref(T, fused):
    """BC! in one launch (k_bc_vec_all, Opt.BC_FUSED = 1) and plane by plane (0), and perBC!, against the reference's
    plane loops replayed by xref.BC / xref.perBC: the whole array, exactly, every subset of periodic directions x
    saveexit, padded and dense layouts alternating; control: the neighbouring setting's result differs."""
    U = (1.0, 0.5, -0.25)
    planes = set()
    with S.options({Opt.BC_FUSED: fused}):
        for q, Ng in enumerate(BC_SHAPES):
            D = len(Ng)
            planes |= {int(np.prod(Ng)) // n for n in Ng}
            for r, perdir in enumerate([()] + periodic_subsets(D)):
                h = field(Ng + (D,), T, "random", 3000 + 10 * q + r)
                for saveexit in (False, True):
                    a = dev(h, D, (q + r) % 2 == 0)
                    S.BC(a, U[:D], saveexit, perdir)
                    got = S.to_host(a)
                    assert np.array_equal(got, X.BC(h, U[:D], saveexit, perdir)), (Ng, perdir, saveexit)
                    assert not np.array_equal(got, X.BC(h, U[:D], *bc_neighbour(saveexit, perdir)))
                if perdir:
                    s = field(Ng, T, "random", 3500 + 10 * q + r)
                    a = dev(s, D, (q + r) % 2 == 1)
                    S.perBC(a, perdir)
                    assert np.array_equal(S.to_host(a), X.perBC(s, perdir)), (Ng, perdir)
                    assert not np.array_equal(S.to_host(a), X.perBC(s, perdir[1:]))
    assert any(256 < p <= 512 for p in planes) and any(p > 512 for p in planes) and {540, 360, 600} <= planes


# ----------------------------------------------------------------------------- b. exitBC!

# exit planes of 1, 255, 256, 257 and a few thousand cells, 2-D and 3-D (257 is prime: 257 x 1)
EXIT_SHAPES = [(6, 3), (5, 257), (5, 258), (5, 259), (5, 3002), (5, 3, 3), (5, 19, 17), (6, 18, 18), (5, 259, 3), (5, 66, 52)]


@pytest.mark.parametrize("T", TYPES)
def test_exitBC_hip_vs_xref(T):
    """exitBC! against xref.exit_bc (K = 8) on exit planes of one cell, of 255 / 256 / 257 cells (the workgroup edge of
    the reduction) and of 3000 and 3200, every other cell untouched; controls: the imbalance correction left out, dt off
    by 64 K eps, the next sample."""
    tn = np.dtype(T).name
    counts = set()
    for q, Ng in enumerate(EXIT_SHAPES):
        D = len(Ng)
        kind = ("random", "ties", "random", "scaled-up", "scaled-down")[q % 5] if min(Ng[1:]) > 3 else "random"
        sc = {"scaled-up": 2.0 ** (20 if T == np.float32 else 60), "scaled-down": 2.0 ** -(20 if T == np.float32 else 60)}.get(kind, 1.0)
        u0, h = field(Ng + (D,), T, kind, 3600 + q), field(Ng + (D,), T, kind, 3650 + q)
        U1, dt = float(T(0.75 * sc)), float(T(0.3))
        a, a0 = dev(h, D, q % 2 == 0), dev(u0, D, q % 2 == 0)
        S.exitBC(a, a0, (U1, 0.0, 0.0), dt)
        got = S.to_host(a)
        n = XP.check_exit(WORST, f"exit_bc {tn}", T, got, u0, U1, dt, dt_control=kind == "random" and min(Ng[1:]) > 3)
        counts.add(n)
        got[XP.exit_cells(Ng) + (0,)] = h[XP.exit_cells(Ng) + (0,)]
        assert np.array_equal(got, h) and np.array_equal(S.to_host(a0), u0)
    assert {1, 255, 256, 257, 3000, 3200} <= counts


# ----------------------------------------------------------------------------- c. project! alone

def stencil7_ok(Ng, T):
    """wl_stencil7.h stencil7_ok"""
    return len(Ng) == 3 and S.get_option(Opt.STENCIL7_VEC) != 0 and (Ng[0] - 2) % V(T) == 0 and Ng[0] - 2 >= V(T)


def pcg_vec_ok(Ng, T):
    return S.get_option(Opt.PCG_VEC) != 0 and stencil7_ok(Ng, T)


def chunking(tpp, nown, cap, target_k):
    """wl_stencil7.h chunking: (planes per chunk, chunks)"""
    target = min(max(target_k * 1024, 1024), WL_MAXB)
    want = target // tpp
    if 0 < cap < want:
        want = cap
    want = min(max(want, 1), nown)
    clen = (nown + want - 1) // want
    return clen, (nown + clen - 1) // clen


def project_plan(Ng, T, perdir):
    """flow_project (wl_api.hip) and op_correct (wl_ops.h) on a single device, the flow and the solver in one layout: which
    correction kernel runs, with how many x tiles and which z chunks; whether div is formed inside residual!"""
    v = V(T)
    plan = {"correct": "k_correct3" if stencil7_ok(Ng, T) else "fallback", "fused_div": False}
    if len(Ng) == 3:
        ntx, nty = (Ng[0] - 2 + 64 * v - 1) // (64 * v), (Ng[1] - 2 + S7_BY - 1) // S7_BY
        tpp = (ntx * nty + 7) // 8 * 8
        rowvec_fits = ((ntx * ((Ng[1] - 2 + 3) // 4) + 7) // 8) * 8 <= WL_MAXB
        plan["fused_div"] = bool(S.get_option(Opt.DIV_IN_RESIDUAL) != 0 and pcg_vec_ok(Ng, T) and rowvec_fits and not perdir)
        if plan["correct"] == "k_correct3":
            plan["ntx"] = ntx
            plan["clen"], plan["nchunk"] = chunking(tpp, Ng[2] - 2, 0, 16)
    return plan


def project_cases(T):
    """(inside extents, periodic directions).  x: V, 63V, 64V, 65V (the vector kernels; one and two x tiles) and V-1, V+1,
    64V+1 (the per-cell fallbacks of op_correct and op_div); y one below, at and one above a multiple of S7_BY; z 1, 2, 3,
    5, 6; two 2-D cases; a y-periodic and an xz-periodic 3-D case (fused div off, d/dx across the periodic faces, whose L
    is 1); a hierarchy (64V x 12 x 12 and 24 x 16: the others are single levels).  Every z chunk of k_correct3 is one
    plane long at these sizes (test_project_plane_pipeline_hip_vs_xref has the longer ones)."""
    v = V(T)
    return [((v, 5, 1), ()), ((63 * v, 8, 2), ()), ((64 * v, 7, 6), ()), ((65 * v, 9, 5), ()), ((64 * v, 3, 3), ()),
            ((v - 1, 4, 3), ()), ((v + 1, 7, 5), ()), ((64 * v + 1, 5, 2), ()), ((24, 16), ()), ((18, 11), ()),
            ((64 * v, 8, 5), (1,)), ((65 * v, 5, 5), (0, 2)), ((64 * v, 12, 12), ())]


def device_flow(dims, T, h, perdir, padded, dt=0.25, exitBC=False):
    """Flow and pressure solver on the host fields of project_fields, the solver type the reference builds"""
    a = S.Flow(dims, h["U"], T=T, nu=0.05, perdir=perdir, padded=padded, dt=dt, exitBC=exitBC)
    for k in ("u", "mu0", "mu1", "V", "p"):
        S.upload(getattr(a, k), h[k])
    if len(XP.levels_of(a.N)) > 2:
        b = S.MultiLevelPoisson(a.p, a.mu0, a.sigma, padded=padded, perdir=perdir)
    else:
        b = S.Poisson(a.p, a.mu0, a.sigma, perdir=perdir)
    return a, b


def run_project_case(T, q, dims, perdir, ws, seen):
    """project! on one case for the weights ws: the checks of test_project_hip_vs_xref; returns the controls that ran"""
    tn = np.dtype(T).name
    Ng = tuple(n + 2 for n in dims)
    plan = project_plan(Ng, T, perdir)
    ran = 0
    for w in ws:
        kind = ("random", "ties", "step")[(q + int(w == 0.5)) % 3]
        h = project_fields(Ng, T, kind, 3700 + q, body_block(Ng), perdir)
        a, b = device_flow(dims, T, h, perdir, (q + int(w == 0.5)) % 2 == 0)
        nu_, nr_ = S.uniform_rows(b, 0)
        if len(Ng) == 3 and not perdir and Ng[1] >= 9 and Ng[2] >= 5:
            assert 0 < nu_ < nr_, (dims, nu_, nr_)            # rows through the block and rows clear of it
            seen.add(("uniform", plan["correct"]))
        n = S.project(a, b, w)
        ao, bo = XP.oracle_flow(dims, T, h, perdir)
        assert n == XP.oracle_project(ao, bo, w) and 1 <= n <= 4, (dims, w, n)
        lv = b.levels[0]
        after = {"u": S.to_host(a.u), "p": S.to_host(a.p), "r": S.to_host(lv.r)}
        assert np.array_equal(S.to_host(lv.L), h["mu0"])
        ran += XP.check_project(WORST, tn, T, perdir, w * 0.25, n, h, after, h["mu0"], S.to_host(lv.D), S.to_host(lv.iD))
    seen |= {("correct", plan["correct"]), ("fused_div", plan["fused_div"])}
    if plan["correct"] == "k_correct3":
        seen |= {("ntx", plan["ntx"]), ("clen", 1 if plan["clen"] == 1 else ("even" if plan["clen"] % 2 == 0 else "odd>=3")),
                 ("chunks>=2", plan["nchunk"] >= 2)}
    return ran


@pytest.mark.parametrize("T", TYPES)
def test_project_hip_vs_xref(T):
    """project! alone, w = 1 and 0.5, dt = 0.25, on random / tie-rich / step-front velocities scaled as in
    test_xref_cpu.py (xref_inputs.project_fields; the body block across the x seam, so that some rows are
    coefficient-uniform and some are not), padded and dense layouts alternating.  At every inside cell and component
    u_after against xref.correct with x = p_after*w*dt (K = 4); r + A x = div(u_before) - shift (xref.project_defect,
    K = 8 + 64 n); n <= 4 and equal to the oracle's count; the periodic ghost cells of p_after exactly the wrapped inside
    cells.  Controls (xref_project.check_project): L of one face off by 64 K eps, x taken one cell to the left, one
    velocity of u_before off by 64 K eps M, the next sample."""
    seen = set()
    ran = 0
    for q, (dims, perdir) in enumerate(project_cases(T)):
        ran += run_project_case(T, q, dims, perdir, (1.0, 0.5), seen)
    assert {("correct", "k_correct3"), ("correct", "fallback"), ("fused_div", True), ("fused_div", False), ("ntx", 1), ("ntx", 2),
            ("clen", 1), ("chunks>=2", True), ("uniform", "k_correct3")} <= seen, seen
    assert ran >= 20


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("rows,perdir,w,clen", [(4 * 3280, (), 0.5, "even"), (4 * 5464, (0,), 1.0, "odd>=3")])
def test_project_plane_pipeline_hip_vs_xref(T, rows, perdir, w, clen):
    """The same checks where k_correct3 marches over more than one plane per workgroup.  Its z chunks are one plane long
    until a plane has more than 16384/planes workgroups (chunking() with the 16 K grid op_correct asks for), so the two
    operand sets of its software pipeline and the xm carried from plane to plane only run on large grids; two tall thin
    ones (x = V: one lane per row) reach them with few cells: 3280 workgroups per plane and 5 planes give chunks of 2, 2, 1
    planes, 5464 give chunks of 3, 2 -- both operand sets, an odd and an even chunk, and the reload at the chunk seams.
    The second is periodic in x: the face of the row's first cell then has L = 1, so the lane-0 load of the left
    neighbour counts in both operand sets (at a wall that face has L = 0 and hides it)."""
    seen = set()
    assert run_project_case(T, 20, (V(T), rows, 5), perdir, (w,), seen) >= 2
    assert {("correct", "k_correct3"), ("clen", clen), ("chunks>=2", True), ("fused_div", not perdir)} <= seen, seen
    assert perdir or ("uniform", "k_correct3") in seen


# ----------------------------------------------------------------------------- d. the scale passes

def scale_plan(p: torch.Tensor):
    """op_scale_all (wl_ops.h) on the pressure array: (unaligned head, tail) of k_scale_flat, in elements"""
    v = 16 // p.element_size()
    n = p.shape[-1] * p.stride()[-1]                                   # span(g)
    mis = (p.data_ptr() & 15) // p.element_size()
    head = min(v - mis if mis else 0, n)
    return head, (n - head) % v


def scale_cases(T):
    """(inside extents, periodic directions, padded): a dense array of a whole number of 16-B vectors (head 0, tail 0); a
    dense one of odd extents (tail != 0), with walls and z-periodic; a padded one (head 1) whose rows fill their pitch, so
    that the last cells of the last row are the tail.  In a z-periodic array the head and the tail are periodic ghost cells:
    perBC! at the end of solver! overwrites them with x, and a scale pass that skipped them leaves them a factor dt from
    the wrapped inside cells -- on a never-written ghost cell a skipped head or tail would show nothing, both passes
    skipping alike."""
    v = V(T)
    return [((v, 4, 2), (), False), ((v + 1, 5, 3), (), False), ((v + 1, 5, 3), (2,), False), ((30, 5, 3), (2,), True),
            ((30, 5, 3), (), True)]


@pytest.mark.parametrize("T", TYPES)
def test_scale_passes_hip_vs_xref(T):
    """project! with dt = 0.3, w = 1 and 0.5: the ghost cells of p in the non-periodic directions, which the solver never
    writes, show the two passes of k_scale_flat alone (xref.scale_x, K = 2), the periodic ones must equal the wrapped
    inside cells exactly; after a whole mom_step! the chained form (*dt, /dt and *0.5dt in one pass, /0.5dt: K = 4).
    Control: the same cells against p*dt fail."""
    tn = np.dtype(T).name
    dt = float(T(0.3))
    seen = set()
    for q, (dims, perdir, padded) in enumerate(scale_cases(T)):
        Ng = tuple(n + 2 for n in dims)
        h = project_fields(Ng, T, "random", 3800 + q, body_block(Ng), perdir)
        for w in (1.0, 0.5):
            a, b = device_flow(dims, T, h, perdir, padded, dt=0.3)
            head, tail = scale_plan(a.p)
            seen |= {("head", head > 0), ("tail", tail > 0), ("periodic", bool(perdir), head > 0, tail > 0)}
            assert 1 <= S.project(a, b, w) <= 4
            pa = S.to_host(a.p)
            XP.check_scale(WORST, f"scale_x {tn}", "scale_x", T, perdir, h["p"], pa, dt)
            assert np.array_equal(pa, X.perBC(pa, perdir))
        # the chain of a whole step
        assert S.get_option(Opt.SCALE_CHAIN) != 0
        a, b = device_flow(dims, T, h, perdir, padded, dt=0.3)
        S.flow_update(a)
        S.mom_step(a, b)
        pa = S.to_host(a.p)
        XP.check_scale(WORST, f"scale_x4 {tn}", "scale_x4", T, perdir, h["p"], pa, dt)
        assert np.array_equal(pa, X.perBC(pa, perdir))
    assert {("head", True), ("head", False), ("tail", True), ("tail", False), ("periodic", True, False, True),
            ("periodic", True, True, True)} <= seen, seen


# ----------------------------------------------------------------------------- e. a whole step on the fused path

@pytest.mark.parametrize("T", TYPES)
def test_mom_step_fused_u_hip_vs_xref(T):
    """The velocity one mom_step! (dt = 0.25) leaves on the fused path, at every inside cell and component, against
    xref.mom_u (K = 12): u' from the u0 array, f as stored, p the final pressure, at the tile-edge shapes of
    test_xref_step_gpu.py.  Controls: dt off by 64 K eps, p shifted one plane, u' replaced by u_start.  And the ghost
    cells: BC!(u, U) replayed by xref.BC changes no bit of the final u."""
    tn = np.dtype(T).name
    for q, dims in enumerate(step_cases(T)):
        a, b, Ng = make_step(dims, T, q % 2 == 1, 3900 + q)
        assert fused_mom_step(a, row_flags_built=True) and a.dt == [0.25]
        us = S.to_host(a.u).copy()
        S.mom_step(a, b)
        up = S.to_host(a.u0)
        assert not np.array_equal(up, us)                      # u0 holds u', not the copy of u_start
        u = S.to_host(a.u)
        h = {"u": up, "got": u, "L": S.to_host(a.mu0), "p": S.to_host(a.p)}
        h.update({k: S.to_host(getattr(a, k)) for k in ("f", "V", "mu0", "mu1")})
        XP.check_mom_u(WORST, f"mom_u {tn}", T, (), h, us, 0.25)
        assert np.array_equal(X.BC(u, (1.0, 0.0, 0.0), False, ()), u)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("xghost,exitBC", [(1, False), (0, False), (1, True), (0, True)])
def test_mom_step_ghost_cells_hip_vs_xref(T, xghost, exitBC):
    """The ghost cells of u after a whole step with the x-ghost cells written by the producing kernels (xbc_apply in
    k_correct3 and the busy-row kernel, CdFin, the skip_x launch of BC!; Opt.XGHOST_IN_KERNEL = 1) and by BC! alone (0), on
    the fused path and with a convective exit (the unfused path, saveexit): applying xref.BC(u, U, exitBC, ()) to a host
    copy changes no bit -- the reference's sequence, independently of any kernel.  Control: neither does it hold for the
    other exit setting, nor for a velocity whose ghost cells were not set."""
    with S.options({Opt.XGHOST_IN_KERNEL: xghost}):
        for q, dims in enumerate(step_cases(T)[:4]):
            Ng = tuple(n + 2 for n in dims)
            if exitBC:
                h = project_fields(Ng, T, "random", 3950 + q, body_block(Ng))
                h["u"] = field(Ng + (3,), T, "random", 3960 + q, 0.7, 1.3)
                h["U"] = (1.0, 0.0, 0.0)
                a, b = device_flow(dims, T, h, (), q % 2 == 0, exitBC=True)
                S.BC(a.u, h["U"], True)
                S.flow_update(a)
            else:
                a, b, _ = make_step(dims, T, q % 2 == 0, 3950 + q)
            assert fused_mom_step(a, row_flags_built=True) == (not exitBC)
            S.mom_step(a, b)
            u = S.to_host(a.u)
            assert np.array_equal(X.BC(u, (1.0, 0.0, 0.0), exitBC, ()), u), (dims, xghost, exitBC)
            assert not np.array_equal(X.BC(u, (1.0, 0.0, 0.0), not exitBC, ()), u) or not exitBC
            assert not np.array_equal(X.BC(S.to_host(a.f), (1.0, 0.0, 0.0), exitBC, ()), S.to_host(a.f))


def test_worst_ratios_are_recorded():
    """(prints the largest |hip-ref|/(eps*M) per check of the projection half seen in this module: -s shows it)"""
    keys = ("exit_bc", "correct", "project_defect", "scale_x", "mom_u")
    print("\nworst |hip-ref|/(eps_T*M):", {k: round(v, 3) for k, v in sorted(WORST.items()) if k.startswith(keys)})
