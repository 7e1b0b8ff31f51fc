"""Every iteration of a pcg! call on the device against the extended-precision replay xref.pcg_step_ref (the driver and
what it checks: xref_pcg.replay; the inputs: xref_inputs.pcg_cases), at the smallest shapes that reach each plan of
wl_pcg.h: scalar and vector kernels, dots finished by finalize launches or inside the next kernel, x updated at once or
owed to the direction kernel, z' and z stored or recomputed (the 7-point update kernel), the z-chunk cap binding, more
partials than one pass of a 256-thread sum, the largest plane of the in-kernel sums and the first beyond it, the periodic
shell sum appended to the partials of z.eps, and the exits :132 and :138 in iteration 2.  A call of it=k is compared
with the replay of iteration k alone, fed from the read-backs of it=k-1 and it=k-2: an error of a few ulp in one
iteration's beta, or in one lane, has nothing to hide behind.  Every case asserts the plan it reached from a mirror of
pcg_plan and chunking, and the mirror against the library's launch counts.  L and x and z are uploaded padded (padding
poisoned) or dense."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xref as X
from waterlily_amd import _lib
from waterlily_amd import sim as S
from waterlily_amd.sim import Opt
from xref_inputs import pcg_body, pcg_cases, pcg_chains
from xref_pcg import replay
from test_xref_gpu import WORST, V, dev                  # one record of worst ratios for the GPU xref files

TYPES = [np.float32, np.float64]
OPTS = {"default": {}, "aeps": {Opt.PCG_RECOMPUTE_AEPS: 2}, "aeps-rows2": {Opt.PCG_RECOMPUTE_AEPS: 2, Opt.STENCIL7_ROWS: 2},
        "finalize": {Opt.PCG_DOTS_IN_KERNEL: 0}, "xnow": {Opt.PCG_DEFER_X: 0}, "zstored": {Opt.PCG_RECOMPUTE_PRECOND: 0},
        "scalar": {Opt.PCG_VEC: 0}}
K_INIT, K_MULT, K_UPDATE, K_DIR, K_SCALAR = 13, 14, 15, 16, 18     # WL_K_* of include/wlhip.h
WL_MAXB, WL_PCG_PARTIALS, WL_GRID = 16384, 1024, 4096              # wl_common.h, wl_stencil7.h


def cdiv(a, b):
    return -(-a // b)


def chunking(tpp, nown, cap, target_k):
    """wl_stencil7.h chunking: (planes per chunk, chunks)"""
    want = min(max(target_k * 1024, 1024), WL_MAXB) // tpp
    if 0 < cap < want:
        want = cap
    want = min(max(want, 1), nown)
    clen = cdiv(nown, want)
    return clen, cdiv(nown, clen)


def range_partials(dims):
    """wl_common.h mk_tiling: the workgroups (= partials) of a scalar range kernel over the interior"""
    ext = tuple(dims) + (1,) * (3 - len(dims))
    a = 0 if ext[0] > 1 else (1 if ext[1] > 1 else (2 if ext[2] > 1 else 0))
    b, c = sorted(((a + 1) % 3, (a + 2) % 3))
    ptb = min(cdiv(cdiv(ext[a], 64) * cdiv(ext[b], 4), 8) * 8, WL_GRID)
    want = min(max(WL_GRID // ptb, 1), ext[c])
    clen = max(cdiv(ext[c], want), 1)
    return ptb * cdiv(ext[c], clen)


def pcg_plan(dims, T, perdir=()):
    """wl_pcg.h pcg_plan on a single device, under the options in force, and the partial counts its launches leave:
    np_init (rho), np_mult (z.eps, the periodic shell sum included: np_shell of them), np_update (r.z')"""
    g = S.get_option
    D, v, cells = len(dims), V(T), int(np.prod(dims))
    s7 = D == 3 and g(Opt.STENCIL7_VEC) != 0 and dims[0] % v == 0 and dims[0] >= v
    vec = s7 and g(Opt.PCG_VEC) != 0
    xdef, zrec = g(Opt.PCG_DEFER_X) != 0, g(Opt.PCG_RECOMPUTE_PRECOND) != 0
    ra, dk = g(Opt.PCG_RECOMPUTE_AEPS), g(Opt.PCG_DOTS_IN_KERNEL)
    zst = D == 3 and vec and zrec and (ra == 2 or (ra == 3 and cells < 2 ** 26) or (ra == 1 and 2 ** 22 <= cells < 2 ** 26))
    ntx = cdiv(dims[0], 64 * v)
    tpp_v = cdiv(ntx * cdiv(dims[1], 4), 8) * 8 if D == 3 else 0
    gates = vec and xdef and zrec and tpp_v > 0 and (dk == 2 or (dk == 1 and cells <= 2 ** 25)) and tpp_v <= WL_PCG_PARTIALS
    zcap = max(WL_PCG_PARTIALS // max(tpp_v, 1), 1) if gates else 0
    pl = dict(vec=vec, s7=s7, xdef=xdef, zrec=zrec, zst=zst, form="IN_KERNEL" if gates else "FINALIZE", zcap=zcap, tpp_v=tpp_v)
    if vec:
        pl["chunks"] = chunking(tpp_v, dims[2], zcap, g(Opt.STREAM_GRID_K))
        pl["np_init"] = pl["np_update"] = tpp_v * pl["chunks"][1]
    else:
        pl["np_init"] = pl["np_update"] = range_partials(dims)
    if s7:                                                    # the 7-point kernel: mult, and the update when z is not stored
        two = dims[1] % 2 == 0 and g(Opt.STENCIL7_ROWS) == 2
        tpp7 = cdiv(ntx * cdiv(dims[1], 8 if two else 4), 8) * 8
        pl["chunks7"] = chunking(tpp7, dims[2], zcap, g(Opt.STENCIL7_GRID_K))
        pl["np_mult"] = tpp7 * pl["chunks7"][1]
        pl["rows2"] = two
        if zst:
            pl["np_update"] = pl["np_mult"]
    else:
        pl["np_mult"] = range_partials(dims)
    pl["np_shell"] = 0
    if perdir:                                                # launch_shell_red: blocks per plane * planes
        Ng = tuple(n + 2 for n in dims)
        big = max(int(np.prod([n for e, n in enumerate(Ng) if e != d])) for d in range(D))
        pl["np_shell"] = min(max(cdiv(big, 256), 1), 32 if gates else 256) * 2 * len(perdir)
        pl["np_mult"] += pl["np_shell"]
    assert max(pl["np_init"], pl["np_mult"], pl["np_update"]) <= WL_MAXB
    return pl


def launches():
    out = {}
    for k in (K_INIT, K_MULT, K_UPDATE, K_DIR, K_SCALAR):
        nl, nc = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().wl_prof_counts(k, C.byref(nl), C.byref(nc)))
        out[k] = nl.value
    return out


def expected_launches(pl, k, perdir):
    """what pcg!(it=k) enqueues, exits or not (a kernel behind a closed gate is still launched): one init, k mult (and k
    shell sums on a periodic level), k updates, k-1 directions; finalize launches after the init kernel and after every
    mult and update (FINALIZE), or the one that publishes the state at the end (IN_KERNEL)"""
    return {K_INIT: 1, K_MULT: k * (2 if perdir else 1), K_UPDATE: k, K_DIR: k - 1,
            K_SCALAR: 1 + 2 * k if pl["form"] == "FINALIZE" else 1}


def device_replay(inp, dims, T, padded, key, want=None):
    """xref_pcg.replay on a single-level S.Poisson under the options in force; every call's launch counts against the
    mirrored plan; `want`: plan entries this case is there to reach.  Returns (plan, replay's result, the Poisson)."""
    D = len(dims)
    ph = S.Poisson(dev(inp["x0"], D, padded), dev(inp["L"], D, padded), dev(inp["z"], D, padded), perdir=inp["perdir"])
    pl = pcg_plan(dims, T, inp["perdir"])
    for name, val in (want or {}).items():
        assert pl[name] == val, f"{key}: plan {name} = {pl[name]}, this case is there for {val} ({pl})"

    def run(k):
        S.upload(ph.x, inp["x0"])
        S.upload(ph.r, inp["r0"])
        S.upload(ph.z, inp["z"])
        before = launches()
        n = S.pcg(ph, it=k)
        after = launches()
        got = {c: after[c] - before[c] for c in after}
        assert got == expected_launches(pl, k, inp["perdir"]), f"{key} it={k}: launches {got} do not fit the plan {pl}"
        return n, S.to_host(ph.x), S.to_host(ph.r), S.to_host(ph.eps)
    out = replay(run, inp, S.to_host(ph.D), S.to_host(ph.iD), T, 6, WORST, f"pcg6 {np.dtype(T).name} ")
    return pl, out, ph


def cases(T, *groups):
    return [c for c in pcg_cases(T) if c["group"] in groups]


# what the shapes of xref_inputs.pcg_cases are there to reach under the default options (index within the group)
WANT = {("first", 0): dict(vec=True, form="IN_KERNEL"), ("first", 1): dict(vec=False, s7=False, form="FINALIZE"),
        ("first", 2): dict(vec=True, form="IN_KERNEL"), ("first", 3): dict(vec=True, form="IN_KERNEL"),
        ("first", 4): dict(vec=True, form="IN_KERNEL"),
        ("small", 0): dict(vec=False, form="FINALIZE"), ("small", 1): dict(vec=False, form="FINALIZE", tpp_v=0),
        ("long", 0): dict(form="IN_KERNEL", np_init=320, np_mult=320),                      # > 256 partials
        ("long", 1): dict(form="IN_KERNEL", zcap=128, chunks=(2, 66), chunks7=(2, 66)),     # the cap of 128 chunks binds
        ("tall", 0): dict(form="IN_KERNEL", tpp_v=1024, zcap=1, np_init=1024, np_mult=1024),
        ("tall", 1): dict(form="FINALIZE", vec=True, tpp_v=1032)}


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("group", ["first", "small", "long", "tall", "rows"])
def test_pcg_every_iteration_default_plan(T, padded, group):
    """the default options on every body and row shape: six updates, no exit (five cells in Float64: pcg! converges and
    leaves through :138 -- whatever the reference does, n and the arrays follow it)"""
    for q, case in enumerate(cases(T, group)):
        inp = case["make"]()
        want = dict(WANT.get((group, q), {}))
        pl, out, ph = device_replay(inp, case["dims"], T, padded, f"{case['id']} default", want)
        if group == "rows":
            nu, nr = S.uniform_rows(ph, 0)
            assert 0 < nu < nr and pl["vec"] and pl["form"] == "IN_KERNEL"   # the row-constant path ran, and not for the odd row
        if not (group == "small" and q == 0):
            assert out["exit"] is None and out["n"] == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("opts", [k for k in OPTS if k != "default"])
def test_pcg_every_iteration_other_plans(T, padded, opts):
    """the first shapes (x = V, V+1, 63V, 64V, 65V) and the row cases under each other plan: the 7-point update kernel
    (one and two rows per thread: the even y extents take two), finalize launches on vector levels, x updated at once,
    z' stored, scalar kernels on vector-capable levels"""
    seen = set()
    with S.options(OPTS[opts]):
        for case in cases(T, "first", "rows"):
            pl, out, _ = device_replay(case["make"](), case["dims"], T, padded, f"{case['id']} {opts}")
            assert out["exit"] is None and out["n"] == [1, 2, 3, 4, 5, 6]
            seen.add((pl["s7"], pl["vec"], pl["zst"], pl["form"], pl["xdef"], pl["zrec"], pl.get("rows2", False)))
    vecs = {s for s in seen if s[0]}                          # the levels the vector kernels can take
    if opts.startswith("aeps"):
        assert vecs and all(s[2] and s[3] == "IN_KERNEL" for s in vecs)
        assert (opts == "aeps-rows2") == any(s[6] for s in vecs) and any(not s[6] for s in vecs)
    elif opts == "scalar":
        assert vecs and all(not s[1] and s[3] == "FINALIZE" for s in vecs)
    else:
        assert vecs and all(s[1] and not s[2] and s[3] == "FINALIZE" for s in vecs)
        assert all(s[4] == (opts != "xnow") and s[5] == (opts != "zstored") for s in vecs)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_pcg_z_chunk_cap_against_finalize_form(T, padded):
    """(V, 4, 131): with the in-kernel sums the cap of 128 chunks cuts z into 66 chunks of two planes (the last of one);
    with finalize launches the same level runs 131 chunks of one plane"""
    case = cases(T, "long")[1]
    with S.options(OPTS["finalize"]):
        device_replay(case["make"](), case["dims"], T, padded, f"{case['id']} finalize",
                      dict(form="FINALIZE", vec=True, zcap=0, chunks=(1, 131), np_init=8 * 131))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("opts", ["default", "xnow", "finalize", "aeps"])
def test_pcg_exits_in_iteration_two(T, padded, opts):
    """`chains` (x = 64V, 65V): two updates, then :138 in iteration 2 -- with a deferred x the direction kernel owes the
    second update and must apply it once, and nothing else; `wave`: one update, then :132 in iteration 2 with the new
    direction in eps.  Every later call leaves the same bits."""
    with S.options(OPTS[opts]):
        for case in cases(T, "chains", "wave"):
            pl, out, _ = device_replay(case["make"](), case["dims"], T, padded, f"{case['id']} {opts}", dict(vec=True, xdef=opts != "xnow"))
            assert pl["form"] == ("IN_KERNEL" if opts in ("default", "aeps") else "FINALIZE") and pl["zst"] == (opts == "aeps")
            if case["group"] == "chains":
                assert out["exit"] == (":138", 2) and out["n"] == [1, 2, 2, 2, 2, 2]
            else:
                assert out["exit"] == (":132", 2) and out["n"] == [1, 1, 1, 1, 1, 1]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("opts", ["default", "aeps"])
def test_pcg_periodic_shell_term(T, padded, opts):
    """periodic directions with ghost values of order 1 in the uploaded z: z.eps is a whole-array dot, the shell sum over
    the planes perBC! fills is appended to the partials of the interior sum (their number is then no multiple of 8); with
    the 7-point update kernel z is never stored inside, so the ghost values are all of z there is.  xref_pcg.replay's
    control drops the shell term from the reference and must fail."""
    with S.options(OPTS[opts]):
        for case in cases(T, "periodic"):
            inp = case["make"]()
            pl, out, _ = device_replay(inp, case["dims"], T, padded, f"{case['id']} {opts}", dict(vec=True, form="IN_KERNEL", zst=opts == "aeps"))
            assert pl["np_shell"] > 0 and pl["np_mult"] % 8 != 0
            assert out["exit"] is None and out["n"] == [1, 2, 3, 4, 5, 6]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("kind", ["body", "chains"])
def test_solver_r2_from_the_last_update_kernel(T, kind):
    """solver!(itmx=1) with the solver log on, at (65V, 5, 5) and (V, 4, 40).  `body`: pcg! makes its six updates and the last
    update kernel accumulates r.r (want_r2); `chains`: pcg! leaves in iteration 2, r2_valid stays 0 and the L2 pass that
    follows produces it.  Either way the logged r2 is within the suite's dot bound (1 ulp Float32, 4 log2(n) eps sum
    Float64) of the exact r.r of the r left behind, and the logged maximum of |r| is exact; control: r.r without its largest
    term fails."""
    v = V(T)
    for q, dims in enumerate([(65 * v, 5, 5), (v, 4, 40)]):
        Ng = tuple(n + 2 for n in dims)
        if kind == "body":
            inp = pcg_body(Ng, T, 900 + q)
            x0, z0 = inp["x0"], inp["z"]
        else:
            inp = pcg_chains(Ng, T, 910 + q, 1)
            x0, z0 = np.zeros(Ng, T, order="F"), inp["r0"]    # residual! then leaves r = z where iD != 0: the chains' r
        ph = S.Poisson(dev(x0, 3, q == 0), dev(inp["L"], 3, q == 0), dev(z0, 3, q == 0))
        assert pcg_plan(dims, T)["form"] == "IN_KERNEL"
        S.residual(ph)                                         # which way pcg! will go: the same start, it = 6
        if kind == "chains":
            assert np.array_equal(S.to_host(ph.r), inp["r0"])
        assert S.pcg(ph, it=6) == (6 if kind == "body" else 2)
        S.upload(ph.x, x0)
        S.upload(ph.z, z0)
        S.solver_log(ph, True)
        S.solver(ph, tol=0.0, itmx=1)
        rows = S.read_solver_log(ph)
        S.solver_log(ph, False)
        assert rows.shape == (2, 3) and rows[1, 0] == 1
        r = S.to_host(ph.r)
        n = int(np.prod(Ng))
        val, M = X.dot(r, r)
        big = float(np.max(np.abs(r.astype(np.float64)))) ** 2
        assert val > 0 and rows[1, 1] == X.Linf(r)
        if np.dtype(T) == np.float32:
            assert X.ulps(rows[1, 2], X.round_to(val, T), T) <= 1, (rows[1, 2], val)
            assert X.ulps(rows[1, 2], X.round_to(val - big, T), T) > 1
        else:
            assert abs(rows[1, 2] - val) <= 4 * math.log2(n) * X.eps(T) * M, (rows[1, 2], val)
            assert abs(rows[1, 2] - (val - big)) > 4 * math.log2(n) * X.eps(T) * M


def test_worst_ratios_are_recorded():
    """(prints the largest |hip-ref|/(eps*M) per check seen in this module: -s shows it)"""
    print("\nworst |hip-ref|/(eps_T*M):", {k: round(v, 3) for k, v in sorted(WORST.items()) if k.startswith("pcg6")})
