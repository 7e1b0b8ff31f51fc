"""GPU parity: every operator of the HIP path (through the C ABI) against the CPU oracle on identical seeded
inputs, then whole solves / time steps, then the reference's own known-answer tests run on the HIP path.

Tolerances (stated per test):
  * operators without reductions: BIT-EXACT (both sides round operation by operation, -ffp-contract=off);
  * operators with reductions (residual!, pcg!, solver!, mom_step!): both sides accumulate in Float64 and
    round once, only the summation tree differs (~1e-16 relative before rounding), so fields agree to a few
    ulp of their scale: 1e-5 (f32) / 1e-12 (f64) relative to max|field| -- far inside the north-star budget
    (u,p within solver tolerance 1e-4 abs on r.r);
  * iteration counts (pois.n) must be identical.
"""
import itertools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bodies
from oracle import geometry as G
from oracle import wl_oracle as O
from waterlily_amd import sim as S
from waterlily_amd.sim import Opt

TYPES = [np.float32, np.float64]
SHAPES = [(18, 12), (12, 10, 8)]


def rnd(shape, T, seed, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((lo + (hi - lo) * rng.random(shape)).astype(T))


def field(h: np.ndarray, D: int, padded=True):
    lay = S.Layout(h.shape[:D], h.dtype, padded)
    a = lay.alloc(h.shape[D:], "cuda:0")
    S.upload(a, h)
    return a


def same(a_dev, h, exact=True, tol=0.0):
    g = S.to_host(a_dev)
    if exact:
        assert np.array_equal(g, h), f"max abs diff {np.max(np.abs(g.astype(np.float64) - h))}"
    else:
        scale = max(1e-30, float(np.max(np.abs(h))))
        assert np.max(np.abs(g.astype(np.float64) - h.astype(np.float64))) <= tol * scale


def rtol(T):
    return 1e-5 if np.dtype(T) == np.float32 else 1e-12


# ----------------------------------------------------------------------------- util.jl operators

@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", SHAPES)
@pytest.mark.parametrize("padded", [True, False])
def test_bc_vec_per_exit(T, Ng, padded):
    D = len(Ng)
    U = (1.0, 0.5, -0.25)[:D]
    for saveexit, perdir in [(False, ()), (True, ()), (True, (1,)), (False, (0, D - 1))]:
        h = rnd(Ng + (D,), T, 1)
        a = field(h, D, padded)
        O.BC(h, U, saveexit, perdir)
        S.BC(a, U, saveexit, perdir)
        same(a, h)
    h = rnd(Ng, T, 2)
    a = field(h, D, padded)
    O.perBC(h, (0, D - 1))
    S.perBC(a, (0, D - 1))
    same(a, h)
    h, h0 = rnd(Ng + (D,), T, 3), rnd(Ng + (D,), T, 4)
    a, a0 = field(h, D, padded), field(h0, D, padded)
    O.exitBC(h, h0, U, 0.3)
    S.exitBC(a, a0, U, 0.3)
    same(a, h, exact=False, tol=4 * np.finfo(T).eps)   # mean flux: reduction order


# ----------------------------------------------------------------------------- Flow.jl operators

@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", SHAPES)
@pytest.mark.parametrize("perdir", [(), (0,), (1,), "all"])
def test_conv_diff_bit_exact(T, Ng, perdir):
    D = len(Ng)
    perdir = tuple(range(D)) if perdir == "all" else perdir
    u = rnd(Ng + (D,), T, 5)
    r, Phi = O.zeros(Ng + (D,), T), O.zeros(Ng, T)
    O.conv_diff(r, u, Phi, nu=0.05, perdir=perdir)
    ud, rd = field(u, D), field(rnd(Ng + (D,), T, 6), D)     # r starts as garbage: must be overwritten
    Pd = field(O.zeros(Ng, T), D)
    S.conv_diff(rd, ud, Pd, nu=0.05, perdir=perdir)
    same(rd, r)
    # Phi: the scatter form's scratch.  What it LEAVES in the ghost cells is read by the reference's whole-array reductions
    # (maximum(a.σ), z⋅ϵ): the shell must be the oracle's, bit for bit (top ghost cells: last flux written; index 1: untouched)
    shell = np.ones(Ng, bool)
    shell[O.inside(Phi)] = False
    assert np.any(Phi[shell] != 0) and np.array_equal(S.to_host(Pd)[shell], Phi[shell])


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(200, 14, 12), (70, 22, 10), (130, 30, 7), (66, 10, 9), (66, 38, 8)])
@pytest.mark.parametrize("shared", [1, 0])
def test_conv_diff_tile_paths_bit_exact(T, Ng, shared):
    """The LDS conv_diff kernels on shapes that exercise every tile kind: several x tiles per row (first / last with the
    domain's x-boundary faces, plain ones in between), partially filled last tiles, first / last tile rows and boundary
    planes (the per-cell-gather kernel) around the interior block (the shared-flux kernel, Opt.CONVDIFF_SHARED_FLUX): bit-exact
    against the oracle either way."""
    with S.options({Opt.CONVDIFF_SHARED_FLUX: 1 if shared else 0}):   # (Float32 runs 64x8 + 64x4 tiles, Float64 64x4: both tile kernels are covered)
        u = rnd(Ng + (3,), T, 8)
        r, Phi = O.zeros(Ng + (3,), T), O.zeros(Ng, T)
        O.conv_diff(r, u, Phi, nu=0.03)
        ud, rd = field(u, 3), field(rnd(Ng + (3,), T, 9), 3)
        Pd = field(O.zeros(Ng, T), 3)
        S.conv_diff(rd, ud, Pd, nu=0.03)
        same(rd, r)
        shell = np.ones(Ng, bool)
        shell[O.inside(Phi)] = False
        assert np.array_equal(S.to_host(Pd)[shell], Phi[shell])          # the flux scratch left in Phi's ghost cells


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", SHAPES + [(18, 12, 10), (70, 9, 11)])     # (x extents that take the 16-B vector kernels too)
def test_accelerate_bdim_scale_div_cfl(T, Ng):
    D = len(Ng)
    a_o = O.Flow(tuple(n - 2 for n in Ng), (1.0,) + (0.0,) * (D - 1), T=T, nu=0.01)
    a_h = S.Flow(tuple(n - 2 for n in Ng), (1.0,) + (0.0,) * (D - 1), T=T, nu=0.01)
    for k, seed in zip(("u", "u0", "f", "V", "mu0", "mu1"), range(10, 16)):
        h = rnd(getattr(a_o, k).shape, T, seed)
        getattr(a_o, k)[...] = h
        S.upload(getattr(a_h, k), h)
    acc = (0.3, -0.2, 0.1)[:D]
    O.accelerate(a_o.f, acc)
    S.accelerate(a_h.f, acc)
    same(a_h.f, a_o.f)
    O.BDIM(a_o)
    S.BDIM(a_h)
    same(a_h.f, a_o.f)
    same(a_h.u, a_o.u)
    O._fn("wlo_scale_u", T)(O._p(a_o.u), O.C.byref(a_o.grid), 0.5)
    S.scale_u(a_h, 0.5)
    same(a_h.u, a_o.u)
    z = O.zeros(Ng, T)
    O._fn("wlo_div", T)(O._p(z), O._p(a_o.u), O.C.byref(a_o.grid))
    zd = S.like(a_h.p)
    S.divergence(zd, a_h.u)
    same(zd, z)
    a_o.sigma[...] = 0   # no stale ghost scratch: the HIP CFL takes the max over inside(sigma)
    assert O.CFL(a_o) == S.CFL(a_h)
    assert np.array_equal(S.to_host(a_h.sigma)[O.inside(z)], a_o.sigma[O.inside(z)])


# ----------------------------------------------------------------------------- Poisson.jl / MultiLevelPoisson.jl

def make_pois(Ng, T, cls_o, cls_h, perdir=(), padded=True, seed=20):
    D = len(Ng)
    L = rnd(Ng + (D,), T, seed, 0.2, 1.0)
    O.BC(L, (0.0,) * D, False, perdir)
    x, z = rnd(Ng, T, seed + 1), rnd(Ng, T, seed + 2)
    z -= z[O.inside(z)].mean().astype(T)
    xo, Lo, zo = x.copy(order="F"), L.copy(order="F"), z.copy(order="F")
    po = cls_o(xo, Lo, zo, perdir=perdir)
    xd, Ld, zd = field(x, D, padded), field(L, D, padded), field(z, D, padded)
    ph = cls_h(xd, Ld, zd, perdir=perdir)
    return po, ph


def lev_o(po):
    return po.levels[0] if isinstance(po, O.MultiLevelPoisson) else po


def lev_h(ph):
    return ph.levels[0]


@pytest.fixture
def rows_option(request):
    """Opt.STENCIL7_ROWS = the test's `rows` parameter while the test runs"""
    with S.options({Opt.STENCIL7_ROWS: request.node.callspec.params["rows"]}):
        yield


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(18, 18), (18, 18, 18)])
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("rows", [0, 2])
def test_poisson_operators(T, Ng, padded, rows, rows_option):
    """rows: Opt.STENCIL7_ROWS: 0 = default tiling of the 7-point kernel, 2 = two rows per thread forced (3-D only)"""
    if rows and len(Ng) == 2:
        pytest.skip("rows per thread only exists in the 3-D vector kernel")
    po, ph = make_pois(Ng, T, O.MultiLevelPoisson, S.MultiLevelPoisson, padded=padded)
    assert len(po.levels) == len(ph.levels)
    for lo, lh in zip(po.levels, ph.levels):            # set_diag!, restrictL!: bit-exact on every level
        same(lh.L, lo.L)
        same(lh.D, lo.D)
        same(lh.iD, lo.iD)
    xt = rnd(Ng, T, 30)
    xd = field(xt, len(Ng), padded)
    O.mult(po, xt)
    S.mult(ph, xd)
    same(ph.z, po.z)
    # residual!: mean shift through a reduction
    po.z[...] = rnd(Ng, T, 31)
    S.upload(ph.z, po.z)
    O.residual(po)
    S.residual(ph)
    same(lev_h(ph).r, lev_o(po).r, exact=False, tol=4 * np.finfo(T).eps)
    S.upload(lev_h(ph).r, lev_o(po).r)                 # re-synchronise, then the pointwise operators are exact
    O.Jacobi(po)
    S.Jacobi(ph)
    same(lev_h(ph).eps, lev_o(po).eps)
    same(lev_h(ph).r, lev_o(po).r)
    same(ph.x, po.x)
    # restrict! / prolongate! between level 1 and 2
    O.restrict(po.levels[1].r, po.levels[0].r)
    S.restrict(ph.levels[1].r, ph.levels[0].r)
    same(ph.levels[1].r, po.levels[1].r)
    po.levels[1].x[...] = rnd(po.levels[1].x.shape, T, 32)
    S.upload(ph.levels[1].x, po.levels[1].x)
    O.prolongate(po.levels[0].eps, po.levels[1].x)
    S.prolongate(ph.levels[0].eps, ph.levels[1].x)
    same(lev_h(ph).eps, lev_o(po).eps)
    O.increment(po)
    S.increment(ph)
    same(lev_h(ph).r, lev_o(po).r)
    same(ph.x, po.x)
    assert abs(S.L2p(ph) - O.L2p(po)) <= max(4 * np.finfo(T).eps, 1e-13) * O.L2p(po)   # f64: summation order


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("Ng", [(34, 18), (18, 18, 10), (34, 34, 18)])
@pytest.mark.parametrize("rows", [0, 2])
def test_pcg_vcycle_solver(T, Ng, rows, rows_option):
    if rows and len(Ng) == 2:
        pytest.skip("rows per thread only exists in the 3-D vector kernel")
    po, ph = make_pois(Ng, T, O.MultiLevelPoisson, S.MultiLevelPoisson)
    z0 = po.z.copy(order="F")
    O.residual(po)
    S.residual(ph)
    n_o, n_h = O.pcg(po), S.pcg(ph)
    assert n_o == n_h
    same(lev_h(ph).r, lev_o(po).r, exact=False, tol=rtol(T))
    same(ph.x, po.x, exact=False, tol=rtol(T))
    O.Vcycle(po)
    S.Vcycle(ph)
    same(lev_h(ph).r, lev_o(po).r, exact=False, tol=rtol(T))
    same(ph.x, po.x, exact=False, tol=rtol(T))
    # z is pcg!'s scratch: the reference leaves A*eps in it, the HIP path (which never stores A*eps)
    # leaves it alone; a solve starts from a source term the caller has set
    po.z[...] = z0
    S.upload(ph.z, z0)
    O.solver(po)
    S.solver(ph)
    assert po.n == ph.n
    same(ph.x, po.x, exact=False, tol=10 * rtol(T))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("xdefer", [1, 0])
def test_pcg_exit_right_after_update(T, padded, xdefer):
    """pcg! leaving through Poisson.jl:138 (|rho2| < 10eps straight after an update).  The x update of that iteration
    still has to land: the default kernels apply it in the direction kernel (Opt.PCG_DEFER_X), which must run for
    exactly that owed update and nothing else.  Fully periodic unit-coefficient system, plane-wave residual: the
    Jacobi-preconditioned direction is an eigenvector, so one iteration solves it."""
    Ng, D = (18, 18, 18), 3
    perdir = (0, 1, 2)
    L = np.ones(Ng + (D,), T, order="F")
    O.BC(L, (0.0,) * D, False, perdir)
    i = np.arange(Ng[0], dtype=np.float64)
    wave = np.cos(2 * np.pi * (i - 1) / (Ng[0] - 2))
    r = np.asfortranarray(np.broadcast_to(wave[:, None, None], Ng).astype(T))
    x = rnd(Ng, T, 77)
    z = O.zeros(Ng, T)
    po = O.Poisson(x.copy(order="F"), L.copy(order="F"), z.copy(order="F"), perdir=perdir)
    ph = S.Poisson(field(x, D, padded), field(L, D, padded), field(z, D, padded), perdir=perdir)
    po.r[...] = r
    S.upload(lev_h(ph).r, r)
    with S.options({Opt.PCG_DEFER_X: xdefer}):
        n_o, n_h = O.pcg(po), S.pcg(ph)
    assert n_o == n_h == 1                              # one (x,r) update, then the :138 return
    ins = O.inside(x)
    assert np.abs(po.x[ins] - x[ins]).max() > 0.1       # and x really moved
    same(ph.x, po.x, exact=False, tol=rtol(T))
    same(lev_h(ph).r, lev_o(po).r, exact=False, tol=rtol(T))


def _blob_system(T, cls_o, cls_h, padded=True):
    """Unit coefficients (as away from a body) with a block of random ones in the middle: most x-rows are
    coefficient-uniform (the kernels skip the loads of L there), the rows through the block are not."""
    Ng, D = (34, 34, 34), 3
    L = np.ones(Ng + (D,), T, order="F")
    L[:, 12:19, 14:22, :] = rnd((34, 7, 8, D), T, 41, 0.2, 1.0)
    L[9:21, 5:8, 25:28, 0] = T(0.5)                     # x faces only, strictly inside a row
    O.BC(L, (0.0,) * D, False, ())
    x, z = rnd(Ng, T, 42), rnd(Ng, T, 43)
    z -= z[O.inside(z)].mean().astype(T)
    po = cls_o(x.copy(order="F"), L.copy(order="F"), z.copy(order="F"))
    ph = cls_h(field(x, D, padded), field(L, D, padded), field(z, D, padded))
    return po, ph, x


@pytest.mark.parametrize("T", TYPES)
def test_uniform_rows_are_skipped_exactly(T):
    """Opt.ROW_CONST_L: rows whose face coefficients are all one number use that number instead of loading L.
    Same values => every operator is bit-identical with the switch on and off, and mult! stays bit-exact
    against the oracle on every level (c = 1, 2, 4 ... down the hierarchy)."""
    po, ph, x = _blob_system(T, O.MultiLevelPoisson, S.MultiLevelPoisson)
    nu, nr = S.uniform_rows(ph, 0)
    assert nr == 32 * 32 and 0.5 * nr < nu < nr          # the block's rows and the rows next to domain faces are not uniform
    nu1, nr1 = S.uniform_rows(ph, 1)
    assert nr1 == 16 * 16 and 0 < nu1 < nr1
    assert float(S.to_host(ph.levels[1].L)[4, 3, 3, 1]) == 2.0   # restrictL!: 0.5*(1+1+1+1)
    for lo, lh in zip(po.levels, ph.levels):
        same(lh.L, lo.L)
        same(lh.iD, lo.iD)
    xd = field(x, 3, True)
    O.mult(po, x)
    S.mult(ph, xd)
    same(ph.z, po.z)
    # the whole solver, switch on vs off, on twin systems
    _, ph0, _ = _blob_system(T, O.MultiLevelPoisson, S.MultiLevelPoisson)
    with S.options({Opt.ROW_CONST_L: 0}):
        S.mult(ph0, field(x, 3, True))                   # same source term z = A x as the twin above
        assert np.array_equal(S.to_host(ph0.z), S.to_host(ph.z))
        S.solver(ph0)
    S.solver(ph)
    O.solver(po)
    assert ph.n == ph0.n == po.n
    assert np.array_equal(S.to_host(ph.x), S.to_host(ph0.x))
    assert np.array_equal(S.to_host(lev_h(ph).r), S.to_host(lev_h(ph0).r))
    same(ph.x, po.x, exact=False, tol=10 * rtol(T))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims", [(64, 32), (192, 64), (32, 32, 32), (64, 48, 16)])
def test_coarse_tail_on_chip_bit_exact(T, dims):
    """Opt.COARSE_PCG_RESIDENT: inside the one-workgroup bottom of the V-cycle pcg! keeps its level in registers + LDS instead of
    going through global memory between its phases.  Same expressions, same order of every sum: every field after several
    steps (and every coarse level's x, r, eps, z after a V-cycle) is bit-identical with the switch on and off; levels of
    1 and of 4 cells per thread, 2-D and 3-D."""
    m = dims[1]
    R, c = m / 8, m / 2 - 1
    ubc = (1.0,) + (0.0,) * (len(dims) - 1)
    runs = []
    for on in (1, 0):
        with S.options({Opt.COARSE_PCG_RESIDENT: on}):
            from waterlily_amd import body as B
            s = S.Simulation(dims, ubc, 2 * R, nu=2 * R / 250, body=B.Sphere(c, R, len(dims)), T=T)
            for _ in range(4):
                S.sim_step(s, remeasure=False)
        runs.append(s)
    a, b = runs
    assert a.pois.n == b.pois.n
    assert torch.equal(a.flow.u, b.flow.u) and torch.equal(a.flow.p, b.flow.p)
    for la, lb in zip(a.pois.levels[1:], b.pois.levels[1:]):
        for k in ("x", "r", "eps", "z"):
            assert torch.equal(getattr(la, k), getattr(lb, k)), k


@pytest.mark.parametrize("T", TYPES)
def test_pcg_without_stored_z_bit_exact(T):
    """Opt.PCG_RECOMPUTE_AEPS: pcg!'s update kernel forms z = A*eps a second time (7-point kernel over eps) instead of reading
    the z the mult kernel stored.  Same expression on the same operands => x and r after the whole solver are
    bit-identical to the run that stores z; both match the oracle."""
    res = []
    for on in (2, 0):
        with S.options({Opt.PCG_RECOMPUTE_AEPS: on}):
            po, ph, _ = _blob_system(T, O.MultiLevelPoisson, S.MultiLevelPoisson)
            S.solver(ph)
        res.append(ph)
    O.solver(po)
    assert res[0].n == res[1].n == po.n
    assert np.array_equal(S.to_host(res[0].x), S.to_host(res[1].x))
    assert np.array_equal(S.to_host(lev_h(res[0]).r), S.to_host(lev_h(res[1]).r))
    same(res[0].x, po.x, exact=False, tol=10 * rtol(T))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
def test_pcg_every_kernel_choice(T, padded):
    """One pcg! call (after residual!) on the blob system -- 34^3, uniform rows and rows through the block -- under every
    combination of the switches that decide which of op_pcg's kernels run and how its dot products are finished:
    PCG_VEC (16-B vector / scalar range kernels), PCG_DEFER_X (x += alpha*eps in the update / direction kernel),
    PCG_RECOMPUTE_PRECOND (z' = r*iD stored / recomputed), PCG_RECOMPUTE_AEPS (update reads z / is a second 7-point kernel),
    PCG_DOTS_IN_KERNEL (finalize launches / in-kernel gates).  Every combination: the oracle's update count, x and r within
    the tolerance of test_pcg_vcycle_solver.
    Bit for bit (x, r, eps) against the run with no switch set: every combination that differs from the defaults only in
    PCG_DEFER_X, PCG_RECOMPUTE_PRECOND or PCG_RECOMPUTE_AEPS (at this size the defaults behave as PCG_VEC = 2,
    PCG_RECOMPUTE_AEPS = 0, PCG_DOTS_IN_KERNEL = 2): same expressions on the same operands, and at 34^3 every reducing kernel
    cuts the level into the same 8 x 32 workgroups, so the sums are grouped alike.  Beyond those, PCG_DOTS_IN_KERNEL = 0 is
    asserted bit for bit as well (all 16 combinations with PCG_VEC = 2): the finalize launch and the in-kernel gate sum the
    same partials in the same order and apply the same scalar steps.  PCG_VEC = 0 (one partial per 256 cells in index order,
    another grouping of every sum) is compared to the tolerance only."""
    keys = (Opt.PCG_VEC, Opt.PCG_DEFER_X, Opt.PCG_RECOMPUTE_PRECOND, Opt.PCG_RECOMPUTE_AEPS, Opt.PCG_DOTS_IN_KERNEL)
    on = (2, 1, 1, 2, 2)

    def run(values):
        with S.options(values):
            po, ph, _ = _blob_system(T, O.MultiLevelPoisson, S.MultiLevelPoisson, padded)
            S.residual(ph)
            n = S.pcg(ph)
        return po, ph, n, [S.to_host(a) for a in (ph.x, lev_h(ph).r, lev_h(ph).eps)]

    po, _, n_def, base = run({})
    O.residual(po)
    n_o = O.pcg(po)
    assert n_def == n_o == 6
    failures = []
    for combo in itertools.product(*[(v, 0) for v in on]):
        _, ph, n, got = run(dict(zip(keys, combo)))
        bits = all(np.array_equal(a, b) for a, b in zip(got, base))
        scale = [max(1e-30, float(np.max(np.abs(h)))) for h in (po.x, lev_o(po).r)]
        err = [float(np.max(np.abs(g.astype(np.float64) - h.astype(np.float64)))) / s for g, h, s in zip(got, (po.x, lev_o(po).r), scale)]
        print(f"{np.dtype(T).name} padded={padded} {dict(zip((k.name for k in keys), combo))}: n={n} bit-equal={bits} "
              f"err x={err[0]:.2e} r={err[1]:.2e}")
        if n != n_o or max(err) > rtol(T):
            failures.append((combo, "oracle", n, err))
        if combo[0] == 2 and not bits:
            failures.append((combo, "bits differ from the default run"))
    assert not failures, failures


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("rows", [1, 2])
def test_rows_per_thread_variants(T, rows):
    """Opt.STENCIL7_ROWS = R: the 7-point kernel with R = 1 or 2 rows per thread (the default picks by level size).  Same
    per-cell expressions => same bits as the default form, on a system with coefficient-uniform rows and body rows."""
    with S.options({Opt.STENCIL7_ROWS: rows}):
        _, ph1, x = _blob_system(T, O.MultiLevelPoisson, S.MultiLevelPoisson)
        S.solver(ph1)
    po, ph2, _ = _blob_system(T, O.MultiLevelPoisson, S.MultiLevelPoisson)
    S.solver(ph2)
    O.solver(po)
    assert ph1.n == ph2.n == po.n
    same(ph1.x, S.to_host(ph2.x), exact=False, tol=10 * rtol(T))     # (reduction partials are grouped differently: a few ulp)
    same(ph1.x, po.x, exact=False, tol=10 * rtol(T))


@pytest.mark.parametrize("T", TYPES)
def test_single_level_poisson_solver(T):
    po, ph = make_pois((18, 18), T, O.Poisson, S.Poisson)
    O.solver(po)
    S.solver(ph)
    assert po.n == ph.n
    same(ph.x, po.x, exact=False, tol=100 * rtol(T))


# ----------------------------------------------------------------------------- whole time steps

def geom_tol(T):
    """product geometry (torch autograd, Float64) vs oracle geometry (closed-form derivatives, Float64), both rounded to
    T: Float32 fields agree to the ulp (the Float64 discrepancy almost never crosses a Float32 rounding boundary);
    Float64 fields show the last-bits difference of the two derivative evaluations and of sin/cos (libm vs torch)"""
    return 4 * np.finfo(np.float32).eps if np.dtype(T) == np.float32 else 32 * np.finfo(np.float64).eps


def pair(dims, u_BC, L, body=None, geometry="host", **kw):
    """The same case on the oracle and on the HIP path.  `body` is a bodies.Twin: the oracle measures its closed-form
    side with oracle/geometry.py, the product its closure side with waterlily_amd.body (geometry = "host" or
    "device") -- no coefficient field of the oracle comes from product code."""
    hip_only = {k: kw.pop(k) for k in ("padded",) if k in kw}
    so = O.Simulation(dims, u_BC, L, body=None if body is None else body.oracle, **kw)
    sh = S.Simulation(dims, u_BC, L, body=None if body is None else body.product, geometry=geometry, **kw, **hip_only)
    # the two measurements agree to rounding (autograd vs analytic derivatives: last bits of the Float64 evaluation)
    eps = geom_tol(so.flow.T)
    for k in ("mu0", "mu1", "V"):
        assert np.allclose(S.to_host(getattr(sh.flow, k)), getattr(so.flow, k), rtol=0, atol=eps), k
    assert np.allclose(S.to_host(sh.flow.u), so.flow.u, rtol=0, atol=eps)
    return so, sh


def check_step(so, sh, T, nsteps, utol=None):
    utol = rtol(T) * 50 if utol is None else utol
    for _ in range(nsteps):
        O.sim_step(so, remeasure=False)
        S.sim_step(sh, remeasure=False)
    assert so.pois.n == sh.pois.n, (so.pois.n, sh.pois.n)
    assert np.allclose(so.flow.dt, sh.flow.dt, rtol=rtol(T) * 10, atol=0)
    same(sh.flow.u, so.flow.u, exact=False, tol=utol)
    same(sh.flow.p, so.flow.p, exact=False, tol=utol * 10)


@pytest.mark.parametrize("T", TYPES)
def test_mom_step_2d_circle(T):
    """BASELINE config C1 shape family: 2-D circle, Re=100 (64x32 here)."""
    n, m = 64, 32
    R, c = m / 8, m / 2 - 1
    so, sh = pair((n, m), (1.0, 0.0), 2 * R, nu=2 * R / 100, body=bodies.sphere(c, R), T=T)
    check_step(so, sh, T, 5)
    fo, fh = O.pressure_force(so), S.pressure_force(sh)
    assert np.allclose(fo, fh, rtol=1e-4 if T == np.float32 else 1e-9, atol=1e-6 if T == np.float32 else 1e-12)


@pytest.mark.parametrize("T", TYPES)
def test_mom_step_3d_sphere(T):
    """BASELINE configs C2/C3 shape family: 3-D sphere, Re=3700, Float32/Float64 (32^3 here)."""
    m = 32
    R, c = m / 8, m / 2 - 1
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R), T=T)
    check_step(so, sh, T, 3)
    fo, fh = O.pressure_force(so), S.pressure_force(sh)
    assert np.allclose(fo, fh, rtol=1e-4 if T == np.float32 else 1e-9, atol=1e-6 if T == np.float32 else 1e-12)


@pytest.mark.parametrize("T", TYPES)
def test_project_div_inside_residual_bit_exact(T):
    """Opt.DIV_IN_RESIDUAL: inside mom_step! the right-hand side z = div(u) of project! is formed by the residual! kernel
    itself (no z array pass).  Same differences in the same order => every field after several steps is bit-identical
    to the run with the separate div pass, which in turn matches the oracle."""
    m = 48
    R, c = m / 8, m / 2 - 1
    runs = []
    for fused in (1, 0):
        with S.options({Opt.DIV_IN_RESIDUAL: fused}):
            so, sh = pair((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R), T=T)
            for _ in range(3):
                S.sim_step(sh, remeasure=False)
            runs.append((sh.pois.n[:], S.to_host(sh.flow.u).copy(), S.to_host(sh.flow.p).copy(), list(sh.flow.dt)))
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    assert runs[0][3] == runs[1][3]
    for _ in range(3):
        O.sim_step(so, remeasure=False)
    assert so.pois.n == runs[0][0]
    assert np.max(np.abs(runs[0][1].astype(np.float64) - so.flow.u)) <= rtol(T) * 50 * float(np.max(np.abs(so.flow.u)))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("case", ["sphere", "sphere-on-the-wall", "moving", "gravity", "dense"])
def test_bdim_finished_inside_conv_diff_bit_exact(T, case):
    """Opt.BDIM_IN_CONVDIFF: inside mom_step! the conv_diff! kernels finish BDIM! (Flow.jl:134, scale_u! :166) on the body-free
    x-rows themselves -- the new velocity of such a row is stored from the registers that hold f, V is not read there, the
    row's x-ghost cells of the following BC! are written too -- and the two velocity arrays take turns (the predictor writes
    u' into the u0 array, the corrector the new velocity back into u), the busy rows keep their own kernel.  Same expressions
    in the same order => u (ghost cells included), p, f, the time steps and the V-cycle counts after several steps are
    bit-identical to the run with the separate BDIM! pass, which matches the oracle.  Cases: several x tiles per row; a body
    cut by the domain wall (busy rows in the shell kernel's tile rows and planes); a moving body (V != 0 in the busy rows);
    a body force (accelerate!); the reference's dense strides."""
    dims = (136, 40, 24) if case != "dense" else (48, 40, 24)
    R, c = dims[1] / 8, dims[1] / 2 - 1
    kw = dict(T=T)
    body = bodies.sphere(c, R)
    if case == "sphere-on-the-wall":
        body = bodies.sphere((c, 1.5, dims[2] - 2.5), R)
    elif case == "moving":
        body = bodies.moving_circle(dims[2] / 2 - 1.0, R, v=0.4, D=3)
    elif case == "gravity":
        kw["g"] = lambda i, t: 0.05 * (i + 1) * (1 + t)
    elif case == "dense":
        kw["padded"] = False
    runs = []
    for fused in (1, 0):
        with S.options({Opt.BDIM_IN_CONVDIFF: fused}):
            so, sh = pair(dims, (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 1000, body=body, **kw)
            u_start = S.to_host(sh.flow.u).copy()
            for _ in range(3):
                u_before = S.to_host(sh.flow.u).copy()
                S.sim_step(sh, remeasure=(case == "moving"))
            runs.append((sh.pois.n[:], list(sh.flow.dt), S.to_host(sh.flow.u).copy(), S.to_host(sh.flow.p).copy(), S.to_host(sh.flow.f).copy(),
                         S.to_host(sh.flow.u0).copy(), u_before))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1]
    for q in (2, 3, 4):
        assert np.array_equal(a[q], b[q]), q
    # the one visible difference: the u0 ARRAY.  Separate pass: the velocity the step started from
    # (Flow.jl:154); fused: the predictor's velocity u' -- the reference overwrites u0 before it ever reads it
    assert np.array_equal(b[5], b[6]) and not np.array_equal(a[5], a[6])
    for _ in range(3):
        O.sim_step(so, remeasure=(case == "moving"))
    assert so.pois.n == a[0]
    assert np.max(np.abs(a[2].astype(np.float64) - so.flow.u)) <= rtol(T) * 50 * float(np.max(np.abs(so.flow.u)))


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("exitBC", [False, True])
def test_x_ghost_cells_written_by_the_producer_bit_exact(T, exitBC):
    """Opt.XGHOST_IN_KERNEL: inside mom_step! the x-ghost cells of the interior rows that BC!(u,U) sets are written by the
    kernel that produces the row (BDIM!, the velocity correction), the BC launch covers the y / z planes only.  Every
    element of u -- ghost cells included -- after several steps is bit-identical to the run whose BC! writes all six
    planes, and matches the oracle."""
    dims = (264, 24, 16)           # several x tiles per row (256 / 128 cells per wavefront for Float32 / Float64)
    R, c = dims[1] / 8, dims[1] / 2 - 1
    runs = []
    for fold in (1, 0):
        with S.options({Opt.XGHOST_IN_KERNEL: fold}):
            so, sh = pair(dims, (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 1000, body=bodies.sphere(c, R), T=T, exitBC=exitBC)
            for _ in range(3):
                S.sim_step(sh, remeasure=False)
            runs.append((sh.pois.n[:], S.to_host(sh.flow.u).copy(), S.to_host(sh.flow.p).copy(), list(sh.flow.dt)))
    assert runs[0][0] == runs[1][0] and runs[0][3] == runs[1][3]
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    for _ in range(3):
        O.sim_step(so, remeasure=False)
    assert so.pois.n == runs[0][0]
    assert np.max(np.abs(runs[0][1].astype(np.float64) - so.flow.u)) <= rtol(T) * 50 * float(np.max(np.abs(so.flow.u)))


def test_c1_full_size_2d_circle_f64():
    """BASELINE configs[0] (C1) at its real size: 2-D circle, 192x64, Re=100, Float64 -- 12 steps against the oracle:
    identical V-cycle counts and time steps, u to 1e-10, p to 1e-9, pressure force to 1e-8 (the solver stops at an
    absolute residual, so Float64 steps agree far below the 1e-6 of SURVEY 8c's protocol)."""
    n, m = 192, 64
    R, c = m / 8, m / 2 - 1
    so, sh = pair((n, m), (1.0, 0.0), 2 * R, nu=2 * R / 100, body=bodies.sphere(c, R), T=np.float64)
    assert len(sh.pois.levels) == 6                            # 192x64 -> 6x2 (C1 has 6 levels)
    check_step(so, sh, np.float64, 12, utol=1e-10)
    assert np.allclose(O.pressure_force(so), S.pressure_force(sh), rtol=1e-8, atol=1e-11)


@pytest.mark.parametrize("geometry", ["host", "device"])
def test_sphere_96_f32(geometry):
    """The C2/C3 case (3-D sphere, Re=3700, Float32) at 96^3 -- the largest size the CPU oracle steps in seconds: 3 steps,
    identical V-cycle counts, u within 5e-4, pressure force within 1e-3; with the product's own measure! on the host
    and on the device."""
    m = 96
    R, c = m / 8, m / 2 - 1
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R), T=np.float32, geometry=geometry)
    check_step(so, sh, np.float32, 3)
    fo, fh = O.pressure_force(so), S.pressure_force(sh)
    assert np.allclose(fo, fh, rtol=1e-3, atol=1e-4)


@pytest.mark.skipif(os.environ.get("WL_SKIP_512") == "1", reason="WL_SKIP_512=1")
def test_c3_full_size_512_f32_against_the_oracle():
    """BASELINE config C3 itself -- the 512^3 Float32 sphere the bench line is quoted on -- stepped by the CPU oracle (half a
    minute per step on the box's 16 cores: ONE full step here -- predictor, corrector, both solves, CFL; rounds 2-3 ran two, the
    twelve steps of C2 below and the 60-step record of tests/checks/longparity.py cover the sequence) and by the HIP path:
    identical V-cycle counts, dt within 1e-4, u within 5e-4 and p within 5e-3 of their maxima.  The size-independent properties of tests/test_fullsize_properties.py hold the
    kernels to account at this size bit for bit; this is the direct comparison."""
    m = 512
    R, c = m / 8, m / 2 - 1
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R), T=np.float32, geometry="device")
    check_step(so, sh, np.float32, 1)


def test_c2_full_size_256_f32_twelve_steps_against_the_oracle():
    """BASELINE config C2 itself (256^3 Float32 sphere, Re=3700; the CPU-baseline case of bench.py) over twelve steps:
    identical V-cycle counts in every solve, time steps, u, p and the pressure force.  (tests/checks/longparity.py runs the same pair
    for 60 steps: bitwise equal fields throughout, profiles/r03c_longparity_c2_256_f32_60steps.txt.)"""
    m = 256
    R, c = m / 8, m / 2 - 1
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R), T=np.float32, geometry="device")
    check_step(so, sh, np.float32, 12)
    assert np.allclose(O.pressure_force(so), S.pressure_force(sh), rtol=1e-4, atol=1e-4)


def test_c5_256_f64_torus_against_the_oracle():
    """BASELINE config C5's case -- torus AutoBody, Float64, Re=1000 -- at 256^3 (the largest 3-D Float64 size the CPU oracle
    steps in seconds): 2 steps, identical V-cycle counts and time steps, u within 1e-10 and p within 1e-9 of their maxima,
    pressure force to 1e-8.  (C5 at its own size, 512^3: tests/test_fullsize_properties.py.)"""
    m = 256
    c, Rm, rm = m / 2, m / 4, m / 16
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), Rm, nu=Rm / 1000, body=bodies.torus(c, Rm, rm), T=np.float64, geometry="device")
    check_step(so, sh, np.float64, 2, utol=1e-10)
    assert np.allclose(O.pressure_force(so), S.pressure_force(sh), rtol=1e-8, atol=1e-9)


def _oracle_moving_cylinder(m, T):
    """the oracle twin of bench.moving_cylinder (closed-form geometry, oracle/geometry.py)"""
    R = m / 16
    body = G.Body(G.Cylinder((m / 4, m / 2, 0.0), R, axes=(0, 1)), G.Translate(v=(1.0, 0.0, 0.0)))
    return O.Simulation((m, m, m), (0.0, 0.0, 0.0), 2 * R, U=1.0, nu=2 * R / 1000, body=body, T=T)


@pytest.mark.parametrize("T", TYPES)
def test_bench_moving_cylinder_case_against_the_oracle(T):
    """`bench.py --body cylinder`: a cylinder through the z walls translating through fluid at rest, measure! + update!
    every step (sim_step!'s default) -- native kernels against the oracle at 64^3: V-cycle counts, time steps, u, p."""
    import bench
    m = 64
    so, sh = _oracle_moving_cylinder(m, T), bench.moving_cylinder((m, m, m), T)
    for _ in range(4):
        O.sim_step(so)
        S.sim_step(sh)
    assert so.pois.n == sh.pois.n, (so.pois.n, sh.pois.n)
    assert np.allclose(so.flow.dt, sh.flow.dt, rtol=rtol(T) * 10, atol=0)
    same(sh.flow.u, so.flow.u, exact=False, tol=rtol(T) * 50)
    same(sh.flow.p, so.flow.p, exact=False, tol=rtol(T) * 500)


SWITCHES = {k: 0 for k in (
    Opt.STENCIL7_VEC, Opt.SMOOTH_FUSED, Opt.CONVDIFF_TILED, Opt.BDIM_ROWFLAGS, Opt.PCG_VEC, Opt.COARSE_TAIL, Opt.BC_FUSED,
    Opt.PCG_DEFER_X, Opt.ROW_CONST_L, Opt.PCG_START_FUSED, Opt.PCG_RECOMPUTE_PRECOND, Opt.SCALE_CHAIN, Opt.PCG_DOTS_IN_KERNEL,
    Opt.CONVDIFF_SHARED_FLUX, Opt.PCG_RECOMPUTE_AEPS, Opt.DIV_IN_RESIDUAL, Opt.XGHOST_IN_KERNEL, Opt.BDIM_IN_CONVDIFF,
    Opt.SWEEP_ALTERNATE, Opt.COARSE_PCG_RESIDENT)}


@pytest.mark.parametrize("group", ["all-at-once", "vector-kernels-kept", "two-rows-and-no-finalize-launches", "x-planes-by-the-BC-launch"])
def test_every_switch_flipped_at_once_changes_no_bit(group):
    """Every wl_set_option key that selects between the reference's form of an operator and a traffic-saving form of it, flipped
    TOGETHER (round 3 tested them one at a time): the default path and the all-reference-forms path -- generic range kernels,
    two-pass smoothers, plane-by-plane BC!, stored z / z', finalize launches, separate div pass, ascending sweeps -- step a 3-D
    sphere case to bitwise identical Float32 fields, time steps and V-cycle counts; two mixed groups cover the combinations in
    between (vector kernels kept with every fusion off; two rows per thread with in-kernel dot products on every level)."""
    m = 48
    R, c = m / 8, m / 2 - 1
    mk = lambda: S.Simulation((2 * m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R).product, T=np.float32)

    def run():
        sim = mk()
        for _ in range(3):
            S.sim_step(sim, remeasure=False)
        return sim
    base = run()
    flips = dict(SWITCHES)
    if group == "vector-kernels-kept":
        for k in (Opt.STENCIL7_VEC, Opt.CONVDIFF_TILED, Opt.PCG_VEC):
            flips.pop(k)
    elif group == "two-rows-and-no-finalize-launches":
        flips = {Opt.STENCIL7_ROWS: 2, Opt.PCG_DOTS_IN_KERNEL: 2, Opt.PCG_RECOMPUTE_AEPS: 2, Opt.SWEEP_ALTERNATE: 0, Opt.BDIM_ROWFLAGS: 0,
                 Opt.ROW_CONST_L: 0}
    elif group == "x-planes-by-the-BC-launch":       # BDIM! still finished inside conv_diff!, the x-ghost cells by BC!'s own launch
        flips = {Opt.XGHOST_IN_KERNEL: 0}
    with S.options(flips):
        other = run()
    assert base.pois.n == other.pois.n and base.flow.dt == other.flow.dt
    assert torch.equal(base.flow.u, other.flow.u) and torch.equal(base.flow.p, other.flow.p)
    assert torch.equal(base.flow.f, other.flow.f)


def test_steady_step_allocates_nothing_and_keeps_the_host_light():
    """The reference bounds the heap traffic of a time step (test/alloctest.jl:17-27: `mom_step!` allocates < 50 kB).  Here a
    steady `sim_step!(remeasure=false)` performs NO allocation at all -- neither in the library (wl_prof_allocs counts its
    hipMalloc / hipHostMalloc calls) nor through torch's allocator -- and the whole step (about 270 dependent launches, two
    host synchronisations per solve iteration and one for CFL) stays within a few milliseconds of wall time on a small grid."""
    import ctypes as C
    import time
    from waterlily_amd import _lib
    L = _lib.lib()
    m = 64
    R, c = m / 8, m / 2 - 1
    sh = S.Simulation((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 3700, body=bodies.sphere(c, R).product, T=np.float32)
    for _ in range(4):
        S.sim_step(sh, remeasure=False)
    torch.cuda.synchronize()

    def counters():
        n, b = C.c_int64(), C.c_int64()
        _lib.check(L.wl_prof_allocs(C.byref(n), C.byref(b)))
        st = torch.cuda.memory_stats()
        return n.value, b.value, st["allocation.all.allocated"], st["segment.all.allocated"]
    before = counters()
    t0 = time.perf_counter()
    for _ in range(10):
        S.sim_step(sh, remeasure=False)
    torch.cuda.synchronize()
    per_step = (time.perf_counter() - t0) / 10
    assert counters() == before, (before, counters())
    assert per_step < 5e-3, per_step          # measured: 0.7 ms per 64^3 step
    # a moving parametric body re-measured every step may size its band buffers once, then runs allocation-free in the library too
    from waterlily_amd import body as B
    mv = S.Simulation((m, m, m), (0.0, 0.0, 0.0), 2 * R, U=1.0, nu=2 * R / 1000, T=np.float64,
                      body=B.Sphere((m / 4, c, c), R, 3, map=B.translation(3, v=(1.0, 0.0, 0.0))))
    for _ in range(4):
        S.sim_step(mv)
    n0 = counters()[:2]
    for _ in range(6):
        S.sim_step(mv)
    assert counters()[:2] == n0


def test_float32_solver_stall_on_the_moving_cylinder_follows_the_oracle():
    """from 256^3 the C restatement of the reference's Float32 solver (oracle/; NOT verified on
    WaterLily.jl itself, whose BLAS Float32 dots and @fastmath may behave differently) cannot bring r.r below tol = 1e-4 on this
    case -- cells frozen by set_diag! (D^2 < 2 eps(T), Poisson.jl:44) keep the residual L*d(eps) their neighbours leave on them.
    The HIP path must stall exactly where the oracle does: the V-cycle counts of the first two steps at 256^3 Float32 are
    those the CPU oracle takes ([3, 2] then [32, 32], recorded in profiles/r03c_cylinder_vcycles.txt; the oracle needs a
    minute for them, so they are pinned here as numbers), with the solver log showing the floor; Float64 converges."""
    import bench
    m = 256
    sh = bench.moving_cylinder((m, m, m), np.float32)
    S.sim_step(sh)
    S.solver_log(sh.pois, True)
    S.sim_step(sh)
    rows = S.read_solver_log(sh.pois)
    S.solver_log(sh.pois, False)
    assert sh.pois.n == [3, 2, 32, 32], sh.pois.n
    first = rows[:33]                                   # n = 0 .. 32 of the predictor's solve
    assert first[0, 0] == 0 and first[4, 0] == 4
    assert 1e-4 < first[4:15, 2].min() and first[4:15, 2].max() < 2e-3     # parked on the floor, above tol
    del sh
    sd = bench.moving_cylinder((m, m, m), np.float64)
    for _ in range(2):
        S.sim_step(sd)
    assert sd.pois.n == [3, 2, 4, 2], sd.pois.n


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims", [(48, 32), (32, 32, 32)])
def test_mom_step_dense_julia_layout(T, dims):
    """The reference's dense column-major layout (row pitch N+2: what a Julia shim passes): rows are
    not 16-B aligned, so the library must take its scalar range kernels -- and the flat x*=dt stream its unaligned
    head/tail -- and still reproduce the oracle."""
    m = dims[1]
    R, c = m / 8, m / 2 - 1
    kw = dict(nu=2 * R / 250, body=bodies.sphere(c, R), T=T)
    ubc = (1.0,) + (0.0,) * (len(dims) - 1)
    so, sh = pair(dims, ubc, 2 * R, padded=False, **kw)
    assert sh.flow.u.stride()[1] == dims[0] + 2                       # really dense
    check_step(so, sh, T, 3)


def test_mom_step_3d_donut_f64():
    """BASELINE config C5 shape family: torus AutoBody, Float64."""
    m = 32
    c, Rm, rm = m / 2, m / 4, m / 16
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), Rm, nu=Rm / 1000, body=bodies.torus(c, Rm, rm), T=np.float64)
    check_step(so, sh, np.float64, 3)
    assert np.allclose(O.pressure_force(so), S.pressure_force(sh), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("exitBC", [False, True])
def test_mom_step_periodic_exit_accel(exitBC):
    """periodic direction + exitBC + body force + time-varying U (Flow.jl:58-60,68-73; util.jl:216-222) against the FAITHFUL
    oracle: its whole-array z⋅ϵ (Poisson.jl:131, z === flow.σ on level 1) picks up σ's stale flux scratch times ϵ's periodic
    ghost copies, its maximum(a.σ) (Flow.jl:174) sees the ghost cells too -- and so does the HIP path (op_sigma_ghosts + the
    shell terms of pcg! and CFL): tight agreement, identical V-cycle counts."""
    T = np.float64
    kw = dict(nu=0.01, g=lambda i, t: 0.1 * t if i == 0 else 0.0, perdir=(1,), exitBC=exitBC, T=T, U=1.0)
    u_BC = lambda i, t: 1.0 + 0.05 * t if i == 0 else 0.0 * t
    so, sh = pair((32, 32), u_BC, 8.0, body=bodies.sphere(15.0, 4.0), **kw)
    check_step(so, sh, T, 4)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("case", ["2d-xper", "2d-allper", "3d-yzper", "3d-noper", "3d-zper-body"])
def test_sigma_ghost_cells_hold_the_reference_flux_scratch(T, case):
    """After mom_step! the reference's flow.σ holds, in its top ghost cells, the flux scratch Φ of the corrector's
    conv_diff! (Flow.jl:45,59,164; inside_u keeps the top ghost, util.jl:55-57) -- the cells its whole-array maximum(a.σ)
    and z⋅ϵ read.  The HIP path has no Φ; op_sigma_ghosts writes those cells: the WHOLE σ shell must equal the oracle's bit
    for bit (the lower ghost cells stay zero), together with Δt."""
    D = 2 if case.startswith("2d") else 3
    dims = (24, 16) if D == 2 else (16, 16, 8)
    perdir = {"2d-xper": (0,), "2d-allper": (0, 1), "3d-yzper": (1, 2), "3d-noper": (), "3d-zper-body": (2,)}[case]
    body = bodies.sphere(7.0, 3.0) if case in ("3d-noper", "3d-zper-body", "2d-xper") else None
    rng = np.random.default_rng(11)

    def ulam(i, x):
        ph = 2 * np.pi * (x[0] / dims[0] + 2 * x[1] / dims[1] + (x[2] / dims[2] if D == 3 else 0))
        return (1.0 if i == 0 else 0.0) + 0.3 * np.sin(ph + i)
    kw = dict(nu=0.02, perdir=perdir, T=T, U=1.0, ulam=ulam)
    so, sh = pair(dims, (1.0,) + (0.0,) * (D - 1), 6.0, body=body, **kw)
    for _ in range(2):
        O.sim_step(so, remeasure=False)
        S.sim_step(sh, remeasure=False)
    assert so.pois.n == sh.pois.n
    sg_o, sg_h = so.flow.sigma, S.to_host(sh.flow.sigma)
    shell = np.ones(sg_o.shape, bool)
    shell[O.inside(sg_o)] = False
    assert np.any(sg_o[shell] != 0)                       # the scratch really is there ...
    # ... and the same on both sides: to the rounding the two velocity fields agree to (the kernel that writes the cells is
    # pinned bit for bit on identical input in test_conv_diff_bit_exact), zeros where the reference never writes
    assert np.array_equal(sg_h[shell] == 0, sg_o[shell] == 0)
    assert np.max(np.abs(sg_h[shell].astype(np.float64) - sg_o[shell])) <= rtol(T) * 50 * np.max(np.abs(sg_o[shell]))
    assert np.allclose(so.flow.dt, sh.flow.dt, rtol=rtol(T) * 10, atol=0)
    same(sh.flow.u, so.flow.u, exact=False, tol=rtol(T) * 50)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims", [(32, 24), (24, 16, 16)])
@pytest.mark.parametrize("case", ["oblique-inflow", "body-on-the-boundary"])
def test_time_step_follows_the_whole_array_maximum_of_sigma(T, dims, case):
    """CFL = inv(maximum(a.σ) + 5ν) over the WHOLE array (Flow.jl:174), ghost cells with conv_diff!'s flux scratch included.
    oblique-inflow: a uniform stream with a large component along the last axis leaves Φ ~ w² in the ghost cells of the exit
    plane, more than twice the largest interior flux_out ~ |u|+|v|+|w| -- a ghost cell SETS the time step (asserted);
    body-on-the-boundary: a sphere poking through the upper faces (the case DESIGN.md named as the one that separated the two
    sides).  Equal Δt and V-cycle counts step after step, fields to rounding."""
    D = len(dims)
    if case == "oblique-inflow":
        U = (0.5,) + (1.0,) * (D - 2) + (4.0,)
        R = dims[1] / 6
        body = bodies.sphere(dims[1] / 2, R)
    else:
        U = (1.0,) + (0.0,) * (D - 1)
        R = dims[1] / 3
        body = bodies.sphere((dims[0] / 2,) + tuple(n - R / 2 for n in dims[1:]), R)
    so, sh = pair(dims, U, 2 * R, nu=2 * R / 200, body=body, T=T)
    for _ in range(6):
        O.sim_step(so, remeasure=False)
        S.sim_step(sh, remeasure=False)
    assert so.pois.n == sh.pois.n, (so.pois.n, sh.pois.n)
    assert np.allclose(so.flow.dt, sh.flow.dt, rtol=rtol(T) * 10, atol=0), (so.flow.dt, sh.flow.dt)
    same(sh.flow.u, so.flow.u, exact=False, tol=rtol(T) * 50)
    sg, sgh = so.flow.sigma, S.to_host(sh.flow.sigma)
    shell = np.ones(sg.shape, bool)
    shell[O.inside(sg)] = False
    assert np.max(np.abs(sgh[shell].astype(np.float64) - sg[shell])) <= rtol(T) * 50 * np.max(np.abs(sg[shell]))
    if case == "oblique-inflow":
        assert sg.max() > 2 * sg[O.inside(sg)].max()                  # the case does what it claims: a ghost cell is the maximum


@pytest.mark.parametrize("cfg", ["TGV-64^2-f64", "TGV-64^2-f32", "channel-8^2-f64"])
def test_periodic_runs_at_the_reference_sizes_match_the_faithful_oracle(cfg):
    """The reference's own periodic configurations at their sizes -- the Taylor-Green vortex (maintests.jl:232-253: 64^2,
    both directions periodic, to t = pi/100) and the accelerating periodic channel (maintests.jl:280-302: 8^2, x periodic,
    to t = 1) -- against the oracle with its faithful whole-array reductions (rounds 1-3 reduced over inside() only and
    differed by 1.2e-4 in Float32 here, with a V-cycle more or less in some solves): the same number of time steps, the same
    V-cycle count in EVERY solve, fields and time steps as close as ROUNDING lets two runs of this case be -- measured in the
    test itself by a second oracle run started one part in 1e16 away."""
    if cfg.startswith("TGV"):
        T = np.float64 if cfg.endswith("f64") else np.float32
        Lg = 64
        k = 2 * math.pi / Lg
        nu = 1 / (k * 1e8)

        def tgv(i, xy):
            x, y = xy[0] * k, xy[1] * k
            return -np.sin(x) * np.cos(y) if i == 0 else np.cos(x) * np.sin(y)
        kw = dict(U=1, ulam=tgv, nu=nu, T=T, perdir=(0, 1))
        ubc = (0.0, 0.0)
        mk = lambda M: M.Simulation((Lg, Lg), ubc, Lg, **kw)
        t_end = math.pi / 100
    else:
        T = np.float64
        N, jerk = 8, 4
        kw = dict(nu=0.001, g=lambda i, t: t * jerk if i == 0 else 0.0, dt=0.001, perdir=(0,), T=T)
        ubc = (math.sqrt(N), 0.0)
        mk = lambda M: M.Simulation((N, N), ubc, N, **kw)
        t_end = 1.0
    so, sh = mk(O), mk(S)
    # a twin of the oracle run whose initial velocity is perturbed by one part in 1e16: how far ROUNDING ALONE moves this case
    # (the fully periodic vortex has a singular Poisson matrix; from the third step on pcg!'s decisions on the coarse levels
    # amplify a last-bit difference by three orders of magnitude -- measured: 5e-10 after three steps in Float64)
    sp = mk(O)
    rng = np.random.default_rng(1)
    sp.flow.u[...] *= (1 + 1e-16 * rng.standard_normal(sp.flow.u.shape)).astype(T)
    O.BC(sp.flow.u, ubc, False, kw["perdir"])
    eps = float(np.finfo(T).eps)
    worst = 0.0
    while O.sim_time(so) < t_end:
        O.sim_step(so, remeasure=False)
        O.sim_step(sp, remeasure=False)
        S.sim_step(sh, remeasure=False)
        uo, uh = so.flow.u, S.to_host(sh.flow.u).astype(np.float64)
        scale = np.max(np.abs(uo))
        du = float(np.max(np.abs(uh - uo)) / scale)
        noise = float(np.max(np.abs(sp.flow.u - uo)) / scale)
        ddt = abs(so.flow.dt[-1] - sh.flow.dt[-1]) / so.flow.dt[-1]
        print(f"\nperiodic run {cfg}: step {len(so.flow.dt) - 1} du={du:.3e} d(dt)={ddt:.3e} (oracle vs its 1e-16 twin: {noise:.3e})")
        # within the case's own sensitivity to rounding (10x the twin's distance, never below 50 eps)
        bound = max(50 * eps, 10 * noise)
        assert du <= bound and ddt <= bound, (du, ddt, bound)
        worst = max(worst, du)
    assert abs(S.sim_time(sh) - O.sim_time(so)) < 1e-12 and len(so.flow.dt) == len(sh.flow.dt)
    assert so.pois.n == sh.pois.n, (so.pois.n, sh.pois.n)          # the same V-cycle count in EVERY solve
    assert worst <= (1e-5 if T == np.float32 else 2e-8)            # (rounds 1-3, reducing over inside(): 1.2e-4 / 1.9e-5)


@pytest.mark.parametrize("plane", [(0, 1), (1, 2), (2, 0)], ids=["xy", "yz", "zx"])
def test_extruded_taylor_green_vortex_in_3d_on_the_hip_path(plane):
    """The reference's periodic Taylor-Green test (maintests.jl:232-253) with the vortex lying in each coordinate plane of a
    fully periodic 64 x 64 x 16 box -- an exact solution in 3-D too (tests/test_oracle_3d_structure.py holds the oracle to
    it): the HIP path meets the reference's analytic bound per plane of cells, keeps the third velocity component exactly 0
    and follows the oracle (within the periodic deviation of DESIGN.md section 7.1)."""
    Lc, nthird = 64, 16
    a, b = plane
    c = 3 - a - b
    dims = [0, 0, 0]
    dims[a], dims[b], dims[c] = Lc, Lc, nthird
    k = 2 * math.pi / Lc
    nu = 1 / (k * 1e8)

    def tgv(i, x, t=0.0):
        xa, xb = x[a] * k, x[b] * k
        decay = math.exp(-2 * k ** 2 * nu * t)
        if i == a:
            return -np.sin(xa) * np.cos(xb) * decay
        if i == b:
            return np.cos(xa) * np.sin(xb) * decay
        return np.zeros_like(xa)

    kw = dict(U=1, ulam=tgv, nu=nu, T=np.float32, perdir=(0, 1, 2))
    so, sh = O.Simulation(tuple(dims), (0, 0, 0), Lc, **kw), S.Simulation(tuple(dims), (0, 0, 0), Lc, **kw)
    O.sim_step(so, math.pi / 100)
    S.sim_step(sh, math.pi / 100)
    assert len(so.flow.dt) == len(sh.flow.dt)
    ue = so.flow.u.copy(order="F")
    t = float(np.sum(np.asarray(sh.flow.dt[:-1], dtype=np.float64)))
    O.apply_vec(lambda i, x: tgv(i, x, t), ue)
    uh = S.to_host(sh.flow.u)
    for i in (a, b):
        assert O.L2(uh[..., i] - ue[..., i]) < 1e-4 * nthird
    assert np.all(uh[..., c][O.inside(uh[..., c])] == 0)
    assert so.pois.n == sh.pois.n
    assert np.abs(uh.astype(np.float64) - so.flow.u).max() <= 1e-5 * np.abs(so.flow.u).max()   # (faithful oracle: whole-array reductions on both sides)


# ----------------------------------------------------------------------------- reference known-answer tests on the HIP path

def Poisson_setup(poisson, N, T=np.float32):
    """maintests.jl:68-79"""
    D = len(N)
    c = np.ones(N + (D,), dtype=T, order="F")
    O.BC(c, (0.0,) * D)
    x, L, z = field(O.zeros(N, T), D), field(c, D), field(O.zeros(N, T), D)
    pois = poisson(x, L, z)
    soln = np.asfortranarray(np.broadcast_to(np.arange(1, N[0] + 1, dtype=T).reshape((-1,) + (1,) * (D - 1)), N).copy())
    I = (1,) * D
    soln -= soln[I]
    S.mult(pois, field(soln, D))
    S.solver(pois)
    xh = S.to_host(x)
    xh -= xh[I]
    return O.L2(xh - soln) / O.L2(soln), pois


def test_ref_poisson_diag_and_iterations():  # maintests.jl:83-92
    err, pois = Poisson_setup(S.Poisson, (5, 5))
    Dm = np.array([[0, 0, 0, 0, 0], [0, -2, -3, -2, 0], [0, -3, -4, -3, 0], [0, -2, -3, -2, 0], [0, 0, 0, 0, 0]], np.float32)
    assert np.array_equal(S.to_host(pois.D), Dm) and err < 1e-5
    err, pois = Poisson_setup(S.Poisson, (2 ** 6 + 2, 2 ** 6 + 2))
    assert err < 1e-6 and pois.n[0] < 310
    err, pois = Poisson_setup(S.Poisson, (2 ** 4 + 2,) * 3)
    assert err < 1e-6 and pois.n[0] < 35


def test_ref_multilevel():  # maintests.jl:99-116
    with pytest.raises(AssertionError, match="MultiLevelPoisson requires size=a2ⁿ, where n>2"):
        Poisson_setup(S.MultiLevelPoisson, (15 + 2, 3 ** 4 + 2))
    err, pois = Poisson_setup(S.MultiLevelPoisson, (10, 10))
    assert np.array_equal(S.to_host(pois.levels[2].D), np.array([[0, 0, 0, 0], [0, -2, -2, 0], [0, -2, -2, 0], [0, 0, 0, 0]], np.float32))
    assert err < 1e-5
    pois.levels[0].L[4:6, :, 0] = 0
    S.update(pois)
    assert np.array_equal(S.to_host(pois.levels[2].D), np.array([[0, 0, 0, 0], [0, -1, -1, 0], [0, -1, -1, 0], [0, 0, 0, 0]], np.float32))
    for T in TYPES:
        err, pois = Poisson_setup(S.MultiLevelPoisson, (2 ** 6 + 2, 2 ** 6 + 2), T)
        assert err < 1e-6 and pois.n[0] <= 3
        err, pois = Poisson_setup(S.MultiLevelPoisson, (2 ** 4 + 2,) * 3, T)
        assert err < 1e-6 and pois.n[0] <= 3


def test_ref_impulsive_flow():  # maintests.jl:172-180
    U = (2 / 3, -1 / 3)
    a = S.Flow((16, 16), U, T=np.float32)
    S.mom_step(a, S.MultiLevelPoisson(a.p, a.mu0, a.sigma))
    u = S.to_host(a.u)
    assert O.L2(u[:, :, 0] - np.float32(U[0])) < 2e-5 and O.L2(u[:, :, 1] - np.float32(U[1])) < 1e-5


def test_ref_increasing_body_force():  # maintests.jl:280-302 ("Flow.jl with increasing body force")
    N, jerk = 8, 4
    s = S.Simulation((N, N), (math.sqrt(N), 0.0), N, nu=0.001, g=lambda i, t: t * jerk if i == 0 else 0.0, dt=0.001,
                     perdir=(0,), T=np.float64)
    S.sim_step(s, 1.0)
    u = S.to_host(s.flow.u)
    uFinal = math.sqrt(N) + 0.5 * jerk * S.time(s.flow) ** 2          # u_x0 + integral of jerk*t dt
    assert O.L2(u[:, :, 0] - uFinal) < 1e-4 and O.L2(u[:, :, 1] - 0) < 1e-4


def test_ref_circle_in_accelerating_flow():  # maintests.jl:304-316
    radius, H = 32, 16
    c = float(H * radius)
    tw = bodies.sphere(c, radius)
    s = S.Simulation((radius * 2 * H, radius * 2 * H), lambda i, t: t if i == 0 else 0.0 * t, radius, U=1, body=tw.product,
                     geometry="device", T=np.float32)
    S.sim_step(s)
    f = S.pressure_force(s) / (math.pi * s.L ** 2)
    assert np.allclose(f, [-1, 0], atol=0.04)                          # added mass of the circle
    u = S.to_host(s.flow.u)
    assert u.max() / u[1, 1, 0] > 1.91                                 # ~2U at the shoulder
    for _ in range(3):
        S.sim_step(s)
    assert all(n <= 2 for n in s.pois.n)


@pytest.mark.parametrize("radius,N", [(16, 128), (32, 384)])
def test_sphere_in_accelerating_flow_added_mass_on_the_hip_path(radius, N):
    """maintests.jl:304-316 in 3-D (tests/test_oracle_3d_structure.py holds the oracle to the same numbers): the added mass of
    a sphere is half its displaced mass, pressure_force / (2/3 pi R^3) = [-1, 0, 0] +- 0.04, peak speed ~1.5 U; native measure!.
    The second case is out of the CPU oracle's reach in a test (56 M cells; 12 R box, 32-cell radius): closer to both limits."""
    from waterlily_amd import body as B
    s = S.Simulation((N, N, N), lambda i, t: t if i == 0 else 0.0 * t, radius, U=1, body=B.Sphere(N / 2, radius, 3), T=np.float32)
    S.sim_step(s)
    f = S.pressure_force(s) / (2 / 3 * math.pi * radius ** 3)
    assert np.allclose(f, [-1, 0, 0], atol=0.04 if radius == 16 else 0.02), f
    u = S.to_host(s.flow.u)
    assert u.max() / u[1, 1, 1, 0] > (1.4 if radius == 16 else 1.44), u.max() / u[1, 1, 1, 0]
    assert all(n <= 2 for n in s.pois.n)
    print(f"\nadded mass of the sphere R={radius} in {N}^3: force/(2/3 pi R^3) = {f}, peak speed {u.max() / u[1, 1, 1, 0]:.4f}")


@pytest.mark.parametrize("T", TYPES)
def test_viscous_decay_of_a_shear_wave_on_the_hip_path(T):
    """tests/test_oracle_3d_structure.py: u_a = 0.5 sin(k x_b) in a fully periodic box decays by 1 - z + z^2/2 per Heun step,
    z = nu dt (2 - 2 cos k) -- every (component, direction) pair of the diffusive flux, against the closed form (Float64 to
    rounding, Float32 to a few ulp per step) and with the oracle's time steps."""
    from test_oracle_3d_structure import shear_wave_case
    n = 32
    for a in range(3):
        for b in range(3):
            if a == b:
                continue
            kw, amplitude, k = shear_wave_case(a, b, n)
            kw["T"] = T
            so, sh = O.Simulation((n, n, n), (0, 0, 0), n, **kw), S.Simulation((n, n, n), (0, 0, 0), n, **kw)
            u0 = S.to_host(sh.flow.u).astype(np.float64)
            for _ in range(5):
                O.sim_step(so)
                S.sim_step(sh)
            assert np.allclose(so.flow.dt, sh.flow.dt, rtol=10 * np.finfo(T).eps, atol=0), (a, b)
            amp = amplitude(sh.flow.dt[:-1])
            ins = (slice(1, -1),) * 3
            err = np.abs(S.to_host(sh.flow.u).astype(np.float64)[ins] - amp * u0[ins]).max()
            assert err < (1e-14 if T == np.float64 else 2e-6), (a, b, err)


def test_ref_periodic_TGV():  # maintests.jl:232-253
    L = 64
    k = 2 * math.pi / L
    nu = 1 / (k * 1e8)

    def TGV(i, xy, t):
        x, y = xy[0] * k, xy[1] * k
        e = np.exp(-2 * k ** 2 * nu * t)
        return -np.sin(x) * np.cos(y) * e if i == 0 else np.cos(x) * np.sin(y) * e

    s = S.Simulation((L, L), (0, 0), L, U=1, ulam=lambda i, x: TGV(i, x, 0.0), nu=nu, T=np.float32, perdir=(0, 1))
    S.sim_step(s, math.pi / 100)
    ue = O.zeros(s.flow.N + (2,), np.float32)
    O.apply_vec(lambda i, x: TGV(i, x, S.time(s.flow)), ue)
    u = S.to_host(s.flow.u)
    assert O.L2(u[:, :, 0] - ue[:, :, 0]) < 1e-4 and O.L2(u[:, :, 1] - ue[:, :, 1]) < 1e-4


@pytest.mark.parametrize("exitBC", [True, False])
def test_ref_moving_bodies(exitBC):  # maintests.jl:391-412 (`for exitBC ∈ (true,false)`) + sim_time stop rule :387-390
    radius = 8
    nu = radius / 250
    nm = (4 * radius, 4 * radius)
    kw = dict(nu=nu, T=np.float32, exitBC=exitBC)
    s = S.Simulation(nm, (1, 0), radius, body=bodies.sphere(2.0 * radius, radius).product, **kw)
    assert S.sim_time(s) == 0
    S.sim_step(s, 0.1, remeasure=False)
    assert S.sim_time(s) >= 0.1 > sum(s.flow.dt[:-2]) * s.U / s.L
    s = S.Simulation(nm, (1, 0), radius, body=bodies.moving_circle(2.0 * radius, radius, v=1.0).product, **kw)
    S.sim_step(s)
    assert np.allclose(S.to_host(s.flow.u)[:, radius - 1, 0], 1, rtol=1e-3)
    s = S.Simulation(nm, (0, 0), radius, U=1, body=bodies.moving_circle(2.0 * radius, radius, a=2.0).product, **kw)
    S.sim_step(s)
    assert s.pois.n == [2, 1]
    assert float(s.flow.u.max()) > float(s.flow.V.max()) > 0
    # non-uniform V doesn't break (:376-379, rotating plate) -- the closures through torch, then the native plate family
    for body in (bodies.rotating_plate(radius).product, bodies.rotating_plate(radius).native(2)):
        s = S.Simulation(nm, (0, 0), radius, U=1, body=body, **kw)
        S.sim_step(s)
        assert s.pois.n == [2, 1]
        assert 1 > s.flow.dt[-1] > 0.5
    # divergent V doesn't break (:380-383, bending plate: a non-affine map, closures only)
    s = S.Simulation(nm, (0, 0), radius, U=1, body=bodies.bending_plate(radius).product, **kw)
    S.sim_step(s)
    assert s.pois.n == [2, 1]
    assert 1.2 > s.flow.dt[-1] > 0.8


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("dims", [(34, 18), (18, 18, 10)])
def test_solver_log_and_Linf(T, dims):
    """L∞(p) (Poisson.jl:147) and the rows of the reference's pressure-solver log (`@log ", $n, $(L∞(p)), $r₂"`,
    MultiLevelPoisson.jl:90,94) from the overridden solver!: against the oracle's operators replayed in the order
    solver! calls them (residual!, then Vcycle! + pcg! per iteration), same iteration count, r∞ and r₂ to rounding."""
    Ng = tuple(dims)
    D = len(Ng)
    c = np.asfortranarray(rnd(Ng + (D,), T, 3, 0.2, 1.0))
    O.BC(c, (0.0,) * D)
    z0 = rnd(Ng, T, 4)
    z0[O.inside(z0)] -= z0[O.inside(z0)].mean().astype(T)
    xo, Lo, zo = O.zeros(Ng, T), c.copy(order="F"), z0.copy(order="F")
    po = O.MultiLevelPoisson(xo, Lo, zo)
    xh, Lh, zh = field(O.zeros(Ng, T), D), field(c, D), field(z0, D)
    ph = S.MultiLevelPoisson(xh, Lh, zh)
    S.solver_log(ph, True)
    S.solver(ph)
    rows = S.read_solver_log(ph)
    # the oracle replay of MultiLevelPoisson.jl:87-99
    p0 = po.levels[0]
    O.residual(p0)
    want = [(0, float(np.max(np.abs(p0.r))), O.L2p(p0))]
    n = 0
    while n < 32:
        O.Vcycle(po)
        O.pcg(p0)
        n += 1
        want.append((n, float(np.max(np.abs(p0.r))), O.L2p(p0)))
        if want[-1][2] < 1e-4:
            break
    assert ph.n == [n] and len(rows) == len(want)
    for got, w in zip(rows, want):
        assert got[0] == w[0]
        assert abs(got[1] - w[1]) <= 200 * rtol(T) * max(want[0][1], 1e-30) and abs(got[2] - w[2]) <= 200 * rtol(T) * max(want[0][2], 1e-30)
    assert abs(S.Linf(ph) - want[-1][1]) <= 200 * rtol(T) * want[0][1]
    txt = S.format_solver_log(rows, "p")
    assert txt.startswith("p, 0, ") and txt.count("\n") == len(rows)
    assert len(S.read_solver_log(ph)) == 0                    # read clears
    S.solver_log(ph, False)
    S.solver(ph)
    assert len(S.read_solver_log(ph)) == 0


def test_ref_hydrostatic_force():  # maintests.jl:341-346
    N = 32
    for T in TYPES:
        p = O.zeros((N, N), T)
        p[O.inside(p)] = O.loc(-1, (N, N))[1][O.inside(p)].astype(T)
        pd = field(p, 2)
        idx, nds = G.nds_band(G.Body(G.Sphere(N / 2, N // 4)), (N - 2, N - 2))
        force = S.pressure_force_band(pd, *S.band_to_device(pd, idx, nds))
        assert np.sum(np.abs(force / (math.pi * (N / 4) ** 2) - np.array([0, 1]))) < 2e-3
        assert np.allclose(force, O.pressure_force_band(p, O.zeros((N, N, 2), T), idx, nds), rtol=1e-12)


@pytest.mark.parametrize("geometry", ["device", "host"])
@pytest.mark.parametrize("T", TYPES)
def test_geometry_matches_oracle(geometry, T):
    """measure! (Body.jl:31-53) of the product -- closures + autograd on the GPU ("device") or on the
    host -- against the closed-form geometry oracle: mu0, mu1, V (after BC!) and sigma = sdf to a few ulp of T for the
    sphere, the torus and a translating circle; then a moving body (remeasure every step, maintests.jl:398-401) steps
    like the oracle's: same V-cycle counts, u within the step tolerance."""
    m = 32
    cases = [((m, m, m), bodies.sphere(m / 2 - 1, m / 8), 0.0), ((m, m, m), bodies.torus(m / 2, m / 4, m / 16), 0.0),
             ((48, 32), bodies.moving_circle(16.0, 8.0, a=2.0), 0.5)]
    eps = geom_tol(T) / 4
    for dims, tw, t in cases:
        ubc = (1.0,) + (0.0,) * (len(dims) - 1)
        so = O.Simulation(dims, ubc, 8.0, body=tw.oracle, T=T)
        sh = S.Simulation(dims, ubc, 8.0, body=tw.product, T=T, geometry=geometry)
        if t:
            O.measure(so, t)
            S.measure(sh, t)
        for k in ("mu0", "mu1", "V"):
            w = getattr(so.flow, k)
            assert np.abs(S.to_host(getattr(sh.flow, k)).astype(np.float64) - w).max() <= 4 * eps * max(1.0, np.abs(w).max()), (k, dims)
        ins = O.inside(so.flow.sigma)
        assert np.abs(S.to_host(sh.flow.sigma)[ins].astype(np.float64) - so.flow.sigma[ins]).max() <= 4 * eps * np.abs(so.flow.sigma).max()
        for lo, lh in zip(so.pois.levels, sh.pois.levels):             # update!: coarse coefficients from measured mu0
            assert np.abs(S.to_host(lh.L).astype(np.float64) - lo.L).max() <= 8 * eps * max(1.0, np.abs(lo.L).max())
        assert np.allclose(S.pressure_force(sh), O.pressure_force(so), atol=1e-10)      # p = 0: band builds, force 0
    radius = 8
    tw = bodies.moving_circle(2.0 * radius, radius, a=2.0)
    so, sh = pair((32, 32), (0, 0), radius, U=1, body=tw, nu=radius / 250, T=T, geometry=geometry)
    for _ in range(2):
        O.sim_step(so)
        S.sim_step(sh)
    assert so.pois.n == sh.pois.n and sh.pois.n[:2] == [2, 1]
    same(sh.flow.u, so.flow.u, exact=False, tol=50 * rtol(T))
    assert np.allclose(S.pressure_force(sh), O.pressure_force(so), rtol=1e-3 if T == np.float32 else 1e-8, atol=1e-5 if T == np.float32 else 1e-10)


@pytest.mark.parametrize("T", TYPES)
def test_native_measure_matches_oracle(T):
    """The hand-written measure! kernels (csrc/wl_measure.h: parametric body = closed-form sdf family + affine map)
    against the closed-form geometry oracle: mu0, mu1, V (after BC!), sigma, the band-cell list and the pressure-force
    band; a second measure! at a later time must leave no trace of the first (rows the body has left are rewritten
    with (1,0,0)); the body-free row flags must mark every row that carries a non-trivial coefficient."""
    m = 32
    cases = [((m, m, m), bodies.sphere(m / 2 - 1, m / 8), (0.0,)), ((m, m, m), bodies.torus(m / 2, m / 4, m / 16), (0.0,)),
             ((48, 32), bodies.sphere(15.0, 4.0), (0.0,)),
             ((48, 32), bodies.moving_circle(14.0, 6.0, v=3.0, a=2.0), (0.0, 0.5, 2.5)),
             ((40, 40), bodies.rotating_circle(9.0, 5.0, 20.0, 0.4, 1.0), (0.0, 1.7)),
             ((32, 32), bodies.rotating_plate(8), (0.0, 0.6, 2.3)),
             ((m, m, m), bodies.moving_circle(12.0, 4.0, a=2.0, D=3), (0.3, 1.2)),
             # the cylinder family and native COMPOSITES (the reference's `Bodies`, AutoBody.jl:40-110): difference +
             # intersection of three leaves with one of them moving; union of a fixed and a moving circle
             ((m, m, 16), bodies.cylinder(14.0, 5.0), (0.0,)),
             ((m, m, m), bodies.drilled_sphere(v=0.7), (0.0, 1.3)),
             ((48, 32), bodies.two_circles(), (0.0, 2.0))]
    eps = geom_tol(T)
    for dims, tw, times in cases:
        D = len(dims)
        ubc = (1.0,) + (0.0,) * (D - 1)
        so = O.Simulation(dims, ubc, 8.0, body=tw.oracle, T=T)
        sh = S.Simulation(dims, ubc, 8.0, body=tw.native(D), T=T)          # geometry="device": native kernels
        for t in times:
            O.measure(so, t)
            S.measure(sh, t)
            for k in ("mu0", "mu1", "V"):
                w = getattr(so.flow, k)
                assert np.abs(S.to_host(getattr(sh.flow, k)).astype(np.float64) - w).max() <= eps * max(1.0, np.abs(w).max()), (k, dims, t)
            ins = O.inside(so.flow.sigma)
            assert np.abs(S.to_host(sh.flow.sigma)[ins].astype(np.float64) - so.flow.sigma[ins]).max() <= eps * np.abs(so.flow.sigma).max()
            # band cells: exactly the cells with sigma^2 < 9, ascending
            sg = so.flow.sigma
            want = np.flatnonzero(np.ravel((sg * sg < T(9)) & _inside_mask(sg.shape), order="F"))
            got = sh.flow._band_cells[1].cpu().numpy()
            if not np.array_equal(got, want):                           # sigma within 1 ulp of 3: membership may flip
                assert len(np.setxor1d(got, want)) <= 2
            # pressure-force band (nds, Metrics.jl:84-87) through wl_body_nds
            so.flow.p[...] = rnd(so.flow.p.shape, T, 5)
            S.upload(sh.flow.p, so.flow.p)
            so.flow.dt[:] = [t, 0.25]                                    # time(flow) = t on both sides
            sh.flow.dt[:] = [t, 0.25]
            sh._band = None
            fo, fh = O.pressure_force(so), S.pressure_force(sh)
            assert np.allclose(fo, fh, rtol=1e-4 if T == np.float32 else 1e-10, atol=1e-5 if T == np.float32 else 1e-11), (dims, t)
    # a moving native body steps like the oracle's (remeasure every step)
    radius = 8
    tw = bodies.moving_circle(2.0 * radius, radius, a=2.0)
    so = O.Simulation((32, 32), (0, 0), radius, U=1, body=tw.oracle, nu=radius / 250, T=T)
    sh = S.Simulation((32, 32), (0, 0), radius, U=1, body=tw.native(2), nu=radius / 250, T=T)
    for _ in range(3):
        O.sim_step(so)
        S.sim_step(sh)
    assert so.pois.n == sh.pois.n and sh.pois.n[:2] == [2, 1]
    same(sh.flow.u, so.flow.u, exact=False, tol=50 * rtol(T))
    # the body-free row flags the native path derives from its touched rows: BDIM! with them == BDIM! without (Opt.BDIM_ROWFLAGS)
    runs = []
    for on in (1, 0):
        with S.options({Opt.BDIM_ROWFLAGS: on}):
            s3 = S.Simulation((m, m, m), (1.0, 0.0, 0.0), 8.0, body=bodies.moving_circle(12.0, 4.0, v=1.0, D=3).native(3), nu=0.05, T=T)
            for _ in range(3):
                S.sim_step(s3)
        runs.append(s3)
    assert runs[0].pois.n == runs[1].pois.n
    assert torch.equal(runs[0].flow.u, runs[1].flow.u) and torch.equal(runs[0].flow.p, runs[1].flow.p)


@pytest.mark.parametrize("T", TYPES)
def test_native_measure_of_a_body_overlapping_the_domain_boundary(T):
    """A body that has moved partly (or wholly) out of the domain: measure! fills inside(p) only and BC! closes the ghost
    cells (Body.jl:36-52) -- the native kernels' row bookkeeping must clip the same way on every face; coefficient fields and
    the diagonals of every multigrid level against the oracle."""
    from waterlily_amd import body as B
    eps = geom_tol(T)
    for dims, c0, R, shifts in (((128, 64), (32.0, 32.0), 8.0, ((88.0, 0.0), (93.5, 0.0), (99.0, 0.0), (-30.0, 0.0), (0.0, 27.0), (0.0, -29.3), (120.0, 0.0))),
                                ((48, 32, 32), (16.0, 16.0, 16.0), 5.0, ((33.0, 0.0, 0.0), (-11.25, 0.0, 0.0), (0.0, 13.5, 0.0), (0.0, 0.0, -14.65), (0.0, 0.0, 14.0)))):
        D = len(dims)
        for v in shifts:
            U = (0.0,) * D
            so = O.Simulation(dims, U, 8.0, U=1.0, body=G.Body(G.Sphere(c0, R), G.Translate(v=v)), T=T)
            sn = S.Simulation(dims, U, 8.0, U=1.0, body=B.Sphere(c0, R, D, map=B.translation(D, v=v)), T=T)
            for t in (0.5, 1.0):            # on the way out, then at the shifted position
                O.measure(so, t)
                S.measure(sn, t)
                for k in ("mu0", "mu1", "V"):
                    w = getattr(so.flow, k)
                    assert np.abs(S.to_host(getattr(sn.flow, k)).astype(np.float64) - w).max() <= eps * max(1.0, np.abs(w).max()), (k, dims, v, t)
                for a, b in zip(so.pois.levels, sn.pois.levels):
                    assert np.abs(S.to_host(b.D).astype(np.float64) - a.D).max() <= 16 * eps, (dims, v, t)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("perdir", [(), (1, 2)], ids=["walls", "yz-periodic"])
def test_update_of_changed_rows_equals_full_update(T, perdir):
    """update!(pois) after a native measure! revisits, on the finest level, only the rows that measure! rewrote (plus the
    lower neighbours whose diagonal reads them): D, iD, the solver's behaviour and every field of a moving-body run are
    bit-identical to the same run with the full update!.  Periodic y / z: the body sits on the lower y / z faces and
    moves along them, so the last interior rows -- whose upper ghost row is the periodic copy of the first interior row --
    must follow the rows next to the opposite face."""
    from waterlily_amd import body as B
    m = 40
    if perdir:
        body = lambda: B.Sphere((14.0, 2.5, 3.0), 5.0, 3, map=B.translation(3, v=(1.5, 0.3, -0.2), a=(0.5, 0.0, 0.0)))
    else:
        body = lambda: bodies.moving_circle(14.0, 5.0, v=1.5, a=0.5, D=3).native(3)
    mk = lambda: S.Simulation((m, m, m), (1.0, 0.0, 0.0), 8.0, body=body(), nu=0.05, T=T, perdir=perdir)
    a, b = mk(), mk()
    for _ in range(4):
        S.sim_step(a)                                   # measure! + update!(pois, flow): changed rows only
        S.measure_flow(b.flow, b.body, t=float(np.sum(np.asarray(b.flow.dt, dtype=np.float64))), eps=b.eps, geometry=b.geometry)
        b._band = None
        S.update(b.pois)                                # full update!
        S.mom_step(b.flow, b.pois)
        for k in ("D", "iD"):
            assert torch.equal(getattr(a.pois.levels[0], k), getattr(b.pois.levels[0], k)), k
        assert S.uniform_rows(a.pois, 0) == S.uniform_rows(b.pois, 0)
    assert a.pois.n == b.pois.n
    assert torch.equal(a.flow.u, b.flow.u) and torch.equal(a.flow.p, b.flow.p)
    for l in range(1, len(a.pois.levels)):
        assert torch.equal(a.pois.levels[l].L, b.pois.levels[l].L) and torch.equal(a.pois.levels[l].iD, b.pois.levels[l].iD), l


def test_two_measures_before_one_update_keep_every_changed_row():
    """measure_flow is public: two native measure! calls in a row (the body jumps twice) followed by ONE update!(pois, flow).
    The rows the first call reset to (1,0,0) and the second did not touch must still be revisited: the changed-row record
    accumulates until update! consumes it.  Result == the full update!."""
    m = 40
    T = np.float32
    mk = lambda: S.Simulation((m, m, m), (1.0, 0.0, 0.0), 8.0, body=bodies.moving_circle(12.0, 4.0, v=1.0, D=3).native(3), nu=0.05, T=T)
    a, b = mk(), mk()
    for s in (a, b):
        for t in (9.0, 18.0):                           # far jumps: three disjoint sets of rows
            S.measure_flow(s.flow, s.body, t=t, eps=s.eps, geometry=s.geometry)
    S.update(a.pois, a.flow)                            # changed rows of BOTH calls
    S.update(b.pois)                                    # full
    for k in ("D", "iD"):
        assert torch.equal(getattr(a.pois.levels[0], k), getattr(b.pois.levels[0], k)), k
    assert S.uniform_rows(a.pois, 0) == S.uniform_rows(b.pois, 0)
    # and the record is consumed: a third measure! + update! is again equal to the full one
    for s in (a, b):
        S.measure_flow(s.flow, s.body, t=20.0, eps=s.eps, geometry=s.geometry)
    S.update(a.pois, a.flow)
    S.update(b.pois)
    assert torch.equal(a.pois.levels[0].iD, b.pois.levels[0].iD) and S.uniform_rows(a.pois, 0) == S.uniform_rows(b.pois, 0)


def _inside_mask(shape):
    m = np.zeros(shape, bool)
    m[tuple(slice(1, n - 1) for n in shape)] = True
    return m


@pytest.mark.parametrize("T", TYPES)
def test_noncubic_partial_tiles(T):
    """Shapes that leave partially filled 64-wide (conv_diff) and 256-wide (vector stencil) tiles plus several tiles
    per row, like the reference's README example (96,64,64): operators bit-exact, a whole solve and steps close."""
    Ng = (96 + 2, 32 + 2, 16 + 2)
    D = 3
    u = rnd(Ng + (D,), T, 41)
    r, Phi = O.zeros(Ng + (D,), T), O.zeros(Ng, T)
    O.conv_diff(r, u, Phi, nu=0.02)
    ud, rd = field(u, D), field(rnd(Ng + (D,), T, 42), D)
    S.conv_diff(rd, ud, nu=0.02)
    same(rd, r)
    po, ph = make_pois(Ng, T, O.MultiLevelPoisson, S.MultiLevelPoisson, seed=50)
    O.residual(po)
    S.residual(ph)
    S.upload(lev_h(ph).r, lev_o(po).r)
    O.Jacobi(po)
    S.Jacobi(ph)
    same(lev_h(ph).r, lev_o(po).r)
    same(ph.x, po.x)
    O.Vcycle(po)
    S.Vcycle(ph)
    same(lev_h(ph).r, lev_o(po).r, exact=False, tol=rtol(T))
    O.solver(po)
    S.solver(ph)
    assert po.n == ph.n
    same(ph.x, po.x, exact=False, tol=10 * rtol(T))
    m = 32
    R = m / 8
    so, sh = pair((96, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 250, body=bodies.sphere(m / 2 - 1, R), T=T)
    check_step(so, sh, T, 2)


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("D", [2, 3])
def test_viscous_force_pressure_moment_parity(T, D):
    """Metrics.jl:103-134 on random fields: HIP band kernels vs the oracle."""
    N = 32
    shp = (N,) * D
    idx, nds = G.nds_band(G.Body(G.Sphere(N / 2, N // 4)), tuple(n - 2 for n in shp))
    u, p = rnd(shp + (D,), T, 70), rnd(shp, T, 71)
    df = O.zeros(shp + (D,), T)
    ud, pd = field(u, D), field(p, D)
    bi, bn = S.band_to_device(pd, idx, nds)
    g = S._grid_of(ud, D)
    out = (S.C.c_double * 3)()
    S.check(S._lib.lib().wl_vforce(S._WLT[np.dtype(T)], S.C.byref(g), S._ptr(ud), S.C.c_void_p(bi.data_ptr()),
                                   S.C.c_void_p(bn.data_ptr()), bi.numel(), 0.37, out))
    ref = O.viscous_force_band(u, 0.37, df, idx, nds)
    assert np.allclose(np.array(out[:D]), ref, rtol=1e-12, atol=1e-12)
    x0 = (N / 2 + 0.25, N / 2 - 1.0, N / 2)[:D]
    S.check(S._lib.lib().wl_pmoment(S._WLT[np.dtype(T)], S.C.byref(S._grid_of(pd, D)), S._ptr(pd), S.C.c_void_p(bi.data_ptr()),
                                    S.C.c_void_p(bn.data_ptr()), bi.numel(), S.d3(x0), out))
    ref = O.pressure_moment_band(x0, p, df, idx, nds)
    assert np.allclose(np.array(out[:D]), ref, rtol=1e-12, atol=1e-10)


def test_total_force_api():
    m = 32
    R = m / 8
    so, sh = pair((m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 100, body=bodies.sphere(m / 2 - 1, R), T=np.float64)
    check_step(so, sh, np.float64, 2)
    assert np.allclose(S.viscous_force(sh), O.viscous_force(so), rtol=1e-8, atol=1e-12)
    assert np.allclose(S.total_force(sh), O.total_force(so), rtol=1e-8, atol=1e-12)
    assert np.allclose(S.pressure_moment((m / 2,) * 3, sh), O.pressure_moment((m / 2,) * 3, so), rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("D", [2, 3])
def test_vtk_write_restart_roundtrip(D, tmp_path):
    """maintests.jl:420-443 (VTKExt.jl): write a snapshot, restart a fresh simulation from it, bitwise equal fields."""
    from waterlily_amd import vtk
    radius = 8

    def sphere_sim():
        c = 2 * radius + 1.5
        body = bodies.sphere(c, radius).product
        dims = (6 * radius, 4 * radius) if D == 2 else (6 * radius, 4 * radius, radius)
        U = (1, 0) if D == 2 else (1, 0, 0)
        return S.Simulation(dims, U, radius, body=body, nu=radius / 250, T=np.float32)

    sim = sphere_sim()
    wr = vtk.vtkWriter(str(tmp_path / f"test_vtk_reader_{D}"), dir=str(tmp_path / "TEST_DIR"))
    S.sim_step(sim, 1.0)
    vtk.write(wr, sim)
    vtk.close(wr)
    restart = sphere_sim()
    vtk.restart_sim(restart, fname=str(tmp_path / f"test_vtk_reader_{D}.pvd"))
    assert torch.equal(sim.flow.p, restart.flow.p)
    assert torch.equal(sim.flow.u, restart.flow.u)
    assert torch.equal(sim.flow.mu0, restart.flow.mu0)
    assert sim.flow.dt[-1] == restart.flow.dt[-1]
    assert abs(S.sim_time(sim) - S.sim_time(restart)) < 1e-3


def test_vtk_snapshots_are_asynchronous_and_complete(tmp_path):
    """The writer only ENQUEUES (device pack + event); D2H on a side stream and the file write happen on a worker thread while
    the simulation keeps stepping.  A burst of snapshots taken every step must each hold the fields of ITS step (the device
    staging ring decouples them from the fields the next step overwrites), a custom attribute (a device field) is written next
    to the defaults, and a Float64 run round-trips bit for bit as well."""
    from waterlily_amd import vtk
    m = 32
    R, c = m / 8, m / 2 - 1
    sim = S.Simulation((2 * m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 250, body=bodies.sphere(c, R).product, T=np.float64)
    attrib = dict(vtk.default_attrib())
    attrib["Body"] = lambda s: s.flow.mu0
    wr = vtk.vtkWriter(str(tmp_path / "burst"), attrib=attrib, dir=str(tmp_path / "BURST"), ring=2, host_buffers=1)
    kept = []
    for _ in range(5):                                     # more snapshots than staging slots: the third write has to wait its turn
        S.sim_step(sim, remeasure=False)
        vtk.write(wr, sim)
        kept.append((S.to_host(sim.flow.u), S.to_host(sim.flow.p)))
    vtk.close(wr)
    assert wr.stats["snapshots"] == 5 and wr.stats["skipped"] == 0
    items = vtk.read_pvd(str(tmp_path / "burst.pvd"))
    assert len(items) == 5
    for (t, path), (u, p) in zip(items, kept):
        d = vtk.read_vti(path)
        assert np.array_equal(np.asarray(d["Pressure"]), p)
        assert np.array_equal(np.moveaxis(np.asarray(d["Velocity"]), 0, -1), u)
    assert np.array_equal(np.moveaxis(np.asarray(vtk.read_vti(items[-1][1])["Body"]), 0, -1), S.to_host(sim.flow.mu0))
    again = S.Simulation((2 * m, m, m), (1.0, 0.0, 0.0), 2 * R, nu=2 * R / 250, body=bodies.sphere(c, R).product, T=np.float64)
    vtk.restart_sim(again, fname=str(tmp_path / "burst.pvd"))
    assert torch.equal(sim.flow.u, again.flow.u) and torch.equal(sim.flow.p, again.flow.p)
    # on_busy="skip": a snapshot that finds its slot in flight is dropped, never a torn one written
    wr2 = vtk.vtkWriter(str(tmp_path / "skip"), dir=str(tmp_path / "SKIP"), ring=1, host_buffers=1, on_busy="skip")
    for _ in range(4):
        vtk.write(wr2, sim)
    vtk.close(wr2)
    assert wr2.stats["snapshots"] + wr2.stats["skipped"] == 4 and wr2.stats["snapshots"] >= 1
    for t, path in vtk.read_pvd(str(tmp_path / "skip.pvd")):
        assert np.array_equal(np.asarray(vtk.read_vti(path)["Pressure"]), S.to_host(sim.flow.p))


@pytest.mark.parametrize("T", TYPES)
def test_field_metrics_parity(T):
    """Metrics.jl:14-77 field metrics: the reference's analytic case + random-field parity."""
    Ng = (14, 12, 10)
    u = rnd(Ng + (3,), T, 90)
    ud = field(u, 3)
    po, pd = O.zeros(Ng, T), field(O.zeros(Ng, T), 3)
    cases = [("ke", {}), ("ke", dict(par=(0.3, -0.2, 0.1))), ("curl", dict(i=0)), ("curl", dict(i=1)), ("curl", dict(i=2)),
             ("omega_mag", {}), ("omega_theta", dict(par=(0, 0, 1), par2=(5.0, 6.5, 3.0))), ("lambda2", {})]
    for kind, kw in cases:
        O.metric(po, kind, u, **kw)
        S.metric(pd, kind, ud, **kw)
        tol = 0 if kind in ("ke", "curl") else (2e-5 if T == np.float32 else 1e-11)
        same(pd, po, exact=(tol == 0), tol=tol)
    u2 = rnd((16, 12, 2), T, 91)                       # 2-D: ke and the out-of-plane curl
    ud2, po2, pd2 = field(u2, 2), O.zeros((16, 12), T), field(O.zeros((16, 12), T), 2)
    for kind, kw in (("ke", {}), ("curl", dict(i=2))):
        same(S.metric(pd2, kind, ud2, **kw), O.metric(po2, kind, u2, **kw))
