"""MeshBody on the GPU: the mesh measure! kernels (csrc/wl_mesh.h) against the brute-force checker tests/mesh_ref.py, against
the closure box on the torch path, the reference's metric known answers on a mesh, moving-mesh bookkeeping, and an icosphere
next to the parametric sphere.

Tolerances are derived, not measured: both sides compute the distance in Float64 from operands of magnitude <= L (the
largest coordinate met in xi space) and differ by operation order only: tol_d = 64 * 2^-52 * L; a normal component carries
tol_d / |d|; a value stored as T may sit one unit in the last place of T away in addition.

Every body sits off the lattice, the identity poses too (centre (23.37, 24.91, 21.19): no two fractional parts add up or differ
by a multiple of 0.5, so no lattice or face point lies on a symmetry plane of an axis-aligned body; with the checker alone on
the CPU these four cases leave out 0, 1, 1, 0 of 9087 - 16104 face points and none at the cut), so that the checker alone stays inside
the issue's caps on what a comparison may leave out, which are asserted for every case: band membership, the sign of sigma and
the (2+eps)^2 cut of n and V where the checker's value is within tol_d + ulp of the cut: at most 2 cells per case; mu1 and nds
where the gap to the second-closest triangle is below 1e-9 (the medial axis): at most 0.1 % of the points compared.  Every
interior cell outside the band must hold exactly (1 or 0 by the sign of sigma, 0, 0).

Test 1 runs 8 of the 128 combinations of grid, type, layout, eps, body and pose (every value of every factor, every body in both
poses, but not every body at both element types in one pose): the brute-force checker costs 1.5 - 5 s per case and the file has
45 s.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_ref  # noqa: E402
import mesh_shapes as MS  # noqa: E402
from test_hip_parity import geom_tol, rtol, same  # noqa: E402
from test_mesh_cpu import SHAPES, off_lattice_map, tol_d  # noqa: E402

from waterlily_amd import _lib, body as B, sim as S  # noqa: E402
from waterlily_amd.mesh import MeshBody  # noqa: E402

pytestmark = pytest.mark.gpu


def ulp(T, v):
    return np.spacing(np.abs(np.asarray(v)).astype(T)).astype(np.float64)


def body_of(shape, posed):
    v, t = SHAPES[shape]()
    return MeshBody(v, t, map=off_lattice_map(1.3)) if posed else MeshBody(v + np.array([23.37, 24.91, 21.19]), t)


CASES = [("cube", False, (48, 48, 48), np.float32, True, 1), ("cube", True, (64, 48, 40), np.float64, False, 2),
         ("icosphere", False, (64, 48, 40), np.float64, True, 2), ("icosphere", True, (48, 48, 48), np.float32, False, 1),
         ("torus", False, (48, 48, 48), np.float64, False, 1), ("torus", True, (64, 48, 40), np.float32, True, 2),
         ("lprism", False, (64, 48, 40), np.float32, False, 2), ("lprism", True, (48, 48, 48), np.float64, True, 1)]


@pytest.mark.parametrize("shape,posed,dims,T,padded,eps", CASES)
def test_fields_against_the_checker(shape, posed, dims, T, padded, eps):
    mb = body_of(shape, posed)
    tt = 0.8 if posed else 0.0
    sim = S.Simulation(dims, (1.0, 0.0, 0.0), 8.0, body=mb, T=T, eps=eps, padded=padded)
    if posed:
        S.measure(sim, tt)
    ref = mesh_ref.Ref(mb.vertices, mb.triangles)
    pose = mb.coeffs(tt)
    R = mb._R / pose[5]
    N = np.array(sim.flow.N)
    sg = S.to_host(sim.flow.sigma)
    mu0, mu1, V = (S.to_host(getattr(sim.flow, k)).astype(np.float64) for k in ("mu0", "mu1", "V"))
    cand = sim.flow._band_cells[1].cpu().numpy()
    d2 = T((2 + eps) * (2 + eps))
    interior = np.zeros(sg.shape, dtype=bool)
    interior[1:-1, 1:-1, 1:-1] = True
    # the device's list is the device's own band, ascending
    assert np.array_equal(cand, np.flatnonzero(np.ravel((sg * sg < d2) & interior, order="F")))
    assert len(cand) > 500
    # the checker at: the band, the shell of cells around it, and a few thousand cells anywhere
    band = np.zeros(sg.shape, dtype=bool)
    band[np.unravel_index(cand, sg.shape, order="F")] = True
    grown = band.copy()
    for ax in range(3):
        grown |= np.roll(band, 1, ax) | np.roll(band, -1, ax)
    rng = np.random.default_rng(5)
    extra = np.zeros(sg.shape, dtype=bool)
    extra[tuple(rng.integers(1, N[a] - 1, size=4000) for a in range(3))] = True
    Q = np.argwhere((grown | extra) & interior)
    xc = Q - 0.5
    L = max(np.max(np.abs(xc @ pose[0].T + pose[1])), np.max(np.abs(mb.vertices)))
    td = tol_d(L)
    dr, _, _, _ = mesh_ref.measure(ref, pose, xc)
    sq = sg[tuple(Q.T)].astype(np.float64)
    u = ulp(T, dr)
    print(f"\n{shape} posed={posed} {dims} {np.dtype(T).name}: band {len(cand)} cells, checked {len(Q)}, L={L:.1f}, tol_d={td:.2e}")
    exact = np.abs(dr) < R - td
    far = np.abs(dr) >= R + td
    err = np.abs(sq - dr)[exact] - u[exact]
    print(f"  sigma exact zone: max |dev - ref| - ulp = {err.max():.3e}")
    assert err.max() <= td
    assert np.all(np.sign(sq[far]) == np.sign(dr[far])) and np.all(np.abs(sq[far]) >= R - td - u[far])
    # band membership and the sign, apart from values within the tolerance of the cut
    want = (dr.astype(T) ** 2 < d2)
    got = band[tuple(Q.T)]
    edge = np.abs(np.abs(dr) - (2 + eps)) <= td + u
    flips = int(np.sum((want != got) & edge))
    assert not np.any((want != got) & ~edge) and flips <= 2
    sflip = (np.sign(sq) != np.sign(dr)) & (sq != 0) & (dr != 0)
    assert not np.any(sflip & (np.abs(dr) > td + u)) and int(sflip.sum()) <= 2
    # faces of the band cells: mu0, mu1, V
    Bc = np.argwhere(band)
    I = tuple(Bc.T)
    kept = left = 0
    for c in range(3):
        xf = Bc - 0.5
        xf[:, c] -= 0.5
        dc, n, Vr, gap = mesh_ref.measure(ref, pose, xf, fastd2=(2.0 + eps) ** 2)
        cut = np.abs(np.abs(dc) - (2 + eps)) <= td       # n, V switch off beyond (2+eps)^2 (AutoBody.jl:118): V is not compared
        assert cut.sum() <= 2
        q = np.clip(dc / eps, -1, 1)
        e0 = np.abs(mu0[I + (c,)] - mesh_ref.kern0(q))
        assert e0.max() <= td / eps + ulp(T, 1.0), (c, e0.max())
        eV = np.abs(V[I][:, c] - Vr[:, c])[~cut]
        assert eV.max() <= 64 * 2.0 ** -52 * max(1.0, np.abs(Vr).max()) + ulp(T, np.abs(Vr).max()), (c, eV.max())
        smooth = (gap > 1e-9) & (np.abs(dc) > 1e-6) & ~cut
        kept += int(smooth.sum())
        left += int((~smooth & ~cut).sum())
        w1 = eps * mesh_ref.kern1(q)[:, None] * n
        e1 = np.abs(mu1[I][:, c, :] - w1)[smooth]
        b1 = (td * (1 + 0.15 * eps / np.maximum(np.abs(dc), 1e-300)) + ulp(T, 0.15 * eps))[smooth]
        assert np.all(e1 <= b1[:, None]), (c, (e1 - b1[:, None]).max())
    print(f"  faces compared for mu1: {kept}, left out on the medial axis: {left}")
    assert left <= 1e-3 * (kept + left)
    # every interior cell outside the band (rows the body never touched, rows it has left, far cells of touched rows) holds
    # exactly (1 or 0 by the sign of sigma, 0, 0); the first interior planes are left to BC!(mu0, 0)
    deep = np.zeros(sg.shape, dtype=bool)
    deep[2:-1, 2:-1, 2:-1] = True
    out = deep & ~band
    assert np.array_equal(mu0[out], np.where(sg[out] < 0, 0.0, 1.0)[:, None] * np.ones(3))
    assert not mu1[out].any() and not V[out].any()
    # nds (Metrics.jl:84-87) on the band list
    g = S._grid_of(sim.flow.p, 3)
    cd = sim.flow._band_cells[1]
    nds = torch.empty((cd.numel(), 3), dtype=torch.float64, device=cd.device)
    h, p = mb.native(tt, eps)
    _lib.check(_lib.lib().wl_body_nds_mesh(C.byref(g), h, C.byref(p), C.c_void_p(cd.data_ptr()), cd.numel(), C.c_void_p(nds.data_ptr())))
    dcn, nn, _, gap = mesh_ref.measure(ref, pose, Bc - 0.5, fastd2=1.0)
    # argwhere is row-major, the list column-major: order both the same way
    order = np.argsort(np.ravel_multi_index(tuple(Bc.T), sg.shape, order="F"))
    dcn, nn, gap = dcn[order], nn[order], gap[order]
    wn = nn * mesh_ref.kern(np.clip(dcn, -1, 1))[:, None]
    ok = (gap > 1e-9) & (np.abs(dcn) > 1e-6) & (np.abs(np.abs(dcn) - 1) > td)
    assert (~ok).sum() <= max(2, 1e-3 * len(ok)), ((~ok).sum(), len(ok))
    en = np.abs(nds.cpu().numpy() - wn)[ok]
    assert np.all(en <= (td * (np.pi / 2 + 1 / np.abs(dcn[ok])))[:, None])


def test_cube_mesh_equals_the_closure_box():
    """The cube mesh and an AutoBody closure of the exact box distance (torch device path), off-lattice pose."""
    a = 9.0
    amap = off_lattice_map(1.3)

    def box(x, t):
        q = torch.abs(x) - a / 2
        # (divided by the map's scale: the exact distance in x -- the closure path tests the RAW sdf against fastd2 and the
        #  band, AutoBody.jl:118, Body.jl:35, so a closure that returned the distance in xi would cut at another place)
        return (torch.sqrt((torch.clamp(q, min=0) ** 2).sum(0)) + torch.clamp(q.max(0).values, max=0)) / 1.3
    for T in (np.float32, np.float64):
        mk = lambda body: S.Simulation((48, 48, 48), (1.0, 0.0, 0.0), 8.0, body=body, nu=0.05, T=T)
        sm, sc = mk(MeshBody(*MS.cube((0.0, 0.0, 0.0), a), map=amap)), mk(B.AutoBody(box, amap))
        for s in (sm, sc):
            S.measure(s, 0.8)
        eps = geom_tol(T) / 4
        for k in ("mu0", "V"):
            w = S.to_host(getattr(sc.flow, k)).astype(np.float64)
            assert np.abs(S.to_host(getattr(sm.flow, k)).astype(np.float64) - w).max() <= 4 * eps * max(1.0, np.abs(w).max()), k
        sgc, sgm = S.to_host(sc.flow.sigma).astype(np.float64), S.to_host(sm.flow.sigma).astype(np.float64)
        zone = np.zeros(sgc.shape, dtype=bool)
        zone[1:-1, 1:-1, 1:-1] = True
        zone &= np.abs(sgc) < 3.9                                              # the mesh's exact zone (R = 4 cells in x)
        assert np.abs(sgm - sgc)[zone].max() <= 4 * eps * np.abs(sgc).max()
        sm2, sc2 = mk(MeshBody(*MS.cube((0.0, 0.0, 0.0), a), map=amap)), mk(B.AutoBody(box, amap))
        S.sim_step(sm2)
        S.sim_step(sc2)
        assert sm2.pois.n == sc2.pois.n
        same(sm2.flow.u, S.to_host(sc2.flow.u), exact=False, tol=50 * rtol(T))


def box_metric(N, L, amap):
    """The reference's two surface metrics (Metrics.jl:84-100, 128-134) for p = loc(0,I)[2] on an N^3 grid and a cube of
    edge L in xi = A x + b, from the CLOSED-FORM box distance and its gradient in numpy Float64 -- no product code:
    (pressure_force / L^3, pressure_moment about the cube's centre / L^4)."""
    A, b, _, _ = amap.coeffs(0.0)
    c = -A.T @ b
    i = np.arange(1, N + 1) - 0.5
    F, M = np.zeros(3), np.zeros(3)
    for zk in i:
        X = np.stack(np.meshgrid(i, i, [zk], indexing="ij"), -1).reshape(-1, 3)
        xi = X @ A.T + b
        q = np.abs(xi) - L / 2
        out = np.maximum(q, 0)
        no = np.linalg.norm(out, axis=1)
        d = no + np.minimum(q.max(1), 0)
        m = np.abs(d) < 1
        if not m.any():
            continue
        X, xi, q, out, no, d = X[m], xi[m], q[m], out[m], no[m], d[m]
        onehot = np.zeros_like(q)
        onehot[np.arange(len(q)), q.argmax(1)] = 1
        g = np.where((no > 0)[:, None], out / np.maximum(no, 1e-300)[:, None], onehot) * np.sign(xi)
        w = (g @ A) * mesh_ref.kern(d)[:, None]
        F += (X[:, 1:2] * w).sum(0)
        M += (X[:, 1:2] * np.cross(X - c, w)).sum(0)
    return F / L ** 3, M / L ** 4


@pytest.mark.parametrize("shape", ["cube", "icosphere"])
def test_reference_metric_known_answers_on_a_mesh(shape):
    """maintests.jl:341-346, 363-368 with the body a mesh: p = loc(0,I)[2] gives pressure_force / volume = (0,1,0) and no
    moment about the centroid, both within the reference's 2e-3 (summed absolute deviation); a uniform u no viscous force.

    Icosphere: subdivision 3, radius N/4 at N = 64 as the reference's sphere: force / volume = (0, 1.00130, 0).

    Cube: the kernel-smoothed surface integral is itself inexact at sharp edges, so the case is fixed by the reference's
    own error, taken from the closed-form box distance (box_metric above, no product code), not by the mesh code.  A cube
    of edge N/4 = 16 aligned with the lattice -- the first version of this case -- gives 0.97885 (deviation 2.1e-2, ten times
    the bound) with the closed-form distance exactly as with the mesh: its faces lie on cell boundaries, the cells on its
    diagonal planes count for one face only, and the deficit is O(1/edge).  Off the lattice the closed-form deviation is
    4.4e-2 at edge 16 (N = 64), 2.26e-3 at edge 54 (N = 128) and 1.26e-3 (moment 1.08e-3) at edge 80 (N = 192): the last
    is the smallest case in which the reference's metric meets its own bound, and the one used.  The test asserts that
    first, then holds the mesh to the same 2e-3 and to the closed-form figures themselves."""
    if shape == "cube":
        N, L = 192, 80.0
        c = np.array([N / 2 - 0.63, N / 2 + 0.91, N / 2 - 2.87])
        amap = B.rotation3d(c, (1.0, 2.0, 0.5), 0.0, th0=0.4)
        fb, mb_ = box_metric(N, L, amap)
        print(f"\nclosed-form box: force / volume = {fb}, moment / (volume L) = {mb_}")
        assert np.sum(np.abs(fb - np.array([0.0, 1.0, 0.0]))) < 2e-3 and np.sum(np.abs(mb_)) < 2e-3
        mb = MeshBody(*MS.cube((0.0, 0.0, 0.0), L), map=amap)
    else:
        N, L = 64, 16.0
        c = np.array([N / 2, N / 2, N / 2])
        mb = MeshBody(*MS.icosphere(c, L, 3))
    sim = S.Simulation((N, N, N), (1.0, 0.0, 0.0), 8.0, body=mb, T=np.float64, nu=0.1)
    p = np.zeros(tuple(sim.flow.N))
    p[...] = (np.arange(sim.flow.N[1]) - 0.5)[None, :, None]
    S.upload(sim.flow.p, p)
    vol = mb.volume
    f = S.pressure_force(sim)
    mom = S.pressure_moment(c, sim)
    print(f"\n{shape}: force / volume = {f / vol}, moment / (volume L) = {mom / (vol * L)}")
    assert np.sum(np.abs(S.viscous_force(sim))) < 1e-12                # sim.flow.u is the uniform (1, 0, 0)
    assert np.sum(np.abs(mom / (vol * L))) < 2e-3, mom
    assert np.sum(np.abs(f / vol - np.array([0.0, 1.0, 0.0]))) < 2e-3, f / vol
    if shape == "cube":
        # ~2e5 band cells, each term within tol_d (1 + 1/|d|) ~ 1e-11 of the closed form's times p <= N, over L^3: << 1e-8
        assert np.max(np.abs(f / vol - fb)) < 1e-8 and np.max(np.abs(mom / (vol * L) - mb_)) < 1e-8


@pytest.mark.parametrize("motion", ["translate", "spin"])
def test_moving_mesh_equals_moved_mesh(motion):
    v, t = SHAPES["torus"]()
    if motion == "translate":
        amap = lambda: B.translation(3, v=(0.9, 0.3, -0.2), s0=(20.3, 24.0, 23.6))
    else:
        amap = lambda: B.rotation3d((23.37, 24.91, 21.13), (1.0, 2.0, 0.5), 0.15, th0=0.4)
    mk = lambda: S.Simulation((48, 48, 48), (1.0, 0.0, 0.0), 8.0, body=MeshBody(v, t, map=amap()), nu=0.05, T=np.float32)

    def run():
        a, b = mk(), mk()
        forces = []
        for step in range(6):
            S.sim_step(a)                                              # measure! + update of the changed rows
            tm = float(np.sum(np.asarray(a.flow.dt[:-1], dtype=np.float64)))
            # a flow whose first and only measure! is at tm: every row is written (nothing "previous" exists)
            fresh = S.Flow((48, 48, 48), (1.0, 0.0, 0.0), nu=0.05, T=np.float32)
            fbody = MeshBody(v, t, map=amap())
            S.measure_flow(fresh, fbody, t=tm, eps=a.eps)
            for k in ("mu0", "mu1", "V"):
                assert torch.equal(getattr(a.flow, k), getattr(fresh, k)), (k, step)
            S.measure_flow(b.flow, b.body, t=tm, eps=b.eps)
            b._band = None
            S.update(b.pois)                                           # full update!
            S.mom_step(b.flow, b.pois)
            for k in ("D", "iD"):
                assert torch.equal(getattr(a.pois.levels[0], k), getattr(b.pois.levels[0], k)), (k, step)
            assert torch.equal(a.flow.u, b.flow.u) and torch.equal(a.flow.p, b.flow.p)
            del fresh, fbody
            forces.append(S.total_force(a))
        assert all(torch.isfinite(getattr(a.flow, k)).all() for k in ("u", "p", "mu0", "mu1", "V"))
        return np.array(forces)
    f1 = run()
    f2 = run()
    assert np.array_equal(f1, f2) and np.all(np.isfinite(f1)) and np.abs(f1).max() > 0


@pytest.mark.parametrize("motion", ["translate", "spin", "spin_scaled"])
def test_steady_moving_mesh_allocates_nothing(motion):
    """wl_prof_allocs does not grow from step 2 on, and the handle is the one built at the first measure!: the scale factor
    of a rotating map is recomputed in floating point at every step and must not rebuild the bins."""
    v, t = SHAPES["torus"]()
    rot = lambda: B.rotation3d((23.37, 24.91, 21.13), (1.0, 2.0, 0.5), 0.15, th0=0.4)
    amap = {"translate": lambda: B.translation(3, v=(0.9, 0.3, -0.2), s0=(20.3, 24.0, 23.6)), "spin": rot,
            "spin_scaled": lambda: B.scaled(rot(), 1.3)}[motion]()
    mb = MeshBody(v, t, map=amap)
    sim = S.Simulation((48, 48, 48), (1.0, 0.0, 0.0), 8.0, nu=0.05, T=np.float32, body=mb)
    h0 = mb._h.value
    L = _lib.lib()
    counts = []
    for step in range(12):
        S.sim_step(sim)
        S.total_force(sim)
        n, by = C.c_int64(), C.c_int64()
        assert L.wl_prof_allocs(C.byref(n), C.byref(by)) == 0
        counts.append(n.value)
    assert counts[1:] == [counts[1]] * 11, counts
    assert mb._h.value == h0


def test_slabs_match_undecomposed():
    """2 ranks sharing the GPU (tests/mesh_worker.py): gathered mu0, mu1, V of a spinning torus mesh equal the undecomposed
    run's bit for bit; V-cycle counts, dt and total_force after 3 steps under test_multi_gpu's comparison (Float32)."""
    from test_multi_gpu import run_workers
    out = run_workers("mesh_worker.py", 2, timeout=300)
    for k in ("mu0", "mu1", "V"):
        assert out["equal_" + k], (k, out)
    tol = 2e-5                                      # test_multi_gpu.check, Float32
    assert out["n_ref"] == out["n_slab"], out
    assert np.allclose(out["dt_ref"], out["dt_slab"], rtol=tol)
    assert np.allclose(out["force_ref"], out["force_slab"], rtol=100 * tol, atol=100 * tol), out


def test_icosphere_flows_like_a_sphere():
    """Subdivision 4, radius 16 on 96x64x64, Re 250, 20 steps next to the parametric Sphere: finite fields, drag of the same
    sign, V-cycle counts within +-1 per step (the relative drag difference is recorded by tools/mesh_bench.py)."""
    dims, r, c = (96, 64, 64), 16.0, (32.0, 32.0, 32.0)
    mk = lambda body: S.Simulation(dims, (1.0, 0.0, 0.0), 2 * r, body=body, nu=2 * r / 250, T=np.float32)
    sm, sp = mk(MeshBody(*MS.icosphere(c, r, 4))), mk(B.Sphere(c, r, 3))
    for _ in range(20):
        S.sim_step(sm, remeasure=False)
        S.sim_step(sp, remeasure=False)
    assert all(torch.isfinite(getattr(sm.flow, k)).all() for k in ("u", "p"))
    fm, fs = S.total_force(sm), S.total_force(sp)
    print(f"\nicosphere vs sphere: drag {fm[0]:.6g} vs {fs[0]:.6g}, |dF|/|F| = {abs(fm[0] - fs[0]) / abs(fs[0]):.3e}")
    assert fm[0] * fs[0] > 0
    assert len(sm.pois.n) == len(sp.pois.n) and np.max(np.abs(np.array(sm.pois.n) - np.array(sp.pois.n))) <= 1, (sm.pois.n, sp.pois.n)
