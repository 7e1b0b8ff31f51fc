"""Forces on the GPU: the fused kernels behind wl_band_loads / wl_body_loads / wl_body_loads_mesh against the
extended-precision restatement tests/forces_ref.py, and the recorder of waterlily_amd/forces.py.
  * stored-band path on synthetic bands, decoupled from any geometry: every column within its bound
    (K * eps_T + tree_adds(n) * eps_64 / 2) * M, for band lengths around the wavefront and workgroup sizes and one past the
    launch cap, both types, 2-D and 3-D, pitched and dense, the field kinds of xref_metrics.KINDS;
  * native path (parametric, composite, mesh) against the restatement fed with host copies of p, u and the band that the
    composed path (sim._band_of) builds;
  * pins that need no tolerance, the power of a translating body, the leaves of a composite, the NaN rule, a live run with a
    growing buffer, z-slabs (tests/forces_worker.py).
The references are computed once per input and shared by the layouts."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import forces_ref as R
import mesh_shapes
import xref_metrics as XM
from test_xref_gpu import dev
from waterlily_amd import body as B
from waterlily_amd import forces as F
from waterlily_amd import sim as S
from waterlily_amd.mesh import MeshBody
from xref_inputs import field

TYPES = [np.float32, np.float64]
WORST = {}

# workgroups of 256 threads: the launch cap FORCES_CAP of csrc/wl_forces.h (test_launch_cap_is_the_one_in_the_source)
CAP = 512
NBANDS = [0, 1, 63, 64, 65, 255, 256, 257]
NBIG = CAP * 256 + 513                                                # the grid-stride loop and a final stage of CAP partials
BAND_GRIDS = [(11, 9, 7), (69, 8, 6), (132, 7), (13, 11)]             # interior (9,7,5), (67,6,4), (130,5), (11,9)
BIG_GRIDS = [(11, 9, 7), (13, 11)]                                    # the long band: one 3-D and one 2-D grid
ZERO_2D = [2, 5, 6, 7, 9, 10]                                         # Fp_z, Fv_z, Mp_x, Mp_y, Mv_x, Mv_y


def test_launch_cap_is_the_one_in_the_source():
    src = open(os.path.join(os.path.dirname(S.__file__), "csrc", "wl_forces.h")).read()
    assert re.findall(r"constexpr int FORCES_CAP = (\d+);", src) == [str(CAP)]


def note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), float(np.max(r)))


@functools.lru_cache(maxsize=None)
def band_case(tn, Ng, nband, kind):
    T = np.dtype(tn).type
    D = len(Ng)
    idx, nds = XM.synthetic_band(Ng, nband, 40 + nband % 1000)
    p, u = field(Ng, T, kind, 41), field(Ng + (D,), T, kind, 42)
    nu = float(T(0.37))
    x0 = XM.X0[:D]
    return idx, nds, p, u, nu, x0, R.rows(p, u, nu, x0, idx, nds)


def band_loads(T, D, pd, ud, bi, bn, nu, x0):
    rows = torch.full((2, 16), 7.0, dtype=torch.float64, device=pd.device)
    S.check(S._lib.lib().wl_band_loads(S._WLT[np.dtype(T)], C.byref(S._grid_of(pd, D)), S._ptr(pd), S._ptr(ud), nu, S._ptr(bi), S._ptr(bn),
                                       bi.numel(), S.d3(x0), S._ptr(rows)))
    return rows.cpu().numpy()


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("padded", [True, False])
@pytest.mark.parametrize("Ng", BAND_GRIDS)
def test_stored_band_hip_vs_ref(T, padded, Ng):
    """wl_band_loads on synthetic bands (cells next to every ghost layer first, nds uniform in [-1, 1], x0 asymmetric and off
    the half-integers): all 16 columns of both rows within their bound, lengths 0 (no launch: zero rows), 1, 63..65, 255..257 and
    -- on one 3-D and one 2-D grid -- cap*256 + 513; Wp, Wv NaN (no V); 2-D: the unused slots exactly 0.  Controls: the
    list shifted by one against nds, and x0 with two components swapped, fail."""
    tn = np.dtype(T).name
    D = len(Ng)
    for nband in NBANDS + ([NBIG] if Ng in BIG_GRIDS else []):
        # (the long band on "random" and "ties" only: the scaled kinds are "random" times a power of two, which changes no
        #  rounding, and each long reference costs seconds)
        for kind in (XM.KINDS if nband != NBIG else XM.KINDS[:2]):
            idx, nds, p, u, nu, x0, (v, M, n) = band_case(tn, Ng, nband, kind)
            pd, ud = dev(p, D, padded), dev(u, D, padded)
            bi, bn = S.band_to_device(pd, idx, nds)
            got = band_loads(T, D, pd, ud, bi, bn, nu, x0)
            assert got[0].tobytes() == got[1].tobytes()                       # one leaf: the total is row 0, bit for bit
            r = R.ratios(got[0], v[0], M[0], n[0], T, adds=XM.tree_adds(nband, CAP))
            for c in range(16):
                note(f"band {R.COLK[c]} {tn}", r[c])
            assert r.max() <= 1, f"{tn} {Ng} n={nband} {kind}: {dict(zip(R.COLUMNS, np.round(r, 3)))}"
            assert np.isnan(got[:, 12:14]).all() and got[0, 14] == nband
            if nband == 0:
                assert not np.delete(got, [12, 13], axis=1).any()
            if D == 2:
                assert not got[:, ZERO_2D].any()
            if 255 <= nband <= 257 and kind == "random":
                vs, Ms, ns = R.rows(p, u, nu, x0, np.roll(idx, 1), nds)
                rs = R.ratios(got[0], vs[0], Ms[0], ns[0], T)
                assert rs[0] > 1 and rs[3] > 1 and rs[8] > 1 and rs[11] > 1
                vx, Mx, nx = R.rows(p, u, nu, (x0[1], x0[0]) + tuple(x0[2:]), idx, nds)
                rx = R.ratios(got[0], vx[0], Mx[0], nx[0], T)
                assert rx[8] > 1 and rx[11] > 1 and rx[:6].max() <= 1


def test_stored_band_skips_zero_vectors_and_repeats_its_bits():
    """an entry whose nds vector is zero is left before p or u is read (NaN there changes nothing) and is not counted; two
    calls give the same bits"""
    T, Ng = np.float32, (11, 9, 7)
    idx, nds, p, u, nu, x0, _ = band_case("float32", Ng, 257, "random")
    nds = nds.copy()
    nds[[3, 100, 256]] = 0.0
    p2, u2 = p.copy(), u.copy()
    assert np.unique(idx).size == idx.size                             # (257 of 315 inside cells: none repeated)
    sub = np.unravel_index(idx[[3, 100, 256]], Ng, order="F")
    p2[sub] = np.nan
    u2[sub] = np.nan
    pd, ud = dev(p, 3, True), dev(u, 3, True)
    bi, bn = S.band_to_device(pd, idx, nds)
    a = band_loads(T, 3, pd, ud, bi, bn, nu, x0)
    b = band_loads(T, 3, pd, ud, bi, bn, nu, x0)
    assert a.tobytes() == b.tobytes() and a[0, 14] == idx.size - 3
    pn = dev(p2, 3, True)
    c = band_loads(T, 3, pn, ud, bi, bn, nu, x0)
    assert np.array_equal(np.delete(c, [12, 13], 1), np.delete(a, [12, 13], 1))
    # u is read at the neighbours too: a NaN in u at a skipped cell reaches its counted neighbours only (Fv, Mv), never Fp, Mp
    un = dev(u2, 3, True)
    d = band_loads(T, 3, pd, un, bi, bn, nu, x0)
    assert np.array_equal(d[:, [0, 1, 2, 6, 7, 8, 14, 15]], a[:, [0, 1, 2, 6, 7, 8, 14, 15]])


# ------------------------------------------------------------------------------------------------ native bodies

C3 = (10.3, 9.2, 8.1)
VT = (0.5, -0.25, 0.125)                                              # the translating sphere's velocity (dyadic)


def make_body(name):
    if name == "circle-2d":
        return (24, 20), 0.0, B.Sphere((11.3, 9.2), 4.1, 2)
    if name == "sphere-moving":                                       # radius 5: the band holds more than 256 cells
        return (24, 20, 20), 1.37, B.Sphere((9.8, 9.4, 8.9), 5.0, 3, map=B.translation(3, v=VT))
    if name == "plate-rotating":
        return (20, 20, 16), 1.37, B.Plate(3.3, 1.2, 3, map=B.rotation3d(C3, (0.3, -0.5, 0.8), 0.21, 0.4))
    if name == "composite":                                           # two disjoint spheres, a cylinder cut out of the first
        return (32, 16, 16), 0.0, B.Bodies([B.Sphere((8.3, 8.2, 7.1), 4.2, 3), B.Sphere((21.4, 7.7, 6.9), 3.6, 3),
                                            B.Cylinder((8.3, 8.2, 7.1), 1.7, 3)], ["+", "-"])
    if name == "two-spheres":
        return (32, 16, 16), 0.0, B.Bodies([B.Sphere((8.3, 8.2, 7.1), 4.2, 3), B.Sphere((21.4, 7.7, 6.9), 3.6, 3)], ["+"])
    if name == "mesh":
        v, t = mesh_shapes.icosphere((9.3, 8.2, 7.6), 4.3, sub=2)
        return (20, 20, 16), 0.0, MeshBody(v, t)
    raise KeyError(name)


def make_sim(name, T, body=None):
    """a Simulation whose body stands at time t (set the way sim_step does: measure! at sum(dt), then one more dt) and whose
    p and u are random fields"""
    dims, t, b = make_body(name)
    sim = S.Simulation(dims, (1.0,) + (0.0,) * (len(dims) - 1), 8.0, nu=0.37, body=b if body is None else body, T=T)
    if t:
        sim.flow.dt = [t]
        S.measure(sim)
        sim.flow.dt.append(0.25)
    Ng = tuple(n + 2 for n in dims)
    S.upload(sim.flow.p, field(Ng, T, "random", 51))
    S.upload(sim.flow.u, field(Ng + (len(dims),), T, "random", 52))
    return sim


def host_band(sim):
    """(dense column-major indices, nds) of the band the composed path builds, at the host"""
    idx, nds = S._band_of(sim)
    p = sim.flow.p
    off = idx.cpu().numpy()
    sub = []
    for d in range(p.ndim - 1, -1, -1):
        sub.append(off // int(p.stride()[d]))
        off = off % int(p.stride()[d])
    lin = np.ravel_multi_index(tuple(reversed(sub)), tuple(p.shape), order="F")
    return lin, nds.cpu().numpy()


NATIVE = ["circle-2d", "sphere-moving", "plate-rotating", "composite", "mesh"]


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", NATIVE)
def test_native_hip_vs_ref(T, name):
    """loads(sim) of a native body against the restatement on host copies of p, u and the downloaded band of the composed
    path: Fp, Fv, Mp (and Mv, A) within their bounds, ncells the band's length exactly; two calls, the same bits; the total row
    is row 0 + row 1 + .. bit for bit; 2-D: the unused slots exactly 0"""
    sim = make_sim(name, T)
    D = sim.flow.D
    x0 = XM.X0[:D]
    L = F.loads(sim, x0)
    rows = L["leaves"]
    assert rows.tobytes() == F.loads(sim, x0)["leaves"].tobytes()
    nl = rows.shape[0] - 1
    assert nl == (3 if name == "composite" else 1)
    tot = rows[0].copy()
    for q in range(1, nl):
        tot = tot + rows[q]
    assert tot.tobytes() == rows[-1].tobytes()
    lin, nds = host_band(sim)
    assert (257 if name == "sphere-moving" else 1) <= lin.size == L["ncells"] == int(rows[:-1, 14].sum())
    p, u = S.to_host(sim.flow.p), S.to_host(sim.flow.u)
    v, M, n = R.rows(p, u, sim.flow.nu, x0, lin, nds)
    r = R.ratios(rows[-1], v[-1], M[-1], n[-1], T, adds=XM.tree_adds(int(sim.flow._band_cells[1].numel()), CAP) + nl)
    r[12:14] = 0                                                      # (the restatement was given no V)
    for c in range(16):
        note(f"native {R.COLK[c]} {np.dtype(T).name}", r[c])
    assert r.max() <= 1, f"{name}: {dict(zip(R.COLUMNS, np.round(r, 3)))}"
    assert np.isfinite(rows).all()
    assert np.array_equal(L["Fp"], rows[-1, :D]) and np.array_equal(L["Fv"], rows[-1, 3:3 + D]) and L["area"] == rows[-1, 15]
    if D == 2:
        assert not rows[:, ZERO_2D].any() and L["Mp"] == rows[-1, 8] and L["Mv"] == rows[-1, 11]
    # control: the same rows against the band shifted by one cell along x
    vs, Ms, ns = R.rows(p, u, sim.flow.nu, x0, lin + 1, nds)
    assert R.ratios(rows[-1], vs[-1], Ms[-1], ns[-1], T)[0] > 1


@pytest.mark.parametrize("T", TYPES)
def test_rigid_rotation_has_no_viscous_load(T):
    """u a rigid rotation with dyadic rates, sampled at the half-integer face positions: every d(i,j) + d(j,i) is exactly 0, so
    Fv, Mv and Wv are exactly +-0, on the moving sphere (V != 0)"""
    sim = make_sim("sphere-moving", T)
    Ng = tuple(sim.flow.p.shape)
    A = np.array([[0, -0.5, 0.25], [0.5, 0, -1.0], [-0.25, 1.0, 0]])
    S.upload(sim.flow.u, XM.linear_field(Ng, T, A, (0.5, -0.25, 0.125)))
    rows = F.loads(sim, XM.X0)["leaves"]
    assert not rows[:, [3, 4, 5, 9, 10, 11, 13]].any() and rows[-1, :3].all() and rows[-1, 12] != 0


@pytest.mark.parametrize("T", TYPES)
def test_power_of_a_translating_body(T):
    """V = v at every cell of a translating body: Wp = Fp . v and Wv = Fv . v within the summation bound of the restatement"""
    sim = make_sim("sphere-moving", T)
    rows = F.loads(sim, XM.X0)["leaves"]
    lin, nds = host_band(sim)
    p, u = S.to_host(sim.flow.p), S.to_host(sim.flow.u)
    V = np.broadcast_to(np.array(VT), nds.shape)
    v, M, n = R.rows(p, u, sim.flow.nu, XM.X0, lin, nds, V=V)
    r = R.ratios(rows[-1], v[-1], M[-1], n[-1], T, adds=XM.tree_adds(int(sim.flow._band_cells[1].numel()), CAP) + 1)
    assert r[12] <= 1 and r[13] <= 1, r
    e64 = np.finfo(np.float64).eps
    assert abs(v[-1, 12] - v[-1, :3] @ np.array(VT)) <= 4 * e64 * M[-1, 12] and abs(v[-1, 13] - v[-1, 3:6] @ np.array(VT)) <= 4 * e64 * M[-1, 13]
    # control: the velocity reversed fails
    vr, Mr, nr = R.rows(p, u, sim.flow.nu, XM.X0, lin, nds, V=-V)
    assert R.ratios(rows[-1], vr[-1], Mr[-1], nr[-1], T)[12] > 1


def _single(T, q):
    """a Simulation holding leaf q of the two-sphere composite alone, with the same p and u"""
    body = make_body("two-spheres")[2].bodies[q]
    return make_sim("two-spheres", T, body=body)


@pytest.mark.parametrize("T", TYPES)
def test_leaves_are_the_bodies_of_a_disjoint_union(T):
    """each leaf row of the two-sphere composite against the row of a Simulation holding that sphere alone with the same p
    and u: the same terms summed in another order.  Each sum is within adds * eps_64 / 2 * M of the exact sum of those
    terms, so the two are apart by at most the bound with the two chains of additions added; ncells exactly"""
    sim = make_sim("two-spheres", T)
    rows = F.loads(sim, XM.X0)["leaves"]
    assert rows.shape == (3, 16) and rows[0, 14] > 0 and rows[1, 14] > 0
    for q in range(2):
        one = _single(T, q)
        alone = F.loads(one, XM.X0)["leaves"][-1]
        lin, nds = host_band(one)
        v, M, n = R.rows(S.to_host(one.flow.p), S.to_host(one.flow.u), one.flow.nu, XM.X0, lin, nds)
        assert alone[14] == rows[q, 14] == lin.size
        t = R.tol(n[-1], M[-1], T, adds=XM.tree_adds(int(sim.flow._band_cells[1].numel()), CAP) + 2
                  + XM.tree_adds(int(one.flow._band_cells[1].numel()), CAP) + 1)
        d = np.abs(alone - rows[q])
        ok = (d <= t) | np.isnan(t)
        ok[12:14] = (alone[12:14] == 0) & (rows[q, 12:14] == 0)               # static bodies: no power, exactly
        assert ok.all(), (q, d, t)
        assert np.abs(alone[:3] - rows[1 - q, :3]).max() > t[:3].max()        # control: the other leaf is another load


@pytest.mark.parametrize("T", TYPES)
def test_nan_rule(T):
    """a NaN in p at a counted cell of leaf 1: Fp, Mp, Wp of leaf 1 and of the total are NaN and nothing else changes; a NaN in
    p and u at candidates of measure! that are not counted (1 <= |d| < 2 + eps) and touch no counted cell changes nothing"""
    sim = make_sim("two-spheres", T)
    base = F.loads(sim, XM.X0)["leaves"]
    one = _single(T, 1)
    off = S._band_of(one)[0]
    cell = int(off[off.numel() // 2])
    flat = torch.as_strided(sim.flow.p, (cell + 1,), (1,))
    keepv = float(flat[cell])
    flat[cell] = float("nan")
    got = F.loads(sim, XM.X0)["leaves"]
    flat[cell] = keepv
    hit = [0, 1, 2, 6, 7, 8, 12]
    assert np.isnan(got[1:, hit]).all()
    rest = np.ones((3, 16), bool)
    rest[1:, hit] = False
    assert np.array_equal(got[rest], base[rest]) and np.isfinite(got[rest]).all()
    # a candidate of measure! that is not counted (1 <= |d| < 2 + eps)
    lin, _ = host_band(sim)
    cand = sim.flow._band_cells[1].cpu().numpy()
    Ng = tuple(sim.flow.p.shape)
    near = np.zeros(int(np.prod(Ng)), bool)
    near[lin] = True
    near = near.reshape(Ng, order="F")
    grown = near.copy()
    for sh in np.ndindex(3, 3, 3):                                    # the 3x3x3 cells whose u a counted cell's stencil reads
        grown |= np.roll(near, tuple(q - 1 for q in sh), (0, 1, 2))
    out = np.setdiff1d(cand, np.flatnonzero(grown.ravel(order="F")))
    assert out.size > 100
    sub = np.unravel_index(out, Ng, order="F")
    hp, hu = S.to_host(sim.flow.p), S.to_host(sim.flow.u)
    hp[sub] = np.nan
    hu[sub] = np.nan
    S.upload(sim.flow.p, hp)
    S.upload(sim.flow.u, hu)
    assert F.loads(sim, XM.X0)["leaves"].tobytes() == base.tobytes()
    # ... while a counted cell's own p is read: the control of the above
    hp[np.unravel_index(lin[0], Ng, order="F")] = np.nan
    S.upload(sim.flow.p, hp)
    assert np.isnan(F.loads(sim, XM.X0)["leaves"][-1, 0])


def test_live_run_records_what_loads_returns():
    """a moving 2-D circle, 10 steps, capacity 2 (the buffer grows three times): series rows equal loads(sim) taken at each
    step bit for bit, record leaves u and p alone, and loads(sim)["Fp"] is pressure_force(sim) within the summation bound"""
    T = np.float32
    body = B.Sphere((14.3, 12.2), 4.1, 2, map=B.translation(2, v=(0.25, 0.0)))
    sim = S.Simulation((40, 24), (1.0, 0.0), 8.2, nu=8.2 / 250, body=body, T=T)
    x0 = (14.3, 12.2)
    fr = F.Forces(sim, x0=x0, capacity=2)
    each, times = [], []
    for k in range(10):
        S.sim_step(sim)
        u0, p0 = sim.flow.u.clone(), sim.flow.p.clone()
        F.record(fr, sim)
        assert torch.equal(u0, sim.flow.u) and torch.equal(p0, sim.flow.p)
        each.append(F.loads(sim, x0)["leaves"])
        times.append(S.time(sim.flow))
    t, v = F.series(fr)
    assert fr.buf.shape[0] == 16 and v.shape == (10, 2, 16) and t.tolist() == times
    assert v.tobytes() == np.stack(each).tobytes()
    assert np.isfinite(v).all() and v[:, -1, 12].any() and (v[:, -1, 14] > 20).all()
    pf = S.pressure_force(sim)
    lin, nds = host_band(sim)
    rv, rM, rn = R.rows(S.to_host(sim.flow.p), S.to_host(sim.flow.u), sim.flow.nu, x0, lin, nds)
    ncand = int(sim.flow._band_cells[1].numel())
    tol = R.tol(rn[-1], rM[-1], T, adds=XM.tree_adds(ncand, CAP) + 1 + XM.tree_adds(lin.size, 1024))[:2]   # two sums of the same terms
    assert (np.abs(each[-1][-1, :2] - pf) <= tol).all(), (each[-1][-1, :2], pf, tol)
    assert np.abs(v[0, -1, :2] - v[-1, -1, :2]).max() > tol.max()              # the series moves: not one row ten times
    F.reset(fr)
    assert F.series(fr)[1].shape == (0, 2, 16)


def test_closure_body_takes_the_stored_band():
    """a body given as torch closures goes through sim._band_of and wl_band_loads: Fp is pressure_force(sim) within the
    summation bound, Wp and Wv are NaN"""
    from waterlily_amd.body import AutoBody, norm2
    T = np.float64
    sim = S.Simulation((24, 20), (1.0, 0.0), 8.0, nu=0.37, body=AutoBody(lambda x, t: norm2(x - 9.7) - 4.1), T=T)
    S.upload(sim.flow.p, field((26, 22), T, "random", 51))
    S.upload(sim.flow.u, field((26, 22, 2), T, "random", 52))
    assert not F._native(sim)
    L = F.loads(sim)
    lin, nds = host_band(sim)
    v, M, n = R.rows(S.to_host(sim.flow.p), S.to_host(sim.flow.u), sim.flow.nu, (0.0, 0.0), lin, nds)
    r = R.ratios(L["leaves"][-1], v[-1], M[-1], n[-1], T, adds=XM.tree_adds(lin.size, CAP))
    assert r.max() <= 1 and np.isnan(L["Wp"]) and np.isnan(L["Wv"]) and L["ncells"] == lin.size > 20
    assert (np.abs(L["Fp"] - S.pressure_force(sim)) <= R.tol(n[-1], M[-1], T, adds=XM.tree_adds(lin.size, CAP) + XM.tree_adds(lin.size, 1024))[:2]).all()


def test_slabs():
    """2 ranks sharing the GPU (tests/forces_worker.py)"""
    from test_multi_gpu import run_workers
    out = run_workers("forces_worker.py", 2, timeout=300)
    assert out["t_equal"] and out["rows"] == 3, out
    assert out["ncells_equal"] and out["within_bound"] and out["worst"] <= 1.0, out
    assert out["local_rows_differ"] and out["one_off_equal"], out


def test_worst_ratios_are_recorded():
    """(prints the largest share of its bound seen per column kind in this module: -s shows it)"""
    print("\nworst |got-ref|/tol:", {k: round(v, 4) for k, v in sorted(WORST.items())})
