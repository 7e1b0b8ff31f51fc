"""SurfaceLoads on the GPU (waterlily_amd.surface: wl_surface_sample, wl_surface_totals) against closed forms on linear fields,
against the numpy restatement tests/surface_ref.py on seeded random fields, the NaN rule, the totals, recording during a run
of a rotating mesh, and a 2-rank slab pair.

Bounds are derived, not measured; test_surface_cpu.py's docstring holds the derivation and the helpers.  Both sides work in
double on operands <= L: positions agree within td = 64 * 2^-52 * L, unit normals within err_n = 16 td / (smallest altitude), a
sample point within pos = td + delta err_n.  Linear fields (test 1) add the storage rounding ulp_T(max |field|) per sample,
weighted by sum |S| for the totals: tol_linear.  On the same stored random field (test 2) a sample moves by at most
3 pos * (largest neighbour difference) + 16 * 2^-52 * max |field|, tau reads 12 samples: tol_sampled; nothing is left out of
the comparison.  Totals against the numpy sums of the device's own rows: nt * 2^-52 * sum |terms|.

Cases: 40x32x24, f32 and f64, padded and dense, cube / icosphere(2) / lprism, identity pose and off_lattice_map(1.3) at
t = 0.8, each at two placements (test_surface_cpu.PLACES): the issue's off-lattice centre, where a body must be smaller than
a cell to keep its samples inside the 24-cell z extent, and the same lattice fractions at the middle of the domain with the
shapes at test_mesh_cpu's sizes.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_shapes as MS  # noqa: E402
import surface_ref as SR  # noqa: E402
from test_surface_cpu import (CENTRE, CU_LIN, C_LIN, DIMS, EPS, G_LIN, M_LIN, NU, PLACES, body_of, make_sim, pose_of,  # noqa: E402
                              random_fields, scales, tol_linear, tol_sampled)

from waterlily_amd import _lib, body as B, sim as S, surface  # noqa: E402
from waterlily_amd.mesh import MeshBody  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
NG = tuple(n + 2 for n in DIMS)
SHAPES3 = ["cube", "icosphere", "lprism"]
X0 = (17.5, 20.25, 9.0)                               # a reference point that is no centroid


@functools.lru_cache(maxsize=None)
def geo_of(shape, posed, place):
    mb = body_of(shape, posed, place)
    return SR.geometry(mb.vertices, mb.triangles, pose_of(mb, posed)[0])


@functools.lru_cache(maxsize=None)
def fields_of(kind, T):
    if kind == "linear":
        return SR.linear_fields(NG, G_LIN, C_LIN, M_LIN, CU_LIN, T)
    return random_fields(17, T)


@functools.lru_cache(maxsize=None)
def ref_of(shape, posed, place, kind, T, delta):
    """surface_ref's sample of a case, computed once and shared (read-only)"""
    p, u = fields_of(kind, T)
    return SR.sample(geo_of(shape, posed, place), p, u, delta, NU)


def device(shape, posed, place, kind, T, padded, delta, x0=(0.0, 0.0, 0.0), mean=False):
    mb = body_of(shape, posed, place)
    sim = make_sim(mb, T, padded, t=pose_of(mb, posed)[1])
    p, u = fields_of(kind, T)
    S.upload(sim.flow.p, p)
    S.upload(sim.flow.u, u)
    sl = surface.SurfaceLoads(sim, delta=delta, x0=x0, mean=mean)
    surface.record(sl, sim)
    return mb, sim, sl


GRID = [(s, po, pl, T, pad) for s in SHAPES3 for po in (False, True) for pl in sorted(PLACES) for T in (F32, F64) for pad in (True, False)]
IDS = [f"{s}-{'posed' if po else 'identity'}-{pl}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for s, po, pl, T, pad in GRID]


@pytest.mark.parametrize("shape,posed,place,T,padded", GRID, ids=IDS)
def test_exact_identities_on_linear_fields(shape, posed, place, T, padded):
    """p = g.x + c, u = M x + c at the faces: Fp = g Vol_x at delta = 0, tau = -nu (M + M^T) n per triangle at any delta,
    Fv = 0, p_t = g.x_s + c: the sign and the transform of every term."""
    geo = geo_of(shape, posed, place)
    p, u = fields_of("linear", T)
    want_tau = -NU * geo["n"] @ (M_LIN + M_LIN.T).T
    for delta in (0.0, 0.6, 1.5):
        mb, sim, sl = device(shape, posed, place, "linear", T, padded, delta)
        f = surface.fields(sl)
        tot = surface.series(sl)[1][0]
        ttau, tfp, tfv = tol_linear(T, mb, geo, delta, p, u)
        L, td, err_n, _ = scales(mb, geo)
        xs = geo["centroid"] + delta * geo["n"]
        ep = tfp / geo["area"].sum()                   # (>= the per-sample bound e_s + |g|_1 pos that tfp is built from)
        d_tau, d_p = np.abs(f["traction"] - want_tau).max(), np.abs(f["p"] - (xs @ G_LIN + C_LIN)).max()
        print(f"\ndelta={delta}: |tau - want| {d_tau:.3e} (bound {ttau:.3e}), |p - want| {d_p:.3e} (bound {ep:.3e}), "
              f"|Fv| {np.abs(tot[3:6]).max():.3e} (bound {tfv:.3e})")
        assert np.all(np.isfinite(f["p"])) and np.all(np.isfinite(f["traction"]))      # the body stays inside the domain
        assert d_tau <= ttau and d_p <= ep
        assert np.abs(tot[3:6]).max() <= tfv
        if delta == 0.0:
            s = 1.0 if mb.amap is None else mb.coeffs(0.8)[5]
            want = G_LIN * mb.volume / s ** 3
            print(f"  Fp {tot[:3]} want {want} (bound {tfp:.3e})")
            assert np.abs(tot[:3] - want).max() <= tfp


def compare_with_ref(f, geo, ref, tols):
    tp, ttau, tx, tS, tV = tols
    pt, tau, _ = ref
    for name, got, want, tol in (("p", f["p"], pt, tp), ("traction", f["traction"], tau, ttau), ("centroid", f["centroid"], geo["centroid"], tx),
                                 ("area_vector", f["area_vector"], geo["S"], tS), ("body_velocity", f["body_velocity"], geo["Vb"], tV)):
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        k = ~np.isnan(want)
        d = np.abs(got[k] - want[k]).max(initial=0.0)
        print(f"  {name}: max |device - ref| = {d:.3e} (bound {tol:.3e})")
        assert d <= tol, name


@pytest.mark.parametrize("shape,posed,place,T,padded", GRID, ids=IDS)
def test_random_fields_against_the_reference(shape, posed, place, T, padded):
    geo = geo_of(shape, posed, place)
    p, u = fields_of("random", T)
    for delta in (0.0, 1.5):
        mb, sim, sl = device(shape, posed, place, "random", T, padded, delta)
        ref = ref_of(shape, posed, place, "random", T, delta)
        assert np.all(np.isfinite(ref[0])) and np.all(np.isfinite(ref[1]))
        print(f"\ndelta={delta}")
        compare_with_ref(surface.fields(sl), geo, ref, tol_sampled(mb, geo, delta, p, u))
        if posed:
            assert np.abs(geo["Vb"]).max() > 1e-3                                    # the moving pose has a body velocity to compare


@pytest.mark.parametrize("T", [F32, F64])
def test_nan_rule(T):
    """The icosphere at SHAPES' size about the issue's centre reaches past the last z plane: those triangles are NaN, in exactly
    the entries the reference marks, every other entry is within the bound, and the totals are NaN."""
    v, t = MS.icosphere((0.0, 0.0, 0.0), 7.0, 2)
    mb = MeshBody(v + CENTRE, t)
    geo = SR.geometry(mb.vertices, mb.triangles, None)
    p, u = fields_of("random", T)
    sim = make_sim(mb, T, True)
    S.upload(sim.flow.p, p)
    S.upload(sim.flow.u, u)
    sl = surface.SurfaceLoads(sim, delta=1.5, x0=X0)
    surface.record(sl, sim)
    ref = SR.sample(geo, p, u, 1.5, NU)
    nan_p, nan_tau = int(np.isnan(ref[0]).sum()), int(np.isnan(ref[1]).any(1).sum())
    print(f"\n{nan_p} of {len(t)} triangles without a pressure, {nan_tau} without a traction")
    assert 0 < nan_p <= nan_tau < len(t)
    compare_with_ref(surface.fields(sl), geo, ref, tol_sampled(mb, geo, 1.5, p, u))
    assert np.all(np.isnan(surface.series(sl)[1][0]))


def test_totals():
    """the twelve totals: the numpy sums of the device's own rows, the same bits twice, and the reference's moments about a
    point that is not the centroid"""
    shape, posed, place, T = "icosphere", True, "mid", F64
    geo = geo_of(shape, posed, place)
    p, u = fields_of("random", T)
    mb, sim, sl = device(shape, posed, place, "random", T, True, 1.5, x0=X0)
    surface.record(sl, sim)
    t, v = surface.series(sl)
    assert len(t) == 2 and np.array_equal(v[0], v[1])
    f = surface.fields(sl)
    nt = len(f["p"])
    area = np.linalg.norm(f["area_vector"], axis=1)
    fp, fv = f["p"][:, None] * f["area_vector"], f["traction"] * area[:, None]
    d = f["centroid"] - np.array(X0)
    host = np.concatenate([fp.sum(0), fv.sum(0), np.cross(d, fp).sum(0), np.cross(d, fv).sum(0)])
    cr = lambda a, b: np.stack([np.abs(a[:, 1] * b[:, 2]) + np.abs(a[:, 2] * b[:, 1]), np.abs(a[:, 2] * b[:, 0]) + np.abs(a[:, 0] * b[:, 2]),
                                np.abs(a[:, 0] * b[:, 1]) + np.abs(a[:, 1] * b[:, 0])], 1)
    terms = np.concatenate([np.abs(fp).sum(0), np.abs(fv).sum(0), cr(d, fp).sum(0), cr(d, fv).sum(0)])
    print("\ntotals", v[0], "\n|device - numpy|", np.abs(v[0] - host), "\nbound", nt * EPS * terms)
    assert np.all(np.abs(v[0] - host) <= nt * EPS * terms)
    # against the reference: every row within tol_sampled, weighted by |S| and the lever arm
    tp, ttau, tx, tS, _ = tol_sampled(mb, geo, 1.5, p, u)
    pt, tau, _ = ref_of(shape, posed, place, "random", T, 1.5)
    Fp, Fv, Mp, Mv = SR.totals(geo, pt, tau, X0)
    sa, dmax = geo["area"].sum(), np.abs(geo["centroid"] - np.array(X0)).max() + tx
    bF = lambda tol, F: sa * tol + nt * tS * F + nt * EPS * F * sa
    bp, bv = bF(tp, np.abs(pt).max()), bF(ttau, np.abs(tau).max())
    for name, got, want, b in (("Fp", v[0][0:3], Fp, bp), ("Fv", v[0][3:6], Fv, bv), ("Mp", v[0][6:9], Mp, 2 * dmax * bp + 2 * tx * np.abs(pt).max() * sa),
                               ("Mv", v[0][9:12], Mv, 2 * dmax * bv + 2 * tx * np.abs(tau).max() * sa)):
        print(f"  {name}: {got} ref {want} bound {b:.3e}")
        assert np.abs(got - want).max() <= b, name
    assert np.abs(Mp).max() > 1e-3 and np.abs(Mv).max() > 1e-5
    # loads(): the same numbers by name
    one = surface.loads(sim, delta=1.5, x0=X0)
    assert tuple(one) == surface.columns(sl) and np.array_equal(np.array(list(one.values())), v[0])


def test_recording_a_rotating_icosphere():
    """48^3 Float32, three steps: times, every row against loads(sim) after that step, the running means against the host's
    time-weighted mean of the per-step rows, and no allocation by the library in the second and third record."""
    c = (24.37, 23.91, 24.19)
    mb = MeshBody(*MS.icosphere((0.0, 0.0, 0.0), 7.0, 2), map=B.rotation3d(c, (1.0, 2.0, 0.5), 0.15, th0=0.4))
    sim = S.Simulation((48, 48, 48), (1.0, 0.0, 0.0), 14.0, body=mb, nu=0.05, T=F32)
    sl = surface.SurfaceLoads(sim, mean=True)
    assert sl.delta == sim.eps + 1.0 and np.allclose(sl.x0, c, atol=1e-12)
    L = _lib.lib()

    def allocs():
        n, by = C.c_int64(), C.c_int64()
        assert L.wl_prof_allocs(C.byref(n), C.byref(by)) == 0
        return n.value
    rows, per_step, grew = [], [], []
    for step in range(3):
        S.sim_step(sim)
        a0 = allocs()
        surface.record(sl, sim)
        grew.append(allocs() - a0)
        one = surface.loads(sim)
        rows.append(np.array([one[k] for k in surface.columns(sl)]))
        f = surface.fields(sl)
        per_step.append(np.concatenate([f["p"][:, None], f["traction"]], 1))
    assert grew[1:] == [0, 0], grew
    t, v = surface.series(sl)
    assert np.array_equal(t, np.cumsum(np.asarray(sim.flow.dt[:-1], dtype=np.float64)))
    assert np.all(np.isfinite(v)) and np.abs(v[:, :3]).max() > 0
    for k in range(3):
        assert np.array_equal(v[k], rows[k]), k
    dt = np.diff(np.concatenate([[0.0], t]))
    want = sum(w * r for w, r in zip(dt, per_step)) / dt.sum()
    f = surface.fields(sl)
    got = np.concatenate([f["mean_p"][:, None], f["mean_traction"]], 1)
    scale = max(np.abs(r).max() for r in per_step)
    print(f"\nmean: max |device - host| = {np.abs(got - want).max():.3e}, scale {scale:.3e}")
    assert np.abs(got - want).max() <= 16 * EPS * scale           # three blends of a few operations each on values <= scale
    assert np.abs(f["body_velocity"]).max() > 0.1                  # the mesh is spinning


def test_slabs():
    """2 ranks sharing the GPU (tests/surface_worker.py): analytic fields, a mesh across the slab interface; the summed rows
    and totals equal the single-device ones within the bounds of the random-field test."""
    from test_multi_gpu import run_workers
    out = run_workers("surface_worker.py", 2, timeout=300)
    print(out)
    assert out["straddles"] and out["geom_equal"] and out["nan_equal"]
    assert out["partial_rows"] > 0                                 # some rows really are sums of two ranks' parts
    for k in ("p", "tau", "mean", "tot"):
        assert out["d_" + k] <= out["b_" + k], (k, out)
