"""Worker for tests/test_probes_gpu.py::test_slabs: launched with torch.distributed.run, 2 ranks sharing ONE GPU, gloo
host-callback transport (as tests/meanflow_worker.py).

1. Every rank steps the undecomposed 32^3 sphere and its z-slab of the decomposed one, each with Probes at points whose
   floor planes are rank 0's top owned plane, rank 1's bottom one, the plane the ranks share, and the z ghost planes; after
   every step the slab run's record is compared with the restatement (tests/probes_ref.py) on its own gathered u and p
   (series() sums the ranks' buffers), and at the end its series with the undecomposed run's.
2. A z-periodic ring of slabs (nobody owns the z ghost planes): random u and p on the owned planes, halo exchange, then
   interp() of the slab fields against the restatement on the gathered ones.
3. Tracers refuse a slab flow."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probes_ref as R  # noqa: E402

from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import probes as P  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402


def diff(a, b, scale):
    """max |a - b| / scale over entries where both are finite; inf where only one of them is NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return float("inf")
    k = ~np.isnan(a)
    return float(np.max(np.abs(a[k] - b[k]), initial=0.0) / max(1e-30, scale))


def points(m, rng):
    zs = [1.0, 1.25, 1.75, 2.0, 2.5, 17.0, 17.25, 17.5, 17.75, 18.0, 18.25, 18.5, 18.75, 19.0, 33.5, 33.75, 34.0, 34.25, 0.75]
    X = [[rng.uniform(2, m), rng.uniform(2, m), z] for z in zs]
    X += [[m / 2 + 1.5, m / 2 + 0.5, 17.5], [m / 2 + 4.0, m / 2, 18.0]]          # beside the sphere, across the shared plane
    return np.array(X)


def record_row(u, p, X):
    return np.concatenate([R.interp_many(X, u, True), R.interp_many(X, p, False)[:, None]], axis=1)


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    m = 32
    Rr, c = m / 8, m / 2 - 1
    dims = (m, m, m)
    kw = dict(nu=2 * Rr / 3700, body=AutoBody(lambda x, t: norm2(x - c) - Rr), T=np.float32)
    ref = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * Rr, slab=None, **kw)
    sim = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * Rr, slab=wd.Slab(rank, size, dims[2]), **kw)
    X = points(m, np.random.default_rng(11))
    pr, ps = P.Probes(ref.flow, X, capacity=2), P.Probes(sim.flow, X, capacity=2)
    out = {"own": [sim.flow.layout.slab.kz0 + sim.flow.layout.slab.own_lo, sim.flow.layout.slab.kz0 + sim.flow.layout.slab.own_hi]}
    want = []
    for _ in range(4):
        S.sim_step(ref, remeasure=False)
        S.sim_step(sim, remeasure=False)
        P.record(pr, ref.flow)
        P.record(ps, sim.flow)
        want.append(record_row(S.gather(sim.flow.u), S.gather(sim.flow.p), X))
    t_ref, v_ref = P.series(pr)
    t_s, v_s = P.series(ps)
    want = np.array(want)
    scale = float(np.nanmax(np.abs(want)))
    out["t_equal"] = bool(np.array_equal(t_ref, t_s))
    out["d_own"] = diff(v_s, want, scale)                    # against its own gathered fields
    out["bitwise_own"] = bool(np.array_equal(v_s, want, equal_nan=True))
    su = float(np.nanmax(np.abs(v_ref[..., :3])))
    sp = float(np.nanmax(np.abs(v_ref[..., 3])))
    out["d_u_ref"] = diff(v_s[..., :3], v_ref[..., :3], su)
    out["d_p_ref"] = diff(v_s[..., 3], v_ref[..., 3], sp)
    out["nan_rows"] = int(np.isnan(v_s[0]).any(axis=1).sum())
    # 2. a ring of slabs: the z ghost planes are halo copies on the edge ranks
    ring = S.Flow(dims, (1.0, 0.0, 0.0), T=np.float32, perdir=(2,), slab=wd.Slab(rank, size, dims[2], ring=True))
    sl = ring.layout.slab
    rng = np.random.default_rng(3)
    Ng = tuple(n + 2 for n in dims)
    gu = rng.standard_normal(Ng + (3,)).astype(np.float32) + 0.5
    gp = rng.standard_normal(Ng).astype(np.float32)
    for a, g in ((ring.u, gu), (ring.p, gp)):
        h = np.zeros(tuple(a.shape), dtype=np.float32)
        for l in range(h.shape[2]):
            k = sl.kz0 + l
            if sl.own_lo <= l <= sl.own_hi:
                h[:, :, l] = g[:, :, k]
        S.upload(a, h)
        S.halo_exchange(a, 2)
    Gu, Gp = S.gather(ring.u), S.gather(ring.p)
    Xr = np.array([[rng.uniform(1.5, m + 1), rng.uniform(1.5, m + 1), z] for z in
                   (1.0, 1.25, 1.5, 1.75, 2.0, 2.5, 17.5, 18.0, 33.0, 33.5, 33.75, 34.0, 34.5, 0.5)])
    got_u, got_p = P.interp(Xr, ring.u), P.interp(Xr, ring.p)
    ru, rp = R.interp_many(Xr, Gu, True), R.interp_many(Xr, Gp, False)
    out["ring_bitwise"] = bool(np.array_equal(got_u, ru, equal_nan=True) and np.array_equal(got_p, rp, equal_nan=True))
    out["ring_d"] = max(diff(got_u, ru, 3.0), diff(got_p, rp, 3.0))
    out["ring_ghost_values"] = int(np.isfinite(ru[:4]).all(axis=1).sum())
    # 3. tracers refuse slabs
    try:
        P.Tracers(sim.flow, X[:2])
        out["tracers_refused"] = False
    except ValueError:
        out["tracers_refused"] = True
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
