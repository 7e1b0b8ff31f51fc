"""Worker for tests/test_surface_gpu.py::test_slabs: launched with torch.distributed.run, 2 ranks sharing ONE GPU, gloo
host-callback transport (as tests/probes_worker.py).

Every rank samples the same moving icosphere, whose samples lie on both sides of the slab interface, on an undecomposed
40x32x24 Float32 flow and on its z-slab of the decomposed one.  Nothing is stepped: two sets of analytic fields are uploaded
(each rank the planes it holds, halo planes included) and recorded at two times, so that the running mean blends twice.  The
slab run's rows, means and totals (fields() and series() sum the ranks' partial rows) are compared with the undecomposed
run's; the bounds are test_surface_cpu.tol_sampled's."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import probes_ref as R  # noqa: E402
import surface_ref as SR  # noqa: E402
from test_surface_cpu import DIMS, EPS, NU, body_of, make_sim, tol_sampled, upload_global  # noqa: E402

from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import surface  # noqa: E402

X0 = (17.5, 20.25, 9.0)
TIMES = (0.8, 1.2)


def analytic(k):
    Ng = tuple(n + 2 for n in DIMS)
    a, b = 0.31 + 0.07 * k, 0.23 - 0.05 * k
    p = R.fill_centres(Ng, lambda x: np.sin(a * x[0]) * np.cos(b * x[1]) + 0.1 * x[2] * np.cos(a * x[2]), np.float32)
    u = R.fill_faces(Ng, lambda i, x: np.cos(b * x[(i + 1) % 3] + 0.3 * i) * np.sin(a * x[(i + 2) % 3]) + 0.05 * (i + 1) * x[i], np.float32)
    return p, u


def run(mb, slab, fields):
    sim = make_sim(mb, np.float32, True, slab=slab)
    sl = surface.SurfaceLoads(sim, delta=1.5, x0=X0, mean=True)
    for t, (p, u) in zip(TIMES, fields):
        sim.flow.dt = [t, 0.25]
        upload_global(sim.flow.p, p)
        upload_global(sim.flow.u, u)
        surface.record(sl, sim)
    return sl, surface.fields(sl), surface.series(sl)[1]


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    mb = body_of("icosphere", True, "mid")
    fields = [analytic(0), analytic(1)]
    _, f1, v1 = run(mb, None, fields)
    sl, f2, v2 = run(mb, wd.Slab(rank, size, DIMS[2]), fields)
    geo = SR.geometry(mb.vertices, mb.triangles, mb.coeffs(TIMES[-1]))
    tp, ttau, _, _, _ = tol_sampled(mb, geo, 1.5, *fields[-1])
    tp0, ttau0, _, _, _ = tol_sampled(mb, geo, 1.5, *fields[0])
    plane = np.floor(geo["centroid"][:, 2] + 1.5 * geo["n"][:, 2] + 1.5) - 1          # floor plane of the pressure sample, global
    top = sl.slab.kz0 + sl.slab.own_hi if rank == 0 else None
    local = sl.rows.cpu().numpy()
    total = np.concatenate([f2["p"][:, None], f2["traction"]], 1)
    dmax = lambda a, b: float(np.abs(np.asarray(a) - np.asarray(b)).max())
    nt, sa = len(plane), float(geo["area"].sum())
    Fp, Fu = max(float(np.abs(p).max()) for p, _ in fields), max(float(np.abs(u).max()) for _, u in fields)
    arm = float(np.abs(geo["centroid"] - np.array(X0)).max())
    out = {
        "straddles": bool(rank != 0 or (np.any(plane <= top) and np.any(plane > top))),
        "geom_equal": all(np.array_equal(f1[k], f2[k]) for k in ("centroid", "area_vector", "body_velocity")),
        "nan_equal": all(np.array_equal(np.isnan(f1[k]), np.isnan(f2[k])) for k in ("p", "traction", "mean_p", "mean_traction"))
        and not np.isnan(f1["p"]).any() and not np.isnan(f1["traction"]).any(),
        "partial_rows": int(np.any((local != 0) & (local != total), axis=1).sum()),
        "d_p": dmax(f1["p"], f2["p"]), "b_p": tp,
        "d_tau": dmax(f1["traction"], f2["traction"]), "b_tau": ttau,
        "d_mean": max(dmax(f1["mean_p"], f2["mean_p"]), dmax(f1["mean_traction"], f2["mean_traction"])),
        "b_mean": max(tp, ttau, tp0, ttau0),
        # totals of partial rows, summed: every row within (tp, ttau), weighted by |S| and the lever arm, plus the rounding of
        # two reductions of nt terms no larger than the entries' own sums of absolute values (p <= Fp, tau <= 12 nu Fu)
        "d_tot": dmax(v1, v2),
        "b_tot": 2 * max(1.0, arm) * sa * (max(tp, ttau, tp0, ttau0) + 2 * nt * EPS * max(Fp, 12 * NU * Fu)),
    }
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
