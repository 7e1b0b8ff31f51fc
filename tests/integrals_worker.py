"""Worker for tests/test_integrals_gpu.py::test_slabs: launched with torch.distributed.run, 2 ranks sharing ONE GPU, gloo
host-callback transport (as tests/probes_worker.py).

1. Every rank steps its z-slab of the 32^3 sphere with an Integrals recorder (capacity 2: the buffer grows) and, after every
   step, gathers u; series() (which combines the ranks' buffers at the host) is compared with the restatement
   (tests/integrals_ref.py) on the gathered fields, within the derived bound with n the global cell count.
2. A z-periodic ring of slabs (the z ghost planes are halo copies): random u on the owned planes, halo exchange, then the
   one-off integrals() against the restatement on the gathered field."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import integrals_ref as R  # noqa: E402

from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import integrals as I  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402


def ratio(got, u, U):
    """largest |got - ref| / tolerance over the columns (umax: 0 when exact, inf otherwise)"""
    row, bound, n = R.integrals(u, U)
    tol = R.tolerance(bound, n)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - row).astype(np.float64)
    w = 0.0
    for q in range(len(tol)):
        w = max(w, (0.0 if err[q] == 0 else float("inf")) if tol[q] == 0 else err[q] / tol[q])
    return float(w)


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    m = 32
    Rr, c = m / 8, m / 2 - 1
    dims = (m, m, m)
    U = (1.0, 0.0, 0.0)
    sim = S.Simulation(dims, U, 2 * Rr, slab=wd.Slab(rank, size, dims[2]), nu=2 * Rr / 3700,
                       body=AutoBody(lambda x, t: norm2(x - c) - Rr), T=np.float32)
    ig = I.Integrals(sim.flow, U=U, capacity=2)
    fields, times = [], []
    for _ in range(4):
        S.sim_step(sim, remeasure=False)
        I.record(ig, sim.flow)
        times.append(S.time(sim.flow))
        fields.append(S.gather(sim.flow.u))
    local = ig.buf[:4].cpu().numpy()
    t, v = I.series(ig)
    out = {"t_equal": t.tolist() == times, "rows": int(v.shape[0])}
    worst = max(ratio(v[k], fields[k], U) for k in range(4))
    out["worst"] = worst
    out["within_bound"] = bool(worst <= 1.0)
    out["local_rows_differ"] = bool(np.all(local[:, 0] < v[:, 0]))            # a rank holds its own share, not the total
    one = I.integrals(sim.flow, U=U)
    out["one_off_equal"] = bool(np.array_equal(np.array(list(one.values())), v[-1]))
    # 2. a ring of slabs
    ring = S.Flow(dims, (1.0, 0.0, 0.0), T=np.float64, perdir=(2,), slab=wd.Slab(rank, size, dims[2], ring=True))
    sl = ring.layout.slab
    rng = np.random.default_rng(3)
    Ng = tuple(n + 2 for n in dims)
    gu = rng.standard_normal(Ng + (3,)) + 0.5
    h = np.zeros(tuple(ring.u.shape))
    for l in range(h.shape[2]):
        if sl.own_lo <= l <= sl.own_hi:
            h[:, :, l] = gu[:, :, sl.kz0 + l]
    S.upload(ring.u, h)
    S.halo_exchange(ring.u, 2)
    Gu = S.gather(ring.u)
    got = np.array(list(I.integrals(ring).values()))
    out["ring_worst"] = ratio(got, Gu, None)
    out["ring_within_bound"] = bool(out["ring_worst"] <= 1.0)
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
