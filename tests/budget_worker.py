"""Worker for tests/test_budget_gpu.py::test_slabs_match_undecomposed: launched with torch.distributed.run, 2 ranks sharing ONE
GPU, gloo host-callback transport (as tests/meanflow_worker.py).  Every rank steps the undecomposed 32^3 sphere and its z-slab of
the decomposed one, each with a Budget, and compares the gathered owned planes of the moments, of the means and of the terms
(whose planes next to the rank boundary read the exchanged halo plane of the moments)."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waterlily_amd import budget as B  # noqa: E402
from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402


def rel(a, b, scale):
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))) / max(1e-30, scale))


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    m = 32
    R, c = m / 8, m / 2 - 1
    dims = (m, m, m)
    kw = dict(nu=2 * R / 3700, body=AutoBody(lambda x, t: norm2(x - c) - R), T=np.float32)
    ref = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * R, slab=None, **kw)
    sim = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * R, slab=wd.Slab(rank, size, dims[2]), **kw)
    br, bs = B.Budget(ref.flow), B.Budget(sim.flow)
    for _ in range(5):
        S.sim_step(ref, remeasure=False)
        S.sim_step(sim, remeasure=False)
        B.update(br, ref.flow)
        B.update(bs, sim.flow)
    out = {"n_ref": list(ref.pois.n), "n_slab": list(sim.pois.n), "t_ref": br.t, "t_slab": bs.t}
    # every difference is scaled by the units of its field: powers of max|U| and max|P| of the undecomposed run, and for the
    # terms (all of the units u^3 / L, L = one cell) u^3 -- except k (u^2) and the pressure transport (p u)
    su, sp = float(np.max(np.abs(S.to_host(br.mean.U)))), float(np.max(np.abs(S.to_host(br.mean.P))))
    fields = {"U": (bs.mean.U, br.mean.U, su), "P": (bs.mean.P, br.mean.P, sp), "R": (bs.R, br.R, su ** 2),
              "PU": (bs.PU, br.PU, sp * su), "GG": (bs.GG, br.GG, su ** 2), "T3": (bs.T3, br.T3, su ** 3)}
    for k, (a, b, scale) in fields.items():
        out["d_" + k] = rel(S.gather(a), S.to_host(b), scale)
    nu = ref.flow.nu
    Ts, Tr = S.gather(B.terms(bs, nu)), S.to_host(B.terms(br, nu))
    pressure = {"P", "PU", "pressure_transport", "residual"}
    for q, name in enumerate(B.columns()):
        scale = su ** 2 if name == "k" else (sp * su if name in pressure else su ** 3)
        out["d_" + name] = rel(Ts[..., q], Tr[..., q], scale)
    out["pressure_derived"] = sorted(pressure)
    out["velocity_derived"] = sorted((set(fields) | set(B.columns())) - pressure)
    out["k_max"] = float(Tr[..., 0].max())
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
