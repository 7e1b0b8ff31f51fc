"""Worker for tests/test_mesh_gpu.py::test_slabs_match_undecomposed: launched with torch.distributed.run, 2 ranks sharing ONE
GPU, gloo host-callback transport (as tests/meanflow_worker.py).  Every rank measures and steps the undecomposed 32^3 case and
its z-slab of the decomposed one with the same spinning torus MeshBody; the gathered owned planes of mu0, mu1, V must equal the
undecomposed run's bit for bit (a cell's value depends on its global position only), total_force after 3 steps is compared by
the caller."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_shapes as MS  # noqa: E402

from waterlily_amd import body as B  # noqa: E402
from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd.mesh import MeshBody  # noqa: E402


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    dims = (32, 32, 32)
    v, t = MS.torus((0.0, 0.0, 0.0), 7.0, 2.4, 24, 12)
    body = lambda: MeshBody(v, t, map=B.rotation3d((15.37, 15.91, 15.13), (1.0, 2.0, 0.5), 0.15, th0=0.4))
    kw = dict(nu=0.05, T=np.float32)
    ref = S.Simulation(dims, (1.0, 0.0, 0.0), 8.0, slab=None, body=body(), **kw)
    sim = S.Simulation(dims, (1.0, 0.0, 0.0), 8.0, slab=wd.Slab(rank, size, dims[2]), body=body(), **kw)
    for _ in range(3):
        S.sim_step(ref)
        S.sim_step(sim)
    out = {"n_ref": list(ref.pois.n), "n_slab": list(sim.pois.n), "dt_ref": list(ref.flow.dt), "dt_slab": list(sim.flow.dt)}
    for k in ("mu0", "mu1", "V"):
        out["equal_" + k] = bool(np.array_equal(S.gather(getattr(sim.flow, k)), S.to_host(getattr(ref.flow, k))))
    out["force_ref"] = [float(x) for x in S.total_force(ref)]
    out["force_slab"] = [float(x) for x in S.total_force(sim)]
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
