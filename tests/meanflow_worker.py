"""Worker for tests/test_meanflow_gpu.py::test_slabs_match_undecomposed: launched with torch.distributed.run, 2 ranks sharing
ONE GPU, gloo host-callback transport (as tests/mg_worker.py).  Every rank steps the undecomposed 32^3 sphere and its z-slab of
the decomposed one, each with a MeanFlow (all statistics), and compares the gathered owned planes of the averages; then both
runs write mean_attrib to VTK (the slab run as one piece per rank + .pvti, the undecomposed one on rank 0) and rank 0 compares
every piece, the plane the two pieces share included, with the one-device file."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import sim as S  # noqa: E402
from waterlily_amd import stats as M  # noqa: E402
from waterlily_amd import vtk  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402


def rel(a, b, scale):
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64))) / max(1e-30, scale))


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    tmp = os.environ["WL_TMP"]
    m = 32
    R, c = m / 8, m / 2 - 1
    dims = (m, m, m)
    kw = dict(nu=2 * R / 3700, body=AutoBody(lambda x, t: norm2(x - c) - R), T=np.float32)
    ref = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * R, slab=None, **kw)
    sim = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * R, slab=wd.Slab(rank, size, dims[2]), **kw)
    mr = M.MeanFlow(ref.flow, uu_stats=True, pp_stats=True)
    ms = M.MeanFlow(sim.flow, uu_stats=True, pp_stats=True)
    for _ in range(4):
        S.sim_step(ref, remeasure=False)
        S.sim_step(sim, remeasure=False)
        M.update(mr, ref.flow)
        M.update(ms, sim.flow)
    out = {"n_ref": list(ref.pois.n), "n_slab": list(sim.pois.n), "t_ref": mr.t, "t_slab": ms.t}
    # the covariances carry the units of u^2 (p^2): their differences are scaled by max|U|^2 (max|P|^2), the means' by max|U|
    uref, pref = S.to_host(mr.U), S.to_host(mr.P)
    su, sp = float(np.max(np.abs(uref))), float(np.max(np.abs(pref)))
    scale = {"U": su, "UU": su * su, "P": sp, "pp": sp * sp}
    for k in ("U", "P", "UU", "pp"):
        out["d_" + k] = rel(S.gather(getattr(ms, k)), S.to_host(getattr(mr, k)), scale[k])
    # VTK: two pieces of the slab run against the one-device file
    ws = vtk.vtkWriter(os.path.join(tmp, "slab"), attrib=M.mean_attrib(ms), dir=os.path.join(tmp, "SLAB"))
    vtk.write(ws, sim)
    vtk.close(ws)
    if rank == 0:
        w1 = vtk.vtkWriter(os.path.join(tmp, "one"), attrib=M.mean_attrib(mr), dir=os.path.join(tmp, "ONE"))
        vtk.write(w1, ref)
        vtk.close(w1)
    dist.barrier()
    if rank == 0:
        one = vtk.read_vti(vtk.read_pvd(os.path.join(tmp, "one.pvd"))[-1][1])
        _, pieces = vtk.read_pieces(vtk.read_pvd(os.path.join(tmp, "slab.pvd"))[-1][1])
        out["pieces"] = len(pieces)
        seen = np.zeros(dims[2] + 2, dtype=int)
        names = {"MeanVelocity": "U", "ReynoldsStress": "UU", "MeanPressure": "P", "PressureVariance": "pp"}
        for name, k in names.items():
            d = 0.0
            for ext, path in pieces:
                lo, hi = ext[2][0] - 1, ext[2][1] - 1
                a = vtk.read_vti(path)[name]
                d = max(d, rel(np.asarray(a), np.asarray(one[name][..., lo:hi + 1]), scale[k]))
                if name == "MeanPressure":
                    seen[lo:hi + 1] += 1
            out["d_vtk_" + name] = d
        out["shared_plane_checked"] = bool(seen.min() >= 1 and seen.max() == 2)
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
