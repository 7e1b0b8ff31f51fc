"""Worker for tests/test_iso_gpu.py::test_slabs: launched with torch.distributed.run, 2 ranks sharing ONE GPU, gloo
host-callback transport (as tests/surface_worker.py).

Every rank extracts the surface of the same seeded random field (33, 12, 10), coloured by a second one, on an undecomposed flow
and on its z-slab of the decomposed one (each rank uploads the planes it owns, then the fields are exchanged to depth 1, as
wl_isosurface asks).  iso.gather() concatenates the parts in rank order; rank 0 compares them with the undecomposed surface by
bits, for Float32 and Float64."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_iso_cpu import LEVEL, random_field  # noqa: E402

from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import iso, sim as S  # noqa: E402

SHAPE = (33, 12, 10)


def upload_owned(a, host):
    """the planes of the undecomposed host array this rank owns; every other local plane holds a value no surface survives"""
    sl = a._wl_slab
    h = np.full(tuple(a.shape), np.nan, dtype=host.dtype)
    for l in range(sl.own_lo, sl.own_hi + 1):
        h[:, :, l] = host[:, :, sl.kz0 + l]
    S.upload(a, h)


def run(T, slab):
    flow = S.Flow(SHAPE, (0.0, 0.0, 0.0), T=T, slab=slab)
    isf = iso.Isosurface(flow, capacity=1 << 16)
    a, b = S.like(flow.p), S.like(flow.p)
    ha, hb = random_field(SHAPE, T), random_field(SHAPE, T, seed=11)
    if slab is None:
        S.upload(a, ha)
        S.upload(b, hb)
    else:
        upload_owned(a, ha)
        upload_owned(b, hb)
        S.halo_exchange(a, 1)
        S.halo_exchange(b, 1)
    tri, val = iso.extract(isf, a, LEVEL, color=b)
    n = iso.count(isf, a, LEVEL)
    return tri.cpu().numpy().copy(), val.cpu().numpy().copy(), n


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    out = {}
    for T in (np.float32, np.float64):
        t1, v1, _ = run(T, None)
        slab = wd.Slab(rank, size, SHAPE[2])
        t2, v2, n2 = run(T, slab)
        parts = [None] * size
        dist.all_gather_object(parts, len(t2))
        counts = [None] * size
        dist.all_gather_object(counts, n2)
        gt, gv = iso.gather(t2, v2, slab)
        if rank == 0:
            out[np.dtype(T).name] = {
                "total": len(t1), "parts": parts, "counts": counts,
                "tri_equal": bool(gt.shape == t1.shape and np.array_equal(gt.view(np.uint64), t1.view(np.uint64))),
                "val_equal": bool(gv.shape == v1.shape and np.array_equal(gv.view(np.uint64), v1.view(np.uint64))),
            }
        else:
            assert gt is None and gv is None
    if rank == 0:
        print("RESULT " + json.dumps(out), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
