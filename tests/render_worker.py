"""Worker for tests/test_render_gpu.py::test_slabs: launched with torch.distributed.run, 2 ranks sharing ONE GPU, gloo
host-callback transport (as tests/iso_worker.py).

Every rank projects the same seeded random fields (33, 12, 12) on an undecomposed flow and on its z-slab of the decomposed one
(each rank uploads the planes it owns; u is then exchanged to depth 2, as mom_step! leaves it).  render.gather() combines the
parts on rank 0, which compares them with the undecomposed images: by bits where the contract says so, and for the axis-2 sum
against the bound of a reordered sum of nz doubles, nz 2^-53 sum|x| per pixel, computed from the data."""
import json
import os
import sys

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import render, sim as S  # noqa: E402

SHAPE = (33, 12, 12)
# (key, field, kind, mode, axis, index)
VIEWS = [("axis1_max", "p", "scalar", "max", 1, None), ("axis1_sum", "p", "scalar", "sum", 1, None),
         ("axis2_max", "p", "scalar", "max", 2, None), ("axis2_sum", "p", "scalar", "sum", 2, None),
         ("axis0_absmax", "u", "centre", "absmax", 0, None), ("axis1_max_lambda2", "u", "lambda2", "max", 1, None),
         ("axis2_min_slice", "u", "ucomp", "slice", 2, 9)]


def host_fields(T):
    Ng = tuple(n + 2 for n in SHAPE)
    rng = np.random.default_rng(13)
    return (np.asfortranarray(rng.standard_normal(Ng).astype(T)), np.asfortranarray(rng.standard_normal(Ng + (3,)).astype(T)))


def upload_owned(a, host):
    """the planes of the undecomposed host array this rank owns; every other local plane holds NaN until the exchange"""
    sl = a._wl_slab
    h = np.full(tuple(a.shape), np.nan, dtype=host.dtype)
    for l in range(sl.own_lo, sl.own_hi + 1):
        h[:, :, l] = host[:, :, sl.kz0 + l]
    S.upload(a, h)


def run(T, slab):
    flow = S.Flow(SHAPE, (0.0, 0.0, 0.0), T=T, slab=slab)
    r = render.Renderer(flow)
    hp, hu = host_fields(T)
    if slab is None:
        S.upload(flow.p, hp)
        S.upload(flow.u, hu)
    else:
        upload_owned(flow.p, hp)
        upload_owned(flow.u, hu)
        S.halo_exchange(flow.u, 2)
    out = {}
    for key, fld, kind, mode, axis, index in VIEWS:
        img = render.project(r, getattr(flow, fld), kind, mode=mode, axis=axis, index=index, i=1)
        out[key] = (img.cpu().numpy().copy(), axis, mode)
    return out, hp


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    res = {}
    for T in (np.float32, np.float64):
        one, hp = run(T, None)
        slab = wd.Slab(rank, size, SHAPE[2])
        parts, _ = run(T, slab)
        rows = [None] * size
        dist.all_gather_object(rows, int(parts["axis1_max"][0].shape[0]))
        o = {"rows": rows}
        for key, (img, axis, mode) in parts.items():
            g = render.gather(img, axis, mode, slab)
            if rank != 0:
                assert g is None
                continue
            want = one[key][0]
            if key == "axis2_sum":
                x = hp[1:-1, 1:-1, 1:-1].astype(np.float64)
                bound = SHAPE[2] * 2.0 ** -53 * np.abs(x).sum(axis=2).T
                err = np.abs(g - want)
                o["axis2_sum_err"] = float(err.max())
                o["axis2_sum_bound"] = float(bound.min())
                o["axis2_sum_ok"] = bool(g.shape == want.shape and np.all(err <= bound))
            else:
                o[key] = bool(g.shape == want.shape and np.array_equal(g.view(np.uint64), want.view(np.uint64)))
        if rank == 0:
            res[np.dtype(T).name] = o
    if rank == 0:
        print("RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
