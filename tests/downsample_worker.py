"""Worker for tests/test_downsample_gpu.py::test_slabs: launched with torch.distributed.run, 2 ranks sharing ONE GPU, gloo
host-callback transport (as tests/render_worker.py).

Every rank downsamples the same seeded random fields (32, 12, 16) at f = 2 and 4 on an undecomposed flow and on its z-slab of the
decomposed one (each rank uploads the planes it owns; u is then exchanged to depth 2, as mom_step! leaves it).
downsample.gather() concatenates the parts on rank 0, which compares them with the undecomposed volumes by bits: no block
straddles two ranks, so nothing is reordered.  The decomposed writer is held to the same volumes: rank 0's one file, read back."""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from waterlily_amd import dist as wd  # noqa: E402
from waterlily_amd import downsample, sim as S  # noqa: E402

SHAPE = (32, 12, 16)
# (key, field, kind, mode, component)
VIEWS = [("p_mean", "p", "scalar", "mean", 0), ("u_face", "u", "face", "mean", 2), ("lambda2_min", "u", "lambda2", "min", 0)]


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


def run(T, slab, f, tmp):
    flow = S.Flow(SHAPE, (0.0, 0.0, 0.0), T=T, slab=slab)
    hp, hu = host_fields(T)
    if slab is None:
        S.upload(flow.p, hp)
        S.upload(flow.u, hu)
    else:
        upload_owned(flow.p, hp)
        upload_owned(flow.u, hu)
        S.halo_exchange(flow.u, 2)
    d = downsample.Downsampler(flow, f)
    out = {key: downsample.volume(d, getattr(flow, fld), kind, mode=mode, i=c).cpu().numpy().copy() for key, fld, kind, mode, c in VIEWS}
    out["velocity"] = downsample.velocity(d, flow.u).cpu().numpy().copy()
    if slab is not None:                                       # the decomposed writer: one file from rank 0
        sim = types.SimpleNamespace(flow=flow, slab=slab, U=1.0, L=1.0)
        w = downsample.DownsampleWriter(os.path.join(tmp, f"s{f}_{np.dtype(T).name}"), factor=f, dir=os.path.join(tmp, "vtk"), T=T,
                                        attrib={"P": (lambda s: s.flow.p, "scalar", "mean"), "U": (lambda s: s.flow.u, "face", "mean")})
        downsample.write(w, sim)
        downsample.close(w)
        out["file"] = w.entries[0][1]
    return out, d


def same(a, b):
    v = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v)))


def main():
    dist.init_process_group("gloo")
    wd.init_host()
    rank, size = dist.get_rank(), dist.get_world_size()
    tmp = [tempfile.mkdtemp(prefix="wl_ds_") if rank == 0 else None]
    dist.broadcast_object_list(tmp, 0)
    res = {}
    for T in (np.float32, np.float64):
        o = {}
        for f in (2, 4):
            one, _ = run(T, None, f, tmp[0])
            slab = wd.Slab(rank, size, SHAPE[2])
            parts, d = run(T, slab, f, tmp[0])
            planes = [None] * size
            dist.all_gather_object(planes, int(d.nc[2]))
            r = {"planes": planes}
            for key in [v[0] for v in VIEWS] + ["velocity"]:
                g = downsample.gather(parts[key], slab)
                if rank != 0:
                    assert g is None
                    continue
                r[key] = same(g, one[key])
            dist.barrier()
            if rank == 0:
                arrays, origin, spacing = downsample.read(parts["file"])
                ok = same(np.asarray(arrays["P"]), one["p_mean"]) and origin == tuple(1 + 1 + (f - 1) / 2 for _ in range(3))
                ok = ok and spacing == (float(f),) * 3 and same(np.asarray(arrays["U"][2]), one["u_face"])
                r["file"] = bool(ok)
                o[str(f)] = r
        if rank == 0:
            res[np.dtype(T).name] = o
    if rank == 0:
        shutil.rmtree(tmp[0], ignore_errors=True)
        print("RESULT " + json.dumps(res), flush=True)
    dist.barrier()
    wd.finalize()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
