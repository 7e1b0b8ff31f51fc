#!/usr/bin/env python3
"""Isosurface extraction at size^3 Float32 (waterlily_amd/iso.py, csrc/wl_iso.h) on the developed sphere flow of bench.py's
kind: `steps` sim_step!s, then the lambda2 field, then three levels chosen (by quantiles of the field's negative part) to give
roughly 1e5, 1e6 and 1e7 triangles at 512^3.  For every level: the triangle count, and the median / min / max over `reps` calls,
between device events, of a pure count (count pass + scan + an emit pass that leaves every row), of an extraction without a
colour and of one coloured by omega_mag.  Beside them, in the same process: wl_metric for lambda2, one plain read of the field
(torch sum over the padded storage) with the rate it reaches, and sim_step! with and without an extraction after every step.
Reported, not asserted.
usage: iso_bench.py [size=512] [reps=25] [--steps=<n, default 300>]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from waterlily_amd import _lib, iso, sim as S
    from waterlily_amd.body import AutoBody, norm2
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    nsteps = int(next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--steps=")), 300))
    prop = torch.cuda.get_device_properties(0)
    print(f"# {' '.join(sys.argv)}   device {prop.name} ({getattr(prop, 'gcnArchName', '')}, {prop.multi_processor_count} CUs)")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    fmt = lambda t: f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    R, c = size / 8, size / 2 - 1
    sim = S.Simulation((size, size, size), (1.0, 0.0, 0.0), 2 * R, body=AutoBody(lambda x, t: norm2(x - c) - R), nu=2 * R / 3700, T=np.float32)
    for _ in range(nsteps):
        S.sim_step(sim, remeasure=False)
    flow = sim.flow
    isf = iso.Isosurface(flow, capacity=1 << 20)
    lam, om = S.like(flow.p), S.like(flow.p)
    S.metric(om, "omega_mag", flow.u)
    t_metric = timed(lambda: S.metric(lam, "lambda2", flow.u))
    nbytes = lam.untyped_storage().nbytes()
    flat = torch.as_strided(lam, (nbytes // 4 - 64,), (1,), lam.storage_offset())
    t_read = timed(lambda: flat.sum())
    print(f"{size}^3 Float32 after {nsteps} steps; field storage {nbytes / 2 ** 20:.1f} MiB")
    print(f"wl_metric lambda2            {fmt(t_metric)}")
    print(f"one plain read (torch sum)   {fmt(t_read)}   {nbytes / t_read[0] / 1e6:.0f} GB/s")
    neg = lam[1:-1, 1:-1, 1:-1]
    neg = neg[neg < 0].double()
    g = S._grid_of(lam, 3)
    L = _lib.lib()

    def raw(level, b, cap):
        _lib.check(L.wl_isosurface(_lib.WL_F32, C.byref(g), S._ptr(lam), None if b is None else S._ptr(b), level, None, None,
                                   S._ptr(isf.tri) if cap else None, S._ptr(isf.val) if (cap and b is not None) else None, cap, S._ptr(isf.cnt)))

    for q in (0.0005, 0.02, 0.3):
        level = float(torch.quantile(neg[:: max(1, len(neg) // (1 << 22))], q)) if len(neg) else -1e-3
        tri, val = iso.extract(isf, lam, level, color=om)            # grows the buffers to this surface
        nt = len(tri)
        line = f"level {level:+.4e}: {nt:9d} triangles ({nt * 72 / 2 ** 20:.1f} MiB, +{nt * 24 / 2 ** 20:.1f} MiB colour)"
        print(line)
        print(f"    count only               {fmt(timed(lambda: raw(level, None, 0)))}")
        print(f"    extract                  {fmt(timed(lambda: raw(level, None, isf.capacity)))}")
        print(f"    extract + colour         {fmt(timed(lambda: raw(level, om, isf.capacity)))}")
    level = float(torch.quantile(neg[:: max(1, len(neg) // (1 << 22))], 0.02)) if len(neg) else -1e-3

    def steps(extract):
        def one():
            S.sim_step(sim, remeasure=False)
            if extract:
                S.metric(lam, "lambda2", flow.u)
                raw(level, None, isf.capacity)
        return one
    a, b = timed(steps(False)), timed(steps(True))
    print(f"sim_step!                    {fmt(a)}")
    print(f"sim_step! + lambda2 + extract{fmt(b)}   (+{b[0] - a[0]:.3f} ms per step)")


if __name__ == "__main__":
    main()
