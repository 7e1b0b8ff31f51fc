#!/usr/bin/env python3
"""Downsampled volumes and snapshots at size^3 (waterlily_amd/downsample.py, csrc/wl_downsample.h) on the developed sphere flow of
bench.py: `steps` sim_step!s, then
  1. for Float32 and Float64 and f = 2, 4, 8, the median / min / max over `reps` calls between device events of p MEAN, u CENTRE
     MEAN (three components: three launches), omega_mag MAX and lambda2 MIN made on the fly (volume()), against the same
     volumes composed from what the library had before: a torch reduction over the inside view reshaped into blocks, for the
     metrics after metric() has filled a scratch field;
  2. (Float32) the stepper's cost of one downsample.write per step (f = 4, the default attributes) and of one vtk.write per step,
     wall clock over a burst of steps as tests/test_fullsize_properties.py measures the full snapshot, and the bytes of both;
  3. the achieved bandwidth of p MEAN at f = 4 (one read of the box, one write of 1/f^3 of it).
Reported, not asserted.
usage: downsample_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--types=f32,f64] [--burst=<steps per burst, default 6>]"""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from waterlily_amd import downsample, sim as S, vtk
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps, burst = int(opt("steps", 300)), int(opt("burst", 6))
    types = [{"f32": np.float32, "f64": np.float64}[t] for t in opt("types", "f32,f64").split(",")]
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

    def blocks(a, f):
        """the inside view [n, n, n] as [n/f, f, n/f, f, n/f, f] (a view: nothing is copied)"""
        return a.unflatten(2, (-1, f)).unflatten(1, (-1, f)).unflatten(0, (-1, f))

    for T in types:
        sim = bench.sphere((size, size, size), T)
        for _ in range(nsteps):
            S.sim_step(sim, remeasure=False)
        flow = sim.flow
        scratch = S.like(flow.p)
        ins = (slice(1, -1),) * 3
        item = np.dtype(T).itemsize
        print(f"{size}^3 {np.dtype(T).name} after {nsteps} steps; u {3 * size ** 3 * item / 1e9:.2f} GB, one scalar field {size ** 3 * item / 1e9:.2f} GB")
        print(f"{'':30s}{'on the fly (volume)':40s}{'composed (torch over blocks)':40s}ratio")
        for f in (2, 4, 8):
            d = downsample.Downsampler(flow, f)
            inv = 1.0 / f ** 3

            def centre_fly():
                for c in range(3):
                    downsample.volume(d, flow.u, "centre", mode="mean", i=c)

            def centre_composed():
                out = []
                for c in range(3):
                    up = tuple(slice(2, None) if k == c else slice(1, -1) for k in range(3))
                    out.append((blocks(flow.u[ins + (c,)], f).sum(dim=(1, 3, 5), dtype=torch.float64)
                                + blocks(flow.u[up + (c,)], f).sum(dim=(1, 3, 5), dtype=torch.float64)) * (0.5 * inv))
                return out

            def metric_composed(kind, red):
                def go():
                    S.metric(scratch, kind, flow.u)
                    return red(blocks(scratch[ins], f), dim=(1, 3, 5))
                return go
            rows = [("p mean", lambda: downsample.volume(d, flow.p, "scalar", mode="mean"),
                     lambda: blocks(flow.p[ins], f).sum(dim=(1, 3, 5), dtype=torch.float64) * inv),
                    ("u centre mean x3", centre_fly, centre_composed),
                    ("omega_mag max", lambda: downsample.volume(d, flow.u, "omega_mag", mode="max"), metric_composed("omega_mag", torch.amax)),
                    ("lambda2 min", lambda: downsample.volume(d, flow.u, "lambda2", mode="min"), metric_composed("lambda2", torch.amin))]
            for name, fly, comp in rows:
                a, b = timed(fly), timed(comp)
                print(f"  f={f} {name:22s} {fmt(a):40s}{fmt(b):40s}{a[0] / b[0]:.2f}")
                if name == "p mean" and f == 4:
                    nb = size ** 3 * item + (size // f) ** 3 * item
                    print(f"      p mean f=4: {nb / 1e9:.3f} GB moved (one read of the box, one write of 1/64 of it): {nb / a[0] / 1e6:.0f} GB/s")
        if T == np.float32:
            out = tempfile.mkdtemp(prefix="wl_ds_bench_")

            def steps(n, each=None):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    S.sim_step(sim, remeasure=False)
                    if each:
                        each()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n
            try:
                base = steps(burst)
                wd = downsample.DownsampleWriter(os.path.join(out, "ds"), factor=4, dir=os.path.join(out, "DS"), T=T, ring=burst)
                downsample.write(wd, sim)                       # the first snapshot sizes the ring and the coarse buffers
                downsample.flush(wd)
                with_ds = steps(burst, lambda: downsample.write(wd, sim))
                downsample.close(wd)
                base2 = steps(burst)
                wv = vtk.vtkWriter(os.path.join(out, "full"), dir=os.path.join(out, "FULL"), ring=burst, host_buffers=1)
                vtk.write(wv, sim)
                vtk.flush(wv)
                with_full = steps(burst, lambda: vtk.write(wv, sim))
                vtk.close(wv)
                pct = lambda a, b: f"{b * 1e3:.2f} -> {a * 1e3:.2f} ms per step (+{(a / b - 1) * 100:.1f} %)"
                print(f"  a snapshot every step for {burst} steps, wall clock:")
                print(f"    downsample.write f=4 (Velocity centre mean, Pressure mean): {pct(with_ds, base)}, "
                      f"{wd.stats['bytes'] / wd.stats['snapshots'] / 1e6:.2f} MB per snapshot")
                print(f"    vtk.write (Velocity, Pressure at full resolution):          {pct(with_full, base2)}, "
                      f"{wv.stats['bytes'] / wv.stats['snapshots'] / 1e6:.2f} MB per snapshot")
            finally:
                shutil.rmtree(out, ignore_errors=True)
        del sim, flow, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
