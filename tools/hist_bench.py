#!/usr/bin/env python3
"""Histograms at size^3 (waterlily_amd/hist.py, csrc/wl_hist.h) on the developed sphere flow of bench.py: `steps` sim_step!s, then
  1. for Float32 and Float64 the median / min / max over `reps` calls between device events of hist.count for p (256 bins),
     omega_mag (256), lambda2 (256), the joint (lambda2, p) at 64 x 64, an auto-ranged p (wl_field_range + wl_histogram), a
     constant field (every cell in one bin) and a field of normal noise, against the same counts composed from what the library had before: metric() into a
     scratch field where needed, torch.histc for one axis, a fused index and torch.bincount for two, torch.aminmax for the range;
  2. the achieved bandwidth of the p case (one read of the box);
  3. (Float32) the stepper's cost of one hist.record per step (lambda2, 512 bins), wall clock over a burst of steps.
Reported, not asserted.  --label=<text> is printed with the header: the same tool run on a build with -DWL_HIST_AGG=0 (WLHIP_LIB
names the library) measures the other way of adding a wavefront's bins to LDS.
usage: hist_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--types=f32,f64] [--burst=<steps per burst, default 6>] [--label=..]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from waterlily_amd import hist, sim as S
    from waterlily_amd.hist import Axis, Histogram
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
    RP, RO, RL, RN = (-1.0, 1.0), (0.0, 1.0), (-0.1, 0.1), (-3.0, 3.0)

    for T in types:
        sim = bench.sphere((size, size, size), T)
        for _ in range(nsteps):
            S.sim_step(sim, remeasure=False)
        flow = sim.flow
        scratch, const = S.like(flow.p), S.like(flow.p, 0.375)
        ins = (slice(1, -1),) * 3
        item = np.dtype(T).itemsize
        print(f"{size}^3 {np.dtype(T).name} after {nsteps} steps; u {3 * size ** 3 * item / 1e9:.2f} GB, one scalar field {size ** 3 * item / 1e9:.2f} GB")
        print(f"{'':30s}{'wl_histogram (hist.count)':40s}{'composed (torch)':40s}ratio")
        hp, ho, hl = Histogram(flow, Axis(bins=256, range=RP)), Histogram(flow, Axis("omega_mag", bins=256, range=RO)), Histogram(flow, Axis("lambda2", bins=256, range=RL))
        hj = Histogram(flow, Axis("lambda2", bins=64, range=RL), Axis("scalar", bins=64, range=RP))
        ha = Histogram(flow, Axis(bins=256))
        noise = S.like(flow.p).normal_()                        # neighbouring cells in different bins: no runs to count once
        hn = Histogram(flow, Axis(bins=256, range=RN))

        def histc(a, r):
            return torch.histc(a[ins], bins=256, min=r[0], max=r[1])

        def metric_histc(kind, r):
            def go():
                S.metric(scratch, kind, flow.u)
                return histc(scratch, r)
            return go

        def index(a, r, n):
            return ((a[ins] - r[0]) * (n / (r[1] - r[0]))).clamp_(0, n - 1).long()

        def joint_composed():
            S.metric(scratch, "lambda2", flow.u)
            return torch.bincount((index(flow.p, RP, 64) * 64 + index(scratch, RL, 64)).reshape(-1), minlength=4096)

        def auto_composed():
            lo, hi = torch.aminmax(flow.p[ins])
            return torch.histc(flow.p[ins], bins=256, min=float(lo), max=float(hi))      # (histc takes host numbers: one read-back)

        rows = [("p 256", lambda: hist.count(hp, flow.p), lambda: histc(flow.p, RP)),
                ("omega_mag 256", lambda: hist.count(ho, flow.u), metric_histc("omega_mag", RO)),
                ("lambda2 256", lambda: hist.count(hl, flow.u), metric_histc("lambda2", RL)),
                ("lambda2 x p 64x64", lambda: hist.count(hj, flow.u, flow.p), joint_composed),
                ("p 256, auto range", lambda: hist.count(ha, flow.p), auto_composed),
                ("constant field 256", lambda: hist.count(hp, const), lambda: histc(const, RP)),
                ("noise 256", lambda: hist.count(hn, noise), lambda: histc(noise, RN))]
        for name, fly, comp in rows:
            a = timed(fly)
            try:
                b = timed(comp)
                print(f"  {name:26s} {fmt(a):40s}{fmt(b):40s}{a[0] / b[0]:.2f}")
            except RuntimeError as e:
                print(f"  {name:26s} {fmt(a):40s}composed path failed: {str(e).splitlines()[0][:60]}")
            if name == "p 256":
                nb = size ** 3 * item
                print(f"      p 256: {nb / 1e9:.3f} GB read once: {nb / a[0] / 1e9:.2f} TB/s")
        c = hist.count(hl, flow.u)
        tot = int(c.sum())
        print(f"      lambda2 256 over {RL}: {int(c[0]) / tot:.3f} of the cells under, {int(c[-1]) / tot:.3f} over, fullest bin {int(c[1:-1].max()) / tot:.3f}")
        if T == np.float32:
            def steps(n, each=None):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(n):
                    S.sim_step(sim, remeasure=False)
                    if each:
                        each()
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) / n
            base = steps(burst)
            hr = Histogram(flow, Axis("lambda2", bins=512, range=(-1, 1)))
            hs = hist.HistSeries(hr, capacity=4 * burst)
            hist.record(hs, sim, flow.u)
            with_rec = steps(burst, lambda: hist.record(hs, sim, flow.u))
            base2 = steps(burst)
            base = 0.5 * (base + base2)
            print(f"  one hist.record (lambda2, 512 bins) per step for {burst} steps, wall clock: {base * 1e3:.2f} -> {with_rec * 1e3:.2f} ms per step "
                  f"(+{(with_rec / base - 1) * 100:.1f} %)")
        del sim, flow, scratch, const, noise
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
