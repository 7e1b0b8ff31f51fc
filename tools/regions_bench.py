#!/usr/bin/env python3
"""Connected regions at size^3 (waterlily_amd/regions.py, csrc/wl_regions.h) on the developed sphere flow of bench.py: `steps`
sim_step!s, then
  1. for Float32 and Float64 the median / min / max over `reps` calls between device events of regions.label (capacity 4096,
     no read-back) for p BELOW its 5 % quantile, omega_mag ABOVE its 95 %, lambda2 BELOW its 5 % (the levels from hist.quantile)
     and an all-IN field (p BELOW +inf: one region, every table atomic on one row), with R and the share of IN cells;
  2. the same four cases on a box of `small`^3 cells behind the sphere, where the fixed number of launches may dominate;
  3. against the only path there was before: the value into a scratch field (metric), to_host, and the breadth-first fill of
     tests/regions_ref.py -- plain Python, so it is timed ONCE and on a box of `ref`^3 cells behind the sphere, with the device's
     time for the same box beside it;
  4. (Float32) the stepper's cost of one regions.record per step (lambda2, the 8 largest regions), wall clock over a burst.
Reported, not asserted.
usage: regions_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--types=f32,f64] [--small=64] [--ref=128] [--burst=6]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import bench
    import regions_ref as RR
    from waterlily_amd import hist, regions, sim as S
    from waterlily_amd.hist import Axis, Histogram
    from waterlily_amd.regions import Regions, Value
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps, burst, small, nref = int(opt("steps", 300)), int(opt("burst", 6)), int(opt("small", 64)), int(opt("ref", 128))
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

    def behind(n):
        """a box of n^3 cells (at most inside()) that starts at the sphere's centre plane and reaches into the wake"""
        n = min(n, size)
        x0 = max(1, min(size // 2, size + 1 - n))
        y0 = max(1, size // 2 - n // 2)
        return (x0, y0, y0), (x0 + n, y0 + n, y0 + n)

    for T in types:
        sim = bench.sphere((size, size, size), T)
        for _ in range(nsteps):
            S.sim_step(sim, remeasure=False)
        flow = sim.flow
        item = np.dtype(T).itemsize
        print(f"{size}^3 {np.dtype(T).name} after {nsteps} steps; u {3 * size ** 3 * item / 1e9:.2f} GB, the label volume {size ** 3 * 4 / 1e9:.2f} GB")
        level = {}
        for kind, rng, q in (("scalar", None, 0.05), ("omega_mag", None, 0.95), ("lambda2", None, 0.05)):
            h = Histogram(flow, Axis(kind, bins=4096))
            f = flow.p if kind == "scalar" else flow.u
            level[kind] = float(hist.quantile(hist.count(h, f), hist.edges(h), q))
            del h
        cases = [("p below q05", "scalar", dict(below=level["scalar"])), ("omega_mag above q95", "omega_mag", dict(above=level["omega_mag"])),
                 ("lambda2 below q05", "lambda2", dict(below=level["lambda2"])), ("all IN (p below inf)", "scalar", dict(below=float("inf")))]
        for title, box in [(f"inside(), {size}^3", None)] + ([(f"a box of {min(small, size)}^3", behind(small))] if small > 0 else []):
            print(f"  {title}")
            for name, kind, kw in cases:
                rg = Regions(flow, Value(kind), box=box, **kw)
                f = flow.p if kind == "scalar" else flow.u
                t = timed(lambda: regions.label(rg, f))
                res = regions.label(rg, f)
                print(f"    {name:24s} {fmt(t)}   level {list(kw.values())[0]:+.4e}  R {int(res.count):8d}  IN {int(res.cells) / int(res.visited):.4f}")
                del rg, res
        box = behind(max(nref, 1))
        if nref > 0 and T is types[0]:
            print(f"  the path before (metric -> scratch, to_host, breadth-first fill in Python), once, on a box of {min(nref, size)}^3 against regions.table on it")
        scratch = S.like(flow.p)
        for name, kind, kw in (cases if nref > 0 and T is types[0] else []):      # (the fill takes its time: the first dtype alone)
            above, c = "above" in kw, list(kw.values())[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if kind == "scalar":
                hostf = S.to_host(flow.p)
            else:
                hostf = S.to_host(S.metric(scratch, kind, flow.u))
            v = RR.box_values(hostf, "scalar", 0, box[0], box[1])
            t1 = time.perf_counter()
            lab, tab, ext, n = RR.regions(v, c, above=above, lo=box[0])
            t2 = time.perf_counter()
            rg = Regions(flow, Value(kind), box=box, **kw)
            f = flow.p if kind == "scalar" else flow.u
            regions.table(rg, f)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            res = regions.table(rg, f)
            torch.cuda.synchronize()
            t4 = time.perf_counter()
            same = np.array_equal(res.lab.cpu().numpy(), lab) and np.array_equal(res.tab.cpu().numpy(), tab)
            print(f"    {name:24s} value + copy {1e3 * (t1 - t0):9.1f} ms, fill {1e3 * (t2 - t1):10.1f} ms; regions.table {1e3 * (t4 - t3):8.3f} ms wall"
                  f"   R {int(n[0])}  {'equal' if same else 'DIFFERENT'}")
            del rg, res
        if T == np.float32 and burst > 0:
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
            rg = Regions(flow, Value("lambda2"), below=level["lambda2"])
            rs = regions.RegionSeries(rg, m=8, capacity=4 * burst)
            regions.record(rs, sim, flow.u)
            with_rec = steps(burst, lambda: regions.record(rs, sim, flow.u))
            base = 0.5 * (base + steps(burst))
            print(f"  one regions.record (lambda2 below q05, 8 largest) per step for {burst} steps, wall clock: {base * 1e3:.2f} -> {with_rec * 1e3:.2f} ms per step "
                  f"(+{(with_rec / base - 1) * 100:.1f} %)")
            del rg, rs
        del sim, flow, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
