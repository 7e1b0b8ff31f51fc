#!/usr/bin/env python3
"""Slice and projection images at size^3 (waterlily_amd/render.py, csrc/wl_render.h) on the developed sphere flow of bench.py's
kind: `steps` sim_step!s, then, for Float32 and Float64, the median / min / max over `reps` calls between device events of
  - project() of omega_mag and lambda2, MAX and MEAN, along each axis: the value formed on the fly, no volume written;
  - the same images composed from what the library had before: metric() into a scratch field, then torch amax / sum over it
    (the scratch field's second pass of one write and one read);
  - one full record() (vorticity magnitude MAX along z, body mask, shade, the copy to the pinned slot started);
  - sim_step! with and without one record() after every step.
Reported, not asserted.
usage: render_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--types=f32,f64]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    from waterlily_amd import render, sim as S
    from waterlily_amd.body import AutoBody, norm2
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps = int(opt("steps", 300))
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
    R, c = size / 8, size / 2 - 1
    for T in types:
        sim = S.Simulation((size, size, size), (1.0, 0.0, 0.0), 2 * R, body=AutoBody(lambda x, t: norm2(x - c) - R), nu=2 * R / 3700, T=T)
        for _ in range(nsteps):
            S.sim_step(sim, remeasure=False)
        flow = sim.flow
        r = render.Renderer(flow)
        scratch = S.like(flow.p)
        inner = scratch[1:-1, 1:-1, 1:-1]
        item = np.dtype(T).itemsize
        print(f"{size}^3 {np.dtype(T).name} after {nsteps} steps; u {3 * size ** 3 * item / 1e9:.2f} GB, one scalar field {size ** 3 * item / 1e9:.2f} GB")
        print(f"{'':34s}{'on the fly (project)':40s}{'composed (metric + torch)':40s}ratio")
        for kind in ("omega_mag", "lambda2"):
            t_metric = timed(lambda: S.metric(scratch, kind, flow.u))
            print(f"  metric() of {kind} alone: {fmt(t_metric)}")
            for mode in ("max", "mean"):
                for axis in (0, 1, 2):
                    fly = timed(lambda: render.project(r, flow.u, kind, mode=mode, axis=axis))

                    def composed():
                        S.metric(scratch, kind, flow.u)
                        return inner.amax(dim=axis) if mode == "max" else inner.sum(dim=axis, dtype=torch.float64)
                    comp = timed(composed)
                    print(f"  {kind:10s} {mode:5s} axis {axis}:     {fmt(fly):40s}{fmt(comp):40s}{fly[0] / comp[0]:.2f}")
        kw = dict(mode="max", axis=2, clims=(0.0, 0.5))
        print(f"  record (omega_mag MAX along z, body mask, shade, copy started): {fmt(timed(lambda: render.record(r, sim, 'omega_mag', **kw)))}")

        def steps(rec):
            def one():
                S.sim_step(sim, remeasure=False)
                if rec:
                    render.record(r, sim, "omega_mag", **kw)
            return one
        a, b = timed(steps(False)), timed(steps(True))
        print(f"  sim_step!                      {fmt(a)}")
        print(f"  sim_step! + record             {fmt(b)}   (+{b[0] - a[0]:.3f} ms per step)")
        r.frames.clear()
        del sim, flow, r, scratch, inner
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
