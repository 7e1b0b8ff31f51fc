#!/usr/bin/env python3
"""Two-point statistics at size^3 (waterlily_amd/twopoint.py, csrc/wl_twopoint.h) on the developed sphere flow of bench.py:
`steps` sim_step!s, then for Float32 and Float64, for the values u (centre component 0) and lambda2, along each axis, for nsep =
16, 64 and 256 (not periodic) and nsep = n (periodic), the median / min / max over `reps` calls between device events of
twopoint.measure, against
  1. the same ten columns composed from what the library had before: the value as a Float64 volume (metric() into a scratch
     field first for lambda2), then per separation two slices (torch.roll for the wrap) and nine torch reductions.  One
     evaluation reads the volume about 15 times per separation, so it is timed over `base_reps` calls (1 beyond nsep = 64);
  2. for the bare covariance column of the periodic case, torch.fft.rfft along the axis in the field's own precision: the
     power summed over the lines, one irfft of n numbers.
With each TwoPoint time: the pairs per second and the double operations per second they stand for (17 per pair: d, d2, six
products, nine additions).  Reported, not asserted.
usage: twopoint_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--types=f32,f64] [--base-reps=<n, default 3>]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS_PER_PAIR = 17


def main():
    import torch
    import bench
    from waterlily_amd import sim as S, twopoint
    from waterlily_amd.twopoint import TwoPoint, Value
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps, base_reps = int(opt("steps", 300)), int(opt("base-reps", 3))
    types = [{"f32": np.float32, "f64": np.float64}[t] for t in opt("types", "f32,f64").split(",")]
    prop = torch.cuda.get_device_properties(0)
    print(f"# {' '.join(sys.argv)}   device {prop.name} ({getattr(prop, 'gcnArchName', '')}, {prop.multi_processor_count} CUs)")

    def timed(fn, n, warm=3):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    fmt = lambda t: f"{t[0]:9.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"

    for T in types:
        sim = bench.sphere((size, size, size), T)
        for _ in range(nsteps):
            S.sim_step(sim, remeasure=False)
        flow = sim.flow
        scratch = S.like(flow.p)
        ins = (slice(1, -1),) * 3
        n = size
        item = np.dtype(T).itemsize
        print(f"{size}^3 {np.dtype(T).name} after {nsteps} steps; u {3 * size ** 3 * item / 1e9:.2f} GB, one scalar field {size ** 3 * item / 1e9:.2f} GB")
        print(f"  {'value axis nsep':28s}{'wl_twopoint (twopoint.measure)':44s}{'composed (torch slices)':44s}ratio   Gpair/s  Tops/s")

        def volume(kind):
            """the value over inside() as a Float64 volume"""
            if kind == "lambda2":
                S.metric(scratch, "lambda2", flow.u)
                return scratch[ins].double()
            u0 = flow.u[..., 0]
            return (u0[1:-1, 1:-1, 1:-1].double() + u0[2:, 1:-1, 1:-1].double()) / 2.0

        def native(kind):
            """the value in the field's own precision (the FFT baseline)"""
            if kind == "lambda2":
                S.metric(scratch, "lambda2", flow.u)
                return scratch[ins]
            u0 = flow.u[..., 0]
            return (u0[1:-1, 1:-1, 1:-1] + u0[2:, 1:-1, 1:-1]) / 2

        def composed(kind, axis, nsep, periodic):
            out = torch.empty(nsep, 10, dtype=torch.float64, device=flow.device)
            v = volume(kind)
            lines = float(n * n)
            for r in range(nsep):
                if periodic:
                    a, b = v, torch.roll(v, -r, dims=axis)
                else:
                    a, b = v.narrow(axis, 0, n - r), v.narrow(axis, r, n - r)
                d = b - a
                d2 = d * d
                out[r, 0] = lines * (n if periodic else n - r)
                for q, x in enumerate((a, b, a * a, b * b, a * b, d2, d2 * d, d2 * d2, d.abs() * d2)):
                    out[r, 1 + q] = x.sum()
            return out

        def fft_cov(kind, axis):
            v = native(kind)
            F = torch.fft.rfft(v, dim=axis)
            P = (F.real * F.real + F.imag * F.imag).sum(dim=[d for d in range(3) if d != axis], dtype=torch.float64)
            c5 = torch.fft.irfft(P, n=n)                          # sum over lines and i of a(i) a(i + r), periodic
            N = float(n) ** 3
            m = v.sum(dtype=torch.float64) / N
            return c5 / N - m * m

        for kind, val in (("u centre 0", Value("centre", i=0)), ("lambda2", Value("lambda2"))):
            key = "lambda2" if kind == "lambda2" else "u"
            for axis in range(3):
                for nsep, periodic in ((16, False), (64, False), (256, False), (n, True)):
                    if nsep > n:
                        continue
                    tp = TwoPoint(flow, val, axis=axis, nsep=nsep, periodic=periodic)
                    a = timed(lambda: twopoint.measure(tp, flow.u), reps)
                    pairs = sum(float(n * n) * (n if periodic else n - r) for r in range(nsep))
                    name = f"{kind} {axis} {nsep}{' periodic' if periodic else ''}"
                    rate = f"{pairs / a[0] / 1e6:8.1f} {pairs * OPS_PER_PAIR / a[0] / 1e9:7.2f}"
                    try:
                        few = base_reps if nsep <= 64 else 1
                        b = timed(lambda: composed(key, axis, nsep, periodic), few, warm=1 if nsep <= 16 else 0)
                        print(f"  {name:28s}{fmt(a):44s}{fmt(b):44s}{a[0] / b[0]:6.4f} {rate}   (composed: {few} timed call{'s' if few > 1 else ''})")
                    except RuntimeError as e:
                        print(f"  {name:28s}{fmt(a):44s}composed path failed: {str(e).splitlines()[0][:60]}   {rate}")
                    if periodic:
                        try:
                            c = timed(lambda: fft_cov(key, axis), reps)
                            tab = twopoint.measure(tp, flow.u)
                            dev = float((twopoint.covariance(tab) - fft_cov(key, axis)).abs().max() / twopoint.covariance(tab)[0].abs())
                            print(f"      covariance alone by torch.fft.rfft ({np.dtype(T).name}): {fmt(c)}   wl_twopoint / fft = {a[0] / c[0]:.2f}   "
                                  f"largest difference of the two covariances over C(0): {dev:.2e}")
                        except RuntimeError as e:
                            print(f"      covariance alone by torch.fft.rfft: failed: {str(e).splitlines()[0][:60]}")
                    del tp
        tab = twopoint.measure(TwoPoint(flow, Value("centre", i=0), axis=2, nsep=256), flow.u)
        rho = twopoint.coefficient(tab)
        print(f"      u centre 0 along z: rho(1) {float(rho[1]):.4f}, rho(16) {float(rho[16]):.4f}, rho(255) {float(rho[255]):.4f}, "
              f"integral scale {float(twopoint.integral_scale(tab)):.2f} cells, flatness of the increments at r = 1: {float(twopoint.flatness(tab)[1]):.2f}")
        del sim, flow, scratch, tab, rho
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
