#!/usr/bin/env python3
"""MeanFlow update at 512^3 Float32 (waterlily_amd/stats.py, csrc/wl_stats.h): hipEvent time per update for
  (a) U + P   (b) + UU + pp   (c) (b) with Float64 accumulators   (d) (b) written as torch element-wise ops on the same strided
tensors (the plumbing baseline; Float32 arithmetic), with the algorithmic bytes (read u, p; read and write every accumulator,
except on the first update; elements n0*n1*n2 of the local array, padding excluded) and the rate they imply; then the cost of
one update per step on the 512^3 sphere's sim_step!, A/B in one process (as tools/ab_step.py).
usage: meanflow_bench.py [size=512] [reps=20]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from waterlily_amd import _lib, sim as S, stats as M  # noqa: E402

HBM = 8.0e12   # B/s, MI355X peak (MI355X_MICROARCH: 6.29 TB/s measured float4 copy)


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    L = _lib.lib()
    sim = bench.sphere((size,) * 3, np.float32)
    for _ in range(3):
        S.sim_step(sim, remeasure=False)
    flow = sim.flow
    ncell = int(np.prod(flow.p.shape))
    print(f"MeanFlow update, {size}^3 Float32 flow, local array {tuple(flow.p.shape)} = {ncell} elements, pitched rows")
    eps = 0.05

    def kernel(mf):
        gf, ga = flow.layout.grid(), mf.layout.grid()
        ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
        args = (S._WLT[mf.flow_T], S._WLT[mf.T], C.byref(gf), ptr(flow.u), ptr(flow.p), C.byref(ga), ptr(mf.U), ptr(mf.P),
                ptr(mf.UU), ptr(mf.pp), eps, 0)
        return lambda: _lib.check(L.wl_meanflow_update(*args))

    def torch_ops(mf):
        u, p, U, P, UU, pp = flow.u, flow.p, mf.U, mf.P, mf.UU, mf.pp
        order = M.UU_ORDER[3]

        def run():
            d = u - U
            U.add_(d, alpha=eps)
            for q, (a, b) in enumerate(order):
                UU[..., q].add_(d[..., a] * d[..., b], alpha=eps).mul_(1 - eps)
            dp = p - P
            P.add_(dp, alpha=eps)
            pp.add_(dp * dp, alpha=eps).mul_(1 - eps)
        return run

    cases = [("a", "U+P", dict(), np.float32, kernel),
             ("b", "U+P+UU+pp", dict(uu_stats=True, pp_stats=True), np.float32, kernel),
             ("c", "U+P+UU+pp, Float64 accumulators", dict(uu_stats=True, pp_stats=True), np.float64, kernel),
             ("d", "(b) as torch element-wise ops", dict(uu_stats=True, pp_stats=True), np.float32, torch_ops)]
    res = {}
    for key, what, kw, A, make in cases:
        mf = M.MeanFlow(flow, dtype=A, **kw)
        ms = timed(make(mf), reps)
        na = 4 + (7 if kw else 0)                               # accumulator arrays: U(3)+P, +UU(6)+pp
        B = ncell * (4 * 4 + na * np.dtype(A).itemsize * 2)
        res[key] = ms
        print(f"({key}) {what:34s} {ms:8.3f} ms  {B / 1e9:7.2f} GB  {B / ms / 1e9:6.2f} TB/s  {B / ms / 1e9 / (HBM / 1e12) * 100:5.1f} % of 8 TB/s"
              f"  ({B / ncell:.0f} B/element)")
        del mf
        torch.cuda.empty_cache()
    print(f"(b) vs (d): {res['d'] / res['b']:.2f}x faster")
    # A/B on the sphere's sim_step!: one update (case b) per step or none, alternating in one process
    mf = M.MeanFlow(flow, uu_stats=True, pp_stats=True)
    out = {0: [], 1: []}
    for r in range(4):
        for on in (0, 1):
            S.sim_step(sim, remeasure=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                S.sim_step(sim, remeasure=False)
                if on:
                    M.update(mf, flow)
            torch.cuda.synchronize()
            out[on].append((time.perf_counter() - t0) / 5 * 1e3)
    a, b = float(np.median(out[0])), float(np.median(out[1]))
    print(f"sim_step! {size}^3: {a:.3f} ms without, {b:.3f} ms with one update (U+P+UU+pp, Float32) per step: +{b - a:.3f} ms "
          f"(+{(b - a) / a * 100:.1f} %)  (all: {[round(x, 2) for x in out[0]]} / {[round(x, 2) for x in out[1]]})")


if __name__ == "__main__":
    main()
