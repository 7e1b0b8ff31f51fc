#!/usr/bin/env python3
"""Budget update at 512^3 Float32 (waterlily_amd/budget.py, csrc/wl_budget.h): median of 25 device-event times of
  (a) wl_budget_update alone   (b) budget.update = (a) + the mean's wl_meanflow_update   (c) stats.update of a MeanFlow with
  uu_stats (what existed before)   (d) the same moments composed in torch from metric-style slices (timed once after one
  warm-up: nine gradient fields and the products per step)   (e) terms, once warm,
with the algorithmic bytes of (a) -- u, p, Uf, Pm read once, 13 moments read and written, on the cells of inside() -- and the
rate they imply; then the cost of one budget.update per step on the 512^3 sphere's sim_step!, A/B in one process.
usage: budget_bench.py [size=512] [reps=25]"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from waterlily_amd import _lib, budget as B, sim as S, stats as M  # noqa: E402

HBM = 8.0e12   # B/s, MI355X peak


def timed(fn, reps, warm=3):
    for _ in range(warm):
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
    return float(np.median(ms))


def torch_moments(flow, bg, eps):
    """the update of wl_budget_update written with torch slices (Float32 arithmetic; the third moment as the same merge)"""
    u, p, U, P = flow.u, flow.p, bg.mean.U, bg.mean.P
    D = 3
    I = tuple(slice(1, n - 1) for n in p.shape)

    def sh(f, *off):
        o = [0, 0, 0]
        for j in off:
            o[abs(j) - 1] += 1 if j > 0 else -1
        return f[tuple(slice(1 + s, n - 1 + s) for s, n in zip(o, f.shape))]

    def run():
        keep = 1 - eps
        d = u - U
        a = [0.5 * (sh(d[..., i]) + sh(d[..., i], i + 1)) for i in range(D)]
        gg = 0
        for i in range(D):
            for j in range(D):
                di = d[..., i]
                h = sh(di, i + 1) - sh(di) if i == j else (sh(di, j + 1) + sh(di, j + 1, i + 1) - sh(di, -(j + 1)) - sh(di, -(j + 1), i + 1)) / 4
                gg = gg + h * h
        s = a[0] * a[0] + a[1] * a[1] + a[2] * a[2]
        R = [bg.R[I + (k,)] for k in range(6)]
        tr = R[0] + R[1] + R[2]
        sym = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (0, 1): 3, (1, 2): 4, (0, 2): 5}
        for j in range(D):
            sr = sum(a[i] * R[sym[(min(i, j), max(i, j))]] for i in range(D))
            bg.T3[I + (j,)].mul_(keep).add_(s * a[j], alpha=keep * eps * (1 - 2 * eps)).sub_(2 * sr + a[j] * tr, alpha=eps * keep)
        for (i, j), k in sym.items():
            R[k].add_(a[i] * a[j], alpha=eps).mul_(keep)
        q = (p - P)[I]
        for j in range(D):
            bg.PU[I + (j,)].add_(q * a[j], alpha=eps).mul_(keep)
        bg.GG[I].add_(gg, alpha=eps).mul_(keep)
    return run


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    L = _lib.lib()
    sim = bench.sphere((size,) * 3, np.float32)
    for _ in range(3):
        S.sim_step(sim, remeasure=False)
    flow = sim.flow
    nin = int(np.prod([n - 2 for n in flow.p.shape]))
    print(f"Budget update, {size}^3 Float32 flow, Float32 accumulators, inside() = {nin} cells, pitched rows, median of {reps}")
    eps = 0.05
    bg = B.Budget(flow)
    gf, ga = flow.layout.grid(), bg.layout.grid()
    ptr = lambda a: C.c_void_p(a.data_ptr())
    ua = (S._WLT[bg.flow_T], S._WLT[bg.T], C.byref(gf), ptr(flow.u), ptr(flow.p), C.byref(ga), ptr(bg.mean.U), ptr(bg.mean.P),
          ptr(bg.R), ptr(bg.PU), ptr(bg.GG), ptr(bg.T3), eps, 0)
    ma = (S._WLT[bg.flow_T], S._WLT[bg.T], C.byref(gf), ptr(flow.u), ptr(flow.p), C.byref(ga), ptr(bg.mean.U), ptr(bg.mean.P), None, None,
          eps, 0)
    kernel = lambda: _lib.check(L.wl_budget_update(*ua))

    def both():
        _lib.check(L.wl_budget_update(*ua))
        _lib.check(L.wl_meanflow_update(*ma))
    Bk = nin * 4 * (8 + 2 * 13)
    ta = timed(kernel, reps)
    print(f"(a) wl_budget_update                     {ta:8.3f} ms  {Bk / 1e9:6.2f} GB  {Bk / ta / 1e9:5.2f} TB/s  {Bk / ta / 1e9 / (HBM / 1e12) * 100:5.1f} % of 8 TB/s")
    tb = timed(both, reps)
    print(f"(b) budget.update (a + mean U, P)        {tb:8.3f} ms")
    mf = M.MeanFlow(flow, uu_stats=True)
    mu = (S._WLT[mf.flow_T], S._WLT[mf.T], C.byref(gf), ptr(flow.u), ptr(flow.p), C.byref(ga), ptr(mf.U), ptr(mf.P), ptr(mf.UU), None,
          eps, 0)
    tc = timed(lambda: _lib.check(L.wl_meanflow_update(*mu)), reps)
    print(f"(c) stats.update with uu_stats           {tc:8.3f} ms   (b) costs {tb / tc:.2f}x of it")
    del mf
    td = timed(torch_moments(flow, bg, eps), 1, warm=1)
    print(f"(d) the moments composed in torch, once  {td:8.3f} ms   (a) is {td / ta:.1f}x faster")
    torch.cuda.empty_cache()
    out = bg.layout.alloc((8,), flow.device)
    te = timed(lambda: B.terms(bg, flow.nu, out=out), 1, warm=1)
    print(f"(e) terms, once                          {te:8.3f} ms")
    # A/B on the sphere's sim_step!: one budget.update per step or none, alternating in one process
    B.reset(bg)
    res = {0: [], 1: []}
    for r in range(4):
        for on in (0, 1):
            S.sim_step(sim, remeasure=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                S.sim_step(sim, remeasure=False)
                if on:
                    B.update(bg, flow)
            torch.cuda.synchronize()
            res[on].append((time.perf_counter() - t0) / 5 * 1e3)
    a, b = float(np.median(res[0])), float(np.median(res[1]))
    print(f"sim_step! {size}^3: {a:.3f} ms without, {b:.3f} ms with one budget.update per step: +{b - a:.3f} ms "
          f"(+{(b - a) / a * 100:.1f} %)  (all: {[round(x, 2) for x in res[0]]} / {[round(x, 2) for x in res[1]]})")


if __name__ == "__main__":
    main()
