#!/usr/bin/env python3
"""Point probes and tracers at 512^3 Float32 on the bench sphere (waterlily_amd/probes.py, csrc/wl_probe.h):
  (a) record() of 1024 probes: hipEvent time per record and host time per call; the ms one record per step adds to the
      sphere's sim_step!, A/B in one process (as tools/meanflow_bench.py)
  (b) advance() of 2^20 and 2^24 tracers, scattered (uniform over the interior) and row-sorted (sort_by_cell), with the
      cost of sort_by_cell itself; positions are restored by a device copy outside the timed window before every advance
  (c) the same Heun step written as torch ops (flat-index gathers, the same Float64 arithmetic) on the same particles
  (d) bytes per advance: distinct 128-B lines of u the two stages touch (both x-corners of every corner row, every
      component) + 48 B of positions per particle, against the time taken.
The distinct lines do not depend on the order of the particles: they are the traffic of one pass that never re-fetches a
line, which the sorted order comes close to and the scattered one does not.
usage: probe_bench.py [size=512] [reps=10]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from waterlily_amd import probes as P, sim as S  # noqa: E402

LINE = 128


def ev_time(fn, reps, before=None):
    """mean device time of fn() over reps calls (events around each call; `before` runs outside the window)"""
    for _ in range(2):
        if before:
            before()
        fn()
    torch.cuda.synchronize()
    tot = 0.0
    for _ in range(reps):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        tot += a.elapsed_time(b)
    return tot / reps


def torch_vel(u, p):
    """the staggered velocity at the points p as torch ops: flat-index gathers from u's storage, the kernel's weights and
    order in Float64 (indices clamped into the array: the benchmark keeps its points in range)"""
    D = p.shape[1]
    flat = u.as_strided((u.untyped_storage().nbytes() // u.element_size(),), (1,), 0)
    off0, st, sc = u.storage_offset(), u.stride()[:D], u.stride()[D]
    n = u.shape[:D]
    out = []
    for c in range(D):
        q = p.clone()
        q[:, c] += 0.5
        f = torch.floor(q)
        y = q - f
        i0 = f.long() - 1
        s = torch.zeros(p.shape[0], dtype=torch.float64, device=p.device)
        for k in range(1 << D):
            w, idx = None, off0 + c * sc
            for d in range(D):
                up = (k >> d) & 1
                wd = y[:, d] if up else 1.0 - y[:, d]
                w = wd if w is None else w * wd
                idx = idx + (i0[:, d] + up).clamp(0, n[d] - 1) * st[d]
            s = s + flat[idx].double() * w
        out.append(s)
    return torch.stack(out, 1)


def torch_heun(u, x, dt):
    k1 = torch_vel(u, x)
    k2 = torch_vel(u, x + dt * k1)
    return x + (0.5 * dt) * (k1 + k2)


def lines_touched(u, x, dt):
    """distinct 128-B lines of u read by both stages of one advance (per component: both x-corners of each corner row)"""
    D = x.shape[1]
    st, sc = u.stride()[:D], u.stride()[D]
    base = u.data_ptr()
    stages = [x, x + dt * torch_vel(u, x)]
    tot = 0
    for c in range(D):
        keys = []
        for p in stages:
            q = p.clone()
            q[:, c] += 0.5
            i0 = torch.floor(q).long() - 1
            for k in range(1 << (D - 1)):
                row = c * sc
                for d in range(1, D):
                    row = row + (i0[:, d] + ((k >> (d - 1)) & 1)) * st[d]
                for up in (0, 1):
                    keys.append((base + (row + i0[:, 0] + up) * u.element_size()) // LINE)
        tot += int(torch.unique(torch.cat(keys)).numel())
        del keys
    return tot


def main():
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    sim = bench.sphere((size,) * 3, np.float32)
    for _ in range(3):
        S.sim_step(sim, remeasure=False)
    flow = sim.flow
    dt = flow.dt[-2]
    print(f"probes and tracers, {size}^3 Float32 sphere, u {tuple(flow.u.shape)} pitched, dt = {dt:.4f}")
    rng = np.random.default_rng(0)
    # (a) record
    X = rng.uniform(1.5, size + 1.5, size=(1024, 3))
    pr = P.Probes(flow, X, capacity=4096)
    ms = ev_time(lambda: P.record(pr, flow), 200)
    P.reset(pr)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        P.record(pr, flow)
    host = (time.perf_counter() - t0) / 200
    torch.cuda.synchronize()
    P.reset(pr)
    print(f"(a) record, 1024 probes: {ms * 1e3:8.1f} us device (events), {host * 1e6:8.1f} us host per call (no synchronisation)")
    out = {0: [], 1: []}
    for r in range(4):
        for on in (0, 1):
            S.sim_step(sim, remeasure=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                S.sim_step(sim, remeasure=False)
                if on:
                    P.record(pr, flow)
            torch.cuda.synchronize()
            out[on].append((time.perf_counter() - t0) / 5 * 1e3)
    a, b = float(np.median(out[0])), float(np.median(out[1]))
    print(f"    sim_step! {size}^3: {a:.3f} ms without, {b:.3f} ms with one record per step: {b - a:+.3f} ms ({(b - a) / a * 100:+.1f} %)"
          f"  (all: {[round(x, 2) for x in out[0]]} / {[round(x, 2) for x in out[1]]})")
    del pr
    # (b)-(d) tracers
    dt = flow.dt[-2]
    for lg in (20, 24):
        M = 1 << lg
        x0 = rng.uniform(1.5 + 2, size + 1.5 - 2, size=(M, 3))
        tr = P.Tracers(flow, x0)
        xs0 = tr.x.clone()
        t_sort = ev_time(lambda: P.sort_by_cell(tr), 3, before=lambda: tr.x.copy_(xs0))
        tr.x.copy_(xs0)
        tr.id = torch.arange(M, device=tr.x.device)
        scat = ev_time(lambda: P.advance(tr, flow, dt), reps, before=lambda: tr.x.copy_(xs0))
        tr.x.copy_(xs0)
        tors = ev_time(lambda: torch_heun(flow.u, xs0, dt), max(2, reps // 3))
        ref = torch_heun(flow.u, xs0, dt)
        P.advance(tr, flow, dt)
        dmax = float((tr.x - ref).abs().max())
        P.sort_by_cell(tr)
        xsorted = tr.x.clone()
        srt = ev_time(lambda: P.advance(tr, flow, dt), reps, before=lambda: tr.x.copy_(xsorted))
        tr.x.copy_(xsorted)
        tors_s = ev_time(lambda: torch_heun(flow.u, xsorted, dt), max(2, reps // 3))
        L_s = lines_touched(flow.u, xsorted, dt)
        L_r = lines_touched(flow.u, xs0, dt)
        B_s, B_r = L_s * LINE + 48 * M, L_r * LINE + 48 * M
        print(f"(b) advance 2^{lg} = {M} tracers: scattered {scat:8.3f} ms, row-sorted {srt:8.3f} ms; sort_by_cell {t_sort:8.3f} ms"
              f"  (break-even after {t_sort / max(1e-9, scat - srt):.1f} steps)")
        print(f"(c)     torch ops: scattered {tors:8.3f} ms ({tors / scat:.1f}x the kernel), row-sorted {tors_s:8.3f} ms ({tors_s / srt:.1f}x);"
              f" max |kernel - torch| = {dmax:.2e}")
        print(f"(d)     distinct 128-B lines of u: {L_s} (scattered set: {L_r}); with positions {B_s / 1e9:.3f} GB = {B_s / M:.1f} B per"
              f" particle: {B_s / srt / 1e9:.2f} TB/s sorted, {B_r / scat / 1e9:.2f} TB/s scattered (which re-fetches lines)")
        del tr, xs0, xsorted, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
