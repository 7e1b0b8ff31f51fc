#!/usr/bin/env python3
"""Integrals.record at 512^3 (waterlily_amd/integrals.py, csrc/wl_integrals.h) against the COMPOSED path to the same numbers
on the operators the package had before: metric("ke") -> wl_sum, metric("omega_mag") -> wl_dot, divergence -> wl_dot and
wl_max, each through one scratch field and each reduction a host synchronisation (9 reads of a velocity component, 3 scratch
writes, 4 scratch reads = 16 field passes against the 3 compulsory ones).  S has no composed equivalent and is left out of the
baseline, and so are umax and P (more passes still): the baseline is the cheaper side of the comparison.

Both are timed in this process on the same field: median of `reps` repetitions, each between two device events, after 3
warm-up repetitions.  Then the 512^3 sphere's sim_step! with and without record after every step, A/B in one process (as
tools/ab_step.py).
usage: integrals_bench.py [size=512] [reps=25]            timings
       integrals_bench.py --steps <n> <0|1> [size=512]     n steady steps of the sphere, with (1) or without (0) record after every
                                                           step: the target of a rocprofv3 kernel trace (tools/gaps.py reads it)
       integrals_bench.py --pmc <counter_collection.csv> <size> <f32|f64>   HBM read traffic of the sweep from a rocprofv3
                                                                            --pmc FETCH_SIZE run of this tool"""
import csv
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM = 8.0e12   # B/s, MI355X peak


def pmc(path, size, dt):
    """FETCH_SIZE (KiB; doubled: gfx950 reports half the bytes of a coalesced streaming read, profiles/parse_pmc.py) of the
    k_integrals dispatches"""
    item = 4 if dt == "f32" else 8
    tname = "<float" if dt == "f32" else "<double"
    v = [2.0 * 1024.0 * float(r["Counter_Value"]) for r in csv.DictReader(open(path))
         if r["Counter_Name"] == "FETCH_SIZE" and "k_integrals<" in r["Kernel_Name"] and tname in r["Kernel_Name"]]
    need = 3 * (size + 2) ** 3 * item
    if not v:
        raise SystemExit("no k_integrals dispatch of that type in " + path)
    m = float(np.median(v))
    print(f"k_integrals {size}^3 {dt}: HBM reads (FETCH_SIZE, corrected) median {m / 1e9:.3f} GB over {len(v)} dispatches "
          f"[{min(v) / 1e9:.3f} .. {max(v) / 1e9:.3f}] = {m / need:.2f} x the compulsory {need / 1e9:.3f} GB")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--pmc":
        return pmc(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    import torch
    import bench
    from waterlily_amd import _lib, integrals as I, sim as S
    if len(sys.argv) > 1 and sys.argv[1] == "--steps":
        n, rec = int(sys.argv[2]), sys.argv[3] == "1"
        sim = bench.sphere((int(sys.argv[4]) if len(sys.argv) > 4 else 512,) * 3, np.float32)
        ig = I.Integrals(sim.flow, U=(1.0, 0.0, 0.0))
        for k in range(5 + n):
            S.sim_step(sim, remeasure=False)
            if rec and k >= 5:
                I.record(ig, sim.flow)
        torch.cuda.synchronize()
        print(f"{n} steps after 5 warm-up steps, record={'on' if rec else 'off'}, {len(ig.t)} records")
        return
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 25
    L = _lib.lib()

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

    sim = bench.sphere((size,) * 3, np.float32)
    for _ in range(6):
        S.sim_step(sim, remeasure=False)
    f32 = sim.flow.u
    lay64 = S.Layout(sim.flow.N, np.float64)
    f64 = lay64.alloc((3,), sim.flow.device)
    f64.copy_(f32)
    res = {}
    for name, u in (("Float32", f32), ("Float64", f64)):
        T = S._T(u)
        item = T.itemsize
        need = 3 * int(np.prod(u.shape[:3])) * item
        g = S._grid_of(u, 3)
        row = torch.zeros(9, dtype=torch.float64, device=u.device)
        U3 = _lib.d3((1.0, 0.0, 0.0))
        scratch = S.like(u[..., 0])
        gs = S._grid_of(scratch, 3)
        out = C.c_double()
        t = S._WLT[T]

        def fused():
            _lib.check(L.wl_flow_integrals(t, C.byref(g), S._ptr(u), U3, S._ptr(row)))

        def composed():
            S.metric(scratch, "ke", u, par=(1.0, 0.0, 0.0))
            _lib.check(L.wl_sum(t, C.byref(gs), S._ptr(scratch), C.byref(out)))
            E = out.value
            S.metric(scratch, "omega_mag", u)
            _lib.check(L.wl_dot(t, C.byref(gs), S._ptr(scratch), S._ptr(scratch), C.byref(out)))
            Z = 0.5 * out.value
            S.divergence(scratch, u)
            _lib.check(L.wl_dot(t, C.byref(gs), S._ptr(scratch), S._ptr(scratch), C.byref(out)))
            d2 = out.value
            _lib.check(L.wl_max(t, C.byref(gs), S._ptr(scratch), C.byref(out)))
            return E, Z, d2, out.value

        scratch.zero_()
        fused()
        got = row.cpu().numpy()
        ref = composed()
        print(f"{size}^3 {name}: fused E={got[0]:.10g} Z={got[1]:.10g} div2={got[3]:.6g} divmax={got[4]:.6g}   "
              f"composed E={ref[0]:.10g} Z={ref[1]:.10g} div2={ref[2]:.6g} max(div)={ref[3]:.6g}")
        mf, lof, hif = timed(fused)
        mc, loc, hic = timed(composed)
        res[name] = (mf, mc)
        print(f"{size}^3 {name}: fused record   {mf:8.3f} ms (min {lof:.3f}, max {hif:.3f})   compulsory {need / 1e9:.3f} GB "
              f"-> {need / mf / 1e9:.2f} TB/s = {need / mf / 1e9 / (HBM / 1e12) * 100:.1f} % of 8 TB/s   [E Z S div2 divmax umax P]")
        print(f"{size}^3 {name}: composed path  {mc:8.3f} ms (min {loc:.3f}, max {hic:.3f})   16 passes = {16 * need / 3 / 1e9:.3f} GB "
              f"-> {16 * need / 3 / mc / 1e9:.2f} TB/s   [E Z div2 max(div) only: S, umax, P have no composed equivalent here]")
        print(f"{size}^3 {name}: fused is {mc / mf:.2f}x faster than the composed path (median of {reps})")
        del scratch
    del f64
    # ---- the step with and without a record after it
    ig = I.Integrals(sim.flow, U=(1.0, 0.0, 0.0))
    ab = {False: [], True: []}
    for r in range(4):
        for rec in (False, True):
            S.sim_step(sim, remeasure=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                S.sim_step(sim, remeasure=False)
                if rec:
                    I.record(ig, sim.flow)
            torch.cuda.synchronize()
            ab[rec].append((time.perf_counter() - t0) / 5 * 1e3)
    a, b = float(np.median(ab[False])), float(np.median(ab[True]))
    print(f"sim_step! {size}^3 Float32 sphere: {a:.3f} ms without, {b:.3f} ms with record after every step: {b - a:+.3f} ms "
          f"({(b - a) / a * 100:+.1f} %)  (all: {[round(x, 2) for x in ab[False]]} / {[round(x, 2) for x in ab[True]]})")
    t, v = I.series(ig)
    print(f"last record: t={t[-1]:.4f} " + " ".join(f"{n}={x:.8g}" for n, x in zip(I.columns(ig), v[-1])))


if __name__ == "__main__":
    main()
