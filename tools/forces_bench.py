#!/usr/bin/env python3
"""Forces.record at 512^3 (waterlily_amd/forces.py, csrc/wl_forces.h) against the COMPOSED path to the same numbers with the
functions the package had before -- pressure_force(sim), viscous_force(sim), pressure_moment(x0, sim) as they stand: three
kernels and three blocking copies of three doubles, and for a moving body one rebuild of the band per step before them
(wl_body_nds, a torch compaction, band_to_device_t).  The composed path yields Fp, Fv and Mp only: Mv, the power, ncells,
the area and the leaves have no composed equivalent, so the baseline is the cheaper side of the comparison.

Two bodies, both types:
  sphere    the bench sphere (bench.sphere: torch closures), static, sim_step!(remeasure=False).  Its band is cached by the
            composed path after the first call; record takes the same stored band (wl_band_loads).
  cylinder  bench.moving_cylinder (parametric, native), measure! every step.  The composed path rebuilds its band at every new
            flow time; here that is forced before every repetition (sim._band = None), as a step would.  record evaluates the
            body in registers (wl_body_loads).
Every figure is the median of `reps` repetitions in this process on the same fields, after 3 warm-up repetitions: `events` between
two device events (what the stream is busy or blocked for), `wall` the host time of a call, from a loop of `reps` calls closed by one
synchronisation for record and per call for the composed path (which synchronises itself).  Then sim_step! with and without a
record after every step, A/B in one process (as tools/integrals_bench.py): the sphere in Float32, the cylinder in Float64.
usage: forces_bench.py [size=512] [reps=25]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import bench
    from waterlily_amd import forces as F, sim as S
    size = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 25

    def events(fn):
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

    def wall_each(fn):
        ms = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms))

    def wall_loop(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        host = (time.perf_counter() - t0) / reps * 1e3
        torch.cuda.synchronize()
        return host, (time.perf_counter() - t0) / reps * 1e3

    for bname, make, moving in (("sphere", bench.sphere, False), ("cylinder", bench.moving_cylinder, True)):
        for tname, T in (("Float32", np.float32), ("Float64", np.float64)):
            sim = make((size,) * 3, T)
            for _ in range(4):
                S.sim_step(sim, remeasure=moving)
            x0 = tuple(n / 2 for n in sim.flow.N[:3])
            fr = F.Forces(sim, x0=x0, capacity=8 * reps + 64)

            def fused():
                F.record(fr, sim)

            def composed():
                if moving:
                    sim._band = None                      # a new flow time: the band is rebuilt, as after every step
                return S.pressure_force(sim), S.viscous_force(sim), S.pressure_moment(x0, sim)

            ref = composed()
            got = F.loads(sim, x0)
            tag = f"{size}^3 {tname} {bname} ({'moving, native' if moving else 'static, stored band'}, {got['ncells']} cells)"
            print(f"{tag}: fused Fp={got['Fp']} Fv={got['Fv']} Mp={got['Mp']} Wp={got['Wp']:.6g} area={got['area']:.6g}")
            print(f"{tag}: composed Fp={ref[0]} Fv={ref[1]} Mp={ref[2]}")
            mf, lof, hif = events(fused)
            mc, loc, hic = events(composed)
            host, through = wall_loop(fused)
            wc = wall_each(composed)
            print(f"{tag}: record        events {mf:8.4f} ms (min {lof:.4f}, max {hif:.4f})   wall {host:.4f} ms host per call, "
                  f"{through:.4f} ms per call with one synchronisation after {reps}   [16 columns x {fr.nleaf + 1} rows]")
            print(f"{tag}: composed path events {mc:8.4f} ms (min {loc:.4f}, max {hic:.4f})   wall {wc:.4f} ms per call (it "
                  f"synchronises)   [Fp Fv Mp only]")
            print(f"{tag}: record / composed = {mf / mc:.3f} by events, {through / wc:.3f} by wall: record is "
                  f"{mc / mf:.2f}x / {wc / through:.2f}x {'faster' if mc > mf else 'SLOWER'} (median of {reps})")
            if (T is np.float32) != moving:       # the step's A/B: the sphere in Float32, the cylinder in Float64 (in Float32 its
                                                  # pressure solver stalls at this size, see bench.py --body, and the fields are NaN)
                F.reset(fr)
                ab = {False: [], True: []}
                for r in range(4):
                    for rec in (False, True):
                        S.sim_step(sim, remeasure=moving)
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(5):
                            S.sim_step(sim, remeasure=moving)
                            if rec:
                                F.record(fr, sim)
                        torch.cuda.synchronize()
                        ab[rec].append((time.perf_counter() - t0) / 5 * 1e3)
                a, b = float(np.median(ab[False])), float(np.median(ab[True]))
                print(f"sim_step! {size}^3 {tname} {bname}: {a:.3f} ms without, {b:.3f} ms with record after every step: {b - a:+.3f} ms "
                      f"({(b - a) / a * 100:+.2f} %)  (all: {[round(x, 2) for x in ab[False]]} / {[round(x, 2) for x in ab[True]]})")
                t, v = F.series(fr)
                print(f"last record: t={t[-1]:.4f} " + " ".join(f"{n}={x:.6g}" for n, x in zip(F.columns(), v[-1, -1])))
            del sim, fr
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
