#!/usr/bin/env python3
"""MeshBody at size^3 Float32 (waterlily_amd/mesh.py, csrc/wl_mesh.h) next to the parametric Sphere of equal radius in the same
process: an icosphere of radius size/8 at subdivision 3, 5 and 6 (1 280 / 20 480 / 81 920 triangles), static and translating.
  * wl_mesh_create (host: pseudonormals, bins) and the first measure! (which uploads the bins), wall clock;
  * measure! per call: device events around wl_measure_rows(_mesh) + wl_measure_fill(_mesh), 3 warm-up calls, the median of
    `reps` (>= 20), the body moved a little before every call when translating;
  * sim_step! (remeasure=False) ms of the static mesh next to the sphere's, and the kernel launch counts by class
    (wl_prof_counts) over the timed steps, which MUST be equal: the stepper does not know what shape the body has -- this tool
    exits non-zero if not.  The pressure solver's classes scale with the number of V-cycles, which depends on the solution (a
    faceted sphere is another body): when the V-cycle totals of the two runs differ, every other class must be equal and a
    solver class must show the sphere run's number of launches per V-cycle exactly (a class with a per-step part besides is named
    as not comparable);
  * with --flow: the issue's 96x64x64 Re 250 icosphere (subdivision 4, radius 16) next to the Sphere, 20 steps: |dF|/|F| of the drag.
usage: mesh_bench.py [size=512] [reps=21] [--flow] [--commit=<hash>]"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import mesh_shapes as MS
    from waterlily_amd import _lib, body as B, sim as S
    from waterlily_amd.mesh import MeshBody
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = max(20, int(args[1])) if len(args) > 1 else 21
    L = _lib.lib()
    commit = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--commit=")), "")
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
        except OSError:
            commit = ""
    prop = torch.cuda.get_device_properties(0)
    print(f"# {' '.join(sys.argv)}   commit {commit or 'unknown'}   device {prop.name} ({getattr(prop, 'gcnArchName', '')}, "
          f"{prop.multi_processor_count} CUs)")
    r, c = size / 8, (size / 2 - 1,) * 3
    mk = lambda body: S.Simulation((size,) * 3, (1.0, 0.0, 0.0), 2 * r, nu=2 * r / 3700, body=body, T=np.float32)
    move = lambda: B.translation(3, v=(0.7, 0.2, -0.1))

    def measure_ms(sim, moving):
        ms = []
        for k in range(3 + reps):
            t = 0.31 * k if moving else 0.0
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            S.measure_flow(sim.flow, sim.body, t=t, eps=sim.eps)
            b.record()
            b.synchronize()
            if k >= 3:
                ms.append(a.elapsed_time(b))
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def step_ms(sim, n=10):
        for _ in range(4):
            S.sim_step(sim, remeasure=False)
        torch.cuda.synchronize()
        L.wl_prof_reset()
        n0 = len(sim.pois.n)
        t0 = time.perf_counter()
        for _ in range(n):
            S.sim_step(sim, remeasure=False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        counts = []
        for k in range(64):
            name = L.wl_kernel_name(k)
            if not name:
                break
            nl, nc = C.c_int64(), C.c_int64()
            if L.wl_prof_counts(k, C.byref(nl), C.byref(nc)) != 0:
                break
            counts.append((name.decode(), nl.value))
        return ms, counts, int(sum(sim.pois.n[n0:]))

    SOLVER = ("smooth", "restrict", "prolongate", "pcg", "dot", "scalar")

    def same_launches(counts, vc, ref_counts, ref_vc):
        """(all compared classes agree, names of the classes that could not be compared).  Equal V-cycle totals: every class
        equal.  Otherwise: every non-solver class equal, and a solver class whose count is a whole number k of launches per
        V-cycle in the sphere run must show exactly k per V-cycle here; a solver class with a per-step part besides (its
        count is not a multiple of the V-cycle total) cannot be compared from one run and is named."""
        if len(counts) != len(ref_counts):
            return False, []
        if vc == ref_vc:
            return counts == ref_counts, []
        ok, skipped = True, []
        for (a, na), (b, nb) in zip(counts, ref_counts):
            if a != b:
                return False, []
            if not a.startswith(SOLVER):
                ok = ok and na == nb
            elif nb % ref_vc == 0:
                ok = ok and na == (nb // ref_vc) * vc
            elif na != nb:
                skipped.append(a)
        return ok, skipped

    def bodies(sub):
        v, t = MS.icosphere((0.0, 0.0, 0.0), r, sub)
        t0 = time.perf_counter()
        st = MeshBody(v + np.array(c), t)
        st.handle(4.0)
        create = (time.perf_counter() - t0) * 1e3
        return st, MeshBody(v + np.array(c), t, map=move()), create

    sp = mk(B.Sphere(c, r, 3))
    print(f"{size}^3 Float32 parametric Sphere r={r:g}: measure! static %.3f ms (min %.3f, max %.3f)" % measure_ms(sp, False))
    spm = mk(B.Sphere(c, r, 3, map=move()))
    print(f"{size}^3 Float32 parametric Sphere r={r:g}: measure! translating %.3f ms (min %.3f, max %.3f)" % measure_ms(spm, True))
    del spm
    sphere_step, sphere_counts, sphere_vc = step_ms(sp)
    print(f"{size}^3 Float32 parametric Sphere: sim_step! (remeasure=False) {sphere_step:.3f} ms")
    del sp
    ok = True
    for sub in (3, 5, 6):
        st, mv, create = bodies(sub)
        t0 = time.perf_counter()
        sim = mk(st)
        torch.cuda.synchronize()
        first = (time.perf_counter() - t0) * 1e3
        i = st.info()
        print(f"icosphere sub {sub}: {i['nt']} triangles, validation + wl_mesh_create {create:.1f} ms (host), Simulation(...) with the first measure! and "
              f"the upload of the bins {first:.1f} ms; {i['bins']} bins, {i['nonempty_bins']} non-empty, max {i['max_per_bin']} / mean "
              f"{i['entries'] / max(1, i['nonempty_bins']):.1f} triangles per non-empty bin, {i['device_bytes'] / 1e6:.1f} MB on the device")
        print(f"icosphere sub {sub}: measure! static %.3f ms (min %.3f, max %.3f)" % measure_ms(sim, False))
        ms, counts, vc = step_ms(sim)
        same, skipped = same_launches(counts, vc, sphere_counts, sphere_vc)
        ok = ok and same
        print(f"icosphere sub {sub}: sim_step! (remeasure=False) {ms:.3f} ms (sphere {sphere_step:.3f} ms); {vc} V-cycles in the timed "
              f"steps (sphere {sphere_vc}); launch counts by class {'EQUAL to' if same else 'DIFFERENT from'} the sphere run's"
              + ("" if vc == sphere_vc else " (non-solver classes equal; solver classes the same number of launches per V-cycle"
                 + (f"; not comparable from one run: {', '.join(skipped)})" if skipped else ")")))
        if not same:
            print("   ", [(a, b) for a, b in zip(counts, sphere_counts) if a != b])
        del sim
        simm = mk(mv)
        print(f"icosphere sub {sub}: measure! translating %.3f ms (min %.3f, max %.3f)" % measure_ms(simm, True))
        del simm, st, mv
    if "--flow" in sys.argv:
        dims, rr, cc = (96, 64, 64), 16.0, (32.0, 32.0, 32.0)
        mk2 = lambda body: S.Simulation(dims, (1.0, 0.0, 0.0), 2 * rr, body=body, nu=2 * rr / 250, T=np.float32)
        sm, ss = mk2(MeshBody(*MS.icosphere(cc, rr, 4))), mk2(B.Sphere(cc, rr, 3))
        for _ in range(20):
            S.sim_step(sm, remeasure=False)
            S.sim_step(ss, remeasure=False)
        fm, fs = S.total_force(sm), S.total_force(ss)
        print(f"96x64x64 Re 250, 20 steps: drag of the subdivision-4 icosphere {fm[0]:.6g}, of the Sphere {fs[0]:.6g}: "
              f"|F_mesh - F_sphere| / |F_sphere| = {abs(fm[0] - fs[0]) / abs(fs[0]):.3e}; V-cycles {sm.pois.n[-6:]} vs {ss.pois.n[-6:]}")
    if not ok:
        raise SystemExit("per-step launch counts differ between the mesh and the sphere run")


if __name__ == "__main__":
    main()
