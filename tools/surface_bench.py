#!/usr/bin/env python3
"""SurfaceLoads.record at size^3 Float32 (waterlily_amd/surface.py, csrc/wl_surface.h) on icospheres of radius size/8 at
subdivision 3, 5 and 6 (1 280 / 20 480 / 81 920 triangles: the meshes of tools/mesh_bench.py), against the COMPOSED path to
the same twelve numbers on what the package had before, in the same process on the same developed flow:
  * composed, device-resident: geometry by torch, 7 wl_interp launches (p at X; the staggered u at X +- e_j/2: 19 entries),
    the traction, the loads and the moments by torch, nothing brought to the host;
  * composed, public API: the same with probes.interp (7 synchronous calls through numpy), what a user writes today;
  * "moving": either of them with the host-side transform of every vertex and its upload before each sample.
Timed between two device events (the synchronous public path: wall clock), 3 warm-up repetitions, the median, minimum and
maximum of `reps`.  Then sim_step! of the static mesh with and without a record after every step, A/B in one process (as
tools/integrals_bench.py), and with --flow the issue's Re 250 icosphere (subdivision 4, radius 16, 96x64x64): Fp and Fv at
delta = 0, 1, 2, 3 next to pressure_force / viscous_force -- reported, not asserted.
usage: surface_bench.py [size=512] [reps=25] [--flow] [--steps=<n, default 200>]"""
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import mesh_shapes as MS
    from waterlily_amd import probes as P, sim as S, surface
    from waterlily_amd.mesh import MeshBody
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    nsteps = int(next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--steps=")), 200))
    prop = torch.cuda.get_device_properties(0)
    print(f"# {' '.join(sys.argv)}   device {prop.name} ({getattr(prop, 'gcnArchName', '')}, {prop.multi_processor_count} CUs)")

    def timed(fn, events=True):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            if events:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), float(min(ms)), float(max(ms))

    def composed(flow, mb, delta, nu, x0, public, moving):
        """the twelve totals without wl_surface_sample: returns a function doing one sample"""
        dev = flow.device
        tri = torch.from_numpy(mb.triangles.astype(np.int64)).to(dev)
        x0d = torch.tensor(x0, dtype=torch.float64, device=dev)
        state = {"v": torch.from_numpy(mb.vertices).to(dev)}
        nt = len(mb.triangles)
        out3 = [torch.empty((nt, 3), dtype=torch.float64, device=dev) for _ in range(2)]
        out1 = torch.empty((nt, 1), dtype=torch.float64, device=dev)

        def vec(X, k):
            if public:
                return torch.from_numpy(P.interp(X.cpu().numpy(), flow.u)).to(dev)
            P._interp_dev(flow.u, 3, X.contiguous(), out3[k], 3, 3)
            return out3[k]

        def one():
            if moving:   # the host transforms every vertex (here by the identity: the arithmetic and the upload are the cost)
                state["v"] = torch.from_numpy(mb.vertices @ np.eye(3) + np.zeros(3)).to(dev)
            a, b, c = (state["v"][tri[:, k]] for k in range(3))
            xc = (a + b + c) / 3.0
            Sv = 0.5 * torch.linalg.cross(b - a, c - a)
            area = torch.linalg.norm(Sv, dim=1, keepdim=True)
            n = Sv / area
            X = xc + delta * n + 1.5
            if public:
                pt = torch.from_numpy(P.interp(X.cpu().numpy(), flow.p)).to(dev)[:, None]
            else:
                P._interp_dev(flow.p, 0, X.contiguous(), out1, 1, 3)
                pt = out1
            G = []
            for j in range(3):
                e = torch.zeros(3, dtype=torch.float64, device=dev)
                e[j] = 0.5
                G.append(vec(X + e, 0) - vec(X - e, 1))
            G = torch.stack(G, dim=2)                                   # G[t, i, j]
            tau = -nu * torch.einsum("tij,tj->ti", G + G.transpose(1, 2), n)
            fp, fv = pt * Sv, tau * area
            d = xc - x0d
            return torch.cat([fp.sum(0), fv.sum(0), torch.linalg.cross(d, fp).sum(0), torch.linalg.cross(d, fv).sum(0)])
        return one

    r, c = size / 8, (size / 2 - 1,) * 3
    bodies = {sub: MeshBody(*MS.icosphere(c, r, sub)) for sub in (3, 5, 6)}
    sim = S.Simulation((size,) * 3, (1.0, 0.0, 0.0), 2 * r, nu=2 * r / 3700, body=bodies[6], T=np.float32)
    for _ in range(6):
        S.sim_step(sim, remeasure=False)
    torch.cuda.synchronize()
    for sub, mb in bodies.items():
        ns = types.SimpleNamespace(flow=sim.flow, body=mb, eps=sim.eps)
        mb.native(0.0, sim.eps)
        sl = surface.SurfaceLoads(ns)
        surface.record(sl, ns)
        got = surface.series(sl)[1][-1]
        ref = composed(sim.flow, mb, sl.delta, sim.flow.nu, sl.x0, False, False)().cpu().numpy()
        nt = sl.nt
        print(f"{size}^3 Float32, icosphere sub {sub} ({nt} triangles), delta {sl.delta:g}: kernel Fp={got[:3]} Fv={got[3:6]}; "
              f"max |kernel - composed| / max |kernel| = {np.abs(got - ref).max() / np.abs(got).max():.2e}")
        fused = timed(lambda: surface.record(sl, ns))
        print(f"  record (1 sample + 2 reduction launches)        %9.4f ms (min %.4f, max %.4f)" % fused)
        only = timed(lambda: surface.sample(sl, ns))
        print(f"  sample alone                                    %9.4f ms (min %.4f, max %.4f)   {19 * 8 * nt} corner loads, "
              f"{nt * (96 + 104) + 19 * 8 * 4 * nt} B moved" % only)
        for public, moving, name in ((False, False, "composed, device-resident, static geometry    "), (False, True, "composed, device-resident, moving (host xform)"),
                                     (True, False, "composed, public probes.interp, static        "), (True, True, "composed, public probes.interp, moving        ")):
            m = timed(composed(sim.flow, mb, sl.delta, sim.flow.nu, sl.x0, public, moving), events=not public)
            print(f"  {name}  %9.4f ms (min %.4f, max %.4f)" % m + f"   = {m[0] / fused[0]:.1f} x record")
        ab = {False: [], True: []}
        for _ in range(4):
            for rec in (False, True):
                S.sim_step(sim, remeasure=False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(5):
                    S.sim_step(sim, remeasure=False)
                    if rec:
                        surface.record(sl, ns)
                torch.cuda.synchronize()
                ab[rec].append((time.perf_counter() - t0) / 5 * 1e3)
        a, b = float(np.median(ab[False])), float(np.median(ab[True]))
        print(f"  sim_step! (remeasure=False): {a:.3f} ms without, {b:.3f} ms with a record after every step: {b - a:+.3f} ms "
              f"({(b - a) / a * 100:+.2f} %)  (all: {[round(x, 2) for x in ab[False]]} / {[round(x, 2) for x in ab[True]]})")
    del sim
    if "--flow" in sys.argv:
        dims, rr, cc = (96, 64, 64), 16.0, (32.0, 32.0, 32.0)
        sm = S.Simulation(dims, (1.0, 0.0, 0.0), 2 * rr, body=MeshBody(*MS.icosphere(cc, rr, 4)), nu=2 * rr / 250, T=np.float32)
        for _ in range(nsteps):
            S.sim_step(sm, remeasure=False)
        fp, fv = S.pressure_force(sm), S.viscous_force(sm)
        print(f"96x64x64 Re 250, subdivision-4 icosphere r=16, {nsteps} steps (t U/L = {S.sim_time(sm):.3f}), eps = {sm.eps}:")
        print(f"  band integrals : pressure_force = {fp}   viscous_force = {fv}")
        for delta in (0.0, 1.0, 2.0, 3.0):
            one = surface.loads(sm, delta=delta)
            F = np.array([one[k] for k in surface.COLUMNS])
            print(f"  surface delta={delta:g}: Fp = {F[:3]}   Fv = {F[3:6]}   Fp_x / pressure_force_x = {F[0] / fp[0]:.4f}   "
                  f"Fv_x / viscous_force_x = {F[3] / fv[0]:.4f}")


if __name__ == "__main__":
    main()
