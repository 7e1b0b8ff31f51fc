#!/usr/bin/env python3
"""Scene (waterlily_amd/scene.py, csrc/wl_scene.h) at size^3 Float32 on the developed sphere flow of bench.py's kind: `steps`
sim_step!s, then the lambda2 surface at the 5 % quantile level (two Histogram passes: the second one over the bin the first one
found), coloured by omega_mag.  Median / min / max over `reps` calls between device events of
  * clear, draw, shade, resolve and their sum at 1024^2 and 2048^2 with ssaa 1 and 2 (draw = (clear + draw) - clear: a draw onto
    drawn keys would skip its atomics), and the share of each kernel;
  * a sweep of large_px over 16, 64, 256 and "all lanes", for the surface alone, for the surface with a radius-size/8 icosphere of
    1 280 triangles in front (the large-triangle path), and for a close-up in which a cell is 32 pixels wide;
  * sim_step! with and without one scene.wake + scene.record per step;
and beside them iso.write_vtp of (a part of) the same triangles, timed once on the host clock, and render.image of lambda2 in
mode "min", the nearest picture there was.  With --apng=<path> it also writes a short movie of the wake with scene.save: the
vortex cores (lambda2 at 2 % of its minimum, seen from downstream) and an icosphere standing in for the AutoBody sphere, ten frames four steps apart.
Reported, not asserted.
usage: scene_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--apng=<path>]"""
import ctypes as C
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import mesh_shapes as MS
    from waterlily_amd import _lib, hist, iso, render, scene, sim as S
    from waterlily_amd.body import AutoBody, norm2
    from waterlily_amd.mesh import MeshBody
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps, apng = int(opt("steps", 300)), opt("apng", None)
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
    sim = S.Simulation((size, size, size), (1.0, 0.0, 0.0), 2 * R, body=AutoBody(lambda x, t: norm2(x - c) - R), nu=2 * R / 3700, T=np.float32)
    for _ in range(nsteps):
        S.sim_step(sim, remeasure=False)
    flow = sim.flow

    # the level: the 5 % quantile of lambda2 over inside(), refined once
    h1 = hist.Histogram(flow, hist.Axis("lambda2", bins=4096))
    cnt, e = hist.count(h1, flow.u), hist.edges(h1)
    q1 = float(hist.quantile(cnt, e, 0.05))
    k = int(torch.searchsorted(e, torch.tensor([q1], dtype=e.dtype, device=e.device), right=True).clamp(1, len(e) - 1)) - 1
    h2 = hist.Histogram(flow, hist.Axis("lambda2", bins=4096, range=(float(e[k]), float(e[k + 1]))))
    cnt2, e2 = hist.count(h2, flow.u), hist.edges(h2)
    level, core = float(hist.quantile(cnt2, e2, 0.05)), 0.02 * float(e[0])   # (core: the movie's level, 2 % of the field's minimum)
    isf = iso.Isosurface(flow, capacity=1 << 22)
    lam = S.like(flow.p)
    t_l2 = timed(lambda: S.metric(lam, "lambda2", flow.u))
    tri, val = iso.lambda2(isf, sim, level, color="omega_mag")
    nt = int(tri.shape[0])
    clims = (0.0, float(val.max()))
    print(f"{size}^3 Float32 after {nsteps} steps; lambda2 5 % quantile {level:+.4e} (first pass {q1:+.4e}): {nt} triangles "
          f"({nt * 72 / 2 ** 20:.1f} MiB, +{nt * 24 / 2 ** 20:.1f} MiB colour); clims {clims}")
    print(f"wl_metric lambda2            {fmt(t_l2)}")
    t_ext = timed(lambda: iso.lambda2(isf, sim, level, color="omega_mag"))
    print(f"iso.lambda2 (two metrics, extract + colour, one read of the count)  {fmt(t_ext)}")

    direction = (1.0, 0.6, -0.5)
    ball = MeshBody(*MS.icosphere((c, c, c), R, 3))
    btri = scene.body_triangles(ball, 0.0)
    L = _lib.lib()

    def picture(sc, cam, body=False, large_px=64):
        scene.clear(sc)
        scene.draw(sc, cam, tri, val, clims=clims, large_px=large_px)
        if body:
            scene.draw(sc, cam, btri, large_px=large_px)

    def raw_shade(sc):
        for d in sc.draws:
            v = d.val is not None
            _lib.check(L.wl_scene_shade(C.c_void_p(sc._key.ptr), sc.Wi, sc.Hi, d.base, d.nt, S._ptr(d.tri), S._ptr(d.val) if v else None, d.M,
                                        float(d.clims[0]) if v else 0.0, float(d.clims[1]) if v else 1.0, d.levels, S._ptr(d.lut) if v else None,
                                        d.color, d.light, d.ambient, d.nan_rgba, C.c_void_p(sc._rgba.ptr)))

    def raw_resolve(sc):
        _lib.check(L.wl_scene_resolve(C.c_void_p(sc._rgba.ptr), sc.Wi, sc.Hi, C.c_void_p(sc._key.ptr), sc.ssaa, scene._u8((255,) * 4),
                                      C.c_void_p(sc._out.ptr)))

    print("\nthe lambda2 surface, perspective view of the whole box, large_px = 64")
    for n in (1024, 2048):
        for ssaa in (1, 2):
            sc = scene.Scene(flow, size=(n, n), ssaa=ssaa, ring=1)
            cam = scene.Camera.fit(flow, direction, fov=30.0)
            t_clear = timed(lambda: scene.clear(sc))
            t_cd = timed(lambda: picture(sc, cam))
            t_shade, t_res = timed(lambda: raw_shade(sc)), timed(lambda: raw_resolve(sc))
            t_all = timed(lambda: (picture(sc, cam), scene.frame(sc)))
            covered = float((sc.keys != -1).double().mean())
            draw = t_cd[0] - t_clear[0]
            tot = t_clear[0] + draw + t_shade[0] + t_res[0]
            print(f"{n}^2 ssaa {ssaa}: clear {t_clear[0]:.3f}  draw {draw:.3f}  shade {t_shade[0]:.3f}  resolve {t_res[0]:.3f} ms "
                  f"(shares {100 * t_clear[0] / tot:.0f} / {100 * draw / tot:.0f} / {100 * t_shade[0] / tot:.0f} / {100 * t_res[0] / tot:.0f} %); "
                  f"all four in one go {fmt(t_all)}; {100 * covered:.1f} % of the pixels covered")
            del sc

    print("\nlarge_px sweep at 1024^2, ssaa 1: clear + draw(s)")
    sc = scene.Scene(flow, size=(1024, 1024), ring=1)
    cam = scene.Camera.fit(flow, direction, fov=30.0)
    centre = np.asarray([int(x) for x in flow.N], dtype=np.float64) / 2 - 1
    close = scene.Camera.look_at(centre - 2.0 * size * scene._unit(direction, "direction"), centre, width=size / 16.0, near=size, far=3.0 * size)
    for name, kw in (("surface", dict(cam=cam)), ("surface + icosphere", dict(cam=cam, body=True)), ("close-up (a cell = 32 px)", dict(cam=close)),
                     ("close-up + icosphere", dict(cam=close, body=True))):
        row = []
        for lp in (16, 64, 256, 1024 * 1024):
            row.append(f"{'all lanes' if lp == 1024 * 1024 else lp}: {timed(lambda: picture(sc, large_px=lp, **kw))[0]:.3f}")
        print(f"{name:28s} " + "   ".join(row) + " ms")
    t_body = timed(lambda: scene.body_triangles(ball, 0.0))
    print(f"scene.body_triangles (1280 triangles, identity pose)  {fmt(t_body)}")

    print("\nper step")
    scw = scene.Scene(flow, size=(1024, 1024), ring=8)

    def step(with_wake):
        def one():
            S.sim_step(sim, remeasure=False)
            if with_wake:
                scene.wake(scw, isf, sim, level, cam, clims=clims)
                scene.record(scw)
        return one
    a, b = timed(step(False)), timed(step(True))
    print(f"sim_step!                                    {fmt(a)}")
    print(f"sim_step! + scene.wake + scene.record (1024^2) {fmt(b)}   (+{b[0] - a[0]:.3f} ms per step)")
    scene.drain(scw)
    scw.frames.clear()

    print("\nbeside it")
    part = min(nt, 200000)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        iso.write_vtp(os.path.join(d, "part.vtp"), tri[:part], val[:part], name="omega_mag")
        dt = time.perf_counter() - t0
    print(f"iso.write_vtp of the first {part} triangles, once, host clock: {dt:.2f} s ({dt / part * 1e6:.2f} us per triangle; "
          f"{dt / part * nt:.1f} s for all {nt} at that rate)")
    r = render.Renderer(flow)
    print(f'render.image("lambda2", mode="min", axis=1)  {fmt(timed(lambda: render.image(r, sim, "lambda2", mode="min", axis=1, clims=(-4.0 * abs(level) - 1e-30, 0.0), body=False)))}')

    if apng:
        mv = scene.Scene(flow, size=(320, 240), ssaa=2, ring=4)
        mcam = scene.Camera.fit(flow, (-0.8, -0.6, -0.4), fov=30.0, aspect=320 / 240)     # from downstream: the wake is in front
        for _ in range(10):
            for _ in range(4):
                S.sim_step(sim, remeasure=False)
            scene.wake(mv, isf, sim, core, mcam, clims=(0.0, 0.5 * clims[1]))
            scene.draw(mv, mcam, btri)                         # the AutoBody sphere has no triangles: its icosphere stands in
            scene.record(mv)
        scene.save(mv, apng, fps=10)
        print(f"\n{apng}: {len(mv.frames)} frames of 320 x 240 (ssaa 2) of lambda2 = {core:+.4e} (2 % of its minimum),{os.path.getsize(apng)} bytes")


if __name__ == "__main__":
    main()
