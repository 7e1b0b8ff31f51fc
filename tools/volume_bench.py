#!/usr/bin/env python3
"""Volume (waterlily_amd/volume.py, csrc/wl_volume.h) at size^3 Float32 on the developed sphere flow of bench.py's kind: `steps`
sim_step!s, then |omega| (wl_metric omega_mag into a scratch field) as the cloud, clims (0, half its maximum), the "ramp" table
at strength 0.05, t_min = 1/256.  Median / min / max over `reps` calls between device events of
  * the volume alone -- wl_scene_volume by itself, and clear + volume.add + frame -- at 1024^2 and at 2048^2 with ssaa 2,
    orthographic and with fov = 30, step 1 and 0.5;
  * the same with the lambda2 surface (5 % quantile level, as tools/scene_bench.py) and an icosphere drawn first;
  * Float64: the same field copied into a Float64 flow's layout (no second simulation: the march reads the field alone);
  * sim_step! with and without one clear + volume.metric + record per step;
and, once, the composed path: per slice k one torch.nn.functional.grid_sample of the W x H sample points plus the compositing
updates in torch (Float32 sampling, so not the same bits), which also counts the samples taken and the share of them whose
opacity is zero -- the price of an empty-space skip that is not there.  Reported, not asserted.
usage: volume_bench.py [size=512] [reps=25] [--steps=<n, default 300>]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    import mesh_shapes as MS
    from waterlily_amd import hist, iso, render, scene, sim as S, volume
    from waterlily_amd.body import AutoBody, norm2
    from waterlily_amd.mesh import MeshBody
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps = int(opt("steps", 300))
    prop = torch.cuda.get_device_properties(0)
    print(f"# {' '.join(sys.argv)}   device {prop.name} ({getattr(prop, 'gcnArchName', '')}, {prop.multi_processor_count} CUs)", flush=True)

    def timed(fn, n=reps):
        for _ in range(2):
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
    R, c = size / 8, size / 2 - 1
    sim = S.Simulation((size, size, size), (1.0, 0.0, 0.0), 2 * R, body=AutoBody(lambda x, t: norm2(x - c) - R), nu=2 * R / 3700, T=np.float32)
    for _ in range(nsteps):
        S.sim_step(sim, remeasure=False)
    flow = sim.flow
    om = S.like(flow.p)
    t_om = timed(lambda: S.metric(om, "omega_mag", flow.u))
    vmax = 0.5 * float(om.max())
    clims = (0.0, vmax)
    print(f"{size}^3 Float32 after {nsteps} steps; wl_metric omega_mag {fmt(t_om)}; clims {clims}", flush=True)
    direction = (1.0, 0.6, -0.5)
    bg = (255, 255, 255, 255)
    kw = dict(strength=0.05, t_min=1.0 / 256.0)

    def composed(sc, cam, step):
        """the march restated with one grid_sample per slice (Float32): (ms, samples taken, of them with zero opacity)"""
        import torch.nn.functional as Fn
        W, H = sc.Wi, sc.Hi
        dev = flow.p.device
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        dense = om.permute(2, 1, 0).contiguous()[None, None]                        # the copy grid_sample needs: no pitch, x fastest
        t1.record()
        Mi = torch.from_numpy(cam.inverse(W, H)).to(dev)
        ds = step / (cam.far - cam.near)
        xn = ((torch.arange(W, device=dev, dtype=torch.float64) + 0.5) / W) * 2 - 1
        yn = 1 - ((torch.arange(H, device=dev, dtype=torch.float64) + 0.5) / H) * 2
        Y, X = torch.meshgrid(yn, xn, indexing="ij")
        h0 = [(Mi[r, 0] * X + Mi[r, 1] * Y) + Mi[r, 3] for r in range(4)]
        P0 = torch.stack([h0[d] / h0[3] for d in range(3)], dim=-1)
        P1 = torch.stack([(h0[d] + Mi[d, 2]) / (h0[3] + Mi[3, 2]) for d in range(3)], dim=-1)
        D = P1 - P0
        n = torch.tensor([float(x) for x in flow.N], device=dev, dtype=torch.float64)
        blo, bhi = torch.full((3,), 0.5, device=dev, dtype=torch.float64), n - 2.5
        ta, tb = (blo - P0) / D, (bhi - P0) / D
        s_in = torch.minimum(ta, tb).amax(dim=-1).clamp(min=0.0)
        s_out = torch.maximum(ta, tb).amin(dim=-1).clamp(max=1.0)
        hit = s_in <= s_out
        k_lo = max(int(float(s_in[hit].min()) / ds) - 1, 0)
        k_hi = int(float(s_out[hit].max()) / ds) + 1
        lut = sc.lut("RdBu")[:, :3].to(torch.float32)
        opac = torch.from_numpy(volume.opacity("ramp", kw["strength"], step)).to(dev).to(torch.float32)
        P0f, Df, s_inf, s_outf = P0.float(), D.float(), s_in.float(), s_out.float()
        scale = (2.0 / (n - 1)).float()
        Cc = torch.zeros((H, W, 3), device=dev, dtype=torch.float32)
        T = torch.ones((H, W), device=dev, dtype=torch.float32)
        taken = torch.zeros((), device=dev, dtype=torch.int64)
        zero = torch.zeros((), device=dev, dtype=torch.int64)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(k_lo, k_hi + 1):
            s = (k + 0.5) * ds
            grid = ((P0f + s * Df) + 0.5) * scale - 1.0                              # 0-based index coordinate J = x + 0.5, align_corners
            v = Fn.grid_sample(dense, grid[None, None], mode="bilinear", padding_mode="border", align_corners=True)[0, 0, 0]
            m = (s_inf <= s) & (s <= s_outf) & (T >= kw["t_min"])
            idx = ((v - clims[0]) / (clims[1] - clims[0]) * 256.0).floor().clamp(0, 255).long()
            al = opac[idx] * m
            taken += m.sum()
            zero += (m & (opac[idx] == 0)).sum()
            Cc += (T * al)[..., None] * lut[idx]
            T = T * (1.0 - al)
        b.record()
        b.synchronize()
        return a.elapsed_time(b), t0.elapsed_time(t1), int(taken), int(zero), k_hi - k_lo + 1

    def volume_rows(flow_, field, label, surface=None, sizes=((1024, 1), (2048, 2)), count=True):
        print(f"\n{label}", flush=True)
        for nn, ssaa in sizes:
            sc = scene.Scene(flow_, size=(nn, nn), ssaa=ssaa, ring=1)
            for cname, cam in (("orthographic", scene.Camera.fit(flow_, direction)), ("fov 30", scene.Camera.fit(flow_, direction, fov=30.0))):
                for step in (1.0, 0.5):
                    def picture():
                        scene.clear(sc)
                        if surface is not None:
                            surface(sc, cam)
                        volume.add(sc, cam, flow_, field, clims, step=step, **kw)
                        return scene.frame(sc, bg)
                    picture()
                    t_v = timed(lambda: volume.run(sc, scene._u8(bg)))
                    t_all = timed(picture)
                    line = f"{nn}^2 ssaa {ssaa} {cname:12s} step {step}: wl_scene_volume {fmt(t_v)}; clear + add + frame {fmt(t_all)}"
                    if count and ssaa == 1:
                        ms, ms_copy, taken, zero, nk = composed(sc, cam, step)
                        line += (f"\n      samples taken {taken:.3e} ({taken / (nn * nn):.0f} per ray), {taken / t_v[0] / 1e6:.1f} G samples/s; "
                                 f"{100 * zero / max(taken, 1):.1f} % of them with zero opacity; composed path ({nk} slices, once): {ms:.1f} ms "
                                 f"+ {ms_copy:.1f} ms for its dense copy ({om.numel() * 4 / 2 ** 20:.0f} MiB)")
                    print(line, flush=True)
            del sc

    volume_rows(flow, om, "the volume alone (omega_mag, ramp 0.05, t_min 1/256)")

    # the lambda2 surface and a body first (tools/scene_bench.py's level and icosphere)
    h1 = hist.Histogram(flow, hist.Axis("lambda2", bins=4096))
    cnt, e = hist.count(h1, flow.u), hist.edges(h1)
    q1 = float(hist.quantile(cnt, e, 0.05))
    k = int(torch.searchsorted(e, torch.tensor([q1], dtype=e.dtype, device=e.device), right=True).clamp(1, len(e) - 1)) - 1
    h2 = hist.Histogram(flow, hist.Axis("lambda2", bins=4096, range=(float(e[k]), float(e[k + 1]))))
    level = float(hist.quantile(hist.count(h2, flow.u), hist.edges(h2), 0.05))
    isf = iso.Isosurface(flow, capacity=1 << 22)
    tri, val = iso.lambda2(isf, sim, level, color="omega_mag")
    ball = MeshBody(*MS.icosphere((c, c, c), R, 3))
    btri = scene.body_triangles(ball, 0.0)
    sclims = (0.0, float(val.max()))

    def surface(sc, cam):
        scene.draw(sc, cam, tri, val, clims=sclims)
        scene.draw(sc, cam, btri)
    volume_rows(flow, om, f"with the lambda2 surface ({int(tri.shape[0])} triangles) and an icosphere drawn first", surface=surface, count=False)

    flow64 = S.Flow((size, size, size), (1.0, 0.0, 0.0), T=np.float64)
    om64 = S.like(flow64.p)
    om64.copy_(om)
    volume_rows(flow64, om64, "Float64 (the same values in a Float64 flow's layout)", sizes=((1024, 1),), count=False)
    del flow64, om64

    print("\nper step", flush=True)
    scw = scene.Scene(flow, size=(1024, 1024), ring=8)
    cam = scene.Camera.fit(flow, direction, fov=30.0)

    def step_fn(with_volume):
        def one():
            S.sim_step(sim, remeasure=False)
            if with_volume:
                scene.clear(scw)
                volume.metric(scw, cam, sim, "omega_mag", clims=clims, **kw)
                scene.record(scw)
        return one
    a, b = timed(step_fn(False)), timed(step_fn(True))
    print(f"sim_step!                                                     {fmt(a)}")
    print(f"sim_step! + clear + volume.metric + scene.record (1024^2)     {fmt(b)}   (+{b[0] - a[0]:.3f} ms per step)")
    scene.drain(scw)
    r = render.Renderer(flow)
    print(f'beside it: render.image("omega_mag", mode="max", axis=1)      {fmt(timed(lambda: render.image(r, sim, "omega_mag", mode="max", axis=1, clims=clims, body=False)))}')


if __name__ == "__main__":
    main()
