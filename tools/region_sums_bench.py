#!/usr/bin/env python3
"""Value-weighted sums per region at size^3 (waterlily_amd/regions.py: sums; csrc/wl_region_sums.h) on the developed sphere flow
of bench.py: `steps` sim_step!s, then for Float32 and Float64 and the four threshold sets of tools/regions_bench.py
  p below its 5 % quantile            1 column : p
  omega_mag above its 95 % quantile   4 columns: circulation (curl_0..2) and enstrophy (omega_mag^2)
  lambda2 below its 5 % quantile      7 columns: the same and the three omega_mag moments
  every cell IN (p below +inf)        1 column : p
  1. the median / min / max over `reps` calls between device events of regions.sums with the scale found (WL_RS_FIND) and given
     (WL_RS_GIVEN: the exponents the first call found), labels and table already made; and the time per pass from the library's
     own event brackets: the row passes (k_rs_sum alone with a given scale; k_rs_scale + k_rs_sum with a found one, so the
     figure for k_rs_scale is the DIFFERENCE of the two brackets, which takes k_rs_sum to cost the same in both modes) and the
     two passes over the rows of the table (k_rs_init + k_rs_finish);
  2. against the composed path: metric() into a scratch field per value, then torch.zeros(R, float64).index_add_ over the IN
     cells per column -- a scatter of float atomics, median of 3 -- with by how many ulps two runs of that path differ from each other and
     from the exact sums, and whether two runs of regions.sums differ at all.
Reported, not asserted.
The composed path runs beside the first two sets only: beside the lambda2 set it hung at 512^3 (cause unknown), and it was not
tried beside the all-IN set, so it is left out there.
usage: region_sums_bench.py [size=512] [reps=25] [--steps=<n, default 300>] [--types=f32,f64]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
COMPOSED = ("p below q05", "omega_mag above q95")              # the sets beside which the composed path is run


def main():
    import torch
    import bench
    from waterlily_amd import _lib, hist, regions, sim as S
    from waterlily_amd.hist import Axis, Histogram
    from waterlily_amd.regions import Regions, Value, Weight
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    size = int(args[0]) if args else 512
    reps = int(args[1]) if len(args) > 1 else 25
    opt = lambda k, d: next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith(f"--{k}=")), d)
    nsteps = int(opt("steps", 300))
    types = [{"f32": np.float32, "f64": np.float64}[t] for t in opt("types", "f32,f64").split(",")]
    prop = torch.cuda.get_device_properties(0)
    print(f"# {' '.join(sys.argv)}   device {prop.name} ({getattr(prop, 'gcnArchName', '')}, {prop.multi_processor_count} CUs)")
    L = _lib.lib()
    names = {L.wl_kernel_name(k).decode(): k for k in range(24)}

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

    def passes(fn, kclass, min_cells):
        """ms per call of the launches of one class with at least min_cells cells, from the library's event brackets"""
        _lib.check(L.wl_prof_reset())
        _lib.check(L.wl_prof_select(names[kclass], int(min_cells)))
        for _ in range(reps):
            fn()
        nl, nc, ms = C.c_int64(), C.c_int64(), C.c_double()
        _lib.check(L.wl_prof_timed(C.byref(nl), C.byref(nc), C.byref(ms)))
        _lib.check(L.wl_prof_select(-1, 0))
        _lib.check(L.wl_prof_reset())
        return ms.value / reps, nl.value // reps

    fmt = lambda t: f"{t[0]:8.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"

    def ulps(a, b):
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
        same = (a < 0) == (b < 0)
        return int((a - b).abs()[same].max()) if bool(same.any()) else 0, int((~same).sum())

    for T in types:
        sim = bench.sphere((size, size, size), T)
        for _ in range(nsteps):
            S.sim_step(sim, remeasure=False)
        flow = sim.flow
        print(f"{size}^3 {np.dtype(T).name} after {nsteps} steps", flush=True)
        level = {}
        for kind, q in (("scalar", 0.05), ("omega_mag", 0.95), ("lambda2", 0.05)):
            h = Histogram(flow, Axis(kind, bins=4096))
            level[kind] = float(hist.quantile(hist.count(h, flow.p if kind == "scalar" else flow.u), hist.edges(h), q))
            del h
        circ = [("curl", i, 1, None) for i in range(3)] + [("omega_mag", 0, 2, None)]
        cases = [("p below q05", "scalar", dict(below=level["scalar"]), [("scalar", 0, 1, None)]),
                 ("omega_mag above q95", "omega_mag", dict(above=level["omega_mag"]), circ),
                 ("lambda2 below q05", "lambda2", dict(below=level["lambda2"]), circ + [("omega_mag", 0, 1, d) for d in range(3)]),
                 ("all IN (p below inf)", "scalar", dict(below=float("inf")), [("scalar", 0, 1, None)])]
        scratch = S.like(flow.p)
        inner = (slice(1, -1),) * 3
        J = [torch.arange(1, size + 1, device=flow.device, dtype=torch.float64).view([-1 if d == a else 1 for a in range(3)]) for d in range(3)]
        for name, kind, kw, spec in cases:
            rg = Regions(flow, Value(kind), **kw)
            f = flow.p if kind == "scalar" else flow.u
            res = regions.table(rg, f)
            R = int(res.count)
            ws = [Weight(Value(k, i=i), power=p, moment=m, field=flow.p if k == "scalar" else flow.u) for k, i, p, m in spec]
            find = lambda: regions.sums(rg, res, ws)
            sm = find()
            E = sm.scale.clone()
            exact = sm.value.clone()
            again = find().value
            rerun = int((exact.view(torch.int64) != again.view(torch.int64)).sum())
            given = lambda: regions.sums(rg, res, ws, scale=E)
            eq = bool((given().value.view(torch.int64) == exact.view(torch.int64)).all())
            print(f"    {name:22s} R {R:6d}  IN {int(res.cells) / int(res.visited):.4f}  {len(ws)} column(s)  E {E.tolist()}", flush=True)
            print(f"      sums, scale found   {fmt(timed(find))}   sums, scale given {fmt(timed(given))}   (given == found: {eq}; a second call differs in {rerun} doubles)", flush=True)
            rf, nf = passes(find, "misc", 0.9 * size ** 3)
            rgv, ng = passes(given, "misc", 0.9 * size ** 3)
            sc, ns = passes(find, "scalar", 0)
            print(f"      per pass: k_rs_sum {rgv:7.3f} ms (given: {ng} row launch), k_rs_scale + k_rs_sum {rf:7.3f} ms (found: {nf} row launches; the difference, "
                  f"k_rs_scale: {rf - rgv:.3f} ms), k_rs_init + k_rs_finish {sc:6.3f} ms ({ns} launches)", flush=True)

            if name not in COMPOSED:
                print("      composed: left out", flush=True)
                del rg, res, sm
                continue
            mask = res.lab >= 0
            idx = res.lab[mask].to(torch.int64)

            def composed():
                out = torch.zeros((R, len(spec)), dtype=torch.float64, device=flow.device)
                for c, (k, i, p, m) in enumerate(spec):
                    v = (flow.p if k == "scalar" else S.metric(scratch, k, flow.u, i=i))[inner].to(torch.float64)
                    v = v * v if p == 2 else v
                    v = v if m is None else v * J[m]
                    out[:, c].index_add_(0, idx, v[mask])
                return out

            runs, ms = [], []
            for _ in range(3):                                 # (all IN: every add lands on one double; three runs are enough)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                runs.append(composed())
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            a, b = runs[1], runs[2]
            u_self, s_self = ulps(a, b)
            u_exact, s_exact = ulps(a, exact)
            print(f"      composed (metric -> scratch, index_add_) {fmt((float(np.median(ms)), min(ms), max(ms)))}   two of its runs differ by up to {u_self} ulp"
                  f" ({int((a.view(torch.int64) != b.view(torch.int64)).sum())} of {a.numel()} doubles), from the exact sums by up to {u_exact} ulp"
                  f"{f' ({s_self + s_exact} of other sign)' if s_self + s_exact else ''}", flush=True)
            del rg, res, sm, idx, mask
        del sim, flow, scratch
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
