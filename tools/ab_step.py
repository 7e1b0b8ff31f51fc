#!/usr/bin/env python3
"""In-process A/B of whole sim_step! time for one wl_set_option key.  usage: ab_step.py <size> <key> [reps [valA valB]]   (e.g. ab_step.py 256 BDIM_IN_CONVDIFF; a key is a name or a number: BDIM_IN_CONVDIFF or 27)
(WL_AB_DTYPE=f64: Float64; WL_AB_LAYOUT=dense: the reference's strides; WL_AB_BODY=donut: bench.py --body donut)
valA == valB is an A/A run: the two legs are timed and reported separately, their medians' difference is the noise floor."""
import os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from waterlily_amd import _lib, sim as S
size, key = int(sys.argv[1]), S.opt_key(sys.argv[2])
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 4
vals = (int(sys.argv[4]), int(sys.argv[5])) if len(sys.argv) > 5 else (1, 0)
L = _lib.lib()
make = bench.donut if os.environ.get('WL_AB_BODY') == 'donut' else bench.sphere
sim = make((size,) * 3, np.float64 if os.environ.get('WL_AB_DTYPE') == 'f64' else np.float32,
           padded=os.environ.get('WL_AB_LAYOUT', 'padded') != 'dense')
for _ in range(6):
    S.sim_step(sim, remeasure=False)
res = [[] for _ in vals]
for r in range(reps):
    for leg, val in enumerate(vals):
        _lib.check(L.wl_set_option(key, val))
        S.sim_step(sim, remeasure=False); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            S.sim_step(sim, remeasure=False)
        torch.cuda.synchronize()
        res[leg].append((time.perf_counter() - t0) / 5 * 1e3)
for leg, val in enumerate(vals):
    print(f"{size}^3 {S.opt_name(key)} = {val} (leg {'AB'[leg]}): median {np.median(res[leg]):.3f} ms/step  (all: {[round(x, 2) for x in res[leg]]})  n={sim.pois.n[-2:]}")
print(f"  difference of the medians, leg B - leg A: {np.median(res[1]) - np.median(res[0]):+.3f} ms/step")
