"""The tile map of the z-marching kernels on the device (waterlily_amd/csrc/wl_tilemap.h, WL_OPT_SWEEP_ALTERNATE): whole z-chunks
dealt round-robin to the XCDs (option value 1, the default), one contiguous slab of z per XCD (3), and dealt chunks without
alternating sweeps (0) step the benchmark's sphere to the SAME BITS -- a workgroup takes another tile, every tile computes
the same cells and its reduction partial goes to the same slot.  Three `sim_step!(remeasure=false)` per run; u, p, f, sigma,
every dt and pois.n are compared exactly.  The shapes are the smallest at which the map can go wrong: 64 and 48 planes give
64 and 48 one-plane chunks (a multiple of 8: dealt), 44 planes give 44 (the contiguous map is kept), and the z-periodic
case appends the partials of its ghost_z shell after the tiles' partials.  wl_prof_dealt counts the launches that dealt."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bench
from waterlily_amd import _lib
from waterlily_amd import sim as S
from waterlily_amd.body import AutoBody
from waterlily_amd.sim import Opt


def dealt_launches():
    n = C.c_int64()
    _lib.check(_lib.lib().wl_prof_dealt(C.byref(n)))
    return n.value


def periodic_sphere(dims, T):
    """bench.sphere with z periodic (bench.sphere takes no perdir)"""
    m = min(dims)
    radius = m / 8
    cx, cy, cz = m / 2 - 1, dims[1] / 2 - 1, dims[2] / 2 - 1
    body = AutoBody(lambda x, t: torch.sqrt((x[0] - cx) ** 2 + (x[1] - cy) ** 2 + (x[2] - cz) ** 2) - radius)
    return S.Simulation(tuple(dims), (1.0, 0.0, 0.0), 2 * radius, nu=2 * radius / 3700.0, body=body, T=T, perdir=(2,))


CASES = {
    "64-f32": ((64, 64, 64), np.float32, bench.sphere, True),
    "64-f64": ((64, 64, 64), np.float64, bench.sphere, True),
    "96x64x48-f32": ((96, 64, 48), np.float32, bench.sphere, True),
    "64x64x44-f32-fallback": ((64, 64, 44), np.float32, bench.sphere, False),
    "64-f32-z-periodic": ((64, 64, 64), np.float32, periodic_sphere, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_dealt_slabs_and_ascending_sweeps_give_the_same_bits(case):
    dims, T, make, engaged = CASES[case]

    def run(value):
        with S.options({Opt.SWEEP_ALTERNATE: value}):
            n0 = dealt_launches()
            sim = make(dims, T)
            for _ in range(3):
                S.sim_step(sim, remeasure=False)
            torch.cuda.synchronize()
            return sim, dealt_launches() - n0
    (a, na), (b, nb), (c, nc) = run(1), run(3), run(0)
    print(f"{case}: launches that dealt their chunks: {na} (value 1), {nb} (3), {nc} (0); pois.n = {a.pois.n}")
    assert nb == 0                                   # bit 1: the contiguous slabs, whatever the shape
    if engaged:
        assert na > 0 and nc == na                   # the dealt map was really taken, with and without alternation
    else:
        assert na == 0 and nc == 0                   # 44 chunks (22, 11 on the coarser levels): no launch can deal
    for other in (b, c):
        assert a.pois.n == other.pois.n and a.flow.dt == other.flow.dt and len(a.flow.dt) == 4
        for k in ("u", "p", "f", "sigma"):
            assert torch.equal(getattr(a.flow, k), getattr(other.flow, k)), k
