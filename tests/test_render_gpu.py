"""Render on the GPU (waterlily_amd.render: wl_render_project, wl_render_shade) against the numpy restatement
tests/render_ref.py, bit for bit and byte for byte.

Shapes (interior cells) are test_iso_cpu.SHAPES -- (70, 9, 7) an x-row longer than 64 lanes and no multiple of it, (33, 12, 10) a
row shorter than 64, (64, 5, 5) -- and the 2-D (70, 9) and (33, 12); Float32 and Float64, padded and dense; fields are seeded
standard_normal, ghost cells included.

Why equality: the modes use additions, comparisons and one division in an order the contract fixes, and the library is built
without contraction; the metric kinds call the device function wl_metric's kernel calls, so the yardstick for them is the
host copy of what wl_metric stored for the same u (the xref tests hold wl_metric itself).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as RR  # noqa: E402
from test_iso_cpu import SHAPES  # noqa: E402

from waterlily_amd import _lib, render, sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES_ALL = list(SHAPES) + [(70, 9), (33, 12)]
CASES = [(sh, T, pad) for sh in SHAPES_ALL for T in (F32, F64) for pad in (True, False)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for sh, T, pad in CASES]
MODES = ("slice",) + RR.MODES


@functools.lru_cache(maxsize=None)
def fields(shape, T):
    """(p, u) host arrays with ghosts, seeded (read-only)"""
    Ng = tuple(n + 2 for n in shape)
    rng = np.random.default_rng(7)
    p = np.asfortranarray(rng.standard_normal(Ng).astype(T))
    u = np.asfortranarray(rng.standard_normal(Ng + (len(shape),)).astype(T))
    return p, u


def make(shape, T, padded, **kw):
    flow = S.Flow(shape, (0.0,) * len(shape), T=T, padded=padded)
    p, u = fields(shape, T)
    S.upload(flow.p, p)
    S.upload(flow.u, u)
    return flow, render.Renderer(flow, **kw), p, u


def host(x):
    return x.cpu().numpy().copy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def boxes(Ng):
    """the default box (inside) and one interior box"""
    D = len(Ng)
    return [None, (tuple([3, 2, 1][:D]), tuple([Ng[0] - 4, Ng[1] - 3, Ng[2] - 2 if D == 3 else 0][:D]))]


def ref_image(vals, axis, mode, index_in_box=None):
    if mode == "slice":
        sl = [slice(None)] * 3
        sl[axis] = slice(index_in_box, index_in_box + 1)
        return RR.project(vals[tuple(sl)], axis, "max")
    return RR.project(vals, axis, mode)


def sweep(r, f, kind, c, href, Ng, what, **par):
    """every mode along every axis on both boxes: project() against the ref applied to `href` (values(kind) of the host field)"""
    D = len(Ng)
    n = 0
    for box in boxes(Ng):
        lo, hi = ((1,) * D, tuple(m - 1 for m in Ng)) if box is None else box
        vals = RR.values(href, what, c, lo, hi)
        for axis in ((0, 1, 2) if D == 3 else (2,)):
            for mode in MODES:
                idx = (lo[axis] + hi[axis]) // 2 if D == 3 else None
                got = host(render.project(r, f, kind, mode=mode, axis=axis, index=idx, box=box, i=c, **par))
                want = ref_image(vals, axis, mode, None if idx is None else idx - lo[axis]) if D == 3 else ref_image(vals, 2, mode, 0)
                assert same_bits(got, want), (kind, c, box, axis, mode, np.abs(got - want).max())
                n += 1
    return n


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_fields_every_mode_and_axis(shape, T, padded):
    flow, r, p, u = make(shape, T, padded)
    Ng = p.shape
    n = sweep(r, flow.p, "scalar", 0, p, Ng, "scalar")
    for c in range(len(shape)):
        n += sweep(r, flow.u, "ucomp", c, u, Ng, "ucomp")
        n += sweep(r, flow.u, "centre", c, u, Ng, "centre")
    assert n == (1 + 2 * len(shape)) * 2 * (3 if len(shape) == 3 else 1) * 6
    if len(shape) == 2:                                        # the image is the field, in every mode
        img = host(render.project(r, flow.p, "scalar", mode="sum"))
        assert np.array_equal(img, p[1:-1, 1:-1].T.astype(F64))


def metric_cases(D):
    z, ctr, U = (0.2, 0.3, 1.0), (10.5, 4.0, 3.5), (0.3, -0.2, 0.1)
    out = [("ke", 0, U, None)]
    if D == 2:
        return out + [("curl", 2, None, None)]
    return out + [("curl", i, None, None) for i in range(3)] + [("omega_mag", 0, None, None), ("lambda2", 0, None, None),
                                                               ("omega_theta", 0, z, ctr)]


@pytest.mark.parametrize("shape,T,padded", CASES, ids=IDS)
def test_metric_kinds_equal_wl_metric(shape, T, padded):
    flow, r, p, u = make(shape, T, padded)
    Ng, D = p.shape, len(shape)
    scratch = S.like(flow.p)
    lo, hi = (1,) * D, tuple(m - 1 for m in Ng)
    for kind, i, par, par2 in metric_cases(D):
        scratch.zero_()
        h = S.to_host(S.metric(scratch, kind, flow.u, i=i, par=par, par2=par2))    # what the existing wl_metric stores
        vals = RR.values(h, "scalar", 0, lo, hi)
        assert np.isfinite(vals).all() and vals.std() > 0
        for axis in ((0, 1, 2) if D == 3 else (2,)):
            assert RR.absmax_ties(vals, axis) == 0                                  # the tie rule is not what decides here
            for mode in MODES:
                idx = (lo[axis] + hi[axis]) // 2 if D == 3 else None
                got = host(render.project(r, flow.u, kind, mode=mode, axis=axis, index=idx, i=i, par=par, par2=par2))
                want = ref_image(vals, axis if D == 3 else 2, mode, None if idx is None else idx - lo[axis]) if D == 3 else ref_image(vals, 2, mode, 0)
                assert same_bits(got, want), (kind, i, axis, mode, np.abs(got - want).max())


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_nan_rules(axis):
    shape, T = (70, 9, 7), F64
    flow, r, p, u = make(shape, T, True)
    at = (67, 6, 5)                                            # (x = 67: a lane's second cell on axis 0)
    inner = p[1:-1, 1:-1, 1:-1]
    assert all(p[at] < inner.max(axis=d)[tuple(a - 1 for k, a in enumerate(at) if k != d)] for d in range(3))   # not its ray's maximum
    others = [d for d in range(3) if d != axis]
    pix = (at[others[1]] - 1, at[others[0]] - 1)               # [b, a] in the default box
    base = {m: host(render.project(r, flow.p, "scalar", mode=m, axis=axis)) for m in RR.MODES}
    pn = p.copy()
    pn[at] = np.nan
    S.upload(flow.p, pn)
    got = {m: host(render.project(r, flow.p, "scalar", mode=m, axis=axis)) for m in RR.MODES}
    for m in ("sum", "mean"):                                  # one NaN cell changes its own pixel only
        changed = ~((got[m] == base[m]) | (np.isnan(got[m]) & np.isnan(base[m])))
        assert np.isnan(got[m][pix]) and changed.sum() == 1 and changed[pix]
        assert same_bits(got[m], RR.project(RR.values(pn, "scalar", 0, (1, 1, 1), tuple(n - 1 for n in pn.shape)), axis, m))
    assert p[at] < base["max"][pix] and same_bits(got["max"], base["max"])       # ... and nothing under MAX
    ray = [slice(a, a + 1) for a in at]
    ray[axis] = slice(None)
    pn[tuple(ray)] = np.nan
    S.upload(flow.p, pn)
    for m in ("max", "min", "absmax"):                         # an all-NaN ray gives NaN, and only there
        img = host(render.project(r, flow.p, "scalar", mode=m, axis=axis))
        assert np.isnan(img[pix]) and np.isnan(img).sum() == 1


@pytest.mark.parametrize("T", [F32, F64])
@pytest.mark.parametrize("zoom", [1, 3])
def test_shade_matches_the_reference(T, zoom):
    shape = (70, 9, 7)
    flow, r, p, u = make(shape, T, True, zoom=zoom)
    pn = p.copy()
    pn[5:9, 3, :] = np.nan                                     # some NaN pixels under MAX along z
    S.upload(flow.p, pn)
    nanc, maskc = (10, 20, 30, 40), (1, 2, 3, 255)
    for axis in (2, 0):
        img = render.project(r, flow.p, "scalar", mode="max", axis=axis)
        mask = render.project(r, flow.u, "centre", mode="min", axis=axis, i=0, out=r.mask)
        hi, hm = host(img), host(mask)
        mlt = float(np.median(hm))
        assert np.isnan(hi).sum() == (4 if axis == 2 else 0) and 0 < (hm < mlt).sum() < hm.size
        vmin, vmax = float(np.nanquantile(hi, 0.1)), float(np.nanquantile(hi, 0.9))   # values on both sides of the limits
        for cmap in ("RdBu", "gray"):
            for levels in (0, 10):
                for flip in (False, True):
                    for m in (None, mask):
                        got = host(render.shade(r, img, (vmin, vmax), cmap=cmap, levels=levels, mask=m, mask_lt=mlt, mask_rgba=maskc,
                                                nan_rgba=nanc, flip_y=flip))
                        want = RR.shade(hi, vmin, vmax, levels, render.colormap(cmap), mask=None if m is None else hm, mask_lt=mlt,
                                        mask_rgba=maskc, nan_rgba=nanc, zoom=zoom, flip_y=flip)
                        assert got.shape == want.shape and np.array_equal(got, want), (axis, cmap, levels, flip, m is not None)


# --------------------------------------------------------------------------- end to end: a 2-D circle

DIMS = (64, 32)                                                # arrays of (66, 34) with the ghost layer
CTR, RAD = (16.0, 16.0), 4.0


def circle_sim(steps=3):
    body = AutoBody(lambda x, t: norm2(x - CTR[0]) - RAD)
    sim = S.Simulation(DIMS, (1.0, 0.0), 2 * RAD, nu=2 * RAD / 250, body=body, T=F64)
    for _ in range(steps):
        S.sim_step(sim)
    return sim


def ref_curl_image(sim, clims, **kw):
    """image(what="curl", body=True) composed on the host from the copies of u and mu0"""
    u, mu0 = S.to_host(sim.flow.u), S.to_host(sim.flow.mu0)
    w = np.zeros(u.shape[:2], dtype=u.dtype)
    w[1:, 1:] = (u[1:, 1:, 1] - u[:-1, 1:, 1]) - (u[1:, 1:, 0] - u[1:, :-1, 0])   # curl(3, I, u), Metrics.jl:54, in T
    lo, hi = (1, 1), tuple(n - 1 for n in w.shape)
    img = RR.project(RR.values(w, "scalar", 0, lo, hi), 2, "max") * (float(sim.L) / float(sim.U))
    mask = RR.project(RR.values(mu0, "centre", 0, lo, hi), 2, "min")
    if clims is None:
        clims = (float(img.min()), float(img.max()))
    return RR.shade(img, clims[0], clims[1], kw.get("levels", 0), render.colormap(kw.get("cmap", "RdBu")), mask=mask, mask_lt=0.5,
                    flip_y=True, zoom=kw.get("zoom", 1)), mask


def test_image_of_a_circle_end_to_end():
    sim = circle_sim()
    r = render.Renderer(sim.flow, zoom=2)
    for clims, levels in ((None, 0), ((-2.0, 2.0), 10)):
        got = host(render.image(r, sim, "curl", clims=clims, levels=levels, body=True))
        want, mask = ref_curl_image(sim, clims, levels=levels, zoom=2)
        assert got.shape == (2 * DIMS[1], 2 * DIMS[0], 4) and np.array_equal(got, want)
    body = mask < 0.5                                          # [y, x] over inside(): cell I at [I_y - 1, I_x - 1]
    cx, cy = int(CTR[0] + 1.5) - 1, int(CTR[1] + 1.5) - 1      # the cell that holds the centre (loc(0, I) = I - 1.5)
    assert 0 < body.sum() < body.size / 4 and body[cy, cx]
    black = np.all(got.reshape(DIMS[1], 2, DIMS[0], 2, 4)[:, 0, :, 0] == np.array([0, 0, 0, 255], dtype=np.uint8), axis=-1)
    assert np.array_equal(black[::-1], body)                   # the body pixels are the mask, the high index at the top
    nobody = host(render.image(r, sim, "curl", clims=(-2.0, 2.0), levels=10, body=False))
    assert not np.array_equal(nobody, got)


def test_record_ring_and_apng(tmp_path):
    sim = circle_sim(steps=1)
    r = render.Renderer(sim.flow, ring=2)
    shown = []
    for _ in range(5):
        S.sim_step(sim)
        render.record(r, sim, "curl", clims=(-2.0, 2.0))
        shown.append(host(render.image(r, sim, "curl", clims=(-2.0, 2.0))))
    assert len(r.frames) == 3 and r.head - r.tail == 2         # a ring of 2: three frames were drained on the way
    path = tmp_path / "wake.png"
    render.save(r, path)
    frames, tags = RR.decode(path.read_bytes())
    assert len(frames) == 5 and tags.count(b"fdAT") == 4
    for k in range(5):
        assert np.array_equal(frames[k], shown[k]), k
        want, _ = ref_curl_image(sim, (-2.0, 2.0)) if k == 4 else (shown[k], None)
        assert np.array_equal(frames[k], want)
    assert not np.array_equal(frames[0], frames[4])
    one = tmp_path / "one.png"
    render.write_png(one, render.image(r, sim, "pressure"))    # a device tensor, limits read from the device
    assert np.array_equal(RR.decode(one.read_bytes())[0][0], host(r.rgba[:DIMS[0] * DIMS[1] * 4].view(DIMS[1], DIMS[0], 4)))


def test_sim_gif_runs_the_reference_loop(tmp_path):
    """sim_gif!'s loop (ext/WaterLilyPlotsExt.jl:41-52): frames at t0, t0 + step, ..., t0 + duration, each taken once the
    simulation has reached its time, the body drawn when asked for"""
    sim = circle_sim(steps=0)
    path = tmp_path / "gif.png"
    r = render.sim_gif(sim, path, duration=0.5, step=0.25, plotbody=True, clims=(-2.0, 2.0), ring=2)
    frames, _ = RR.decode(path.read_bytes())
    assert len(frames) == 3 and len(r.frames) == 3 and all(np.array_equal(a, b) for a, b in zip(frames, r.frames))
    assert 0.5 <= S.sim_time(sim) < 0.5 + sim.flow.dt[-2] * sim.U / sim.L + 1e-12   # the last frame's time was reached by the last step
    want, _ = ref_curl_image(sim, (-2.0, 2.0))
    assert np.array_equal(frames[2], want) and not np.array_equal(frames[0], frames[2])


def test_steady_record_allocates_nothing():
    sim = circle_sim(steps=1)
    r = render.Renderer(sim.flow, ring=2)
    L = _lib.lib()

    def allocs():
        n, by = C.c_int64(), C.c_int64()
        assert L.wl_prof_allocs(C.byref(n), C.byref(by)) == 0
        return n.value
    render.record(r, sim, "curl", clims=(-2.0, 2.0))
    n0 = allocs()
    for _ in range(6):
        render.record(r, sim, "curl", clims=(-2.0, 2.0))
    assert allocs() == n0
    fr = render.drain(r)
    assert len(fr) == 7 and all(np.array_equal(f, fr[0]) for f in fr)


def test_slabs():
    """2 ranks sharing the GPU (tests/render_worker.py), (33, 12, 12): gathered images against the undecomposed ones"""
    from test_multi_gpu import run_workers
    out = run_workers("render_worker.py", 2, timeout=300)
    print(out)
    for T in ("float32", "float64"):
        res = out[T]
        for key in ("axis1_max", "axis1_sum", "axis2_max", "axis0_absmax", "axis1_max_lambda2", "axis2_min_slice"):
            assert res[key], (T, key)
        assert res["rows"] == [6, 6]                           # the box is inside(): six planes of z each
        # a sum of nz doubles reordered: within nz 2^-53 sum|x| per pixel (the worker computes both from the data)
        assert res["axis2_sum_ok"] and 0 <= res["axis2_sum_err"], res
