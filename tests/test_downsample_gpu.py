"""Downsample on the GPU (waterlily_amd.downsample: wl_downsample) against the numpy restatement tests/downsample_ref.py, bit for
bit (uint64 / uint32 views).

Interior shapes: (72, 8, 8) at f = 2, 4, 8 -- a row of 64 + 8 fine cells: a second, short wavefront; (80, 16, 16) at f = 16 -- one
block across y and z; the 2-D (40, 24) and (72, 8) at f = 2, 4, 8.  Float32 and Float64, padded and dense; fields are seeded
standard_normal, ghost cells included.  Every shape runs on inside() and on an interior box that starts at (3, 2, 1) and is
trimmed to multiples of the factor, so its blocks are not aligned to 64-lane boundaries.  Where a direction is too short to
hold one block from that start ((72, 8, 8) at f = 8: seven cells are left along y from 2), that direction starts at 1.

Why equality: the modes use additions, comparisons and one multiplication by a power of two in an order the contract fixes,
and the library is built without contraction; the metric kinds call the device function wl_metric's kernel calls, so the
yardstick for them is the host copy of what wl_metric stored for the same u (the xref tests hold wl_metric itself).
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import downsample_ref as DR  # noqa: E402

from waterlily_amd import _lib, downsample, sim as S  # noqa: E402
from waterlily_amd.body import AutoBody, norm2  # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [((72, 8, 8), (2, 4, 8)), ((80, 16, 16), (16,)), ((40, 24), (2, 4, 8)), ((72, 8), (2, 4, 8))]
CASES = [(sh, fs, T, pad) for sh, fs in SHAPES for T in (F32, F64) for pad in (True, False)]
IDS = [f"{'x'.join(map(str, sh))}-{np.dtype(T).name}-{'padded' if pad else 'dense'}" for sh, fs, T, pad in CASES]


@functools.lru_cache(maxsize=None)
def fields(shape, T):
    """(p, u) host arrays with ghosts, seeded (read-only)"""
    Ng = tuple(n + 2 for n in shape)
    rng = np.random.default_rng(17)
    p = np.asfortranarray(rng.standard_normal(Ng).astype(T))
    u = np.asfortranarray(rng.standard_normal(Ng + (len(shape),)).astype(T))
    return p, u


def make(shape, T, padded):
    flow = S.Flow(shape, (0.0,) * len(shape), T=T, padded=padded)
    p, u = fields(shape, T)
    S.upload(flow.p, p)
    S.upload(flow.u, u)
    return flow, p, u


def host(x):
    return x.cpu().numpy().copy()


def same_bits(a, b):
    v = np.uint64 if a.dtype == F64 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(v), np.ascontiguousarray(b).view(v))


def boxes(Ng, f):
    """the default box (inside) and the interior one"""
    start = [3, 2, 1][:len(Ng)]
    lo = tuple(s if n - 1 - s >= f else 1 for s, n in zip(start, Ng))
    return [None, (lo, tuple(n - 1 for n in Ng))]


def ref(vals, f, mode, D, T, face=None):
    r = DR.downsample(vals, f, mode, D, face=face, out=T)
    return r[:, :, 0] if D == 2 else r


@pytest.mark.parametrize("shape,factors,T,padded", CASES, ids=IDS)
def test_fields_every_mode(shape, factors, T, padded):
    flow, p, u = make(shape, T, padded)
    D, Ng = len(shape), p.shape
    n = 0
    for f in factors:
        for box in boxes(Ng, f):
            d = downsample.Downsampler(flow, f, box)
            lo, hi = d.box
            assert all((h - l) % f == 0 and h - l > 0 for l, h in zip(lo, hi)) and (box is None or lo == box[0])
            for mode in DR.MODES:
                got = host(downsample.volume(d, flow.p, "scalar", mode=mode))
                assert same_bits(got, ref(DR.values(p, "scalar", 0, lo, hi), f, mode, D, T)), ("scalar", f, box, mode)
                n += 1
                for c in range(D):
                    for kind in ("ucomp", "centre", "face"):
                        got = host(downsample.volume(d, flow.u, kind, mode=mode, i=c))
                        want = ref(DR.values(u, kind, c, lo, hi), f, mode, D, T, face=c if kind == "face" else None)
                        assert same_bits(got, want), (kind, c, f, box, mode, np.abs(got - want).max())
                        n += 1
    assert n == len(factors) * 2 * 6 * (1 + 3 * D)


@pytest.mark.parametrize("shape,factors,T,padded", [c for c in CASES if len(c[0]) == 3], ids=[i for c, i in zip(CASES, IDS) if len(c[0]) == 3])
def test_metric_kinds_equal_wl_metric(shape, factors, T, padded):
    flow, p, u = make(shape, T, padded)
    Ng = p.shape
    scratch = S.like(flow.p)
    for kind in ("omega_mag", "lambda2"):
        scratch.zero_()
        h = S.to_host(S.metric(scratch, kind, flow.u))         # what the existing wl_metric stores
        assert np.isfinite(h).all() and h[1:-1, 1:-1, 1:-1].std() > 0
        for f in factors:
            for box in boxes(Ng, f):
                d = downsample.Downsampler(flow, f, box)
                lo, hi = d.box
                vals = DR.values(h, "scalar", 0, lo, hi)
                for mode in ("mean", "min", "max"):
                    got = host(downsample.volume(d, flow.u, kind, mode=mode))
                    assert same_bits(got, ref(vals, f, mode, 3, T)), (kind, f, box, mode)


@pytest.mark.parametrize("T,out", [(F32, F64), (F64, F32)])
def test_output_dtype_is_rounded_once(T, out):
    shape, f = (72, 8, 8), 4
    flow, p, u = make(shape, T, True)
    d = downsample.Downsampler(flow, f, out=out)
    lo, hi = d.box
    for kind, c, mode in (("scalar", 0, "mean"), ("centre", 1, "sum"), ("face", 2, "mean"), ("ucomp", 0, "sample")):
        fld, hf = (flow.p, p) if kind == "scalar" else (flow.u, u)
        got = host(downsample.volume(d, fld, kind, mode=mode, i=c))
        assert got.dtype == out and same_bits(got, ref(DR.values(hf, kind, c, lo, hi), f, mode, 3, out, face=c if kind == "face" else None))


def test_2d_volume_of_factor_1_is_the_field():
    flow, p, u = make((40, 24), F64, True)
    d = downsample.Downsampler(flow, 1)
    for mode in DR.MODES:
        assert same_bits(host(downsample.volume(d, flow.p, "scalar", mode=mode)), p[1:-1, 1:-1])


def test_python_refuses_what_the_kinds_do_not_take():
    flow, p, u = make((40, 24), F64, True)
    d = downsample.Downsampler(flow, 2)
    for kind in ("face", "centre", "ucomp"):
        with pytest.raises(ValueError):
            downsample.volume(d, flow.p, kind)                  # a component of a scalar field
    with pytest.raises(ValueError):
        downsample.volume(d, flow.u, "scalar")
    with pytest.raises(_lib.WlError):
        downsample.volume(d, flow.u, "face", i=2)              # a 2-D field has no third component
    with pytest.raises(ValueError):
        downsample.Downsampler(flow, 3)
    with pytest.raises(ValueError):
        downsample.Downsampler(flow, 16, ((1, 1), (41, 12)))   # nothing is left of 11 cells


def test_nan_rules():
    shape, T, f = (72, 8, 8), F64, 4
    flow, p, u = make(shape, T, True)
    d = downsample.Downsampler(flow, f)
    lo, hi = d.box
    pn = p.copy()
    pn[1 + 66, 1 + 5, 1 + 2] = np.nan                          # one NaN in block (16, 1, 0): the short second wavefront
    pn[1 + 8:1 + 12, 1 + 4:1 + 8, 1 + 4:1 + 8] = np.nan        # block (2, 1, 1) holds nothing but NaN
    pn[1 + 20, 1 + 1, 1 + 1], pn[1 + 22, 1 + 0, 1 + 0] = -7.0, 7.0      # block (5, 0, 0): +7 comes first (y, z = 0), -7 is in a lower lane
    pn[1 + 24, 1 + 0, 1 + 0], pn[1 + 24, 1 + 3, 1 + 3] = -7.0, 7.0      # block (6, 0, 0): one lane, -7 first
    S.upload(flow.p, pn)
    vals = DR.values(pn, "scalar", 0, lo, hi)
    got = {}
    for mode in DR.MODES:
        got[mode] = host(downsample.volume(d, flow.p, "scalar", mode=mode))
        want = ref(vals, f, mode, 3, T)
        assert got[mode].shape == want.shape and np.all((got[mode] == want) | (np.isnan(got[mode]) & np.isnan(want))), mode
    one, allnan = (16, 1, 0), (2, 1, 1)
    blk = pn[1 + 64:1 + 68, 1 + 4:1 + 8, 1:1 + 4]
    for mode, fn in (("max", np.nanmax), ("min", np.nanmin)):
        assert got[mode][one] == fn(blk) and np.isnan(got[mode][allnan]) and np.isnan(got[mode]).sum() == 1     # skipped; NaN only there
    assert abs(got["absmax"][one]) == np.nanmax(np.abs(blk)) and np.isnan(got["absmax"][allnan])
    for mode in ("mean", "sum"):
        assert np.isnan(got[mode][one]) and np.isnan(got[mode][allnan]) and np.isnan(got[mode]).sum() == 2      # propagates, and only there
    # equal candidates: the lanes' own accumulators are combined with the LOWER lane first, so lane 0's -7 stays in block 5 ...
    assert got["absmax"][5, 0, 0] == -7.0 and got["absmax"][6, 0, 0] == -7.0 and got["max"][5, 0, 0] == 7.0


def test_interleaved_output_touches_only_its_component():
    shape, T, f = (72, 8, 8), F32, 2
    flow, p, u = make(shape, T, True)
    d = downsample.Downsampler(flow, f)
    nc = d.nc
    ncell = nc[0] * nc[1] * nc[2]
    sentinel = -12345.0
    buf = torch.full((3 * ncell + 64,), sentinel, dtype=torch.float32, device=flow.device)

    def put(c):
        downsample._call(d, flow.u, downsample._KIND["centre"], downsample._MODE["mean"], c, None, None, d.box, buf.data_ptr(), 3, c)
        return host(buf)
    want = [host(downsample.volume(d, flow.u, "centre", mode="mean", i=c)).transpose(2, 1, 0).reshape(-1) for c in range(3)]
    h = put(1)
    assert np.all(h[3 * ncell:] == sentinel)                   # nothing past the last tuple
    t = h[:3 * ncell].reshape(ncell, 3)
    assert np.all(t[:, 0] == sentinel) and np.all(t[:, 2] == sentinel) and same_bits(t[:, 1].copy(), want[1])
    put(0)
    t = put(2)[:3 * ncell].reshape(ncell, 3)
    for c in range(3):
        assert same_bits(t[:, c].copy(), want[c]), c
    assert np.all(host(buf)[3 * ncell:] == sentinel)


@pytest.mark.parametrize("T", [F32, F64])
def test_factor_1_lambda2_is_the_crop_of_wl_metric(T):
    shape = (72, 8, 8)
    flow, p, u = make(shape, T, True)
    h = S.to_host(S.metric(S.like(flow.p), "lambda2", flow.u))
    for box in (None, ((3, 2, 1), (70, 8, 9))):
        d = downsample.Downsampler(flow, 1, box)
        lo, hi = d.box
        crop = h[tuple(slice(l, hh) for l, hh in zip(lo, hi))]
        for mode in ("mean", "min", "sample"):
            assert same_bits(host(downsample.volume(d, flow.u, "lambda2", mode=mode)), crop), (box, mode)


# --------------------------------------------------------------------------- end to end: a 32^3 sphere

M = 32


@functools.lru_cache(maxsize=None)
def sphere_sim():
    R, c = M / 8, M / 2 - 1
    sim = S.Simulation((M, M, M), (1.0, 0.0, 0.0), 2 * R, body=AutoBody(lambda x, t: norm2(x - c) - R), nu=2 * R / 3700, T=F64)
    for _ in range(5):
        S.sim_step(sim, remeasure=False)
    return sim


@pytest.mark.parametrize("f", [2, 4])
@pytest.mark.parametrize("box", [None, ((1, 1, 1), (1 + M - 8, 1 + M - 8, 1 + M - 8))], ids=["inside", "fits"])
def test_velocity_divergence_identity(f, box):
    sim = sphere_sim()
    flow = sim.flow
    d = downsample.Downsampler(flow, f, box)
    lo, hi = d.box
    fits = box is not None
    assert d.vbox == (lo, tuple(h + f for h in hi) if fits else hi)            # one more coarse layer where it fits
    U = host(downsample.velocity(d, flow.u))
    assert U.shape == tuple(n + (1 if fits else 0) for n in d.nc) + (3,)
    hu = S.to_host(flow.u)
    for c in range(3):                                                           # the face means themselves, by bits
        assert same_bits(U[..., c].copy(), DR.downsample(DR.values(hu, "face", c, *d.vbox), f, "mean", 3, face=c))
    z = S.like(flow.p)
    S.divergence(z, flow.u)
    fine = S.to_host(z)[tuple(slice(l, h) for l, h in zip(lo, hi))]
    cells = tuple(slice(0, n) for n in DR.coarse_div(U).shape)                   # the coarse cells that have their high faces
    want = (DR.block_sum(fine, f, 3)[0] * float(f) ** -2)[cells]
    got = DR.coarse_div(U)
    bound = DR.div_bound(hu, lo, hi, f)[cells]
    assert got.shape == (tuple(d.nc) if fits else tuple(n - 1 for n in d.nc))
    err = np.abs(got - want)
    print(f"f={f} box={box}: max err {err.max():.3e}, min bound {bound.min():.3e}, max |div| {np.abs(want).max():.3e}")
    assert np.all(err <= bound)


def test_writer_end_to_end(tmp_path):
    sim = sphere_sim()
    flow = sim.flow
    L = _lib.lib()

    def allocs():
        n, by = C.c_int64(), C.c_int64()
        assert L.wl_prof_allocs(C.byref(n), C.byref(by)) == 0
        return n.value
    f, box = 4, ((3, 2, 1), (31, 33, 30))                                        # trimmed to (31, 30, 29)
    attrib = dict(downsample.default_attrib(), Lambda2=(lambda s: s.flow.u, "lambda2", "min"))
    w = downsample.DownsampleWriter(str(tmp_path / "wake"), factor=f, box=box, attrib=attrib, dir=str(tmp_path / "vtk"), T=F32, ring=2)
    downsample.write(w, sim)
    n0 = allocs()
    for _ in range(2):
        downsample.write(w, sim)
    assert allocs() == n0                                                        # steady writes allocate nothing
    downsample.close(w)
    d = downsample.Downsampler(flow, f, box, out=F32)
    assert d.box == ((3, 2, 1), (31, 30, 29)) and w.d.box == d.box and d.nc == (7, 7, 7)
    want = {"Pressure": host(downsample.volume(d, flow.p, "scalar", mode="mean")), "Lambda2": host(downsample.volume(d, flow.u, "lambda2", mode="min"))}
    vel = [host(downsample.volume(d, flow.u, "centre", mode="mean", i=c)) for c in range(3)]
    assert np.abs(want["Lambda2"]).max() > 0
    from waterlily_amd import vtk
    items = vtk.read_pvd(str(tmp_path / "wake.pvd"))
    assert len(items) == 3 and w.stats["snapshots"] == 3 and w.stats["skipped"] == 0
    for t, path in items:
        arrays, origin, spacing = downsample.read(path)
        assert origin == (3 + 1 + 1.5, 2 + 1 + 1.5, 1 + 1 + 1.5) and spacing == (4.0, 4.0, 4.0)
        assert set(arrays) == {"Velocity", "Pressure", "Lambda2"}
        for name in ("Pressure", "Lambda2"):
            assert same_bits(np.asarray(arrays[name]), want[name]), name
        for c in range(3):
            assert same_bits(np.asarray(arrays["Velocity"][c]), vel[c]), c
    assert w.stats["bytes"] == 3 * sum(-(-7 ** 3 * 4 * k // 256) * 256 for k in (3, 1, 1))


def test_writer_2d_pads_the_vector_with_a_zero_component(tmp_path):
    body = AutoBody(lambda x, t: norm2(x - 16.0) - 4.0)
    sim = S.Simulation((64, 32), (1.0, 0.0), 8.0, nu=8.0 / 250, body=body, T=F64)
    S.sim_step(sim)
    w = downsample.DownsampleWriter(str(tmp_path / "c"), factor=8, dir=str(tmp_path / "vtk"), T=F64,
                                    attrib={"Velocity": (lambda s: s.flow.u, "face", "mean"), "Speed": (lambda s: s.flow.u, "ke", "max")})
    for _ in range(2):                                                           # the second one reuses a slot the first left its zeros in
        downsample.write(w, sim)
    downsample.close(w)
    d = downsample.Downsampler(sim.flow, 8)
    vel = [host(downsample.volume(d, sim.flow.u, "face", mode="mean", i=c)) for c in range(2)]
    ke = host(downsample.volume(d, sim.flow.u, "ke", mode="max", par=(0.0, 0.0)))
    arrays, origin, spacing = downsample.read(w.entries[-1][1])
    assert origin == (1 + 1 + 3.5, 1 + 1 + 3.5, 1.0) and spacing == (8.0, 8.0, 1.0)
    v = np.asarray(arrays["Velocity"])
    assert v.shape == (3, 8, 4, 1) and not v[2].any() and np.abs(v[0]).max() > 0
    assert same_bits(v[0][:, :, 0].copy(), vel[0]) and same_bits(v[1][:, :, 0].copy(), vel[1])
    assert same_bits(np.asarray(arrays["Speed"])[:, :, 0].copy(), ke)


def test_slabs():
    """2 ranks sharing the GPU (tests/downsample_worker.py), (32, 12, 16) at f = 2 and 4: gathered volumes against the undecomposed ones"""
    from test_multi_gpu import run_workers
    out = run_workers("downsample_worker.py", 2, timeout=300)
    print(out)
    for T in ("float32", "float64"):
        for f in ("2", "4"):
            res = out[T][f]
            for key in ("p_mean", "u_face", "lambda2_min", "velocity", "file"):
                assert res[key], (T, f, key)
            assert res["planes"] == [8 // int(f), 8 // int(f)]
