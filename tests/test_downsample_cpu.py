"""Downsample without a GPU: the numpy restatement tests/downsample_ref.py against closed forms and the divergence identity of the
face means, the argument checks of wl_downsample / wl_downsample_extent (which refuse a bad call before they touch the
device), the slab arithmetic of wl_downsample_extent for 1, 2 and 4 ranks, and the frame of the writer's file."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import downsample_ref as DR  # noqa: E402

from waterlily_amd import _lib, downsample, render  # noqa: E402
from waterlily_amd.dist import Slab  # noqa: E402

F64 = np.float64
FACTORS = (1, 2, 4, 8, 16)


# --------------------------------------------------------------------------- the reference against closed forms

@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("f", FACTORS)
def test_constant_field(D, f):
    n = (2 * f, f, 3 * f)[:D] + (1,) * (3 - D)
    vals = np.full(n, 1.5, dtype=F64)
    for mode in DR.MODES:
        for face in (None, 0, 1, 2)[:D + 1]:
            got = DR.downsample(vals, f, mode, D, face=face)
            cnt = f ** (D - 1 if face is not None else D)
            want = 1.5 * cnt if mode == "sum" else 1.5
            assert got.shape == (2, 1, 3 if D == 3 else 1) and np.all(got == want), (mode, face)
    assert DR.downsample(vals, f, "mean", D, out=np.float32).dtype == np.float32


@pytest.mark.parametrize("f", FACTORS)
def test_linear_field_mean_is_the_block_centre(f):
    a = 0.37
    n = (4 * f, 2 * f, f)
    x = np.arange(5, 5 + n[0], dtype=F64)
    vals = np.broadcast_to((a * x)[:, None, None], n).copy()
    got = DR.downsample(vals, f, "mean", 3)
    centre = 5 + np.arange(4) * f + (f - 1) / 2
    # f^3 terms of magnitude <= a max|x|: a sum within f^3 2^-53 sum|x| of the exact one, and the mean scales that by f^-3
    bound = f ** 3 * 2.0 ** -53 * a * x.max() + 2.0 ** -52 * a * x.max()
    assert np.all(np.abs(got - (a * centre)[:, None, None]) <= bound)
    assert np.array_equal(DR.downsample(vals, f, "sample", 3)[:, 0, 0], a * x[::f])
    assert np.array_equal(DR.downsample(vals, f, "max", 3)[:, 0, 0], a * x[f - 1::f])
    assert np.array_equal(DR.downsample(vals, f, "min", 3)[:, 0, 0], a * x[::f])


def test_order_is_column_walk_then_lane_tree():
    """a block on which the order of the additions shows: the restated order equals the explicit loops of the contract"""
    rng = np.random.default_rng(5)
    f = 4
    v = rng.standard_normal((f, f, f)) * 10.0 ** rng.integers(-8, 8, (f, f, f))
    lanes = [0.0] * f
    for a in range(f):
        for c in range(f):
            for b in range(f):
                lanes[a] = lanes[a] + v[a, b, c]
    lanes[0] = lanes[0] + lanes[2]
    lanes[1] = lanes[1] + lanes[3]
    lanes[0] = lanes[0] + lanes[1]
    assert DR.downsample(v, f, "sum", 3)[0, 0, 0] == lanes[0]
    assert DR.downsample(v, f, "mean", 3)[0, 0, 0] == lanes[0] * (1.0 / 64)
    seq = 0.0
    for x in v.reshape(-1):
        seq = seq + x
    assert lanes[0] != seq
    # faces: the low face of the component alone
    assert DR.downsample(v, f, "sum", 3, face=0)[0, 0, 0] == sum_in_order([v[0, b, c] for c in range(f) for b in range(f)])
    y = [sum_in_order([v[a, 0, c] for c in range(f)]) for a in range(f)]
    assert DR.downsample(v, f, "sum", 3, face=1)[0, 0, 0] == (y[0] + y[2]) + (y[1] + y[3])


def sum_in_order(xs):
    s = 0.0
    for x in xs:
        s = s + x
    return s


def test_nan_and_tie_rules():
    nan = np.nan
    blk = lambda xs: np.asarray(xs, dtype=F64).reshape(2, 2, 1)                 # [a, b]: a 2-D block of f = 2
    one = lambda xs, mode: DR.downsample(blk(xs), 2, mode, 2)[0, 0, 0]
    assert one([1, nan, 3, 2], "max") == 3 and one([1, nan, 3, 2], "min") == 1 and one([1, nan, -3, 2], "absmax") == -3
    assert np.isnan(one([1, nan, 3, 2], "mean")) and np.isnan(one([1, nan, 3, 2], "sum"))
    for mode in ("max", "min", "absmax"):
        assert np.isnan(one([nan] * 4, mode))
    assert one([-3, 2, 3, 1], "absmax") == -3 and one([3, 2, -3, 1], "absmax") == 3     # the first of two equal candidates stays
    assert one([nan, 2, 3, 1], "sample") != one([nan, 2, 3, 1], "sample")               # the first cell, whatever it holds
    assert one([5, 2, 3, 1], "sample") == 5


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("f", [2, 4])
def test_face_mean_divergence_identity(D, f):
    rng = np.random.default_rng(11)
    ncell = (3, 2, 2)[:D]
    Ng = tuple(f * (n + 1) + 2 for n in ncell)                                   # room for one more coarse layer on the high side
    u = rng.standard_normal(Ng + (D,))
    lo = (1,) * D
    hi = tuple(1 + f * n for n in ncell)
    hiv = tuple(h + f for h in hi)
    U = np.stack([DR.downsample(DR.values(u, "face", i, lo, hiv), f, "mean", D, face=i) for i in range(D)], axis=-1)
    U = U[:, :, 0] if D == 2 else U
    div = np.zeros(tuple(h - l for l, h in zip(lo, hi)))
    box = tuple(slice(l, h) for l, h in zip(lo, hi))
    for i in range(D):
        up = tuple(slice(l + (d == i), h + (d == i)) for d, (l, h) in enumerate(zip(lo, hi)))
        div += u[up + (i,)] - u[box + (i,)]
    want = DR.block_sum(div, f, D)[0] * float(f) ** (1 - D)
    got = DR.coarse_div(U)
    bound = DR.div_bound(u, lo, hi, f)
    assert got.shape == want.shape == ncell and np.all(np.abs(got - want) <= bound)
    assert np.abs(want).min() > 100 * bound.max()                                # the identity is not met by smallness


# --------------------------------------------------------------------------- refusals before the device is touched

def grid(D=3, n=(10, 11, 14)):
    g = _lib.Grid()
    g.D = D
    n = tuple(n[:D]) + (1,) * (3 - D)
    g.n[:] = list(n)
    g.s[:] = [1, n[0], n[0] * n[1]]
    g.sc = n[0] * n[1] * n[2]
    return g


def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_downsample_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    g3, g2 = grid(3), grid(2)
    buf = (C.c_double * 4)()                                   # never reached
    f = C.cast(buf, C.c_void_p)
    OM, CURL, FACE = render.R_METRIC + 2, render.R_METRIC + 1, downsample.R_FACE

    def call(g=g3, fld=f, kind=0, ipar=0, mode=4, factor=1, lo=None, hi=None, t_out=_lib.WL_F32, out=f, ntuple=1, c=0, t=_lib.WL_F32):
        return L.wl_downsample(t, None if g is None else C.byref(g), fld, kind, ipar, None, None, mode, factor, lo, hi, t_out, out, ntuple, c)

    def refused(word, **kw):
        assert call(**kw) == _lib.WL_E_ARG, kw
        assert word in L.wl_last_error(), (kw, L.wl_last_error())

    refused(b"null", g=None)
    refused(b"null", fld=None)
    refused(b"null", out=None)
    refused(b"dtype t", t=7)
    refused(b"dtype t_out", t_out=2)
    for kind in (-1, 4, 15, render.R_METRIC + 5, 99):
        refused(b"kind", kind=kind)
    refused(b"kind", kind=1, ipar=3)                           # UCOMP / CENTRE: the component must exist
    refused(b"kind", kind=2, ipar=-1)
    refused(b"kind", g=g2, kind=2, ipar=2)
    refused(b"kind", g=g2, kind=OM)                            # omega_mag needs D == 3
    refused(b"kind", kind=CURL, ipar=3)
    refused(b"WL_R_FACE", kind=FACE, ipar=3)                   # a face mean needs a component of a vector field
    refused(b"WL_R_FACE", kind=FACE, ipar=-1)
    refused(b"WL_R_FACE", g=g2, kind=FACE, ipar=2)
    for mode in (-1, 6):
        refused(b"mode", mode=mode)
    for factor in (0, 3, 5, 32, -2):
        refused(b"factor", factor=factor)
    refused(b"multiples of factor", factor=2, lo=i3(1, 1, 1), hi=i3(4, 5, 5))
    refused(b"multiples of factor", factor=4)                  # inside() is 8 x 9 x 12
    refused(b"multiples of factor", g=g2, factor=2, lo=i3(1, 1, 0), hi=i3(5, 4, 0))
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"only one", hi=i3(2, 2, 2))
    refused(b"box", lo=i3(-1, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(5, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(4, 1, 1), hi=i3(4, 4, 4))           # an empty extent
    refused(b"box", lo=i3(1, 1, 1), hi=i3(10, 4, 4))          # hi <= n - 1
    refused(b"box", lo=i3(1, 1, 1), hi=i3(4, 4, 14))
    refused(b"inside", kind=OM, lo=i3(0, 1, 1), hi=i3(4, 4, 4))      # a metric box outside inside()
    refused(b"inside", kind=OM, lo=i3(1, 1, 0), hi=i3(4, 4, 4))
    for ntuple in (0, 10, -1):
        refused(b"ntuple", ntuple=ntuple)
    refused(b"bad c", ntuple=3, c=3)
    refused(b"bad c", ntuple=3, c=-1)
    refused(b"bad c", c=1)
    assert L.wl_render_project(_lib.WL_F32, C.byref(g3), f, 0, 0, None, None, 2, 5, None, None, f, 64) == _lib.WL_E_ARG   # SAMPLE is not Render's
    assert L.wl_render_project(_lib.WL_F32, C.byref(g3), f, FACE, 0, None, None, 2, 0, None, None, f, 64) == _lib.WL_E_ARG


def test_extent_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    g3 = grid(3)
    nc, k0 = (C.c_int32 * 3)(), C.c_int32()

    def refused(word, g=g3, factor=1, lo=None, hi=None, out=nc, k=C.byref(k0)):
        assert L.wl_downsample_extent(None if g is None else C.byref(g), factor, lo, hi, out, k) == _lib.WL_E_ARG
        assert word in L.wl_last_error(), L.wl_last_error()

    refused(b"null", g=None)
    refused(b"null", out=None)
    refused(b"null", k=None)
    refused(b"factor", factor=3)
    refused(b"multiples of factor", factor=8)
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"box", lo=i3(1, 1, 1), hi=i3(4, 4, 14))
    assert downsample.extent(g3, 1, (1, 1, 1), (9, 10, 13)) == ((8, 9, 12), 0)
    assert downsample.extent(g3, 4, (1, 2, 1), (9, 10, 13)) == ((2, 2, 3), 0)
    assert downsample.extent(grid(2), 2, (1, 1), (9, 9)) == ((4, 4, 1), 0)


# --------------------------------------------------------------------------- slabs: wl_downsample_extent's arithmetic

def slab_grid(sl, nx=34, ny=14):
    g = grid(3, (nx, ny, sl.n2l))
    g.nzg, g.kz0, g.own_lo, g.own_hi, g.zring = sl.nzg, sl.kz0, sl.own_lo, sl.own_hi, int(sl.ring)
    return g


@pytest.mark.parametrize("size", [1, 2, 4])
def test_extent_over_slabs(size):
    nz = 16
    for f, lo2, hi2 in ((1, 1, 17), (2, 1, 17), (4, 1, 17), (1, 0, 17), (1, 3, 16), (4, 5, 13)):
        got = [downsample.extent(slab_grid(Slab(r, size, nz)), f, (1, 1, lo2), (33, 13, hi2)) for r in range(size)]
        # every coarse plane of the box belongs to exactly one rank, in rank order
        planes = []
        for (nc, k0) in got:
            assert nc[:2] == (32 // f, 12 // f)
            planes += list(range(k0, k0 + nc[2])) if nc[2] else []
        assert planes == list(range((hi2 - lo2) // f)), (size, f, lo2, hi2, got)
    # by hand: 4 ranks own the global planes 0..4, 5..8, 9..12, 13..17; the box 5..13 at f = 4 is ranks 1 and 2's
    if size == 4:
        got = [downsample.extent(slab_grid(Slab(r, 4, nz)), 4, (1, 1, 5), (33, 13, 13)) for r in range(4)]
        assert [(nc[2], k0) for nc, k0 in got] == [(0, 0), (1, 0), (1, 1), (0, 2)]
    # a ring: nobody owns the ghost planes, the first rank takes the bottom one when the box asks for it
    got = [downsample.extent(slab_grid(Slab(r, size, nz, ring=True)), 1, (1, 1, 0), (33, 13, 17)) for r in range(size)]
    assert sum(nc[2] for nc, _ in got) == 17 and got[0][1] == 0


def test_extent_refuses_a_misaligned_slab_boundary():
    L = _lib.lib()
    nz = 16                                                    # 2 ranks: the planes 0..8 and 9..17, the boundary at 9
    for r in range(2):
        g = slab_grid(Slab(r, 2, nz))
        nc, k0 = (C.c_int32 * 3)(), C.c_int32()
        assert L.wl_downsample_extent(C.byref(g), 4, i3(1, 1, 3), i3(33, 13, 15), nc, C.byref(k0)) == _lib.WL_E_ARG      # (9 - 3) % 4 != 0
        assert b"lo_2 + m*factor" in L.wl_last_error()
        g16 = slab_grid(Slab(r, 2, nz), ny=18)
        assert L.wl_downsample_extent(C.byref(g16), 16, None, None, nc, C.byref(k0)) == _lib.WL_E_ARG                    # one block across both
        assert b"lo_2 + m*factor" in L.wl_last_error()
        buf = (C.c_double * 4)()
        p = C.cast(buf, C.c_void_p)
        assert L.wl_downsample(_lib.WL_F32, C.byref(g), p, 0, 0, None, None, 4, 4, i3(1, 1, 3), i3(33, 13, 15), _lib.WL_F32, p, 1, 0) == _lib.WL_E_ARG
        assert b"lo_2 + m*factor" in L.wl_last_error()
        assert downsample.extent(g, 4, (1, 1, 5), (33, 13, 13)) == ((8, 3, 1), r)      # aligned: (9 - 5) % 4 == 0
    # the box ends on the boundary: nothing is cut
    assert downsample.extent(slab_grid(Slab(0, 2, nz)), 4, (1, 1, 1), (33, 13, 9)) == ((8, 3, 2), 0)
    assert downsample.extent(slab_grid(Slab(1, 2, nz)), 4, (1, 1, 1), (33, 13, 9))[0][2] == 0


# --------------------------------------------------------------------------- the file's frame

def test_trim_records_what_is_left():
    assert downsample.trim((34, 34, 34), 4) == ((1, 1, 1), (33, 33, 33))
    assert downsample.trim((74, 10, 10), 4, ((3, 2, 1), (70, 9, 8))) == ((3, 2, 1), (67, 6, 5))
    assert downsample.trim((42, 26), 8) == ((1, 1), (41, 25))
    with pytest.raises(ValueError):
        downsample.trim((10, 10, 10), 16)                      # nothing is left
    with pytest.raises(ValueError):
        downsample.trim((10, 10, 10), 2, ((1, 1), (9, 9)))


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_header_origin_and_spacing(f):
    lo = (3, 2, 1)
    origin, spacing = downsample.frame(lo, f)
    assert origin == tuple(l + 1 + (f - 1) / 2 for l in lo) and spacing == (float(f),) * 3
    xml = downsample.header((5, 4, 3), origin, spacing, [("Pressure", "Float32", 1, 0), ("Velocity", "Float32", 3, 8 + 5 * 4 * 3 * 4)]).decode()
    assert 'WholeExtent="0 4 0 3 0 2"' in xml and 'Piece Extent="0 4 0 3 0 2"' in xml
    got_o = tuple(float(v) for v in re.search(r'Origin="([^"]*)"', xml).group(1).split())
    got_s = tuple(float(v) for v in re.search(r'Spacing="([^"]*)"', xml).group(1).split())
    assert got_o == origin and got_s == spacing
    # coarse sample I is the mean position of its fine cells, which vtk.write's file puts at J + 1
    for d in range(3):
        for I in range(3):
            fine = np.arange(lo[d] + I * f, lo[d] + (I + 1) * f) + 1.0
            assert got_o[d] + I * got_s[d] == fine.mean()
    assert xml.endswith('<AppendedData encoding="raw">\n   _')
    o2, s2 = downsample.frame((1, 1), 4)                       # 2-D: the one plane of vtk.write's file sits at z = 1
    assert o2 == (3.5, 3.5, 1.0) and s2 == (4.0, 4.0, 1.0)


def test_file_round_trip_through_read_vti(tmp_path):
    """a file laid out by the writer's header function, read back by downsample.read (built on vtk.read_vti)"""
    import struct
    rng = np.random.default_rng(3)
    nc = (5, 4, 3)
    p = rng.standard_normal(nc[::-1]).astype(np.float32)                          # [K, J, I]: x fast
    v = rng.standard_normal(nc[::-1] + (3,)).astype(np.float32)
    origin, spacing = downsample.frame((3, 2, 1), 4)
    path = tmp_path / "c.vti"
    with open(path, "wb") as o:
        o.write(downsample.header(nc, origin, spacing, [("Pressure", "Float32", 1, 0), ("Velocity", "Float32", 3, 8 + p.nbytes)]))
        for a in (p, v):
            o.write(struct.pack("<Q", a.nbytes))
            o.write(a.tobytes())
        o.write(b"\n  </AppendedData>\n</VTKFile>\n")
    arrays, o_, s_ = downsample.read(str(path))
    assert o_ == origin and s_ == spacing
    assert np.array_equal(arrays["Pressure"], p.transpose(2, 1, 0)) and np.array_equal(arrays["Velocity"], v.transpose(3, 2, 1, 0))
