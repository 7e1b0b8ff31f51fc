"""Render without a GPU: the numpy restatement tests/render_ref.py against closed forms, the shade arithmetic's edge cases, the
PNG / APNG writer of waterlily_amd.render decoded chunk by chunk, the colour maps, and the argument checks of the two entry
points (which refuse a bad call before they touch the device)."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as RR  # noqa: E402

from waterlily_amd import _lib, render  # noqa: E402

F64 = np.float64


# --------------------------------------------------------------------------- the reference against closed forms

def linear(n, g=(0.375, -0.25, 1.5), c0=2.0):
    x = np.stack(np.meshgrid(*[np.arange(m, dtype=F64) for m in n], indexing="ij"))
    return g[0] * x[0] + g[1] * x[1] + g[2] * x[2] + c0          # eighths: every value and partial sum below is exact


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_linear_field(axis):
    n = (70, 9, 7)
    g = (0.375, -0.25, 1.5)
    f = linear(n, g)
    lo, hi = (3, 1, 2), (69, 8, 6)
    v = RR.values(f, "scalar", 0, lo, hi)
    others = [d for d in range(3) if d != axis]
    end = {d: (hi[d] - 1 if g[d] > 0 else lo[d]) for d in range(3)}
    ia, ib = np.meshgrid(np.arange(lo[others[0]], hi[others[0]]), np.arange(lo[others[1]], hi[others[1]]), indexing="xy")
    base = g[others[0]] * ia + g[others[1]] * ib + 2.0
    assert np.array_equal(RR.project(v, axis, "max"), base + g[axis] * end[axis])                     # the box end
    assert np.array_equal(RR.project(v, axis, "min"), base + g[axis] * (lo[axis] + hi[axis] - 1 - end[axis]))
    mid = (lo[axis] + hi[axis] - 1) / 2.0
    assert np.array_equal(RR.project(v, axis, "mean"), base + g[axis] * mid)                          # the mid value
    assert np.array_equal(RR.project(v, axis, "sum"), (base + g[axis] * mid) * (hi[axis] - lo[axis]))
    assert RR.project(v, axis, "max").shape == (hi[others[1]] - lo[others[1]], hi[others[0]] - lo[others[0]])


def ray(vals, axis):
    """a box that is one ray along `axis`"""
    shape = [1, 1, 1]
    shape[axis] = len(vals)
    return np.asarray(vals, dtype=F64).reshape(shape)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_absmax_and_nan_rules(axis):
    nan = np.nan
    one = lambda vals, mode: RR.project(ray(vals, axis), axis, mode)[0, 0]
    assert one([-3, 2, 3], "absmax") == -3                        # the first one wins the tie
    assert one([3, 2, -3], "absmax") == 3
    assert one([1, -4, 2], "absmax") == -4
    assert one([nan, -1, nan, 2], "absmax") == 2
    assert one([nan, 1, 5, nan, 3], "max") == 5 and one([nan, 1, 5, nan, 3], "min") == 1
    for mode in ("max", "min", "absmax"):
        assert np.isnan(one([nan, nan, nan], mode))               # an all-NaN ray
        assert one([nan, 7, nan], mode) == 7
    assert np.isnan(one([1, nan, 2], "sum")) and np.isnan(one([1, nan, 2], "mean"))
    assert one([1, 2, 4], "sum") == 7 and one([1, 2, 6], "mean") == 3
    long = np.arange(1, 201, dtype=F64)                           # > 64 cells along the ray: three rounds per lane on axis 0
    assert one(long, "sum") == 20100 and one(long, "max") == 200 and one(-long, "absmax") == -200
    long[130] = nan
    assert np.isnan(one(long, "sum")) and one(long, "max") == 200 and one(long, "min") == 1


def test_axis0_order_is_lanes_then_tree():
    """a ray on which the order of the additions shows: the restated order differs from a left-to-right sum and equals the
    explicit lane / tree formula"""
    rng = np.random.default_rng(5)
    v = rng.standard_normal(150) * 10.0 ** rng.integers(-8, 8, 150)
    got = RR.project(ray(v, 0), 0, "sum")[0, 0]
    lanes = [0.0] * 64
    for l in range(64):
        for i in range(l, 150, 64):
            lanes[l] = lanes[l] + v[i]
    off = 32
    while off:
        for l in range(off):
            lanes[l] = lanes[l] + lanes[l + off]
        off //= 2
    assert got == lanes[0]
    seq = 0.0
    for x in v:
        seq = seq + x
    assert RR.project(ray(v, 2), 2, "sum")[0, 0] == seq and got != seq


def test_values_kinds():
    rng = np.random.default_rng(1)
    u = rng.standard_normal((8, 7, 6, 3)).astype(np.float32)
    lo, hi = (1, 2, 0), (7, 6, 5)
    assert np.array_equal(RR.values(u, "ucomp", 1, lo, hi), u[1:7, 2:6, 0:5, 1].astype(F64))
    c = RR.values(u, "centre", 2, lo, hi)
    assert np.array_equal(c, (u[1:7, 2:6, 0:5, 2].astype(F64) + u[1:7, 2:6, 1:6, 2].astype(F64)) / 2)
    p = rng.standard_normal((8, 7))
    assert RR.values(p, "scalar", 0, (1, 1), (7, 6)).shape == (6, 5, 1)
    img = [RR.project(RR.values(p, "scalar", 0, (1, 1), (7, 6)), 2, m) for m in RR.MODES]
    assert all(np.array_equal(i, p[1:7, 1:6].T) for i in img)     # 2-D: the image is the field in every mode


# --------------------------------------------------------------------------- shade

LUT = render.colormap("gray")


def test_shade_edges():
    nanc, maskc = (9, 8, 7, 6), (1, 2, 3, 4)
    img = np.array([[0.0, 1.0, 2.0, -5.0, np.nan, 0.999999, 1.0 + 1e-9, np.inf, -np.inf]])
    out = RR.shade(img, 0.0, 2.0, 0, LUT, nan_rgba=nanc)
    assert out.shape == (1, 9, 4)
    assert list(out[0, :, 0]) == [0, 128, 255, 0, 9, 127, 128, 255, 0]       # v == vmax -> 255, v < vmin -> 0
    assert tuple(out[0, 4]) == nanc and np.all(out[0, [0, 1, 2], 3] == 255)
    # levels = 10: the band centres floor((b + 0.5) * 25.6)
    centres = [int(np.floor((b + 0.5) * 256 / 10)) for b in range(10)]
    assert centres == [12, 38, 64, 89, 115, 140, 166, 192, 217, 243]
    v = np.array([[-1.0, 0.0, 0.0999, 0.1, 0.55, 0.9, 0.99999, 1.0, 3.0]])
    out = RR.shade(v, 0.0, 1.0, 10, LUT)
    assert list(out[0, :, 0]) == [12, 12, 12, 38, 140, 243, 243, 243, 243]
    out = RR.shade(v, 0.0, 1.0, 256, LUT)                                    # 256 bands: the table itself
    assert np.array_equal(out, RR.shade(v, 0.0, 1.0, 0, LUT))
    # the mask threshold is strict, and the mask wins over NaN
    img = np.array([[0.5, 0.5, np.nan], [0.5, 0.5, 0.5]])
    mask = np.array([[0.5, 0.49999, 0.0], [1.0, np.nan, 0.75]])
    out = RR.shade(img, 0.0, 1.0, 0, LUT, mask=mask, mask_lt=0.5, mask_rgba=maskc, nan_rgba=nanc)
    assert [tuple(x) for x in out[0]] == [(128, 128, 128, 255), maskc, maskc] and np.all(out[1, :, 0] == 128)
    # zoom and flip_y
    img = np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]) / 8
    z = RR.shade(img, 0.0, 1.0, 0, LUT, zoom=3, flip_y=True)
    assert z.shape == (9, 6, 4)
    small = RR.shade(img, 0.0, 1.0, 0, LUT)
    for oy in range(9):
        for ox in range(6):
            assert tuple(z[oy, ox]) == tuple(small[2 - oy // 3, ox // 3])


def test_colormaps():
    for name in ("RdBu", "gray"):
        t = render.colormap(name)
        assert t.shape == (256, 4) and t.dtype == np.uint8 and np.all(t[:, 3] == 255)
    t = render.colormap("RdBu").astype(int)
    assert tuple(t[0, :3]) == (103, 0, 31) and tuple(t[255, :3]) == (5, 48, 97)          # the end anchors
    lum = 0.299 * t[:, 0] + 0.587 * t[:, 1] + 0.114 * t[:, 2]
    top = int(np.argmax(lum))
    assert 120 <= top <= 135 and np.all(np.diff(lum[:top + 1]) >= -1.0) and np.all(np.diff(lum[top:]) <= 1.0)   # diverging about white
    assert np.all(t[:120, 0] > t[:120, 2]) and np.all(t[136:, 2] > t[136:, 0])        # red below the middle, blue above
    for k, anchor in enumerate(render._RDBU11):                                          # every anchor is met where k/10 falls on an entry
        if (k * 255) % 10 == 0:
            assert tuple(t[k * 255 // 10, :3]) == anchor
    g = render.colormap("gray")
    assert np.array_equal(g[:, 0], np.arange(256)) and np.array_equal(g[:, 0], g[:, 1]) and np.array_equal(g[:, 1], g[:, 2])
    own = np.zeros((256, 4), dtype=np.uint8)
    assert render.colormap(own) is not None
    with pytest.raises(ValueError):
        render.colormap(np.zeros((255, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        render.colormap("viridis")


# --------------------------------------------------------------------------- PNG / APNG

def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, (13, 7, 4), dtype=np.uint8)
    p = tmp_path / "one.png"
    render.write_png(p, a)
    data = p.read_bytes()
    ch = RR.chunks(data)                                                         # walks the chunks, checks every CRC
    assert [t for t, _ in ch] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (7, 13, 8, 6, 0, 0, 0)
    frames, _ = RR.decode(data)                                                  # inflates, undoes filter 0
    assert len(frames) == 1 and np.array_equal(frames[0], a)
    with pytest.raises(ValueError):
        render.write_png(p, a[:, :, :3])


def test_apng_structure(tmp_path):
    rng = np.random.default_rng(3)
    fr = [rng.integers(0, 256, (5, 9, 4), dtype=np.uint8) for _ in range(4)]
    p = tmp_path / "movie.png"
    render.write_apng(p, fr, fps=20)
    data = p.read_bytes()
    ch = RR.chunks(data)
    tags = [t for t, _ in ch]
    assert tags == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert struct.unpack(">II", ch[1][1]) == (4, 0)                               # num_frames, loop for ever
    seqs = [struct.unpack(">I", d[:4])[0] for t, d in ch if t in (b"fcTL", b"fdAT")]
    assert seqs == list(range(7))                                                # ascending over fcTL and fdAT together
    assert struct.unpack(">IIIIIHHBB", ch[2][1])[5:7] == (100, 2000)
    frames, _ = RR.decode(data)
    assert len(frames) == 4 and all(np.array_equal(a, b) for a, b in zip(frames, fr))
    render.write_apng(p, fr[:1])                                                 # one frame: a plain PNG
    assert RR.decode(p.read_bytes())[1] == [b"IHDR", b"IDAT", b"IEND"]
    with pytest.raises(ValueError):
        render.write_apng(p, [fr[0], fr[1][:4]])


# --------------------------------------------------------------------------- refusals before the device is touched

def grid(D=3, n=(8, 9, 10)):
    g = _lib.Grid()
    g.D = D
    n = tuple(n[:D]) + (1,) * (3 - D)
    g.n[:] = list(n)
    g.s[:] = [1, n[0], n[0] * n[1]]
    g.sc = n[0] * n[1] * n[2]
    return g


def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_project_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    g3, g2 = grid(3), grid(2)
    buf = (C.c_double * 4)()                                   # never reached
    f = C.cast(buf, C.c_void_p)
    OM, CURL = render.R_METRIC + 2, render.R_METRIC + 1

    def call(g=g3, fld=f, kind=0, ipar=0, axis=2, mode=0, lo=None, hi=None, img=f, ld=64, t=_lib.WL_F32):
        return L.wl_render_project(t, None if g is None else C.byref(g), fld, kind, ipar, None, None, axis, mode, lo, hi, img, ld)

    def refused(word, **kw):
        assert call(**kw) == _lib.WL_E_ARG, kw
        assert word in L.wl_last_error(), (kw, L.wl_last_error())

    refused(b"null", g=None)
    refused(b"null", fld=None)
    refused(b"null", img=None)
    refused(b"dtype", t=7)
    for kind in (-1, 3, 15, render.R_METRIC + 5, 99):
        refused(b"kind", kind=kind)
    refused(b"kind", kind=1, ipar=3)                           # UCOMP / CENTRE: the component must exist
    refused(b"kind", kind=2, ipar=-1)
    refused(b"kind", g=g2, kind=2, ipar=2)
    refused(b"kind", g=g2, kind=OM)                            # omega_mag needs D == 3
    refused(b"kind", kind=CURL, ipar=3)
    for mode in (-1, 5):
        refused(b"mode", mode=mode)
    for axis in (-1, 3):
        refused(b"axis", axis=axis)
    for axis in (0, 1):
        refused(b"axis", g=g2, axis=axis)                      # a 2-D grid is viewed along 2
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"only one", hi=i3(2, 2, 2))
    refused(b"box", lo=i3(-1, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(5, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(1, 1, 1), hi=i3(8, 4, 4))           # hi <= n - 1
    refused(b"box", lo=i3(1, 1, 1), hi=i3(4, 4, 10))
    refused(b"box", g=g2, lo=i3(1, 1, 0), hi=i3(4, 9, 0))
    refused(b"inside", kind=OM, lo=i3(0, 1, 1), hi=i3(4, 4, 4))      # a metric box outside inside()
    refused(b"inside", kind=OM, lo=i3(1, 1, 0), hi=i3(4, 4, 4))
    refused(b"ld", ld=5)                                       # default box: 6 wide along x
    refused(b"ld", axis=0, ld=6)                               # ... 7 wide along y when x is reduced
    refused(b"ld", lo=i3(1, 1, 1), hi=i3(4, 4, 4), ld=2)


def test_shade_refuses_bad_arguments_without_gpu():
    L = _lib.lib()
    buf = (C.c_double * 4)()
    p = C.cast(buf, C.c_void_p)
    c4 = (C.c_uint8 * 4)(0, 0, 0, 255)

    def call(img=p, ld=4, nx=4, ny=4, vmin=0.0, vmax=1.0, levels=0, lut=p, mask=None, ldm=0, mask_lt=0.5, mc=c4, nc=c4, zoom=1, out=p):
        return L.wl_render_shade(img, ld, nx, ny, vmin, vmax, levels, lut, mask, ldm, mask_lt, mc, nc, zoom, 0, out)

    def refused(word, **kw):
        assert call(**kw) == _lib.WL_E_ARG, kw
        assert word in L.wl_last_error(), (kw, L.wl_last_error())

    refused(b"null", img=None)
    refused(b"null", lut=None)
    refused(b"null", out=None)
    refused(b"vmin", vmin=1.0, vmax=1.0)
    refused(b"vmin", vmin=2.0, vmax=1.0)
    for bad in (np.nan, np.inf, -np.inf):
        refused(b"vmin", vmin=bad)
        refused(b"vmin", vmax=bad)
    refused(b"levels", levels=-1)
    refused(b"levels", levels=257)
    refused(b"zoom", zoom=0)
    refused(b"ld", ld=3)
    refused(b"ld", nx=-1)
    refused(b"mask", mask=p, ldm=3)
    refused(b"mask", mask=p, ldm=4, mc=None)
    refused(b"aligned", out=C.c_void_p(C.addressof(buf) + 1))
