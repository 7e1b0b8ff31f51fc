"""Volume without a GPU: the argument checks of wl_scene_volume and wl_scene_average, which refuse a bad call before they touch
the device; properties of the restatement tests/volume_ref.py (the yardstick of test_volume_gpu.py) that do not come from the
restatement itself -- a closed form, empty and blocked rays; the opacity table's correction to the step; Camera.inverse."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_ref as SR  # noqa: E402
import volume_ref as VR  # noqa: E402

from waterlily_amd import _lib, volume  # noqa: E402
from waterlily_amd.scene import Camera  # noqa: E402

F64 = np.float64


# --------------------------------------------------------------------------- the entry points refuse bad calls without a device

def grid(n=(8, 8, 8), D=3):
    g = _lib.Grid()
    g.D = D
    g.n[:] = list(n)
    g.s[:] = [1, n[0], n[0] * n[1]]
    g.sc = n[0] * n[1] * n[2]
    return g


def test_volume_entries_validate_without_gpu():
    L = _lib.lib()
    E = _lib.WL_E_ARG
    buf = (C.c_uint64 * 8)()                                   # never reached: every call below is refused first
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 1)
    g = grid()
    M = (C.c_double * 16)(*np.eye(4).ravel())
    bad_M = (C.c_double * 16)(*([1.0] * 5 + [float("inf")] + [0.0] * 10))
    u8 = (C.c_uint8 * 4)(1, 2, 3, 4)
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    names = ("t", "g", "f", "Minv", "ds", "lo", "hi", "vmin", "vmax", "levels", "lut", "opac", "t_min", "key", "bg", "rgba", "acc", "W", "H")
    good = dict(t=_lib.WL_F32, g=C.byref(g), f=p, Minv=M, ds=0.01, lo=None, hi=None, vmin=0.0, vmax=1.0, levels=0, lut=p, opac=p, t_min=0.0,
                key=p, bg=u8, rgba=p, acc=None, W=4, H=4)
    vol = lambda **k: L.wl_scene_volume(*[k.get(n, good[n]) for n in names])
    g2 = grid((8, 8, 1), D=2)
    slab = grid()
    slab.nzg, slab.kz0, slab.own_lo, slab.own_hi = 16, 0, 1, 6
    bad = [dict(g=None), dict(f=None), dict(Minv=None), dict(lut=None), dict(opac=None), dict(key=None), dict(bg=None), dict(rgba=None),
           dict(t=7), dict(g=C.byref(g2)),
           dict(lo=i3(1, 1, 1)), dict(hi=i3(7, 7, 7)),                              # only one of lo and hi
           dict(lo=i3(-1, 1, 1), hi=i3(7, 7, 7)), dict(lo=i3(1, 1, 1), hi=i3(7, 8, 7)), dict(lo=i3(1, 5, 1), hi=i3(7, 5, 7)),
           dict(lo=i3(1, 1, 3), hi=i3(7, 7, 4)),                                     # an extent below 2
           dict(Minv=bad_M), dict(Minv=(C.c_double * 16)(*([float("nan")] * 16))),
           dict(ds=0.0), dict(ds=2.0 ** -21), dict(ds=1.5), dict(ds=float("nan")), dict(ds=-0.1),
           dict(vmin=1.0), dict(vmin=2.0), dict(vmax=float("inf")), dict(vmin=float("nan")),
           dict(levels=-1), dict(levels=257),
           dict(t_min=-0.1), dict(t_min=1.0), dict(t_min=float("nan")),
           dict(W=0), dict(H=0), dict(W=4097), dict(H=4097), dict(W=-3),
           dict(rgba=odd), dict(key=odd), dict(acc=odd)]
    for k in bad:
        assert vol(**k) == E, k
    assert vol(g=C.byref(slab)) == _lib.WL_E_STATE and b"z-slab" in L.wl_last_error()
    assert vol(t=7) == E and b"dtype" in L.wl_last_error()
    assert vol(ds=1.5) == E and b"ds" in L.wl_last_error()
    assert vol(lo=i3(1, 1, 3), hi=i3(7, 7, 4)) == E and b"two cells" in L.wl_last_error()
    # the bounds themselves are accepted as far as the checks go: the next refusal is a later one
    assert vol(ds=2.0 ** -20, W=0) == E and b"1..4096" in L.wl_last_error()
    assert vol(ds=1.0, t_min=0.0, levels=256, lo=i3(0, 0, 0), hi=i3(7, 7, 7), W=0) == E and b"1..4096" in L.wl_last_error()
    # average
    assert L.wl_scene_average(None, 4, 4, 1, p) == E
    assert L.wl_scene_average(p, 4, 4, 1, None) == E
    assert L.wl_scene_average(p, 0, 4, 1, p) == E and L.wl_scene_average(p, 4, 4097, 1, p) == E
    for ssaa in (0, 3, 8, -2):
        assert L.wl_scene_average(p, 4, 4, ssaa, p) == E and b"ssaa" in L.wl_last_error()
    assert L.wl_scene_average(p, 6, 4, 4, p) == E and b"multiples" in L.wl_last_error()
    assert L.wl_scene_average(p, 4, 4, 1, odd) == E and b"aligned" in L.wl_last_error()
    assert L.wl_scene_average(odd, 4, 4, 1, p) == E


# --------------------------------------------------------------------------- the restatement against what is known without it

NX, NY, NZ = 6, 5, 7                                           # interior cells; the arrays carry one ghost layer per side


def down_camera():
    """orthographic, looking along -z, one pixel per cell (W = NX, H = NY): pixel (i, j) looks down the column of cell centres
    x = i + 0.5, y = NY - (j + 0.5).  The near plane lies at z = NZ + 0.75, the far plane NZ + 2 below it, and ds = 1/(NZ + 2), so
    the samples sit at z = NZ + 0.25 - k: a quarter of a cell from every plane of the box, whatever the last bit of ds."""
    depth = NZ + 2.0
    M = np.array([[2.0 / NX, 0, 0, -1.0], [0, 2.0 / NY, 0, -1.0], [0, 0, -1.0 / depth, (NZ + 0.75) / depth], [0, 0, 0, 1.0]], dtype=F64)
    return M, np.linalg.inv(M), 1.0 / depth


def test_closed_form_constant_field():
    """a constant field under a uniform table.  The largest box, lo = 0 and hi = n - 1, holds the cell centres z = -0.5 .. NZ - 0.5:
    a column takes the n = NZ samples k = 1..NZ.  Then T = (1 - a)^n and C = col (1 - T) exactly in real numbers; the march
    multiplies n times (n roundings of 2^-53 each) and adds n terms of two products each, so both stay within n 2^-52 relative.
    Row 0 and the last column look down the box's own upper y and x planes (the last bit decides): nothing is asked of them."""
    M, Minv, ds = down_camera()
    W, H = NX, NY
    field = np.full((NX + 2, NY + 2, NZ + 2), 0.3, dtype=F64)
    lut = np.zeros((256, 4), dtype=np.uint8)
    lut[:, 0], lut[:, 1], lut[:, 2], lut[:, 3] = 200, 90, 10, 255
    a = 0.1
    opac = np.full(256, a)
    keys = SR.clear(W, H)
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    bg = (10, 20, 30, 255)
    whole = ((0, 0, 0), (NX + 1, NY + 1, NZ + 1))
    inner = (slice(1, None), slice(0, -1))
    out, acc, taken, early, nans = VR.march(field, Minv, ds, *whole, W, H, keys, rgba, bg, 0.0, 1.0, 0, lut, opac, 0.0)
    n = NZ
    assert np.all(taken[inner] == n) and not early.any() and not nans.any()
    T = (1.0 - a) ** n
    tol = n * 2.0 ** -52
    assert np.all(np.abs(acc[inner][..., 3] - T) <= tol * T)
    for c, col in enumerate((200.0, 90.0, 10.0)):
        assert np.all(np.abs(acc[inner][..., c] - col * (1.0 - T)) <= tol * col * (1.0 - T))
    want = [int(np.floor(col * (1.0 - T) + T * b + 0.5)) for col, b in zip((200.0, 90.0, 10.0), bg)] + [255]
    assert np.all(out[inner] == np.array(want, dtype=np.uint8))
    # the inside() box: z from 0.5 to NZ - 0.5 holds the samples k = 1..NZ - 1 (now the first column and the last row lie on planes too)
    _, acc2, taken2, _, _ = VR.march(field, Minv, ds, (1, 1, 1), (NX + 1, NY + 1, NZ + 1), W, H, keys, rgba, bg, 0.0, 1.0, 0, lut, opac, 0.0)
    assert np.all(taken2[1:-1, 1:-1] == NZ - 1)
    T2 = (1.0 - a) ** (NZ - 1)
    assert np.all(np.abs(acc2[1:-1, 1:-1, 3] - T2) <= tol * T2)
    # t_min: the march stops after the first sample that brings T below it, with T kept (0.9^3 = 0.729, 0.9^4 = 0.6561)
    _, acc3, taken3, early3, _ = VR.march(field, Minv, ds, *whole, W, H, keys, rgba, bg, 0.0, 1.0, 0, lut, opac, 0.7)
    assert np.all(taken3[inner] == 4) and early3[inner].all() and np.all(np.abs(acc3[inner][..., 3] - 0.9 ** 4) <= tol)


def test_empty_and_blocked_rays_return_base():
    M, Minv, ds = down_camera()
    W, H = NX, NY
    rng = np.random.default_rng(2)
    field = rng.uniform(0.0, 1.0, (NX + 2, NY + 2, NZ + 2))
    lut = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    opac = np.full(256, 0.2)
    rgba = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    bg = (7, 8, 9, 10)
    keys = SR.clear(W, H)
    front = int(0.01 * 2 ** 32) << 32 | 5                      # a surface at depth 0.01: before the first sample at 0.5 ds = 0.055
    for i in range(W):
        keys[0][i] = front
        keys[3][i] = int(0.45 * 2 ** 32) << 32 | 6             # ... and one in the middle of the march
    # the cell centres x = 1.5 .. 4.5, y = -0.5 .. NY - 0.5, z = -0.5 .. NZ - 0.5: pixels 2 and 3 look down the inside of the box,
    # pixels 0 and 5 pass it by (1 and 4, and row 0, look down its own planes: the last bit decides, nothing is asked of them)
    lo, hi = (2, 0, 0), (6, NY + 1, NZ + 1)
    out, acc, taken, early, _ = VR.march(field, Minv, ds, lo, hi, W, H, keys, rgba, bg, 0.0, 1.0, 0, lut, opac, 0.0)
    base = np.where((SR.as_array(keys) == np.uint64(SR.NOTHING))[..., None], np.array(bg, dtype=np.uint8), rgba)
    for i in (0, 5):                                           # empty rays: base exactly, with and without a key
        assert np.all(taken[:, i] == 0) and np.array_equal(out[:, i], base[:, i])
        assert np.all(acc[:, i] == np.array([0.0, 0.0, 0.0, 1.0]))
    assert np.all(taken[0] == 0) and np.array_equal(out[0], base[0]) and np.array_equal(out[0], rgba[0])   # blocked: the frame's pixel
    for i in (2, 3):
        assert np.all(taken[[1, 2, 4], i] == NZ) and np.all(acc[[1, 2, 4], i, 3] < 0.8 ** NZ * 1.001)
        # the surface at depth 0.45 cuts the march short: s_k = (k + 0.5)/(NZ + 2) < 0.45 for k = 0..3, and k = 0 lies above the box
        assert taken[3, i] == 3 and abs(acc[3, i, 3] - 0.8 ** 3) < 1e-15
    assert np.any(out[1:, 2:4] != base[1:, 2:4])


def test_opacity_table_follows_the_step():
    """two steps of 0.5 absorb what one step of 1 does.  With t = fl(1 - A) (shared by both), the table of step 1 leaves the
    transmission 1 - (1 - t) = t exactly (t >= 0.5: both subtractions are exact); the table of step 0.5 leaves r = t**0.5 with a
    relative error e1 of at most an ulp of r (2^-53 of 1), and r*r adds a rounding e2: |r*r - t| <= t (2 e1 + e2) <= 3 2^-53, which
    is below 2 ulp of 1 = 2^-51."""
    for kind in ("uniform", "ramp", "abs", np.linspace(0.0, 0.5, 256)):
        one, half = volume.opacity(kind, 0.4, 1.0), volume.opacity(kind, 0.4, 0.5)
        assert one.shape == half.shape == (256,) and one.dtype == half.dtype == F64
        assert np.all(np.abs((1.0 - half) * (1.0 - half) - (1.0 - one)) <= 2 * np.spacing(1.0))
        assert np.all((0.0 <= half) & (half <= one) & (one <= 0.5))
    ramp = volume.opacity("ramp", 0.3)
    assert ramp[0] == 0.0 and abs(ramp[255] - 0.3) < 1e-15 and np.all(np.diff(ramp) > 0)
    ab = volume.opacity("abs", 0.3)
    assert abs(ab[0] - 0.3) < 1e-15 and abs(ab[255] - 0.3) < 1e-15 and np.allclose(ab, ab[::-1], atol=1e-15) and ab[127] == ab[128] < 0.002
    assert np.all(volume.opacity("uniform", 0.25) == 0.25)
    for bad in (dict(kind="cloud"), dict(kind=np.zeros(255)), dict(kind="ramp", strength=1.5), dict(kind="ramp", step=0.0),
                dict(kind="ramp", step=-1.0), dict(kind=np.full(256, -0.1))):
        with pytest.raises(ValueError):
            volume.opacity(**bad)


def test_camera_inverse():
    class FlowLike:
        N = (24, 21, 19)
    cams = [Camera.fit(FlowLike, (1.0, 0.6, -0.5), aspect=40 / 24), Camera.fit(FlowLike, (1.0, 0.6, -0.5), fov=40.0, aspect=37 / 19),
            Camera.look_at((30.0, -12.0, 9.0), (4.0, 5.0, 6.0), fov=55.0, near=0.5, far=70.0)]
    for cam in cams:
        for W, H in ((40, 24), (37, 19)):
            inv = cam.inverse(W, H)
            assert inv.shape == (4, 4) and inv.dtype == F64
            assert np.abs(inv @ cam.matrix(W, H) - np.eye(4)).max() <= 1e-12
            assert np.abs(cam.matrix(W, H) @ inv - np.eye(4)).max() <= 1e-12
