"""Scene without a GPU: properties of the restatement tests/scene_ref.py (the yardstick of test_scene_gpu.py), the cameras of
waterlily_amd.scene, and the argument checks of every wl_scene_* entry, which refuse a bad call before they touch the device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_ref as SR  # noqa: E402

from waterlily_amd import _lib  # noqa: E402
from waterlily_amd.scene import Camera  # noqa: E402

F64 = np.float64
SIZES = [(64, 48), (70, 33)]


def ndc(M, p):
    c = np.asarray(M) @ np.array([p[0], p[1], p[2], 1.0])
    return c[:3] / c[3], c[3]


@pytest.mark.parametrize("kind", ["perspective", "orthographic"])
def test_look_at_centre_near_far(kind):
    eye, target = np.array([30.0, -12.0, 9.0]), np.array([4.0, 5.0, 6.0])
    near, far = 3.0, 70.0
    cam = Camera.look_at(eye, target, fov=40.0, near=near, far=far) if kind == "perspective" else \
        Camera.look_at(eye, target, width=25.0, near=near, far=far)
    W, H = 70, 33
    M = cam.matrix(W, H)
    assert M.shape == (4, 4) and M.dtype == F64
    n, w = ndc(M, target)
    assert abs(n[0]) < 1e-13 and abs(n[1]) < 1e-13 and w > 0                       # the image centre
    v = SR.vertex(M, target, W, H)
    assert v is not None and abs(v[0] - 128 * W) <= 1 and abs(v[1] - 128 * H) <= 1
    f = (target - eye) / np.linalg.norm(target - eye)
    side = np.cross(f, [0, 0, 1.0])
    for dist, want in ((near, 0.0), (far, 1.0)):
        n, _ = ndc(M, eye + dist * f + 0.3 * side)                                  # any point of the plane
        assert abs(n[2] - want) < 1e-12
    # up is up and right is right: a point above the target has a smaller row, one to the right a larger column
    up = SR.vertex(M, target + np.array([0, 0, 1.0]), W, H)
    rt = SR.vertex(M, target + side / np.linalg.norm(side), W, H)
    assert up[1] < v[1] and abs(up[0] - v[0]) <= 1 and rt[0] > v[0]
    # square pixels (orthographic: no foreshortening): a world unit across and one upwards span the same number of sub-pixels
    assert kind == "perspective" or abs((rt[0] - v[0]) - (v[1] - up[1]) / np.sqrt(1 - f[2] ** 2)) <= 2


def test_camera_refusals_and_fit():
    with pytest.raises(ValueError):
        Camera.look_at((0, 0, 5), (0, 0, 0))                                        # neither fov nor width
    with pytest.raises(ValueError):
        Camera.look_at((0, 0, 5), (0, 0, 0), fov=30, width=3)
    with pytest.raises(ValueError):
        Camera.look_at((0, 0, 5), (0, 0, 0), fov=30)                                # up parallel to the view

    class FlowLike:
        N = (34, 14, 12)
    for kw in (dict(), dict(fov=35.0)):
        for aspect, (W, H) in ((64 / 48, (64, 48)), (33 / 70, (33, 70))):
            cam = Camera.fit(FlowLike, (1.0, 0.7, -0.4), aspect=aspect, **kw)
            M = cam.matrix(W, H)
            for corner in np.ndindex(2, 2, 2):                                      # every corner of the box is inside the picture
                p = np.array(corner, dtype=F64) * (np.array(FlowLike.N) - 2.0)
                n, w = ndc(M, p)
                assert w > 0 and np.all(np.abs(n[:2]) <= 1.0) and 0.0 <= n[2] <= 1.0


@pytest.mark.parametrize("W,H", SIZES)
def test_quad_pair_covers_once(W, H):
    """two triangles sharing a diagonal through pixel centres, the square's sides through centres too: every pixel of the square
    is covered by exactly one of them, top and left sides in, bottom and right out"""
    M = SR.ortho_screen(W, H)
    x0, y0, n = 3, 2, 9
    tris = SR.quad_pair(x0, y0, n)
    count = np.zeros((H, W), dtype=int)
    on_diagonal = 0
    for t in range(2):
        T = SR.setup(M, tris[t], W, H)
        assert T is not None
        for j in range(H):
            for i in range(W):
                ok, E = SR.cover(T, i, j)
                count[j, i] += ok
                on_diagonal += (ok and 0 in E and i - x0 == j - y0)
    want = np.zeros((H, W), dtype=int)
    want[y0:y0 + n, x0:x0 + n] = 1
    assert np.array_equal(count, want)
    assert on_diagonal == n                                    # the diagonal's centres were really on the shared edge
    # both windings: the mirrored order gives the same coverage
    keys_a, keys_b = SR.clear(W, H), SR.clear(W, H)
    SR.draw(keys_a, M, tris, W, H)
    SR.draw(keys_b, M, tris[:, ::-1], W, H)
    assert np.array_equal(SR.ids(keys_a), SR.ids(keys_b))     # (the depth's last bit may follow the order of the vertices)
    assert np.array_equal(SR.ids(keys_a) >= 0, want == 1)


@pytest.mark.parametrize("W,H", SIZES)
def test_jittered_sheet_leaves_no_hole(W, H):
    M = SR.ortho_screen(W, H)
    tris = SR.sheet(W, H)
    count = np.zeros((H, W), dtype=int)
    for t in range(len(tris)):
        T = SR.setup(M, tris[t], W, H)
        if T is None:
            continue
        for j in range(T.jlo, T.jhi + 1):
            for i in range(T.ilo, T.ihi + 1):
                count[j, i] += SR.cover(T, i, j)[0]
    assert np.all(count == 1)                                  # no background pixel, and no pixel twice
    keys = SR.clear(W, H)
    SR.draw(keys, M, tris, W, H)
    assert np.all(SR.ids(keys) >= 0)


def test_coplanar_copies_lower_id_wins():
    W, H = 64, 48
    M = SR.ortho_screen(W, H)
    one = np.array([[[5.2, 4.1, 0.3], [50.7, 9.9, 0.6], [20.3, 40.2, 0.8]]], dtype=F64)
    for order in ((0, 1), (1, 0)):                             # whichever is drawn first
        keys = SR.clear(W, H)
        for t in order:
            SR.draw(keys, M, one, W, H, base=10 + t)
        got = SR.ids(keys)
        assert (got >= 0).sum() > 300 and set(np.unique(got)) == {-1, 10}
    # ... and a nearer copy wins whatever its id
    keys = SR.clear(W, H)
    SR.draw(keys, M, one, W, H, base=1)
    near = one.copy()
    near[..., 2] -= 0.125
    SR.draw(keys, M, near, W, H, base=7)
    assert set(np.unique(SR.ids(keys))) == {-1, 7}


def test_dropped_triangles():
    W, H = 64, 48
    M = SR.perspective(W, H)
    ok = [[-0.5, -0.3, 0.0], [0.5, -0.3, 0.1], [0.0, 0.4, -0.1]]
    assert SR.setup(M, np.array(ok), W, H) is not None
    nan = [[np.nan, -0.3, 0.0], ok[1], ok[2]]
    behind = [[-0.5, -0.3, 4.0], ok[1], ok[2]]                # c_3 = 3 - z < 0
    near = [[-0.5, -0.3, 2.5], ok[1], ok[2]]                  # between the eye and the near plane (distance 0.5 < 1)
    far = [[-0.5, -0.3, -4.0], ok[1], ok[2]]                  # beyond the far plane (distance 7 > 6)
    flat = [ok[0], ok[1], [0.0, -0.3, 0.05]]                  # zero area on the screen
    huge = [[-0.5, -0.3, 0.0], [3.0e4, -0.3, 0.0], ok[2]]      # s_x beyond 2^19
    for bad in (nan, behind, near, far, flat, huge):
        assert SR.setup(M, np.array(bad, dtype=F64), W, H) is None


def test_resolve_rounding():
    rgba = np.zeros((2, 4, 4), dtype=np.uint8)
    rgba[..., 0] = [[1, 2, 255, 255], [2, 2, 255, 254]]
    rgba[..., 3] = 255
    keys = SR.clear(4, 2)
    for j in range(2):
        for i in range(4):
            keys[j][i] = 5
    keys[0][0] = SR.NOTHING
    out = SR.resolve(rgba, keys, 2, (9, 9, 9, 9))
    assert out.shape == (1, 2, 4)
    assert out[0, 0, 0] == (9 + 2 + 2 + 2 + 2) // 4 and out[0, 1, 0] == 255 and out[0, 0, 3] == (9 + 3 * 255 + 2) // 4


# --------------------------------------------------------------------------- the entry points refuse bad calls without a device

def test_scene_entries_validate_without_gpu():
    L = _lib.lib()
    E = _lib.WL_E_ARG
    buf = (C.c_uint64 * 8)()                                   # never reached: every call below is refused first
    p = C.cast(buf, C.c_void_p)
    M = (C.c_double * 16)(*np.eye(4).ravel())
    bad_M = (C.c_double * 16)(*([float("nan")] + [0.0] * 15))
    u8 = (C.c_uint8 * 4)(1, 2, 3, 4)
    l3 = (C.c_double * 3)(0, 0, 1)
    # clear
    assert L.wl_scene_clear(None, 4, 4) == E
    for W, H in ((0, 4), (4, 0), (4097, 4), (4, 4097), (-1, 4)):
        assert L.wl_scene_clear(p, W, H) == E and b"1..4096" in L.wl_last_error()
    # scratch
    nb = C.c_int64(-1)
    assert L.wl_scene_scratch(10, C.byref(nb)) == 0 and nb.value == 16 + 40
    assert L.wl_scene_scratch(-1, C.byref(nb)) == E and L.wl_scene_scratch(1 << 32, C.byref(nb)) == E
    assert L.wl_scene_scratch(1, None) == E
    # draw
    assert L.wl_scene_draw(None, 4, 4, M, p, 1, 0, 64, p, 64) == E
    assert L.wl_scene_draw(p, 4, 4, M, p, 1, 0, 64, None, 64) == E
    assert L.wl_scene_draw(p, 4, 4, None, p, 1, 0, 64, p, 64) == E
    assert L.wl_scene_draw(p, 4, 4, bad_M, p, 1, 0, 64, p, 64) == E and b"finite" in L.wl_last_error()
    assert L.wl_scene_draw(p, 4, 4, M, None, 1, 0, 64, p, 64) == E
    assert L.wl_scene_draw(p, 0, 4, M, p, 1, 0, 64, p, 64) == E
    assert L.wl_scene_draw(p, 4, 5000, M, p, 1, 0, 64, p, 64) == E
    assert L.wl_scene_draw(p, 4, 4, M, p, -1, 0, 64, p, 64) == E and b"negative nt" in L.wl_last_error()
    assert L.wl_scene_draw(p, 4, 4, M, p, 2, 0xFFFFFFFE, 64, p, 64) == E and b"2^32" in L.wl_last_error()
    assert L.wl_scene_draw(p, 4, 4, M, p, 1, 0, -1, p, 64) == E and b"large_px" in L.wl_last_error()
    assert L.wl_scene_draw(p, 4, 4, M, p, 4, 0, 64, p, 31) == E and b"scratch" in L.wl_last_error()
    # shade
    shade = lambda **k: L.wl_scene_shade(*[k.get(n, d) for n, d in (
        ("key", p), ("W", 4), ("H", 4), ("base", 0), ("nt", 1), ("tri", p), ("val", p), ("M", M), ("vmin", 0.0), ("vmax", 1.0), ("levels", 0),
        ("lut", p), ("solid", u8), ("light", l3), ("ambient", 0.3), ("nan", u8), ("out", p))])
    for k in (dict(key=None), dict(out=None), dict(light=None), dict(M=None), dict(tri=None), dict(lut=None), dict(W=0), dict(H=4097),
              dict(nt=-1), dict(base=0xFFFFFFFF), dict(vmin=1.0), dict(vmax=float("inf")), dict(levels=257), dict(levels=-1),
              dict(ambient=1.5), dict(ambient=float("nan")), dict(light=(C.c_double * 3)(0, float("inf"), 0)), dict(M=bad_M),
              dict(val=None, solid=None)):
        assert shade(**k) == E, k
    # resolve
    assert L.wl_scene_resolve(None, 4, 4, p, 1, u8, p) == E
    assert L.wl_scene_resolve(p, 4, 4, None, 1, u8, p) == E
    assert L.wl_scene_resolve(p, 4, 4, p, 1, None, p) == E
    assert L.wl_scene_resolve(p, 4, 4, p, 1, u8, None) == E
    assert L.wl_scene_resolve(p, 4, 0, p, 1, u8, p) == E
    for ssaa in (0, 3, 8, -2):
        assert L.wl_scene_resolve(p, 4, 4, p, ssaa, u8, p) == E and b"ssaa" in L.wl_last_error()
    assert L.wl_scene_resolve(p, 6, 4, p, 4, u8, p) == E and b"multiples" in L.wl_last_error()
