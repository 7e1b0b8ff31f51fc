"""Scene on the GPU (waterlily_amd.scene: wl_scene_clear / draw / shade / resolve) against the restatement tests/scene_ref.py.

Images are 64 x 48 and 70 x 33 (no multiple of the wavefront path's 8 x 8 tile); the ssaa = 2 set draws at 64 x 48 and 70 x 66 and
resolves to 32 x 24 and 35 x 33.  The orthographic camera is the one under which world coordinates are pixels; the perspective
camera has an eye at distance 3 of the picture plane with the soup spread +-0.45 around it.

Why equality of the keys: the vertex stage is IEEE double operations in an order the contract fixes (the library is built without
contraction), everything after the snap to sub-pixels is integers and three correctly rounded divisions; the minimum of
integers has no order.  The lit colour channels alone may differ by one: the normal's length takes the one sqrt that is not
held to a correctly rounded result, and a last-bit difference in s moves floor(c*s + 0.5) by at most one."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_ref as RR  # noqa: E402
import scene_ref as SR  # noqa: E402

from waterlily_amd import body as B, iso, render, scene, sim as S  # noqa: E402
from waterlily_amd.mesh import MeshBody  # noqa: E402
from waterlily_amd.surface import _to_x  # noqa: E402

pytestmark = pytest.mark.gpu

F64 = np.float64
DEV = "cuda"
CASES = [(64, 48, "ortho"), (70, 33, "persp"), (70, 33, "ortho"), (64, 48, "persp")]
IDS = [f"{W}x{H}-{c}" for W, H, c in CASES]
LIGHT = (0.3, -0.2, 0.9)


def camera(W, H, cam):
    return SR.ortho_screen(W, H) if cam == "ortho" else SR.perspective(W, H)


@functools.lru_cache(maxsize=None)
def soup_case(W, H, cam):
    """(M, tris, reference keys as uint64 [H, W], pixels of every triangle's clamped box): made once, read-only"""
    tris = SR.soup(W, H)
    if cam == "persp":
        tris = SR.to_world(tris, W, H)
    M = camera(W, H, cam)
    keys = SR.clear(W, H)
    npix = np.array(SR.draw(keys, M, tris, W, H))
    out = SR.as_array(keys)
    for a in (tris, out, npix):
        a.setflags(write=False)
    return M, tris, out, npix


def dev(a):
    return torch.from_numpy(np.array(a, dtype=F64, order="C")).to(DEV)


def keys_of(sc):
    return sc.keys.cpu().numpy().view(np.uint64).copy()


def drawn(W, H, M, tris, large_px=64, ssaa=1):
    sc = scene.Scene(DEV, size=(W // ssaa, H // ssaa), ssaa=ssaa, ring=2)
    scene.clear(sc)
    scene.draw(sc, M, dev(tris), light=LIGHT, large_px=large_px)
    return sc


@pytest.mark.parametrize("W,H,cam", CASES, ids=IDS)
def test_keys_bit_for_bit(W, H, cam):
    M, tris, want, npix = soup_case(W, H, cam)
    assert len(tris) == 2000
    lanes, waves = int(((npix > 0) & (npix <= 64)).sum()), int((npix > 64).sum())
    assert 20 <= lanes <= 1900 and 20 <= waves <= 1900, (lanes, waves)            # both paths run
    assert (want != np.uint64(SR.NOTHING)).sum() * 3 > W * H                        # more than a third of the picture is covered
    got = keys_of(drawn(W, H, M, tris))
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("W,H,cam", CASES[:2], ids=IDS[:2])
def test_path_and_order_independence(W, H, cam):
    M, tris, want, _ = soup_case(W, H, cam)
    assert np.array_equal(keys_of(drawn(W, H, M, tris, large_px=0)), want)          # every triangle by a wavefront
    assert np.array_equal(keys_of(drawn(W, H, M, tris, large_px=W * H)), want)      # every triangle by its lane
    perm = np.random.default_rng(11).permutation(len(tris))
    got = keys_of(drawn(W, H, M, tris[perm]))
    hit = got != np.uint64(SR.NOTHING)
    back = (got & np.uint64(0xFFFFFFFF00000000)) | perm[(got & np.uint64(0xFFFFFFFF)).astype(np.int64) % len(tris)].astype(np.uint64)
    assert np.array_equal(hit, want != np.uint64(SR.NOTHING)) and np.array_equal(back[hit], want[hit])


def test_dropped_triangles_leave_nothing():
    W, H = 70, 33
    M = SR.perspective(W, H)
    ok = [[-0.5, -0.3, 0.0], [0.5, -0.3, 0.1], [0.0, 0.4, -0.1]]
    bad = [[[np.nan, -0.3, 0.0], ok[1], ok[2]],                # a NaN vertex
           [[-0.5, -0.3, 4.0], ok[1], ok[2]],                  # behind the eye
           [[-0.5, -0.3, 2.5], ok[1], ok[2]],                  # crossing the near plane
           [ok[0], ok[1], [0.0, -0.3, 0.05]],                  # zero area
           [[-0.5, -0.3, 0.0], [3.0e4, -0.3, 0.0], ok[2]]]     # beyond 2^19 pixels
    tris = np.array([ok] + bad, dtype=F64)
    alone = SR.clear(W, H)
    SR.draw(alone, M, tris[:1], W, H)
    assert (SR.ids(alone) == 0).sum() > 100
    for large_px in (64, 0):
        assert np.array_equal(keys_of(drawn(W, H, M, tris, large_px=large_px)), SR.as_array(alone))


@pytest.mark.parametrize("W,H", [(64, 48), (70, 33)])
def test_quad_pair_and_sheet(W, H):
    M = SR.ortho_screen(W, H)
    quad = SR.quad_pair()
    want = SR.clear(W, H)
    SR.draw(want, M, quad, W, H)
    got = keys_of(drawn(W, H, M, quad))
    assert np.array_equal(got, SR.as_array(want))
    inside = np.zeros((H, W), dtype=bool)
    inside[2:11, 3:12] = True
    assert np.array_equal(got != np.uint64(SR.NOTHING), inside)                     # every pixel of the square, no other
    sheet = SR.sheet(W, H)
    want = SR.clear(W, H)
    SR.draw(want, M, sheet, W, H)
    for large_px in (64, 0):
        got = keys_of(drawn(W, H, M, sheet, large_px=large_px))
        assert np.all(got != np.uint64(SR.NOTHING)) and np.array_equal(got, SR.as_array(want))


def check_rgba(got, want, ident, nan_mask, what):
    """alpha, background, NaN pixels exact; lit channels within one; prints how many channels differ"""
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got[..., 3], want[..., 3])
    exact = (ident < 0) | nan_mask
    assert np.array_equal(got[exact], want[exact])
    diff = np.abs(got[..., :3].astype(int) - want[..., :3].astype(int))
    print(f"{what}: {int((diff != 0).sum())} of {diff.size} colour channels differ from the reference (largest {int(diff.max())})")
    assert diff.max() <= 1


def test_depth_order_across_draws():
    """a large grey triangle at depth 0.5 and a coloured, jittered planar sheet whose depth rises from 0.2 on the left to 0.8 on the
    right: the sheet shows left of the column where the planes cross, the triangle right of it"""
    W, H = 70, 33
    M = SR.ortho_screen(W, H)
    grey = np.array([[[2.0, 1.0, 0.5], [68.0, 3.0, 0.5], [30.0, 32.5, 0.5]]], dtype=F64)
    zfun = lambda x, y: 0.2 + 0.6 * x / W
    sheet = SR.sheet(W, H, zfun=zfun)
    val = np.ascontiguousarray(sheet[..., 1] / H)                # coloured by the row
    lut = render.colormap("RdBu")
    sc = scene.Scene(DEV, size=(W, H), ring=2)
    scene.clear(sc)
    tg, ts, tv = dev(grey), dev(sheet), dev(val)
    scene.draw(sc, M, tg, light=LIGHT, color=(128, 128, 128, 255))
    scene.draw(sc, M, ts, tv, clims=(0.0, 1.0), light=LIGHT, large_px=16)
    got = scene.frame(sc, background=(1, 2, 3, 4)).cpu().numpy()
    keys = SR.clear(W, H)
    SR.draw(keys, M, grey, W, H, base=0)
    SR.draw(keys, M, sheet, W, H, base=1)
    assert np.array_equal(keys_of(sc), SR.as_array(keys))
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    SR.shade(rgba, keys, M, grey, W, H, base=0, solid=(128, 128, 128, 255), light=unit(LIGHT), ambient=0.3)
    SR.shade(rgba, keys, M, sheet, W, H, base=1, val=val, vmin=0.0, vmax=1.0, lut=lut, light=unit(LIGHT), ambient=0.3)
    ident = SR.ids(keys)
    check_rgba(got, SR.resolve(rgba, keys, 1, (1, 2, 3, 4)), ident, np.zeros((H, W), dtype=bool), "two draws")
    only = SR.clear(W, H)
    SR.draw(only, M, grey, W, H)
    in_grey = SR.ids(only) == 0
    x = np.arange(W)[None, :] + 0.5 + np.zeros((H, 1))
    cross = W / 2                                              # 0.2 + 0.6 x / W == 0.5
    assert in_grey.sum() > 500
    assert np.all(ident[in_grey & (x < cross - 1)] >= 1) and np.all(ident[in_grey & (x > cross + 1)] == 0)
    assert np.all(ident[~in_grey] >= 1)                        # the sheet is everywhere else


def unit(v):
    v = np.asarray(v, dtype=F64)
    return v / np.sqrt(np.dot(v, v))


@pytest.mark.parametrize("W,H,cam,ssaa,levels", [(64, 48, "persp", 1, 0), (70, 33, "ortho", 1, 5), (64, 48, "ortho", 2, 0),
                                                 (70, 66, "persp", 2, 7)])
def test_shade_and_resolve(W, H, cam, ssaa, levels):
    """W x H is the size the triangles are drawn at; the frame is (W / ssaa) x (H / ssaa)"""
    M = camera(W, H, cam)
    rng = np.random.default_rng(5)
    tris = SR.soup(W, H, seed=9, n_small=300, n_big=12, n_edge=8)
    if cam == "persp":
        tris = SR.to_world(tris, W, H)
    val = rng.uniform(-1.0, 2.0, (len(tris), 3))
    val[rng.uniform(size=len(tris)) < 0.1, 1] = np.nan          # a tenth of the triangles carry a NaN
    lut = render.colormap("RdBu")
    sc = scene.Scene(DEV, size=(W // ssaa, H // ssaa), ssaa=ssaa, ring=2)
    scene.clear(sc)
    tt, tv = dev(tris), dev(val)
    scene.draw(sc, M, tt, tv, clims=(-0.5, 1.5), levels=levels, light=LIGHT, ambient=0.25, nan_rgba=(9, 8, 7, 6))
    bg = (250, 240, 230, 255)
    got = scene.frame(sc, background=bg).cpu().numpy()
    keys = SR.clear(W, H)
    SR.draw(keys, M, tris, W, H)
    assert np.array_equal(keys_of(sc), SR.as_array(keys))
    rgba = np.zeros((H, W, 4), dtype=np.uint8)
    values = np.zeros((H, W), dtype=F64)
    SR.shade(rgba, keys, M, tris, W, H, val=val, vmin=-0.5, vmax=1.5, levels=levels, lut=lut, light=unit(LIGHT), ambient=0.25,
             nan_rgba=(9, 8, 7, 6), values=values)
    ident = SR.ids(keys)
    nan = (ident >= 0) & np.isnan(values)
    assert nan.sum() > 10 and (ident >= 0).sum() > 200 and (ident < 0).sum() > 200
    # at the drawn size: the frame before the resolve (every pixel of a triangle, background excluded)
    raw = sc._rgba.tensor(torch.uint8, sc.device)[:W * H * 4].view(H, W, 4).cpu().numpy()
    raw = np.where((ident >= 0)[..., None], raw, 0)
    check_rgba(raw, rgba, np.where(ident >= 0, ident, 0), nan, f"{W}x{H} {cam} shade")
    assert np.array_equal(raw[nan], np.broadcast_to(np.array((9, 8, 7, 6), dtype=np.uint8), raw[nan].shape))
    want = SR.resolve(rgba, keys, ssaa, bg)
    assert got.shape == (H // ssaa, W // ssaa, 4)
    if ssaa == 1:
        check_rgba(got, want, ident, nan, f"{W}x{H} {cam} frame")
    else:                                                      # a block's average moves by at most one when its pixels do
        assert np.abs(got.astype(int) - want.astype(int)).max() <= 1
        assert np.array_equal(got, SR.resolve(np.where((ident >= 0)[..., None], raw, 0).astype(np.uint8), keys, ssaa, bg))
        untouched = (ident < 0).reshape(H // ssaa, ssaa, W // ssaa, ssaa).all(axis=(1, 3))
        assert untouched.sum() > 20 and np.all(got[untouched] == np.array(bg, dtype=np.uint8))


def test_end_to_end_sphere():
    """iso.extract of a sphere's distance field on a (33, 12, 10) Float32 flow, seen orthographically along z, coloured by a linear
    field through the gray table with ambient = 1 (no lighting: the channel IS the colour index)"""
    shape = (33, 12, 10)
    flow = S.Flow(shape, (0.0, 0.0, 0.0), T=np.float32)
    Ng = tuple(n + 2 for n in shape)
    J = np.stack(np.meshgrid(*[np.arange(n, dtype=F64) for n in Ng], indexing="ij"))
    X = J - 0.5                                                # the frame of the triangles
    c, r = np.array([15.3, 6.1, 5.2]), 3.7
    g, c0 = np.array([0.5, -0.25]), 2.0
    a, b = S.like(flow.p), S.like(flow.p)
    S.upload(a, np.asfortranarray((np.sqrt(sum((X[d] - c[d]) ** 2 for d in range(3))) - r).astype(np.float32)))
    S.upload(b, np.asfortranarray((g[0] * X[0] + g[1] * X[1] + c0).astype(np.float32)))
    isf = iso.Isosurface(flow, capacity=1 << 14)
    tri, val = iso.extract(isf, a, 0.0, color=b)
    assert tri.shape[0] > 200
    W, H, s = 64, 48, 4.0                                      # s pixels per cell
    cam = scene.Camera.look_at((c[0], c[1], 30.0), (c[0], c[1], c[2]), up=(0, 1, 0), width=W / s, near=1.0, far=40.0)
    vmin, vmax = 0.0, 16.0
    sc = scene.Scene(flow, size=(W, H), ring=2)
    scene.clear(sc)
    scene.draw(sc, cam, tri, val, clims=(vmin, vmax), cmap="gray", ambient=1.0)
    got = scene.frame(sc, background=(0, 0, 255, 255)).cpu().numpy().copy()
    covered = keys_of(sc) != np.uint64(SR.NOTHING)
    # the disc: pixel (i, j) is the square [i, i+1] x [j, j+1] around the centre (W/2, H/2), radius r s
    ii, jj = np.meshgrid(np.arange(W, dtype=F64), np.arange(H, dtype=F64), indexing="xy")
    corners = [np.hypot(ii + a0 - W / 2, jj + b0 - H / 2) for a0 in (0, 1) for b0 in (0, 1)]
    R = r * s
    outline = (np.minimum.reduce(corners) < R) & (np.maximum.reduce(corners) > R)
    assert abs(int(covered.sum()) - np.pi * R * R) <= outline.sum()
    # (the surface is a polyhedron inscribed in the sphere: its outline may lie a fraction of a pixel inside the circle, never outside)
    assert np.all(covered[np.maximum.reduce(corners) <= R - 1.0]) and not np.any(covered[np.minimum.reduce(corners) >= R])
    assert np.all(got[~covered] == np.array((0, 0, 255, 255), dtype=np.uint8))
    # the value of every covered pixel, read back from the colour index (bins 1/16 wide, an eighth of the bound), against the field
    # at the pixel centre's (x, y): right = +x, up = +y
    xw = c[0] + (ii + 0.5 - W / 2) / s
    yw = c[1] + (H / 2 - (jj + 0.5)) / s
    expect = g[0] * xw + g[1] * yw + c0
    idx = got[..., 0].astype(F64)
    assert np.array_equal(got[covered][:, 0], got[covered][:, 1]) and np.all(got[covered][:, 3] == 255)
    value = vmin + (idx + 0.5) / 256.0 * (vmax - vmin)
    assert np.abs(value - expect)[covered].max() <= np.abs(g).max()                 # the field's change over one cell
    # two records and a save: the APNG holds the two frames
    scene.record(sc)
    scene.clear(sc)
    scene.draw(sc, cam, tri, val, clims=(vmin, vmax), cmap="gray", ambient=0.5)
    second = scene.frame(sc).cpu().numpy().copy()
    scene.record(sc)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "sphere.png")
        scene.save(sc, path, fps=5)
        frames, tags = RR.decode(open(path, "rb").read())
    assert len(frames) == 2 and b"acTL" in tags
    assert np.array_equal(frames[0], np.where(covered[..., None], got, np.array((255, 255, 255, 255), dtype=np.uint8)))
    assert np.array_equal(frames[1], second) and not np.array_equal(frames[0], frames[1])


def test_body_triangles_pose():
    """the golden cube under body.rotation3d: the device's posed triangles against the host's posed vertices (the pose
    surface.write_vtp writes).  Both sides form three products and two sums per coordinate, each rounded at half an ulp of a
    term no larger than the largest coordinate's scale: 4 ulp of that coordinate bounds their difference."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_cube_bin.stl")
    mb = MeshBody.from_stl(path, map=B.rotation3d((9.0, 7.5, 6.0), (1.0, 2.0, 0.5), 0.15, th0=0.4), scale=3.0)
    for t in (0.0, 2.75):
        got = scene.body_triangles(mb, t)
        assert got.dtype == torch.float64 and got.is_cuda and got.is_contiguous() and tuple(got.shape) == (len(mb.triangles), 3, 3)
        want = _to_x(mb, mb.vertices, t)[mb.triangles]
        assert np.abs(got.cpu().numpy() - want).max() <= 4 * np.spacing(np.abs(want).max())
    plain = MeshBody.from_stl(path)
    assert np.array_equal(scene.body_triangles(plain, 1.0).cpu().numpy(), plain.vertices[plain.triangles])
