"""Volume on the GPU (waterlily_amd.volume: wl_scene_volume / wl_scene_average) against the restatement tests/volume_ref.py.

The grid has 22 x 19 x 17 cells plus ghosts in pitched rows, Float32 and Float64; the field is seeded noise plus a smooth blob with
about 1 % of the cells NaN.  Images are 40 x 24 and 37 x 19 (no multiple of the kernel's 8 x 8 tile: tiles hang over the right and
the lower edge, and there is more than one workgroup of four tiles).  Cameras: Camera.fit along (1, 0.6, -0.5), orthographic and
with fov = 40, and one camera INSIDE the box, whose rays start at s_in = 0 with the near plane inside the sampled region.

Why equality: the march is IEEE double operations in an order the contract fixes (the library is built without contraction),
with correctly rounded divisions and no sqrt or transcendental on the device; the tables are made on the host and handed to both
sides.  So acc and rgba carry no tolerance.  The one thing taken from the device is the shaded frame UNDER the cloud where a
surface was drawn: its lit channels hold the one sqrt of wl_scene_shade, which test_scene_gpu.py holds to within one.

The kernel has one path and one launch shape (a wavefront per tile, four tiles per workgroup; a tile whose rays all miss leaves
after the setup, which test_rays_that_miss covers), so there is no internal option to force."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_ref as SR  # noqa: E402
import volume_ref as VR  # noqa: E402

from waterlily_amd import render, scene, sim as S, volume  # noqa: E402
from waterlily_amd.scene import Camera  # noqa: E402

F64 = np.float64
DEV = "cuda"
SHAPE = (22, 19, 17)
NG = tuple(n + 2 for n in SHAPE)
SIZES = [(40, 24), (37, 19)]
CAMS = ["ortho", "persp", "inside"]
DTYPES = ["f32", "f64"]
CLIMS = (0.0, 1.0)
STRENGTH = 0.5                                                # chosen on the reference alone: see check_inputs
SEED = 4
T_MIN = 1.0 / 256.0
BG = (250, 240, 230, 255)
LIGHT = (0.3, -0.2, 0.9)


class FlowLike:
    N = NG


@functools.lru_cache(maxsize=None)
def host_field(dtype):
    """the dense host array with ghosts, already rounded to the flow's type: made once, read-only"""
    rng = np.random.default_rng(SEED)
    J = np.stack(np.meshgrid(*[np.arange(n, dtype=F64) for n in NG], indexing="ij"))
    c = np.array([12.3, 9.1, 8.4])
    r2 = sum((J[d] - 0.5 - c[d]) ** 2 for d in range(3))
    a = rng.uniform(0.0, 0.4, NG) + 0.8 * np.exp(-r2 / (2 * 5.0 ** 2))
    a[rng.uniform(size=NG) < 0.01] = np.nan
    a = np.asfortranarray(a.astype(np.float32 if dtype == "f32" else F64))
    a.setflags(write=False)
    return a


def camera(name, W, H):
    """(M, Minv, ds) at W x H with samples one cell length apart"""
    if name == "ortho":
        cam = Camera.fit(FlowLike, (1, 0.6, -0.5))
    elif name == "persp":
        cam = Camera.fit(FlowLike, (1, 0.6, -0.5), fov=40)
    else:
        cam = Camera.look_at((5.3, 4.2, 9.1), (20.0, 15.0, 5.0), fov=70, near=0.75, far=30.0)
    return cam, cam.matrix(W, H), cam.inverse(W, H), 1.0 / (cam.far - cam.near)


def sheet_camera(W, H):
    """the orthographic camera looking along +z under which SR.sheet's pixel coordinates cover the grid: world x = s_x 22 / W,
    y = s_y 19 / H, z = 24 z_ndc - 3 (the cell centres z = 0.5 .. 16.5 lie at depths 0.146 .. 0.8125); ds: one cell length"""
    A = np.diag([W / 22.0, H / 19.0, 1.0 / 24.0, 1.0])
    A[2, 3] = 3.0 / 24.0
    M = SR.ortho_screen(W, H) @ A
    return M, np.linalg.inv(M), np.linalg.inv(A), 1.0 / 24.0


def to_world(tris, Ainv):
    t = np.concatenate([tris, np.ones(tris.shape[:-1] + (1,))], axis=-1) @ Ainv.T
    return np.ascontiguousarray(t[..., :3])


_values = {}                                                   # the sampled values of a case's rays: they do not depend on the tables


def reference(what, W, H, dtype, levels, keys=None, rgba=None, box=None, strength=STRENGTH, kind="ramp", cam=None):
    """(out, acc, taken, early, nans) of volume_ref.march for the named camera; keys / rgba: a drawn depth buffer and its frame"""
    _, M, Minv, ds = camera(what, W, H) if cam is None else cam
    lo, hi = ((1, 1, 1), tuple(n - 1 for n in NG)) if box is None else box
    if keys is None:
        keys, rgba = SR.clear(W, H), np.zeros((H, W, 4), dtype=np.uint8)
    tag = (what, W, H, dtype, lo, hi, hash(tuple(map(tuple, keys))))
    cache = _values.setdefault(tag, {})
    return VR.march(host_field(dtype), Minv, ds, lo, hi, W, H, keys, rgba, BG, CLIMS[0], CLIMS[1], levels, render.colormap("RdBu"),
                    volume.opacity(kind, strength, 1.0), T_MIN, cache=cache)


@functools.lru_cache(maxsize=None)
def plain_case(what, W, H, dtype, levels):
    """the reference of a picture without surfaces: made once, read-only"""
    out = reference(what, W, H, dtype, levels)
    for a in out:
        a.setflags(write=False)
    return out


def check_inputs(taken, early, nans):
    """conditions on the reference alone, so that no test passes vacuously"""
    rays = taken > 0
    assert rays.sum() * 3 > rays.size, rays.sum()               # more than a third of the pixels take a sample
    share = early[rays].mean()
    assert 0.05 <= share <= 0.95, share                        # some rays end early at t_min = 1/256, some do not
    assert nans.sum() >= 1                                     # a taken sample is NaN


def flow_and_field(dtype):
    flow = S.Flow(SHAPE, (0.0, 0.0, 0.0), T=np.float32 if dtype == "f32" else F64)
    a = S.like(flow.p)
    assert a.stride(1) > NG[0]                                 # pitched rows
    S.upload(a, host_field(dtype))
    return flow, a


def keys_of(sc):
    return sc.keys.cpu().numpy().view(np.uint64).copy()


def raw_frame(sc):
    return sc._rgba.tensor(torch.uint8, sc.device)[:sc.Wi * sc.Hi * 4].view(sc.Hi, sc.Wi, 4).cpu().numpy().copy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("W,H", SIZES, ids=[f"{W}x{H}" for W, H in SIZES])
@pytest.mark.parametrize("what", CAMS)
def test_bit_for_bit(what, W, H, dtype):
    flow, a = flow_and_field(dtype)
    cam = camera(what, W, H)[0]
    sc = scene.Scene(flow, size=(W, H), ring=2)
    for levels in (0, 5):
        want, acc, taken, early, nans = plain_case(what, W, H, dtype, levels)
        check_inputs(taken, early, nans)
        scene.clear(sc)
        volume.add(sc, cam, flow, a, CLIMS, strength=STRENGTH, levels=levels, t_min=T_MIN, keep_acc=True)
        got = scene.frame(sc, background=BG).cpu().numpy()
        assert same_bits(sc.volume.acc.cpu().numpy(), acc)
        assert np.array_equal(got, want)
        assert np.all(keys_of(sc) == np.uint64(SR.NOTHING))


def test_inside_camera_starts_inside():
    """the camera inside the box: rays whose first sample is k = 0 (s_in = 0) exist, on the reference"""
    W, H = SIZES[0]
    _, M, Minv, ds = camera("inside", W, H)
    blo, bhi = [F64(0.5)] * 3, [F64(n - 2.5) for n in NG]
    n0 = sum(VR.ray(Minv, i, j, W, H, blo, bhi, SR.NOTHING).s_in == 0.0 for j in range(H) for i in range(W))
    assert n0 * 2 > W * H


@functools.lru_cache(maxsize=None)
def sheet_keys(W, H, front):
    """(tris in world coordinates, the reference keys) of the jittered sheet: tilted through the middle of the box, or flat in
    front of all of it"""
    M, _, Ainv, _ = sheet_camera(W, H)
    zfun = (lambda x, y: 0.05) if front else (lambda x, y: 0.3 + 0.35 * x / W)
    tris = to_world(SR.sheet(W, H, zfun=zfun), Ainv)
    keys = SR.clear(W, H)
    SR.draw(keys, M, tris, W, H)
    return tris, keys


@pytest.mark.parametrize("W,H,dtype", [(40, 24, "f32"), (37, 19, "f64")])
def test_with_surfaces(W, H, dtype):
    flow, a = flow_and_field(dtype)
    M, Minv, _, ds = sheet_camera(W, H)
    sc = scene.Scene(flow, size=(W, H), ring=2)
    for front in (False, True):
        tris, keys = sheet_keys(W, H, front)
        tt = torch.from_numpy(tris).to(DEV)
        scene.clear(sc)
        scene.draw(sc, M, tt, light=LIGHT, color=(90, 160, 60, 255))
        plain = scene.frame(sc, background=BG).cpu().numpy().copy()
        assert np.array_equal(keys_of(sc), SR.as_array(keys))
        shaded = raw_frame(sc)                                 # the frame under the cloud (its lit channels: test_scene_gpu.py)
        volume.add(sc, M, flow, a, CLIMS, strength=STRENGTH, ds=ds, keep_acc=True)
        got = scene.frame(sc, background=BG).cpu().numpy()
        assert np.array_equal(keys_of(sc), SR.as_array(keys))  # the volume pass leaves the keys alone
        want, acc, taken, early, nans = reference("sheet" + str(front), W, H, dtype, 0, keys=keys, rgba=shaded, cam=(None, M, Minv, ds))
        assert same_bits(sc.volume.acc.cpu().numpy(), acc) and np.array_equal(got, want)
        covered = SR.as_array(keys) != np.uint64(SR.NOTHING)
        assert covered.all()                                   # (the sheet reaches beyond the viewport)
        if front:                                              # the sheet hides the whole box: the picture without a volume
            assert taken.sum() == 0 and np.array_equal(got, plain)
        else:                                                  # the cloud in front of the sheet shows, and the sheet cuts rays short
            free = reference("sheet-free", W, H, dtype, 0, cam=(None, M, Minv, ds))[2]
            assert (taken > 0).sum() * 3 > W * H and (taken < free).sum() * 3 > W * H and not np.array_equal(got, plain)


def test_ssaa_and_the_plain_path():
    W, H, dtype = 40, 24, "f32"                               # the internal size; the frame is 20 x 12
    flow, a = flow_and_field(dtype)
    cam = camera("persp", W, H)[0]
    sc = scene.Scene(flow, size=(W // 2, H // 2), ssaa=2, ring=2)
    scene.clear(sc)
    volume.add(sc, cam, flow, a, CLIMS, strength=STRENGTH, t_min=T_MIN)
    got = scene.frame(sc, background=BG).cpu().numpy()
    want = plain_case("persp", W, H, dtype, 0)[0]
    assert got.shape == (H // 2, W // 2, 4) and np.array_equal(got, VR.average(want, 2))
    assert np.array_equal(raw_frame(sc), want)
    # nothing queued: the calls of a picture without a volume, against scene_ref.resolve
    M, _, Ainv, _ = sheet_camera(W, H)
    tris = to_world(SR.sheet(W, H, n=5, m=4, margin=-6.0), Ainv)                     # (a sheet that leaves a rim of background)
    keys = SR.clear(W, H)
    SR.draw(keys, M, tris, W, H)
    scene.clear(sc)
    assert sc.volume is None
    scene.draw(sc, M, torch.from_numpy(tris).to(DEV), light=LIGHT)
    got = scene.frame(sc, background=BG).cpu().numpy()
    hit = SR.as_array(keys) != np.uint64(SR.NOTHING)
    assert 100 < hit.sum() < W * H - 100 and np.array_equal(keys_of(sc), SR.as_array(keys))
    assert np.array_equal(got, SR.resolve(np.where(hit[..., None], raw_frame(sc), 0).astype(np.uint8), keys, 2, BG))


def test_rays_that_miss():
    """a volume whose box lies outside the view changes no byte of the frame: every tile leaves after the setup"""
    W, H, dtype = 37, 19, "f32"
    flow, a = flow_and_field(dtype)
    away = Camera.look_at((40.0, 30.0, 20.0), (80.0, 50.0, 30.0), fov=40, near=1.0, far=60.0)
    c = away.eye + 20.0 * away.forward                         # a triangle in the middle of that view
    tris = np.ascontiguousarray(np.array([[c - 4.0 * away.right, c + 4.0 * away.right, c + 3.0 * away.upv]], dtype=F64))
    sc = scene.Scene(flow, size=(W, H), ring=2)
    frames = []
    for with_volume in (False, True):
        scene.clear(sc)
        scene.draw(sc, away, torch.from_numpy(tris).to(DEV))
        if with_volume:
            volume.add(sc, away, flow, a, CLIMS, strength=STRENGTH, keep_acc=True)
        frames.append(scene.frame(sc, background=BG).cpu().numpy().copy())
    acc = sc.volume.acc.cpu().numpy()
    assert np.all(acc == np.array([0.0, 0.0, 0.0, 1.0]))
    assert np.array_equal(frames[0], frames[1]) and np.any(frames[0] != np.array(BG, dtype=np.uint8))
    assert np.any(np.all(frames[0] == np.array(BG, dtype=np.uint8), axis=-1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_box_on_the_ghost_planes(dtype):
    """lo = 0: the box's lower planes are the centres of the ghost cells, the array's first planes; a sample a last bit beyond
    them has a weighted corner outside the array and is NaN on both sides"""
    W, H = 37, 19
    flow, a = flow_and_field(dtype)
    box = ((0, 0, 0), tuple(n - 1 for n in NG))
    small = ((3, 2, 5), (14, 4, 15))                           # ... and a small one: two cells in y
    sc = scene.Scene(flow, size=(W, H), ring=2)
    for what, b in (("ortho", box), ("inside", box), ("persp", small)):
        want, acc, taken, _, _ = reference(what, W, H, dtype, 0, box=b)
        assert (taken > 0).sum() > 15
        scene.clear(sc)
        volume.add(sc, camera(what, W, H)[0], flow, a, CLIMS, strength=STRENGTH, box=b, t_min=T_MIN, keep_acc=True)
        got = scene.frame(sc, background=BG).cpu().numpy()
        assert same_bits(sc.volume.acc.cpu().numpy(), acc) and np.array_equal(got, want)


def test_tables_and_zero_opacity():
    """the "abs" table under RdBu has entries that are exactly 0 only with strength 0 at its middle; a table of the caller's with
    a run of zeros exercises the skip before the colour fetch: the same bits as the reference, which skips nothing"""
    W, H, dtype = 40, 24, "f64"
    flow, a = flow_and_field(dtype)
    table = np.where(np.arange(256) < 96, 0.0, 0.3)
    want, acc, taken, early, _ = reference("ortho", W, H, dtype, 0, kind=table, strength=0.0)
    assert (taken > 0).sum() * 3 > W * H and early.any()
    sc = scene.Scene(flow, size=(W, H), ring=2)
    scene.clear(sc)
    volume.add(sc, camera("ortho", W, H)[0], flow, a, CLIMS, opacity=table, t_min=T_MIN, keep_acc=True)
    got = scene.frame(sc, background=BG).cpu().numpy()
    assert same_bits(sc.volume.acc.cpu().numpy(), acc) and np.array_equal(got, want)


def test_metric_and_record():
    """volume.metric fills the scene's scratch field with |ω| and queues it; record() and the ring work as without a volume"""
    flow = S.Flow(SHAPE, (1.0, 0.0, 0.0), T=np.float32)

    class Sim:
        pass
    sim = Sim()
    sim.flow = flow
    rng = np.random.default_rng(1)
    S.upload(flow.u, np.asfortranarray(rng.uniform(-1.0, 1.0, NG + (3,)).astype(np.float32)))
    W, H = 40, 24
    cam = camera("ortho", W, H)[0]
    sc = scene.Scene(flow, size=(W, H), ring=2)
    scene.clear(sc)
    volume.metric(sc, cam, sim, "omega_mag", clims=(0.0, 3.0), strength=0.3, keep_acc=True)
    scene.record(sc, background=BG)
    frames = scene.drain(sc)
    om = S.like(flow.p)
    S.metric(om, "omega_mag", flow.u)
    assert torch.equal(sc._vfield, om)
    host = S.to_host(om)
    _, M, Minv, ds = camera("ortho", W, H)
    want, acc, taken, _, _ = VR.march(host, Minv, ds, (1, 1, 1), tuple(n - 1 for n in NG), W, H, SR.clear(W, H), np.zeros((H, W, 4), np.uint8), BG,
                                      0.0, 3.0, 0, render.colormap("RdBu"), volume.opacity("ramp", 0.3, 1.0), 1.0 / 256.0)
    assert (taken > 0).sum() * 3 > W * H
    assert same_bits(sc.volume.acc.cpu().numpy(), acc) and len(frames) == 1 and np.array_equal(frames[0], want)


def test_python_refusals():
    flow, a = flow_and_field("f32")
    W, H = 40, 24
    cam = camera("ortho", W, H)[0]
    sc = scene.Scene(flow, size=(W, H), ring=2)
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, CLIMS)                    # no clear()
    scene.clear(sc)
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, None)                     # clims are required
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, (1.0, 1.0))
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, CLIMS, step=0.0)
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, CLIMS, step=1e-6)         # more than 2^20 steps
    with pytest.raises(ValueError):
        volume.add(sc, cam.matrix(W, H), flow, a, CLIMS)       # a matrix without ds
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a.cpu(), CLIMS)              # another device (and another layout)
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, flow.u, CLIMS)               # not a scalar field
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, CLIMS, box=((1, 1, 1), (5, 2, 5)))            # an extent below 2
    flow2 = S.Flow((16, 12), (0.0, 0.0), T=np.float32)
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow2, S.like(flow2.p), CLIMS)     # a 2-D flow
    assert sc.volume is None
    volume.add(sc, cam, flow, a, CLIMS)
    with pytest.raises(ValueError):
        volume.add(sc, cam, flow, a, CLIMS)                    # a second volume
    scene.clear(sc)
    assert sc.volume is None
