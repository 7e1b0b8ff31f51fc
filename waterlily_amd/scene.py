"""3-D pictures made on the device: the triangles of an isosurface (iso.extract, iso.lambda2) and of a posed MeshBody drawn
through a camera into a depth buffer, coloured by a second field, lit, anti-aliased and recorded into (A)PNG files -- a λ₂
movie of a wake without a volume, a copy of the triangles to the host or a plotting package.

    cam = Camera.fit(sim.flow, direction=(1, 1, -0.5), fov=30, aspect=4 / 3)     # or Camera.look_at(eye, target, width=...)
    sc = Scene(sim.flow, size=(1024, 768), ssaa=2, ring=8)      # owns the keys, the RGBA frames, the pinned host ring
    clear(sc)
    draw(sc, cam, tri, val, clims=(0, 0.5))                     # the surface, coloured by its vertex values
    draw(sc, cam, body_triangles(sim.body, S.time(sim.flow)))   # the body, solid grey, into the same depth buffer
    rgba = frame(sc)                                            # device view [H, W, 4] (uint8)
    wake(sc, isf, sim, -0.01, cam, clims=(0, 0.5)); record(sc)  # the one-call twin of iso.lambda2, once per step
    save(sc, "wake.png", fps=20)

The rasteriser and its contract -- the vertex stage, the snap to 8 sub-pixel bits, the top-left rule, the 64-bit key
(depth << 32 | triangle id) and its atomic minimum, the two paths, the shade and resolve arithmetic -- are in include/wlhip.h
(wl_scene_*) and csrc/wl_scene.h; tests/scene_ref.py restates them with numpy scalars and Python integers and gets the same keys
bit for bit.  The picture is a function of the triangles and the camera alone: no launch shape, triangle order or path shows.
THERE IS NO CLIPPING: a triangle with a vertex behind the eye, or outside the near and far planes, is dropped whole.

Nothing here synchronises with the device except (1) `clims=None` with vertex values, which reads their minimum and maximum
once per draw -- give clims for a recording -- and (2) record() on a full ring, which waits for the oldest frame's copy.  The
view frame() returns aliases the object's buffer: the next frame() overwrites it.  On a decomposed flow a Scene takes
triangles only: draw what iso.gather returned on rank 0; nothing distributed is built.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _lib
from . import render
from . import sim as S
from ._lib import check
from ._readout import DevBuf
from .mesh import MeshBody
from .render import drain, write_apng, write_png  # noqa: F401  (drain(sc): every recorded frame, as for a Renderer)

MAX_DRAWS = 8
MAX_SIZE = 4096


def _unit(v, what: str) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64).reshape(3)
    n = float(np.sqrt(np.dot(v, v)))
    if not (np.isfinite(n) and n > 0):
        raise ValueError(f"Camera: {what} must be a finite vector that is not zero")
    return v / n


class Camera:
    """A view: where the eye is, where it looks, and a perspective (fov: the horizontal field of view in degrees) or orthographic
    (width: the world length the image's width shows) projection between the planes at distances near < far along the view.
    matrix(W, H) is the row-major 4x4 Float64 M of wl_scene_draw: clip = M (x, y, z, 1), z_ndc = 0 at near and 1 at far."""

    def __init__(self, eye, forward, right, upv, fov, width, near, far):
        self.eye, self.forward, self.right, self.upv = eye, forward, right, upv
        self.fov, self.width, self.near, self.far = fov, width, float(near), float(far)

    @classmethod
    def look_at(cls, eye, target, up=(0, 0, 1), fov=None, width=None, near=None, far=None) -> "Camera":
        """The camera at `eye` looking at `target`.  Exactly one of fov (perspective) and width (orthographic).  near, far:
        default 1/100 and 100 times the distance to the target (orthographic: 0 and twice the distance)."""
        if (fov is None) == (width is None):
            raise ValueError("Camera: give exactly one of fov (perspective) and width (orthographic)")
        eye = np.asarray(eye, dtype=np.float64).reshape(3)
        d = np.asarray(target, dtype=np.float64).reshape(3) - eye
        dist = float(np.sqrt(np.dot(d, d)))
        f = _unit(d, "target - eye")
        r = np.cross(f, np.asarray(up, dtype=np.float64).reshape(3))
        if not np.dot(r, r) > 1e-24 * np.dot(up, up):
            raise ValueError("Camera: up is parallel to the view")
        r = _unit(r, "up")
        u = np.cross(r, f)
        if fov is not None:
            if not 0 < float(fov) < 180:
                raise ValueError("Camera: fov lies in (0, 180) degrees")
            near = 0.01 * dist if near is None else near
            far = 100.0 * dist if far is None else far
            if not float(near) > 0:
                raise ValueError("Camera: a perspective view needs near > 0")
        else:
            if not float(width) > 0:
                raise ValueError("Camera: width must be > 0")
            near = 0.0 if near is None else near
            far = 2.0 * dist if far is None else far
        if not (np.isfinite(near) and np.isfinite(far) and float(near) < float(far)):
            raise ValueError("Camera: need finite near < far")
        return cls(eye, f, r, u, None if fov is None else float(fov), None if width is None else float(width), near, far)

    @classmethod
    def fit(cls, flow, direction, up=(0, 0, 1), fov=None, aspect: float = 1.0, margin: float = 0.05) -> "Camera":
        """The camera that looks along `direction` at the centre of the grid's box 0 <= x_d <= N_d - 2 (the frame x = J - 0.5)
        and shows all of it: orthographic unless fov is given; aspect = W / H of the scene it is for, so that the box fits
        vertically too.  near and far: the extent of the box's bounding sphere along the view plus `margin` of its radius."""
        n = np.asarray([int(x) for x in flow.N], dtype=np.float64) - 2.0
        if len(n) != 3:
            raise ValueError("Camera: a 3-D flow is needed")
        centre, R = 0.5 * n, 0.5 * float(np.sqrt(np.dot(n, n))) * (1.0 + float(margin))
        f = _unit(direction, "direction")
        a = max(float(aspect), 1e-6)
        if fov is None:
            dist, kw = 2.0 * R, dict(width=2.0 * R * max(1.0, a))
        else:
            th = np.tan(np.radians(float(fov)) / 2.0)
            dist, kw = R / np.sin(np.arctan(min(th, th / a))), dict(fov=fov)
        return cls.look_at(centre - dist * f, centre, up=up, near=dist - R, far=dist + R, **kw)

    def matrix(self, W: int, H: int) -> np.ndarray:
        a = float(W) / float(H)
        V = np.zeros((4, 4), dtype=np.float64)                 # view: (right, up, depth along the view, 1)
        for k, ax in enumerate((self.right, self.upv, self.forward)):
            V[k, :3] = ax
            V[k, 3] = -np.dot(ax, self.eye)
        V[3, 3] = 1.0
        P = np.zeros((4, 4), dtype=np.float64)
        n, f = self.near, self.far
        if self.fov is not None:
            th = np.tan(np.radians(self.fov) / 2.0)
            P[0, 0], P[1, 1] = 1.0 / th, a / th
            P[2, 2], P[2, 3] = f / (f - n), -f * n / (f - n)
            P[3, 2] = 1.0
        else:
            P[0, 0], P[1, 1] = 2.0 / self.width, 2.0 * a / self.width
            P[2, 2], P[2, 3] = 1.0 / (f - n), -n / (f - n)
            P[3, 3] = 1.0
        return np.ascontiguousarray(P @ V)

    def inverse(self, W: int, H: int) -> np.ndarray:
        """the inverse of matrix(W, H): what wl_scene_volume makes its rays from"""
        return np.linalg.inv(self.matrix(W, H))


def _device(d) -> torch.device:
    """a torch device with its index ("cuda" is the current one), so that it compares equal to a tensor's"""
    d = torch.device(d)
    return torch.device("cuda", torch.cuda.current_device()) if (d.type == "cuda" and d.index is None) else d


class _Draw:
    def __init__(self, **kw):
        self.__dict__.update(kw)


class Scene:
    """The buffers of one picture pipeline of W x H pixels, made once: the uint64 keys and the RGBA frame at (W ssaa) x (H ssaa),
    the resolved frame, the scratch of wl_scene_draw (from the library's allocator; it grows with the largest draw), `ring` RGBA
    frames on the device with their pinned host twins and one event each (the ring of a Renderer: record() waits only when it
    is full).  frames: the host copies drained so far, oldest first.  flow_or_device: a Flow (its device is used) or a torch
    device.  On a decomposed flow a Scene draws triangles only, on the rank that holds them (iso.gather)."""

    def __init__(self, flow_or_device, size=(640, 480), ssaa: int = 1, ring: int = 8):
        W, H = (int(x) for x in size)
        ssaa = int(ssaa)
        if ssaa not in (1, 2, 4):
            raise ValueError("Scene: ssaa is 1, 2 or 4")
        if int(ring) < 1:
            raise ValueError("Scene: ring must be >= 1")
        if not (1 <= W and 1 <= H and W * ssaa <= MAX_SIZE and H * ssaa <= MAX_SIZE):
            raise ValueError(f"Scene: size times ssaa must lie in 1..{MAX_SIZE}")
        self.device = _device(getattr(flow_or_device, "device", flow_or_device))
        self.W, self.H, self.ssaa, self.ring = W, H, ssaa, int(ring)
        self.Wi, self.Hi = W * ssaa, H * ssaa
        self._key = DevBuf(8 * self.Wi * self.Hi)
        self._rgba = DevBuf(4 * self.Wi * self.Hi)
        self._out = DevBuf(4 * W * H)
        self._scratch = DevBuf(16)
        nb = W * H * 4
        self.ring_dev = torch.zeros((self.ring, nb), dtype=torch.uint8, device=self.device)
        self.ring_host = torch.zeros((self.ring, nb), dtype=torch.uint8).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(self.ring)]
        self.shapes: List[Optional[tuple]] = [None] * self.ring
        self.head = 0
        self.tail = 0
        self.frames: List[np.ndarray] = []
        self.draws: List[_Draw] = []
        self.volume = None                                     # the picture's queued volume (waterlily_amd.volume.add)
        self._vfield = None                                    # volume.metric's scratch scalar field
        self._lut = {}
        self._cleared = False

    def lut(self, cmap) -> torch.Tensor:
        key = cmap if isinstance(cmap, str) else render.colormap(cmap).tobytes()
        if key not in self._lut:
            self._lut[key] = torch.from_numpy(render.colormap(cmap).copy()).to(self.device)
        return self._lut[key]

    @property
    def keys(self) -> torch.Tensor:
        """the depth buffer: a device view [H ssaa, W ssaa] of int64 holding the uint64 keys' bits (-1: nothing)"""
        return self._key.tensor(torch.int64, self.device)[:self.Wi * self.Hi].view(self.Hi, self.Wi)


def _u8(c):
    return (C.c_uint8 * 4)(*[int(x) for x in c])


def _m16(M: np.ndarray):
    return (C.c_double * 16)(*[float(x) for x in np.asarray(M, dtype=np.float64).reshape(16)])


def clear(sc: Scene) -> None:
    """Start a picture: every key becomes "nothing" and the list of draws is emptied."""
    check(_lib.lib().wl_scene_clear(C.c_void_p(sc._key.ptr), sc.Wi, sc.Hi))
    sc.draws = []
    sc.volume = None
    sc._cleared = True


def draw(sc: Scene, cam, tri: torch.Tensor, val: Optional[torch.Tensor] = None, clims=None, cmap="RdBu", levels: int = 0,
         color=(200, 200, 200, 255), ambient: float = 0.3, light=None, large_px: int = 64, nan_rgba=(0, 0, 0, 0)) -> None:
    """Draw the triangles tri [nt, 3, 3] (Float64, contiguous, on the scene's device: what iso.extract and body_triangles
    return) into the depth buffer through `cam` (a Camera, or a 4x4 matrix for the scene's internal size).  val [nt, 3]: vertex
    values, shown through `cmap` between clims (None: their minimum and maximum are read from the device, the ONE synchronising
    path; a constant gets +-1 around it) in `levels` bands (0: continuous); without val the triangles have the solid `color`.
    light: a direction in world space (None: a headlight along the view); ambient: the share of the colour a face edge-on to
    the light keeps.  large_px: the bounding-box size in pixels above which a triangle gets a wavefront instead of a lane.
    Up to 8 draws share one depth buffer; the object keeps tri and val alive until the next clear()."""
    if not sc._cleared:
        raise ValueError("Scene: clear() starts a picture")
    if len(sc.draws) >= MAX_DRAWS:
        raise ValueError(f"Scene: at most {MAX_DRAWS} draws share one depth buffer")
    ok = lambda a, shape: (isinstance(a, torch.Tensor) and a.dtype == torch.float64 and a.device == sc.device and a.is_contiguous()
                           and a.dim() == len(shape) and tuple(a.shape[1:]) == shape[1:])
    if not ok(tri, (0, 3, 3)):
        raise ValueError("Scene: tri must be a contiguous Float64 [nt, 3, 3] tensor on the scene's device")
    nt = int(tri.shape[0])
    if val is not None and not (ok(val, (0, 3)) and int(val.shape[0]) == nt):
        raise ValueError("Scene: val must be a contiguous Float64 [nt, 3] tensor on the scene's device")
    M = cam.matrix(sc.Wi, sc.Hi) if isinstance(cam, Camera) else np.asarray(cam, dtype=np.float64).reshape(4, 4)
    if light is None:
        if not isinstance(cam, Camera):
            raise ValueError("Scene: a camera given as a matrix needs a light direction")
        light = cam.forward
    light = _unit(light, "light")
    base = sum(d.nt for d in sc.draws)
    if val is not None and clims is None:
        fin = val[~torch.isnan(val)]
        lo, hi = (float(fin.min().item()), float(fin.max().item())) if fin.numel() else (0.0, 0.0)
        clims = (lo, hi) if (np.isfinite(lo) and np.isfinite(hi) and lo < hi) else (lo - 1.0, lo + 1.0) if np.isfinite(lo) else (-1.0, 1.0)
    need = C.c_int64()
    check(_lib.lib().wl_scene_scratch(nt, C.byref(need)))
    if sc._scratch.nbytes < need.value:
        sc._scratch = DevBuf(need.value)                      # (wl_free waits for the device: the old block outlives its last use)
    d = _Draw(nt=nt, base=base, tri=tri, val=val, M=_m16(M), clims=clims, lut=sc.lut(cmap) if val is not None else None, levels=int(levels),
              color=_u8(color), ambient=float(ambient), light=_lib.d3(light), nan_rgba=_u8(nan_rgba))
    check(_lib.lib().wl_scene_draw(C.c_void_p(sc._key.ptr), sc.Wi, sc.Hi, d.M, S._ptr(tri) if nt else None, nt, base, int(large_px),
                                   C.c_void_p(sc._scratch.ptr), sc._scratch.nbytes))
    sc.draws.append(d)


def frame(sc: Scene, background=(255, 255, 255, 255), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Shade every draw's pixels, fill the rest with `background`, average ssaa x ssaa blocks: the RGBA uint8 device view
    [H, W, 4] of `out` (default: the object's frame, which the next frame() overwrites).  A queued volume (waterlily_amd.volume.add)
    is composited over the shaded frame and the background before the average."""
    if not sc._cleared:
        raise ValueError("Scene: clear() starts a picture")
    L = _lib.lib()
    for d in sc.draws:
        v = d.val is not None
        check(L.wl_scene_shade(C.c_void_p(sc._key.ptr), sc.Wi, sc.Hi, d.base, d.nt, S._ptr(d.tri) if d.nt else None, S._ptr(d.val) if v else None,
                               d.M, float(d.clims[0]) if v else 0.0, float(d.clims[1]) if v else 1.0, d.levels, S._ptr(d.lut) if v else None,
                               d.color, d.light, d.ambient, d.nan_rgba, C.c_void_p(sc._rgba.ptr)))
    n = sc.W * sc.H * 4
    dst = sc._out.tensor(torch.uint8, sc.device) if out is None else out
    if dst.numel() < n or dst.dtype != torch.uint8 or not dst.is_contiguous():
        raise ValueError("Scene: the output must be a contiguous uint8 tensor of H*W*4 elements or more")
    if sc.volume is not None:                                  # the cloud over the shaded frame and the background, then the plain average
        from . import volume
        volume.run(sc, _u8(background))
        check(L.wl_scene_average(C.c_void_p(sc._rgba.ptr), sc.Wi, sc.Hi, sc.ssaa, S._ptr(dst)))
    else:
        check(L.wl_scene_resolve(C.c_void_p(sc._rgba.ptr), sc.Wi, sc.Hi, C.c_void_p(sc._key.ptr), sc.ssaa, _u8(background), S._ptr(dst)))
    return dst.reshape(-1)[:n].view(sc.H, sc.W, 4)


def record(sc: Scene, background=(255, 255, 255, 255)) -> None:
    """frame() into the next slot of the ring, and the start of its copy into the slot's pinned host twin behind an event.  It
    waits for nothing unless the ring is full: then the oldest frame is drained to sc.frames first."""
    if sc.head - sc.tail >= sc.ring:
        render.drain_one(sc)
    slot = sc.head % sc.ring
    rgba = frame(sc, background, out=sc.ring_dev[slot])
    sc.ring_host[slot].copy_(sc.ring_dev[slot], non_blocking=True)
    sc.events[slot].record()
    sc.shapes[slot] = (int(rgba.shape[0]), int(rgba.shape[1]))
    sc.head += 1


def save(sc: Scene, path, fps: float = 10.0) -> None:
    """Drain the ring and write the recorded frames: a PNG for one frame, an APNG for several (render.write_apng).  The frame
    list is kept; clear sc.frames to start another recording."""
    frames = drain(sc)
    if not frames:
        raise ValueError("Scene: nothing was recorded")
    write_apng(path, frames, fps=fps)


def body_triangles(body: MeshBody, t: float, device=None) -> torch.Tensor:
    """The triangles of a MeshBody posed at time t (the flow's time, S.time(flow)) as a device tensor [nt, 3, 3] (Float64), in
    the frame of the isosurface: x = Ainv (xi - b), the pose surface.write_vtp writes.  The vertices go to the device once; a
    pose is nine multiplications and six additions per vertex there.  device: default cuda (the current device)."""
    if not isinstance(body, MeshBody):
        raise TypeError(f"Scene: body_triangles needs a MeshBody, not {type(body).__name__}")
    dev = _device("cuda" if device is None else device)
    cache = getattr(body, "_scene_dev", None)
    if cache is None or cache[0].device != dev:
        cache = (torch.from_numpy(np.ascontiguousarray(body.vertices, dtype=np.float64)).to(dev),
                 torch.from_numpy(np.ascontiguousarray(body.triangles, dtype=np.int64)).to(dev))
        body._scene_dev = cache
    xi, idx = cache
    if body.amap is None:
        return xi[idx].contiguous()
    _, b, _, _, Ai, _ = body.coeffs(float(t))
    p = [xi[:, k] - float(b[k]) for k in range(3)]
    x = torch.stack([(p[0] * float(Ai[d, 0]) + p[1] * float(Ai[d, 1])) + p[2] * float(Ai[d, 2]) for d in range(3)], dim=1)
    return x[idx].contiguous()


def wake(sc: Scene, isf, sim, c: float, cam, color="omega_mag", clims=None, body_color=(200, 200, 200, 255), background=(255, 255, 255, 255),
         **kw) -> torch.Tensor:
    """The one-call twin of iso.lambda2: clear, draw the λ₂ = c surface of sim.flow coloured by `color` (iso.lambda2's: None,
    "omega_mag", "pressure" or a field), draw the body when it is a MeshBody, and return frame().  kw: draw()'s arguments
    (cmap, levels, ambient, light, large_px).  Give clims: None reads them from the device, per call."""
    from . import iso
    tri, val = iso.lambda2(isf, sim, c, color=color)
    clear(sc)
    draw(sc, cam, tri, val, clims=clims, **kw)
    body = getattr(sim, "body", None)
    if isinstance(body, MeshBody):
        shared = {k: v for k, v in kw.items() if k in ("ambient", "light", "large_px")}
        draw(sc, cam, body_triangles(body, S.time(sim.flow), sc.device), color=body_color, **shared)
    return frame(sc, background)
