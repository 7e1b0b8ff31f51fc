"""Pictures of the flow made on the device: slices and projections of a field or a Metrics.jl metric as images, shaded through a
colour map, recorded into (A)PNG files -- the twin of `flood`, `body_plot!` and `sim_gif!` (ext/WaterLilyPlotsExt.jl:17-52)
without filling a volume, copying it to the host or an external plotting tool.

    r = Renderer(sim.flow, ring=8, zoom=2)            # owns the image, the mask, the RGBA ring and the pinned host slots
    img = project(r, sim.flow.u, "lambda2", mode="min", axis=1)      # device view [ny, nx] (Float64) of one projection
    img = project(r, sim.flow.p, "scalar", mode="slice", axis=2, index=40)
    rgba = image(r, sim, "omega_mag", mode="max", axis=2, clims=(0, 0.5))   # device view [ny*zoom, nx*zoom, 4] (uint8)
    record(r, sim, "curl", clims=(-5, 5))             # one frame into the ring; its copy to the host runs behind an event
    save(r, "wake.png")                               # a PNG for one frame, an APNG for several
    sim_gif(sim, "wake.png", duration=10, step=0.25, clims=(-5, 5), plotbody=True)

The two kernels and their contract -- kinds, modes, the order of every reduction, the box, the z-slab rules, the shade
arithmetic -- are in include/wlhip.h (wl_render_project, wl_render_shade) and csrc/wl_render.h; tests/render_ref.py restates
both with numpy loops and reproduces every bit and byte.  An image is indexed [b, a]: a runs along the lower of the two axes
that are not reduced.  The views returned by project / image alias the object's buffers: the next call overwrites them.

Nothing here synchronises with the device except (1) `clims=None`, which reads the image's minimum and maximum once per call --
give clims for a recording -- and (2) record() on a full ring, which waits for the oldest frame's copy before it reuses the slot.
On z-slabs every rank renders the planes it owns and gather() combines the parts on rank 0.
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import _series
from . import sim as S
from ._lib import check
from ._readout import R_CENTRE, R_METRIC, R_SCALAR, R_UCOMP  # noqa: F401  (the kinds' numbers, under this module's name too)

# ColorBrewer RdBu, 11 classes (red = low, blue = high)
_RDBU11 = ((103, 0, 31), (178, 24, 43), (214, 96, 77), (244, 165, 130), (253, 219, 199), (247, 247, 247), (209, 229, 240),
           (146, 197, 222), (67, 147, 195), (33, 102, 172), (5, 48, 97))


def colormap(cmap="RdBu") -> np.ndarray:
    """A (256, 4) uint8 table: "RdBu" (the 11 ColorBrewer anchors interpolated linearly; entries 0 and 255 are the end anchors),
    "gray" (black to white), or any (256, 4) uint8 array."""
    if isinstance(cmap, str):
        if cmap == "RdBu":
            a = np.asarray(_RDBU11, dtype=np.float64)
            x = np.arange(256, dtype=np.float64) * (len(a) - 1) / 255.0
            k = np.minimum(np.floor(x).astype(np.int64), len(a) - 2)
            rgb = a[k] + (x - k)[:, None] * (a[k + 1] - a[k])
            rgb = np.floor(rgb + 0.5)
        elif cmap == "gray":
            rgb = np.repeat(np.arange(256, dtype=np.float64)[:, None], 3, axis=1)
        else:
            raise ValueError(f'Renderer: cmap must be "RdBu", "gray" or a (256, 4) uint8 array, not {cmap!r}')
        return np.concatenate([rgb.astype(np.uint8), np.full((256, 1), 255, dtype=np.uint8)], axis=1)
    t = np.ascontiguousarray(cmap)
    if t.shape != (256, 4) or t.dtype != np.uint8:
        raise ValueError("Renderer: a colour table must be a (256, 4) uint8 array")
    return t


class Renderer:
    """The buffers of one picture pipeline, sized for the largest face of the flow's grid (ghost cells included) and made once:
    img, mask (Float64), `ring` RGBA frames on the device with their pinned host twins and one event each.  frames: the host
    copies record() has drained so far, oldest first."""

    def __init__(self, flow, ring: int = 8, zoom: int = 1):
        if int(ring) < 1 or int(zoom) < 1:
            raise ValueError("Renderer: ring and zoom must be >= 1")
        self.flow, self.ring, self.zoom = flow, int(ring), int(zoom)
        n = tuple(int(x) for x in flow.N)
        self.maxpix = n[0] * n[1] if flow.D == 2 else max(n[0] * n[1], n[0] * n[2], n[1] * n[2])
        dev = flow.device
        self.img = torch.zeros(self.maxpix, dtype=torch.float64, device=dev)
        self.mask = torch.zeros(self.maxpix, dtype=torch.float64, device=dev)
        nb = self.maxpix * self.zoom * self.zoom * 4
        self.rgba = torch.zeros(nb, dtype=torch.uint8, device=dev)               # image()'s own frame
        self.ring_dev = torch.zeros((self.ring, nb), dtype=torch.uint8, device=dev)
        self.ring_host = torch.zeros((self.ring, nb), dtype=torch.uint8).pin_memory()
        self.events = [torch.cuda.Event() for _ in range(self.ring)]
        self.shapes: List[Optional[tuple]] = [None] * self.ring
        self.head = 0                                                            # frames recorded so far
        self.tail = 0                                                            # frames drained so far
        self.frames: List[np.ndarray] = []
        self._lut = {}

    def lut(self, cmap) -> torch.Tensor:
        key = cmap if isinstance(cmap, str) else colormap(cmap).tobytes()
        if key not in self._lut:
            self._lut[key] = torch.from_numpy(colormap(cmap).copy()).to(self.flow.device)
        return self._lut[key]


def project(r: Renderer, f: torch.Tensor, kind="scalar", mode: str = "slice", axis: int = 2, index: Optional[int] = None, box=None,
            i: int = 0, par=None, par2=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The image of `f` reduced along `axis` inside `box` = (lo, hi) (default: inside()): a device view [nb, na] of Float64.
    kind: "scalar" (f a scalar field), "ucomp" / "centre" (component i of a vector field, as stored / averaged to the cell centre),
    or a metric of f = u: "ke", "curl", "omega_mag", "omega_theta", "lambda2" (i, par, par2 as waterlily_amd.sim.metric).
    mode: "slice" (the plane `index` along `axis`; a 2-D field needs none), "max", "min", "absmax" (the signed value of largest
    magnitude), "sum", "mean".  out: the Float64 buffer the image goes to (default: the object's image; image() renders the body mask into
    the object's second one).  On a z-slab the view holds this rank's rows (axis 0, 1) or its partial image (axis 2)."""
    D = r.flow.D
    v = R.Value(kind, i, par, par2)
    g = R.field_grid(r.flow, f, v.kind != R_SCALAR, "Renderer")
    axis = int(axis)
    if D == 2 and axis != 2:
        raise ValueError("Renderer: a 2-D flow is viewed along axis 2")
    if axis < 0 or axis > 2:
        raise ValueError("Renderer: axis must be 0, 1 or 2")
    lo, hi = ([int(x) for x in side] for side in (R.inside(r.flow.N) if box is None else (box[0], box[1])))      # (N: undecomposed)
    if mode == "slice":
        if D == 3:
            if index is None:
                raise ValueError('Renderer: mode="slice" needs index, the plane along the axis')
            lo[axis], hi[axis] = int(index), int(index) + 1
        m = R.MODE["max"]
    else:
        m = R.MODE[mode]
    a, b = (1 if axis == 0 else 0), (1 if axis == 2 else 2)
    na, nb = hi[a] - lo[a], hi[b] - lo[b]
    if na < 0 or nb < 0 or na * nb > r.maxpix:
        raise ValueError("Renderer: bad box")
    out = r.img if out is None else out
    check(_lib.lib().wl_render_project(S._WLT[S._T(f)], C.byref(g), S._ptr(f), *v.flat(), axis, m, R.i3(lo), R.i3(hi), S._ptr(out), na))
    view = out[:na * nb].view(nb, na)
    sl = r.flow.layout.slab
    if sl is not None and axis != 2:                       # this rank's rows: the planes of the box it owns
        own_lo = sl.kz0 + sl.own_lo - (1 if (sl.ring and sl.rank == 0) else 0)
        z0, z1 = max(lo[2], own_lo), min(hi[2], sl.kz0 + sl.own_hi + 1)
        view = view[z0 - lo[2]:max(z1, z0) - lo[2]]
    return view


def shade(r: Renderer, img: torch.Tensor, clims, cmap="RdBu", levels: int = 0, mask: Optional[torch.Tensor] = None, mask_lt: float = 0.5,
          mask_rgba=(0, 0, 0, 255), nan_rgba=(0, 0, 0, 0), zoom: Optional[int] = None, flip_y: bool = True,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """RGBA8 of a [ny, nx] Float64 device image (contiguous rows): device view [ny*zoom, nx*zoom, 4] of `out` (default: the
    object's frame).  The arithmetic is wl_render_shade's (include/wlhip.h)."""
    ny, nx = (int(x) for x in img.shape)
    z = r.zoom if zoom is None else int(zoom)
    out = r.rgba if out is None else out
    nbytes = ny * nx * z * z * 4
    if out.numel() < nbytes:
        raise ValueError("Renderer: the frame buffer is too small for this image and zoom")
    u8 = lambda c: None if c is None else (C.c_uint8 * 4)(*[int(x) for x in c])
    check(_lib.lib().wl_render_shade(S._ptr(img), int(img.stride(0)) if ny > 1 else nx, nx, ny, float(clims[0]), float(clims[1]), int(levels),
                                     S._ptr(r.lut(cmap)), None if mask is None else S._ptr(mask),
                                     0 if mask is None else (int(mask.stride(0)) if ny > 1 else nx), float(mask_lt),
                                     u8(mask_rgba if mask is not None else None), u8(nan_rgba), z, int(bool(flip_y)), S._ptr(out)))
    return out[:nbytes].view(ny * z, nx * z, 4)


def _what(r: Renderer, sim, what, axis: int, i):
    """(field, kind, component, par, par2, scale) of a named picture"""
    flow = sim.flow
    if not isinstance(what, str):
        return what, ("scalar" if what.ndim == flow.D else "centre"), (0 if i is None else i), None, None, None
    if what in ("omega_mag", "lambda2"):
        return flow.u, what, 0, None, None, None
    if what == "curl":                                     # the component along the view (2-D: the only one), scaled as sim_gif! scales it
        return flow.u, "curl", (2 if flow.D == 2 else (axis if i is None else i)), None, None, float(sim.L) / float(sim.U)
    if what == "ke":
        return flow.u, "ke", 0, (0.0, 0.0, 0.0), None, None
    if what == "pressure":
        return flow.p, "scalar", 0, None, None, None
    if what == "u":
        return flow.u, "centre", (0 if i is None else i), None, None, None
    raise ValueError('Renderer: what must be "omega_mag", "lambda2", "curl", "omega_theta", "ke", "pressure", "u" or a field, '
                     f"not {what!r}")


def image(r: Renderer, sim, what="omega_mag", mode: str = "max", axis: int = 2, index: Optional[int] = None, box=None, i=None, par=None,
          par2=None, clims=None, cmap="RdBu", levels: int = 0, body: bool = True, flip_y: bool = True,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One shaded picture of the simulation: the RGBA uint8 device view [ny*zoom, nx*zoom, 4].
    what: "omega_mag", "lambda2", "curl" (times sim.L/sim.U), "omega_theta" (par = the axis z, par2 = the centre), "ke",
    "pressure", "u" (component i at the cell centre) or a field on the flow's grid; mode, axis, index, box as project().
    clims=None reads the image's minimum and maximum from the device: the ONE synchronising path (a constant image gets
    +-1 around its value).  body=True paints black the pixels where the MIN projection over the same box of mu0, averaged to
    the cell centre along the image's fast axis, is < 0.5: the on-device stand-in for body_plot!'s sdf contour (flow.sigma
    cannot serve: the step overwrites it)."""
    flow = sim.flow
    if flow is not r.flow:
        raise ValueError("Renderer: the simulation's flow differs from the one the object was made for")
    if isinstance(what, str) and what == "omega_theta":
        f, kind, ii, p1, p2, scale = flow.u, "omega_theta", 0, par, par2, None
    else:
        f, kind, ii, p1, p2, scale = _what(r, sim, what, axis, i)
        p1 = par if par is not None else p1
    img = project(r, f, kind, mode=mode, axis=axis, index=index, box=box, i=ii, par=p1, par2=p2)
    if scale is not None:
        img.mul_(scale)
    mask = None
    if body:
        c = 1 if axis == 0 else 0
        mask = project(r, flow.mu0, "centre", mode=("slice" if mode == "slice" else "min"), axis=axis, index=index, box=box, i=c, out=r.mask)
    if clims is None:
        ok = img[~torch.isnan(img)]
        lo, hi = (float(ok.min().item()), float(ok.max().item())) if ok.numel() else (0.0, 0.0)
        clims = (lo, hi) if (np.isfinite(lo) and np.isfinite(hi) and lo < hi) else (lo - 1.0, lo + 1.0) if np.isfinite(lo) else (-1.0, 1.0)
    return shade(r, img, clims, cmap=cmap, levels=levels, mask=mask, flip_y=flip_y, out=out)


# --------------------------------------------------------------------------- recording

def drain_one(r: Renderer) -> None:
    """wait for the oldest frame's copy and move it to r.frames (r: a Renderer, or a Scene, which has the same ring)"""
    slot = r.tail % r.ring
    r.events[slot].synchronize()
    shp = r.shapes[slot]
    n = shp[0] * shp[1] * 4
    r.frames.append(r.ring_host[slot, :n].numpy().reshape(shp[0], shp[1], 4).copy())
    r.tail += 1


def record(r: Renderer, sim, what="curl", **kw) -> None:
    """Render one frame (image()'s arguments) into the next slot of the ring and start its copy into the slot's pinned host twin
    behind an event.  It waits for nothing unless the ring is full: then the oldest frame is drained to r.frames first."""
    if r.head - r.tail >= r.ring:
        drain_one(r)
    slot = r.head % r.ring
    rgba = image(r, sim, what, out=r.ring_dev[slot], **kw)
    n = rgba.numel()
    r.ring_host[slot, :n].copy_(r.ring_dev[slot, :n], non_blocking=True)
    r.events[slot].record()
    r.shapes[slot] = (int(rgba.shape[0]), int(rgba.shape[1]))
    r.head += 1


def drain(r: Renderer) -> List[np.ndarray]:
    """wait for every copy in flight; all frames recorded so far, oldest first (host arrays [h, w, 4])"""
    while r.tail < r.head:
        drain_one(r)
    return r.frames


def save(r: Renderer, path, fps: float = 10.0) -> None:
    """Drain the ring and write the recorded frames: a PNG for one frame, an APNG (every PNG reader shows its first frame) for
    several.  The frame list is kept; clear r.frames to start another recording."""
    frames = drain(r)
    if not frames:
        raise ValueError("Renderer: nothing was recorded")
    write_apng(path, frames, fps=fps)


# --------------------------------------------------------------------------- PNG / APNG (zlib and struct only)

_PNG_SIG = b"\x89PNG\r\n\x1a\n"


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def _host_rgba(rgba) -> np.ndarray:
    a = rgba.detach().cpu().numpy() if isinstance(rgba, torch.Tensor) else np.asarray(rgba)
    if a.ndim != 3 or a.shape[2] != 4 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png: an image is a [h, w, 4] uint8 array")
    return np.ascontiguousarray(a)


def _idat(a: np.ndarray) -> bytes:
    """the zlib stream of the scanlines, each behind filter byte 0"""
    h, w, _ = a.shape
    raw = np.zeros((h, 1 + 4 * w), dtype=np.uint8)
    raw[:, 1:] = a.reshape(h, 4 * w)
    return zlib.compress(raw.tobytes(), 6)


def _ihdr(a: np.ndarray) -> bytes:
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", a.shape[1], a.shape[0], 8, 6, 0, 0, 0))     # 8-bit RGBA, no interlace


def write_png(path, rgba) -> None:
    """one [h, w, 4] uint8 image (a device tensor or a host array) as a PNG file"""
    a = _host_rgba(rgba)
    with open(path, "wb") as o:
        o.write(_PNG_SIG + _ihdr(a) + _chunk(b"IDAT", _idat(a)) + _chunk(b"IEND", b""))


def write_apng(path, frames: Sequence, fps: float = 10.0) -> None:
    """Frames of one size as an animated PNG: IHDR, acTL, then per frame fcTL and its data (IDAT for the first frame, fdAT after
    it), sequence numbers ascending over fcTL and fdAT together, IEND.  One frame: a plain PNG."""
    fr = [_host_rgba(f) for f in frames]
    if len(fr) == 1:
        return write_png(path, fr[0])
    if any(f.shape != fr[0].shape for f in fr):
        raise ValueError("write_apng: every frame must have the first one's size")
    h, w, _ = fr[0].shape
    num, den = 100, max(1, int(round(100 * float(fps))))
    seq = 0
    out = [_PNG_SIG, _ihdr(fr[0]), _chunk(b"acTL", struct.pack(">II", len(fr), 0))]
    for k, f in enumerate(fr):
        out.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, w, h, 0, 0, num, den, 0, 0)))
        seq += 1
        if k == 0:
            out.append(_chunk(b"IDAT", _idat(f)))
        else:
            out.append(_chunk(b"fdAT", struct.pack(">I", seq) + _idat(f)))
            seq += 1
    out.append(_chunk(b"IEND", b""))
    with open(path, "wb") as o:
        o.write(b"".join(out))


def sim_gif(sim, path, duration=1, step=0.1, remeasure=False, plotbody=False, verbose=False, ring: int = 8, zoom: int = 1, fps: float = 10.0,
            **kw) -> Renderer:
    """sim_gif! (ext/WaterLilyPlotsExt.jl:41-52): from t0 = round(sim_time(sim)), advance to t0, t0 + step, ..., t0 + duration and
    record the scaled vorticity after each; then write the APNG.  kw: image()'s arguments (clims, cmap, levels, axis, mode, ...);
    give clims, or every frame reads its own limits from the device.  Returns the Renderer (its frames are the movie)."""
    r = Renderer(sim.flow, ring=ring, zoom=zoom)
    t0 = float(np.round(S.sim_time(sim)))
    for k in range(int(np.floor(float(duration) / float(step) + 1e-9)) + 1):
        t = t0 + k * float(step)
        S.sim_step(sim, t, remeasure=remeasure)
        record(r, sim, "curl", body=plotbody, **kw)
        if verbose:
            print(f"tU/L={t:.4f}, Δt={sim.flow.dt[-1]:.3f}")
    save(r, path, fps=fps)
    return r


# --------------------------------------------------------------------------- z-slabs

def combine(mode: str, acc: np.ndarray, v: np.ndarray) -> np.ndarray:
    """acc (+)= v elementwise with the kernel's rule, acc the earlier operand (NaN: nothing yet / skipped for max, min, absmax)"""
    if mode in ("sum", "mean"):
        return acc + v
    with np.errstate(invalid="ignore"):
        if mode == "max":
            take = v > acc
        elif mode == "min":
            take = v < acc
        elif mode == "absmax":
            take = np.abs(v) > np.abs(acc)
        else:
            raise ValueError(f"Renderer: no such mode: {mode!r}")
    return np.where(take | np.isnan(acc), v, acc)


def gather(img, axis: int, mode: str, slab=None):
    """The ranks' parts of one project() on rank 0 as a host array (None on the other ranks; every rank must call it).  axis 0 or
    1: the rows concatenated in rank order, the undecomposed image bit for bit.  axis 2: max, min, absmax combined in rank
    order (exact); sum and mean partials added in ascending rank order (a reordered sum: within nz 2^-53 sum|x| of the
    undecomposed one)."""
    parts, root = _series.host_parts(img, slab)
    if not root:
        return None
    if int(axis) != 2:
        return np.concatenate(parts, axis=0)
    acc = parts[0]
    m = "max" if mode == "slice" else mode
    for p in parts[1:]:
        acc = combine(m, acc, p)
    return acc
