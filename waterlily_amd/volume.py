"""The field itself in a Scene's picture: a scalar field (|ω|, a tracer-like quantity, the pressure) ray-marched on the device as a
semi-transparent cloud through the same camera as the λ₂ surface and the body, which hide the cloud behind them.

    sc = scene.Scene(sim.flow, size=(1024, 768), ssaa=2)
    scene.clear(sc)
    scene.draw(sc, cam, tri, val, clims=(0, 0.5))               # the λ₂ surface
    scene.draw(sc, cam, scene.body_triangles(sim.body, t))      # the body
    volume.metric(sc, cam, sim, "omega_mag", clims=(0, 2))      # |ω| into a scratch field the scene owns, queued as the volume
    scene.record(sc)                                            # shade, march, average, into the ring

add() queues ONE volume for the picture begun by scene.clear(); scene.frame() runs it after the shade loop (wl_scene_volume) and
then averages with wl_scene_average in place of wl_scene_resolve.  The march and its contract -- the ray from the inverse
camera, the box of cell centres, the stop at the depth buffer's surface, the samples at (k + 0.5) ds, the front-to-back
composite written in place -- are in include/wlhip.h (wl_scene_volume) and csrc/wl_volume.h; tests/volume_ref.py restates
them with numpy scalars and gets the same bits.

Limits.  The samples lie on planes parallel to the picture plane (view-aligned slices): `step` is the distance between the
planes, and an oblique ray of a wide perspective walks 1/cos θ more length per sample.  Emission and absorption only, no
gradient lighting.  One volume per picture.  No distributed picture: a decomposed flow is refused.  metric() goes through a
scratch field: forming λ₂ per sample would cost 24 rotations at four times the cell count.  Nothing here synchronises with
the device: clims are required.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import scene
from . import sim as S
from ._lib import check

MAX_STEPS = 1 << 20


def opacity(kind="ramp", strength: float = 0.05, step: float = 1.0) -> np.ndarray:
    """The opacity table of a march with `step` between its samples: 256 doubles, entry idx the share a sample of colour index
    idx absorbs.  A[idx] is the share absorbed per cell length: "uniform" (strength everywhere), "ramp" (0 at vmin to strength at
    vmax), "abs" (0 at the middle of the table to strength at both ends: signed fields under "RdBu") or a (256,) array of the
    caller's.  The correction to the step, 1 - (1 - A)**step, is made here, on the host: the one place a power is taken."""
    strength, step = float(strength), float(step)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("Volume: step must be positive")
    idx = np.arange(256, dtype=np.float64)
    if isinstance(kind, str):
        if kind == "uniform":
            A = np.full(256, strength, dtype=np.float64)
        elif kind == "ramp":
            A = strength * (idx / 255.0)
        elif kind == "abs":
            A = strength * (np.abs(idx - 127.5) / 127.5)
        else:
            raise ValueError(f"Volume: no such opacity: {kind!r} (uniform, ramp, abs or 256 values)")
    else:
        A = np.array(kind, dtype=np.float64)
        if A.shape != (256,):
            raise ValueError("Volume: an opacity table holds 256 values")
    if not np.all((A >= 0.0) & (A <= 1.0)):
        raise ValueError("Volume: opacities lie in [0, 1]")
    return 1.0 - (1.0 - A) ** step


_table = opacity                                               # (add() has an argument of that name)


class _Volume:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def add(sc: scene.Scene, cam, flow, a: torch.Tensor, clims, cmap="RdBu", opacity="ramp", strength: float = 0.05, step: float = 1.0, box=None,
        levels: int = 0, t_min: float = 1.0 / 256.0, keep_acc: bool = False, ds: Optional[float] = None) -> None:
    """Queue the scalar field `a` (the layout of flow.p) as the volume of the picture begun by scene.clear(sc): seen through
    `cam` -- a Camera, the samples `step` apart between its near and far planes, or a 4x4 matrix for the scene's internal size
    with ds=, the step as a fraction of near..far -- coloured through `cmap` between clims (required) in `levels` bands, absorbing
    by opacity(opacity, strength, step), inside `box` = (lo, hi) (default: inside()).  A ray stops once less than t_min of what
    lies behind would show.  keep_acc: sc.volume.acc [H ssaa, W ssaa, 4] (Float64) gets C_r, C_g, C_b, T of every pixel.  The
    object keeps a, the tables and acc alive until the next clear()."""
    if not sc._cleared:
        raise ValueError("Scene: clear() starts a picture")
    if sc.volume is not None:
        raise ValueError("Volume: at most one volume per picture")
    if flow.D != 3:
        raise ValueError("Volume: a 3-D flow is needed")
    if flow.slab is not None:
        raise ValueError("Volume: a decomposed flow has no distributed picture")
    g = R.field_grid(flow, a, False, "Volume")
    if a.device != sc.device:
        raise ValueError("Volume: the field must be on the scene's device")
    (lo, hi), given = R.box_of("Volume", flow.N, box)
    if any(h - l < 2 for l, h in zip(lo, hi)):
        raise ValueError("Volume: the box needs two cells or more in every direction")
    if clims is None:
        raise ValueError("Volume: give clims (nothing here reads the field's range from the device)")
    vmin, vmax = float(clims[0]), float(clims[1])
    if not (np.isfinite(vmin) and np.isfinite(vmax) and vmin < vmax):
        raise ValueError("Volume: clims must be finite with clims[0] < clims[1]")
    step = float(step)
    if not (np.isfinite(step) and step > 0):
        raise ValueError("Volume: step must be positive")
    if isinstance(cam, scene.Camera):
        Minv = cam.inverse(sc.Wi, sc.Hi)
        ds = step / (cam.far - cam.near)
    else:
        if ds is None:
            raise ValueError("Volume: a camera given as a matrix needs ds, the step as a fraction of near..far")
        Minv = np.linalg.inv(np.asarray(cam, dtype=np.float64).reshape(4, 4))
        ds = float(ds)
    if not ds > 0:
        raise ValueError("Volume: ds must be positive")
    if ds < 1.0 / MAX_STEPS:
        raise ValueError(f"Volume: more than {MAX_STEPS} steps between near and far")
    if ds > 1.0:
        raise ValueError("Volume: the step is longer than near..far")
    if not np.all(np.isfinite(Minv)):
        raise ValueError("Volume: the camera matrix has no finite inverse")
    if not 0.0 <= float(t_min) < 1.0:
        raise ValueError("Volume: t_min lies in [0, 1)")
    table = _table(opacity, strength, step)
    sc.volume = _Volume(a=a, g=g, dtype=S._WLT[S._T(a)], Minv=scene._m16(Minv), ds=ds, box=R.box_args((lo, hi) if given else None), vmin=vmin,
                        vmax=vmax, levels=int(levels), lut=sc.lut(cmap), opac=torch.from_numpy(np.ascontiguousarray(table)).to(sc.device),
                        t_min=float(t_min),
                        acc=torch.zeros((sc.Hi, sc.Wi, 4), dtype=torch.float64, device=sc.device) if keep_acc else None)


def run(sc: scene.Scene, background) -> None:
    """scene.frame()'s volume pass: the queued volume composited in place over the shaded frame and the background"""
    v = sc.volume
    check(_lib.lib().wl_scene_volume(v.dtype, C.byref(v.g), S._ptr(v.a), v.Minv, v.ds, v.box[0], v.box[1], v.vmin, v.vmax, v.levels, S._ptr(v.lut),
                                     S._ptr(v.opac), v.t_min, C.c_void_p(sc._key.ptr), background, C.c_void_p(sc._rgba.ptr),
                                     None if v.acc is None else S._ptr(v.acc), sc.Wi, sc.Hi))


def metric(sc: scene.Scene, cam, sim, kind: str = "omega_mag", clims=None, i: int = 0, par=None, par2=None, **kw) -> None:
    """add() of a metric of sim.flow.u ("omega_mag", "ke", "curl", "omega_theta", "lambda2": waterlily_amd.sim.metric, with its i,
    par, par2), filled into a scratch scalar field the Scene owns (taken once with sim.like(flow.p)).  kw: add()'s arguments."""
    flow = sim.flow
    if flow.D != 3:
        raise ValueError("Volume: a 3-D flow is needed")
    if flow.slab is not None:
        raise ValueError("Volume: a decomposed flow has no distributed picture")
    if clims is None:
        raise ValueError("Volume: give clims (nothing here reads the field's range from the device)")
    if sc.volume is not None:
        raise ValueError("Volume: at most one volume per picture")
    if sc._vfield is None or not R.laid_out_like(sc._vfield, flow.p) or sc._vfield.device != flow.p.device:
        sc._vfield = S.like(flow.p)
    S.metric(sc._vfield, kind, flow.u, i, par, par2)
    add(sc, cam, flow, sc._vfield, clims, **kw)
