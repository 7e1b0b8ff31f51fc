"""The flow at points: WaterLily's `interp` on the device, point probes recorded during a run, and passive tracers.

    pr = Probes(sim.flow, [(40.5, 33.5, 33.5), (60.5, 33.5, 33.5)])
    tr = Tracers(sim.flow, x0)                       # (M, D) release positions
    for _ in range(n):
        sim_step(sim)
        record(pr, sim.flow)                         # two kernel launches, no synchronisation
        advance(tr, sim.flow)                        # one Heun step on the frozen end-of-step velocity
    t, v = series(pr)                                # v[k, q] = (u_1, .., u_D, p) at point q after step k
    x = positions(tr)                                # release order

Points are in the reference's 1-based INDEX coordinates of a cell-centred array: physical position + 1.5 (`loc`,
util.jl:160); on a z-slab z is the global coordinate.  Interpolation, out-of-range rule and slab ownership:
include/wlhip.h (wl_interp) and csrc/wl_probe.h.  Values are Float64 for Float32 and Float64 flows alike.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import _series
from . import sim as S
from ._lib import check
from ._series import _rank_parts, _rank_sum  # noqa: F401  (imported from here by other modules)


def _points(x, D: Optional[int] = None) -> np.ndarray:
    X = np.asarray(x, dtype=np.float64)
    if X.ndim == 0 or X.ndim > 2 or (D is not None and X.shape[-1] != D):
        raise ValueError(f"points must be D floats or an (M, D) array, got shape {X.shape}")
    return np.ascontiguousarray(X.reshape(-1, X.shape[-1]))


def _interp_dev(a: torch.Tensor, ncomp: int, x: torch.Tensor, out: torch.Tensor, ldo: int, D: int) -> None:
    g = S._grid_of(a, D)
    check(_lib.lib().wl_interp(S._WLT[S._T(a)], C.byref(g), S._ptr(a), ncomp, S._ptr(x), x.shape[0], S._ptr(out), ldo))


def interp(x, a: torch.Tensor):
    """util.jl:238-257.  x: one point (D floats) or an (M, D) array, D = len(x[-1]); a: a scalar field if a.ndim == D, else
    a staggered vector field (the reference's dispatch).  Returns Float64: a scalar or (D,) for one point, (M,) or (M, D) for
    many; NaN where a weighted corner lies outside the array.  Synchronous; on z-slabs every rank must call it (the ranks'
    values are combined at the host)."""
    if not isinstance(a, torch.Tensor) or a.device.type != "cuda":
        raise TypeError("interp: `a` must be a device field of this package")
    single = np.asarray(x).ndim == 1
    X = _points(x)
    D = X.shape[1]
    if a.ndim not in (D, D + 1) or (a.ndim == D + 1 and a.shape[D] != D):
        raise ValueError(f"interp: a field of shape {tuple(a.shape)} does not match {D}-D points")
    ncomp = 0 if a.ndim == D else D
    xd = torch.from_numpy(X).to(a.device)
    out = torch.empty((X.shape[0], max(1, ncomp)), dtype=torch.float64, device=a.device)
    _interp_dev(a, ncomp, xd, out, out.shape[1], D)
    v = _rank_sum(out.cpu().numpy(), getattr(a, "_wl_slab", None))
    v = v[:, 0] if ncomp == 0 else v
    return (float(v[0]) if ncomp == 0 else v[0]) if single else v


class Probes(_series.Series):
    """Point probes of u and p.  points: (M, D) index coordinates (or one point), kept on the device.  series: Float64 device
    buffer [capacity, M, D+1] -- row k holds u_1..u_D, p at every point after the k-th record; t: host list of the times."""

    def __init__(self, flow: S.Flow, points, capacity: int = 256):
        X = _points(points, flow.D)
        super().__init__(("Probes", "the probes were"), flow.D, flow.layout.slab, (X.shape[0], flow.D + 1), capacity, flow.device)
        self.M = X.shape[0]
        self.x = torch.from_numpy(X).to(flow.device)


def record(pr: Probes, flow: S.Flow) -> None:
    """Append u and p at the points: two wl_interp launches into the next row of the series, no synchronisation.  A full
    buffer is doubled by a device copy."""
    row = _series.next_row(pr, flow.D, flow.layout.slab)
    if pr.M:
        g = flow.layout.grid()
        L, t = _lib.lib(), S._WLT[flow.T]
        ld = pr.D + 1
        check(L.wl_interp(t, C.byref(g), S._ptr(flow.u), pr.D, S._ptr(pr.x), pr.M, S._ptr(row), ld))
        check(L.wl_interp(t, C.byref(g), S._ptr(flow.p), 0, S._ptr(pr.x), pr.M, C.c_void_p(row.data_ptr() + 8 * pr.D), ld))
    pr.t.append(S.time(flow))


def series(pr: Probes) -> Tuple[np.ndarray, np.ndarray]:
    """(t[K], values[K, M, D+1]) of the K records so far (synchronises; on z-slabs every rank must call it: the ranks'
    buffers are summed once, here)."""
    t, parts = _series.rank_rows(pr)
    return t, _series._add(parts)


reset = _series.reset


class Tracers:
    """Passive tracers: Float64 positions x (M, D) on the device, in index coordinates, and the release index `id` of every
    row (reorderings permute both).  Dead particles (left the domain through a non-periodic side, or met a NaN velocity)
    have NaN coordinates.  sort_every = s > 0: advance() calls sort_by_cell() after every s-th step (default 10: at 512^3 a
    row-sorted advance of 2^24 tracers takes 1.9 ms against 14.6 ms scattered, and one sort 2.6 ms; at 2^20, 0.70 / 0.92 /
    0.34 ms -- profiles/probes_512_f32.txt); 0 never sorts.  Not on z-slabs."""

    def __init__(self, flow: S.Flow, x0, sort_every: int = 10):
        if flow.layout.slab is not None:
            raise ValueError("Tracers: z-slab decompositions are not supported (particles would have to migrate between ranks)")
        X = _points(x0, flow.D)
        self.D, self.T, self.N = flow.D, flow.T, tuple(flow.N)
        self.x = torch.from_numpy(X).to(flow.device)
        self.id = torch.arange(X.shape[0], device=flow.device)
        self.sort_every, self.steps = int(sort_every), 0


def advance(tr: Tracers, flow: S.Flow, dt: Optional[float] = None) -> None:
    """Move the tracers by the step just taken (dt = flow.dt[-2], default) on the frozen end-of-step velocity: one Heun step,
    one kernel launch, no synchronisation.  Periodic directions are the flow's perdir."""
    if flow.D != tr.D or tuple(flow.N) != tr.N or flow.layout.slab is not None:
        raise ValueError("Tracers: the flow's grid differs from the one the tracers were made for")
    if dt is None:
        if len(flow.dt) < 2:
            return
        dt = flow.dt[-2]
    g = flow.layout.grid()
    check(_lib.lib().wl_tracer_advance(S._WLT[flow.T], C.byref(g), S._ptr(flow.u), S._ptr(tr.x), tr.x.shape[0], float(dt),
                                       S.permask(flow.perdir)))
    tr.steps += 1
    if tr.sort_every > 0 and tr.steps % tr.sort_every == 0:
        sort_by_cell(tr)


def sort_by_cell(tr: Tracers) -> None:
    """Reorder the particles by their floor cell, rows (k, j) first and i within a row, dead ones last (a stable torch
    argsort): neighbouring lanes of the advance kernel then read the same cache lines."""
    n = tr.N
    f = torch.floor(tr.x)
    key = f[:, 0]
    for d in range(1, tr.D):
        key = key + f[:, d] * float(np.prod(n[:d]))
    key = torch.nan_to_num(key, nan=float("inf"))
    perm = torch.argsort(key, stable=True)
    tr.x = tr.x[perm].contiguous()
    tr.id = tr.id[perm]


def positions(tr: Tracers) -> np.ndarray:
    """(M, D) positions in release order (synchronises)."""
    out = torch.empty_like(tr.x)
    out[tr.id] = tr.x
    return out.cpu().numpy()


def alive(tr: Tracers) -> int:
    """number of live particles (synchronises)"""
    return int((~torch.isnan(tr.x[:, 0])).sum().item())
