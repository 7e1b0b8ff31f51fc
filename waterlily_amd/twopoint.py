"""How the value of a flow field at x relates to the value at x + r, summed on the device: correlations, structure functions and
the 1-D spectrum along one grid axis -- the member of the read-only family beside the stepper (MeanFlow, Probes, Integrals,
Forces, SurfaceLoads, Isosurface, Render, Downsample, Histogram) that reduces over PAIRS of cells.  Both values are formed in
registers from the flow arrays -- a stored field, a face pair's mean or a Metrics.jl metric -- and a line of the box is read once
for all its separations: no snapshot, no scratch field, no pass per separation.

    tp = TwoPoint(sim.flow, Value("centre", i=0), axis=2, nsep=256, periodic=True)      # u along the periodic span
    tab = measure(tp, sim.flow.u)                                  # device view [256, 10], float64
    L = integral_scale(tab)                                        # is the span wide enough?  (one .item() is the one read)
    for _ in range(1000): sim_step(sim); measure(tp, sim.flow.u, accumulate=True)       # the time-averaged statistic
    E = spectrum(measure(TwoPoint(flow, Value("ucomp", i=0), axis=0, periodic=True), flow.u))          # nsep = n
    s = TwoPoint(flow, Value("lambda2"), axis=0, nsep=64)          # the structure functions of lambda2, no scratch field
    S2, S3, F = structure(t := measure(s, flow.u), 2), structure(t, 3), flatness(t)

The table: row r = 0 .. nsep - 1, ten columns with a = A(I), b = B(I'), d = b - a, I' the cell r further along the axis:
N(r), sum a, sum b, sum a*a, sum b*b, sum a*b, sum d^2, sum d^3, sum d^4, sum |d|^3.  The kernels and their contract -- kinds,
the box, the pair rule, the exact operations, the ORDER of every sum, the slab rule, every refusal -- are in include/wlhip.h
(wl_twopoint) and csrc/wl_twopoint.h; tests/twopoint_ref.py restates them with numpy and gets the same bits.  The view returned
by measure aliases the object's buffer: the next call overwrites it.  Nothing here synchronises with the device; the functions
of the table are torch operations on whatever device their argument lives on.  On z-slabs (axes 0 and 1 only) every rank sums
the lines in the planes it owns and gather() adds the parts on rank 0.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import _series
from . import sim as S
from ._lib import check
from ._readout import Value  # noqa: F401  (one of the two values of a pair: the family's one descriptor of a cell's value)

COLS, MAX_LINE = 10, 1024


class TwoPoint:
    """The buffers of one (flow, a, b, axis, nsep, periodic, box), made and validated once: the [nsep, 10] table and the scratch
    of wl_twopoint.  b: the value at the partner cell (default: a itself, an auto-correlation).  nsep: the separations
    0 .. nsep - 1 in cells (default: the box's extent n along the axis).  periodic: the partner index wraps inside the box.
    box = (lo, hi): the cells lo_d <= J_d < hi_d, 0-based, global along z (default: inside())."""

    def __init__(self, flow, a: Value, b: Optional[Value] = None, axis: int = 0, nsep: Optional[int] = None, periodic: bool = False, box=None):
        self.flow, self.a, self.b, self.D = flow, a, b, flow.D
        self.axis, self.periodic = int(axis), bool(periodic)
        if not 0 <= self.axis < self.D:
            raise ValueError(f"TwoPoint: axis is 0..{self.D - 1}")
        if a.absval or (b is not None and b.absval):
            raise ValueError("TwoPoint: a Value with absval=True (wl_twopoint has no such switch)")
        sl = flow.layout.slab
        if self.axis == 2 and sl is not None and sl.size > 1:
            raise ValueError("TwoPoint: axis 2 of a flow decomposed along z: the lines cross ranks")
        (lo, hi), given = R.box_of("TwoPoint", tuple(int(x) for x in flow.N), box)
        self.box = (lo, hi) if given else None
        self.n = hi[self.axis] - lo[self.axis]
        if self.n > MAX_LINE:
            raise ValueError(f"TwoPoint: the box is longer than {MAX_LINE} cells along the axis")
        self.nsep = self.n if nsep is None else int(nsep)
        if not 1 <= self.nsep <= self.n:
            raise ValueError(f"TwoPoint: nsep is 1..{self.n}, the box's extent along the axis")
        self._grid = flow.layout.grid()
        self._val = {name: x.fill(_lib.TpValue()) for name, x in (("a", a), ("b", b)) if x is not None}
        nb = C.c_int64()
        blo, bhi = R.box_args(self.box)
        check(_lib.lib().wl_twopoint_scratch(C.byref(self._grid), self.axis, self.nsep, blo, bhi, C.byref(nb)))
        self._scratch = R.DevBuf(nb.value)
        self._tab = R.DevBuf(8 * COLS * self.nsep)


def measure(tp: TwoPoint, fa: torch.Tensor, fb: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """wl_twopoint of `fa` (and of `fb`, the field the value b reads; default: fa): a device view [nsep, 10] (float64) of the
    object's table, no synchronisation.  accumulate: add this call's sums, N(r) included, to the table that is there -- over
    many steps the time-averaged statistic.  The view carries n, periodic and auto (b is a) as the attributes tp_n,
    tp_periodic and tp_auto, which spectrum() reads."""
    if fb is not None and tp.b is None:
        raise ValueError("TwoPoint: a second field needs a second Value")
    fb = fa if (fb is None and tp.b is not None) else fb
    for x, f in ((tp.a, fa), (tp.b, fb)):
        if x is None:
            continue
        if S._T(f) != np.dtype(tp.flow.T):
            raise ValueError("TwoPoint: the fields must have the flow's dtype")
        R.field_grid(tp.flow, f, x.kind != R.R_SCALAR, "TwoPoint")
    tp._val["a"].f = fa.data_ptr()
    if tp.b is not None:
        tp._val["b"].f = fb.data_ptr()
    lo, hi = R.box_args(tp.box)
    check(_lib.lib().wl_twopoint(S._WLT[S._T(fa)], C.byref(tp._grid), C.byref(tp._val["a"]), C.byref(tp._val["b"]) if tp.b is not None else None,
                                 tp.axis, tp.nsep, int(tp.periodic), lo, hi, int(bool(accumulate)), C.c_void_p(tp._scratch.ptr),
                                 tp._scratch.nbytes, C.c_void_p(tp._tab.ptr)))
    return _view(tp)


def _view(tp: TwoPoint) -> torch.Tensor:
    t = tp._tab.tensor(torch.float64, tp.flow.device)[:COLS * tp.nsep].view(tp.nsep, COLS)
    t.tp_n, t.tp_periodic, t.tp_auto = tp.n, tp.periodic, tp.b is None
    return t


# --------------------------------------------------------------------------- what one reads off the table (any torch device)

def _cols(tab: torch.Tensor):
    t = torch.as_tensor(tab, dtype=torch.float64)
    return [t[:, q] for q in range(COLS)]


def covariance(tab: torch.Tensor) -> torch.Tensor:
    """C(r) = c5/N - (c1/N) * (c2/N): the mean of a*b over the pairs at separation r less the product of the two means over the
    same pairs.  [nsep], float64."""
    c = _cols(tab)
    return c[5] / c[0] - (c[1] / c[0]) * (c[2] / c[0])


def coefficient(tab: torch.Tensor) -> torch.Tensor:
    """rho(r) = C(r) / sqrt(var_a(r) * var_b(r)) with var_a = c3/N - (c1/N)^2 and var_b = c4/N - (c2/N)^2, the variances of a and
    of b over the pairs at separation r: 1 at r = 0 of an auto-correlation, and in [-1, 1] up to rounding."""
    c = _cols(tab)
    ma, mb = c[1] / c[0], c[2] / c[0]
    return (c[5] / c[0] - ma * mb) / torch.sqrt((c[3] / c[0] - ma * ma) * (c[4] / c[0] - mb * mb))


def structure(tab: torch.Tensor, p) -> torch.Tensor:
    """The structure function of order p of the increments d = b - a: p = 2: c6/N = <d^2>; 3: c7/N = <d^3>; 4: c8/N = <d^4>;
    "abs3": c9/N = <|d|^3>."""
    q = {2: 6, 3: 7, 4: 8, "abs3": 9}.get(p)
    if q is None:
        raise ValueError('structure: p is 2, 3, 4 or "abs3"')
    c = _cols(tab)
    return c[q] / c[0]


def skewness(tab: torch.Tensor) -> torch.Tensor:
    """<d^3> / <d^2>^(3/2) of the increments (0/0 = NaN where every increment is zero: r = 0 of an auto-correlation)."""
    s2 = structure(tab, 2)
    return structure(tab, 3) / (s2 * torch.sqrt(s2))


def flatness(tab: torch.Tensor) -> torch.Tensor:
    """<d^4> / <d^2>^2 of the increments (3 for Gaussian increments; NaN where every increment is zero)."""
    s2 = structure(tab, 2)
    return structure(tab, 4) / (s2 * s2)


def zero_crossing(tab: torch.Tensor) -> torch.Tensor:
    """Where rho(r) first reaches zero, in cells: with k the first separation at which rho(k) <= 0, the point
    (k - 1) + rho(k-1) / (rho(k-1) - rho(k)) of the chord; nsep - 1 if rho stays positive.  A 0-d float64 tensor."""
    return _scale(coefficient(tab))[1]


def integral_scale(tab: torch.Tensor) -> torch.Tensor:
    """The integral of rho(r) dr in cells from 0 to zero_crossing(tab): the trapezoid rule over the separations before the
    crossing plus the triangle under the chord up to it; rho positive throughout: the trapezoid rule over 0 .. nsep - 1."""
    return _scale(coefficient(tab))[0]


def _scale(rho: torch.Tensor):
    one, zero = torch.ones_like(rho[:1]), torch.zeros_like(rho[:1])
    pos = torch.cumsum((rho <= 0).to(torch.int64), 0) == 0           # the separations before the first rho <= 0
    left, right = rho[:-1], rho[1:]
    whole = pos[:-1] & pos[1:]
    last = pos[:-1] & ~pos[1:]                                       # the interval that holds the crossing (at most one)
    frac = torch.where(last, left / torch.where(last, left - right, one), zero)
    area = torch.where(whole, 0.5 * (left + right), zero).sum() + torch.where(last, 0.5 * left * frac, zero).sum()
    r0 = whole.to(torch.float64).sum() + frac.sum()
    return area, r0


def spectrum(tab: torch.Tensor, n: Optional[int] = None) -> torch.Tensor:
    """The one-sided 1-D spectrum E[k], k = 0 .. n div 2, of a periodic auto-covariance with nsep == n: with
    P[k] = (1/n) sum_r C(r) cos(2 pi k r / n) (torch.fft.rfft of covariance(tab), real part, over n), E[0] = P[0],
    E[k] = 2 P[k] for 0 < k < n/2 and E[n/2] = P[n/2] for even n, so that E.sum() == C(0) up to rounding.  n: the line's length;
    a view returned by measure() carries it.  Refused (ValueError) for a table that is not the periodic auto-covariance over the
    whole line: nsep != n, periodic=False, or a second value b."""
    if n is None:
        n = getattr(tab, "tp_n", None)
    if n is None:
        raise ValueError("spectrum: give n, the line's length (a view returned by measure() carries it)")
    if not getattr(tab, "tp_periodic", True) or not getattr(tab, "tp_auto", True) or tab.shape[0] != int(n):
        raise ValueError("spectrum: needs the periodic auto-covariance with nsep == n")
    P = torch.fft.rfft(covariance(tab)).real / float(n)
    w = torch.full_like(P, 2.0)
    w[0] = 1.0
    if int(n) % 2 == 0:
        w[-1] = 1.0
    return P * w


# --------------------------------------------------------------------------- over ranks

def combine(parts) -> np.ndarray:
    """The ranks' tables added in rank order, from the first: column 0, N(r), is exact (integers below 2^53); the nine sums are
    the DECOMPOSED sums -- each rank's sum in the contract's order, then the ranks in order -- not the bits of the
    undecomposed call."""
    out = np.array(parts[0], dtype=np.float64, copy=True)
    for p in parts[1:]:
        out = out + np.asarray(p, dtype=np.float64)
    return out


def gather(tab, slab=None):
    """The ranks' tables added in rank order on rank 0 as a host array (None on the other ranks; every rank must call it).
    Column 0 is exact; the sums are the decomposed sums, not the undecomposed bits (combine)."""
    parts, root = _series.host_parts(tab, slab)
    return combine(parts) if root else None
