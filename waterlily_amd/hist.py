"""How the values of a flow field are distributed, counted on the device: PDFs, joint PDFs, conditional PDFs, volume fractions
and quantiles of a stored field, a face pair's mean or a Metrics.jl metric -- the member of the read-only family beside the
stepper (MeanFlow, Probes, Integrals, Forces, SurfaceLoads, Isosurface, Render, Downsample) that reduces over VALUES.  The
value of a cell is formed in registers, so the histogram of lambda2 or |omega| costs one read of u: no scratch field, no index
volume, and Float64 fields are not rounded.

    h = Histogram(sim.flow, Axis("lambda2", bins=512, range=(-1, 1)))
    c = count(h, sim.flow.u)                                      # device view [514] (int64): underflow, 512 bins, overflow
    q1, q99 = quantile(c, edges(h), [0.01, 0.99]).tolist()        # the one read: colour limits, an iso-level
    j = Histogram(sim.flow, Axis("lambda2", bins=64, range=(-1, 1)), Axis("scalar", bins=64))     # p auto-ranged on the device
    cj = count(j, sim.flow.u, sim.flow.p)                         # [66, 66]: cj[jb, ia]
    core = Histogram(sim.flow, Axis("scalar", bins=64, range=(-1, 1)), Axis("lambda2", edges=(-1e30, 0.0)))
    pc = conditional(count(core, sim.flow.p, sim.flow.u), 1)      # the PDF of p where -1e30 <= lambda2 <= 0
    hs = HistSeries(h); record(hs, sim, sim.flow.u); t, rows = series(hs)      # a PDF per step, no synchronisation

A joint histogram with ONE interior B-bin [blo, bhi] is the conditional count "A where blo <= B <= bhi": row 1 of the table.
fraction(c, k0, k1) of such counts over time is the volume-fraction series ("how much of the box is vortex core").

The kernels and their contract -- kinds, the bin rule, the layout of the counts, the slab rule, every refusal -- are in
include/wlhip.h (wl_histogram, wl_field_range) and csrc/wl_hist.h; tests/hist_ref.py restates them with numpy and gets the same
integers.  Counts are integers added with integer atomics: the result is a function of the field alone, bit for bit, decomposed
or not.  The views returned by count / range alias the object's buffers: the next call overwrites them.  Nothing here
synchronises with the device; pdf, cdf, quantile, marginal, conditional and fraction are torch operations on whatever device
their argument lives on, and the caller's .item() / .tolist() is the one read.  On z-slabs every rank counts the cells it owns
and gather() adds the parts on rank 0.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import _series
from . import sim as S
from ._lib import check

MAX_BINS, MAX_EDGES = 8192, 1024


class Axis(R.Value):
    """One axis of a histogram: a Value (kind, i, par, par2 as there) with bins.  abs: count |v| (.absval is the same).  The bins,
    one of: range=(lo, hi) with `bins` uniform bins (finite, hi > lo); range=None: `bins` uniform bins over the extremes of the
    field, found on the device by every non-accumulating count(); edges: bins + 1 strictly increasing finite numbers (at most
    1024 bins), the last one closed as in numpy."""

    def __init__(self, kind="scalar", i: int = 0, par=None, par2=None, bins: int = 256, range=None, edges=None, abs: bool = False):
        super().__init__(kind, i, par, par2, absval=abs)
        self.abs = self.absval
        self.edges = None
        self.range = None
        if edges is not None:
            if range is not None:
                raise ValueError("Axis: give range or edges, not both")
            e = np.array(edges, dtype=np.float64).ravel()
            if e.size < 2 or e.size - 1 > MAX_EDGES:
                raise ValueError(f"Axis: edges are 2 to {MAX_EDGES + 1} numbers")
            if not np.all(np.isfinite(e)) or not np.all(e[1:] > e[:-1]):
                raise ValueError("Axis: edges must be finite and strictly increasing")
            self.edges, self.bins = e, int(e.size - 1)
        else:
            self.bins = int(bins)
            if self.bins < 1:
                raise ValueError("Axis: bins must be >= 1")
            if range is not None:
                lo, hi = float(range[0]), float(range[1])
                if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo):
                    raise ValueError("Axis: range must be finite with hi > lo")
                self.range = (lo, hi)
        self.auto = self.edges is None and self.range is None


class Histogram:
    """The buffers of one (flow, a, b, box), made and validated once: the int64 counts, the four doubles of each axis's range,
    the uploaded edges and the scratch of wl_field_range.  b: the second axis of a joint histogram.  box = (lo, hi): the cells
    lo_d <= J_d < hi_d, 0-based, global along z (default: inside())."""

    def __init__(self, flow, a: Axis, b: Optional[Axis] = None, box=None):
        self.flow, self.a, self.b, self.D = flow, a, b, flow.D
        self.A, self.B = a.bins + 2, (b.bins + 2 if b is not None else 1)
        if self.A * self.B > MAX_BINS:
            raise ValueError(f"Histogram: (bins_a + 2) * (bins_b + 2) must not exceed {MAX_BINS}")
        sl = flow.layout.slab
        if sl is not None and sl.size > 1 and any(x is not None and x.auto for x in (a, b)):
            raise ValueError("Histogram: an automatic range is found per rank; on a decomposed flow give range=(lo, hi) or edges")
        box, given = R.box_of("Histogram", tuple(int(x) for x in flow.N), box)
        self.box = box if given else None
        self._grid = flow.layout.grid()
        nb = C.c_int64()
        check(_lib.lib().wl_field_range_scratch(C.byref(self._grid), C.byref(nb)))
        self._scratch = R.DevBuf(nb.value)
        self._cnt = R.DevBuf(8 * (2 + self.A * self.B))
        self._rng = R.DevBuf(8 * 8)                              # a: doubles 0..3, b: 4..7
        self._edges = {}
        for name, x in (("a", a), ("b", b)):
            if x is not None and x.edges is not None:
                self._edges[name] = R.DevBuf(8 * x.edges.size)
                self._edges[name].tensor(torch.float64, flow.device)[:x.edges.size].copy_(torch.from_numpy(x.edges))
        self._ax = {name: self._axis(name, x) for name, x in (("a", a), ("b", b)) if x is not None}

    def _axis(self, name: str, x: Axis) -> _lib.HistAxis:
        s = x.fill(_lib.HistAxis())
        s.nbins = x.bins
        if x.range is not None:
            s.lo, s.hi = x.range
        if x.auto:
            s.range_dev = self._rng.ptr + (0 if name == "a" else 32)
        if x.edges is not None:
            s.edges_dev = self._edges[name].ptr
        return s


def _field(h: Histogram, f: torch.Tensor, x: Axis) -> None:
    R.field_grid(h.flow, f, x.kind != R.R_SCALAR, "Histogram")


def range(h: Histogram, f: torch.Tensor, axis: str = "a") -> torch.Tensor:  # (hist.range; nothing below needs the builtin)
    """wl_field_range of the axis's value of `f` over the box: a device view of four doubles -- minimum, maximum, non-NaN cells,
    NaN cells -- in the object's buffer (NaN is skipped, -0 < +0, a box of nothing but NaN gives NaN, NaN)."""
    x = h.a if axis == "a" else h.b
    _field(h, f, x)
    lo, hi = R.box_args(h.box)
    out = h._rng.ptr + (0 if axis == "a" else 32)
    check(_lib.lib().wl_field_range(S._WLT[S._T(f)], C.byref(h._grid), S._ptr(f), *x.flat(), int(x.absval), lo, hi, C.c_void_p(h._scratch.ptr),
                                    h._scratch.nbytes, C.c_void_p(out)))
    k = 0 if axis == "a" else 4
    return h._rng.tensor(torch.float64, h.flow.device)[k:k + 4]


def count(h: Histogram, fa: torch.Tensor, fb: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """The counts of `fa` (and `fb` on the second axis): a device view, int64 [A] or [B, A] (bin 0: underflow, 1..bins: interior,
    bins + 1: overflow; cnt[jb, ia]), of the object's buffer, with two more views as attributes: .visited (the cells of the box)
    and .nan (the cells dropped because a value is NaN); visited == nan + cnt.sum().  accumulate: add to the counts that are
    there (a PDF over many steps); an automatic range is then NOT found again: the one of the last plain count() stays."""
    if (fb is None) != (h.b is None):
        raise ValueError("Histogram: a joint histogram takes two fields, a 1-D one takes one")
    if S._T(fa) != np.dtype(h.flow.T) or (fb is not None and S._T(fb) != np.dtype(h.flow.T)):
        raise ValueError("Histogram: the fields must have the flow's dtype")
    for name, x, f in (("a", h.a, fa), ("b", h.b, fb)):
        if x is None:
            continue
        _field(h, f, x)
        h._ax[name].f = f.data_ptr()
        if x.auto and not accumulate:
            range(h, f, name)
    lo, hi = R.box_args(h.box)
    check(_lib.lib().wl_histogram(S._WLT[S._T(fa)], C.byref(h._grid), C.byref(h._ax["a"]), C.byref(h._ax["b"]) if h.b is not None else None,
                                  lo, hi, int(bool(accumulate)), C.c_void_p(h._cnt.ptr)))
    return _view(h)


def _view(h: Histogram) -> torch.Tensor:
    t = h._cnt.tensor(torch.int64, h.flow.device)[:2 + h.A * h.B]
    c = t[2:] if h.b is None else t[2:].view(h.B, h.A)
    c.visited, c.nan = t[0], t[1]
    return c


def edges(h: Histogram, axis: str = "a") -> torch.Tensor:
    """The bins + 1 edges of an axis as a Float64 device tensor: the given edges; lo + k * ((hi - lo) / bins) of a uniform axis,
    formed from the device range of an automatic one without a read."""
    x = h.a if axis == "a" else h.b
    dev = h.flow.device
    if x.edges is not None:
        return h._edges[axis].tensor(torch.float64, dev)[:x.bins + 1]
    k = torch.arange(x.bins + 1, dtype=torch.float64, device=dev)
    if x.auto:
        r = h._rng.tensor(torch.float64, dev)[(0 if axis == "a" else 4):]
        return r[0] + k * ((r[1] - r[0]) / x.bins)
    lo, hi = x.range
    return lo + k * ((hi - lo) / x.bins)


# --------------------------------------------------------------------------- what one reads off the counts (any torch device)

def pdf(cnt: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """Density over the interior bins of a 1-D count: count / (N * width), N all non-NaN cells (underflow and overflow included),
    so the density integrates to the share of the cells that are in range."""
    e = torch.as_tensor(edges, dtype=torch.float64, device=cnt.device)
    return cnt[1:-1].to(torch.float64) / (cnt.sum().to(torch.float64) * (e[1:] - e[:-1]))


def cdf(cnt: torch.Tensor) -> torch.Tensor:
    """The share of the non-NaN cells in the bins 0..k of a 1-D count, for every k (the last entry is 1)."""
    return torch.cumsum(cnt, 0).to(torch.float64) / cnt.sum().to(torch.float64)


def quantile(cnt: torch.Tensor, edges: torch.Tensor, q) -> torch.Tensor:
    """The q-quantiles (q a number or a sequence in [0, 1]) of a 1-D count: N = all non-NaN cells, underflow and overflow as
    mass at the ends; target = q * N; k = the first bin whose cumulative count is >= target; the result lies the fraction
    (target - cumulative count before k) / count_k into that bin, between its edges.  A quantile inside the underflow gives
    e_0, one inside the overflow e_n.  A Float64 tensor on cnt's device."""
    e = torch.as_tensor(edges, dtype=torch.float64, device=cnt.device)
    n = cnt.numel() - 2
    qq = torch.as_tensor(q, dtype=torch.float64, device=cnt.device)
    cum = torch.cumsum(cnt, 0).to(torch.float64)
    target = qq * cum[-1]
    k = torch.clamp(torch.searchsorted(cum, target.reshape(-1), right=False), max=n + 1)
    before = torch.where(k > 0, cum[torch.clamp(k - 1, min=0)], torch.zeros_like(target.reshape(-1)))
    c = cnt[k].to(torch.float64)
    frac = torch.where(c > 0, (target.reshape(-1) - before) / torch.clamp(c, min=1.0), torch.zeros_like(before))
    e_lo, e_hi = e[torch.clamp(k - 1, 0, n)], e[torch.clamp(k, 0, n)]
    return (e_lo + frac * (e_hi - e_lo)).reshape(qq.shape)


def marginal(cnt: torch.Tensor, axis: str = "a") -> torch.Tensor:
    """The 1-D count of one axis of a joint count [B, A]: the sum over the other one."""
    return cnt.sum(0) if axis == "a" else cnt.sum(1)


def conditional(cnt: torch.Tensor, jb: int) -> torch.Tensor:
    """Row jb of a joint count: the 1-D count of A over the cells whose B value is in bin jb."""
    return cnt[int(jb)]


def fraction(cnt: torch.Tensor, k0: int, k1: int) -> torch.Tensor:
    """The share of the non-NaN cells that lie in the bins k0..k1 (both included) of a 1-D count."""
    return cnt[int(k0):int(k1) + 1].sum().to(torch.float64) / cnt.sum().to(torch.float64)


# --------------------------------------------------------------------------- over time, over ranks

class HistSeries(_series.Series):
    """Recorder of one Histogram's counts: row k = (visited, nan, the bins as count() lays them out), as Float64 (exact below
    2^53)."""

    def __init__(self, h: Histogram, capacity: int = 64):
        super().__init__(("HistSeries", "the recorder was"), h.D, h.flow.layout.slab, (2 + h.A * h.B,), capacity, h.flow.device)
        self.h = h


def record(hs: HistSeries, sim_or_flow, fa: torch.Tensor, fb: Optional[torch.Tensor] = None) -> None:
    """Append the counts of fa (and fb) now: one count() and one torch copy into the next row, no synchronisation."""
    flow = getattr(sim_or_flow, "flow", sim_or_flow)
    row = _series.next_row(hs, flow.D, flow.layout.slab)
    count(hs.h, fa, fb)
    row.copy_(hs.h._cnt.tensor(torch.int64, flow.device)[:row.numel()])
    hs.t.append(S.sim_time(sim_or_flow) if sim_or_flow is not flow else S.time(flow))


def series(hs: HistSeries) -> Tuple[np.ndarray, np.ndarray]:
    """(t[K], rows[K, 2 + A*B]) of the K records so far, the ranks' rows added (synchronises; on z-slabs every rank must call
    it).  rows[k, 2:] reshaped to [B, A] is the count of record k."""
    t, parts = _series.rank_rows(hs)
    return t, _series._add(parts)


reset = _series.reset


def combine(parts) -> np.ndarray:
    """The ranks' counts added: integer sums, so the result is the undecomposed count whatever the order."""
    out = np.array(parts[0], dtype=np.int64, copy=True)
    for p in parts[1:]:
        out += np.asarray(p, dtype=np.int64)
    return out


def gather(cnt, slab=None):
    """The ranks' counts added on rank 0 as a host array (None on the other ranks; every rank must call it)."""
    parts, root = _series.host_parts(cnt, slab)
    return combine(parts) if root else None
