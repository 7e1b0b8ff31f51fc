"""The connected regions of a threshold set, labelled on the device: how many vortices there are, where they are, how big, how
strong, and which one at step n is the one from step n - 1 -- the member of the read-only family beside the stepper (MeanFlow,
Probes, Integrals, Forces, SurfaceLoads, Isosurface, Render, Downsample, Histogram, TwoPoint) that treats the cells as a GRAPH.
A cell is IN when its value -- a stored field, a face pair's mean or a Metrics.jl metric, formed in registers -- is below
(above) a level; IN cells that share a face are joined; every connected component is a region with a number, a row of integers
and two extremes.  No scratch field of values, no copy to the host, no flood fill.

    rg = Regions(sim.flow, Value("lambda2"), below=-0.01)          # the vortex cores; the level e.g. from hist.quantile
    res = table(rg, sim.flow.u)                                    # labels + one row per region (reads the count once)
    big = select(res, min_cells=50)                                # indices of the regions worth looking at
    volume(res)[big], centroid(res)[big], bbox(res)[big], peak(res, "min")[0][big]
    core = mask(res, big[0])                                       # bool, shaped like the box: feed it to Histogram, Render, ...
    nxt = table(rg2, sim.flow.u); follow(res, nxt)                 # res's regions in nxt's numbering, -1: lost
    rs = RegionSeries(rg, m=4); record(rs, sim, sim.flow.u); t, rows = series(rs)     # per step, no synchronisation
    circulation(rg, res, sim.flow.u)[big], enstrophy(rg, res, sim.flow.u)[big]        # how strong: exact integer sums
    sm = sums(rg, res, [Weight(Value("omega_mag"), power=2, moment=0)], sim.flow.u)   # any value, squared or not, times an index

The kernels and their contract -- kinds, the set, the box, the joins, the numbering, the 13 columns, every refusal -- are in
include/wlhip.h (wl_regions) and csrc/wl_regions.h; tests/regions_ref.py restates the definition with a breadth-first fill and
gets the same integers.  Every output is an integer or an extreme: a function of the field, the level and the box alone, bit
for bit.  Value-weighted sums per region (sums, circulation, enstrophy, kinetic_energy, weighted_centroid: wl_region_sums) are
integers too -- every term cut to fixed point against a per-column scale and added limb by limb -- so they need no order and
have the same bits on any launch shape; combine() adds the limbs of two calls made with the same scale.  Limits: face
neighbours only (no edge or corner joins); one rank (a decomposed flow is refused: regions cross ranks); fewer than 2^31 cells
in the box.

The views a result carries alias the object's buffers: the next call overwrites them.  label() does not synchronise; table()
reads the count once.  volume, centroid, bbox, peak, select, mask and follow are torch operations on whatever device the
result lives on (a Result may be built from CPU tensors).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import _series
from . import sim as S
from ._lib import check
from ._readout import Value

COLS = 13


class Result:
    """What one labelling gives.  lab: int32, shaped like the box (nx, ny[, nz]) with x fast, -1 or the region's number;
    tab [R', 13] int64 and ext [R', 2] float64 (include/wlhip.h has the columns); count, cells, nan, visited: 0-d int64
    tensors (regions, IN cells, NaN cells, cells of the box); lo: the box's low corner (array indices); n: its extents."""

    def __init__(self, lab, tab, ext, count, cells, nan, visited, lo, n):
        self.lab, self.tab, self.ext = lab, tab, ext
        self.count, self.cells, self.nan, self.visited = count, cells, nan, visited
        self.lo, self.n = tuple(int(x) for x in lo), tuple(int(x) for x in n)

    @property
    def flat(self) -> torch.Tensor:
        """the labels in the order of the dense index q = (k*ny + j)*nx + i"""
        return self.lab.permute(*reversed(range(self.lab.dim()))).reshape(-1)


class Regions:
    """The buffers of one (flow, value, level, box, periodic), made and validated once: the int32 label volume of the box, the
    [capacity, 13] table, the [capacity, 2] extremes, the four counts and the scratch of wl_regions.  Exactly one of below / above
    (the level c; a cell is IN when v < c / v > c, strictly).  box = (lo, hi): the cells lo_d <= J_d < hi_d, 0-based (default:
    inside()).  periodic: the axes along which the first and the last cell of every line of the box are joined too.  capacity:
    the rows of the table (table() grows it; 0: labels and counts only)."""

    def __init__(self, flow, value: Value, below=None, above=None, box=None, periodic=(), capacity: int = 4096):
        if (below is None) == (above is None):
            raise ValueError("Regions: give exactly one of below and above")
        self.flow, self.value, self.D = flow, value, flow.D
        self.cmp = _lib.WL_RG_BELOW if above is None else _lib.WL_RG_ABOVE
        self.c = _level(below if above is None else above)
        sl = flow.layout.slab
        if sl is not None and sl.size > 1:
            raise ValueError("Regions: a decomposed flow: regions cross ranks (merging rank-boundary labels is not there yet)")
        (lo, hi), given = R.box_of("Regions", tuple(int(x) for x in flow.N), box)
        self.box = (lo, hi) if given else None
        if value.kind >= R.R_METRIC and min(lo) < 1:
            raise ValueError("Regions: the box of a metric kind must lie in inside()")
        self.lo, self.n = lo, tuple(h - l for l, h in zip(lo, hi))
        self.ncell = int(np.prod(self.n, dtype=np.int64))
        if self.ncell >= 1 << 31:
            raise ValueError("Regions: the box holds 2^31 cells or more")
        axes = sorted(set(int(d) for d in (periodic if hasattr(periodic, "__iter__") else (periodic,))))
        if any(not 0 <= d < self.D for d in axes):
            raise ValueError(f"Regions: periodic holds axes 0..{self.D - 1}")
        self.periodic_mask = sum(1 << d for d in axes)
        if int(capacity) < 0:
            raise ValueError("Regions: capacity must be >= 0")
        self._grid = flow.layout.grid()
        self._val = value.fill(_lib.RgValue())
        nb = C.c_int64()
        blo, bhi = R.box_args(self.box)
        check(_lib.lib().wl_regions_scratch(C.byref(self._grid), blo, bhi, C.byref(nb)))
        self._scratch = R.DevBuf(nb.value)
        self._lab = R.DevBuf(4 * self.ncell)
        self._n = R.DevBuf(8 * 4)
        self._tables(int(capacity))

    def _tables(self, capacity: int) -> None:
        self.capacity = capacity
        self._tab = R.DevBuf(8 * COLS * capacity) if capacity else None
        self._ext = R.DevBuf(8 * 2 * capacity) if capacity else None


def _level(c) -> float:
    c = float(c)
    if c != c:
        raise ValueError("Regions: the level must not be NaN")
    return c


def label(rg: Regions, field: torch.Tensor, c=None) -> Result:
    """wl_regions of `field` (u for the component and metric kinds): a Result of device views with R' = capacity rows, of which
    the rows >= count mean nothing.  c: another level for this call.  No synchronisation."""
    if S._T(field) != np.dtype(rg.flow.T):
        raise ValueError("Regions: the field must have the flow's dtype")
    R.field_grid(rg.flow, field, rg.value.kind != R.R_SCALAR, "Regions")
    rg._val.f = field.data_ptr()
    lo, hi = R.box_args(rg.box)
    cap = rg.capacity
    check(_lib.lib().wl_regions(S._WLT[S._T(field)], C.byref(rg._grid), C.byref(rg._val), rg.cmp, rg.c if c is None else _level(c),
                                rg.periodic_mask, lo, hi, C.c_void_p(rg._lab.ptr), cap, C.c_void_p(rg._tab.ptr) if cap else None,
                                C.c_void_p(rg._ext.ptr) if cap else None, C.c_void_p(rg._n.ptr), C.c_void_p(rg._scratch.ptr),
                                rg._scratch.nbytes))
    return _view(rg, cap)


def _view(rg: Regions, rows: int) -> Result:
    dev = rg.flow.device
    lab = rg._lab.tensor(torch.int32, dev)[:rg.ncell].view(*reversed(rg.n)).permute(*reversed(range(rg.D)))
    if rg.capacity:
        tab = rg._tab.tensor(torch.int64, dev)[:COLS * rg.capacity].view(rg.capacity, COLS)[:rows]
        ext = rg._ext.tensor(torch.float64, dev)[:2 * rg.capacity].view(rg.capacity, 2)[:rows]
    else:
        tab, ext = torch.zeros((0, COLS), dtype=torch.int64, device=dev), torch.zeros((0, 2), dtype=torch.float64, device=dev)
    n = rg._n.tensor(torch.int64, dev)
    return Result(lab, tab, ext, n[0], n[1], n[2], n[3], rg.lo, rg.n)


def table(rg: Regions, field: torch.Tensor, c=None) -> Result:
    """label(), one read of the count, and the views cut to the R regions there are.  When R > capacity the table and the
    extremes grow to R and the call is made once more (the labels do not depend on the capacity)."""
    label(rg, field, c)
    R = int(rg._n.tensor(torch.int64, rg.flow.device)[0].item())
    if R > rg.capacity:
        rg._tables(R)
        label(rg, field, c)
    return _view(rg, R)


# --------------------------------------------------------------------------- what one reads off the table (any torch device)

def volume(res: Result) -> torch.Tensor:
    """the cells of every region: [R] int64"""
    return res.tab[:, 1]


def centroid(res: Result) -> torch.Tensor:
    """[R, D] float64: the mean of the cell centres, sum / cells - 0.5, in the frame x = J - 0.5 of iso and MeshBody.  It means
    nothing for a region that wraps around a periodic axis (the mean of indices on both sides of the seam)."""
    D = len(res.n)
    return res.tab[:, 2:2 + D].to(torch.float64) / res.tab[:, 1:2].to(torch.float64) - 0.5


def bbox(res: Result) -> torch.Tensor:
    """[R, D, 2] int64: the smallest and the largest array index of the region's cells along every axis (both included)"""
    D = len(res.n)
    return res.tab[:, 5:5 + 2 * D].reshape(-1, D, 2)


def position(res: Result, q: torch.Tensor) -> torch.Tensor:
    """the array indices [.., D] (the frame of the box arguments) of the dense indices q"""
    out, q = [], q.to(torch.int64)
    for d in range(len(res.n)):
        out.append(res.lo[d] + q % res.n[d])
        q = torch.div(q, res.n[d], rounding_mode="floor")
    return torch.stack(out, dim=-1)


def peak(res: Result, which: str = "min") -> Tuple[torch.Tensor, torch.Tensor]:
    """(value [R] float64, array indices [R, D] int64) of every region's minimum ("min") or maximum ("max"); where several
    cells attain it, the one with the smallest dense index"""
    if which not in ("min", "max"):
        raise ValueError('peak: which is "min" or "max"')
    k = 0 if which == "min" else 1
    return res.ext[:, k], position(res, res.tab[:, 11 + k])


def select(res: Result, min_cells: int = 1, touching_box: Optional[bool] = None) -> torch.Tensor:
    """The numbers of the regions with at least min_cells cells; touching_box: None: all of them, True: only those with a cell
    on a face of the box (cut by it, probably), False: only those without.  [.] int64."""
    keep = res.tab[:, 1] >= int(min_cells)
    if touching_box is not None:
        D = len(res.n)
        bb = bbox(res)
        lo = torch.tensor(res.lo[:D], dtype=torch.int64, device=res.tab.device)
        hi = lo + torch.tensor(res.n[:D], dtype=torch.int64, device=res.tab.device) - 1
        touch = ((bb[:, :, 0] == lo) | (bb[:, :, 1] == hi)).any(dim=1)
        keep = keep & (touch if touching_box else ~touch)
    return torch.nonzero(keep).reshape(-1)


def mask(res: Result, r) -> torch.Tensor:
    """bool, shaped like the box: the cells of region r"""
    return res.lab == int(r)


def follow(prev: Result, now: Result, which: str = "min") -> torch.Tensor:
    """For every region of `prev`, the number in `now` of the cell where its peak (minimum or maximum) was: -1: lost (the cell
    is not IN any more).  One gather; both results must be of the same box.  [R_prev] int64.  A row of `prev` beyond its
    count gives -1."""
    if which not in ("min", "max"):
        raise ValueError('follow: which is "min" or "max"')
    if prev.lo != now.lo or prev.n != now.n:
        raise ValueError("follow: the two results are of different boxes")
    q = prev.tab[:, 11 if which == "min" else 12]
    live = torch.arange(q.numel(), device=q.device) < prev.count
    got = now.flat[torch.where(live, q, torch.zeros_like(q))].to(torch.int64)
    return torch.where(live, got, torch.full_like(got, -1))


# --------------------------------------------------------------------------- value-weighted sums per region (wl_region_sums)

class Weight:
    """One column of sums(): the term of a cell is w = v (power 1) or v * v (power 2), v the Value's double, times the cell's
    0-based array index along axis `moment` when that is not None.  field: the tensor this column reads (default: the one
    sums() is given): the columns of one call may read p and u."""

    def __init__(self, value: Value, power: int = 1, moment: Optional[int] = None, field: Optional[torch.Tensor] = None):
        if int(power) not in (1, 2):
            raise ValueError("Weight: power is 1 or 2")
        if moment is not None and not 0 <= int(moment) <= 2:
            raise ValueError("Weight: moment is None or an axis")
        self.value, self.power, self.moment, self.field = value, int(power), None if moment is None else int(moment), field


def _weight(w) -> Weight:
    return w if isinstance(w, Weight) else Weight(w)


class Sums:
    """What one sums() gives: value [rows, ncol] float64 (the limbs rounded once; NaN where a term was not finite), acc
    [rows, ncol, 5] int64 (four limbs, low to high, and the count of non-finite terms), scale [ncol] int32 (E_c: the unit of
    column c is 2^(E_c - 126)) and over [ncol] int64 (terms at or beyond 2^(E_c + 1) under a given scale: a non-zero count
    means the column is invalid).  Device views that the next sums() of the same Regions object overwrites."""

    def __init__(self, value, acc, scale, over):
        self.value, self.acc, self.scale, self.over = value, acc, scale, over


class _SumBufs:
    """the buffers of one wl_region_sums call of up to 8 columns, sized with the Regions table"""

    def __init__(self, capacity: int):
        n = _lib.WL_RS_MAX_COLS
        self.capacity = capacity
        self.acc, self.val = R.DevBuf(8 * 5 * n * capacity), R.DevBuf(8 * n * capacity)
        self.scale, self.over = R.DevBuf(4 * n), R.DevBuf(8 * n)
        self.cols = (_lib.RsCol * n)()


def sums(rg: Regions, res: Result, weights: Sequence, field: Optional[torch.Tensor] = None, scale=None) -> Sums:
    """The sums of `weights` (Weight objects; a Value counts as Weight(value)) over the regions of `res`, the result of the last
    label() / table() of rg, whose labels are still in rg's buffer.  scale=None: every column finds its own exponent (the
    largest |term| of the box); an int tensor or list of len(weights) exponents: they are given, so that the limbs of several
    calls or boxes can be added (combine).  No synchronisation; the buffers come from the library's allocator, are sized with
    rg's table and grow with it; more than 8 weights are split over several calls, and the Sums returned then holds
    concatenated COPIES (torch.cat, still without a synchronisation), not views of the library's buffers."""
    ws = [_weight(w) for w in weights]
    if not ws:
        raise ValueError("Regions: sums needs at least one weight")
    if rg.capacity < 1:
        raise ValueError("Regions: sums needs a table (capacity >= 1)")
    if res.lo != rg.lo or res.n != rg.n:
        raise ValueError("Regions: the result is of another box than the Regions object")
    dev, T = rg.flow.device, np.dtype(rg.flow.T)
    rows, cap, n = res.tab.shape[0], rg.capacity, _lib.WL_RS_MAX_COLS
    given = None
    if scale is not None:
        given = torch.as_tensor(scale, dtype=torch.int32, device=dev).reshape(-1)
        if given.numel() != len(ws):
            raise ValueError("Regions: a given scale has one exponent per weight")
    chunks = [ws[k:k + n] for k in range(0, len(ws), n)]
    bufs = getattr(rg, "_sums", [])
    if bufs and bufs[0].capacity != cap:
        bufs = []
    while len(bufs) < len(chunks):
        bufs.append(_SumBufs(cap))
    rg._sums = bufs
    lo, hi = R.box_args(rg.box)
    parts = []
    for k, (ch, b) in enumerate(zip(chunks, bufs)):
        for c, w in enumerate(ch):
            f = field if w.field is None else w.field
            if f is None:
                raise ValueError("Regions: a weight without a field, and no field given to sums")
            if S._T(f) != T:
                raise ValueError("Regions: the field must have the flow's dtype")
            R.field_grid(rg.flow, f, w.value.kind != R.R_SCALAR, "Regions")
            col = b.cols[c]
            w.value.fill(col.v).f = f.data_ptr()
            col.power, col.moment = w.power, -1 if w.moment is None else w.moment
        nc = len(ch)
        sc = b.scale.tensor(torch.int32, dev)[:nc]
        if given is not None:
            sc.copy_(given[k * n:k * n + nc])
        check(_lib.lib().wl_region_sums(S._WLT[T], C.byref(rg._grid), lo, hi, C.c_void_p(rg._lab.ptr), C.c_void_p(rg._n.ptr), cap, nc,
                                        C.cast(b.cols, C.c_void_p), _lib.WL_RS_FIND if given is None else _lib.WL_RS_GIVEN,
                                        C.c_void_p(b.scale.ptr), C.c_void_p(b.acc.ptr), C.c_void_p(b.val.ptr), C.c_void_p(b.over.ptr)))
        parts.append(Sums(b.val.tensor(torch.float64, dev)[:cap * nc].view(cap, nc)[:rows],
                          b.acc.tensor(torch.int64, dev)[:cap * nc * 5].view(cap, nc, 5)[:rows], sc, b.over.tensor(torch.int64, dev)[:nc]))
    if len(parts) == 1:
        return parts[0]
    return Sums(*(torch.cat([getattr(p, a) for p in parts], dim=d) for a, d in (("value", 1), ("acc", 1), ("scale", 0), ("over", 0))))


def _round_once(N: int, E: int) -> float:
    """N * 2^(E - 126) rounded once to nearest-even: the finish rule of wl_region_sums with Python integers (normalise, round
    bit, sticky bit); never subnormal for E >= WL_RS_EMIN, +-inf beyond the largest double"""
    if N == 0:
        return 0.0
    mag = -N if N < 0 else N
    h = mag.bit_length() - 1
    mag <<= 191 - h                                            # the top bit is bit 191
    mant, rnd, sticky = mag >> 139, (mag >> 138) & 1, mag & ((1 << 138) - 1)
    if rnd and (sticky or mant & 1):
        mant += 1
    e = h + E - 126
    if mant >> 53:
        mant, e = mant >> 1, e + 1
    bits = (0x7FF << 52) if e > 1023 else ((e + 1023) << 52) | (mant & ((1 << 52) - 1))
    return float(np.array([bits | ((1 << 63) if N < 0 else 0)], dtype=np.uint64).view(np.float64)[0])


def finish(acc: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """[rows, ncol] float64 from limbs acc [rows, ncol, 5] and exponents scale [ncol]: what wl_region_sums writes to sum_dev,
    restated at the host with Python integers (synchronises; the result goes back to acc's device)"""
    a = acc.detach().cpu().numpy().astype(object)
    E = [min(max(int(e), _lib.WL_RS_EMIN), 1023) for e in scale.detach().cpu().tolist()]
    rows, ncol = a.shape[0], a.shape[1]
    out = np.empty((rows, ncol), dtype=np.float64)
    for r in range(rows):
        for c in range(ncol):
            l = a[r, c]
            out[r, c] = float("nan") if l[4] else _round_once(int(l[0]) + (int(l[1]) << 32) + (int(l[2]) << 64) + (int(l[3]) << 96), E[c])
    return torch.from_numpy(out).to(acc.device)


def combine(a: Sums, b: Sums) -> torch.Tensor:
    """The doubles of a's and b's limbs added: the sums over the union of two boxes (or ranks, or calls) whose region numbers
    agree and whose sums() were made with the same given scale.  [rows, ncol] float64, bit-equal to one call over the union."""
    if a.acc.shape != b.acc.shape or not torch.equal(a.scale.cpu(), b.scale.cpu()):
        raise ValueError("Regions: combine needs two Sums of the same shape and the same scale")
    return finish(a.acc + b.acc.to(a.acc.device), a.scale)


def circulation(rg: Regions, res: Result, u: torch.Tensor) -> torch.Tensor:
    """[rows, 3] float64: the sum of curl_i over every region's cells (the cell volume is 1); 2-D: [rows, 1], the one component"""
    comps = (0, 1, 2) if rg.D == 3 else (2,)
    return sums(rg, res, [Weight(Value("curl", i=i)) for i in comps], u).value


def enstrophy(rg: Regions, res: Result, u: torch.Tensor) -> torch.Tensor:
    """[rows] float64: the sum of omega_mag^2 (2-D: curl^2) over every region's cells"""
    w = Weight(Value("omega_mag"), power=2) if rg.D == 3 else Weight(Value("curl", i=2), power=2)
    return sums(rg, res, [w], u).value[:, 0]


def kinetic_energy(rg: Regions, res: Result, u: torch.Tensor) -> torch.Tensor:
    """[rows] float64: the sum of the metric ke (|u|^2 / 2 at the cell centre) over every region's cells"""
    return sums(rg, res, [Weight(Value("ke"))], u).value[:, 0]


def mean(sm: Sums, res: Result) -> torch.Tensor:
    """[rows, ncol] float64: sum / cells"""
    return sm.value / res.tab[:, 1:2].to(torch.float64)


def weighted_centroid(rg: Regions, res: Result, weight, field: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[rows, D] float64: sum(w * J) / sum(w) - 0.5, the frame of centroid(); NaN where sum(w) == 0.  weight: a Weight without
    a moment, or a Value."""
    w = _weight(weight)
    if w.moment is not None:
        raise ValueError("Regions: weighted_centroid takes a weight without a moment")
    return centroid_of(sums(rg, res, [w] + [Weight(w.value, w.power, d, w.field) for d in range(rg.D)], field).value)


def centroid_of(v: torch.Tensor) -> torch.Tensor:
    """[rows, D] from sums v [rows, 1 + D] whose columns are sum(w), sum(w * J_0), ..: sum(w * J) / sum(w) - 0.5, NaN where
    sum(w) == 0 (any torch device)"""
    den = v[:, 0:1]
    return torch.where(den == 0, torch.full_like(v[:, 1:], float("nan")), v[:, 1:] / den - 0.5)


# --------------------------------------------------------------------------- over time

SCOLS = COLS + 2


class RegionSeries(_series.Series):
    """Recorder of one Regions object: row k = (regions, IN cells, NaN cells, cells visited, then the m largest regions, largest
    first and equal sizes by ascending number, 15 numbers each: the 13 columns of the table and the two extremes), as Float64
    (integers are exact below 2^53).  A step with fewer than m regions leaves NaN in the rows that are missing.  Only the first
    `capacity` regions of the Regions object are seen: make it large enough (column 0 tells).  weights: Weight objects (or
    Values) whose sums() over the same m regions follow the existing columns, region by region: m * len(weights) numbers more."""

    def __init__(self, rg: Regions, m: int = 8, capacity: int = 64, weights: Sequence = ()):
        if int(m) < 0:
            raise ValueError("RegionSeries: m must be >= 0")
        self.m = int(m)
        self.weights = tuple(_weight(w) for w in weights)
        super().__init__(("RegionSeries", "the recorder was"), rg.D, rg.flow.layout.slab, (4 + (SCOLS + len(self.weights)) * self.m,), capacity,
                         rg.flow.device)
        self.rg = rg


def _largest(res: Result, m: int):
    """(order [mm] int64, live [mm] bool): the rows of the mm = min(m, rows) largest regions, largest first, equal sizes by
    ascending number; live: the row is below count"""
    rows = res.tab.shape[0]
    live = torch.arange(rows, device=res.tab.device) < res.count
    size = torch.where(live, res.tab[:, 1], torch.full_like(res.tab[:, 1], -1))
    order = torch.sort(size, descending=True, stable=True).indices[:min(m, rows)]
    return order, size[order] >= 0


def largest(res: Result, m: int) -> torch.Tensor:
    """[m, 15] float64: the rows (table, extremes) of the m largest regions among the rows below count, largest first, equal
    sizes by ascending number; NaN rows where there are fewer.  No synchronisation."""
    out = torch.full((m, SCOLS), float("nan"), dtype=torch.float64, device=res.tab.device)
    mm = min(m, res.tab.shape[0])
    if mm == 0:
        return out
    order, live = _largest(res, m)
    both = torch.cat([res.tab[order].to(torch.float64), res.ext[order]], dim=1)
    out[:mm] = torch.where(live.unsqueeze(1), both, out[:mm])
    return out


def record(rs: RegionSeries, sim_or_flow, field: torch.Tensor) -> None:
    """Append the regions of `field` now: one label() and torch copies into the next row, no synchronisation."""
    flow = getattr(sim_or_flow, "flow", sim_or_flow)
    row = _series.next_row(rs, flow.D, flow.layout.slab)
    res = label(rs.rg, field)
    row[:4].copy_(rs.rg._n.tensor(torch.int64, flow.device)[:4])
    if rs.m:
        row[4:4 + SCOLS * rs.m].copy_(largest(res, rs.m).reshape(-1))
    if rs.m and rs.weights:
        nw, mm = len(rs.weights), min(rs.m, res.tab.shape[0])
        out = torch.full((rs.m, nw), float("nan"), dtype=torch.float64, device=res.tab.device)
        if mm:
            order, live = _largest(res, rs.m)
            out[:mm] = torch.where(live.unsqueeze(1), sums(rs.rg, res, rs.weights, field).value[order], out[:mm])
        row[4 + SCOLS * rs.m:].copy_(out.reshape(-1))
    rs.t.append(S.sim_time(sim_or_flow) if sim_or_flow is not flow else S.time(flow))


def series(rs: RegionSeries) -> Tuple[np.ndarray, np.ndarray]:
    """(t[K], rows[K, 4 + 15*m (+ m*len(weights))]) of the K records so far (synchronises).  rows[k, 4:4 + 15*m] reshaped to
    [m, 15] are the largest regions of record k; with weights, rows[k, 4 + 15*m:] reshaped to [m, len(weights)] are their sums."""
    t, parts = _series.rank_rows(rs)
    return t, parts[0]


reset = _series.reset


def lambda2(rg: Regions, sim, c=None) -> Result:
    """table() of the lambda2 cores of sim.flow -- the twin of iso.lambda2, without its scratch field: rg was made with
    Value("lambda2") and below=...; c: another level for this call (hist.quantile picks one)."""
    if sim.flow is not rg.flow:
        raise ValueError("Regions: the simulation's flow differs from the one the object was made for")
    if rg.value.kind != R.KIND["lambda2"] or rg.cmp != _lib.WL_RG_BELOW:
        raise ValueError('Regions: lambda2 needs Regions(flow, Value("lambda2"), below=c)')
    return table(rg, sim.flow.u, c)
