"""Box-filtered, cropped volumes of the flow made on the device, and snapshots of them: the 3-D member of the read-only family
beside the stepper (MeanFlow, Probes, Integrals, SurfaceLoads, Isosurface, Render).  A box of fine cells is cut into blocks of
factor^D cells and every block becomes one coarse cell; the cell's value -- a stored element, a face pair's mean or a Metrics.jl
metric -- is formed in registers, so a downsampled lambda2 or |omega| volume costs one read of u and a store of 1/factor^D of a
field, without a scratch volume.

    d = Downsampler(sim.flow, factor=4, box=((1, 1, 1), (129, 129, 129)))     # owns the coarse buffers, validates once
    p4 = volume(d, sim.flow.p, "scalar", mode="mean")                         # device view [ncx, ncy, ncz]
    l2 = volume(d, sim.flow.u, "lambda2", mode="min")
    U = velocity(d, sim.flow.u)                                               # [ncx', ncy', ncz', D] face means: staggered, coarse
    w = DownsampleWriter("wake", factor=4, attrib={"Lambda2": (lambda s: s.flow.u, "lambda2", "min")})
    write(w, sim); ...; close(w)                                              # .vti files of the coarse box and a .pvd

The kernel and its contract -- kinds, modes, the order of every accumulation, the box, the z-slab rules -- are in include/wlhip.h
(wl_downsample, wl_downsample_extent) and csrc/wl_downsample.h; tests/downsample_ref.py restates it with numpy loops and
reproduces every bit.  The views returned by volume / velocity alias the object's buffers: the next call overwrites them.
Nothing here synchronises with the device.  On z-slabs every rank makes the coarse planes whose blocks it owns and gather()
concatenates the parts on rank 0.
"""
from __future__ import annotations

import ctypes as C
import os
import time as _time
import xml.etree.ElementTree as ET
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import _series
from . import sim as S
from . import vtk
from ._lib import check
from ._readout import R_FACE  # noqa: F401  (the kind's number, under this module's name too)

FACTORS = (1, 2, 4, 8, 16)
_MODE = dict(R.MODE, sample=5)
_KIND = dict(R.KIND, face=R_FACE)


def extent(g, factor: int, lo, hi) -> Tuple[Tuple[int, int, int], int]:
    """wl_downsample_extent: (this rank's coarse extents (ncx, ncy, ncz), its first coarse plane) for the grid g and the box"""
    nc, k0 = (C.c_int32 * 3)(), C.c_int32()
    check(_lib.lib().wl_downsample_extent(C.byref(g), int(factor), R.i3(lo), R.i3(hi), nc, C.byref(k0)))
    return (int(nc[0]), int(nc[1]), int(nc[2])), int(k0.value)


def trim(N, factor: int, box=None):
    """The box (lo, hi) -- default: inside() of arrays of extents N -- with its high side cut down to extents that are multiples
    of `factor`."""
    D, f = len(N), int(factor)
    lo, hi = R.inside(N) if box is None else R.sides(box)
    if len(lo) != D or len(hi) != D:
        raise ValueError(f"Downsampler: a box is (lo, hi) with {D} entries each")
    hi = tuple(l + (h - l) // f * f for l, h in zip(lo, hi))
    if not R.box_ok(lo, hi, N):
        raise ValueError(f"Downsampler: bad box: after trimming to multiples of {f} it must hold 0 <= lo < hi <= n - 1, got {list(lo)}, {list(hi)}")
    return lo, hi


class Downsampler:
    """The coarse buffers of one (flow, factor, box), made and validated once.  factor: 1, 2, 4, 8 or 16 (1: a crop).  box =
    (lo, hi): the fine cells lo_d <= J_d < hi_d, 0-based, global along z (default: inside()); an extent that is no multiple of
    the factor is trimmed on the high side, and .box records what is left.  out: the dtype of the result (default: the flow's).
    .nc: this rank's coarse extents, .k0: its first coarse plane; .vbox, .vnc, .vk0: the same for velocity(), whose box is
    .box plus one coarse layer on the high side of every direction in which that fits (hi_d + factor <= n_d - 1)."""

    def __init__(self, flow, factor: int = 4, box=None, out=None):
        if int(factor) not in FACTORS:
            raise ValueError(f"Downsampler: factor must be one of {FACTORS}")
        self.flow, self.factor, self.D = flow, int(factor), flow.D
        self.T = np.dtype(flow.T if out is None else out)
        if self.T not in S._WLT:
            raise ValueError("Downsampler: out must be float32 or float64")
        N = tuple(int(x) for x in flow.N)
        self.box = trim(N, self.factor, box)
        g = S._grid_of(flow.p, self.D)
        self.nc, self.k0 = extent(g, self.factor, *self.box)
        lo, hi = self.box
        self.vbox = (lo, tuple(h + self.factor if h + self.factor <= n - 1 else h for h, n in zip(hi, N)))
        self.vnc, self.vk0 = extent(g, self.factor, *self.vbox)
        self._vol = R.DevBuf(int(np.prod(self.nc)) * self.T.itemsize)
        self._vel: Optional[R.DevBuf] = None


def _call(d: Downsampler, f: torch.Tensor, k: int, m: int, i: int, par, par2, box, ptr: int, ntuple: int, c: int) -> None:
    g = R.field_grid(d.flow, f, k != R.R_SCALAR, "Downsampler")
    check(_lib.lib().wl_downsample(S._WLT[S._T(f)], C.byref(g), S._ptr(f), *R.Value(k, i, par, par2).flat(), m, d.factor, R.i3(box[0]),
                                   R.i3(box[1]), S._WLT[d.T], C.c_void_p(ptr), int(ntuple), int(c)))


def volume(d: Downsampler, f: torch.Tensor, kind="scalar", mode: str = "mean", i: int = 0, par=None, par2=None) -> torch.Tensor:
    """The coarse volume of `f` over d.box: a device view [ncx, ncy, ncz] ([ncx, ncy] in 2-D) of the object's buffer, in d.T.
    kind: "scalar" (f a scalar field), "ucomp" / "centre" / "face" (component i of a vector field: as stored / averaged to the
    cell centre / the fine faces on the block's low i-face), or a metric of f = u: "ke", "curl", "omega_mag", "omega_theta",
    "lambda2" (i, par, par2 as waterlily_amd.sim.metric).  mode: "mean", "sum", "max", "min", "absmax" (the signed value of
    largest magnitude), "sample" (the block's first cell).  On a z-slab the view holds this rank's coarse planes."""
    _call(d, f, R.code(_KIND, kind), R.code(_MODE, mode), i, par, par2, d.box, d._vol.ptr, 1, 0)
    nc = d.nc
    t = d._vol.tensor(S._TORCH[d.T], d.flow.device)[:nc[0] * nc[1] * nc[2]]
    return t.view(nc[1], nc[0]).permute(1, 0) if d.D == 2 else t.view(nc[2], nc[1], nc[0]).permute(2, 1, 0)


def velocity(d: Downsampler, u: torch.Tensor) -> torch.Tensor:
    """The staggered coarse velocity over d.vbox: a device view [ncx', ncy', ncz', D] ([ncx', ncy', D] in 2-D) whose component i
    is the mean of the fine faces on the low i-face of each block.  In cells, sum_i U[I + e_i, i] - U[I, i] equals
    factor^(1-D) times the sum of the fine div over the block: every interior fine face cancels."""
    nc, D = d.vnc, d.D
    if d._vel is None:
        d._vel = R.DevBuf(int(np.prod(nc)) * D * d.T.itemsize)
    for c in range(D):
        _call(d, u, R_FACE, _MODE["mean"], c, None, None, d.vbox, d._vel.ptr, D, c)
    t = d._vel.tensor(S._TORCH[d.T], d.flow.device)[:nc[0] * nc[1] * nc[2] * D]
    return t.view(nc[1], nc[0], D).permute(1, 0, 2) if D == 2 else t.view(nc[2], nc[1], nc[0], D).permute(2, 1, 0, 3)


def gather(part, slab=None):
    """The ranks' parts of one volume() or velocity() on rank 0 as a host array (None on the other ranks; every rank must call
    it): the parts concatenated along z in rank order, which is the undecomposed volume bit for bit, since no block straddles
    two ranks."""
    parts, root = _series.host_parts(part, slab)
    if not root:
        return None
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=2)            # (a 2-D volume has no axis 2, and no ranks)


# --------------------------------------------------------------------------- snapshots

def default_attrib() -> Dict[str, tuple]:
    """name -> (field function of the simulation, kind, mode).  A vector field with kind "ucomp", "centre" or "face" is written
    as a 3-tuple (one call per component), every other entry as a scalar."""
    return {"Velocity": (vtk._velocity, "centre", "mean"), "Pressure": (vtk._pressure, "scalar", "mean")}


def header(nc, origin, spacing, arrays) -> bytes:
    """XML of a coarse ImageData file up to the '_' of the appended section.  nc: the coarse extents (3 entries), written from 0;
    arrays: (name, vtk type, ncomp, offset).  Origin and Spacing put coarse sample I_d at origin_d + I_d * spacing_d: the mean
    position of its fine cells in the frame of vtk.write's file."""
    ext = " ".join(f"0 {int(n) - 1}" for n in nc)
    num = lambda v: " ".join(repr(float(x)) for x in v)
    out = ['<?xml version="1.0" encoding="utf-8"?>',
           '<VTKFile type="ImageData" version="1.0" byte_order="LittleEndian" header_type="UInt64">',
           f'  <ImageData WholeExtent="{ext}" Origin="{num(origin)}" Spacing="{num(spacing)}">',
           f'    <Piece Extent="{ext}">', '      <PointData>']
    for name, vt, ncomp, off in arrays:
        out.append(f'        <DataArray type="{vt}" Name="{name}" NumberOfComponents="{ncomp}" format="appended" offset="{off}"/>')
    out += ['      </PointData>', '    </Piece>', '  </ImageData>', '  <AppendedData encoding="raw">', '   _']
    return "\n".join(out).encode()


def frame(lo, factor: int):
    """(origin, spacing) of the coarse file of a box that starts at `lo`: in vtk.write's file array index J sits at coordinate
    J + 1, so coarse sample 0 sits at lo_d + 1 + (factor - 1)/2 and the samples are `factor` apart (2-D: z = 1, spacing 1)."""
    f = int(factor)
    origin = [l + 1 + (f - 1) / 2 for l in lo] + [1.0] * (3 - len(lo))
    return tuple(origin), tuple([float(f)] * len(lo) + [1.0] * (3 - len(lo)))


class DownsampleWriter(vtk.VTKWriter):
    """vtk.VTKWriter for coarse volumes: the same ring of device slots, side stream, pinned host buffers and worker thread; what
    differs is what write() puts into a slot (wl_downsample instead of wl_snapshot_pack) and the file's frame.  attrib: name ->
    (field function, kind, mode); T: the dtype of the file.  ring, host_buffers, on_busy as vtk.VTKWriter.

    On a decomposed run the parts are already small: write() gathers them through the host (it then waits for the device and
    for the other ranks) and rank 0 writes ONE file itself; per-rank pieces are not written."""

    def __init__(self, fname="WaterLily_ds", factor: int = 4, box=None, attrib=None, dir="vtk_data", T=np.float32, ring=4, host_buffers=2,
                 on_busy="wait"):
        super().__init__(fname, default_attrib() if attrib is None else attrib, dir, ring=ring, host_buffers=host_buffers, on_busy=on_busy)
        if int(factor) not in FACTORS:
            raise ValueError(f"DownsampleWriter: factor must be one of {FACTORS}")
        self.factor, self.box, self.T = int(factor), box, np.dtype(T)
        self.d: Optional[Downsampler] = None                    # made at the first write, for that simulation's flow


def _plan(w: DownsampleWriter, sim):
    """[(name, field, kind code, mode code, vector?, ntuple, slot offset, bytes)] and the slot's size"""
    flow = sim.flow
    D, nc, tsz = flow.D, w.d.nc, w.T.itemsize
    fields, nbytes = [], 0
    for name, (func, kind, mode) in w.output_attrib.items():
        a = func(sim)
        if not isinstance(a, torch.Tensor) or not a.is_cuda:
            raise TypeError(f"attribute {name!r}: the function must return a device field of the simulation (e.g. sim.flow.u)")
        k, m = R.code(_KIND, kind), R.code(_MODE, mode)
        vec = a.ndim > D and k in (R.R_UCOMP, R.R_CENTRE, R_FACE)
        nct = 3 if vec else 1                                   # vectors carry 3 components (2-D: a zero third one)
        n = nc[0] * nc[1] * nc[2] * nct * tsz
        fields.append((name, a, k, m, vec, nct, nbytes, n))
        nbytes += (n + 255) // 256 * 256
    return fields, nbytes


def write(w: DownsampleWriter, sim) -> None:
    """A coarse snapshot at sim_time(sim).  Like vtk.write it only enqueues: one wl_downsample launch per attribute component
    into a device slot, one event; the worker thread does the one D2H copy on the side stream and writes the file."""
    w._check()
    t0 = _time.perf_counter()
    flow = sim.flow
    D = flow.D
    if w.d is None or w.d.flow is not flow:
        w.d = Downsampler(flow, w.factor, w.box, out=w.T)
    d = w.d
    fields, nbytes = _plan(w, sim)
    sl = sim.slab
    multi = sl is not None and sl.size > 1
    nbytes = max(nbytes, 256)
    slot = vtk._take_slot(w, nbytes, flow.device, zero=True)
    if slot is None:
        return
    base = slot.buf.data_ptr()
    for name, a, k, m, vec, nct, off, n in fields:
        for c in (range(D) if vec else (0,)):
            _call(d, a, k, m, c if vec else 0, None, None, d.box, base + off, nct, c)
    stem = f"{w.fname}_{w.count:06d}"
    path = os.path.join(w.dir_name, os.path.basename(stem) + ".vti")
    origin, spacing = frame(d.box[0], d.factor)
    ncg = tuple((h - l) // d.factor for l, h in zip(*d.box)) + (1,) * (3 - D)      # the whole box's coarse extents
    arrays, blocks, foff = [], [], 0
    for name, a, k, m, vec, nct, off, n in fields:
        nfile = ncg[0] * ncg[1] * ncg[2] * nct * w.T.itemsize
        arrays.append((name, vtk._VTK_T[w.T], nct, foff))
        blocks.append((off, n))
        foff += 8 + nfile
    head = header(ncg, origin, spacing, arrays)
    if not multi:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.default_stream(flow.device))     # the stream the library works on
        w._q.put((slot, ev, nbytes, path, head, blocks, None))
    else:
        _write_gathered(w, slot, nbytes, path, head, blocks, sl)
    w.entries.append((round(S.sim_time(sim), 4), path))
    w.count += 1
    w.stats["snapshots"] += 1
    w.stats["enqueue_s"] += _time.perf_counter() - t0


def _write_gathered(w: DownsampleWriter, slot, nbytes, path, head, blocks, sl) -> None:
    """the decomposed path: every rank's slot through the host to rank 0, which writes the arrays' parts in rank order (z is
    the slow axis of an array, so the parts of one array simply follow each other)"""
    import struct

    import torch.distributed as dist
    host = slot.buf[:nbytes].cpu().numpy()
    slot.free.set()
    parts = [None] * sl.size
    dist.all_gather_object(parts, [host[off:off + n].tobytes() for off, n in blocks])
    if sl.rank != 0:
        return
    with open(path + ".part", "wb") as f:
        f.write(head)
        for a in range(len(blocks)):
            f.write(struct.pack("<Q", sum(len(p[a]) for p in parts)))
            for p in parts:
                f.write(p[a])
        f.write(b"\n  </AppendedData>\n</VTKFile>\n")
    os.replace(path + ".part", path)
    w.stats["bytes"] += sum(len(b) for p in parts for b in p)


flush = vtk.flush
close = vtk.close


def read(path: str):
    """(arrays, origin, spacing) of a file write() made: arrays as vtk.read_vti returns them -- {name: (ncx, ncy, ncz) or
    (3, ncx, ncy, ncz)} over the coarse box -- and where they sit: sample I_d at origin_d + I_d * spacing_d in the frame of
    vtk.write's full-resolution file."""
    arrays = vtk.read_vti(path)
    with open(path, "rb") as f:
        head = f.read(min(os.path.getsize(path), 1 << 16))
    k = head.find(b"<AppendedData")
    root = ET.fromstring(head[:k] + b"</VTKFile>" if k >= 0 else head)
    img = root.find("ImageData")
    vec = lambda name: tuple(float(v) for v in img.get(name).split())
    return arrays, vec("Origin"), vec("Spacing")
