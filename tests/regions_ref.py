"""The definition of wl_regions (include/wlhip.h) restated with numpy and plain Python: the value of every cell of the box from
the host restatements the other read-outs are held to (render_ref.values through hist_ref; a metric kind: the host copy of what
wl_metric stored), then an explicit breadth-first fill over the box in ascending dense index q.  A region gets its number when
the scan meets its first cell, which is its smallest q, and every cell the fill takes from the queue adds to its region's row
straight from the definition.  Nothing here imports the package, and nothing is shared with the kernels: no union-find, no runs,
no keys but total_order(), which spells out the IEEE total order the contract names.

    box_values(f, kind, c, lo, hi, absval)   the doubles of the box [nx, ny(, nz)]
    regions(v, c, above, periodic, lo)        labels [nx, ny(, nz)] int32, tab [R, 13] int64, ext [R, 2] float64, n [4] int64
"""
import os
import struct
import sys
from collections import deque

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hist_ref import values  # noqa: E402

F64 = np.float64


def box_values(f, kind, c, lo, hi, absval=False):
    v = values(f, kind, c, lo, hi)
    v = v if len(lo) == 3 else v[:, :, 0]                      # (render_ref gives a 2-D box a third axis of one)
    return np.abs(v) if absval else v


def total_order(x: float) -> int:
    """an integer that orders doubles as the IEEE total order does: -inf < .. < -0 < +0 < .. < +inf"""
    u = struct.unpack("<Q", struct.pack("<d", x))[0]
    return (~u & 0xFFFFFFFFFFFFFFFF) if u >> 63 else (u | (1 << 63))


def regions(v, c, above=False, periodic=(), lo=None):
    """v: the values of the box, [nx, ny] or [nx, ny, nz]; lo: the box's low corner in array indices (default: ones)"""
    v = np.asarray(v, dtype=F64)
    D = v.ndim
    n = list(v.shape) + [1] * (3 - D)
    nx, ny, nz = n
    lo = list(lo if lo is not None else [1] * D) + [0] * (3 - D)
    N = nx * ny * nz
    flat = v.reshape(-1, order="F")                            # the order of q
    with np.errstate(invalid="ignore"):
        inset = (flat > c) if above else (flat < c)
    nan = np.isnan(flat)
    vals = flat.tolist()
    isin = inset.tolist()
    wrap = [d in tuple(periodic) for d in range(3)]
    label = [-1] * N
    tab, ext = [], []
    for q0 in range(N):
        if not isin[q0] or label[q0] >= 0:
            continue
        r = len(tab)
        big = 1 << 62
        row = [q0, 0, 0, 0, 0, big, -1, big, -1, big, -1, -1, -1]
        vmin = vmax = None
        label[q0] = r
        todo = deque([q0])
        cells = []
        while todo:
            q = todo.popleft()
            cells.append(q)
            i, j, k = q % nx, (q // nx) % ny, q // (nx * ny)
            for d, (x, m) in enumerate(((i, nx), (j, ny), (k, nz))):
                for step in (-1, 1):
                    y = x + step
                    if y < 0 or y >= m:
                        if not wrap[d]:
                            continue
                        y %= m
                    p = [i, j, k]
                    p[d] = y
                    qq = (p[2] * ny + p[1]) * nx + p[0]
                    if isin[qq] and label[qq] < 0:
                        label[qq] = r
                        todo.append(qq)
        for q in sorted(cells):                                # ascending q: the first of equal extremes stays
            i, j, k = q % nx, (q // nx) % ny, q // (nx * ny)
            I, J, K = lo[0] + i, lo[1] + j, lo[2] + k
            row[1] += 1
            row[2] += I
            row[3] += J
            row[4] += K
            row[5], row[6] = min(row[5], I), max(row[6], I)
            row[7], row[8] = min(row[7], J), max(row[8], J)
            row[9], row[10] = min(row[9], K), max(row[10], K)
            key = total_order(vals[q])
            if vmin is None or key < vmin[0]:
                vmin = (key, vals[q])
                row[11] = q
            if vmax is None or key > vmax[0]:
                vmax = (key, vals[q])
                row[12] = q
        tab.append(row)
        ext.append([vmin[1], vmax[1]])
    labels = np.asarray(label, dtype=np.int32).reshape(v.shape, order="F")
    counts = np.asarray([len(tab), int(inset.sum()), int(nan.sum()), N], dtype=np.int64)
    return labels, np.asarray(tab, dtype=np.int64).reshape(-1, 13), np.asarray(ext, dtype=F64).reshape(-1, 2), counts
