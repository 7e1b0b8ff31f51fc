"""Numpy restatement of the Histogram kernels (include/wlhip.h: wl_histogram, wl_field_range) and of waterlily_amd.hist.quantile,
in exact vector forms: every step is one IEEE double operation or a comparison, so the integers are the device's.  Nothing here
imports the package.  The per-cell values come from render_ref.values (the same values Render and Downsample are held to).

    bins_uniform(v, lo, hi, n)   the bin 0..n+1 of every non-NaN v: v < lo: 0; v > hi: n + 1; !(hi > lo): 1 if lo <= v <= hi else
                                 n + 1; else 1 + min(n - 1, trunc((v - lo) * (n / (hi - lo)))), a product that is not < n - 1
                                 (NaN included) taking n - 1
    bins_edges(v, e)             v < e_0: 0; v > e_n: n + 1; else 1 + #{k in 1..n-1: e_k <= v}
    histogram(va, a, vb, b)      (visited, nan, table): an axis is {"n", "lo", "hi"} or {"edges"}; a cell with a NaN on either
                                 axis is dropped; table [A] or [B, A]
    field_range(v)               (min, max, non-NaN, NaN) as four doubles; -0 < +0; nothing but NaN: NaN, NaN
    quantile(cnt, edges, q)      the rule of hist.quantile on plain arrays, one q at a time, with a loop
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from render_ref import values  # noqa: E402,F401

F64 = np.float64


def bins_uniform(v, lo, hi, n):
    v, lo, hi = np.asarray(v, dtype=F64), F64(lo), F64(hi)
    out = np.empty(v.shape, dtype=np.int64)
    with np.errstate(all="ignore"):
        under = v < lo
        over = ~under & (v > hi)
        mid = ~under & ~over
        out[under] = 0
        out[over] = n + 1
        if not (hi > lo):
            out[mid] = np.where((lo <= v[mid]) & (v[mid] <= hi), 1, n + 1)
        else:
            scale = F64(n) / (hi - lo)
            t = (v[mid] - lo) * scale
            small = t < F64(n - 1)
            out[mid] = 1 + np.where(small, np.trunc(np.where(small, t, 0.0)).astype(np.int64), n - 1)
    return out


def bins_edges(v, e):
    v, e = np.asarray(v, dtype=F64), np.asarray(e, dtype=F64)
    n = e.size - 1
    out = np.empty(v.shape, dtype=np.int64)
    for idx in np.ndindex(v.shape):
        x = v[idx]
        if x < e[0]:
            out[idx] = 0
        elif x > e[n]:
            out[idx] = n + 1
        else:
            out[idx] = 1 + sum(1 for k in range(1, n) if e[k] <= x)
    return out


def bins(v, ax):
    return bins_edges(v, ax["edges"]) if "edges" in ax else bins_uniform(v, ax["lo"], ax["hi"], ax["n"])


def nbins(ax):
    return (len(ax["edges"]) - 1 if "edges" in ax else ax["n"]) + 2


def histogram(va, a, vb=None, b=None):
    va = np.asarray(va, dtype=F64).reshape(-1)
    nan = np.isnan(va)
    if vb is not None:
        vb = np.asarray(vb, dtype=F64).reshape(-1)
        nan = nan | np.isnan(vb)
    A, B = nbins(a), (nbins(b) if b is not None else 1)
    idx = bins(va[~nan], a)
    if b is not None:
        idx = idx + A * bins(vb[~nan], b)
    table = np.bincount(idx, minlength=A * B).astype(np.int64)
    return int(va.size), int(nan.sum()), (table if b is None else table.reshape(B, A))


def field_range(v):
    v = np.asarray(v, dtype=F64).reshape(-1)
    nan = np.isnan(v)
    w = v[~nan]
    if w.size == 0:
        return np.array([np.nan, np.nan, 0.0, float(nan.sum())], dtype=F64)
    mn, mx = w.min(), w.max()
    zeros = w[w == 0.0]
    if mn == 0.0:
        mn = F64(-0.0) if np.signbit(zeros).any() else F64(0.0)
    if mx == 0.0:
        mx = F64(0.0) if (~np.signbit(zeros)).any() else F64(-0.0)
    return np.array([mn, mx, float(w.size), float(nan.sum())], dtype=F64)


def quantile(cnt, edges, q):
    cnt, e = [int(c) for c in cnt], [float(x) for x in edges]
    n = len(cnt) - 2
    target = F64(q) * F64(sum(cnt))
    cum = 0
    for k, c in enumerate(cnt):
        before, cum = cum, cum + c
        if F64(cum) >= target:
            break
    if k == 0:
        return e[0]
    if k == n + 1:
        return e[n]
    frac = (target - F64(before)) / F64(c) if c > 0 else F64(0.0)
    return float(F64(e[k - 1]) + frac * (F64(e[k]) - F64(e[k - 1])))
