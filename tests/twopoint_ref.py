"""Numpy restatement of the TwoPoint kernels (include/wlhip.h: wl_twopoint), with loops in the contract's order: every step is
one IEEE double operation, so the bits are the device's.  Nothing here imports the package.  The per-cell values come from
hist_ref.values (the same values Render, Downsample and Histogram are held to).

    lines(vals, axis)                 the box's values [n0, n1, n2] as [lines, n], line q as the contract numbers them
    launch(nlines, n)                 (L, R, G): lines per round, rounds, workgroups
    wave_lines(nlines, n)             [4G, T] the lines of every wavefront in the order it takes them, -1 where it has no more
    terms(a, b)                       the nine terms of one pair (arrays), each operation on its own
    twopoint(A, B, nsep, periodic)    the table [nsep, 10] in the contract's order: i ascending within a line, a wavefront's
                                      lines ascending, the wavefronts' sums ascending, everything from +0
    exact(A, B, nsep, periodic)       (table, mag): the same terms, formed in double, summed in np.longdouble in no particular
                                      order, and sum |term| per entry (column 0: N(r), and 0)
    dyadic(A, B, nsep, periodic)      the table of data that are multiples of 1/16, by int64 arithmetic: exact, no order
    bound(table, mag)                 N * 2^-53 * sum |term|: what ANY order of adding N doubles can differ from the exact sum by
                                      (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: (N - 1) u to first order)
    fields(shape, T)                  the seeded host arrays the GPU tests upload (and the CPU test checks the two evaluations on)
    cosine(n, m), cosine_tol(n, m)    the line cos(2 pi m i / n) and what covariance() of its periodic table may be off by
"""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hist_ref import values  # noqa: E402,F401

F64 = np.float64
LD = np.longdouble
COLS, WG_CAP = 10, 512


@functools.lru_cache(maxsize=None)
def fields(shape, T):
    """(p, u, p8, u8) host arrays with ghosts, seeded (read-only); p8, u8: rounded to multiples of 1/8"""
    Ng = tuple(n + 2 for n in shape)
    rng = np.random.default_rng(17)
    p = np.asfortranarray(rng.standard_normal(Ng).astype(T))
    u = np.asfortranarray(rng.standard_normal(Ng + (len(shape),)).astype(T))
    out = p, u, np.asfortranarray((np.round(p * 8) / 8).astype(T)), np.asfortranarray((np.round(u * 8) / 8).astype(T))
    for a in out:
        a.setflags(write=False)
    return out


def lines(vals, axis):
    vals = np.asarray(vals, dtype=F64)
    order = {0: (2, 1, 0), 1: (2, 0, 1), 2: (1, 0, 2)}[axis]
    return np.ascontiguousarray(np.transpose(vals, order)).reshape(-1, vals.shape[axis])


def launch(nlines, n):
    L = 16 if n <= 255 else (8 if n <= 511 else 4)
    R = -(-nlines // L)
    return L, R, min(WG_CAP, R)


def wave_lines(nlines, n):
    L, R, G = launch(nlines, n)
    per = []
    for g in range(G):
        for w in range(4):
            per.append([q for t in range(g, R, G) for q in range(t * L + w, min(t * L + L, nlines), 4)])
    T = max(1, max(len(x) for x in per)) if per else 1
    out = np.full((len(per), T), -1, dtype=np.int64)
    for v, x in enumerate(per):
        out[v, :len(x)] = x
    return out


def terms(a, b):
    d = b - a
    d2 = d * d
    return [a, b, a * a, b * b, a * b, d2, d2 * d, d2 * d2, np.abs(d) * d2]


def count(nlines, n, nsep, periodic):
    r = np.arange(nsep, dtype=F64)
    return F64(nlines) * (np.full(nsep, F64(n)) if periodic else F64(n) - r)


def twopoint(A, B, nsep, periodic):
    A, B = np.asarray(A, dtype=F64), np.asarray(B, dtype=F64)
    nlines, n = A.shape
    wl = wave_lines(nlines, n)
    r = np.arange(nsep)
    acc = np.zeros((9, wl.shape[0], nsep), dtype=F64)
    with np.errstate(all="ignore"):
        for t in range(wl.shape[1]):
            q = wl[:, t]
            have = q >= 0
            if not have.any():
                continue
            qa = np.where(have, q, 0)
            for i in range(n):
                p = (i + r) % n if periodic else np.minimum(i + r, n - 1)
                valid = have[:, None] & (np.ones(nsep, dtype=bool) if periodic else (i + r < n))[None, :]
                a = np.broadcast_to(A[qa, i][:, None], (qa.size, nsep))
                b = B[qa][:, p]
                for c, term in enumerate(terms(a, b)):
                    acc[c] = np.where(valid, acc[c] + term, acc[c])
        tot = np.zeros((9, nsep), dtype=F64)
        for v in range(wl.shape[0]):
            tot = tot + acc[:, v, :]
    out = np.empty((nsep, COLS), dtype=F64)
    out[:, 0] = count(nlines, n, nsep, periodic)
    out[:, 1:] = tot.T
    return out


def exact(A, B, nsep, periodic):
    A, B = np.asarray(A, dtype=F64), np.asarray(B, dtype=F64)
    nlines, n = A.shape
    out, mag = np.zeros((nsep, COLS), dtype=LD), np.zeros((nsep, COLS), dtype=LD)
    out[:, 0] = count(nlines, n, nsep, periodic)
    with np.errstate(all="ignore"):
        for r in range(nsep):
            a, b = (A, np.roll(B, -r, axis=1)) if periodic else (A[:, :n - r], B[:, r:])
            for c, term in enumerate(terms(a, b)):
                out[r, 1 + c] = term.astype(LD).sum()
                mag[r, 1 + c] = np.abs(term).astype(LD).sum()
    return out, mag


def dyadic(A, B, nsep, periodic, q=16):
    """The table of data that are multiples of 1/q, in int64: every term and every sum is an integer over a power of q, so the
    order does not matter and nothing rounds (the caller's data are small: |q a|^4 * pairs stays far below 2^63, and every sum
    below 2^53 quanta, so the double it is returned as holds it exactly)."""
    a16, b16 = np.rint(np.asarray(A, dtype=F64) * q).astype(np.int64), np.rint(np.asarray(B, dtype=F64) * q).astype(np.int64)
    assert np.array_equal(a16 / F64(q), A) and np.array_equal(b16 / F64(q), B)
    nlines, n = a16.shape
    out = np.empty((nsep, COLS), dtype=F64)
    out[:, 0] = count(nlines, n, nsep, periodic)
    power = [1, 1, 2, 2, 2, 2, 3, 4, 3]
    for r in range(nsep):
        a, b = (a16, np.roll(b16, -r, axis=1)) if periodic else (a16[:, :n - r], b16[:, r:])
        d = b - a
        sums = [int(t.sum()) for t in (a, b, a * a, b * b, a * b, d * d, d * d * d, d * d * d * d, np.abs(d) * d * d)]
        assert max(abs(x) for x in sums) < 2 ** 53
        out[r, 1:] = [F64(x) / F64(q ** k) for x, k in zip(sums, power)]
    return out


def bound(table, mag):
    """per entry: N(r) * 2^-53 * sum |term| (column 0: 0)"""
    return np.asarray(table[:, :1], dtype=LD) * LD(2.0) ** -53 * mag


def cosine(n, m):
    return np.cos(2.0 * np.pi * m * np.arange(n) / n)


def cosine_tol(n, m):
    """What covariance() of the periodic auto table of equal lines cosine(n, m) may differ from cos(2 pi m r / n) / 2 by.  A
    sample: the argument 2 pi m i / n is formed with 3 roundings, so it is off by at most 3 * 2 pi m * u, and cos adds one
    rounding: e = (6 pi m + 1) u.  A product a*b: 2e + u.  The sum of N such terms, |term| <= 1, divided by N, in ANY order: N u
    with N = n per line (the lines are equal).  The two means are 0 to within e + n u, so their product is second order.  Twice
    the first-order total covers the second order and the division's own roundings."""
    return 2.0 * (2.0 * (6.0 * np.pi * m + 1.0) + 1.0 + n) * 2.0 ** -53
