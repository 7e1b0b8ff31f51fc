"""Numpy restatement of the Downsample kernel (include/wlhip.h: wl_downsample), with explicit loops over a block's cells in the
contract's order, double accumulators and ONE rounding to the output dtype.  Nothing here imports the package.

    values(f, kind, c, lo, hi)            the box's per-cell values as doubles [n0, n1, n2] (render_ref.values; "face" reads the
                                          stored component, like "ucomp"; a metric kind: the host copy of wl_metric's field as "scalar")
    downsample(vals, f, mode, D, face)    the coarse volume [ncx, ncy, ncz] (ncz = 1 in 2-D)

Order: the lane of fine x walks the f x f rows of its column of the block, z outer and y inner, ascending, with one
accumulator; then the f lanes of a block are combined by `for off in f/2, ..., 1: s[l] (+)= s[l + off]` over the lanes l < off.
face = c visits the block's low c-face alone: c == 0: lane 0 only (the others enter the tree with the start value), c == 1: the
first y row, c == 2: the first z plane.  (+)= is render_ref.acc_op.  "mean" multiplies the sum once by the exact power of two
1 / f^D (face: 1 / f^(D-1)); "sample" is the block's first cell.
"""
import numpy as np

import render_ref as RR

F64 = np.float64
MODES = RR.MODES + ("sample",)


def values(f, kind, c, lo, hi):
    return RR.values(f, "ucomp" if kind == "face" else kind, c, lo, hi)


def downsample(vals, f, mode, D, face=None, out=F64):
    n0, n1, n2 = vals.shape
    fz = f if D == 3 else 1
    assert n0 % f == 0 and n1 % f == 0 and n2 % fz == 0
    ncx, ncy, ncz = n0 // f, n1 // f, n2 // fz
    v = vals.reshape(ncx, f, ncy, f, ncz, fz)                  # [I, a, J, b, K, c]: fine x = I f + a, ...
    if mode == "sample":
        res = v[:, 0, :, 0, :, 0]
    else:
        acc = RR.start(mode, (ncx, f, ncy, ncz))               # one accumulator per lane a of every block
        lanes = slice(0, 1) if face == 0 else slice(None)
        for c in range(1 if face == 2 else fz):                # z outer
            for b in range(1 if face == 1 else f):             # y inner
                acc[:, lanes] = RR.acc_op(mode, acc[:, lanes], v[:, lanes, :, b, :, c])
        off = f // 2
        while off >= 1:
            acc[:, :off] = RR.acc_op(mode, acc[:, :off], acc[:, off:2 * off])
            off //= 2
        res = acc[:, 0]
        if mode == "mean":
            res = res * F64(1.0 / f ** (D - 1 if face is not None else D))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(res).astype(out)


def coarse_div(U):
    """sum_i U[I + e_i, i] - U[I, i] over the coarse cells that have their high faces: [n0 - 1, n1 - 1(, n2 - 1)] of U [n0, n1(, n2), D]"""
    D = U.shape[-1]
    inner = tuple(slice(0, n - 1) for n in U.shape[:D])
    div = np.zeros(tuple(n - 1 for n in U.shape[:D]), dtype=F64)
    for i in range(D):
        up = tuple(slice(1, n) if d == i else slice(0, n - 1) for d, n in enumerate(U.shape[:D]))
        div = div + (U[up + (i,)].astype(F64) - U[inner + (i,)].astype(F64))
    return div


def block_sum(a, f, D):
    """the plain sum of `a` [n0, n1(, n2)] over blocks of f^D cells, and of |a|"""
    sh = []
    for n in a.shape[:D]:
        sh += [n // f, f]
    ax = tuple(range(1, 2 * D, 2))
    b = a.astype(F64).reshape(sh)
    return b.sum(axis=ax), np.abs(b).sum(axis=ax)


def div_bound(u, lo, hi, f):
    """The bound of the divergence identity per coarse cell.  Both sides are sums, in different orders, of signed fine face
    values whose exact total is the same: the right side f^(1-D) sum_block div adds 2 D f^D of them (the interior ones cancel),
    the left side the 2 D f^(D-1) of the block's surface.  A sum of n doubles in any order is within n 2^-53 sum|x| of the
    exact one, so the two differ by at most (n_l + n_r) 2^-53 sum|x|, with sum|x| taken over the right side's (larger) set and
    scaled like the values by f^(1-D)."""
    D = len(lo)
    box = tuple(slice(l, h) for l, h in zip(lo, hi))
    tot = np.zeros(tuple(h - l for l, h in zip(lo, hi)), dtype=F64)
    for i in range(D):
        up = tuple(slice(l + (d == i), h + (d == i)) for d, (l, h) in enumerate(zip(lo, hi)))
        tot += np.abs(u[up + (i,)].astype(F64)) + np.abs(u[box + (i,)].astype(F64))
    n = 2 * D * f ** D + 2 * D * f ** (D - 1)
    return n * 2.0 ** -53 * block_sum(tot, f, D)[0] * float(f) ** (1 - D)
