"""The definition of wl_region_sums (include/wlhip.h) restated with Python integers, `math` and `fractions`: the scale of a
column from the largest finite |term|, the truncation of term * 2^(126 - E) toward zero as an exact rational, the four signed
32-bit digits, the count of non-finite terms, and ONE rounding of the integer sum to a double.  The values of the cells come
from regions_ref.box_values (the host restatements every read-out is held to) and labels from regions_ref.regions (the
breadth-first fill).  Nothing here imports the package and nothing is shared with the kernels: no bit fields of doubles, no
shifts of significands, no carries between words.

    scale_of(terms)                       E of a column: max(ilogb(M), EMIN)
    fixed(term, E)                        the integer n, or "nan" (not finite), or "over" (|term| >= 2^(E + 1))
    finish(N, E)                          N * 2^(E - 126) rounded once, to nearest-even
    sums(labels, cols, lo, cap, scale)    acc [rows, ncol, 5], value [rows, ncol], scale [ncol], over [ncol]
"""
import math
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from regions_ref import box_values, regions  # noqa: E402,F401

EMIN = -894
TWO = Fraction(2)


def term_of(v: float, power: int, J) -> float:
    """v, v*v, times (double)J when J is not None: Python floats are IEEE doubles, one rounding per operation"""
    w = v * v if power == 2 else v
    return w if J is None else w * float(J)


def scale_of(terms) -> int:
    M = max((abs(t) for t in terms if math.isfinite(t)), default=0.0)
    if M == 0.0:
        return EMIN
    return max(math.frexp(M)[1] - 1, EMIN)                    # frexp: M = m * 2^e with 0.5 <= m < 1, so ilogb(M) = e - 1


def clamp(E: int) -> int:
    return min(max(int(E), EMIN), 1023)


def fixed(term: float, E: int):
    if not math.isfinite(term):
        return "nan"
    if Fraction(abs(term)) >= TWO ** (E + 1):
        return "over"
    return int(Fraction(term) * TWO ** (126 - E))              # int() of a Fraction truncates toward zero


def digits(n: int):
    s, a = (-1 if n < 0 else 1), abs(n)
    assert a < 1 << 127
    return [s * ((a >> (32 * k)) & 0xFFFFFFFF) for k in range(4)]


def finish(N: int, E: int) -> float:
    if N == 0:
        return 0.0
    mag = abs(N)
    h = mag.bit_length() - 1
    if h <= 52:
        mant = mag << (52 - h)
    else:
        cut = h - 52
        mant, rem, half = mag >> cut, mag & ((1 << cut) - 1), 1 << (cut - 1)
        if rem > half or (rem == half and mant & 1):
            mant += 1
        if mant == 1 << 53:
            mant, h = mant >> 1, h + 1
    e = h + E - 126
    out = math.inf if e > 1023 else math.ldexp(float(mant), e - 52)      # (mant < 2^53: exact; e >= -1020: normal)
    return -out if N < 0 else out


def value_of(limbs, E: int) -> float:
    """limbs: the five entries of one (region, column)"""
    if limbs[4]:
        return math.nan
    return finish(sum(int(limbs[k]) << (32 * k) for k in range(4)), E)


def sums(labels, cols, lo, cap=None, scale=None, R=None):
    """labels: [nx, ny(, nz)] int, -1 or a region's number; cols: a list of (v, power, moment) with v the doubles of the box
    shaped like labels and moment None or an axis; lo: the box's low corner (array indices); cap: the rows of the table
    (default: R); scale: None (FIND) or the exponents (GIVEN); R: the regions there are (default: max label + 1)."""
    labels = np.asarray(labels)
    D = labels.ndim
    lab = labels.reshape(-1, order="F").tolist()
    R = (max(lab) + 1 if lab else 0) if R is None else int(R)
    cap = R if cap is None else int(cap)
    rows = min(R, cap)
    n = list(labels.shape)
    idx = np.indices(labels.shape)
    J = [(idx[d] + int(lo[d])).reshape(-1, order="F").tolist() for d in range(D)]
    ncol = len(cols)
    acc = [[[0] * 5 for _ in range(ncol)] for _ in range(rows)]
    Es, over = [], []
    for c, (v, power, moment) in enumerate(cols):
        assert list(np.shape(v)) == n
        vals = np.asarray(v, dtype=np.float64).reshape(-1, order="F").tolist()
        terms = [term_of(vals[q], power, None if moment is None else J[moment][q]) if lab[q] >= 0 else None for q in range(len(lab))]
        E = scale_of(t for t in terms if t is not None) if scale is None else clamp(scale[c])
        nover = 0
        for q, t in enumerate(terms):
            if t is None:
                continue
            nn = fixed(t, E)
            if nn == "over":
                nover += 1
            elif lab[q] < rows:
                if nn == "nan":
                    acc[lab[q]][c][4] += 1
                else:
                    for k, d in enumerate(digits(nn)):
                        acc[lab[q]][c][k] += d
        Es.append(E)
        over.append(nover)
    assert all(abs(x) < 1 << 63 for row in acc for col in row for x in col)
    value = [[value_of(acc[r][c], Es[c]) for c in range(ncol)] for r in range(rows)]
    return (np.asarray(acc, dtype=np.int64).reshape(rows, ncol, 5), np.asarray(value, dtype=np.float64).reshape(rows, ncol),
            np.asarray(Es, dtype=np.int32), np.asarray(over, dtype=np.int64))
