"""Numpy restatement of the two Render kernels (include/wlhip.h: wl_render_project, wl_render_shade), with explicit loops in the
contract's order, and a PNG / APNG reader for what waterlily_amd.render writes.  Nothing here imports the package.

    values(f, kind, c, lo, hi)   the box's per-cell values as doubles [n0, n1, n2] (a 2-D field gets n2 = 1)
    project(vals, axis, mode)    the image [nb, na]: one accumulator per pixel and plane-by-plane `acc (+)= plane` for axis 1 and 2;
                                 for axis 0 the 64 lane partials (lane l: cells l, l + 64, ...) and the tree
                                 `for off in 32, 16, ..., 1: s[l] (+)= s[l + off]` over the lanes l < off
    shade(img, ...)              the RGBA bytes, all arithmetic in IEEE double

(+)= is the kernel's: MAX / MIN / ABSMAX start from NaN = "nothing yet", skip a NaN operand and use strict comparisons (the
earlier operand stays on a tie); SUM / MEAN start from +0 and add; MEAN divides once by the count.
"""
import struct
import zlib

import numpy as np

F64 = np.float64
MODES = ("max", "min", "absmax", "sum", "mean")


def values(f, kind, c, lo, hi):
    """kind: "scalar" (f [n0, n1(, n2)]), "ucomp" / "centre" (f [..., D], component c).  Every element is converted to double first."""
    D = len(lo)
    box = tuple(slice(int(l), int(h)) for l, h in zip(lo, hi))
    if kind == "scalar":
        v = np.asarray(f)[box].astype(F64)
    else:
        a = np.asarray(f)[..., c]
        v = a[box].astype(F64)
        if kind == "centre":
            up = tuple(slice(int(l) + (d == c), int(h) + (d == c)) for d, (l, h) in enumerate(zip(lo, hi)))
            v = (v + a[up].astype(F64)) / 2.0
        elif kind != "ucomp":
            raise ValueError(kind)
    return v if D == 3 else v[:, :, None]


def acc_op(mode, acc, v):
    """acc (+)= v, acc the earlier operand"""
    if mode in ("sum", "mean"):
        return acc + v
    with np.errstate(invalid="ignore"):
        take = {"max": lambda: v > acc, "min": lambda: v < acc, "absmax": lambda: np.abs(v) > np.abs(acc)}[mode]()
    return np.where(take | np.isnan(acc), v, acc)


def start(mode, shape):
    return np.zeros(shape, dtype=F64) if mode in ("sum", "mean") else np.full(shape, np.nan, dtype=F64)


def project(vals, axis, mode):
    """vals [n0, n1, n2] doubles -> the image [nb, na] (pixel (a, b) at [b, a]; the image axes are the two others, ascending)"""
    n = vals.shape
    if axis in (1, 2):
        planes = np.moveaxis(vals, axis, 0)                    # [n_axis, na, nb]
        acc = start(mode, planes.shape[1:])
        for k in range(n[axis]):                               # ascending, one accumulator per pixel
            acc = acc_op(mode, acc, planes[k])
    else:
        part = start(mode, (64,) + n[1:])                      # lane partials
        for lane in range(64):
            for i in range(lane, n[0], 64):
                part[lane] = acc_op(mode, part[lane], vals[i])
        off = 32
        while off >= 1:
            part[:off] = acc_op(mode, part[:off], part[off:2 * off])
            off //= 2
        acc = part[0]
    if mode == "mean":
        with np.errstate(invalid="ignore", divide="ignore"):
            acc = acc / F64(n[axis])
    return np.ascontiguousarray(acc.T)


def absmax_ties(vals, axis):
    """the number of rays whose largest magnitude is attained by more than one cell (the tie rule would then matter)"""
    a = np.abs(vals)
    with np.errstate(invalid="ignore"):
        m = np.nanmax(a, axis=axis, keepdims=True)
    return int((((a == m).sum(axis=axis)) > 1).sum())


def shade(img, vmin, vmax, levels, lut, mask=None, mask_lt=0.5, mask_rgba=(0, 0, 0, 255), nan_rgba=(0, 0, 0, 0), zoom=1, flip_y=False):
    img = np.asarray(img, dtype=F64)
    nan = np.isnan(img)
    with np.errstate(invalid="ignore"):
        t = (img - F64(vmin)) / (F64(vmax) - F64(vmin))
        if levels == 0:
            x = np.clip(np.floor(t * 256.0), 0.0, 255.0)
        else:
            n = F64(levels)
            b = np.clip(np.floor(t * n), 0.0, n - 1.0)
            x = np.floor((b + 0.5) * 256.0 / n)
    out = np.asarray(lut, dtype=np.uint8)[np.where(nan, 0.0, x).astype(np.int64)]
    out[nan] = np.asarray(nan_rgba, dtype=np.uint8)
    if mask is not None:
        out[np.asarray(mask, dtype=F64) < mask_lt] = np.asarray(mask_rgba, dtype=np.uint8)
    if flip_y:
        out = out[::-1]
    return np.ascontiguousarray(np.repeat(np.repeat(out, zoom, axis=0), zoom, axis=1))


# --------------------------------------------------------------------------- PNG / APNG reader

def chunks(data):
    """[(tag, payload)] of a PNG byte string; the signature, every length and every CRC are checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, p = [], 8
    while p < len(data):
        (n,) = struct.unpack(">I", data[p:p + 4])
        tag, payload = data[p + 4:p + 8], data[p + 8:p + 8 + n]
        (crc,) = struct.unpack(">I", data[p + 8 + n:p + 12 + n])
        assert len(payload) == n and crc == (zlib.crc32(tag + payload) & 0xFFFFFFFF), tag
        out.append((tag, payload))
        p += 12 + n
    assert p == len(data) and out[0][0] == b"IHDR" and out[-1] == (b"IEND", b"")
    return out


def _unfilter0(raw, w, h):
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert not rows[:, 0].any()                                # filter type 0 on every scanline
    return rows[:, 1:].reshape(h, w, 4).copy()


def decode(data):
    """the frames [h, w, 4] of a PNG (one) or APNG (acTL.num_frames of them) written with 8-bit RGBA and filter 0, and the chunk tags"""
    ch = chunks(data)
    tags = [t for t, _ in ch]
    w, h, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", ch[0][1])
    assert (depth, ctype, comp, filt, lace) == (8, 6, 0, 0, 0)
    if b"acTL" not in tags:
        assert tags == [b"IHDR", b"IDAT", b"IEND"]
        return [_unfilter0(zlib.decompress(ch[1][1]), w, h)], tags
    assert tags[1] == b"acTL"
    nframes, _plays = struct.unpack(">II", ch[1][1])
    frames, seq, k = [], 0, 2
    for fno in range(nframes):
        assert tags[k] == b"fcTL"
        s, fw, fh, x0, y0, _num, _den, _disp, _blend = struct.unpack(">IIIIIHHBB", ch[k][1])
        assert (s, fw, fh, x0, y0) == (seq, w, h, 0, 0)
        seq += 1
        assert tags[k + 1] == (b"IDAT" if fno == 0 else b"fdAT")
        body = ch[k + 1][1]
        if fno > 0:
            assert struct.unpack(">I", body[:4])[0] == seq          # fcTL and fdAT share one ascending sequence
            seq += 1
            body = body[4:]
        frames.append(_unfilter0(zlib.decompress(body), w, h))
        k += 2
    assert tags[k:] == [b"IEND"]
    return frames, tags
