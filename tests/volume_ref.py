"""The definition of wl_scene_volume and wl_scene_average (include/wlhip.h) restated without the package: the ray, the box, the
stop at the surface, the samples and the composite with numpy float64 scalars, one operation at a time; the field's value
from probes_ref.interp, the colour index from render_ref.shade (the rule scene_ref.shade_index wraps), the block average in
scene_ref.resolve's integers.  Slow on purpose: loops over pixels and samples."""
import numpy as np

import probes_ref as PR
import render_ref as RR
import scene_ref as SR

F = np.float64
BIG = SR.BIG
IDENT = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 4, axis=1)


def _fin3(P):
    return all(bool(abs(x) <= BIG) for x in P)                 # False for NaN and +-inf


def point(h0, g, z):
    """the world point of NDC depth z on the ray whose homogeneous point is h0 + z g"""
    w = h0[3] + z * g[3]
    return [(h0[d] + z * g[d]) / w for d in range(3)]


def byte(x):
    x = np.floor(x + F(0.5))
    if x != x:
        return 0
    return int(min(max(x, 0.0), 255.0))


class Ray:
    """one pixel's ray: P0, D, s_in, s_out, s_stop, empty"""


def ray(Minv, i, j, W, H, blo, bhi, key):
    Minv = np.asarray(Minv, dtype=F).reshape(4, 4)
    R = Ray()
    with np.errstate(all="ignore"):
        xn = ((F(i) + F(0.5)) / F(W)) * F(2.0) - F(1.0)
        yn = F(1.0) - ((F(j) + F(0.5)) / F(H)) * F(2.0)
        h0 = [(Minv[r, 0] * xn + Minv[r, 1] * yn) + Minv[r, 3] for r in range(4)]
        g = [Minv[r, 2] for r in range(4)]
        P0, P1 = point(h0, g, F(0.0)), point(h0, g, F(1.0))
        R.P0 = P0
        R.D = D = [P1[d] - P0[d] for d in range(3)]
        R.empty = not (_fin3(P0) and _fin3(P1))
        s_in, s_out = F(0.0), F(1.0)
        for d in range(3):
            if D[d] == 0.0:
                if not (blo[d] <= P0[d] and P0[d] <= bhi[d]):
                    R.empty = True
            else:
                ta, tb = (blo[d] - P0[d]) / D[d], (bhi[d] - P0[d]) / D[d]
                tn = ta if ta < tb else tb
                tx = ta if ta > tb else tb
                s_in = s_in if s_in > tn else tn
                s_out = s_out if s_out < tx else tx
        R.s_in, R.s_out = s_in, s_out
        R.s_stop = F(np.inf)
        if key != SR.NOTHING:
            z = F(key >> 32) / SR.TWO32
            Ps = point(h0, g, z)
            R.s_stop = (((Ps[0] - P0[0]) * D[0] + (Ps[1] - P0[1]) * D[1]) + (Ps[2] - P0[2]) * D[2]) / ((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2])
    return R


def samples(R, ds, field, cache=None, at=None):
    """[(s_k, v)] of every sample the ray could take (the early stop cuts the list short later); the values of a pixel are kept
    in cache[at] when a cache is given: they do not depend on the tables"""
    if cache is not None and at in cache:
        return cache[at]
    out = []
    if not R.empty:
        ds = F(ds)
        k = 0
        while True:
            s = (F(k) + F(0.5)) * ds
            if not (s <= R.s_out and s < R.s_stop):
                break
            if s >= R.s_in:
                x = [(R.P0[d] + s * R.D[d]) + F(1.5) for d in range(3)]
                out.append((s, PR.interp(x, field)))
            k += 1
    if cache is not None:
        cache[at] = out
    return out


def march(field, Minv, ds, lo, hi, W, H, keys, rgba, background, vmin, vmax, levels, lut, opac, t_min, cache=None):
    """field: the dense host array with ghosts (any float dtype); keys: rows of Python integers (scene_ref.clear / draw); rgba: the
    shaded frame [H, W, 4] (uint8), read where the key is not "nothing".  Returns (out [H, W, 4] uint8, acc [H, W, 4] float64,
    taken [H, W] int: samples taken, NaN ones included, early [H, W] bool: the march ended at t_min, nans [H, W] int: taken samples
    whose value was NaN)."""
    blo = [F(lo[d]) - F(0.5) for d in range(3)]
    bhi = [F(hi[d]) - F(1.5) for d in range(3)]
    assert all(hi[d] - lo[d] >= 2 for d in range(3))
    out = np.zeros((H, W, 4), dtype=np.uint8)
    acc = np.zeros((H, W, 4), dtype=F)
    taken = np.zeros((H, W), dtype=np.int64)
    nans = np.zeros((H, W), dtype=np.int64)
    early = np.zeros((H, W), dtype=bool)
    opac = np.asarray(opac, dtype=F)
    t_min = F(t_min)
    for j in range(H):
        for i in range(W):
            key = keys[j][i]
            R = ray(Minv, i, j, W, H, blo, bhi, key)
            sv = samples(R, ds, field, cache, (j, i))
            C, T = [F(0.0), F(0.0), F(0.0)], F(1.0)
            if sv:
                idx = RR.shade(np.array([[v for _, v in sv]], dtype=F), vmin, vmax, levels, IDENT)[0, :, 0]
            for n, (_, v) in enumerate(sv):
                taken[j, i] += 1
                if v != v:
                    nans[j, i] += 1
                    continue
                a = opac[idx[n]]
                w = T * a
                for c in range(3):
                    C[c] = C[c] + w * F(lut[idx[n]][c])
                T = T * (F(1.0) - a)
                if T < t_min:
                    early[j, i] = True
                    break
            base = background if key == SR.NOTHING else rgba[j, i]
            px = [byte(C[c] + T * F(base[c])) for c in range(3)]
            px.append(byte((F(1.0) - T) * F(255.0) + T * F(base[3])))
            out[j, i] = px
            acc[j, i] = (C[0], C[1], C[2], T)
    return out, acc, taken, early, nans


def average(rgba, ssaa):
    """wl_scene_average: scene_ref.resolve's integers without the key test"""
    H, W = rgba.shape[:2]
    n = ssaa * ssaa
    s = rgba.astype(np.int64).reshape(H // ssaa, ssaa, W // ssaa, ssaa, 4).sum(axis=(1, 3))
    return ((s + n // 2) // n).astype(np.uint8)
