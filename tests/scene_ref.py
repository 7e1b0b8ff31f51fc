"""The definition of wl_scene_* (include/wlhip.h) restated without the package: the vertex stage with numpy float64 scalars, one
operation at a time; coverage and keys with Python integers; shade and resolve in the same order of operations.  Slow on
purpose: loops over triangles and pixels."""
import numpy as np

import render_ref

F = np.float64
NOTHING = (1 << 64) - 1
BIG = F(1.79769313486231570815e308)
TWO19, TWO32 = F(524288.0), F(4294967296.0)


def _fin(x):
    return bool(abs(x) <= BIG)                                 # False for NaN and +-inf


def vertex(M, p, W, H):
    """None (the triangle is dropped) or (X, Y, z_ndc, c_3) of one vertex"""
    M = np.asarray(M, dtype=F).reshape(4, 4)
    x, y, z = F(p[0]), F(p[1]), F(p[2])
    with np.errstate(all="ignore"):
        c = [((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(4)]
        if not all(_fin(v) for v in (x, y, z, *c)) or not c[3] > 0.0:
            return None
        zn = c[2] / c[3]
        if not (zn >= 0.0 and zn <= 1.0):
            return None
        sx = ((c[0] / c[3]) * F(0.5) + F(0.5)) * F(W)
        sy = (F(0.5) - (c[1] / c[3]) * F(0.5)) * F(H)
        if not (abs(sx) < TWO19 and abs(sy) < TWO19):
            return None
        X = int(np.floor(sx * F(256.0) + F(0.5)))
        Y = int(np.floor(sy * F(256.0) + F(0.5)))
    return X, Y, zn, c[3]


def edge(a, b, P):
    return (b[0] - a[0]) * (P[1] - a[1]) - (b[1] - a[1]) * (P[0] - a[0])


def bias(a, b):
    """0 on a top or left edge a -> b (a centre on it is accepted), -1 elsewhere"""
    return 0 if (b[1] < a[1] or (b[1] == a[1] and b[0] > a[0])) else -1


class Tri:
    """one triangle after the vertex stage and the exchange: V (three (X, Y)), z, w, A2, swapped, the clamped box"""


def setup(M, tri, W, H):
    """None when the triangle draws nothing, else a Tri"""
    vs = [vertex(M, tri[k], W, H) for k in range(3)]
    if any(v is None for v in vs):
        return None
    order = [0, 1, 2]
    A2 = edge(vs[0], vs[1], vs[2])
    if A2 == 0:
        return None
    if A2 < 0:
        order, A2 = [0, 2, 1], -A2
    T = Tri()
    T.order, T.A2 = order, A2
    T.V = [(vs[k][0], vs[k][1]) for k in order]
    T.z = [vs[k][2] for k in order]
    T.w = [vs[k][3] for k in order]
    xs, ys = [v[0] for v in T.V], [v[1] for v in T.V]
    T.ilo, T.ihi = max((min(xs) + 127) >> 8, 0), min((max(xs) - 128) >> 8, W - 1)
    T.jlo, T.jhi = max((min(ys) + 127) >> 8, 0), min((max(ys) - 128) >> 8, H - 1)
    if T.ilo > T.ihi or T.jlo > T.jhi:
        return None
    T.npix = (T.ihi - T.ilo + 1) * (T.jhi - T.jlo + 1)
    return T


def cover(T, i, j):
    """(covered, (E_0, E_1, E_2)) of pixel (i, j): column, row"""
    P = (256 * i + 128, 256 * j + 128)
    V = T.V
    E = (edge(V[1], V[2], P), edge(V[2], V[0], P), edge(V[0], V[1], P))
    ok = E[0] + bias(V[1], V[2]) >= 0 and E[1] + bias(V[2], V[0]) >= 0 and E[2] + bias(V[0], V[1]) >= 0
    return ok, E


def bary(T, E):
    a = F(T.A2)
    return [F(E[k]) / a for k in range(3)]


def depth_key(T, E, ident):
    b = bary(T, E)
    d = (b[0] * T.z[0] + b[1] * T.z[1]) + b[2] * T.z[2]
    q = np.floor(d * TWO32)
    q = F(0.0) if q < 0.0 else (F(4294967295.0) if q > 4294967295.0 else q)
    return (int(q) << 32) | ident


def clear(W, H):
    return [[NOTHING] * W for _ in range(H)]


def draw(keys, M, tris, W, H, base=0):
    """lower the keys (a list of rows of Python integers) with the triangles tris [nt, 3, 3]; returns per triangle the number of
    pixels of its clamped box (0: it draws nothing) -- what decides the path"""
    npix = []
    for t in range(len(tris)):
        T = setup(M, tris[t], W, H)
        npix.append(0 if T is None else T.npix)
        if T is None:
            continue
        for j in range(T.jlo, T.jhi + 1):
            row = keys[j]
            for i in range(T.ilo, T.ihi + 1):
                ok, E = cover(T, i, j)
                if ok:
                    k = depth_key(T, E, base + t)
                    if k < row[i]:
                        row[i] = k
    return npix


def as_array(keys):
    return np.array(keys, dtype=np.uint64)


def ids(keys):
    """int64 [H, W]: the triangle id of every pixel, -1 where there is nothing"""
    k = as_array(keys)
    return np.where(k == np.uint64(NOTHING), np.int64(-1), (k & np.uint64(0xFFFFFFFF)).astype(np.int64))


def shade_index(v, vmin, vmax, levels):
    """wl_render_shade's colour index of one value, through render_ref.shade with an identity table"""
    lut = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 4, axis=1)
    return int(render_ref.shade(np.array([[v]], dtype=F), vmin, vmax, levels, lut)[0, 0, 0])


def value(T, E, val):
    """the perspective-correct value at a pixel with edge values E; val: the triangle's three vertex values as stored"""
    b = bary(T, E)
    v = [F(val[k]) for k in T.order]
    with np.errstate(all="ignore"):
        q = [b[k] / T.w[k] for k in range(3)]
        return ((q[0] * v[0] + q[1] * v[1]) + q[2] * v[2]) / ((q[0] + q[1]) + q[2])


def light_factor(tri, light, ambient):
    P = np.asarray(tri, dtype=F)
    a, b = P[1] - P[0], P[2] - P[0]
    n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    s = F(ambient)
    if ln > 0.0:
        s = F(ambient) + (F(1.0) - F(ambient)) * abs(((n[0] * F(light[0]) + n[1] * F(light[1])) + n[2] * F(light[2])) / ln)
    return s


def lit(c, s):
    x = np.floor(F(c) * s + F(0.5))
    if x != x:
        return 0
    return int(min(max(x, 0.0), 255.0))


def shade(rgba, keys, M, tris, W, H, base=0, val=None, vmin=0.0, vmax=1.0, levels=0, lut=None, solid=(200, 200, 200, 255),
          light=(0, 0, 1), ambient=0.3, nan_rgba=(0, 0, 0, 0), values=None):
    """write rgba [H, W, 4] (uint8) at the pixels whose id lies in [base, base + nt); values: an optional float64 [H, W] array that
    receives the interpolated value of those pixels"""
    nt = len(tris)
    cache = {}
    for j in range(H):
        for i in range(W):
            k = keys[j][i]
            ident = k & 0xFFFFFFFF
            if k == NOTHING or not (base <= ident < base + nt):
                continue
            t = ident - base
            if t not in cache:
                cache[t] = (setup(M, tris[t], W, H), light_factor(tris[t], light, ambient))
            T, s = cache[t]
            col = solid
            if val is not None:
                v = value(T, cover(T, i, j)[1], val[t])
                if values is not None:
                    values[j, i] = v
                if v != v:
                    rgba[j, i] = nan_rgba
                    continue
                col = lut[shade_index(v, vmin, vmax, levels)]
            rgba[j, i] = (lit(col[0], s), lit(col[1], s), lit(col[2], s), 255)


def resolve(rgba, keys, ssaa, background):
    H, W = rgba.shape[:2]
    img = rgba.astype(np.int64)
    img[as_array(keys) == np.uint64(NOTHING)] = np.asarray(background, dtype=np.int64)
    n = ssaa * ssaa
    s = img.reshape(H // ssaa, ssaa, W // ssaa, ssaa, 4).sum(axis=(1, 3))
    return ((s + n // 2) // n).astype(np.uint8)


# --------------------------------------------------------------------------- cameras and cases the tests share

def ortho_screen(W, H):
    """the camera under which world (x, y, z) is pixel coordinates: s_x = x, s_y = y (y downwards), z_ndc = z"""
    return np.array([[2.0 / W, 0, 0, -1.0], [0, -2.0 / H, 0, 1.0], [0, 0, 1.0, 0], [0, 0, 0, 1.0]], dtype=F)


def perspective(W, H, eye_z=3.0, near=1.0, far=6.0, half=1.0):
    """an eye on the +z axis looking down -z at the plane z = 0, where x in [-half', half'] fills the image; c_3 = eye_z - z"""
    a = W / H
    f = eye_z / half
    return np.array([[f, 0, 0, 0], [0, f * a, 0, 0], [0, 0, -far / (far - near), far * (eye_z - near) / (far - near)],
                     [0, 0, -1.0, eye_z]], dtype=F)


def soup(W, H, seed=7, n_small=1940, n_big=40, n_edge=20):
    """a seeded triangle soup in ortho_screen's pixel coordinates: most 1-6 pixels wide, n_big spanning 10-60 pixels, n_edge hanging
    over the viewport's edges; depths in (0.05, 0.95)"""
    rng = np.random.default_rng(seed)
    tris = []
    for k in range(n_small + n_big + n_edge):
        if k < n_small:
            c = rng.uniform([0, 0], [W, H])
            r = rng.uniform(1.0, 6.0) / 2
        elif k < n_small + n_big:
            c = rng.uniform([0, 0], [W, H])
            r = rng.uniform(10.0, 60.0) / 2
        else:
            side = k % 4
            c = [(rng.uniform(0, W), -1.0), (rng.uniform(0, W), H + 1.0), (-1.0, rng.uniform(0, H)), (W + 1.0, rng.uniform(0, H))][side]
            r = rng.uniform(3.0, 12.0)
        ang = np.sort(rng.uniform(0, 2 * np.pi, 3))
        if rng.uniform() < 0.5:
            ang = ang[::-1]
        xy = np.asarray(c)[None, :] + r * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        z = rng.uniform(0.05, 0.95, 3)
        tris.append(np.concatenate([xy, z[:, None]], axis=1))
    return np.ascontiguousarray(np.array(tris, dtype=F))


def to_world(tris, W, H, half=1.0, zamp=0.5):
    """triangles given in ortho_screen's pixel coordinates moved in front of perspective(W, H, half=half): a point at depth 0.5
    lands on the plane z = 0 at the same pixel, the others within zamp of it (nearer ones grow, farther ones shrink)"""
    t = np.array(tris, dtype=F)
    out = np.empty_like(t)
    out[..., 0] = (t[..., 0] / W * 2.0 - 1.0) * half
    out[..., 1] = (1.0 - t[..., 1] / H * 2.0) * half * H / W
    out[..., 2] = (0.5 - t[..., 2]) * 2.0 * zamp
    return np.ascontiguousarray(out)


def quad_pair(x0=3, y0=2, n=9):
    """two triangles forming the square [x0 + 0.5, x0 + n + 0.5]^2 in pixel coordinates, their shared diagonal through pixel
    centres; the square's sides pass through centres too (top and left are in, bottom and right out)"""
    a, b = x0 + 0.5, x0 + n + 0.5
    c, d = y0 + 0.5, y0 + n + 0.5
    z = 0.5
    return np.array([[[a, c, z], [b, c, z], [b, d, z]], [[a, c, z], [b, d, z], [a, d, z]]], dtype=F)


def sheet(W, H, n=12, m=9, seed=3, margin=4.0, zfun=None):
    """a jittered n x m quad sheet (two triangles per quad, alternating diagonals) that reaches `margin` pixels beyond the viewport
    on every side; the outer ring of points is not jittered"""
    rng = np.random.default_rng(seed)
    xs = np.linspace(-margin, W + margin, n + 1)
    ys = np.linspace(-margin, H + margin, m + 1)
    P = np.zeros((m + 1, n + 1, 3), dtype=F)
    for b in range(m + 1):
        for a in range(n + 1):
            jx = 0.0 if a in (0, n) else rng.uniform(-0.35, 0.35) * (xs[1] - xs[0])
            jy = 0.0 if b in (0, m) else rng.uniform(-0.35, 0.35) * (ys[1] - ys[0])
            x, y = xs[a] + jx, ys[b] + jy
            P[b, a] = (x, y, 0.5 if zfun is None else zfun(x, y))
    tris = []
    for b in range(m):
        for a in range(n):
            p00, p10, p01, p11 = P[b, a], P[b, a + 1], P[b + 1, a], P[b + 1, a + 1]
            if (a + b) % 2 == 0:
                tris += [[p00, p10, p11], [p00, p11, p01]]
            else:
                tris += [[p00, p10, p01], [p10, p11, p01]]
    return np.ascontiguousarray(np.array(tris, dtype=F))
