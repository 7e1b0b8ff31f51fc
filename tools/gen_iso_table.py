"""Generate the marching-tetrahedra tables of waterlily_amd/csrc/wl_iso.h (Kuhn split of a cube into 6 tetrahedra).

    python tools/gen_iso_table.py            # prints the two constexpr tables; paste them into wl_iso.h

Tetrahedron `tet` belongs to the permutation (p0, p1, p2) of the axes, in lexicographic order; its local corners are
v0 = J, v1 = v0 + e_p0, v2 = v1 + e_p1, v3 = J + (1, 1, 1).  ISO_TET[tet][v] is the cube corner dx + 2 dy + 4 dz of local corner v.
For every (tet, mask) -- bit v of mask set: local corner v is inside (a < c) -- the triangles are those of the rule in
include/wlhip.h (wl_isosurface); a vertex is the code 4 p + q of its edge (local corners p < q).  The last two vertices of a
triangle are swapped where the normal, with every crossing at the midpoint of its edge (exact in halves, so integers after
doubling), would point to the inside: the sign of n . (mean(O) - mean(I)).  ISO_TRI[tet][mask] packs vertex k of the list into
bits 4k .. 4k+3 (k = 0..5) and the number of triangles into bits 24..25.
"""
import itertools


def corners(perm):
    v = [(0, 0, 0)]
    for d in perm[:2]:
        w = list(v[-1])
        w[d] += 1
        v.append(tuple(w))
    return v + [(1, 1, 1)]


def triangles(mask):
    """the unoriented rule: lists of three (p, q) edges"""
    I = [v for v in range(4) if mask >> v & 1]
    O = [v for v in range(4) if not mask >> v & 1]
    e = lambda a, b: (min(a, b), max(a, b))
    if len(I) == 1:
        return [[e(I[0], O[0]), e(I[0], O[1]), e(I[0], O[2])]]
    if len(I) == 3:
        return [[e(I[0], O[0]), e(I[1], O[0]), e(I[2], O[0])]]
    if len(I) == 2:
        q = [e(I[0], O[0]), e(I[0], O[1]), e(I[1], O[1]), e(I[1], O[0])]
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def oriented(perm, mask):
    V = corners(perm)
    I = [v for v in range(4) if mask >> v & 1]
    O = [v for v in range(4) if not mask >> v & 1]
    out = []
    for tri in triangles(mask):
        m = [tuple(V[p][d] + V[q][d] for d in range(3)) for p, q in tri]            # twice the midpoints
        a = [m[1][d] - m[0][d] for d in range(3)]
        b = [m[2][d] - m[0][d] for d in range(3)]
        n = (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
        w = [len(I) * sum(V[v][d] for v in O) - len(O) * sum(V[v][d] for v in I) for d in range(3)]   # |I||O| (mean O - mean I)
        s = sum(n[d] * w[d] for d in range(3))
        assert s != 0
        out.append(tri if s > 0 else [tri[0], tri[2], tri[1]])
    return out


def main():
    perms = list(itertools.permutations(range(3)))
    print("constexpr int ISO_TET[6][4] = {")
    for perm in perms:
        print("    {" + ", ".join(str(x + 2 * y + 4 * z) for x, y, z in corners(perm)) + "},   // " + "".join(map(str, perm)))
    print("};")
    print("constexpr uint32_t ISO_TRI[6][16] = {")
    for perm in perms:
        row = []
        for mask in range(16):
            tris = oriented(perm, mask)
            word = len(tris) << 24
            for k, (p, q) in enumerate(e for t in tris for e in t):
                word |= (4 * p + q) << (4 * k)
            row.append(f"0x{word:07x}u")
        print("    {" + ", ".join(row) + "},")
    print("};")


if __name__ == "__main__":
    main()
