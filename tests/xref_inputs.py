"""Adversarial inputs shared by the xref checks (test_xref_cpu.py against the oracle, test_xref_gpu.py and
test_xref_step_gpu.py against the kernels)."""
import itertools

import numpy as np

KINDS = ["random", "ties", "step", "scaled-up", "scaled-down"]


def field(shape, T, kind, seed, lo=-1.0, hi=1.0, seam=64):
    """random: uniform in [lo,hi); ties: values in {-1,-1/2,0,1/2,1} (exact median ties, u == 0 faces); step: two levels
    with fronts along x at the x-tile seams (every `seam` cells from 1) and along y/z at index 4; scaled-*: random times
    2^±20 (Float32) / 2^±60 (Float64)."""
    rng = np.random.default_rng(seed)
    T = np.dtype(T)
    if kind == "ties":
        a = rng.integers(-2, 3, size=shape) * 0.5
    elif kind == "step":
        ix = np.indices(shape[:3] if len(shape) >= 3 else shape)
        x = ix[0]
        s = ((x - 1) // seam) % 2 + (ix[1] >= 4)
        if len(ix) > 2:
            s = s + (ix[2] >= 4)
        s = s.astype(np.float64)
        a = np.broadcast_to(s.reshape(s.shape + (1,) * (len(shape) - s.ndim)), shape) - 1.0 + 0.01 * rng.random(shape)
    else:
        a = lo + (hi - lo) * rng.random(shape)
        if kind == "scaled-up":
            a = a * 2.0 ** (20 if T == np.float32 else 60)
        elif kind == "scaled-down":
            a = a * 2.0 ** (-20 if T == np.float32 else -60)
    return np.asfortranarray(np.asarray(a, dtype=T))


def coefficients(Ng, T, seed, kind="body", edge=None, seam=64):
    """Face coefficients L (Ng + (D,)) in [0.2, 1] with a body: a block of L = 0 cells (solid, iD = 0 there), and with
    kind="row" a unit field where one x-row differs in a single coefficient: edge in {"f1","f2","seam","n-2","n-1","y","z"}
    picks the row's first and second free x face (0-based 2, 3), the face at x = seam + 1, the last two free faces (0-based
    n0-3, n0-2), or L_y[j+1] / L_z[k+1]."""
    D = len(Ng)
    rng = np.random.default_rng(seed)
    if kind == "row":
        L = np.ones(Ng + (D,), T, order="F")
        j, k = min(2, Ng[1] - 2), (min(2, Ng[2] - 2) if D == 3 else None)
        row = (slice(None), j) + ((k,) if D == 3 else ())
        n0 = Ng[0]
        # 0-based index of the x face: BC! keeps 0 on faces 0, 1 and n0-1, so the row's first free face is 2
        i = {"f1": 2, "f2": 3, "seam": min(seam + 1, n0 - 2), "n-2": n0 - 3, "n-1": n0 - 2}.get(edge)
        if i is not None:
            L[(i,) + row[1:] + (0,)] = T(0.75)
        elif edge == "y":
            L[(min(3, n0 - 2), j + 1) + ((k,) if D == 3 else ()) + (1,)] = T(0.75)
        elif edge == "z" and D == 3:
            L[(min(3, n0 - 2), j, k + 1, 2)] = T(0.75)
        keep = L.copy()
    else:
        L = np.asfortranarray((0.2 + 0.8 * rng.random(Ng + (D,))).astype(T))
        blk = tuple(slice(max(1, n // 3), max(2, n // 3 + 2)) for n in Ng)
        L[blk] = 0                                         # a solid block: its cells have D = 0, iD = 0
    # BC!(L, 0): zero normal coefficient on planes 1, 2 and N, zero-Neumann tangential ghosts (util.jl:192-210)
    for c in range(D):
        for j in range(D):
            sl = lambda q: tuple(q if d == j else slice(None) for d in range(D)) + (c,)
            if c == j:
                for q in (0, 1, Ng[j] - 1):
                    L[sl(q)] = 0
            else:
                L[sl(0)] = L[sl(1)]
                L[sl(Ng[j] - 1)] = L[sl(Ng[j] - 2)]
    if kind == "row" and edge is not None:
        assert np.any(L == T(0.75)) and np.any(keep == T(0.75)), "the odd coefficient must survive BC!"
    return L



def device_cells(tensors: dict, idx, N, NA=None):
    """xref.Cells over device fields (any strides, padded or dense): the values are gathered on the device by flat
    offset -- int64 throughout, C4 vector fields span more than 2^32 elements -- and copied to the host."""
    import torch
    import xref as X
    base = {}
    for k, t in tensors.items():
        span = 1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))
        base[k] = (torch.as_strided(t, (span,), (1,), t.storage_offset()), t.stride())
    D = len(N)

    def get(name, ix, c):
        b, st = base[name]
        off = sum(torch.as_tensor(a, device=b.device) * st[d] for d, a in enumerate(ix))
        if c is not None:
            off = off + c * st[D]
        return b[off].cpu().numpy()
    return X.Cells(idx, N, get, NA)


def samples(Ng, nrand, seed, row_step=None):
    """Inside cells of a grid of extents Ng (ghosts included) to compare at: `nrand` random cells; the x rows of the planes
    k = 1, 2, mid, N-1, N (1-based inside planes, every `row_step`-th row: all rows when None); every inside plane of four
    (i, j) columns -- every z-chunk seam -- among them the last row's last cell, the highest addresses of a field."""
    rng = np.random.default_rng(seed)
    n0, n1, n2 = Ng
    out = [tuple(rng.integers(1, n - 1, size=nrand) for n in Ng)]
    step = row_step or 1
    for k in sorted({1, 2, n2 // 2, n2 - 3, n2 - 2}):
        i, j = np.meshgrid(np.arange(1, n0 - 1), np.arange(1, n1 - 1, step), indexing="ij")
        j = np.where(j == j.max(), n1 - 2, j)                     # the last row always in
        out.append((i.ravel(), j.ravel(), np.full(i.size, k)))
    k = np.arange(1, n2 - 1)
    for i, j in ((1, 1), (n0 // 2, n1 // 3), (n0 - 2, 1), (n0 - 2, n1 - 2)):
        out.append((np.full(k.size, i), np.full(k.size, j), k))
    return tuple(np.concatenate([o[d] for o in out]).astype(np.int64) for d in range(3))


def step_fields(Ng, T, seed, block):
    """Start of a mom_step! check on a grid of extents Ng (ghosts included): a non-uniform velocity u (x component
    1 + 0.3*random, the others 0.3*random) and a synthetic body inside `block` (one slice per dimension, clear of the
    ghost cells): mu0 in [0.3, 1], mu1 in [-0.3, 0.3], V in [-0.4, 0.4] there -- the rows through it are busy, every other
    row is body-free (mu0 = 1, mu1 = 0, V = 0).  mu0 carries BC!(mu0, 0): zero normal coefficient on planes 1, 2 and N."""
    D = len(Ng)
    rng = np.random.default_rng(seed)
    T = np.dtype(T)
    u = 0.3 * (2 * rng.random(Ng + (D,)) - 1)
    u[..., 0] += 1.0
    mu0 = np.ones(Ng + (D,))
    mu1 = np.zeros(Ng + (D, D))
    V = np.zeros(Ng + (D,))
    nb = tuple(s.stop - s.start for s in block)
    mu0[block] = 0.3 + 0.7 * rng.random(nb + (D,))
    mu1[block] = 0.3 * (2 * rng.random(nb + (D, D)) - 1)
    V[block] = 0.4 * (2 * rng.random(nb + (D,)) - 1)
    for c in range(D):
        for q in (0, 1, Ng[c] - 1):
            mu0[tuple(q if d == c else slice(None) for d in range(D)) + (c,)] = 0
    return {k: np.asfortranarray(a.astype(T)) for k, a in (("u", u), ("mu0", mu0), ("mu1", mu1), ("V", V))}


def project_scale(Ng) -> float:
    """The velocity scale of project_fields: project!'s solver stops on the ABSOLUTE sum of r^2 over the grid (tol = 1e-4,
    Poisson.jl:168, MultiLevelPoisson.jl:95), and on a long box the restarted six-step pcg! of a single level needs
    hundreds of iterations to bring a residual down by a decade.  So the amplitude s (a power of two: scaling is exact)
    keeps the START near the tolerance, n_cells * s^2 <= 2^-8: the oracle then needs 1 to 3 iterations on every case of
    the project! checks (at n_cells * s^2 <= 2^-7 a single-level 18x11 grid takes 5).  Every check is relative to eps * M,
    which scales with s."""
    n = int(np.prod(Ng))
    return 2.0 ** -int(np.ceil((8 + np.log2(n)) / 2))


def body_block(Ng):
    """The block of make_step (test_xref_step_gpu.py) for any extents: across the x seam at cell 64 where the grid reaches
    it (else from mid-length), y from 2 to mid-height, every inside plane"""
    x0 = min(58, max(1, Ng[0] // 2))
    out = [slice(x0, max(x0 + 1, min(71, Ng[0] - 2))), slice(min(2, Ng[1] - 2), max(min(2, Ng[1] - 2) + 1, Ng[1] // 2 + 1))]
    if len(Ng) == 3:
        out.append(slice(1, Ng[2] - 1))
    return tuple(out)


def project_fields(Ng, T, kind, seed, block, perdir=()):
    """Start of a project! check on a grid of extents Ng (ghosts included): a velocity of the given `kind` (field above:
    random, ties, step, ...) times project_scale(Ng), the body of step_fields in `block` (mu0 is the solver's L: rows through
    the block have varying coefficients, every other row is coefficient-uniform), a random start pressure p (ghost cells
    included: the solver never writes the non-periodic ones), and BC! applied as mom_step! does before project!: u with
    U = (scale, 0, ..), mu0 with 0 -- in a periodic direction the normal coefficient of planes 1, 2 and N stays 1."""
    import xref as X
    D = len(Ng)
    s = project_scale(Ng)
    h = step_fields(Ng, T, seed, block)
    for c in perdir:
        for q in (0, 1, Ng[c] - 1):
            h["mu0"][tuple(q if d == c else slice(None) for d in range(D)) + (c,)] = 1
    h["mu0"] = X.BC(h["mu0"], (0.0,) * D, False, perdir)
    u = field(Ng + (D,), T, kind, seed + 1) * np.dtype(T).type(s)
    h["u"] = X.BC(u, (s,) + (0.0,) * (D - 1), False, perdir)
    h["p"] = X.perBC(field(Ng, T, "random", seed + 2) * np.dtype(T).type(s), perdir)
    h["U"] = (s,) + (0.0,) * (D - 1)
    return h


# ------------------------------------------------------------------------------------------------ pcg! replay inputs
# Each returns a dict of host arrays on a grid of extents Ng (ghosts included): L, the start x0 and r0 (ghost cells of r
# are 0: outside(p.r) ≡ 0, Poisson.jl:146), the z to upload, and "perdir".

def _zero_ghosts(a):
    for d in range(a.ndim):
        ix = [slice(None)] * a.ndim
        ix[d] = [0, a.shape[d] - 1]
        a[tuple(ix)] = 0
    return a


def pcg_body(Ng, T, seed, kind="body", edge=None, seam=64, perdir=(), solid=True):
    """`coefficients` bodies and row cases, a random x0 (not zero), a random r, a random z of order 1 everywhere (pcg! never
    reads what is uploaded inside; the ghost cells count where perBC! fills eps).  With periodic directions L is
    BC!(L, 0, false, perdir) of the random field with its solid block: a periodic operator, coupled across the seam.
    solid=False (grids of a handful of cells, where pcg! converges within the six iterations): no solid block, so the cells
    are one connected set, and the mean of r over them is removed -- r then has no component along the constant vector, on
    which A eps = 0 and alpha = rho/(z.eps) is a quotient of two rounding errors that no bound could place."""
    import xref as X
    D = len(Ng)
    if not solid:
        rng = np.random.default_rng(seed)
        L = np.asfortranarray((0.2 + 0.8 * rng.random(Ng + (D,))).astype(T))
        L = X.BC(L, (0.0,) * D, False, ())
        r = _zero_ghosts(field(Ng, T, "random", seed + 2))
        ins = tuple(slice(1, n - 1) for n in Ng)
        r[ins] -= np.dtype(T).type(r[ins].astype(np.float64).mean())
        return {"L": L, "x0": field(Ng, T, "random", seed + 1), "r0": r, "z": field(Ng, T, "random", seed + 3), "perdir": ()}
    if perdir:
        rng = np.random.default_rng(seed)
        L = np.asfortranarray((0.2 + 0.8 * rng.random(Ng + (D,))).astype(T))
        L[tuple(slice(max(1, n // 3), max(2, n // 3 + 2)) for n in Ng)] = 0
        L = X.BC(L, (0.0,) * D, False, perdir)
    else:
        L = coefficients(Ng, T, seed, kind, edge, seam)
    return {"L": L, "x0": field(Ng, T, "random", seed + 1), "r0": _zero_ghosts(field(Ng, T, "random", seed + 2)),
            "z": field(Ng, T, "random", seed + 3), "perdir": tuple(perdir)}


def pcg_chains(Ng, T, seed, axis=1):
    """L is non-zero only on the `axis` faces inside disjoint triples of cells (inside indices 1-3, 4-6, ... along `axis`,
    in every line of cells), with random dyadic coefficients k/8, k = 2..8; r is dyadic (multiples of 1/16) and sums to
    zero over each triple; x0 is dyadic too.  A triple is a weighted path of three vertices, whose Jacobi-preconditioned
    operator has the eigenvalues {0, 1, 2} whatever the weights, and r has no component along the null vector: pcg! makes
    exactly two updates, after which r is zero up to rounding, and leaves through :138 in iteration 2.  Cells outside the
    triples have D = 0, iD = 0 and r = 0."""
    D = len(Ng)
    rng = np.random.default_rng(seed)
    L = np.zeros(Ng + (D,), T, order="F")
    r = np.zeros(Ng, T, order="F")
    nt = (Ng[axis] - 2) // 3
    assert nt >= 1, "chains need three inside cells along the axis"
    other = tuple(n - 2 for d, n in enumerate(Ng) if d != axis)
    for t in range(nt):
        a = 1 + 3 * t
        at = lambda q: tuple(q if d == axis else slice(1, n - 1) for d, n in enumerate(Ng))
        for f in (a + 1, a + 2):                              # the face between cells f-1 and f belongs to cell f
            L[at(f) + (axis,)] = rng.integers(2, 9, size=other) / 8.0
        ra, rb = (rng.integers(-8, 9, size=other) / 16.0 for _ in range(2))
        ra = np.where((ra == 0) & (rb == 0), 0.5, ra)
        r[at(a)], r[at(a + 1)], r[at(a + 2)] = ra, rb, -(ra + rb)
    x0 = np.asfortranarray((rng.integers(-8, 9, size=Ng) / 8.0).astype(T))
    return {"L": L, "x0": x0, "r0": r, "z": field(Ng, T, "random", seed + 3), "perdir": ()}


def pcg_wave(Ng, T):
    """A fully periodic box with unit coefficients and r = cos(2π 8i/n) + 0.01 cos(2π i/n) over the n = Ng[0] - 2 inside
    cells of x (n = 32: waves 4 and 32 cells long), constant in the other directions; z and x0 are zero.  The first
    iteration removes the short wave (alpha_1 = 3 in 3-D: A has the eigenvalue -2 there, iD = -1/6); the second direction
    is the long wave, whose Rayleigh quotient is 0.0064, so alpha_2 is about 156 > 100: pcg! leaves through :132 in
    iteration 2 after one update."""
    D = len(Ng)
    n = Ng[0] - 2
    i = np.arange(n)
    w = np.cos(2 * np.pi * (n // 4) * i / n) + 0.01 * np.cos(2 * np.pi * i / n)
    r = np.zeros(Ng, T, order="F")
    r[tuple(slice(1, m - 1) for m in Ng)] = w.reshape((n,) + (1,) * (D - 1)).astype(T)
    zero = np.zeros(Ng, T, order="F")
    return {"L": np.ones(Ng + (D,), T, order="F"), "x0": zero.copy(order="F"), "r0": r, "z": zero, "perdir": tuple(range(D))}


def pcg_cases(T):
    """The cases of the per-iteration pcg! checks on the kernels (test_xref_pcg_gpu.py; test_xref_cpu.py runs the oracle
    through the same inputs, the 4096-row ones excepted, so that their branch margins are checked without a GPU): dicts of
    id, group, dims (interior extents) and make() -> the inputs.  V = 4 (Float32) / 2 (Float64) cells per 16-B vector.
      first   x = V, V+1 (no vector kernels: scalar, finalize launches), 63V, 64V, 65V; y = 3..9; z = 2..6
      small   (V-1, 5, 1) (five cells in Float64: pcg! converges and leaves, see pcg_body's solid=False) and 2-D: scalar
              kernels, one plane
      long    (V, 4, 40): 320 partials, more than one pass of a 256-thread sum; (V, 4, 131): the cap of 128 z chunks binds
      tall    (V, 4096, 3): the largest plane of the in-kernel sums (1024 workgroups, one chunk); (V, 4100, 3): the first
              that falls back to the finalize launches on a vector level (1032)
      rows    (65V, 5, 4) uniform except one coefficient at the first face, the x seam and the last face of a row
      chains  x = 64V and 65V with triples along y, x = 65V with triples along z
      wave    32 cells in x
      periodic  body coefficients with perdir (0,), (1, 2) and (0, 1, 2), z uploaded with ghost values of order 1; extents at
              which the shell sum's partials (blocks of 256 cells of the largest plane, per plane) are no multiple of 8"""
    v = 4 if np.dtype(T) == np.float32 else 2
    out = []

    def add(group, dims, make):
        q = len(out)
        out.append({"id": f"{group}-{'x'.join(map(str, dims))}-{q}", "group": group, "dims": tuple(dims),
                    "make": (lambda: make(tuple(n + 2 for n in dims), 700 + 10 * q))})
    for s in [(v, 4, 2), (v + 1, 9, 3), (63 * v, 8, 5), (64 * v, 3, 6), (65 * v, 5, 5)]:
        add("first", s, lambda Ng, sd: pcg_body(Ng, T, sd))
    add("small", (v - 1, 5, 1), lambda Ng, sd: pcg_body(Ng, T, sd, solid=False))
    add("small", (7, 6), lambda Ng, sd: pcg_body(Ng, T, sd))
    for s in [(v, 4, 40), (v, 4, 131)]:
        add("long", s, lambda Ng, sd: pcg_body(Ng, T, sd))
    for s in [(v, 4096, 3), (v, 4100, 3)]:
        add("tall", s, lambda Ng, sd: pcg_body(Ng, T, sd))
    for edge in ("f1", "seam", "n-1"):
        add("rows", (65 * v, 5, 4), lambda Ng, sd, edge=edge: pcg_body(Ng, T, sd, "row", edge, seam=64 * v))
    for s, ax in [((64 * v, 6, 3), 1), ((65 * v, 7, 4), 1), ((65 * v, 4, 6), 2)]:
        add("chains", s, lambda Ng, sd, ax=ax: pcg_chains(Ng, T, sd, ax))
    add("wave", (32, 4, 3), lambda Ng, sd: pcg_wave(Ng, T))
    for s, per in [((65 * v, 3, 3), (0,)), ((3 * v, 6, 5), (1, 2)), ((65 * v, 3, 3), (0, 1, 2)), ((3 * v, 6, 5), (0, 1, 2))]:
        add("periodic", s, lambda Ng, sd, per=per: pcg_body(Ng, T, sd, perdir=per))
    return out


def periodic_subsets(D):
    """every non-empty set of periodic directions of a D-dimensional grid"""
    return [p for n in range(1, D + 1) for p in itertools.combinations(range(D), n)]
