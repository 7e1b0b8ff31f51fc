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


def periodic_subsets(D):
    """every non-empty set of periodic directions of a D-dimensional grid"""
    return [p for n in range(1, D + 1) for p in itertools.combinations(range(D), n)]
