"""Every iteration of a pcg! call against xref.pcg_step_ref (TEST INFRASTRUCTURE shared by test_xref_cpu.py, which holds
the CPU oracle to it, and test_xref_pcg_gpu.py, which holds the kernels to it).

pcg! keeps nothing between calls, and a call of it=k leaves x_k, r_k and eps_k.  Every sum of the code under test has a
fixed order, so the first k-1 iterations of pcg!(it=k) ARE the run pcg!(it=k-1): `replay` runs it = 1..kmax from the same
start and checks every transition on its own, from the stored T values of the runs before it -- nothing compounds."""
import numpy as np

import xref as X

K = X.K


def _flat(a):
    return np.asarray(a).ravel(order="F")


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b))


def replay(run, inp, D, iD, T, kmax=6, worst=None, key="", controls=True):
    """run(k) -> (n, x, r, eps): host copies after pcg!(it=k) from the start inp["x0"], inp["r0"], inp["z"] (the caller
    restores them).  Checks, for k = 1..kmax, while the reference has not left:
      - every branching scalar of the reference farther from its threshold than its bound;
      - n == k; eps_k (K["pcg_eps"]), x_k and r_k (K["pcg"]) at every inside cell, fed from the runs k-1 and k-2;
      - controls that must fail: the next sample, alpha off by 64 K eps M_alpha/|alpha| (x and r), beta likewise (eps),
        x_{k-2} in place of x_{k-1} (a deferred update applied twice, or never), the periodic shell term dropped;
    and once the reference leaves in iteration j (n_ref updates made):
      - :127 (j = 1): n == 0, x and r untouched;
      - :132: n == j-1, eps_j by the replay, x and r those of the run it=j-1 bit for bit;
      - :138 (after update j): n == j, r and eps those of the run it=j bit for bit, x within K["pcg"] of the replay's x_j
        (with a deferred x the direction kernel owes that update);
      - every later run equals the first run past the exit bit for bit;
      - control: the exit moved by one iteration (the arrays and n of the run one earlier) must not match.
    Returns {"exit": None | (kind, j), "n": [n_1..n_kmax]}; the largest ratios go into `worst` under key + name."""
    worst = {} if worst is None else worst
    L, z, perdir = inp["L"], inp["z"], inp["perdir"]
    runs = {0: (0, inp["x0"], inp["r0"], None)}
    refs = {}
    left = None                                               # (kind, iteration, number of updates)
    ns = []

    def cmp(name, knd, got, ref, k, control=True):
        v, M = ref
        ins = refs[k]["ins"]
        g = _flat(got)[ins]
        w = X.worst(g, v[ins], M[ins], T)
        worst[f"{key}{name}"] = max(worst.get(f"{key}{name}", 0.0), w)
        assert w <= K[knd], f"{key}{name} of iteration {k}: |got-ref| = {w:.3g} eps*M > K = {K[knd]}"
        # (where the reference itself does not tell a sample from the next -- r after the last update of `chains` is zero
        # within the bound at every cell -- that control has nothing to show)
        if control and controls and X.worst(v[ins][:-1], v[ins][1:], M[ins][1:], T) > K[knd]:
            assert X.worst(g[:-1], v[ins][1:], M[ins][1:], T) > K[knd], f"{key}{name} {k}: control (next sample) did not fail"

    def fails(knd, got, ref, ins):
        v, M = ref
        return X.worst(_flat(got)[ins], v[ins], M[ins], T) > K[knd]

    for k in range(1, kmax + 1):
        n, x, r, e = run(k)
        ns.append(n)
        if left is not None:
            kind, j, nref = left
            first = runs[j if kind != ":138" else j + 1]      # the first run past the exit
            assert n == nref, f"{key}it={k}: n = {n}, the reference left through {kind} in iteration {j} after {nref}"
            assert _same(x, first[1]) and _same(r, first[2]) and _same(e, first[3]), f"{key}it={k}: arrays changed after the exit"
            runs[k] = (n, x, r, e)
            continue
        _, xp, rp, ep = runs[k - 1]
        rpp = runs[k - 2][2] if k >= 2 else None
        ref_k = X.pcg_step_ref(L, D, iD, z, perdir, xp, rp, ep, rpp, e, T)
        refs[k] = ref_k
        ins = ref_k["ins"]
        for name, val, thr, bound in ref_k["branch"]:
            assert abs(val - thr) > bound, f"{key}iteration {k}: {name} = {float(val):.6g} within {float(bound):.3g} of {float(thr):.3g}"
        runs[k] = (n, x, r, e)
        if ref_k["exit"] in (":127", ":138"):
            nref = k - 1
            assert n == nref, f"{key}it={k}: n = {n}, the reference leaves through {ref_k['exit']} after {nref}"
            assert _same(r, rp) and (ref_k["exit"] == ":127" or _same(e, ep)), f"{key}it={k}: r or eps changed after {ref_k['exit']}"
            if ref_k["exit"] == ":127":
                assert _same(x, xp)
                left = (":127", 1, 0)
            else:
                cmp("x", "pcg", x, refs[k - 1]["x"], k - 1)    # the owed update: x_j once, neither twice nor never
                left = (":138", k - 1, nref)
                if controls and k >= 3:                       # exit moved one iteration earlier: the run it=j-1
                    assert n != runs[k - 2][0] and not _same(r, runs[k - 2][2]) and not _same(x, runs[k - 2][1])
            continue
        cmp("eps", "pcg_eps", e, ref_k["eps"], k)
        if controls and k >= 2:
            assert fails("pcg_eps", e, X.pcg_step_planted(ref_k, "beta", T)["eps"], ins), f"{key}eps {k}: control (beta) did not fail"
        if ref_k["exit"] == ":132":
            nref = k - 1
            assert n == nref, f"{key}it={k}: n = {n}, the reference leaves through :132 after {nref}"
            assert _same(x, xp) and _same(r, rp), f"{key}it={k}: x or r changed after :132"
            left = (":132", k, nref)
            if controls and k >= 2:                           # exit moved one iteration earlier: the run it=k-2
                assert n != runs[k - 2][0] and not _same(r, runs[k - 2][2]) and not _same(x, runs[k - 2][1])
            continue
        assert n == k, f"{key}it={k}: n = {n}, the reference makes {k} updates"
        cmp("x", "pcg", x, ref_k["x"], k)
        cmp("r", "pcg", r, ref_k["r"], k)
        if controls:
            pl = X.pcg_step_planted(ref_k, "alpha", T)
            assert fails("pcg", x, pl["x"], ins) and fails("pcg", r, pl["r"], ins), f"{key}iteration {k}: control (alpha) did not fail"
            if k >= 2:
                twice = (np.asarray(_flat(runs[k - 2][1]), X.LD) + ref_k["alpha"][0] * ref_k["_eps_k"], ref_k["x"][1])
                assert fails("pcg", x, twice, ins), f"{key}x {k}: control (x of iteration {k - 2}) did not fail"
            if perdir and np.any(np.asarray(z) != 0):
                bare = X.pcg_step_ref(L, D, iD, z, perdir, xp, rp, ep, rpp, e, T, shell=False)
                assert bare["exit"] is not None or fails("pcg", x, bare["x"], ins), f"{key}x {k}: control (no shell term) did not fail"
    return {"exit": None if left is None else left[:2], "n": ns}
