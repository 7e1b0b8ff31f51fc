"""pcg!'s scalar logic (waterlily_amd/csrc/wl_pcg_scalars.h: the one statement of Poisson.jl:127,131-132,135,137-139 that both
the in-kernel gates and the finalize epilogues of op_pcg call), built alone with the host compiler and run under the address
and undefined-behaviour sanitizers: tests/pcg_host.cpp drives a PcgS through after_init -> (after_mult -> after_update)* ->
after_last on scripted dot products.  Here the control flow of Poisson.jl:123-143 is restated with numpy scalars of the
element type and every field after every step is compared exactly.  No GPU, no HIP."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("rho", "alpha", "beta", "r2", "active", "xpend", "nupd", "r2_valid")


def reference(T, xdef, want_r2, it, v):
    """The states after init and after the mult and update step of each of the `it` iterations.  An exit of pcg! is a
    `return` here; the device form has the remaining steps enqueued already, and they do nothing -- except that the
    direction kernel after a :138 exit applies the owed x update, so the next mult step finds xpend cleared."""
    T = np.dtype(T).type
    eps10 = T(10) * np.finfo(T).eps
    s = dict(rho=0.0, alpha=0.0, beta=0.0, r2=0.0, active=1, xpend=0, nupd=0, r2_valid=0)
    trace = []

    def snap():
        trace.append(tuple(s[k] for k in FIELDS))

    def pcg():
        rho = T(v[0])                                    # :126  rho = r⋅z
        s["rho"] = float(rho)
        if abs(rho) < eps10:                             # :127
            return
        snap()
        for i in range(1, it + 1):
            alpha = rho / T(v[2 * i - 1])                # :131  alpha = rho/(z⋅ϵ)
            s["alpha"] = float(alpha)
            if np.float64(abs(alpha)) < 1e-2 or np.float64(abs(alpha)) > 1e2:   # :132 (Float64 literals: the test promotes)
                return
            snap()
            s["nupd"] += 1                               # :133  x += alpha ϵ ; r -= alpha z
            if i == it:                                  # :135
                if want_r2:                              # (solver!: L2(p) right after, :146)
                    s["r2"], s["r2_valid"] = float(T(v[2 * i])), 1
                return
            rho2 = T(v[2 * i])                           # :137  rho2 = r⋅z
            if abs(rho2) < eps10:                        # :138
                s["xpend"] = int(bool(xdef))             # (deferred x: :133's x update of this iteration is still owed)
                return
            s["beta"] = float(rho2 / rho)                # :139
            rho = rho2                                   # :141
            s["rho"] = float(rho)
            snap()

    pcg()
    s["active"] = 0
    while len(trace) < 1 + 2 * it:
        if len(trace) % 2 == 1:                          # a mult step
            s["xpend"] = 0
        snap()
    return trace


def scripts():
    """(T, xdef, want_r2, it, values): every exit, both element types"""
    out = []
    for T, tiny in ((np.float32, 1e-7), (np.float64, 1e-16)):
        full = [0.7300000001, 0.91, 0.41, 0.55, -0.23, -0.31, 0.11, 0.17, 0.05, 0.09, -0.02, -0.05, 0.0123456789]
        for xdef in (1, 0):
            out.append((T, xdef, 0, 6, [tiny] + full[1:]))                      # :127, |rho| < 10 eps
            out.append((T, xdef, 0, 6, [-tiny] + full[1:]))
            out.append((T, xdef, 0, 6, [1.0, 1000.0 / 3] + full[2:]))           # :132, |alpha| < 1e-2
            out.append((T, xdef, 0, 6, [1.0, -1e-3 / 3] + full[2:]))            # :132, |alpha| > 1e2
            out.append((T, xdef, 0, 6, full[:4] + [0.2, 5000.0] + full[6:]))    # :132 in the third iteration
            out.append((T, xdef, 0, 6, full[:2] + [tiny] + full[3:]))           # :138 in the first iteration (xpend = xdef)
            out.append((T, xdef, 1, 6, full[:6] + [-tiny] + full[7:]))          # :138 in the third
            out.append((T, xdef, 0, 6, full))                                   # six iterations, no r.r wanted
            out.append((T, xdef, 1, 6, full))                                   # six iterations, r.r from the last update
            out.append((T, xdef, 1, 1, full[:3]))                               # it = 1: the first update is the last
            # alpha = 1/100: Float32 rounds it to 0.0099999998 (< 1e-2: exit), Float64 keeps 0.01 (not < 1e-2: goes on)
            out.append((T, xdef, 1, 6, [1.0, 100.0] + full[2:]))
    return out


def test_rounding_case_takes_both_sides():
    f32 = reference(np.float32, 1, 1, 6, [1.0, 100.0] + [0.5] * 11)
    f64 = reference(np.float64, 1, 1, 6, [1.0, 100.0] + [0.5] * 11)
    act = FIELDS.index("active")
    assert f32[1][act] == 0 and f64[1][act] == 1


def test_pcg_scalars_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pcg_host")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "waterlily_amd", "csrc"),
                         os.path.join(ROOT, "tests", "pcg_host.cpp"), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    cases = scripts()
    script = tmp_path / "script.txt"
    script.write_text("".join(f"{int(np.dtype(T) == np.float32)} {xdef} {wr2} {it} " + " ".join(float(x).hex() for x in v) + "\n"
                              for T, xdef, wr2, it, v in cases))
    run = subprocess.run([exe, str(script)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.split("\n")
    assert "pcg_host ok" in lines
    got, steps = [], []
    for ln in lines:
        w = ln.split()
        if w and w[0] == "case":
            got.append([])
            steps.append([])
        elif w and w[0] in ("init", "mult", "update", "last"):
            got[-1].append(tuple(float.fromhex(x) for x in w[1:5]) + tuple(int(x) for x in w[5:9]))
            steps[-1].append(w[0])
    assert len(got) == len(cases)
    exits = set()
    for n, ((T, xdef, wr2, it, v), g, st) in enumerate(zip(cases, got, steps)):
        want = reference(T, xdef, wr2, it, v)
        assert st == ["init"] + ["mult", "update"] * (it - 1) + ["mult", "last"]
        for k, (a, b) in enumerate(zip(g, want)):
            assert a == b, f"case {n} ({np.dtype(T).name}, xdef={xdef}, want_r2={wr2}) step {k} ({st[k]}): {dict(zip(FIELDS, a))} != {dict(zip(FIELDS, b))}"
        act = [row[FIELDS.index("active")] for row in want]
        exits.add((np.dtype(T).name, st[act.index(0)], act.index(0), want[act.index(0)][FIELDS.index("xpend")], want[-1][FIELDS.index("r2_valid")]))
    # the scripts really leave through every door: :127 (init), :132 (mult), :138 (update, owed x or not), :135 (last, r.r or not)
    for name in ("float32", "float64"):
        doors = {(e[1], e[3], e[4]) for e in exits if e[0] == name}
        assert {("init", 0, 0), ("mult", 0, 0), ("update", 1, 0), ("update", 0, 0), ("last", 0, 0), ("last", 0, 1)} <= doors, doors
