"""The tile map of the z-marching launches (waterlily_amd/csrc/wl_tilemap.h: which logical tile a physical workgroup takes, and
the slot of that tile's reduction partial), built alone with the host compiler and run under the address and
undefined-behaviour sanitizers: tests/tilemap_host.cpp prints tile_of's results for every workgroup of every launch shape,
under both maps and both sweep directions.  Here every property the kernels rely on is checked with numpy against formulas
restated from the description of the map, not from the header.  No GPU, no HIP."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBLK = (8, 64, 1000, 1024, 4096, 16384, 4100)      # 4100: not a multiple of 8
TPP = (8, 16, 128, 256, 504)
NCHUNK = (1, 3, 8, 12, 16, 32, 64)


def shapes():
    """(nblk, tpp): every listed grid size with every listed tpp (most of them no whole number of chunks: fallback), and
    every grid that IS tpp x nchunk for the listed values"""
    out = [(n, t) for n in NBLK for t in TPP]
    out += [(t * c, t) for t in TPP for c in NCHUNK]
    return sorted(set(out))


def contiguous(nblk, rev):
    """the parent's map: XCD b&7 takes [x*per, (x+1)*per) in order, backwards with rev; slot = the workgroup of rev = 0"""
    b = np.arange(nblk)
    if nblk % 8:
        return b.copy(), b.copy()
    per, x, q = nblk // 8, b & 7, b >> 3
    qq = per - 1 - q if rev else q
    return x * per + qq, (qq << 3) | x


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("tilemap")
    exe = str(tmp / "tilemap_host")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-I", os.path.join(ROOT, "waterlily_amd", "csrc"), os.path.join(ROOT, "tests", "tilemap_host.cpp"),
                         "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    script = tmp / "script.txt"
    script.write_text("".join(f"{n} {t}\n" for n, t in shapes()))
    run = subprocess.run([exe, str(script)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.split("\n")
    assert "tilemap_host ok" in lines
    got, key = {}, None
    for ln in lines:
        w = ln.split()
        if w and w[0] == "case":
            key = tuple(int(x) for x in w[1:5])
            got[key] = {"dealt": int(w[5])}
        elif w and w[0] in ("lb", "slot", "tslot"):
            got[key][w[0]] = np.array(w[1:], dtype=np.int64)
    assert len(got) == 4 * len(shapes())
    return got


def engaged(nblk, tpp):
    return nblk % 8 == 0 and nblk % tpp == 0 and (nblk // tpp) % 8 == 0


def test_the_cases_take_both_paths():
    s = shapes()
    assert any(engaged(n, t) for n, t in s) and any(not engaged(n, t) and n % 8 == 0 for n, t in s) and any(n % 8 for n, t in s)
    assert (4096, 128) in s and (16384, 256) in s          # the two finest-level launch shapes of the 512^3 benchmark
    assert engaged(4096, 128) and engaged(16384, 256) and not engaged(12 * 128, 128) and not engaged(4100, 8)


def test_every_map_is_a_bijection(maps):
    for (nblk, tpp, mp, rev), m in maps.items():
        assert m["lb"].shape == (nblk,) and np.array_equal(np.sort(m["lb"]), np.arange(nblk)), (nblk, tpp, mp, rev)


def test_the_partial_of_a_tile_keeps_its_slot(maps):
    """slot(lb) = the workgroup that takes lb in the contiguous map with rev = 0, whatever the map and the direction; the slots
    are a permutation of [0, nblk) (the partial buffer holds nblk values)"""
    for (nblk, tpp, mp, rev), m in maps.items():
        lb0, b0 = contiguous(nblk, 0)
        slot_of = np.empty(nblk, dtype=np.int64)
        slot_of[lb0] = b0
        assert np.array_equal(m["slot"], slot_of[m["lb"]]), (nblk, tpp, mp, rev)
        assert np.array_equal(m["tslot"], slot_of), (nblk, tpp, mp, rev)
        assert np.array_equal(np.sort(m["slot"]), np.arange(nblk))


def test_contiguous_map_and_fallback_are_the_parents_map(maps):
    for (nblk, tpp, mp, rev), m in maps.items():
        assert m["dealt"] == int(bool(mp) and engaged(nblk, tpp)), (nblk, tpp, mp, rev)
        if not m["dealt"]:
            lb, slot = contiguous(nblk, rev)
            assert np.array_equal(m["lb"], lb) and np.array_equal(m["slot"], slot), (nblk, tpp, mp, rev)


def test_dealt_map_puts_chunk_c_whole_and_in_order_on_xcd_c_mod_8(maps):
    seen = 0
    for (nblk, tpp, mp, rev), m in maps.items():
        if not m["dealt"]:
            continue
        seen += 1
        b = np.arange(nblk)
        inv = np.empty(nblk, dtype=np.int64)
        inv[m["lb"]] = b                                   # the workgroup of logical tile lb = ch*tpp + pt
        wg = inv.reshape(nblk // tpp, tpp)                 # [chunk, pt]
        xcd, q = wg & 7, wg >> 3
        nchunk = nblk // tpp
        assert np.array_equal(xcd, np.broadcast_to((np.arange(nchunk) % 8)[:, None], xcd.shape)), (nblk, tpp, rev)
        step = -1 if rev else 1                            # a chunk's tiles are consecutive on their XCD, in tile order
        assert np.array_equal(np.diff(q, axis=1), np.full((nchunk, tpp - 1), step)), (nblk, tpp, rev)
        # the XCD's chunks x, x+8, x+16, ... follow each other without a gap
        first = q[:, -1] if rev else q[:, 0]
        want = (np.arange(nchunk) // 8) * tpp
        if rev:
            want = (nchunk // 8 - 1 - np.arange(nchunk) // 8) * tpp
        assert np.array_equal(first, want), (nblk, tpp, rev)
    assert seen >= 2 * 10


def test_rev_reverses_each_xcds_order_and_nothing_else(maps):
    for (nblk, tpp, mp, rev), m in maps.items():
        if rev or nblk % 8:
            continue
        r = maps[(nblk, tpp, mp, 1)]
        per, b = nblk // 8, np.arange(nblk)
        mirror = ((per - 1 - (b >> 3)) << 3) | (b & 7)     # same XCD, position counted from the other end
        assert np.array_equal(r["lb"], m["lb"][mirror]) and np.array_equal(r["slot"], m["slot"][mirror]), (nblk, tpp, mp)
    for (nblk, tpp, mp, rev), m in maps.items():
        if nblk % 8:                                       # no XCD structure: identity, either direction
            assert np.array_equal(m["lb"], np.arange(nblk)) and np.array_equal(m["slot"], np.arange(nblk))
