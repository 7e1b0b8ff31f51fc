"""CPU-side checks of the runtime options (wl_set_option): the names in include/wlhip.h, their Python twin `Opt`, the
defaults a freshly loaded library reports, and the `options` context manager.  None of these calls touches the device."""
import json
import os
import re
import subprocess
import sys

import pytest

from waterlily_amd import _lib
from waterlily_amd import sim as S
from waterlily_amd.sim import Opt

RETIRED = (11, 12, 20, 21, 24, 25, 28, 29)
# Ctx::opt as the positional initialiser spelled it before the table of csrc/wl_common.h existed (None: a retired key)
DEFAULTS = [1, 1, 1, 1, 0, 2, 1, 1, 1, 1, 1, None, None, 1, 1, 1, 4, 16, 1, 1, None, None, 1, 1, None, None, 600, 1, None, None, 1, 1]


def test_opt_matches_the_header():
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    header = {m.group(1): int(m.group(2)) for m in re.finditer(r"\bWL_OPT_([A-Z0-9_]+)\s*=\s*(\d+)", txt)}
    assert header == {k.name: int(k) for k in Opt}
    assert len(set(header.values())) == len(header) == 24 and not set(header.values()) & set(RETIRED)


def test_defaults_of_a_freshly_loaded_library():
    code = ("import ctypes as C, json\n"
            "from waterlily_amd import _lib\n"
            "L, v, out = _lib.lib(), C.c_int(), []\n"
            "for k in range(32):\n"
            "    rc = L.wl_get_option(k, C.byref(v))\n"
            "    out.append([rc, v.value if rc == 0 else None])\n"
            "print(json.dumps(out))\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                       cwd=os.path.dirname(os.path.dirname(_lib.HEADER)))
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert [k for k, d in enumerate(DEFAULTS) if d is None] == list(RETIRED)
    for k, (rc, val) in enumerate(got):
        if DEFAULTS[k] is None:
            assert rc == _lib.WL_E_ARG, k
        else:
            assert rc == 0 and val == DEFAULTS[k], (k, val)


def test_keys_by_name_number_and_enum():
    assert _lib.opt_key(Opt.BDIM_IN_CONVDIFF) == _lib.opt_key(27) == _lib.opt_key("27") == 27
    assert _lib.opt_key("BDIM_IN_CONVDIFF") == _lib.opt_key("WL_OPT_BDIM_IN_CONVDIFF") == _lib.opt_key("bdim_in_convdiff") == 27
    assert S.get_option("MBOX_TIMEOUT_S") == S.get_option(Opt.MBOX_TIMEOUT_S) == S.get_option(int(Opt.MBOX_TIMEOUT_S))
    with pytest.raises(_lib.WlError, match="no such option"):
        _lib.opt_key("NO_SUCH_KEY")
    with pytest.raises(_lib.WlError, match="no such option"):
        S.get_option(RETIRED[0])                                   # (refused by the library)


def test_options_restores_the_previous_values():
    a, b = Opt.PCG_DEFER_X, Opt.STREAM_GRID_K
    before = {k: S.get_option(k) for k in Opt}
    assert before[a] == 1 and before[b] == 16
    with S.options({a: 0, "STREAM_GRID_K": 8}):
        assert S.get_option(a) == 0 and S.get_option(b) == 8
    assert {k: S.get_option(k) for k in Opt} == before             # after a normal exit
    with pytest.raises(ZeroDivisionError):
        with S.options({a: 0, b: 8}):
            assert S.get_option(a) == 0 and S.get_option(b) == 8
            1 / 0
    assert {k: S.get_option(k) for k in Opt} == before             # after an exception
    S.set_option(b, 32)                                            # a previous value that is not the default
    try:
        with S.options({b: 8}):
            assert S.get_option(b) == 8
            with S.options({b: 4, a: 0}):                          # nested: each level puts back what IT found
                assert S.get_option(b) == 4 and S.get_option(a) == 0
            assert S.get_option(b) == 8 and S.get_option(a) == 1
        assert S.get_option(b) == 32
        with pytest.raises(ZeroDivisionError):
            with S.options({b: 8}):
                1 / 0
        assert S.get_option(b) == 32
        with pytest.raises(_lib.WlError):                          # a key the library refuses: nothing stays changed
            with S.options({b: 8, RETIRED[0]: 1}):
                pass
        assert S.get_option(b) == 32
    finally:
        S.set_option(b, before[b])
    assert {k: S.get_option(k) for k in Opt} == before
