"""wl::Buf (waterlily_amd/csrc/wl_buf.h), the owner of every block the library allocates, built alone with the host compiler
and run under the address and undefined-behaviour sanitizers: tests/buf_host.cpp is the program, with its own main and an
allocator over malloc that counts live blocks and fails on request.  No GPU, no HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_buf_under_sanitizers(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "buf_host")
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-I", os.path.join(ROOT, "waterlily_amd", "csrc"), os.path.join(ROOT, "tests", "buf_host.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buf_host ok" in run.stdout
