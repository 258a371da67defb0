"""csrc/qoc_devbuf.hpp on the host: tests/host/devbuf_check.cpp (a stand-alone program that includes the header alone)
compiled with hipcc and run.  It walks allocate, grow, release, move-in and scope exit, asks for SIZE_MAX / 2 bytes
among them, and after every call checks that a pointer is null exactly when the size is 0, that the ledger is the sum
of the live counted buffers, that a failed grow leaves the buffer empty and that a second release is a no-op.  Without
a device every allocation fails and the same invariants hold; with one the successful paths run too.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "devbuf_check.cpp")


def test_devbuf_invariants(tmp_path):
    hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.fail("hipcc not found (the library itself is built with it)")
    exe = str(tmp_path / "devbuf_check")
    subprocess.run([hipcc, "-std=c++17", "-O1", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout
    assert "0 violation(s)" in r.stdout
