"""mosrx_fwd_rings_send (csrc/fwd_tx.c): the rings handed to an io_module_func.
The checks are the stand-alone driver's (tests/csrc/fwd_rings_send_driver.c, its
own main and a recording stub), built plain and with a host sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "csrc", "fwd_rings_send_driver.c"),
       os.path.join(ROOT, "mos-networking-stack_amd", "csrc", "fwd_tx.c")]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_fwd_rings_send_driver(tmp_path, san):
    exe = tmp_path / ("fwd_rings_send_" + (san.split(",")[0] if san else "plain"))
    cmd = ["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if san:
        cmd += ["-fsanitize=" + san, "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    b = subprocess.run(cmd + SRC + ["-o", str(exe)], capture_output=True, text=True)
    if san and b.returncode and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san + " runtime")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_rings_send_driver ok" in r.stdout


def test_library_exports_it():
    import ctypes as C

    import mosrx
    assert isinstance(mosrx.lib().mosrx_fwd_rings_send, C._CFuncPtr)
