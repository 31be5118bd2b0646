"""mosrx_fwd_desc_send (csrc/fwd_tx.c): the descriptor rings and the received
batch handed to an io_module_func, equal call for call and byte for byte to
mosrx_fwd_rings_send over the byte rings of the same entries.  The checks are
the stand-alone driver's (tests/csrc/fwd_desc_send_driver.c, its own main and a
recording stub), built plain and with a host sanitizer."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "tests", "csrc", "fwd_desc_send_driver.c"),
       os.path.join(ROOT, "mos-networking-stack_amd", "csrc", "fwd_tx.c")]


@pytest.mark.parametrize("san", [None, "address,undefined"])
def test_fwd_desc_send_driver(tmp_path, san):
    exe = tmp_path / ("fwd_desc_send_" + (san.split(",")[0] if san else "plain"))
    cmd = ["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include")]
    if san:
        cmd += ["-fsanitize=" + san, "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
        # the sanitizer runtime is looked for with a program of no content: a failure
        # to build the code under test is then never taken for a missing runtime
        probe = tmp_path / "probe.c"
        probe.write_text("int main(void) { return 0; }\n")
        p = subprocess.run(["gcc", "-fsanitize=" + san, str(probe), "-o", str(tmp_path / "probe")],
                           capture_output=True, text=True)
        if p.returncode:
            pytest.skip("this toolchain has no -fsanitize=" + san + " runtime")
    b = subprocess.run(cmd + SRC + ["-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fwd_desc_send_driver ok" in r.stdout


def test_library_exports_the_new_symbols():
    import ctypes as C

    import mosrx
    L = mosrx.lib()
    for name in ("mosrx_fwd_desc_send", "mosrx_fwd_desc_rings_dev", "mosrx_fwd_desc_scratch_bytes",
                 "mosrx_queue_set_fwd_desc"):
        assert isinstance(getattr(L, name), C._CFuncPtr), name
    assert mosrx.OP_FWD_DESC == 13
