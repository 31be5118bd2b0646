"""The batch-queue form of forwarding (mosrx_queue_set_fwd), without a GPU: the
layout of its structures as a C compiler sees them against the Python mirror
and the sizes csrc/mosrx_fwd.h asserts, and the entry point's argument check."""
import ctypes as C
import os
import subprocess

import mosrx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, I32, U64 = C.c_void_p, C.c_uint32, C.c_int32, C.c_uint64


class FDesc(C.Structure):
    """mosrx_fdesc (csrc/mosrx_fwd.h): a queue's batch as the forwarding kernels read it."""
    _fields_ = [(k, P) for k in ("frames", "off", "len", "rec", "plan", "tx", "tx_off", "tx_len", "tx_src", "rings")] + \
               [(k, U32) for k in ("frames_bytes", "n", "in_ifidx", "tile_base")]


class FQParams(C.Structure):
    """mosrx_fqparams: the launch parameters of the queue form."""
    _fields_ = [("desc", P), ("tab", P), ("scratch", P), ("nb", U32), ("total_tiles", U32), ("rec_bytes", U32),
                ("forward", I32), ("num_msp", U32), ("listener", U32), ("nrings", U32), ("cap_units", U32)]


MIRROR = {"mosrx_queue_fwd": mosrx.QueueFwd, "mosrx_fdesc": FDesc, "mosrx_fqparams": FQParams}


def test_layout_matches_c(tmp_path):
    exe = tmp_path / "fwd_queue_layout"
    b = subprocess.run(["gcc", "-O0", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "mos-networking-stack_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "fwd_queue_layout.c"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr                      # (the header's _Static_asserts hold, too)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = dict(line.rsplit(" ", 1) for line in r.stdout.splitlines())
    want = {}
    for name, t in MIRROR.items():
        want[f"sizeof({name})"] = str(C.sizeof(t))
        for k, _ in t._fields_:
            want[f"{name}.{k}"] = str(getattr(t, k).offset)
    assert got == want
    # the sizes csrc/mosrx_fwd.h pins, and the public structure's
    assert (got["sizeof(mosrx_fdesc)"], got["sizeof(mosrx_fqparams)"], got["sizeof(mosrx_queue_fwd)"]) == ("96", "56", "72")


def test_entry_point_checks_its_arguments():
    L = mosrx.lib()
    assert isinstance(L.mosrx_queue_set_fwd, C._CFuncPtr)
    f = mosrx.QueueFwd()
    assert L.mosrx_queue_set_fwd(None, None, C.byref(f)) == -22     # EINVAL: no context, no queue
    assert L.mosrx_queue_set_fwd(None, None, None) == -22
