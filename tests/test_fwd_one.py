"""The one-launch forwarding form, the parts that need no GPU: the constant,
the new entry points and their mirrors, their argument checks, the module's
setting, and the new parameter struct's layout as a C compiler sees it against
a Python mirror and the size csrc/mosrx_fwd.h pins.  (A context needs a GPU: its
setting's round trip is in tests/test_fwd_one_gpu.py.)"""
import ctypes as C
import os
import subprocess

import pytest

import mosrx
from test_fwd_queue import FDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, U32, I32 = C.c_void_p, C.c_uint32, C.c_int32
EINVAL = -22


class DDesc(C.Structure):
    """mosrx_ddesc (csrc/mosrx_fwd.h): a batch as the descriptor store reads it."""
    _fields_ = [(k, P) for k in ("frames", "off", "plan", "tx_src", "tx_len", "tx_mac", "rings")] + \
               [(k, U32) for k in ("frames_bytes", "n", "tile_base", "pad")]


class OParams(C.Structure):
    """mosrx_oparams: the launch parameters of the one-launch form."""
    _fields_ = [("fdesc", P), ("ddesc", P), ("tab", P), ("nb", U32), ("rec_bytes", U32), ("forward", I32),
                ("num_msp", U32), ("listener", U32), ("nrings", U32), ("onef", FDesc), ("oned", DDesc)]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fwd_one") / "fwd_one_layout"
    b = subprocess.run(["gcc", "-O0", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "mos-networking-stack_amd", "csrc"),
                        os.path.join(ROOT, "tests", "csrc", "fwd_one_layout.c"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr                      # (the header's _Static_asserts hold, too)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return {k: int(v) for k, v in (line.rsplit(" ", 1) for line in r.stdout.splitlines())}


def test_constant_symbols_and_mirrors(layout):
    L = mosrx.lib()
    hdr = open(os.path.join(ROOT, "include", "mosrx.h")).read()
    assert "#define MOSRX_FWD_ONE_MAX 8192u" in hdr
    assert mosrx.FWD_ONE_MAX == 8192 == layout["MOSRX_FWD_ONE_MAX"]
    assert mosrx.FWD_ONE_MAX == 32 * layout["MOSRX_FWD_TILE"] == 32 * L.mosrx_fwd_tile()   # 32 tiles: one workgroup's walk
    for name in ("mosrx_set_fwd_one", "mosrx_get_fwd_one", "mosrx_fwd_one_count", "mosrx_gpu_module_set_fwd_one",
                 "mosrx_gpu_module_get_fwd_one", "mosrx_gpu_module_fwd_one_count", "mosrx_launch_fwd_one"):
        assert hasattr(L, name), name
    for name in ("set_fwd_one", "get_fwd_one", "fwd_one_count"):
        assert callable(getattr(mosrx.Context, name)), name
    assert callable(mosrx.GpuBackend.fwd_one_count)
    import inspect
    assert inspect.signature(mosrx.GpuBackend.__init__).parameters["fwd_one"].default == 0
    # the prototypes: a 64-bit count, an unsigned limit
    assert L.mosrx_fwd_one_count.restype is C.c_uint64 and L.mosrx_gpu_module_fwd_one_count.restype is C.c_uint64
    assert L.mosrx_get_fwd_one.restype is C.c_uint32 and L.mosrx_set_fwd_one.argtypes[1] is C.c_uint32
    assert L.mosrx_abi_version() == 3                                  # additive: the ABI version stands


def test_parameter_struct_layout(layout):
    want = {}
    for name, t in (("mosrx_oparams", OParams), ("mosrx_ddesc", DDesc)):
        want[f"sizeof({name})"] = C.sizeof(t)
        for k, _ in t._fields_:
            want[f"{name}.{k}"] = getattr(t, k).offset
    assert {k: layout[k] for k in want} == want
    assert layout["sizeof(mosrx_oparams)"] == 216                      # the size csrc/mosrx_fwd.h pins
    # the queue form's pinned sizes stay as they are
    assert (layout["sizeof(mosrx_fdesc)"], layout["sizeof(mosrx_fqparams)"]) == (96, 56) == (C.sizeof(FDesc), 56)
    assert (layout["sizeof(mosrx_ddesc)"], layout["sizeof(mosrx_dqparams)"]) == (72, 40)


def test_module_setting(layout):
    """A setting of the module, not a field of its configuration struct, whose size stands."""
    L = mosrx.lib()
    assert C.sizeof(mosrx.ModuleCfg) == 624 and not hasattr(mosrx.ModuleCfg, "fwd_one")
    try:
        assert L.mosrx_gpu_module_get_fwd_one() == 0                   # off by default
        for v in (0, 1, 256, mosrx.FWD_ONE_MAX):
            assert L.mosrx_gpu_module_set_fwd_one(v) == 0 and L.mosrx_gpu_module_get_fwd_one() == v
        assert L.mosrx_gpu_module_set_fwd_one(256) == 0
        for bad in (mosrx.FWD_ONE_MAX + 1, -1, -(1 << 31), (1 << 31) - 1):
            assert L.mosrx_gpu_module_set_fwd_one(bad) == EINVAL, bad
            assert L.mosrx_gpu_module_get_fwd_one() == 256            # the old value is kept
    finally:
        L.mosrx_gpu_module_set_fwd_one(0)
    assert L.mosrx_gpu_module_fwd_one_count(None) == 0


def test_validation_without_a_gpu():
    L = mosrx.lib()
    for v in (0, 1, mosrx.FWD_ONE_MAX, mosrx.FWD_ONE_MAX + 1, 0xFFFFFFFF):
        assert L.mosrx_set_fwd_one(None, v) == EINVAL
    assert L.mosrx_get_fwd_one(None) == 0
    assert L.mosrx_fwd_one_count(None) == 0
    # the launch function refuses before it launches: no parameters, no tables, no batch, bad sizes
    L.mosrx_launch_fwd_one.restype = C.c_int
    L.mosrx_launch_fwd_one.argtypes = [C.POINTER(OParams), P]
    assert L.mosrx_launch_fwd_one(None, None) == EINVAL
    op = OParams(nb=1, nrings=4)
    assert L.mosrx_launch_fwd_one(C.byref(op), None) == EINVAL       # tab NULL
    op.tab = 0x1000
    for kw in (dict(nb=0), dict(nrings=0), dict(nrings=17), dict(rec_bytes=4), dict(nb=2)):
        bad = OParams.from_buffer_copy(op)
        for k, v in kw.items():
            setattr(bad, k, v)
        assert L.mosrx_launch_fwd_one(C.byref(bad), None) == EINVAL, kw
    op.oned.n = mosrx.FWD_ONE_MAX + 1                                 # one workgroup walks at most 32 tiles
    op.oned.rings = 0x2000
    assert L.mosrx_launch_fwd_one(C.byref(op), None) == EINVAL
    op.oned.n = 0
    op.oned.rings = 0x2008                                            # 16-byte alignment
    assert L.mosrx_launch_fwd_one(C.byref(op), None) == EINVAL
