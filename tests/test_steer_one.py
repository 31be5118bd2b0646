"""The one-launch steer form, the parts that need no GPU: the constant, the
new entries' argument checks, the descriptor layouts (mosrx_sparams.fused is
appended) and the configuration struct, which stays as it was."""
import ctypes as C
import os
import subprocess

import pytest

import mosrx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -22


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    exe = tmp_path_factory.mktemp("steer_one") / "steer_one_sizes"
    subprocess.check_call(["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "mos-networking-stack_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "steer_one_sizes.c"), "-o", str(exe)])
    names = ("sdesc", "gdesc", "xdesc", "sparams", "side", "fused", "one_max", "cfg", "steer", "direct_frames")
    return dict(zip(names, map(int, subprocess.check_output([str(exe)], text=True).split())))


def test_constant_and_symbols(layout):
    L = mosrx.lib()
    hdr = open(os.path.join(ROOT, "include", "mosrx.h")).read()
    assert "#define MOSRX_STEER_ONE_MAX 65536u" in hdr
    assert mosrx.STEER_ONE_MAX == 65536 == layout["one_max"]
    assert mosrx.STEER_ONE_MAX == 32 * L.mosrx_steer_tile()          # 32 tiles: one workgroup's walk
    for name in ("mosrx_set_steer_one", "mosrx_get_steer_one", "mosrx_steer_one_count",
                 "mosrx_gpu_module_steer_one_count", "mosrx_gpu_module_set_steer_one",
                 "mosrx_gpu_module_get_steer_one", "mosrx_launch_steer"):
        assert hasattr(L, name), name
    assert L.mosrx_abi_version() == 3                                  # additive: the ABI version stands


def test_descriptor_layouts(layout):
    assert (layout["sdesc"], layout["gdesc"], layout["xdesc"]) == (32, 40, 48)
    assert layout["fused"] == layout["side"] + 4                       # appended behind the last field
    assert layout["sparams"] >= layout["fused"] + 4


def test_module_setting_leaves_the_cfg_struct_alone(layout):
    """The backend's setting is a function of the module, not a field: the
    configuration struct has the size and the offsets it had, steer its last field."""
    L = mosrx.lib()
    M = mosrx.ModuleCfg
    assert C.sizeof(M) == layout["cfg"] == 624
    assert (M.steer.offset, M.direct_frames.offset) == (layout["steer"], layout["direct_frames"]) == (620, 616)
    assert not hasattr(M, "steer_one")
    try:
        assert L.mosrx_gpu_module_get_steer_one() == 0                 # off by default
        for v in (1, 2048, mosrx.STEER_ONE_MAX, 0):
            assert L.mosrx_gpu_module_set_steer_one(v) == 0 and L.mosrx_gpu_module_get_steer_one() == v
        assert L.mosrx_gpu_module_set_steer_one(2048) == 0
        # out of range: refused like the other bad values, before anything is opened, and the setting stays
        for bad in (-1, mosrx.STEER_ONE_MAX + 1, -(1 << 31), (1 << 31) - 1):
            assert L.mosrx_gpu_module_set_steer_one(bad) == EINVAL, bad
            assert L.mosrx_gpu_module_get_steer_one() == 2048
    finally:
        L.mosrx_gpu_module_set_steer_one(0)


def test_validation_without_a_gpu():
    L = mosrx.lib()
    assert L.mosrx_set_steer_one(None, 0) == EINVAL
    assert L.mosrx_set_steer_one(None, mosrx.STEER_ONE_MAX + 1) == EINVAL
    assert L.mosrx_get_steer_one(None) == 0
    assert L.mosrx_steer_one_count(None) == 0
    assert L.mosrx_gpu_module_steer_one_count(None) == 0
