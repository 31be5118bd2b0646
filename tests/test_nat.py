"""NAT translation, the parts that need no GPU: the ABI records against the Python
mirrors, mosrx_nat_check's refusals, the lookup table as the host builds it (every
key found by a walk within the recorded probe bound; a 16-way collision),
mosrx_nat_patch_frame against the restatement (tests/nat_oracle.py), the
checksum arithmetic of csrc/mosrx_nat.h as a stand-alone program (plain and under
-fsanitize=address,undefined), the recorded answers of tests/golden/nat.npz, and
the launch functions' refusals that come before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mosrx
import nat_cases as NC
import nat_oracle as N
import oracle_py as O
from test_fwd_gpu import pack_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nat.npz")
EINVAL = -22
PHASES = [2, 7, 0, 13, 1, 11]


def test_abi_records_and_constants():
    assert mosrx.NAT_BINDING_DTYPE.itemsize == 20 and mosrx.NAT_XLAT_DTYPE.itemsize == 16
    assert [mosrx.NAT_XLAT_DTYPE.fields[k][1] for k in ("addr", "port", "ip_check", "tcp_check", "kind", "ihl", "bind")] == \
        [0, 4, 6, 8, 10, 11, 12]
    assert [mosrx.NAT_SLOT_DTYPE.fields[k][1] for k in ("saddr", "daddr", "ports", "port", "kind", "addr", "bind")] == \
        [0, 4, 8, 12, 14, 16, 20] and mosrx.NAT_SLOT_DTYPE.itemsize == 32
    assert mosrx.NAT_MAX_BINDINGS == 64510 == 65535 - 1025                 # nat.c:244: ports 1025 .. 65534
    assert (mosrx.FWD_NAT_MISS, mosrx.FWD_NAT_HOST) == (7, 8) == (mosrx.FWD_DROP + 1, mosrx.FWD_DROP + 2)
    assert mosrx.OP_FWD_NAT == 15 == mosrx.OP_ACL + 1
    assert mosrx.lib().mosrx_abi_version() == 3                             # additive: the ABI version stands
    L = mosrx.lib()
    for name in ("mosrx_nat_check", "mosrx_nat_set", "mosrx_nat_count", "mosrx_nat_hash", "mosrx_fwd_plan_nat_dev",
                 "mosrx_nat_patch_rings_dev", "mosrx_nat_patch_frame", "mosrx_queue_set_nat", "mosrx_launch_nat_plan",
                 "mosrx_launch_nat_patch"):
        assert hasattr(L, name), name
    for name in ("nat_set", "fwd_plan_nat_dev", "nat_patch_rings_dev"):
        assert callable(getattr(mosrx.Context, name)), name
    assert callable(mosrx.Queue.set_nat) and callable(mosrx.nat_patch_frame)
    b = mosrx.nat_bindings([("10.0.0.1", 1234, "8.8.8.8", 80, 1025)], nat_ip="192.0.2.1")
    assert b[0].tobytes() == bytes([10, 0, 0, 1, 8, 8, 8, 8, 192, 0, 2, 1, 0x04, 0xD2, 0, 80, 0x04, 0x01, 0, 0])


def test_check_refusals():
    L = mosrx.lib()
    ok = mosrx.nat_bindings([("10.0.0.1", 1000 + i, "8.8.8.8", 80, 2000 + i) for i in range(5)], nat_ip="192.0.2.1")
    assert L.mosrx_nat_check(ok.ctypes.data, 5) == 0 and L.mosrx_nat_check(None, 0) == 0
    assert L.mosrx_nat_check(None, 1) == EINVAL
    assert L.mosrx_nat_check(ok.ctypes.data, mosrx.NAT_MAX_BINDINGS + 1) == EINVAL
    for field in ("nat_ip", "nat_port"):
        bad = ok.copy()
        bad[field][3] = 0
        assert L.mosrx_nat_check(bad.ctypes.data, 5) == EINVAL, field
    bad = ok.copy()                                 # two client-side keys equal (the NAT ports differ)
    for k in ("cli_ip", "cli_port", "svr_ip", "svr_port"):
        bad[k][4] = bad[k][1]
    assert L.mosrx_nat_check(bad.ctypes.data, 5) == EINVAL
    bad = ok.copy()                                 # two server-side keys equal (the clients differ)
    bad["nat_port"][4] = bad["nat_port"][1]
    assert L.mosrx_nat_check(bad.ctypes.data, 5) == EINVAL
    with pytest.raises(mosrx.MosrxError):
        mosrx.nat_table(bad)
    with pytest.raises(ValueError):
        mosrx.nat_bindings([("10.0.0.1", 1, "8.8.8.8", 80, 1025)] * (mosrx.NAT_MAX_BINDINGS + 1), nat_ip="192.0.2.1")


def keys_of(b):
    """(saddr, daddr, ports, kind, addr, port) of both keys of every binding, index order."""
    c = np.stack([b["cli_ip"], b["svr_ip"], b["cli_port"].astype(np.uint32) | b["svr_port"].astype(np.uint32) << 16,
                  np.full(len(b), N.SNAT, np.uint32), b["nat_ip"], b["nat_port"].astype(np.uint32)], 1)
    s = np.stack([b["svr_ip"], b["nat_ip"], b["svr_port"].astype(np.uint32) | b["nat_port"].astype(np.uint32) << 16,
                  np.full(len(b), N.DNAT, np.uint32), b["cli_ip"], b["cli_port"].astype(np.uint32)], 1)
    return np.concatenate([c, s]).astype(np.uint32), np.concatenate([np.arange(len(b)), np.arange(len(b))])


def walk(slots, probe, keys):
    """The kernel's lookup on the host: from the key's hash, at most `probe` slots, a free slot ends it.
    Returns the slot found per key (-1: none)."""
    L, mask = mosrx.lib(), len(slots) - 1
    h = np.array([L.mosrx_nat_hash(int(a), int(b), int(c)) for a, b, c in keys[:, :3]], np.uint32)
    found = np.full(len(keys), -1, np.int64)
    looking = np.ones(len(keys), bool)
    for d in range(probe):
        s = slots[(h + np.uint32(d)) & np.uint32(mask)]
        free = looking & (s["kind"] == 0)
        hit = looking & ~free & (s["saddr"] == keys[:, 0]) & (s["daddr"] == keys[:, 1]) & (s["ports"] == keys[:, 2])
        found[hit] = ((h + np.uint32(d)) & np.uint32(mask))[hit]
        looking &= ~(free | hit)
    return found


def big(n):
    i = np.arange(n)
    b = np.zeros(n, mosrx.NAT_BINDING_DTYPE)
    b["cli_ip"] = 10 | (i // 62500) << 8 | (i // 250 % 250) << 16 | (i % 250 + 1) << 24
    b["svr_ip"], b["nat_ip"] = mosrx.ip_raw("198.51.100.7"), mosrx.ip_raw("192.0.2.1")
    b["cli_port"] = ((1000 + i % 60000) & 0xFF) << 8 | (1000 + i % 60000) >> 8
    b["svr_port"] = 80 << 8
    b["nat_port"] = ((1025 + i) & 0xFF) << 8 | (1025 + i) >> 8
    return b


@pytest.mark.parametrize("n", [0, 1, mosrx.NAT_MAX_BINDINGS])
def test_table_build_every_key_found_within_the_probe_bound(n):
    b = big(n)
    slots, probe = mosrx.nat_table(b)
    cap = len(slots)
    assert cap == mosrx.lib().mosrx_nat_slots(n) and cap & (cap - 1) == 0 and cap >= max(4 * n, 16)
    assert (slots["kind"] != 0).sum() == 2 * n and (probe == 0) == (n == 0) and probe <= 64
    keys, idx = keys_of(b)
    at = walk(slots, probe, keys)
    assert (at >= 0).all()
    s = slots[at]
    assert (s["kind"] == keys[:, 3]).all() and (s["addr"] == keys[:, 4]).all() and (s["port"] == keys[:, 5]).all()
    assert (s["bind"] == idx).all()
    if n:
        assert (walk(slots, probe - 1, keys) < 0).any()                  # the bound is the longest run, no more
        miss = keys[:64].copy()
        miss[:, 2] ^= 0x00010000
        assert (walk(slots, probe, miss) < 0).all()


def test_sixteen_bindings_in_one_slot():
    b = NC.bindings()
    coll = b[NC.NPLAIN:NC.NPLAIN + NC.NCOLL]
    L = mosrx.lib()
    hs = {L.mosrx_nat_hash(int(x["cli_ip"]), int(x["svr_ip"]), int(x["cli_port"]) | int(x["svr_port"]) << 16) & 255 for x in coll}
    assert len(coll) == 16 and len(hs) == 1
    slots, probe = mosrx.nat_table(b)
    assert len(slots) == 256 and probe >= 16
    keys, idx = keys_of(b)
    at = walk(slots, probe, keys)
    assert (at >= 0).all() and (slots[at]["bind"] == idx).all()


def oracle_mix(n=513):
    buf, off, ln = pack_at(NC.mix(n), PHASES)
    rec = NC.forced(O.classify(buf, off, ln, O.params(num_msp=1, forward=1)), n)
    t = mosrx.fwd_tables(**NC.TABLES)
    x, pl, tr = N.plan(buf, off, ln, rec["reason"], NC.bindings(), t, 0)
    return buf, off, ln, rec, x, pl, tr


def test_patch_frame_against_the_restatement():
    buf, off, ln, rec, x, pl, tr = oracle_mix()
    xl = np.isin(x["kind"], [N.SNAT, N.DNAT])
    tcp = buf[off.astype(np.int64) + 23] == 6
    tcp &= buf[off.astype(np.int64) + 12] == 8
    assert xl.sum() >= 0.8 * tcp.sum() and {int(k) for k in x["kind"]} == {0, 1, 2, 3, 4}
    assert {5, 6, 15} <= {int(v) for v in x["ihl"][xl]}
    for i in range(len(off)):
        o, n = int(off[i]), int(ln[i])
        got = mosrx.nat_patch_frame(buf[o:o + n], x[i])
        assert got.tobytes() == tr[o:o + n].tobytes(), (i, x[i])
        if not xl[i]:
            assert got.tobytes() == buf[o:o + n].tobytes()
    # the translated frames are valid TCP again: the restatement's checks verify under the oracle's classify
    again = O.classify(tr, off, ln, O.params(num_msp=1, forward=1))
    assert (again["reason"][xl] == mosrx.R["TCP_OK"]).all()


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_checksum_arithmetic_standalone(tmp_path, flags):
    exe = tmp_path / "nat_csum_driver"
    b = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                        "-I" + os.path.join(ROOT, "mos-networking-stack_amd", "csrc"), "-I" + os.path.join(ROOT, "oracle"),
                        os.path.join(ROOT, "tests", "csrc", "nat_csum_driver.c"), os.path.join(ROOT, "oracle", "mosrx_oracle.c"),
                        "-lpthread", "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("checked 60000 ")


def test_golden_answers_are_the_restatement():
    z = np.load(GOLDEN)
    buf, off, ln, rec, x, pl, tr = oracle_mix(int(z["n"][0]))
    assert buf.tobytes() == z["frames"].tobytes() and off.tobytes() == z["off"].tobytes()
    assert rec["reason"].tobytes() == z["reason"].tobytes()
    assert NC.bindings().tobytes() == z["bindings"].tobytes()
    assert x.tobytes() == z["xlat"].tobytes() and pl.tobytes() == z["plan"].tobytes()


def test_launch_functions_refuse_before_any_launch():
    L = mosrx.lib()
    L.mosrx_launch_nat_plan.restype = L.mosrx_launch_nat_patch.restype = C.c_int
    L.mosrx_launch_nat_plan.argtypes = L.mosrx_launch_nat_patch.argtypes = [C.c_void_p, C.c_void_p]
    zero = (C.c_uint8 * 512)()
    assert L.mosrx_launch_nat_plan(None, None) == EINVAL and L.mosrx_launch_nat_patch(None, None) == EINVAL
    assert L.mosrx_launch_nat_plan(zero, None) == EINVAL and L.mosrx_launch_nat_patch(zero, None) == EINVAL
    assert L.mosrx_nat_patch_rings_dev(None, None, None, None, None, None, 1, 1, None) == EINVAL
    assert L.mosrx_fwd_plan_nat_dev(None, None, None, 16, 0, None, None, None) == EINVAL
    assert L.mosrx_queue_set_nat(None, None, None) == EINVAL and L.mosrx_nat_set(None, None, 0) == EINVAL
    assert L.mosrx_nat_count(None) == 0
