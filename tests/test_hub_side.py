"""The hub's side arrays (csrc/hub.c) over a stand-in backend
(tests/csrc/hub_side_stub.c), no GPU: the stub serves MOSRX_PKT_RX_QUEUE_SIDE
from numpy-made queue-major arrays; every core runs mosrx_rx_loop over its own
endpoint on its own thread and asks the endpoint for MOSRX_PKT_RX_MATCH /
RX_FHASH / RX_TCPINFO per frame.  Expected values are the numpy partition.
The stub logs every backend call with its command and thread: every
RX_QUEUE_SIDE call must come from the owner's thread."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import mosrx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOIN_TIMEOUT = 60.0
MAX_ROUNDS = 400000
NONE = 0xFFFFFFFF
HAS_FH, HAS_MT, HAS_TI, HAS_SIDE = 1, 2, 4, 8


class SideBatch(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("qrec", C.c_void_p), ("qoff", C.c_void_p), ("qlen", C.c_void_p),
                ("idx", C.c_void_p), ("qstart", C.c_void_p), ("qfhash", C.c_void_p), ("qmatch", C.c_void_p),
                ("qtcpinfo", C.c_void_p), ("n", C.c_uint32), ("rec_bytes", C.c_uint32)]


class SideCore(C.Structure):
    _fields_ = [("ep", C.c_void_p), ("dev_ioctl", C.c_void_p), ("log", C.c_void_p), ("log_cap", C.c_uint32),
                ("log_n", C.c_uint32), ("bad", C.c_uint32)]


CALL = np.dtype([("tid", "<u8"), ("what", "<u4"), ("cmd", "<i4")])
DELIVERY = np.dtype([("batch", "<u4"), ("orig", "<u4"), ("index", "<i4"), ("has", "<u4"), ("fhash", "<u4"),
                     ("match", "<u4"), ("ti", "u1", 12), ("side_n", "<u4"), ("side_same", "<u4")])


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = tmp_path_factory.mktemp("hub_side_stub") / "libhub_side_stub.so"
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "hub_side_stub.c"), "-o", str(so)])
    S = C.CDLL(str(so))
    S.hub_side_set.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32]
    S.hub_side_set.restype = None
    S.hub_side_calls.restype = C.c_uint32
    S.hub_side_self.restype = C.c_uint64
    S.iom = C.addressof(mosrx.IoModuleFunc.in_dll(S, "hub_side_func"))
    return S


def make_batches(ns, lacks, compact, rng, nq=8):
    """The stub's table and, per batch, (queue, idx, fhash, match, tcpinfo) in
    batch order; batch k lacks the arrays named in lacks[k % len(lacks)]."""
    keep, table, expect = [], (SideBatch * len(ns))(), []
    for k, n in enumerate(ns):
        lack = lacks[k % len(lacks)]
        ln = np.full(n, 64, np.uint16)
        off = (np.arange(n, dtype=np.uint32) * 64).astype(np.uint32)
        frames = np.zeros(64 * n, np.uint8)
        q = rng.integers(0, nq, n).astype(np.uint8)
        res = np.zeros(n, mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE)
        res["queue"] = q
        res["verdict"] = 1
        fh = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        mt = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        ti = rng.integers(0, 256, (n, 12)).astype(np.uint8)
        idx = np.argsort(q, kind="stable").astype(np.uint32)
        qstart = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=256))]).astype(np.uint32)
        qrec, qoff, qlen = res[idx].copy(), off[idx].copy(), ln[idx].copy()
        qfh = None if "fhash" in lack else fh[idx].copy()
        qmt = None if "match" in lack else mt[idx].copy()
        qti = None if "tcpinfo" in lack else ti[idx].copy()
        keep += [frames, qrec, qoff, qlen, idx, qstart, qfh, qmt, qti]
        table[k] = SideBatch(frames.ctypes.data, qrec.ctypes.data, qoff.ctypes.data, qlen.ctypes.data,
                             idx.ctypes.data, qstart.ctypes.data, *[a.ctypes.data if a is not None else None
                                                                    for a in (qfh, qmt, qti)], n, 8 if compact else 16)
        expect.append((q, idx, fh, mt, ti, lack))
    return table, keep, expect


def run_hub(S, table, nb, ncores, side, total):
    """Core 0 on this thread (the owner), cores 1.. on threads of their own, each
    calling mosrx_rx_loop over its endpoint.  (per-core delivery logs, calls, owner tid, bad)."""
    calls = np.zeros(1 << 14, CALL)
    S.hub_side_set(C.addressof(table), nb, side, calls.ctypes.data, len(calls))
    hub = mosrx.Hub(S.iom, None, 1, ncores)
    logs = [np.zeros(total + 1, DELIVERY) for _ in range(ncores)]
    cores = [SideCore(hub.endpoint(c), C.cast(hub.m.dev_ioctl, C.c_void_p), logs[c].ctypes.data, len(logs[c]), 0, 0)
             for c in range(ncores)]
    fn = C.cast(S.hub_side_consume, C.c_void_p)
    done = threading.Event()
    errors = []

    def core_loop(c):
        try:
            for _ in range(MAX_ROUNDS):
                rc, st = hub.run_loop(c, fn, C.byref(cores[c]))
                if rc:
                    errors.append((c, rc))
                    return
                if done.is_set():
                    return
                if st.rx_packets == 0:
                    time.sleep(0.0001)
            errors.append((c, "round limit"))
        except Exception as e:   # noqa: BLE001 -- reported by the main thread
            errors.append((c, repr(e)))

    threads = [threading.Thread(target=core_loop, args=(c,), daemon=True) for c in range(1, ncores)]
    for t in threads:
        t.start()
    try:
        for _ in range(MAX_ROUNDS):
            h0 = hub.stats()
            rc, st = hub.run_loop(0, fn, C.byref(cores[0]))
            assert rc == 0
            hs = hub.stats()
            # an idle round that was the backend's own: every share of the last batch went back
            if hs.frames == total and hs.batches == h0.batches and hs.owner_waits == h0.owner_waits:
                break
            if st.rx_packets == 0:
                time.sleep(0.0001)
        else:
            pytest.fail("the owner never drained the backend")
    finally:
        done.set()
        for t in threads:
            t.join(JOIN_TIMEOUT)
    assert not [t for t in threads if t.is_alive()], "a core's loop did not end: the hub is stuck"
    assert not errors, errors
    assert hub.close() == 0
    ncalls = S.hub_side_calls()
    assert ncalls <= len(calls)
    return [logs[c][:cores[c].log_n] for c in range(ncores)], calls[:ncalls], S.hub_side_self(), [c.bad for c in cores]


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("ncores", [2, 3, 8])
def test_endpoints_serve_their_shares_side_arrays(stub, ncores, compact):
    """Each endpoint's RX_MATCH / RX_FHASH / RX_TCPINFO is its share's run, per
    frame the numpy partition's value; -1 for an array the batch lacks."""
    t = int(mosrx.lib().mosrx_steer_tile())
    ns = [t + 17, 65, 1, 700, 2 * t + 1]
    lacks = [(), ("match",), ("tcpinfo", "fhash"), ("fhash", "match", "tcpinfo"), ("tcpinfo",)]
    rng = np.random.default_rng(300 + ncores)
    table, keep, expect = make_batches(ns, lacks, compact, rng)
    logs, calls, owner, bad = run_hub(stub, table, len(ns), ncores, 1, sum(ns))
    assert bad == [0] * ncores
    for c in range(ncores):
        want = [(k, int(i)) for k, (q, idx, *_) in enumerate(expect) for i in idx[q[idx] == c]]
        assert list(zip(logs[c]["batch"].tolist(), logs[c]["orig"].tolist())) == want, f"core {c}"
        for k, (q, idx, fh, mt, ti, lack) in enumerate(expect):
            d = logs[c][logs[c]["batch"] == k]
            np.testing.assert_array_equal(d["index"], np.arange(len(d)))       # indexed like get_rptr
            has = HAS_SIDE | (0 if "fhash" in lack else HAS_FH) | (0 if "match" in lack else HAS_MT) | \
                (0 if "tcpinfo" in lack else HAS_TI)
            assert (d["has"] == has).all(), f"core {c}, batch {k}"
            assert (d["side_same"] == 1).all() and (d["side_n"] == len(d)).all()
            if has & HAS_FH:
                np.testing.assert_array_equal(d["fhash"], fh[d["orig"]], err_msg=f"core {c}, batch {k}")
            else:
                assert (d["fhash"] == NONE).all()
            if has & HAS_MT:
                np.testing.assert_array_equal(d["match"], mt[d["orig"]], err_msg=f"core {c}, batch {k}")
            else:
                assert (d["match"] == NONE).all()
            if has & HAS_TI:
                np.testing.assert_array_equal(d["ti"], ti[d["orig"]], err_msg=f"core {c}, batch {k}")
    # every backend call, the RX_QUEUE_SIDE ones among them, on the owner's thread
    assert (calls["tid"] == owner).all()
    side_calls = calls[(calls["what"] == 2) & (calls["cmd"] == mosrx.PKT_RX_QUEUE_SIDE)]
    assert len(side_calls) == 1 + len(ns) * ncores        # the probe at open, then one per core and batch
    assert (side_calls["tid"] == owner).all()
    del keep


@pytest.mark.parametrize("ncores", [2, 8])
def test_endpoints_over_a_backend_without_side_views(stub, ncores):
    """Over a stub that answers only RX_QUEUE (a cfg.steer = 2 backend) the hub
    delivers as before and every side ioctl of an endpoint is -1."""
    ns = [700, 65, 2049]
    rng = np.random.default_rng(7)
    table, keep, expect = make_batches(ns, [()], False, rng)
    logs, calls, owner, bad = run_hub(stub, table, len(ns), ncores, 0, sum(ns))
    assert bad == [0] * ncores
    for c in range(ncores):
        want = [(k, int(i)) for k, (q, idx, *_) in enumerate(expect) for i in idx[q[idx] == c]]
        assert list(zip(logs[c]["batch"].tolist(), logs[c]["orig"].tolist())) == want, f"core {c}"
        assert (logs[c]["has"] == 0).all()
    side_calls = calls[(calls["what"] == 2) & (calls["cmd"] == mosrx.PKT_RX_QUEUE_SIDE)]
    assert len(side_calls) == 1 and (calls["tid"] == owner).all()       # the probe alone
    del keep


@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_hub_side_driver_under_sanitizers(tmp_path, san):
    """The stand-alone driver (its own main: the hub over the side stub, cores on
    pthreads) built with a host sanitizer and run on the CPU; nothing is preloaded."""
    exe = tmp_path / ("hub_side_driver_" + san.split(",")[0])
    src = [os.path.join(ROOT, "tests", "csrc", "hub_side_driver.c"),
           os.path.join(ROOT, "tests", "csrc", "hub_side_stub.c"),
           os.path.join(ROOT, "mos-networking-stack_amd", "csrc", "hub.c"),
           os.path.join(ROOT, "mos-networking-stack_amd", "csrc", "rx_loop.c")]
    cmd = ["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=" + san,
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include")] + src + ["-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hub_side_driver ok" in r.stdout
