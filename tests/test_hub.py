"""The hub (csrc/hub.c) over a stand-in steering + gathering backend
(tests/csrc/hub_stub.c), no GPU: every core runs mosrx_rx_loop over its own
endpoint on its own thread; expected shares are plain numpy partitions.  The
stub records every backend call with its thread and with how many frames the
cores had consumed by then, which is how the two rules are checked: only the
owner's thread calls the backend, and the backend's recv_pkts (which takes the
lent batch back) never arrives while a core still holds a share."""
import ctypes as C
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import mosrx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EBUSY, ENOTSUP = -22, -16, -95
QS = 257
CALL_RECV, CALL_IOCTL, CALL_SEND, CALL_RPTR = 1, 2, 3, 4
JOIN_TIMEOUT = 60.0
MAX_ROUNDS = 400000


class StubBatch(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("qrec", C.c_void_p), ("qoff", C.c_void_p), ("qlen", C.c_void_p),
                ("idx", C.c_void_p), ("qstart", C.c_void_p), ("n", C.c_uint32), ("rec_bytes", C.c_uint32)]


class StubCore(C.Structure):
    _fields_ = [("ep", C.c_void_p), ("dev_ioctl", C.c_void_p), ("log", C.c_void_p), ("log_cap", C.c_uint32),
                ("log_n", C.c_uint32), ("sleep_us", C.c_uint32), ("sleep_every", C.c_uint32), ("bad", C.c_uint32)]


CALL = np.dtype([("tid", "<u8"), ("consumed", "<u8"), ("what", "<u4"), ("cur", "<i4")])
DELIVERY = np.dtype([("batch", "<u4"), ("orig", "<u4"), ("index", "<i4"), ("len", "<u4"), ("sum", "<u4"),
                     ("rec", "u1", 16)])


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = tmp_path_factory.mktemp("hub_stub") / "libhub_stub.so"
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "hub_stub.c"), "-o", str(so)])
    S = C.CDLL(str(so))
    S.hub_stub_set.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32]
    S.hub_stub_set.restype = None
    S.hub_stub_calls.restype = C.c_uint32
    S.hub_stub_exhausted.restype = C.c_uint32
    S.hub_stub_consumed.restype = C.c_uint64
    S.hub_stub_self.restype = C.c_uint64
    S.iom = C.addressof(mosrx.IoModuleFunc.in_dll(S, "hub_stub_func"))
    return S


def keys_of(pattern, n, rng):
    i = np.arange(n)
    if pattern == "mod3":
        return (i % 3).astype(np.uint8)
    return rng.integers(0, 8, n).astype(np.uint8)


def make_batches(ns, pattern, compact, rng):
    """The stub's table (queue-major arrays by numpy) and, per batch, what a
    core must see: (queue, idx, record as rx_loop hands it, len, byte sum)."""
    keep, table, expect = [], (StubBatch * len(ns))(), []
    for k, n in enumerate(ns):
        ln = rng.integers(60, 200, n).astype(np.uint16)
        off = np.concatenate([[0], np.cumsum(ln[:-1].astype(np.uint32))]).astype(np.uint32)
        frames = rng.integers(0, 256, int(ln.sum())).astype(np.uint8)
        q = keys_of(pattern, n, rng)
        res = np.zeros(n, mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE)
        res["rss"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        res["queue"] = q
        res["verdict"] = 1
        res["reason"] = rng.integers(0, 4, n).astype(np.uint8)
        res["tcp_flags"] = rng.integers(0, 256, n).astype(np.uint8)
        if not compact:
            res["payloadlen"] = rng.integers(0, 1500, n).astype(np.uint16)
        idx = np.argsort(q, kind="stable").astype(np.uint32)
        qstart = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=256))]).astype(np.uint32)
        qrec, qoff, qlen = res[idx].copy(), off[idx].copy(), ln[idx].copy()
        keep += [frames, qrec, qoff, qlen, idx, qstart]
        table[k] = StubBatch(frames.ctypes.data, qrec.ctypes.data, qoff.ctypes.data, qlen.ctypes.data,
                             idx.ctypes.data, qstart.ctypes.data, n, 8 if compact else 16)
        # what mosrx_rx_loop hands the consumer: the 16-byte record, or the compact one's fields in it
        full = np.zeros(n, mosrx.RESULT_DTYPE)
        for f in (("rss", "reason", "queue", "verdict", "tcp_flags") if compact else mosrx.RESULT_DTYPE.names):
            full[f] = res[f]
        sums = np.add.reduceat(frames.astype(np.uint32), off).astype(np.uint32)
        expect.append((q, idx, full.view(np.uint8).reshape(n, 16), ln, sums))
    return table, keep, expect


def run_hub(S, table, nb, ncores, slow_core=None):
    """Core 0 on this thread (the owner), cores 1.. on threads of their own,
    each calling mosrx_rx_loop over its endpoint for a bounded number of rounds.
    Returns (per-core delivery logs, calls, hub stats, close codes, owner tid)."""
    calls = np.zeros(1 << 16, CALL)
    S.hub_stub_set(C.addressof(table), nb, 1, calls.ctypes.data, len(calls))
    hub = mosrx.Hub(S.iom, None, 1, ncores)
    ioctl = hub.m.dev_ioctl
    logs = [np.zeros(1 << 15, DELIVERY) for _ in range(ncores)]
    cores = [StubCore(hub.endpoint(c), ioctl, logs[c].ctypes.data, len(logs[c]), 0,
                      200 if c == slow_core else 0, 8, 0) for c in range(ncores)]
    fn = C.cast(S.hub_stub_consume, C.c_void_p)
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
    # the owner: first one batch only (max_pkts = 1 ends the loop after the round that reached it)
    rc, st = hub.run_loop(0, fn, C.byref(cores[0]), max_pkts=1)
    assert rc == 0 and st.batches == 1
    busy = hub.close()
    for _ in range(MAX_ROUNDS):
        if S.hub_stub_exhausted():
            break
        rc, st = hub.run_loop(0, fn, C.byref(cores[0]))
        assert rc == 0
        if st.rx_packets == 0:
            time.sleep(0.0001)
    done.set()
    for t in threads:
        t.join(JOIN_TIMEOUT)
    stuck = [t for t in threads if t.is_alive()]
    assert not stuck, "a core's loop did not end: the hub is stuck"
    assert S.hub_stub_exhausted(), "the owner never drained the backend"
    assert not errors, errors
    stats = hub.stats()
    closed = hub.close()
    ncalls = S.hub_stub_calls()
    assert ncalls <= len(calls)
    return ([logs[c][:cores[c].log_n] for c in range(ncores)], calls[:ncalls], stats, (busy, closed),
            S.hub_stub_self(), [c.bad for c in cores])


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("pattern", ["mod3", "random"])
@pytest.mark.parametrize("ncores", [1, 2, 4])
def test_hub_delivers_each_cores_partition(stub, ncores, pattern, compact):
    t = mosrx.lib().mosrx_steer_tile()
    ns = [3 * t + 17, 65, t + 1, 1, 700]
    rng = np.random.default_rng(100 + ncores)
    table, keep, expect = make_batches(ns, pattern, compact, rng)
    logs, calls, stats, (busy, closed), owner, bad = run_hub(stub, table, len(ns), ncores,
                                                              slow_core=ncores - 1 if ncores > 1 else None)
    assert bad == [0] * ncores
    # each core's sequence of (batch, original index, record, frame) is the numpy partition
    for c in range(ncores):
        want = [(k, int(i)) for k, (q, idx, _, _, _) in enumerate(expect) for i in idx[q[idx] == c]]
        got = list(zip(logs[c]["batch"].tolist(), logs[c]["orig"].tolist()))
        assert got == want, f"core {c}"
        for k, (q, idx, rec, ln, sums) in enumerate(expect):
            d = logs[c][logs[c]["batch"] == k]
            np.testing.assert_array_equal(d["index"], np.arange(len(d)))       # the share is a contiguous ring
            np.testing.assert_array_equal(d["rec"], rec[d["orig"]])
            np.testing.assert_array_equal(d["len"], ln[d["orig"]])
            np.testing.assert_array_equal(d["sum"], sums[d["orig"]])
    # frames of queues >= ncores: counted, handed to nobody
    owned = [int((q < ncores).sum()) for q, *_ in expect]
    assert stats.batches == len(ns) and stats.frames == sum(ns)
    assert stats.delivered == sum(owned) == sum(len(lg) for lg in logs)
    assert stats.unowned == sum(ns) - sum(owned)
    if pattern == "random" or ncores < 3:
        assert stats.unowned > 0
    # only the owner's thread called the backend, and never get_rptr
    assert (calls["tid"] == owner).all()
    assert not (calls["what"] == CALL_RPTR).any()
    # no recv_pkts while a core still held a share: the k-th recv_pkts (which takes
    # batch k - 1 back) found every frame of batches 0 .. k - 1 consumed
    recv = calls[calls["what"] == CALL_RECV]
    assert len(recv) == len(ns) + 1
    np.testing.assert_array_equal(recv["consumed"], np.concatenate([[0], np.cumsum(owned)]))
    if ncores > 1:
        assert stats.owner_waits > 0        # the slow core made the owner idle, not block
    assert busy == EBUSY and closed == 0
    del keep


def test_hub_open_validation(stub):
    L = mosrx.lib()
    h = C.c_void_p()
    calls = np.zeros(64, CALL)
    stub.hub_stub_set(None, 0, 1, calls.ctypes.data, len(calls))
    assert L.mosrx_hub_open(None, None, 1, 2, C.byref(h)) == EINVAL
    assert L.mosrx_hub_open(stub.iom, None, 0, 2, C.byref(h)) == EINVAL
    assert L.mosrx_hub_open(stub.iom, None, 1, 0, C.byref(h)) == EINVAL
    assert L.mosrx_hub_open(stub.iom, None, 1, 65, C.byref(h)) == EINVAL
    assert L.mosrx_hub_open(stub.iom, None, 1, 2, None) == EINVAL
    assert L.mosrx_hub_close(None) == EINVAL
    assert L.mosrx_hub_endpoint(None, 0) is None
    # a backend that steers but does not gather
    stub.hub_stub_set(None, 0, 0, calls.ctypes.data, len(calls))
    assert L.mosrx_hub_open(stub.iom, None, 1, 2, C.byref(h)) == ENOTSUP and not h.value
    # a backend that gathers: endpoints for its cores only; an idle backend is an idle round
    stub.hub_stub_set(None, 0, 1, calls.ctypes.data, len(calls))
    hub = mosrx.Hub(stub.iom, None, 1, 2)
    assert hub.endpoint(0) and hub.endpoint(1) and hub.endpoint(0) != hub.endpoint(1)
    assert L.mosrx_hub_endpoint(hub.handle, 2) is None
    rc, st = hub.run_loop(0)
    assert rc == 0 and st.rx_packets == 0 and st.rounds == 1
    rc, st = hub.run_loop(1)
    assert rc == 0 and st.rx_packets == 0
    assert hub.close() == 0


def test_owner_endpoint_refuses_other_threads(stub):
    """Core 0's endpoint is the only caller of the backend, on the opening
    thread: from another thread its recv_pkts is an error, and the backend
    sees no call."""
    rng = np.random.default_rng(5)
    table, keep, _ = make_batches([100], "mod3", False, rng)
    calls = np.zeros(256, CALL)
    stub.hub_stub_set(C.addressof(table), 1, 1, calls.ctypes.data, len(calls))
    hub = mosrx.Hub(stub.iom, None, 1, 2)
    before = stub.hub_stub_calls()
    out = []
    t = threading.Thread(target=lambda: out.append(hub.run_loop(0)), daemon=True)
    t.start()
    t.join(JOIN_TIMEOUT)
    assert not t.is_alive()
    rc, st = out[0]
    assert rc == 0 and st.recv_errors == 1 and st.rx_packets == 0
    assert stub.hub_stub_calls() == before
    assert hub.close() == 0
    del keep


@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_hub_driver_under_sanitizers(tmp_path, san):
    """The stand-alone driver (its own main: the hub over the same stub, cores on
    pthreads) built with a host sanitizer and run on the CPU."""
    exe = tmp_path / ("hub_driver_" + san.split(",")[0])
    src = [os.path.join(ROOT, "tests", "csrc", "hub_driver.c"), os.path.join(ROOT, "tests", "csrc", "hub_stub.c"),
           os.path.join(ROOT, "mos-networking-stack_amd", "csrc", "hub.c"),
           os.path.join(ROOT, "mos-networking-stack_amd", "csrc", "rx_loop.c")]
    cmd = ["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=" + san,
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include")] + src + ["-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    if b.returncode and ("cannot find" in b.stderr or "unrecognized" in b.stderr):
        pytest.skip("this toolchain has no -fsanitize=" + san + " runtime")
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "hub_driver ok" in r.stdout
