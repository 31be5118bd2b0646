"""Queue steering, the parts that need no GPU: the new entries' argument
validation, the scratch size, the exported symbols, the configuration field,
and mosrx_rx_loop_queues over a stand-in io_module_func (tests/csrc/steer_stub.c)
whose ioctl serves idx / qstart computed by numpy."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mosrx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOTSUP = -22, -95
QS = 257


def test_constants_and_symbols():
    L = mosrx.lib()
    assert mosrx.STEER_QSLOTS == QS and mosrx.OP_STEER == 7 and mosrx.PKT_RX_STEER == 0x19
    hdr = open(os.path.join(ROOT, "include", "mosrx.h")).read()
    assert "#define MOSRX_STEER_QSLOTS 257" in hdr and "MOSRX_OP_STEER = 7" in hdr
    assert "#define MOSRX_ABI_VERSION 3" in hdr and L.mosrx_abi_version() == 3
    for name in ("mosrx_steer_scratch_bytes", "mosrx_steer_dev", "mosrx_queue_set_steer", "mosrx_slot_steer",
                 "mosrx_rx_loop_queues", "mosrx_steer_tile"):
        assert hasattr(L, name), name
    t = L.mosrx_steer_tile()
    assert t % 64 == 0 and 64 <= t <= 4096


def test_scratch_bytes_needs_no_gpu_and_grows():
    L = mosrx.lib()
    t = L.mosrx_steer_tile()
    ns = [0, 1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17, 32768, 65536, 1 << 20, 0x7FFFFFFF, 0xFFFFFFFF]
    got = [L.mosrx_steer_scratch_bytes(n) for n in ns]
    assert all(g > 0 and g % 4 == 0 for g in got)
    assert got == sorted(got)
    # one histogram row of 256 u32 per tile of frames
    assert got[ns.index(3 * t + 17)] >= 4 * 256 * 4
    assert got[-1] >= (0xFFFFFFFF // t) * 1024


def test_validation_without_a_context():
    L = mosrx.lib()
    buf = (C.c_uint32 * 1024)()
    p = C.addressof(buf)
    sb = L.mosrx_steer_scratch_bytes(4)
    assert L.mosrx_steer_dev(None, p, 4, 16, p, p, p, sb, None) == EINVAL
    assert L.mosrx_queue_set_steer(None, None, None, None) == EINVAL
    assert L.mosrx_slot_steer(None, 0, None, None) == EINVAL
    tot = C.c_float()
    b = mosrx.Batch()
    outs = (C.c_void_p * 1)(p)
    assert L.mosrx_time_op(None, mosrx.OP_STEER, 16, C.byref(b), 1, outs, outs, 1, 1, C.byref(tot), None) == EINVAL
    assert L.mosrx_time_op_dispatch(None, mosrx.OP_STEER, 16, C.byref(b), 1, outs, outs, 1, C.byref(tot)) == EINVAL


def test_module_cfg_steer_is_last_and_off_by_default():
    L = mosrx.lib()
    cfg = mosrx.ModuleCfg()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    L.mosrx_gpu_module_cfg_default(C.byref(cfg))
    assert cfg.steer == 0
    assert mosrx.ModuleCfg._fields_[-1][0] == "steer"
    assert mosrx.ModuleCfg.steer.offset == mosrx.ModuleCfg.direct_frames.offset + 4


class StubBatch(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("off", C.c_void_p), ("len", C.c_void_p), ("res", C.c_void_p),
                ("idx", C.c_void_p), ("qstart", C.c_void_p), ("n", C.c_uint32), ("compact", C.c_uint32)]


DELIVERY = np.dtype([("arg", "<u8"), ("ifidx", "<i4"), ("index", "<i4"), ("len", "<u4"), ("queue", "u1"),
                     ("first_byte", "u1"), ("batch", "<u2")])


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    so = tmp_path_factory.mktemp("steer_stub") / "libsteer_stub.so"
    subprocess.check_call(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared",
                           "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "csrc", "steer_stub.c"), "-o", str(so)])
    S = C.CDLL(str(so))
    S.steer_stub_set.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_uint32]
    S.steer_stub_set.restype = None
    S.steer_stub_delivered.restype = C.c_uint32
    S.steer_stub_sends.restype = C.c_uint32
    S.iom = C.addressof(mosrx.IoModuleFunc.in_dll(S, "steer_stub_func"))
    return S


def make_batches(ns, nq, compact, rng):
    """Batches of ns frames with random queues below nq: the stub's table, the
    arrays it points into (kept alive by the caller) and the queues."""
    keep, table, queues = [], (StubBatch * len(ns))(), []
    for k, n in enumerate(ns):
        ln = rng.integers(60, 200, n).astype(np.uint16)
        off = (np.concatenate([[0], np.cumsum(ln[:-1].astype(np.uint32))]) if n else np.zeros(0)).astype(np.uint32)
        frames = rng.integers(0, 256, int(ln.sum()) + 1).astype(np.uint8)
        q = rng.integers(0, nq, n).astype(np.uint8)
        res = np.zeros(n, mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE)
        res["queue"] = q
        res["verdict"] = 1
        idx = np.argsort(q, kind="stable").astype(np.uint32)
        qstart = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=256))]).astype(np.uint32)
        keep += [ln, off, frames, res, idx, qstart]
        table[k] = StubBatch(frames.ctypes.data, off.ctypes.data, ln.ctypes.data, res.ctypes.data,
                             idx.ctypes.data, qstart.ctypes.data, n, int(compact))
        queues.append((q, ln, frames, off))
    return table, keep, queues


def run_loop(S, table, nb, nq_cfg, nq_loop, steer=1, fn=True, args=None, max_rounds=0, cap=1 << 16):
    log = np.zeros(cap, DELIVERY)
    S.steer_stub_set(C.addressof(table), nb, nq_cfg, steer, log.ctypes.data, cap)
    st = mosrx.RxStats()
    a = (C.c_void_p * max(nq_loop, 1))(*(args if args is not None else [1000 + q for q in range(max(nq_loop, 1))]))
    rc = mosrx.lib().mosrx_rx_loop_queues(S.iom, None, 1, nq_loop,
                                          C.cast(S.steer_stub_consume, C.c_void_p) if fn else None, a, max_rounds,
                                          C.byref(st))
    return rc, st, log[:min(S.steer_stub_delivered(), cap)]


@pytest.mark.parametrize("compact", [False, True])
def test_rx_loop_queues_over_stub(stub, compact):
    """Every frame is delivered exactly once, to arg[queue], indices ascending
    within each queue, queue 0 first; per batch."""
    nq = 5
    ns = [1, 64, 300, 4097]
    rng = np.random.default_rng(7)
    table, keep, queues = make_batches(ns, nq, compact, rng)
    rc, st, log = run_loop(stub, table, len(ns), nq, nq)
    assert rc == 0
    assert st.rx_packets == sum(ns) == len(log) and st.batches == len(ns) and st.rx_errors == 0
    assert st.rounds == len(ns) + 1 and stub.steer_stub_sends() == st.rounds
    for k, (q, ln, frames, off) in enumerate(queues):
        d = log[log["batch"] == k]
        assert sorted(d["index"].tolist()) == list(range(ns[k]))            # exactly once
        np.testing.assert_array_equal(d["arg"], 1000 + q[d["index"]].astype(np.uint64))   # to its queue's consumer
        np.testing.assert_array_equal(d["queue"], q[d["index"]])
        np.testing.assert_array_equal(d["len"], ln[d["index"]])
        np.testing.assert_array_equal(d["first_byte"], frames[off[d["index"]]])
        np.testing.assert_array_equal(d["index"], np.argsort(q, kind="stable"))   # queue by queue, ascending within
    assert st.rx_bytes == sum(int(ln.sum()) + 24 * len(ln) for _, ln, _, _ in queues)
    del keep


def test_rx_loop_queues_fewer_consumers_and_round_limit(stub):
    """Frames of queues >= nq are counted and handed to nobody; max_rounds ends the loop."""
    rng = np.random.default_rng(8)
    table, keep, queues = make_batches([500, 500], 8, False, rng)
    rc, st, log = run_loop(stub, table, 2, 8, 3)
    assert rc == 0 and st.rx_packets == 1000
    assert len(log) == sum(int((q < 3).sum()) for q, _, _, _ in queues)
    assert (log["queue"] < 3).all()
    rc, st, log = run_loop(stub, table, 2, 8, 8, max_rounds=1)
    assert rc == 0 and st.rounds == 1 and st.rx_packets == 500 == len(log)
    rc, st, log = run_loop(stub, table, 2, 8, 8, fn=False)      # no consumer: the census only
    assert rc == 0 and st.rx_packets == 1000 and len(log) == 0
    del keep


def test_rx_loop_queues_validation(stub):
    rng = np.random.default_rng(9)
    table, keep, _ = make_batches([10], 2, False, rng)
    L = mosrx.lib()
    st = mosrx.RxStats()
    a = (C.c_void_p * 2)(1, 2)
    iom = stub.iom
    fn = C.cast(stub.steer_stub_consume, C.c_void_p)
    stub.steer_stub_set(C.addressof(table), 1, 2, 1, None, 0)
    assert L.mosrx_rx_loop_queues(None, None, 1, 2, fn, a, 0, C.byref(st)) == EINVAL
    assert L.mosrx_rx_loop_queues(iom, None, 0, 2, fn, a, 0, C.byref(st)) == EINVAL
    assert L.mosrx_rx_loop_queues(iom, None, 1, 0, fn, a, 0, C.byref(st)) == EINVAL
    assert L.mosrx_rx_loop_queues(iom, None, 1, 257, fn, a, 0, C.byref(st)) == EINVAL
    assert L.mosrx_rx_loop_queues(iom, None, 1, 2, fn, None, 0, C.byref(st)) == EINVAL
    assert L.mosrx_rx_loop_queues(iom, None, 1, 2, fn, a, 0, None) == EINVAL
    # a backend that does not steer (its ioctl returns -1 for MOSRX_PKT_RX_STEER)
    rc, _, log = run_loop(stub, table, 1, 2, 2, steer=0)
    assert rc == ENOTSUP and len(log) == 0
    del keep
