"""Queue steering on the GPU (mosrx_steer_dev, mosrx_queue_set_steer,
mosrx_slot_steer, cfg.steer): the stable partition of a batch's frame indices
by its records' queue byte.  The expected value needs no reference code:

    idx    == argsort(queue, kind="stable")
    qstart == concatenate([[0], cumsum(bincount(queue, minlength=256))])

both compared exactly; end to end `queue` comes from the oracle's records.
Every output buffer carries a 64-byte sentinel behind its last element, checked
after the launches."""
import ctypes as C

import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_direct_gpu import _pinned_like, _stage

pytestmark = pytest.mark.gpu

QS = mosrx.STEER_QSLOTS
GUARD = 64
SENT = 0xA5
BIG = 1 << 30


def tile() -> int:
    return int(mosrx.lib().mosrx_steer_tile())


def expect(queue: np.ndarray):
    q = np.asarray(queue, np.int64)
    idx = np.argsort(q, kind="stable").astype(np.uint32)
    qstart = np.concatenate([[0], np.cumsum(np.bincount(q, minlength=256))]).astype(np.uint32)
    return idx, qstart


class Guarded:
    """A device buffer of `nbytes` + a 64-byte sentinel behind it, all sentinel-filled."""

    def __init__(self, ctx, nbytes: int):
        self.nbytes = nbytes
        self.buf = mosrx.DevBuffer(ctx, nbytes + GUARD)
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.nbytes + GUARD, SENT, np.uint8))

    @property
    def ptr(self):
        return self.buf.ptr

    def read(self, dtype=np.uint32) -> np.ndarray:
        raw = self.buf.download(np.zeros(self.nbytes + GUARD, np.uint8))
        assert (raw[self.nbytes:] == SENT).all(), "sentinel behind the buffer overwritten"
        return raw[:self.nbytes].view(dtype).copy()

    def free(self):
        self.buf.free()


def steer_dev(ctx, d_rec: int, n: int, rb: int):
    """mosrx_steer_dev over device records into guarded buffers: (idx, qstart)."""
    sb = int(mosrx.lib().mosrx_steer_scratch_bytes(n))
    idx, qs, scr = Guarded(ctx, 4 * n), Guarded(ctx, 4 * QS), Guarded(ctx, sb)
    try:
        ctx.steer_dev(d_rec, n, rb, idx.ptr, qs.ptr, scr.ptr, sb)
        scr.read(np.uint8)
        return idx.read(), qs.read()
    finally:
        for g in (idx, qs, scr):
            g.free()


def sizes():
    t = tile()
    return [1, 63, 64, 65, t - 1, t, t + 1, 3 * t + 17]


def keys_of(pattern: str, n: int, rng) -> np.ndarray:
    i = np.arange(n)
    if pattern == "one":          # config S's single flow: every frame on one queue
        return np.full(n, 5, np.uint8)
    if pattern.startswith("mod"):
        return (i % int(pattern[3:])).astype(np.uint8)
    if pattern == "random":
        return rng.integers(0, 256, n).astype(np.uint8)
    if pattern == "last":         # one key on every frame but the last
        k = np.full(n, 200, np.uint8)
        k[-1] = 3
        return k
    raise ValueError(pattern)


@pytest.mark.parametrize("rb", [8, 16])
@pytest.mark.parametrize("pattern", ["one", "mod2", "mod3", "mod8", "mod256", "random", "last"])
def test_steer_dev_synthetic(gpu_ctx, rb, pattern):
    """Chosen key bytes in records whose other bytes are random (a wrong key offset
    shows), every size around the wave and the tile."""
    assert tile() % 64 == 0 and tile() <= 4096
    rng = np.random.default_rng(1234 + rb)
    for n in sizes():
        rec = rng.integers(0, 256, (n, rb)).astype(np.uint8)
        key = keys_of(pattern, n, rng)
        rec[:, rb - 3] = key
        d = mosrx.DevBuffer(gpu_ctx, rec.nbytes)
        try:
            d.upload(rec)
            idx, qs = steer_dev(gpu_ctx, d.ptr, n, rb)
        finally:
            d.free()
        eidx, eqs = expect(key)
        np.testing.assert_array_equal(qs, eqs, err_msg=f"qstart n={n}")
        np.testing.assert_array_equal(idx, eidx, err_msg=f"idx n={n}")


@pytest.fixture(scope="module")
def imix():
    return mosrx.Trace(mosrx.TRACE_IMIX, 2 * tile() + 100, nflows=1000)


@pytest.mark.parametrize("nq,mode", [(8, 1), (8, 0), (3, 1)])
def test_steer_real_records(gpu_ctx, imix, nq, mode):
    """Records the classify kernels wrote (both queue maps, a queue count that
    is no power of two), steered from the 16-byte and the compact form."""
    t = imix
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=nq, queue_mode=mode))
    assert len(np.unique(ora["queue"])) == nq
    eidx, eqs = expect(ora["queue"])
    assert (eqs[nq:] == t.n).all()
    db = None
    try:
        gpu_ctx.set_params(mosrx.default_params(num_queues=nq, queue_mode=mode))
        db = gpu_ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
        gpu_ctx.classify_dev(db)
        gpu_ctx.classify_dev_compact(db)
        np.testing.assert_array_equal(db.results()["queue"], ora["queue"])
        for rb, ptr in ((16, db.d_out.ptr), (8, db.d_out8.ptr)):
            idx, qs = steer_dev(gpu_ctx, ptr, t.n, rb)
            np.testing.assert_array_equal(qs, eqs, err_msg=f"rec_bytes {rb}")
            np.testing.assert_array_equal(idx, eidx, err_msg=f"rec_bytes {rb}")
    finally:
        gpu_ctx.set_params(mosrx.default_params())
        if db is not None:
            db.free()


@pytest.mark.parametrize("compact", [False, True])
def test_queue_steer(gpu_ctx, compact):
    """Three batches of T + 5, 1 and 2T frames in one batch queue: outputs attached,
    run, detached; records byte-identical to a run with nothing attached."""
    T = tile()
    ns = [T + 5, 1, 2 * T]
    t = mosrx.Trace(mosrx.TRACE_IMIX, sum(ns), nflows=700, seed=5)
    p = mosrx.default_params(num_queues=8)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=8))
    dbs, bufs, q = [], [], None
    try:
        gpu_ctx.set_params(p)
        lo = 0
        for n in ns:
            o = t.off[lo:lo + n]
            base = int(o[0]) & ~15
            end = int(t.off[lo + n - 1]) + int(t.len[lo + n - 1])
            dbs.append(gpu_ctx.upload(t.frames[base:end], o - base, t.len[lo:lo + n], frames_bytes=end - base))
            lo += n
        q = gpu_ctx.queue_ex(dbs, compact=compact)

        def records():
            return [(d.results8() if compact else d.results()).tobytes() for d in dbs]

        q.run()
        plain = records()
        idxs = [Guarded(gpu_ctx, 4 * n) for n in ns]
        qss = [Guarded(gpu_ctx, 4 * QS) for _ in ns]
        bufs = idxs + qss
        q.set_steer([g.ptr for g in idxs], [g.ptr for g in qss])
        q.run()
        assert records() == plain
        lo = 0
        for i, n in enumerate(ns):
            eidx, eqs = expect(ora["queue"][lo:lo + n])
            np.testing.assert_array_equal(qss[i].read(), eqs, err_msg=f"batch {i}")
            np.testing.assert_array_equal(idxs[i].read(), eidx, err_msg=f"batch {i}")
            lo += n
        q.set_steer(None, None)
        for g in bufs:
            g.fill()
        q.run()
        assert records() == plain
        for g in bufs:
            assert (g.read(np.uint8) == SENT).all(), "a detached queue wrote steer outputs"
    finally:
        gpu_ctx.set_params(mosrx.default_params())
        if q is not None:
            q.destroy()
        for g in bufs:
            g.free()
        for d in dbs:
            d.free()


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("compact", [False, True])
def test_slot_steer_group(gpu_ctx, direct, compact):
    """A host group armed with mosrx_slot_steer: copied (pageable outputs) and
    direct with pinned outputs written in place.  Arming is one-shot: the next
    submit leaves sentinel-filled h_idx untouched."""
    T = tile()
    nb = 3
    t = mosrx.Trace(mosrx.TRACE_IMIX, 2 * T + 100, nflows=900, seed=9)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=4))
    frees = []
    rdt = mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE

    def arr(dtype, k):
        if not direct:
            return np.zeros(k, dtype)
        p, a = _pinned_like(gpu_ctx, dtype, k)
        frees.append(p)
        return a

    try:
        gpu_ctx.set_params(mosrx.default_params(num_queues=4))
        base, blk = gpu_ctx.host_alloc(t.frames_bytes + 8 * t.n + 256 * (nb + 1))
        frees.append(base)
        batches, parts = _stage(blk, base, t, nb)
        recs = [arr(rdt, b.n) for b in batches]
        # the outputs with their sentinels behind them
        idxb = [arr(np.uint8, 4 * b.n + GUARD) for b in batches]
        qsb = [arr(np.uint8, 4 * QS + GUARD) for b in batches]
        gpu_ctx.set_direct(BIG if direct else 0)

        def submit():
            outs = [r.ctypes.data for r in recs]
            if compact:
                gpu_ctx.group_submit_c8(1, batches, outs)
            else:
                gpu_ctx.group_submit_ex(1, batches, outs)
            gpu_ctx.group_wait(1)
            assert gpu_ctx.slot_direct(1) == direct

        for a in idxb + qsb:
            a[...] = SENT
        gpu_ctx.slot_steer(1, [a.ctypes.data for a in idxb], [a.ctypes.data for a in qsb])
        submit()
        lo = 0
        for i, b in enumerate(batches):
            eidx, eqs = expect(ora["queue"][lo:lo + b.n])
            assert (idxb[i][4 * b.n:] == SENT).all() and (qsb[i][4 * QS:] == SENT).all(), f"sentinel, batch {i}"
            np.testing.assert_array_equal(qsb[i][:4 * QS].view(np.uint32), eqs, err_msg=f"batch {i}")
            np.testing.assert_array_equal(idxb[i][:4 * b.n].view(np.uint32), eidx, err_msg=f"batch {i}")
            np.testing.assert_array_equal(recs[i]["queue"], ora["queue"][lo:lo + b.n])
            lo += b.n
        first = [r.tobytes() for r in recs]
        for a in idxb + qsb:
            a[...] = SENT
        submit()                                  # not armed any more
        assert [r.tobytes() for r in recs] == first
        for a in idxb + qsb:
            assert (a == SENT).all(), "an unarmed submit wrote steer outputs"
    finally:
        gpu_ctx.set_direct(0)
        gpu_ctx.set_params(mosrx.default_params())
        for p in frees:
            gpu_ctx.host_free(p)


@pytest.mark.parametrize("compact", [False, True])
def test_backend_steer_ioctl(compact):
    """cfg.steer over a memory source of T + 100 IMIX frames, num_queues 4:
    MOSRX_PKT_RX_STEER matches the oracle for every exposed batch."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, tile() + 100, nflows=500, seed=3)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=4))
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    be = mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=4), batch=512, group=2, cpu=2,
                          compact=compact, steer=True)
    try:
        seen = 0
        while True:
            n = be.recv_pkts(0)
            assert n >= 0
            if n == 0:
                break
            got = (be.results8(0, n) if compact else be.results(0, n))["queue"]
            np.testing.assert_array_equal(got, ora["queue"][seen:seen + n])
            view = be.steer_view(0)
            assert view is not None
            idx, qs, nq = view
            eidx, eqs = expect(ora["queue"][seen:seen + n])
            assert nq == 4 and len(idx) == n
            np.testing.assert_array_equal(qs, eqs, err_msg=f"batch@{seen}")
            np.testing.assert_array_equal(idx, eidx, err_msg=f"batch@{seen}")
            seen += n
        assert seen == t.n
    finally:
        be.close()


def test_backend_steer_off_ioctl_unsupported():
    t = mosrx.Trace(mosrx.TRACE_IMIX, 300, nflows=50, seed=3)
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    be = mosrx.GpuBackend([src], batch=512, cpu=2)
    try:
        assert be.recv_pkts(0) == t.n
        assert be.ioctl_raw(0, mosrx.PKT_RX_STEER, C.byref(mosrx.SteerView())) == -1
        assert be.steer_view(0) is None
    finally:
        be.close()


def test_backend_rx_loop_queues():
    """mosrx_rx_loop_queues delivers each frame once, to its queue's consumer, in
    arrival order within the queue."""
    nq = 4
    t = mosrx.Trace(mosrx.TRACE_IMIX, tile() + 100, nflows=500, seed=3)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=nq))
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    be = mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=nq), batch=4096, cpu=2, steer=True)
    got = []

    def consume(arg, ifidx, index, pkt, ln, res):
        got.append((int(arg or 0), index, res.contents.queue, ln))

    fn = mosrx._PKTFN(consume)
    try:
        st = be.run_loop_queues(nq, fn, [100 + q for q in range(nq)])
    finally:
        be.close()
    assert st.rx_packets == t.n and len(got) == t.n
    a = np.array(got, np.int64)
    assert sorted(a[:, 1].tolist()) == list(range(t.n))                   # every frame exactly once
    np.testing.assert_array_equal(a[:, 0] - 100, a[:, 2])                 # to arg[queue]
    np.testing.assert_array_equal(a[:, 2], ora["queue"][a[:, 1]])
    np.testing.assert_array_equal(a[:, 3], t.len[a[:, 1]])
    np.testing.assert_array_equal(a[:, 1], expect(ora["queue"])[0])       # queue 0, 1, ...; ascending within


def test_steer_dev_validation(gpu_ctx):
    """-EINVAL for rec_bytes not in {8, 16}, NULL or misaligned pointers and
    scratch that is too small; n == 0 returns 0 and launches nothing."""
    L = mosrx.lib()
    n = tile() + 1
    sb = int(L.mosrx_steer_scratch_bytes(n))
    rec, idx, qs, scr = (Guarded(gpu_ctx, k) for k in (16 * n, 4 * n, 4 * QS, sb))
    h = gpu_ctx.handle
    try:
        for rb in (0, 4, 12, 15, 17, 32, -8):
            assert L.mosrx_steer_dev(h, rec.ptr, n, rb, idx.ptr, qs.ptr, scr.ptr, sb, None) == -22, rb
        assert L.mosrx_steer_dev(h, None, n, 16, idx.ptr, qs.ptr, scr.ptr, sb, None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, n, 16, None, qs.ptr, scr.ptr, sb, None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, n, 16, idx.ptr, None, scr.ptr, sb, None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, n, 16, idx.ptr, qs.ptr, None, sb, None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, n, 16, idx.ptr + 2, qs.ptr, scr.ptr, sb, None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, n, 16, idx.ptr, qs.ptr, scr.ptr, sb - 1, None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, n, 16, idx.ptr, qs.ptr, scr.ptr,
                                 int(L.mosrx_steer_scratch_bytes(tile())), None) == -22
        assert L.mosrx_steer_dev(h, rec.ptr, 0, 16, idx.ptr, qs.ptr, scr.ptr, sb, None) == 0
        gpu_ctx.device_sync()
        for g in (idx, qs, scr):      # nothing above launched anything
            assert (g.read(np.uint8) == SENT).all()
        assert L.mosrx_slot_steer(h, 2, None, None) == -22
        assert L.mosrx_slot_steer(h, -1, None, None) == -22
        one = (C.c_void_p * 1)(idx.ptr)
        assert L.mosrx_slot_steer(h, 0, one, None) == -22
        assert L.mosrx_slot_steer(h, 0, None, one) == -22
    finally:
        for g in (rec, idx, qs, scr):
            g.free()


def test_slot_steer_busy_and_queue_validation(gpu_ctx, imix):
    """mosrx_slot_steer is -EBUSY while the slot runs (until its wait);
    mosrx_queue_set_steer refuses a NULL or misaligned output."""
    L = mosrx.lib()
    t = imix
    rec = np.zeros(t.n, mosrx.RESULT_DTYPE)
    b = mosrx.Batch(t.frames.ctypes.data, t.frames_bytes, t.off.ctypes.data, t.len.ctypes.data, t.n, t.max_len)
    hidx, hqs = np.zeros(t.n, np.uint32), np.zeros(QS, np.uint32)
    gpu_ctx.group_submit_ex(0, [b], [rec.ctypes.data])
    try:
        ia, qa = (C.c_void_p * 1)(hidx.ctypes.data), (C.c_void_p * 1)(hqs.ctypes.data)
        assert L.mosrx_slot_steer(gpu_ctx.handle, 0, ia, qa) == -16
    finally:
        gpu_ctx.group_wait(0)
    db = gpu_ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
    q = gpu_ctx.queue_ex([db])
    g = Guarded(gpu_ctx, 4 * t.n)
    try:
        ok, bad, null = (C.c_void_p * 1)(g.ptr), (C.c_void_p * 1)(g.ptr + 1), (C.c_void_p * 1)(None)
        h = gpu_ctx.handle
        assert L.mosrx_queue_set_steer(h, q.handle, ok, None) == -22
        assert L.mosrx_queue_set_steer(h, q.handle, ok, null) == -22
        assert L.mosrx_queue_set_steer(h, q.handle, bad, ok) == -22
        assert L.mosrx_queue_set_steer(h, None, ok, ok) == -22
        assert L.mosrx_queue_set_steer(h, q.handle, None, None) == 0
    finally:
        q.destroy()
        g.free()
        db.free()


def test_time_op_steer(gpu_ctx, imix):
    """MOSRX_OP_STEER times the steer sequence over records already made (one and
    several streams) and leaves the right idx; the dispatch form is -ENOTSUP."""
    t = imix
    ora = O.classify(t.frames, t.off, t.len, O.params())
    dbs = [gpu_ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len) for _ in range(2)]
    try:
        for d in dbs:
            gpu_ctx.classify_dev(d)
            gpu_ctx.classify_dev_compact(d)
        for rb in (16, 8):
            tot, avg = gpu_ctx.time_op(mosrx.OP_STEER, dbs, 6, nstreams=1, arg=rb)
            assert tot > 0 and avg > 0
            tot, _ = gpu_ctx.time_op(mosrx.OP_STEER, dbs, 6, nstreams=3, arg=rb, kernels=False)
            assert tot > 0
            for d in dbs:
                idx = d.d_sidx.download(np.zeros(t.n, np.uint32))
                np.testing.assert_array_equal(idx, expect(ora["queue"])[0])
        assert gpu_ctx.time_op_dispatch(mosrx.OP_STEER, dbs, 4, arg=16) is None
        with pytest.raises(mosrx.MosrxError):
            gpu_ctx.time_op(mosrx.OP_STEER, dbs, 2, arg=12)
    finally:
        for d in dbs:
            d.free()
