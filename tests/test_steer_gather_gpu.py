"""The queue-major gather on the GPU (mosrx_steer_gather_dev,
mosrx_queue_set_steer_gather, mosrx_slot_steer_gather, cfg.steer = 2 and
MOSRX_PKT_RX_QUEUE): besides idx and qstart (exact as in test_steer_gpu.py)

    qrec == rec[idx]     qoff == off[idx]     qlen == len[idx]

all plain numpy; end to end the queue byte comes from the oracle's records.
Every output sits in a sentinel-guarded buffer, checked after the launches."""
import ctypes as C

import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_direct_gpu import _pinned_like, _stage
from test_steer_gpu import BIG, GUARD, QS, SENT, Guarded, expect, keys_of, sizes, tile

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95


def gather_dev(ctx, d_rec, d_off, d_len, n, rb, descs=True):
    """mosrx_steer_gather_dev into guarded buffers: (idx, qstart, qrec[n, rb], qoff, qlen);
    descs False: d_qoff / d_qlen NULL, and the two buffers must stay sentinel-filled."""
    sb = int(mosrx.lib().mosrx_steer_scratch_bytes(n))
    idx, qs, scr = Guarded(ctx, 4 * n), Guarded(ctx, 4 * QS), Guarded(ctx, sb)
    qrec, qoff, qlen = Guarded(ctx, rb * n), Guarded(ctx, 4 * n), Guarded(ctx, 2 * n)
    try:
        ctx.steer_gather_dev(d_rec, d_off, d_len, n, rb, idx.ptr, qs.ptr, qrec.ptr,
                             qoff.ptr if descs else None, qlen.ptr if descs else None, scr.ptr, sb)
        scr.read(np.uint8)
        return (idx.read(), qs.read(), qrec.read(np.uint8).reshape(n, rb), qoff.read(np.uint32),
                qlen.read(np.uint16))
    finally:
        for g in (idx, qs, scr, qrec, qoff, qlen):
            g.free()


def synthetic(ctx, rng, pattern, n, rb):
    rec = rng.integers(0, 256, (n, rb)).astype(np.uint8)
    key = keys_of(pattern, n, rng)
    rec[:, rb - 3] = key
    off = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    ln = rng.integers(0, 1 << 16, n).astype(np.uint16)
    bufs = [mosrx.DevBuffer(ctx, a.nbytes) for a in (rec, off, ln)]
    for b, a in zip(bufs, (rec, off, ln)):
        b.upload(a)
    return rec, key, off, ln, bufs


@pytest.mark.parametrize("rb", [8, 16])
@pytest.mark.parametrize("pattern", ["one", "mod2", "mod3", "mod8", "mod256", "random", "last"])
def test_steer_gather_dev_synthetic(gpu_ctx, rb, pattern):
    """Random records with chosen key bytes, random u32 offsets and u16 lengths,
    every size around the wave and the tile."""
    rng = np.random.default_rng(4321 + rb)
    for n in sizes():
        rec, key, off, ln, bufs = synthetic(gpu_ctx, rng, pattern, n, rb)
        try:
            idx, qs, qrec, qoff, qlen = gather_dev(gpu_ctx, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, rb)
        finally:
            for b in bufs:
                b.free()
        eidx, eqs = expect(key)
        np.testing.assert_array_equal(qs, eqs, err_msg=f"qstart n={n}")
        np.testing.assert_array_equal(idx, eidx, err_msg=f"idx n={n}")
        np.testing.assert_array_equal(qrec, rec[eidx], err_msg=f"qrec n={n}")
        np.testing.assert_array_equal(qoff, off[eidx], err_msg=f"qoff n={n}")
        np.testing.assert_array_equal(qlen, ln[eidx], err_msg=f"qlen n={n}")


@pytest.mark.parametrize("rb", [8, 16])
def test_steer_gather_dev_records_only(gpu_ctx, rb):
    """d_qoff / d_qlen NULL: the records are gathered, the descriptor buffers untouched
    (with and without the batch's own descriptors given)."""
    rng = np.random.default_rng(77)
    n = 3 * tile() + 17
    rec, key, off, ln, bufs = synthetic(gpu_ctx, rng, "mod8", n, rb)
    try:
        for d_off, d_len in ((bufs[1].ptr, bufs[2].ptr), (None, None)):
            idx, qs, qrec, qoff, qlen = gather_dev(gpu_ctx, bufs[0].ptr, d_off, d_len, n, rb, descs=False)
            eidx, eqs = expect(key)
            np.testing.assert_array_equal(qs, eqs)
            np.testing.assert_array_equal(idx, eidx)
            np.testing.assert_array_equal(qrec, rec[eidx])
            assert (qoff.view(np.uint8) == SENT).all() and (qlen.view(np.uint8) == SENT).all()
    finally:
        for b in bufs:
            b.free()


def _sub(t, lo, n):
    """Frames [lo, lo + n) of trace t as (frames, off, len, frames_bytes), frames 16-byte aligned."""
    if n == 0:
        return t.frames[:16], np.zeros(0, np.uint32), np.zeros(0, np.uint16), 0
    o = t.off[lo:lo + n]
    base = int(o[0]) & ~15
    end = int(t.off[lo + n - 1]) + int(t.len[lo + n - 1])
    return t.frames[base:end], (o - base).astype(np.uint32), t.len[lo:lo + n], end - base


@pytest.mark.parametrize("compact", [False, True])
def test_queue_steer_gather(gpu_ctx, compact):
    """Four batches of 0, 65, T + 1 and 3T + 17 frames from different traces (so
    different queue patterns: one flow, few flows, many flows) in one batch
    queue, records from the queue's own classify launch; attached, run,
    detached; records byte-identical to a run with nothing attached."""
    T = tile()
    ns = [0, 65, T + 1, 3 * T + 17]
    traces = [mosrx.Trace(mosrx.TRACE_IMIX, 64, nflows=10, seed=1),
              mosrx.Trace(mosrx.TRACE_S64, 65, nflows=1, seed=2),
              mosrx.Trace(mosrx.TRACE_IMIX, T + 1, nflows=6, seed=3),
              mosrx.Trace(mosrx.TRACE_IMIX, 3 * T + 17, nflows=2000, seed=4)]
    rb = 8 if compact else 16
    dbs, bufs, q = [], [], None
    try:
        gpu_ctx.set_params(mosrx.default_params(num_queues=8))
        subs = [_sub(t, 0, n) for t, n in zip(traces, ns)]
        oras = [O.classify(fr, o, ln, O.params(num_queues=8)) if n else None for (fr, o, ln, fb), n in zip(subs, ns)]
        for fr, o, ln, fb in subs:
            dbs.append(gpu_ctx.upload(fr, o, ln, frames_bytes=fb, hint=None))
        q = gpu_ctx.queue_ex(dbs, compact=compact)

        def records():
            return [(d.results8() if compact else d.results()) for d in dbs]

        q.run()
        plain = [r.tobytes() for r in records()]
        idxs = [Guarded(gpu_ctx, 4 * n) for n in ns]
        qss = [Guarded(gpu_ctx, 4 * QS) for _ in ns]
        qrs = [Guarded(gpu_ctx, rb * n) for n in ns]
        qos = [Guarded(gpu_ctx, 4 * n) for n in ns]
        qls = [Guarded(gpu_ctx, 2 * n) for n in ns]
        bufs = idxs + qss + qrs + qos + qls
        q.set_steer_gather(*[[g.ptr for g in gs] for gs in (idxs, qss, qrs, qos, qls)])
        q.run()
        recs = records()
        assert [r.tobytes() for r in recs] == plain
        for i, n in enumerate(ns):
            if n == 0:
                for gs in (idxs, qss, qrs, qos, qls):
                    assert (gs[i].read(np.uint8) == SENT).all(), "an empty batch wrote outputs"
                continue
            fr, o, ln, fb = subs[i]
            np.testing.assert_array_equal(recs[i]["queue"], oras[i]["queue"])
            eidx, eqs = expect(oras[i]["queue"])
            np.testing.assert_array_equal(qss[i].read(), eqs, err_msg=f"batch {i}")
            np.testing.assert_array_equal(idxs[i].read(), eidx, err_msg=f"batch {i}")
            want = recs[i].view(np.uint8).reshape(n, rb)[eidx]
            np.testing.assert_array_equal(qrs[i].read(np.uint8).reshape(n, rb), want, err_msg=f"batch {i}")
            np.testing.assert_array_equal(qos[i].read(np.uint32), o[eidx], err_msg=f"batch {i}")
            np.testing.assert_array_equal(qls[i].read(np.uint16), ln[eidx], err_msg=f"batch {i}")
        q.set_steer_gather(None)
        for g in bufs:
            g.fill()
        q.run()
        assert [r.tobytes() for r in records()] == plain
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
def test_slot_steer_gather_group(gpu_ctx, direct, compact):
    """A host group of three batches armed with mosrx_slot_steer_gather: copied
    (pageable outputs) and direct with pinned outputs written in place.  One-shot:
    the next submit leaves the sentinel-filled outputs untouched."""
    T = tile()
    nb = 3
    t = mosrx.Trace(mosrx.TRACE_IMIX, 2 * T + 100, nflows=900, seed=9)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=4))
    frees = []
    rdt = mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE
    rb = rdt.itemsize

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
        sizes_of = (lambda b: 4 * b.n, lambda b: 4 * QS, lambda b: rb * b.n, lambda b: 4 * b.n, lambda b: 2 * b.n)
        outs5 = [[arr(np.uint8, f(b) + GUARD) for b in batches] for f in sizes_of]
        flat = [a for group in outs5 for a in group]
        gpu_ctx.set_direct(BIG if direct else 0)

        def submit():
            outs = [r.ctypes.data for r in recs]
            if compact:
                gpu_ctx.group_submit_c8(1, batches, outs)
            else:
                gpu_ctx.group_submit_ex(1, batches, outs)
            gpu_ctx.group_wait(1)
            assert gpu_ctx.slot_direct(1) == direct

        for a in flat:
            a[...] = SENT
        gpu_ctx.slot_steer_gather(1, *[[a.ctypes.data for a in group] for group in outs5])
        submit()
        lo = 0
        for i, b in enumerate(batches):
            fr, o, ln, fb = parts[i]
            eidx, eqs = expect(ora["queue"][lo:lo + b.n])
            for group, f in zip(outs5, sizes_of):
                assert (group[i][f(b):] == SENT).all(), f"sentinel, batch {i}"
            np.testing.assert_array_equal(recs[i]["queue"], ora["queue"][lo:lo + b.n])
            np.testing.assert_array_equal(outs5[1][i][:4 * QS].view(np.uint32), eqs, err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs5[0][i][:4 * b.n].view(np.uint32), eidx, err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs5[2][i][:rb * b.n].reshape(b.n, rb),
                                          recs[i].view(np.uint8).reshape(b.n, rb)[eidx], err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs5[3][i][:4 * b.n].view(np.uint32), np.asarray(o)[eidx])
            np.testing.assert_array_equal(outs5[4][i][:2 * b.n].view(np.uint16), np.asarray(ln)[eidx])
            lo += b.n
        first = [r.tobytes() for r in recs]
        for a in flat:
            a[...] = SENT
        submit()                                  # not armed any more
        assert [r.tobytes() for r in recs] == first
        for a in flat:
            assert (a == SENT).all(), "an unarmed submit wrote steer outputs"
    finally:
        gpu_ctx.set_direct(0)
        gpu_ctx.set_params(mosrx.default_params())
        for p in frees:
            gpu_ctx.host_free(p)


def _backend(t, steer, compact, nq=4, batch=512, group=2):
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    return mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=nq), batch=batch, group=group, cpu=2,
                            compact=compact, steer=steer)


@pytest.mark.parametrize("compact", [False, True])
def test_backend_rx_queue_ioctl(compact):
    """cfg.steer = 2 over a memory source of T + 100 IMIX frames, num_queues 4:
    MOSRX_PKT_RX_QUEUE for every queue is the numpy partition of the oracle's
    records, offsets, lengths and frames."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, tile() + 100, nflows=500, seed=3)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=4))
    rb = 8 if compact else 16
    be = _backend(t, 2, compact)
    try:
        seen = 0
        while True:
            n = be.recv_pkts(0)
            assert n >= 0
            if n == 0:
                break
            got = be.results8(0, n) if compact else be.results(0, n)
            np.testing.assert_array_equal(got["queue"], ora["queue"][seen:seen + n])
            if not compact:
                assert got.tobytes() == ora[seen:seen + n].tobytes()
            q = ora["queue"][seen:seen + n].astype(np.int64)
            total = 0
            for qq in range(256):
                v = be.queue_view(0, qq)
                assert v is not None
                rec, off, ln, idx, fbase = v
                members = np.nonzero(q == qq)[0]
                np.testing.assert_array_equal(idx, members, err_msg=f"queue {qq} @{seen}")
                if len(members) == 0:
                    continue
                np.testing.assert_array_equal(rec, got.view(np.uint8).reshape(n, rb)[members])
                np.testing.assert_array_equal(ln, t.len[seen + members])
                for j in (0, len(members) - 1):   # the frame bytes behind the view
                    fr = C.string_at(fbase + int(off[j]), int(ln[j]))
                    o0 = int(t.off[seen + members[j]])
                    assert fr == t.frames[o0:o0 + int(ln[j])].tobytes()
                total += len(members)
            assert total == n
            assert be.queue_view(0, 256) is None
            seen += n
        assert seen == t.n
    finally:
        be.close()


@pytest.mark.parametrize("steer", [0, 1])
def test_backend_rx_queue_needs_gather(steer):
    t = mosrx.Trace(mosrx.TRACE_IMIX, 300, nflows=50, seed=3)
    be = _backend(t, steer, False)
    try:
        assert be.recv_pkts(0) == t.n
        v = mosrx.QueueView()
        assert be.ioctl_raw(0, mosrx.PKT_RX_QUEUE, C.byref(v)) == -1
        v.q = mosrx.QUEUE_PROBE
        assert be.ioctl_raw(0, mosrx.PKT_RX_QUEUE, C.byref(v)) == -1
        assert be.queue_view(0, 0) is None
    finally:
        be.close()


@pytest.mark.parametrize("compact", [False, True])
def test_backend_rx_loop_queues_same_under_gather(compact):
    """mosrx_rx_loop_queues: the same per-queue call sequences and stats under
    cfg.steer = 2 (through the contiguous views) as under cfg.steer = 1 (through idx)."""
    nq = 4
    t = mosrx.Trace(mosrx.TRACE_IMIX, tile() + 100, nflows=500, seed=3)
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=nq))
    runs = {}
    for steer in (1, 2):
        be = _backend(t, steer, compact, nq=nq, batch=4096, group=1)
        got = []

        def consume(arg, ifidx, index, pkt, ln, res, got=got):
            r = res.contents
            got.append((int(arg or 0), index, r.queue, ln, r.rss, r.verdict, r.reason, C.string_at(pkt, 8)))

        fn = mosrx._PKTFN(consume)
        try:
            st = be.run_loop_queues(nq, fn, [100 + q for q in range(nq)])
        finally:
            be.close()
        runs[steer] = (got, (st.rx_packets, st.rx_bytes, st.rx_errors, st.rounds, st.batches, list(st.by_reason)))
    assert runs[1][1] == runs[2][1]
    assert runs[1][0] == runs[2][0]
    got = runs[2][0]
    assert len(got) == t.n
    a = np.array([g[:4] for g in got], np.int64)
    np.testing.assert_array_equal(a[:, 0] - 100, a[:, 2])
    np.testing.assert_array_equal(a[:, 2], ora["queue"][a[:, 1]])
    np.testing.assert_array_equal(a[:, 1], expect(ora["queue"])[0])
    for g in got[:: max(1, t.n // 50)]:
        o0 = int(t.off[g[1]])
        assert g[7] == t.frames[o0:o0 + 8].tobytes()


def test_steer_gather_validation(gpu_ctx):
    """-EINVAL for rec / qrec not aligned to rec_bytes and for only one of qoff /
    qlen, nothing launched; n == 0 returns 0; the timing op's dispatch form is -ENOTSUP."""
    L = mosrx.lib()
    n = tile() + 1
    sb = int(L.mosrx_steer_scratch_bytes(n))
    rec, idx, qs, scr, qrec, qoff, qlen, off, ln = (Guarded(gpu_ctx, k) for k in
                                                    (16 * n + 16, 4 * n, 4 * QS, sb, 16 * n + 16, 4 * n, 2 * n,
                                                     4 * n, 2 * n))
    h = gpu_ctx.handle

    def call(rb=16, r=rec.ptr, qr=qrec.ptr, qo=qoff.ptr, ql=qlen.ptr, o=off.ptr, l=ln.ptr, nn=n, ix=idx.ptr):
        return L.mosrx_steer_gather_dev(h, r, o, l, nn, rb, ix, qs.ptr, qr, qo, ql, scr.ptr, sb, None)

    try:
        for rb, delta in ((16, 8), (16, 4), (8, 4)):
            assert call(rb=rb, r=rec.ptr + delta) == EINVAL, (rb, delta)
            assert call(rb=rb, qr=qrec.ptr + delta) == EINVAL, (rb, delta)
        assert call(rb=8, r=rec.ptr + 8, qr=qrec.ptr + 8) == 0      # 8-byte records at 8-byte alignment
        gpu_ctx.device_sync()
        for g in (idx, qs, qrec, qoff, qlen, scr):     # that one launched; the rest must not
            g.fill()
        assert call(qo=None) == EINVAL and call(ql=None) == EINVAL
        assert call(o=None) == EINVAL and call(l=None) == EINVAL      # descriptors asked for, none to read
        assert call(qo=qoff.ptr + 2) == EINVAL and call(ql=qlen.ptr + 1) == EINVAL
        assert call(qr=None) == EINVAL and call(ix=idx.ptr + 2) == EINVAL
        assert call(rb=12) == EINVAL
        assert L.mosrx_steer_gather_dev(h, rec.ptr, off.ptr, ln.ptr, n, 16, idx.ptr, qs.ptr, qrec.ptr, qoff.ptr,
                                        qlen.ptr, scr.ptr, sb - 1, None) == EINVAL
        assert call(nn=0) == 0
        gpu_ctx.device_sync()
        for g in (idx, qs, qrec, qoff, qlen, scr):     # none of these launched anything
            assert (g.read(np.uint8) == SENT).all()
        one = (C.c_void_p * 1)(idx.ptr)
        assert L.mosrx_slot_steer_gather(h, 0, one, one, None, None, None) == EINVAL
        assert L.mosrx_slot_steer_gather(h, 0, one, one, one, one, None) == EINVAL
        assert L.mosrx_slot_steer_gather(h, 2, None, None, None, None, None) == EINVAL
        assert L.mosrx_slot_steer_gather(h, 0, None, None, None, None, None) == 0
        assert L.mosrx_queue_set_steer_gather(h, None, one, one, one, None, None) == EINVAL
    finally:
        for g in (rec, idx, qs, scr, qrec, qoff, qlen, off, ln):
            g.free()


def test_time_op_steer_gather(gpu_ctx):
    """MOSRX_OP_STEER_GATHER times the three launches over records already made
    and leaves the right idx; from the dispatch-stamped timer it is -ENOTSUP."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, 2 * tile() + 100, nflows=1000)
    ora = O.classify(t.frames, t.off, t.len, O.params())
    dbs = [gpu_ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len) for _ in range(2)]
    try:
        for d in dbs:
            gpu_ctx.classify_dev(d)
            gpu_ctx.classify_dev_compact(d)
        for rb in (16, 8):
            tot, avg = gpu_ctx.time_op(mosrx.OP_STEER_GATHER, dbs, 6, nstreams=1, arg=rb)
            assert tot > 0 and avg > 0
            tot, _ = gpu_ctx.time_op(mosrx.OP_STEER_GATHER, dbs, 6, nstreams=3, arg=rb, kernels=False)
            assert tot > 0
            for d in dbs:
                idx = d.d_sidx.download(np.zeros(t.n, np.uint32))
                np.testing.assert_array_equal(idx, expect(ora["queue"])[0])
        assert gpu_ctx.time_op_dispatch(mosrx.OP_STEER_GATHER, dbs, 4, arg=16) is None
        bs = (mosrx.Batch * 2)(*[d.batch() for d in dbs])
        outs = (C.c_void_p * 2)(*[d.d_out.ptr for d in dbs])
        aux = (C.c_void_p * 2)(*[d.d_sidx.ptr for d in dbs])
        ms = C.c_float()
        assert mosrx.lib().mosrx_time_op_dispatch(gpu_ctx.handle, mosrx.OP_STEER_GATHER, 16, bs, 2, outs, aux, 4,
                                                  C.byref(ms)) == ENOTSUP
        assert mosrx.lib().mosrx_time_op_dispatch(gpu_ctx.handle, mosrx.OP_STEER, 16, bs, 2, outs, aux, 4,
                                                  C.byref(ms)) == ENOTSUP
    finally:
        for d in dbs:
            d.free()
