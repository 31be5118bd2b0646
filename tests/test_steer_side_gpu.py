"""The gather's side form on the GPU (mosrx_steer_gather_side_dev,
mosrx_queue_set_steer_gather_side, mosrx_slot_steer_gather_side, cfg.steer = 3
and MOSRX_PKT_RX_QUEUE_SIDE): besides everything the gather tests expect,

    qfhash == fhash[idx]     qmatch == match[idx]     qtcpinfo == tcpinfo[idx]

exact, each array on its own (an absent one leaves its buffer untouched); end
to end the hashes, masks and pkt_info are the oracle's.  Every output sits in a
sentinel-guarded buffer, checked after the launches."""
import ctypes as C

import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_bpf import random_sets
from test_direct_gpu import _pinned_like
from test_steer_gather_gpu import _sub, gather_dev
from test_steer_gpu import BIG, GUARD, QS, SENT, Guarded, expect, keys_of, sizes, tile

pytestmark = pytest.mark.gpu

EINVAL, ENOTSUP = -22, -95
TI = 12   # sizeof(mosrx_tcpinfo)
ARRAYS = ("fhash", "match", "tcpinfo")


def bpf_set():
    """Four random programs: a set small enough to compile quickly, whose masks differ between frames."""
    return random_sets(5, 1)[0][:4]


def synthetic(ctx, rng, pattern, n, rb):
    """Records with chosen key bytes, offsets, lengths and the three side arrays,
    all random; (host arrays dict, device buffers dict)."""
    h = {"rec": rng.integers(0, 256, (n, rb)).astype(np.uint8),
         "off": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
         "len": rng.integers(0, 1 << 16, n).astype(np.uint16),
         "fhash": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
         "match": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
         "tcpinfo": rng.integers(0, 256, (n, TI)).astype(np.uint8)}
    h["key"] = keys_of(pattern, n, rng) if n else np.zeros(0, np.uint8)
    h["rec"][:, rb - 3] = h["key"]
    d = {}
    for k in ("rec", "off", "len") + ARRAYS:
        d[k] = mosrx.DevBuffer(ctx, max(h[k].nbytes, 4))
        if n:
            d[k].upload(h[k])
    return h, d


def side_dev(ctx, d, n, rb, which):
    """mosrx_steer_gather_side_dev into guarded buffers with the side arrays of
    `which` given: (idx, qstart, qrec, qoff, qlen, {name: raw bytes of its destination})."""
    sb = int(mosrx.lib().mosrx_steer_scratch_bytes(n))
    idx, qs, scr = Guarded(ctx, 4 * n), Guarded(ctx, 4 * QS), Guarded(ctx, sb)
    qrec, qoff, qlen = Guarded(ctx, rb * n), Guarded(ctx, 4 * n), Guarded(ctx, 2 * n)
    dst = {"fhash": Guarded(ctx, 4 * n), "match": Guarded(ctx, 4 * n), "tcpinfo": Guarded(ctx, TI * n)}
    try:
        ctx.steer_gather_side_dev(d["rec"].ptr, d["off"].ptr, d["len"].ptr, n, rb, idx.ptr, qs.ptr, qrec.ptr, qoff.ptr,
                                  qlen.ptr, scr.ptr, sb,
                                  **{k: (d[k].ptr, dst[k].ptr) for k in which})
        scr.read(np.uint8)
        return (idx.read(), qs.read(), qrec.read(np.uint8).reshape(n, rb), qoff.read(np.uint32), qlen.read(np.uint16),
                {k: g.read(np.uint8) for k, g in dst.items()})
    finally:
        for g in (idx, qs, scr, qrec, qoff, qlen, *dst.values()):
            g.free()


def check_side(h, eidx, side, which, msg=""):
    for k in ARRAYS:
        if k not in which:
            assert (side[k] == SENT).all(), f"{k} not asked for, but written {msg}"
        elif k == "tcpinfo":
            np.testing.assert_array_equal(side[k].reshape(-1, TI), h[k][eidx], err_msg=f"qtcpinfo {msg}")
        else:
            np.testing.assert_array_equal(side[k].view(np.uint32), h[k][eidx], err_msg=f"q{k} {msg}")


@pytest.mark.parametrize("rb", [8, 16])
@pytest.mark.parametrize("pattern", ["one", "mod3", "mod256", "random", "last"])
def test_steer_gather_side_dev_synthetic(gpu_ctx, rb, pattern):
    """All three side arrays, every size around the wave and the tile, and n == 0
    (nothing launched: every buffer stays sentinel-filled)."""
    rng = np.random.default_rng(9876 + rb)
    for n in [0] + sizes():
        h, d = synthetic(gpu_ctx, rng, pattern, n, rb)
        try:
            idx, qs, qrec, qoff, qlen, side = side_dev(gpu_ctx, d, n, rb, ARRAYS)
        finally:
            for b in d.values():
                b.free()
        if n == 0:
            assert (qs.view(np.uint8) == SENT).all()
            continue
        eidx, eqs = expect(h["key"])
        np.testing.assert_array_equal(qs, eqs, err_msg=f"qstart n={n}")
        np.testing.assert_array_equal(idx, eidx, err_msg=f"idx n={n}")
        np.testing.assert_array_equal(qrec, h["rec"][eidx], err_msg=f"qrec n={n}")
        np.testing.assert_array_equal(qoff, h["off"][eidx], err_msg=f"qoff n={n}")
        np.testing.assert_array_equal(qlen, h["len"][eidx], err_msg=f"qlen n={n}")
        check_side(h, eidx, side, ARRAYS, f"n={n}")


@pytest.mark.parametrize("rb", [8, 16])
@pytest.mark.parametrize("which", [("fhash",), ("match",), ("tcpinfo",), ARRAYS, ()])
def test_steer_gather_side_dev_presence(gpu_ctx, rb, which):
    """Each side array alone, all three, none: an absent array's destination
    stays sentinel-filled; with none the outputs are mosrx_steer_gather_dev's."""
    rng = np.random.default_rng(55)
    n = 3 * tile() + 17
    h, d = synthetic(gpu_ctx, rng, "mod3", n, rb)
    try:
        idx, qs, qrec, qoff, qlen, side = side_dev(gpu_ctx, d, n, rb, which)
        eidx, eqs = expect(h["key"])
        np.testing.assert_array_equal(qs, eqs)
        np.testing.assert_array_equal(idx, eidx)
        np.testing.assert_array_equal(qrec, h["rec"][eidx])
        np.testing.assert_array_equal(qoff, h["off"][eidx])
        np.testing.assert_array_equal(qlen, h["len"][eidx])
        check_side(h, eidx, side, which)
        if not which:
            plain = gather_dev(gpu_ctx, d["rec"].ptr, d["off"].ptr, d["len"].ptr, n, rb)
            for a, b in zip(plain, (idx, qs, qrec, qoff, qlen)):
                np.testing.assert_array_equal(a, b)
    finally:
        for b in d.values():
            b.free()


def test_steer_gather_side_validation(gpu_ctx):
    """-EINVAL for half a pair, a pointer off by 2 bytes and side outputs with no
    d_qrec, nothing launched; the arm and the queue form refuse side outputs
    without records; the timing op's dispatch form is -ENOTSUP."""
    L = mosrx.lib()
    n = tile() + 1
    sb = int(L.mosrx_steer_scratch_bytes(n))
    rec, idx, qs, scr, qrec, src, dst = (Guarded(gpu_ctx, k) for k in
                                         (16 * n, 4 * n, 4 * QS, sb, 16 * n, TI * n + 4, TI * n + 4))
    h = gpu_ctx.handle

    def call(fh=(None, None), mt=(None, None), ti=(None, None), qr=qrec.ptr):
        return L.mosrx_steer_gather_side_dev(h, rec.ptr, None, None, n, 16, idx.ptr, qs.ptr, qr, None, None, *fh, *mt,
                                             *ti, scr.ptr, sb, None)

    try:
        for slot in ("fh", "mt", "ti"):
            assert call(**{slot: (src.ptr, None)}) == EINVAL, slot
            assert call(**{slot: (None, dst.ptr)}) == EINVAL, slot
            assert call(**{slot: (src.ptr + 2, dst.ptr)}) == EINVAL, slot
            assert call(**{slot: (src.ptr, dst.ptr + 2)}) == EINVAL, slot
            assert call(**{slot: (src.ptr, dst.ptr)}, qr=None) == EINVAL, slot
        gpu_ctx.device_sync()
        for g in (idx, qs, scr, qrec, dst):
            assert (g.read(np.uint8) == SENT).all(), "a refused call launched"
        assert call(fh=(src.ptr + 4, dst.ptr + 4)) == 0          # 4-byte alignment is enough
        gpu_ctx.device_sync()
        one = (C.c_void_p * 1)(idx.ptr)
        assert L.mosrx_slot_steer_gather_side(h, 0, one, one, None, None, None, one, None, None) == EINVAL
        assert L.mosrx_slot_steer_gather_side(h, 2, None, None, None, None, None, None, None, None) == EINVAL
        assert L.mosrx_slot_steer_gather_side(h, 0, None, None, None, None, None, None, None, None) == 0
        assert L.mosrx_queue_set_steer_gather_side(h, None, one, one, one, None, None, one, None) == EINVAL
    finally:
        for g in (rec, idx, qs, scr, qrec, src, dst):
            g.free()


def test_time_op_steer_gather_side(gpu_ctx):
    """MOSRX_OP_STEER_GATHER_SIDE runs the three launches with the timing call's
    own side arrays and leaves the right idx; -ENOTSUP from the dispatch timer."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, 2 * tile() + 100, nflows=1000)
    ora = O.classify(t.frames, t.off, t.len, O.params())
    dbs = [gpu_ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len) for _ in range(2)]
    try:
        for d in dbs:
            gpu_ctx.classify_dev(d)
            gpu_ctx.classify_dev_compact(d)
        for rb in (16, 8):
            for which in (0, mosrx.SIDE_FHASH, mosrx.SIDE_MATCH, mosrx.SIDE_TCPINFO):
                tot, avg = gpu_ctx.time_op(mosrx.OP_STEER_GATHER_SIDE, dbs, 4, nstreams=1, arg=rb | which << 8)
                assert tot > 0 and avg > 0
            for d in dbs:
                idx = d.d_sidx.download(np.zeros(t.n, np.uint32))
                np.testing.assert_array_equal(idx, expect(ora["queue"])[0])
        bs = (mosrx.Batch * 2)(*[d.batch() for d in dbs])
        outs = (C.c_void_p * 2)(*[d.d_out.ptr for d in dbs])
        aux = (C.c_void_p * 2)(*[d.d_sidx.ptr for d in dbs])
        ms = C.c_float()
        L = mosrx.lib()
        assert L.mosrx_time_op_dispatch(gpu_ctx.handle, mosrx.OP_STEER_GATHER_SIDE, 16, bs, 2, outs, aux, 4,
                                        C.byref(ms)) == ENOTSUP
        assert L.mosrx_time_op(gpu_ctx.handle, mosrx.OP_STEER_GATHER_SIDE, 12, bs, 2, outs, aux, 4, 1, C.byref(ms),
                               None) == EINVAL
        assert L.mosrx_time_op(gpu_ctx.handle, mosrx.OP_STEER_GATHER_SIDE, 16 | 8 << 8, bs, 2, outs, aux, 4, 1,
                               C.byref(ms), None) == EINVAL
    finally:
        for d in dbs:
            d.free()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("what", ["fhash", "match"])
def test_queue_steer_gather_side(gpu_ctx, what, compact):
    """Four batches of 0, 65, T + 1 and 3T + 17 frames in one batch queue made
    with d_fhash (or, with a BPF set installed, d_match): the gathered hashes
    (masks) are the oracle's taken at idx, the records byte-identical to a run
    with nothing attached, detach restores the plain run, and a destination for
    the array the queue lacks is -EINVAL."""
    T = tile()
    ns = [0, 65, T + 1, 3 * T + 17]
    traces = [mosrx.Trace(mosrx.TRACE_IMIX, 64, nflows=10, seed=1),
              mosrx.Trace(mosrx.TRACE_S64, 65, nflows=1, seed=2),
              mosrx.Trace(mosrx.TRACE_IMIX, T + 1, nflows=6, seed=3),
              mosrx.Trace(mosrx.TRACE_IMIX, 3 * T + 17, nflows=2000, seed=4)]
    rb = 8 if compact else 16
    ps = bpf_set()
    dbs, bufs, q = [], [], None
    try:
        gpu_ctx.set_params(mosrx.default_params(num_queues=8))
        if what == "match":
            gpu_ctx.bpf_set(ps)
        subs = [_sub(t, 0, n) for t, n in zip(traces, ns)]
        oras = [O.classify_fh(fr, o, ln, O.params(num_queues=8)) if n else None for (fr, o, ln, fb), n in zip(subs, ns)]
        for fr, o, ln, fb in subs:
            dbs.append(gpu_ctx.upload(fr, o, ln, frames_bytes=fb, hint=None))
        q = gpu_ctx.queue_ex(dbs, flow_hash=what == "fhash", match=what == "match", compact=compact)

        def records():
            return [(d.results8() if compact else d.results()) for d in dbs]

        q.run()
        plain = [r.tobytes() for r in records()]
        groups = [[Guarded(gpu_ctx, f(n)) for n in ns] for f in
                  (lambda n: 4 * n, lambda n: 4 * QS, lambda n: rb * n, lambda n: 4 * n, lambda n: 2 * n,
                   lambda n: 4 * n, lambda n: 4 * n)]
        idxs, qss, qrs, qos, qls, qfs, qms = groups
        bufs = [g for gs in groups for g in gs]
        ptrs = [[g.ptr for g in gs] for gs in groups]
        # the array the queue does not make has no source
        lacks = ptrs[:5] + ([None, ptrs[6]] if what == "fhash" else [ptrs[5], None])
        with pytest.raises(mosrx.MosrxError) as e:
            q.set_steer_gather_side(*lacks)
        assert e.value.errno == 22
        q.set_steer_gather_side(*ptrs[:5], ptrs[5] if what == "fhash" else None, ptrs[6] if what == "match" else None)
        q.run()
        recs = records()
        assert [r.tobytes() for r in recs] == plain
        for i, n in enumerate(ns):
            if n == 0:
                for gs in groups:
                    assert (gs[i].read(np.uint8) == SENT).all(), "an empty batch wrote outputs"
                continue
            fr, o, ln, fb = subs[i]
            orec, ofh = oras[i]
            eidx, eqs = expect(orec["queue"])
            np.testing.assert_array_equal(qss[i].read(), eqs, err_msg=f"batch {i}")
            np.testing.assert_array_equal(idxs[i].read(), eidx, err_msg=f"batch {i}")
            np.testing.assert_array_equal(qrs[i].read(np.uint8).reshape(n, rb),
                                          recs[i].view(np.uint8).reshape(n, rb)[eidx], err_msg=f"batch {i}")
            np.testing.assert_array_equal(qos[i].read(np.uint32), o[eidx], err_msg=f"batch {i}")
            np.testing.assert_array_equal(qls[i].read(np.uint16), ln[eidx], err_msg=f"batch {i}")
            if what == "fhash":
                np.testing.assert_array_equal(dbs[i].flow_hashes(), ofh, err_msg=f"batch {i}")
                np.testing.assert_array_equal(qfs[i].read(), ofh[eidx], err_msg=f"batch {i}")
                assert (qms[i].read(np.uint8) == SENT).all()
            else:
                om = O.bpf_eval(ps, fr[:fb], o, ln)
                np.testing.assert_array_equal(dbs[i].matches(), om, err_msg=f"batch {i}")
                np.testing.assert_array_equal(qms[i].read(), om[eidx], err_msg=f"batch {i}")
                assert (qfs[i].read(np.uint8) == SENT).all()
        q.set_steer_gather_side(None)
        for g in bufs:
            g.fill()
        q.run()
        assert [r.tobytes() for r in records()] == plain
        for g in bufs:
            assert (g.read(np.uint8) == SENT).all(), "a detached queue wrote steer outputs"
    finally:
        gpu_ctx.set_params(mosrx.default_params())
        gpu_ctx.bpf_set([])
        if q is not None:
            q.destroy()
        for g in bufs:
            g.free()
        for d in dbs:
            d.free()


def _stage_sizes(arr, base, t, ns):
    """Consecutive runs of ns[i] frames of trace t laid out in arr (host address
    base): frames | off | len per batch, 16-byte aligned; the Batch list and parts."""
    batches, parts, pos, lo = [], [], 0, 0
    for n in ns:
        fr, o, ln, fb = _sub(t, lo, n)
        fa = (fb + 15) & ~15
        arr[pos:pos + fb] = fr[:fb]
        arr[pos + fa:pos + fa + 4 * n].view(np.uint32)[:] = o
        arr[pos + fa + 4 * n:pos + fa + 6 * n].view(np.uint16)[:] = ln
        batches.append(mosrx.Batch(base + pos, fb, base + pos + fa, base + pos + fa + 4 * n, n, int(ln.max())))
        parts.append((fr, o, ln, fb))
        pos += ((fa + 6 * n) + 255) & ~255
        lo += n
    return batches, parts


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("form", ["ex", "bpf_c8"])
def test_slot_steer_gather_side_group(gpu_ctx, direct, form):
    """One group of three batches (65, T + 1, 17 frames) armed with
    mosrx_slot_steer_gather_side and all three destinations: _submit_ex with
    tcpinfo and fhash gathers those two, _submit_bpf_c8 the masks (and the hashes
    it is given); the destination of an array the submit does not make stays
    sentinel-filled.  Copied back (pageable outputs) and written in place (pinned
    outputs, direct groups on).  One-shot: the next submit leaves them untouched."""
    T = tile()
    ns = [65, T + 1, 17]
    t = mosrx.Trace(mosrx.TRACE_IMIX, sum(ns), nflows=900, seed=9)
    orec, ofh, oti = O.classify_ex(t.frames, t.off, t.len, O.params(num_queues=4))
    ps = bpf_set()
    om = O.bpf_eval(ps, t.frames[:t.frames_bytes], t.off, t.len)
    compact = form == "bpf_c8"
    rdt = mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE
    rb = rdt.itemsize
    frees = []

    def arr(dtype, k):
        if not direct:
            return np.zeros(k, dtype)
        p, a = _pinned_like(gpu_ctx, dtype, k)
        frees.append(p)
        return a

    try:
        gpu_ctx.set_params(mosrx.default_params(num_queues=4))
        if compact:
            gpu_ctx.bpf_set(ps)
        base, blk = gpu_ctx.host_alloc(t.frames_bytes + 8 * t.n + 512 * (len(ns) + 1))
        frees.append(base)
        batches, parts = _stage_sizes(blk, base, t, ns)
        recs = [arr(rdt, n) for n in ns]
        fhs = [arr(np.uint32, n) for n in ns]
        tis = [arr(mosrx.TCPINFO_DTYPE, n) for n in ns]
        mts = [arr(np.uint32, n) for n in ns]
        sizes_of = (lambda n: 4 * n, lambda n: 4 * QS, lambda n: rb * n, lambda n: 4 * n, lambda n: 2 * n,
                    lambda n: 4 * n, lambda n: 4 * n, lambda n: TI * n)
        outs8 = [[arr(np.uint8, f(n) + GUARD) for n in ns] for f in sizes_of]
        flat = [a for group in outs8 for a in group]
        gpu_ctx.set_direct(BIG if direct else 0)

        def submit():
            outs = [r.ctypes.data for r in recs]
            f = [a.ctypes.data for a in fhs]
            if compact:
                gpu_ctx.group_submit_c8(1, batches, outs, f, [a.ctypes.data for a in mts])
            else:
                gpu_ctx.group_submit_ex(1, batches, outs, [a.ctypes.data for a in tis], f)
            gpu_ctx.group_wait(1)
            assert gpu_ctx.slot_direct(1) == direct

        for a in flat:
            a[...] = SENT
        gpu_ctx.slot_steer_gather_side(1, *[[a.ctypes.data for a in group] for group in outs8])
        submit()
        lo = 0
        for i, n in enumerate(ns):
            fr, o, ln, fb = parts[i]
            eidx, eqs = expect(orec["queue"][lo:lo + n])
            for group, f in zip(outs8, sizes_of):
                assert (group[i][f(n):] == SENT).all(), f"sentinel, batch {i}"
            np.testing.assert_array_equal(recs[i]["queue"], orec["queue"][lo:lo + n])
            np.testing.assert_array_equal(outs8[1][i][:4 * QS].view(np.uint32), eqs, err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs8[0][i][:4 * n].view(np.uint32), eidx, err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs8[2][i][:rb * n].reshape(n, rb),
                                          recs[i].view(np.uint8).reshape(n, rb)[eidx], err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs8[3][i][:4 * n].view(np.uint32), np.asarray(o)[eidx])
            np.testing.assert_array_equal(outs8[4][i][:2 * n].view(np.uint16), np.asarray(ln)[eidx])
            np.testing.assert_array_equal(fhs[i], ofh[lo:lo + n], err_msg=f"batch {i}")
            np.testing.assert_array_equal(outs8[5][i][:4 * n].view(np.uint32), ofh[lo:lo + n][eidx],
                                          err_msg=f"qfhash, batch {i}")
            if compact:
                np.testing.assert_array_equal(mts[i], om[lo:lo + n], err_msg=f"batch {i}")
                np.testing.assert_array_equal(outs8[6][i][:4 * n].view(np.uint32), om[lo:lo + n][eidx],
                                              err_msg=f"qmatch, batch {i}")
                assert (outs8[7][i] == SENT).all(), "tcpinfo destination written by a submit that makes none"
            else:
                assert tis[i].tobytes() == oti[lo:lo + n].tobytes(), f"batch {i}"
                np.testing.assert_array_equal(outs8[7][i][:TI * n].reshape(n, TI),
                                              oti[lo:lo + n].view(np.uint8).reshape(n, TI)[eidx],
                                              err_msg=f"qtcpinfo, batch {i}")
                assert (outs8[6][i] == SENT).all(), "match destination written by a submit that makes none"
            lo += n
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
        gpu_ctx.bpf_set([])
        for p in frees:
            gpu_ctx.host_free(p)


def _backend(t, steer, compact, bpf=None, nq=4, batch=512, group=2):
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    return mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=nq), batch=batch, group=group, cpu=2,
                            compact=compact, steer=steer, flowhash=True, bpf=bpf)


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("with_bpf", [False, True])
def test_backend_rx_queue_side_ioctl(with_bpf, compact):
    """cfg.steer = 3 with flowhash (and then a BPF set) over a memory source:
    for every exposed batch and queue MOSRX_PKT_RX_QUEUE_SIDE's runs are the
    batch-order arrays (RX_FHASH, RX_MATCH) at RX_STEER's idx, and the oracle's."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, tile() + 100, nflows=500, seed=3)
    orec, ofh = O.classify_fh(t.frames, t.off, t.len, O.params(num_queues=4))
    ps = bpf_set() if with_bpf else None
    om = O.bpf_eval(ps, t.frames[:t.frames_bytes], t.off, t.len) if with_bpf else None
    be = _backend(t, 3, compact, bpf=ps)
    try:
        v = mosrx.QueueSide()
        v.q = mosrx.QUEUE_PROBE
        assert be.ioctl_raw(0, mosrx.PKT_RX_QUEUE_SIDE, C.byref(v)) == 0
        seen = 0
        while True:
            n = be.recv_pkts(0)
            assert n >= 0
            if n == 0:
                break
            idx, qs, _ = be.steer_view(0)
            eidx, eqs = expect(orec["queue"][seen:seen + n])
            np.testing.assert_array_equal(idx, eidx)
            np.testing.assert_array_equal(qs, eqs)
            fh = be.fhashes(0, n)
            np.testing.assert_array_equal(fh, ofh[seen:seen + n])
            mt = be.matches(0, n) if with_bpf else None
            if with_bpf:
                np.testing.assert_array_equal(mt, om[seen:seen + n])
            total = 0
            for qq in range(256):
                side = be.queue_side(0, qq)
                assert side is not None
                qfh, qmt, qti = side
                view = be.queue_view(0, qq)            # RX_QUEUE keeps answering as under steer = 2
                assert view is not None and len(view[3]) == len(qfh)
                np.testing.assert_array_equal(view[3], idx[qs[qq]:qs[qq + 1]])
                assert qti is None
                np.testing.assert_array_equal(qfh, fh[idx[qs[qq]:qs[qq + 1]]], err_msg=f"queue {qq} @{seen}")
                if with_bpf:
                    np.testing.assert_array_equal(qmt, mt[idx[qs[qq]:qs[qq + 1]]], err_msg=f"queue {qq} @{seen}")
                else:
                    assert qmt is None
                total += len(qfh)
            assert total == n
            assert be.queue_side(0, 256) is None
            seen += n
        assert seen == t.n
    finally:
        be.close()


def test_backend_rx_queue_side_tcpinfo():
    """cfg.steer = 3 with cfg.tcpinfo: the share's pkt_info run is the oracle's at idx."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, 700, nflows=300, seed=5)
    orec, ofh, oti = O.classify_ex(t.frames, t.off, t.len, O.params(num_queues=4))
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    be = mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=4), batch=512, group=2, cpu=2, steer=3,
                          tcpinfo=True)
    try:
        seen = 0
        while True:
            n = be.recv_pkts(0)
            if n <= 0:
                break
            assert be.tcpinfo(0, n).tobytes() == oti[seen:seen + n].tobytes()
            idx, qs, _ = be.steer_view(0)
            for qq in range(4):
                qfh, qmt, qti = be.queue_side(0, qq)
                assert qfh is None and qmt is None
                assert qti.tobytes() == oti[seen:seen + n][idx[qs[qq]:qs[qq + 1]]].tobytes(), f"queue {qq} @{seen}"
            seen += n
        assert seen == t.n
    finally:
        be.close()


def test_backend_rx_queue_side_needs_steer3():
    """cfg.steer = 2 gathers records only: -1 to MOSRX_PKT_RX_QUEUE_SIDE and to its probe."""
    t = mosrx.Trace(mosrx.TRACE_IMIX, 300, nflows=50, seed=3)
    be = _backend(t, 2, False)
    try:
        assert be.recv_pkts(0) == t.n
        v = mosrx.QueueSide()
        assert be.ioctl_raw(0, mosrx.PKT_RX_QUEUE_SIDE, C.byref(v)) == -1
        v.q = mosrx.QUEUE_PROBE
        assert be.ioctl_raw(0, mosrx.PKT_RX_QUEUE_SIDE, C.byref(v)) == -1
        assert be.queue_side(0, 0) is None
        assert be.queue_view(0, 0) is not None
    finally:
        be.close()
