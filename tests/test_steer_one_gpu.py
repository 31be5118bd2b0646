"""The one-launch steer form on the GPU (mosrx_set_steer_one,
mosrx_steer_one_kernel): histogram, scan and scatter / gather in one kernel, one
workgroup per batch.  Expected values are the ones test_steer_gpu.py defines,
compared exactly and never against another GPU run:

    idx    == argsort(queue, kind="stable")
    qstart == [0] + cumsum(bincount(queue, 256))
    gathered arrays == src[idx]

Every output buffer carries a 64-byte sentinel behind it; mosrx_steer_one_count
tells which form ran."""
import ctypes as C

import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_direct_gpu import _pinned_like
from test_steer_gather_gpu import _sub
from test_steer_gpu import BIG, GUARD, QS, SENT, Guarded, expect, sizes, tile
from test_steer_side_gpu import ARRAYS, TI, check_side, synthetic

pytestmark = pytest.mark.gpu

EINVAL = -22
MAX = mosrx.STEER_ONE_MAX


@pytest.fixture
def one(gpu_ctx):
    """The session's context with the limit at MOSRX_STEER_ONE_MAX; off again afterwards."""
    gpu_ctx.set_steer_one(MAX)
    yield gpu_ctx
    gpu_ctx.set_steer_one(0)


def run_form(ctx, d, n, rb, form, descs=True, which=()):
    """One of the three _dev forms over the device arrays d into guarded buffers.
    Returns (idx, qstart, qrec, qoff, qlen, side bytes, growth of steer_one_count);
    the scratch must come back all sentinel when the one-launch form ran."""
    sb = int(mosrx.lib().mosrx_steer_scratch_bytes(n))
    idx, qs, scr = Guarded(ctx, 4 * n), Guarded(ctx, 4 * QS), Guarded(ctx, sb)
    qrec, qoff, qlen = Guarded(ctx, rb * n), Guarded(ctx, 4 * n), Guarded(ctx, 2 * n)
    dst = {"fhash": Guarded(ctx, 4 * n), "match": Guarded(ctx, 4 * n), "tcpinfo": Guarded(ctx, TI * n)}
    before = ctx.steer_one_count()
    try:
        if form == "plain":
            ctx.steer_dev(d["rec"].ptr, n, rb, idx.ptr, qs.ptr, scr.ptr, sb)
        elif form == "gather":
            ctx.steer_gather_dev(d["rec"].ptr, d["off"].ptr, d["len"].ptr, n, rb, idx.ptr, qs.ptr, qrec.ptr,
                                 qoff.ptr if descs else None, qlen.ptr if descs else None, scr.ptr, sb)
        else:
            ctx.steer_gather_side_dev(d["rec"].ptr, d["off"].ptr, d["len"].ptr, n, rb, idx.ptr, qs.ptr, qrec.ptr,
                                      qoff.ptr if descs else None, qlen.ptr if descs else None, scr.ptr, sb,
                                      **{k: (d[k].ptr, dst[k].ptr) for k in which})
        grew = ctx.steer_one_count() - before
        if grew:
            assert (scr.read(np.uint8) == SENT).all(), "the one-launch form wrote the scratch"
        else:
            scr.read(np.uint8)
        return (idx.read(), qs.read(), qrec.read(np.uint8), qoff.read(np.uint8), qlen.read(np.uint8),
                {k: g.read(np.uint8) for k, g in dst.items()}, grew)
    finally:
        for g in (idx, qs, scr, qrec, qoff, qlen, *dst.values()):
            g.free()


def check_form(h, n, rb, out, form, descs, which, msg):
    idx, qs, qrec, qoff, qlen, side, _ = out
    eidx, eqs = expect(h["key"])
    np.testing.assert_array_equal(qs, eqs, err_msg=f"qstart {msg}")
    np.testing.assert_array_equal(idx, eidx, err_msg=f"idx {msg}")
    if form == "plain":
        assert (qrec == SENT).all(), f"qrec written by the plain form {msg}"
    else:
        np.testing.assert_array_equal(qrec.reshape(n, rb), h["rec"][eidx], err_msg=f"qrec {msg}")
    if form != "plain" and descs:
        np.testing.assert_array_equal(qoff.view(np.uint32), h["off"][eidx], err_msg=f"qoff {msg}")
        np.testing.assert_array_equal(qlen.view(np.uint16), h["len"][eidx], err_msg=f"qlen {msg}")
    else:
        assert (qoff == SENT).all() and (qlen == SENT).all(), f"descriptors not asked for, but written {msg}"
    check_side(h, eidx, side, which, msg)


# (form, qoff / qlen given, side arrays given)
FORMS = [("plain", False, ()), ("gather", True, ()), ("gather", False, ()), ("side", True, ("fhash",)),
         ("side", True, ("match",)), ("side", False, ("tcpinfo",)), ("side", True, ARRAYS)]


@pytest.mark.parametrize("rb", [8, 16])
@pytest.mark.parametrize("pattern", ["one", "mod3", "mod256", "random", "last"])
def test_steer_one_dev_synthetic(one, rb, pattern):
    """The three _dev forms with the limit at MOSRX_STEER_ONE_MAX: chosen key
    bytes in otherwise random records, n around the wave, around the single-tile
    path (T - 1, T, T + 1) and over several tiles with a ragged last slice
    (3T + 17); gather with and without qoff / qlen, side with each array alone
    and all three.  Each call is one fused launch and leaves the scratch alone."""
    T = tile()
    assert sizes() == [1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]
    rng = np.random.default_rng(2468 + rb)
    for n in sizes():
        h, d = synthetic(one, rng, pattern, n, rb)
        try:
            for form, descs, which in FORMS:
                out = run_form(one, d, n, rb, form, descs, which)
                assert out[-1] == 1, f"steer_one_count grew by {out[-1]} ({form}, n={n})"
                check_form(h, n, rb, out, form, descs, which, f"({form} descs={descs} {which}, n={n})")
        finally:
            for b in d.values():
                b.free()


class SDesc(C.Structure):
    _fields_ = [("rec", C.c_void_p), ("idx", C.c_void_p), ("qstart", C.c_void_p), ("n", C.c_uint32),
                ("tile_base", C.c_uint32)]


class GDesc(C.Structure):
    _fields_ = [("off", C.c_void_p), ("len", C.c_void_p), ("qrec", C.c_void_p), ("qoff", C.c_void_p),
                ("qlen", C.c_void_p)]


class XDesc(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("fhash", "qfhash", "match", "qmatch", "tcpinfo", "qtcpinfo")]


class SParams(C.Structure):
    """mosrx_sparams (csrc/mosrx_steer.h); its layout is pinned in test_steer_one.py."""
    _fields_ = [("desc", C.c_void_p), ("one", SDesc), ("hist", C.c_void_p), ("nb", C.c_uint32),
                ("rec_bytes", C.c_uint32), ("total_tiles", C.c_uint32), ("gather", C.c_uint32),
                ("gdesc", C.c_void_p), ("gone", GDesc), ("xdesc", C.c_void_p), ("xone", XDesc),
                ("side", C.c_uint32), ("fused", C.c_uint32)]


def test_steer_one_empty_batch_qstart(gpu_ctx):
    """n == 0 with a non-NULL qstart (a table entry; the public calls give an
    empty batch a NULL one): 257 zeros, idx untouched, hist not needed."""
    L = mosrx.lib()
    L.mosrx_launch_steer.restype = C.c_int
    L.mosrx_launch_steer.argtypes = [C.POINTER(SParams), C.c_void_p]
    rec, idx, qs, tab = Guarded(gpu_ctx, 64), Guarded(gpu_ctx, 64), Guarded(gpu_ctx, 4 * QS), Guarded(gpu_ctx, 32)
    try:
        for rb in (8, 16):
            qs.fill()
            tab.buf.upload(np.frombuffer(bytes(SDesc(rec.ptr, idx.ptr, qs.ptr, 0, 0)), np.uint8))
            sp = SParams(desc=tab.ptr, nb=1, rec_bytes=rb, total_tiles=0, fused=1)
            assert L.mosrx_launch_steer(C.byref(sp), None) == 0
            gpu_ctx.device_sync()
            assert (qs.read() == 0).all()
            assert (idx.read(np.uint8) == SENT).all() and (rec.read(np.uint8) == SENT).all()
        # the single-batch form's own condition
        sp = SParams(one=SDesc(rec.ptr, idx.ptr, qs.ptr, MAX + 1, 0), nb=1, rec_bytes=8, total_tiles=33, fused=1)
        assert L.mosrx_launch_steer(C.byref(sp), None) == EINVAL
        sp = SParams(one=SDesc(rec.ptr, idx.ptr, qs.ptr, 4, 0), nb=1, rec_bytes=8, total_tiles=1, fused=0)
        assert L.mosrx_launch_steer(C.byref(sp), None) == EINVAL          # three launches need hist
    finally:
        for g in (rec, idx, qs, tab):
            g.free()


def test_steer_one_limit(gpu_ctx):
    """Limit T: n = T is fused, n = T + 1 takes the three launches, both right;
    limit 0 never counts; a limit above the cap is -EINVAL and changes nothing."""
    T = tile()
    L = mosrx.lib()
    rng = np.random.default_rng(99)
    try:
        for n, limit, want in ((T, T, 1), (T + 1, T, 0), (T, 0, 0), (65, 0, 0), (3 * T + 17, MAX, 1)):
            gpu_ctx.set_steer_one(limit)
            assert gpu_ctx.get_steer_one() == limit
            h, d = synthetic(gpu_ctx, rng, "random", n, 8)
            try:
                for form, descs, which in (FORMS[0], FORMS[1], FORMS[-1]):
                    out = run_form(gpu_ctx, d, n, 8, form, descs, which)
                    assert out[-1] == want, f"n={n} limit={limit} {form}"
                    check_form(h, n, 8, out, form, descs, which, f"(n={n} limit={limit} {form})")
            finally:
                for b in d.values():
                    b.free()
        gpu_ctx.set_steer_one(T)
        assert L.mosrx_set_steer_one(gpu_ctx.handle, MAX + 1) == EINVAL
        assert L.mosrx_set_steer_one(gpu_ctx.handle, 0xFFFFFFFF) == EINVAL
        assert gpu_ctx.get_steer_one() == T
        assert L.mosrx_set_steer_one(gpu_ctx.handle, MAX) == 0 and gpu_ctx.get_steer_one() == MAX
    finally:
        gpu_ctx.set_steer_one(0)


@pytest.mark.parametrize("nq,compact", [(8, False), (3, True)])
def test_steer_one_queue(gpu_ctx, nq, compact):
    """Five batches of T + 9, 0, 64, 1 and 2T IMIX frames in one batch queue with
    flow hashes; steer, gather and side (fhash) attached in turn.  Limit 2T: each
    run is one fused launch; limit 2T - 1: the three launches; the same outputs,
    the oracle's, on both of two runs (the running positions are per launch)."""
    T = tile()
    ns = [T + 9, 0, 64, 1, 2 * T]
    rb = 8 if compact else 16
    t = mosrx.Trace(mosrx.TRACE_IMIX, sum(ns), nflows=1200, seed=17)
    los = np.concatenate([[0], np.cumsum(ns)]).astype(int)
    subs = [_sub(t, int(lo), n) for lo, n in zip(los, ns)]
    oras = [O.classify_fh(fr, o, ln, O.params(num_queues=nq)) if n else None for (fr, o, ln, fb), n in zip(subs, ns)]
    dbs, bufs, q = [], [], None
    try:
        gpu_ctx.set_params(mosrx.default_params(num_queues=nq))
        for fr, o, ln, fb in subs:
            dbs.append(gpu_ctx.upload(fr, o, ln, frames_bytes=fb, hint=None))
        q = gpu_ctx.queue_ex(dbs, flow_hash=True, compact=compact)
        groups = [[Guarded(gpu_ctx, f(n)) for n in ns] for f in
                  (lambda n: 4 * n, lambda n: 4 * QS, lambda n: rb * n, lambda n: 4 * n, lambda n: 2 * n,
                   lambda n: 4 * n)]
        idxs, qss, qrs, qos, qls, qfs = groups
        bufs = [g for gs in groups for g in gs]
        ptrs = [[g.ptr for g in gs] for gs in groups]
        for form in ("steer", "gather", "side"):
            if form == "steer":
                q.set_steer(ptrs[0], ptrs[1])
            elif form == "gather":
                q.set_steer_gather(*ptrs[:5])
            else:
                q.set_steer_gather_side(*ptrs[:5], ptrs[5], None)
            for limit, want in ((2 * T, 1), (2 * T - 1, 0)):
                gpu_ctx.set_steer_one(limit)
                for run in range(2):
                    for g in bufs:
                        g.fill()
                    before = gpu_ctx.steer_one_count()
                    q.run()
                    assert gpu_ctx.steer_one_count() - before == want, f"{form} limit {limit} run {run}"
                    for i, n in enumerate(ns):
                        msg = f"{form} limit {limit} run {run} batch {i}"
                        if n == 0:
                            for gs in groups:
                                assert (gs[i].read(np.uint8) == SENT).all(), f"an empty batch wrote outputs, {msg}"
                            continue
                        fr, o, ln, fb = subs[i]
                        orec, ofh = oras[i]
                        rec = (dbs[i].results8() if compact else dbs[i].results()).view(np.uint8).reshape(n, rb)
                        np.testing.assert_array_equal(rec[:, rb - 3], orec["queue"], err_msg=msg)
                        eidx, eqs = expect(orec["queue"])
                        np.testing.assert_array_equal(qss[i].read(), eqs, err_msg=msg)
                        np.testing.assert_array_equal(idxs[i].read(), eidx, err_msg=msg)
                        if form == "steer":
                            assert (qrs[i].read(np.uint8) == SENT).all(), msg
                            continue
                        np.testing.assert_array_equal(qrs[i].read(np.uint8).reshape(n, rb), rec[eidx], err_msg=msg)
                        np.testing.assert_array_equal(qos[i].read(np.uint32), o[eidx], err_msg=msg)
                        np.testing.assert_array_equal(qls[i].read(np.uint16), ln[eidx], err_msg=msg)
                        if form == "side":
                            np.testing.assert_array_equal(qfs[i].read(), ofh[eidx], err_msg=msg)
                        else:
                            assert (qfs[i].read(np.uint8) == SENT).all(), msg
    finally:
        gpu_ctx.set_steer_one(0)
        gpu_ctx.set_params(mosrx.default_params())
        if q is not None:
            q.destroy()
        for g in bufs:
            g.free()
        for d in dbs:
            d.free()


def _stage_ns(arr, base, t, ns):
    """Consecutive runs of ns[i] frames of trace t (0 allowed) laid out in arr
    (host address base): frames | off | len per batch, 16-byte aligned."""
    batches, parts, pos, lo = [], [], 0, 0
    for n in ns:
        fr, o, ln, fb = _sub(t, lo, n)
        fa = (fb + 15) & ~15
        arr[pos:pos + fb] = fr[:fb]
        arr[pos + fa:pos + fa + 4 * n].view(np.uint32)[:] = o
        arr[pos + fa + 4 * n:pos + fa + 6 * n].view(np.uint16)[:] = ln
        batches.append(mosrx.Batch(base + pos, fb, base + pos + fa, base + pos + fa + 4 * n, n,
                                   int(ln.max()) if n else 0))
        parts.append((fr, o, ln, fb))
        pos += ((fa + 6 * n) + 255 + 256) & ~255
        lo += n
    return batches, parts


@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("compact", [True, False])
def test_steer_one_slot_group(one, direct, compact):
    """A group of three batches (65, 0, T + 1 frames) armed with
    mosrx_slot_steer_gather_side: 8-byte records with h_fhash, 16-byte records
    with h_tcpinfo; written in place (direct group, everything pinned) and
    copied back (pageable outputs).  One fused launch per submit; the oracle's values."""
    T = tile()
    ns = [65, 0, T + 1]
    t = mosrx.Trace(mosrx.TRACE_IMIX, sum(ns), nflows=900, seed=9)
    orec, ofh, oti = O.classify_ex(t.frames, t.off, t.len, O.params(num_queues=4))
    rdt = mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE
    rb = rdt.itemsize
    frees = []

    def arr(dtype, k):
        if not direct:
            return np.zeros(k, dtype)
        p, a = _pinned_like(one, dtype, k)
        frees.append(p)
        return a

    try:
        one.set_params(mosrx.default_params(num_queues=4))
        base, blk = one.host_alloc(t.frames_bytes + 8 * t.n + 1024 * (len(ns) + 1))
        frees.append(base)
        batches, parts = _stage_ns(blk, base, t, ns)
        recs = [arr(rdt, n) for n in ns]
        fhs = [arr(np.uint32, n) for n in ns]
        tis = [arr(mosrx.TCPINFO_DTYPE, n) for n in ns]
        sizes_of = (lambda n: 4 * n, lambda n: 4 * QS, lambda n: rb * n, lambda n: 4 * n, lambda n: 2 * n,
                    lambda n: 4 * n, lambda n: 4 * n, lambda n: TI * n)
        outs8 = [[arr(np.uint8, f(n) + GUARD) for n in ns] for f in sizes_of]
        one.set_direct(BIG if direct else 0)
        for rnd in range(2):
            for group in outs8:
                for a in group:
                    a[...] = SENT
            one.slot_steer_gather_side(1, *[[a.ctypes.data for a in group] for group in outs8])
            before = one.steer_one_count()
            outs = [r.ctypes.data for r in recs]
            if compact:
                one.group_submit_c8(1, batches, outs, [a.ctypes.data for a in fhs])
            else:
                one.group_submit_ex(1, batches, outs, [a.ctypes.data for a in tis], None)
            one.group_wait(1)
            assert one.slot_direct(1) == direct
            assert one.steer_one_count() - before == 1
            lo = 0
            for i, n in enumerate(ns):
                msg = f"round {rnd} batch {i}"
                if n == 0:
                    for group in outs8:
                        assert (group[i] == SENT).all(), f"an empty batch wrote outputs, {msg}"
                    continue
                fr, o, ln, fb = parts[i]
                eidx, eqs = expect(orec["queue"][lo:lo + n])
                for group, f in zip(outs8, sizes_of):
                    assert (group[i][f(n):] == SENT).all(), f"sentinel, {msg}"
                np.testing.assert_array_equal(recs[i]["queue"], orec["queue"][lo:lo + n], err_msg=msg)
                np.testing.assert_array_equal(outs8[1][i][:4 * QS].view(np.uint32), eqs, err_msg=msg)
                np.testing.assert_array_equal(outs8[0][i][:4 * n].view(np.uint32), eidx, err_msg=msg)
                np.testing.assert_array_equal(outs8[2][i][:rb * n].reshape(n, rb),
                                              recs[i].view(np.uint8).reshape(n, rb)[eidx], err_msg=msg)
                np.testing.assert_array_equal(outs8[3][i][:4 * n].view(np.uint32), np.asarray(o)[eidx], err_msg=msg)
                np.testing.assert_array_equal(outs8[4][i][:2 * n].view(np.uint16), np.asarray(ln)[eidx], err_msg=msg)
                assert (outs8[6][i] == SENT).all(), f"match destination written, {msg}"
                if compact:
                    np.testing.assert_array_equal(fhs[i], ofh[lo:lo + n], err_msg=msg)
                    np.testing.assert_array_equal(outs8[5][i][:4 * n].view(np.uint32), ofh[lo:lo + n][eidx],
                                                  err_msg=f"qfhash, {msg}")
                    assert (outs8[7][i] == SENT).all(), f"tcpinfo destination written, {msg}"
                else:
                    assert tis[i].tobytes() == oti[lo:lo + n].tobytes(), msg
                    np.testing.assert_array_equal(outs8[7][i][:TI * n].reshape(n, TI),
                                                  oti[lo:lo + n].view(np.uint8).reshape(n, TI)[eidx],
                                                  err_msg=f"qtcpinfo, {msg}")
                    assert (outs8[5][i] == SENT).all(), f"fhash destination written, {msg}"
                lo += n
    finally:
        one.set_direct(0)
        one.set_params(mosrx.default_params())
        for p in frees:
            one.host_free(p)


def test_steer_one_graph_replay(one):
    """mosrx_steer_gather_side_dev in its one-launch form captured into a graph
    (it allocates nothing) and replayed twice, the records, descriptors and side
    values replaced between the replays: the outputs follow them."""
    hip = C.CDLL("libamdhip64.so")
    n, rb = tile() + 77, 8
    rng = np.random.default_rng(31)
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0        # hipStreamNonBlocking
    h, d = synthetic(one, rng, "random", n, rb)
    sb = int(mosrx.lib().mosrx_steer_scratch_bytes(n))
    idx, qs, scr = Guarded(one, 4 * n), Guarded(one, 4 * QS), Guarded(one, sb)
    qrec, qoff, qlen = Guarded(one, rb * n), Guarded(one, 4 * n), Guarded(one, 2 * n)
    dst = {"fhash": Guarded(one, 4 * n), "match": Guarded(one, 4 * n), "tcpinfo": Guarded(one, TI * n)}
    try:
        before = one.steer_one_count()
        assert hip.hipStreamBeginCapture(stream, 1) == 0                # hipStreamCaptureModeThreadLocal
        one.steer_gather_side_dev(d["rec"].ptr, d["off"].ptr, d["len"].ptr, n, rb, idx.ptr, qs.ptr, qrec.ptr,
                                  qoff.ptr, qlen.ptr, scr.ptr, sb, sync=False, stream=stream.value,
                                  **{k: (d[k].ptr, dst[k].ptr) for k in ARRAYS})
        assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
        assert one.steer_one_count() - before == 1
        assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
        for rnd in range(2):
            if rnd:
                h2, d2 = synthetic(one, rng, "mod3", n, rb)
                for k in ("rec", "off", "len") + ARRAYS:
                    d[k].upload(h2[k])
                    d2[k].free()
                h = h2
            assert hip.hipGraphLaunch(gexec, stream) == 0
            assert hip.hipStreamSynchronize(stream) == 0
            out = (idx.read(), qs.read(), qrec.read(np.uint8), qoff.read(np.uint8), qlen.read(np.uint8),
                   {k: g.read(np.uint8) for k, g in dst.items()}, 1)
            check_form(h, n, rb, out, "side", True, ARRAYS, f"(replay {rnd})")
            assert (scr.read(np.uint8) == SENT).all()
    finally:
        if gexec:
            hip.hipGraphExecDestroy(gexec)
        if graph:
            hip.hipGraphDestroy(graph)
        hip.hipStreamDestroy(stream)
        for g in (idx, qs, scr, qrec, qoff, qlen, *dst.values(), *d.values()):
            g.free()
