"""mosrx_gpu_module_set_steer_one in the drop-in backend and under the hub: small batches of a
memory source go out as direct groups, each steered by the one launch; the
views and the endpoints serve what they serve with the three launches -- the
oracle's per-queue runs."""
import ctypes as C

import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_steer_gpu import expect

pytestmark = pytest.mark.gpu

NQ = 4
N = 3000


def _trace():
    return mosrx.Trace(mosrx.TRACE_IMIX, N, nflows=700, seed=13)


def _backend(t, compact, nq=NQ):
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    return mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=nq), batch=256, group=3, cpu=2,
                            compact=compact, steer=3, flowhash=True, steer_one=mosrx.STEER_ONE_MAX)


@pytest.mark.parametrize("compact", [False, True])
def test_backend_steer_one_views(compact):
    """Every MOSRX_PKT_RX_QUEUE / RX_QUEUE_SIDE view equals the oracle's
    per-queue run of its batch, and the groups took the one-launch form."""
    t = _trace()
    orec, ofh = O.classify_fh(t.frames, t.off, t.len, O.params(num_queues=NQ))
    be = _backend(t, compact)
    try:
        seen = 0
        while True:
            n = be.recv_pkts(0)
            assert n >= 0
            if n == 0:
                break
            got = (be.results8(0, n) if compact else be.results(0, n))
            np.testing.assert_array_equal(got["queue"], orec["queue"][seen:seen + n])
            idx, qs, nq = be.steer_view(0)
            eidx, eqs = expect(orec["queue"][seen:seen + n])
            assert nq == NQ
            np.testing.assert_array_equal(qs, eqs, err_msg=f"batch@{seen}")
            np.testing.assert_array_equal(idx, eidx, err_msg=f"batch@{seen}")
            rb = 8 if compact else 16
            raw = got.view(np.uint8).reshape(n, rb)
            total = 0
            for q in range(256):
                mine = eidx[eqs[q]:eqs[q + 1]]
                view = be.queue_view(0, q)
                assert view is not None
                np.testing.assert_array_equal(view[3], mine, err_msg=f"queue {q} @{seen}")
                np.testing.assert_array_equal(np.asarray(view[0]).view(np.uint8).reshape(len(mine), rb), raw[mine],
                                              err_msg=f"queue {q} @{seen}")
                np.testing.assert_array_equal(view[2], t.len[seen:seen + n][mine], err_msg=f"queue {q} @{seen}")
                qfh, qmt, qti = be.queue_side(0, q)
                assert qmt is None and qti is None
                np.testing.assert_array_equal(qfh, ofh[seen:seen + n][mine], err_msg=f"queue {q} @{seen}")
                total += len(mine)
            assert total == n
            seen += n
        assert seen == t.n
        assert be.steer_one_count() > 0
    finally:
        be.close()


@pytest.mark.parametrize("compact", [False, True])
def test_hub_over_steer_one_backend(compact):
    """Two cores over that backend, both endpoints driven round robin from one
    thread: each endpoint's frames, records and RX_FHASH are the oracle's for
    its queue, in trace order."""
    ncores = 2
    t = _trace()
    orec, ofh = O.classify_fh(t.frames, t.off, t.len, O.params(num_queues=ncores))
    be = _backend(t, compact, nq=ncores)
    hub = None
    try:
        hub = mosrx.Hub(C.addressof(be.m), be.ctx, 1, ncores)
        ioctl = mosrx._IOCTLFN(hub.m.dev_ioctl)
        got = [[] for _ in range(ncores)]
        hashes = [[] for _ in range(ncores)]
        errors = []

        def consumer(c):
            ep = hub.endpoint(c)

            def consume(arg, ifidx, index, pkt, ln, res):
                r = res.contents
                if index == 0:                      # a new share: its hashes, once
                    v, pf = mosrx.QueueView(), C.c_void_p()
                    if ioctl(ep, ifidx, mosrx.PKT_RX_QUEUE, C.byref(v)) or ioctl(ep, ifidx, mosrx.PKT_RX_FHASH,
                                                                                   C.byref(pf)):
                        errors.append((c, "an endpoint ioctl answered -1"))
                        return
                    hashes[c].append(np.ctypeslib.as_array(C.cast(pf, C.POINTER(C.c_uint32)), (int(v.n),)).copy())
                got[c].append((r.rss, r.queue, r.reason, r.verdict, r.tcp_flags, ln, C.string_at(pkt, ln)))
            return mosrx._PKTFN(consume)

        fns = [consumer(c) for c in range(ncores)]
        for _ in range(20000):
            h0 = hub.stats()
            for c in range(ncores):
                rc, st = hub.run_loop(c, fns[c])
                assert rc == 0
            hs = hub.stats()
            if hs.frames == t.n and hs.delivered == t.n and hs.batches == h0.batches:
                break
        else:
            pytest.fail("the hub never drained the backend")
        assert not errors, errors
        assert be.steer_one_count() > 0
        assert hub.close() == 0
        for c in range(ncores):
            mine = np.nonzero(orec["queue"] == c)[0]
            assert len(got[c]) == len(mine), f"core {c}"
            for k, i in enumerate(mine):
                o, ln = int(t.off[i]), int(t.len[i])
                want = (int(orec["rss"][i]), c, int(orec["reason"][i]), int(orec["verdict"][i]),
                        int(orec["tcp_flags"][i]), ln, t.frames[o:o + ln].tobytes())
                assert got[c][k] == want, f"core {c}, its frame {k} (trace frame {i})"
            np.testing.assert_array_equal(np.concatenate(hashes[c]), ofh[mine], err_msg=f"core {c} hashes")
    finally:
        if hub is not None and hub.handle:
            hub.close()
        be.close()
