"""The hub over the real backend with cfg.steer = 3, cfg.flowhash and a BPF set:
every core runs mosrx_rx_loop over its own endpoint on its own thread and, per
share, asks the endpoint for MOSRX_PKT_RX_QUEUE, MOSRX_PKT_RX_MATCH and
MOSRX_PKT_RX_FHASH.  For every batch the union over the cores of (frame index,
mask, hash) must be the oracle's per-frame values, no frame missing or doubled."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_bpf import random_sets

pytestmark = pytest.mark.gpu

JOIN_TIMEOUT = 60.0
MAX_ROUNDS = 200000
NQ = 4


@pytest.mark.parametrize("compact", [False, True])
def test_hub_endpoints_serve_gpu_masks_and_hashes(compact):
    T = int(mosrx.lib().mosrx_steer_tile())
    per = T + 50
    t = mosrx.Trace(mosrx.TRACE_IMIX, 2 * per + 37, nflows=600, seed=21)      # three batches, the last short
    ns = [per, per, 37]
    ps = random_sets(5, 1)[0][:4]
    orec, ofh = O.classify_fh(t.frames, t.off, t.len, O.params(num_queues=NQ))
    om = O.bpf_eval(ps, t.frames[:t.frames_bytes], t.off, t.len)
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    be = mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=NQ), batch=per, group=1, cpu=2,
                          compact=compact, steer=3, flowhash=True, bpf=ps)
    hub = None
    done, threads = threading.Event(), []
    try:
        hub = mosrx.Hub(C.addressof(be.m), be.ctx, 1, NQ)
        ioctl = mosrx._IOCTLFN(hub.m.dev_ioctl)
        shares = [[] for _ in range(NQ)]
        errors = []

        def consumer(c):
            ep = hub.endpoint(c)

            def consume(arg, ifidx, index, pkt, ln, res):
                if index != 0:
                    return
                v, side = mosrx.QueueView(), mosrx.QueueSide()       # a new share: its arrays, once
                pm, pf, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
                if (ioctl(ep, ifidx, mosrx.PKT_RX_QUEUE, C.byref(v)) or ioctl(ep, ifidx, mosrx.PKT_RX_MATCH, C.byref(pm))
                        or ioctl(ep, ifidx, mosrx.PKT_RX_FHASH, C.byref(pf))
                        or ioctl(ep, ifidx, mosrx.PKT_RX_QUEUE_SIDE, C.byref(side))):
                    errors.append((c, "an endpoint ioctl answered -1"))
                    return
                if ioctl(ep, ifidx, mosrx.PKT_RX_TCPINFO, C.byref(pt)) != -1:
                    errors.append((c, "RX_TCPINFO answered for a batch without pkt_info"))
                if side.match != pm.value or side.fhash != pf.value or side.tcpinfo or side.n != v.n:
                    errors.append((c, "RX_QUEUE_SIDE is not the share's own view"))
                n = int(v.n)
                shares[c].append((mosrx._queue_view_arrays(v)[3],
                                  np.ctypeslib.as_array(C.cast(pm, C.POINTER(C.c_uint32)), (n,)).copy(),
                                  np.ctypeslib.as_array(C.cast(pf, C.POINTER(C.c_uint32)), (n,)).copy()))
            return mosrx._PKTFN(consume)

        fns = [consumer(c) for c in range(NQ)]

        def core_loop(c):
            try:
                for _ in range(MAX_ROUNDS):
                    rc, st = hub.run_loop(c, fns[c])
                    if rc:
                        errors.append((c, rc))
                        return
                    if done.is_set():
                        return
                    if st.rx_packets == 0:
                        time.sleep(0.0002)
                errors.append((c, "round limit"))
            except Exception as e:   # noqa: BLE001 -- reported by the main thread
                errors.append((c, repr(e)))

        threads += [threading.Thread(target=core_loop, args=(c,), daemon=True) for c in range(1, NQ)]
        for th in threads:
            th.start()
        for _ in range(MAX_ROUNDS):
            h0 = hub.stats()
            rc, st = hub.run_loop(0, fns[0])
            assert rc == 0
            hs = hub.stats()
            # an idle round that was the backend's own: every share of the last batch went back
            if hs.frames == t.n and hs.batches == h0.batches and hs.owner_waits == h0.owner_waits:
                break
            if st.rx_packets == 0:
                time.sleep(0.0002)
        else:
            pytest.fail("the owner never drained the backend")
        done.set()
        for th in threads:
            th.join(JOIN_TIMEOUT)
        assert not [th for th in threads if th.is_alive()], "a core's loop did not end: the hub is stuck"
        assert not errors, errors
        assert hub.close() == 0
        assert hs.batches == len(ns) and hs.frames == hs.delivered == t.n
        # 600 flows over 4 queues: every core has frames in every batch, so share k of a core is batch k's
        assert [len(s) for s in shares] == [len(ns)] * NQ
        lo = 0
        for k, n in enumerate(ns):
            idx = np.concatenate([shares[c][k][0] for c in range(NQ)]).astype(np.int64)
            mt = np.concatenate([shares[c][k][1] for c in range(NQ)])
            fh = np.concatenate([shares[c][k][2] for c in range(NQ)])
            np.testing.assert_array_equal(np.sort(idx), np.arange(n), err_msg=f"batch {k}: a frame missing or doubled")
            np.testing.assert_array_equal(mt, om[lo + idx], err_msg=f"batch {k} masks")
            np.testing.assert_array_equal(fh, ofh[lo + idx], err_msg=f"batch {k} hashes")
            for c in range(NQ):
                assert (orec["queue"][lo + shares[c][k][0]] == c).all(), f"batch {k}, core {c}"
            lo += n
    finally:
        done.set()
        for th in threads:
            th.join(JOIN_TIMEOUT)
        if hub is not None and hub.handle and not [th for th in threads if th.is_alive()]:
            hub.close()
        be.close()
