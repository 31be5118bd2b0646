"""The hub over the real backend (gpu_module_func, cfg.steer = 2) and a memory
source: every core runs mosrx_rx_loop over its own endpoint on its own thread,
core 0 (the owner) on the thread that opened the backend.  Batches cut the
trace in arrival order and a queue keeps arrival order within a batch, so core
c must see exactly the oracle's frames of queue c, in trace order."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import mosrx
import oracle_py as O

pytestmark = pytest.mark.gpu

JOIN_TIMEOUT = 60.0
MAX_ROUNDS = 200000
NQ = 4


@pytest.mark.parametrize("ncores", [2, 4])
@pytest.mark.parametrize("compact", [False, True])
def test_hub_over_gpu_backend(compact, ncores):
    T = int(mosrx.lib().mosrx_steer_tile())
    per = T + 50
    t = mosrx.Trace(mosrx.TRACE_IMIX, 2 * per + 37, nflows=600, seed=21)      # three batches, the last short
    ora = O.classify(t.frames, t.off, t.len, O.params(num_queues=NQ))
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=1)
    be = mosrx.GpuBackend([src], params=mosrx.default_params(num_queues=NQ), batch=per, group=1, cpu=2,
                          compact=compact, steer=2)
    hub = None
    done, threads = threading.Event(), []
    try:
        hub = mosrx.Hub(C.addressof(be.m), be.ctx, 1, ncores)
        ioctl = mosrx._IOCTLFN(hub.m.dev_ioctl)
        got = [[] for _ in range(ncores)]
        shares = [[] for _ in range(ncores)]

        def consumer(c):
            ep = hub.endpoint(c)

            def consume(arg, ifidx, index, pkt, ln, res):
                r = res.contents
                if index == 0:                      # a new share: its view, once
                    v = mosrx.QueueView()
                    assert ioctl(ep, ifidx, mosrx.PKT_RX_QUEUE, C.byref(v)) == 0
                    shares[c].append(mosrx._queue_view_arrays(v)[3])
                got[c].append((index, r.rss, r.queue, r.reason, r.verdict, r.tcp_flags, ln, C.string_at(pkt, ln)))
            return mosrx._PKTFN(consume)

        fns = [consumer(c) for c in range(ncores)]
        errors = []

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

        threads += [threading.Thread(target=core_loop, args=(c,), daemon=True) for c in range(1, ncores)]
        for th in threads:
            th.start()
        # the owner, on this thread: until the source is dry and every share went back
        # an idle round that was not a wait for a share is the backend's own: the
        # countdown was zero, so every share of the last batch went back
        for _ in range(MAX_ROUNDS):
            h0 = hub.stats()
            rc, st = hub.run_loop(0, fns[0])
            assert rc == 0
            hs = hub.stats()
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
        assert hs.batches == 3 and hs.frames == t.n
        owned = int((ora["queue"] < ncores).sum())
        assert hs.delivered == owned == sum(len(g) for g in got)
        assert hs.unowned == t.n - owned and hs.delivered + hs.unowned == t.n
        assert (hs.unowned > 0) == (ncores < NQ)
        for c in range(ncores):
            members = np.nonzero(ora["queue"] == c)[0]
            assert len(got[c]) == len(members), f"core {c}"
            o = ora[members]
            a = got[c]
            np.testing.assert_array_equal([g[1] for g in a], o["rss"], err_msg=f"core {c} rss")
            np.testing.assert_array_equal([g[2] for g in a], o["queue"])
            np.testing.assert_array_equal([g[3] for g in a], o["reason"])
            np.testing.assert_array_equal([g[4] for g in a], o["verdict"])
            np.testing.assert_array_equal([g[5] for g in a], o["tcp_flags"])
            np.testing.assert_array_equal([g[6] for g in a], t.len[members])
            for g, m in zip(a, members):
                o0 = int(t.off[m])
                assert g[7] == t.frames[o0:o0 + int(t.len[m])].tobytes(), f"core {c}, frame {m}"
            # each share is a contiguous ring (indices 0 .. n - 1) whose idx is the batch-local partition
            starts = [k for k, g in enumerate(a) if g[0] == 0]
            assert len(starts) == len(shares[c])
            pos = 0
            for s, idx in zip(starts, shares[c]):
                assert [g[0] for g in a[s:s + len(idx)]] == list(range(len(idx)))
                assert (np.diff(idx.astype(np.int64)) > 0).all()
                pos += len(idx)
            assert pos == len(a)
    finally:
        done.set()
        for th in threads:
            th.join(JOIN_TIMEOUT)
        if hub is not None and hub.handle and not [th for th in threads if th.is_alive()]:
            hub.close()
        be.close()
