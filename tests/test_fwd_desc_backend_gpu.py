"""Forwarding on the drop-in backend (mosrx_gpu_module_set_fwd, MOSRX_PKT_RX_FWD,
mosrx_backend_forward): GpuBackend over memory sources of mixed frames on two
netdevs, batches small enough for several batches and groups.  The view of every
batch equals the restatements applied to that batch alone (fwd_oracle.plan on
oracle_py.classify's reasons with in_ifidx = the netdev, fwd_desc_oracle.build),
and after forward() each source's TX pcap holds the restatement's frames for
that netdev, in order.  Expected values never come from the GPU."""
import ctypes as C

import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_oracle as F
import mosrx
import oracle_py as O
from test_fwd_desc_gpu import mixed
from test_fwd_gpu import PAD, WALK, ee, pack_at

pytestmark = pytest.mark.gpu

PARAMS = dict(num_msp=1, forward=1)
# netdev 0 takes the nic_forward_table shortcut to netdev 1; netdev 1 walks the tables (netdevs 0 .. 3)
TABLES = dict(WALK, nic_fwd={0: 1})
BATCH = 96


def traces():
    a = pack_at(mixed(500), [2, 9, 0, 7])
    b = pack_at(mixed(430)[::-1], [0, 5])
    return a, b


def expected(tr, ifidx, lo, n, tab):
    """The restatement's (plan, tx_src, tx_len, tx_mac, rings, frames per ring) for frames lo .. lo + n of a trace."""
    buf, off, ln = tr
    o, l = off[lo:lo + n], ln[lo:lo + n]
    rec = O.classify(buf, o, l, O.params(**PARAMS))
    want = F.plan(buf, o, l, rec["reason"], tab, ifidx, forward=1, num_msp=1)
    init = [ee(n + PAD, np.uint32), ee(n + PAD, np.uint16), ee(12 * (n + PAD), np.uint8), ee(4 + 2, mosrx.FWD_RING_DTYPE)]
    src, tl, mac, rings = FD.build(buf, o, want, tab, 4, *init)
    m = int(rings["count"][:4].sum())
    lists = [FD.ring_list(buf, o, src, tl, mac, rings, q) for q in range(4)]
    return want, src[:m], tl[:m], mac[:12 * m], rings[:4], lists, rec


def backend(trs, tmp_path=None, fwd=True, compact=False, group=2, steer=False, **kw):
    srcs = [mosrx.mem_source(b, o, l, loops=1) for b, o, l in trs]
    outs = []
    if tmp_path is not None:
        for i, s in enumerate(srcs):
            outs.append(str(tmp_path / f"tx{i}.pcap"))
            mosrx.source_tx_pcap(s, outs[-1])
    be = mosrx.GpuBackend(srcs, params=mosrx.default_params(**PARAMS, **({"num_queues": 2} if steer else {})),
                          batch=BATCH, group=group, cpu=9, compact=compact, steer=steer,
                          fwd=mosrx.fwd_tables(**TABLES) if fwd else None, **kw)
    return be, outs


@pytest.mark.parametrize("direct_kb", [None, 0])
@pytest.mark.parametrize("compact", [False, True])
def test_view_and_forward_equal_the_oracle(tmp_path, compact, direct_kb):
    """direct_kb None: the default, small groups written in place; 0: every group copied back."""
    trs = traces()
    tab = mosrx.fwd_tables(**TABLES)
    be, outs = backend(trs, tmp_path, compact=compact, direct_kb=direct_kb)
    sent = [[], []]
    pos, batches, total = [0, 0], 0, mosrx.FwdSendStats()
    try:
        assert be.fwd_view(0) is None                           # no batch exposed yet
        while True:
            any_rx = False
            for i in (0, 1):
                n = be.recv_pkts(i)
                assert n >= 0
                if not n:
                    continue
                any_rx = True
                batches += 1
                want, src, tl, mac, rings, lists, rec = expected(trs[i], i, pos[i], n, tab)
                got = be.fwd_view(i)
                assert got is not None
                assert np.array_equal(got[0].view(np.uint64), want.view(np.uint64)), (i, pos[i])
                assert got[4].tobytes() == rings.tobytes(), (i, pos[i], got[4], rings)
                assert np.array_equal(got[1], src) and np.array_equal(got[2], tl) and np.array_equal(got[3], mac)
                rc, st = be.forward(i)
                # the backend has netdevs 0 and 1: frames routed to 2 and 3 find no TX buffer there
                assert rc == int(rings["count"][:2].sum()) == st.sent
                assert st.no_buffer == int(rings["count"][2:].sum())
                assert st.send_calls == int((rings["count"] > 0).sum())
                for q in range(2):
                    sent[q] += lists[q]
                pos[i] += n
            if not any_rx:
                break
        assert pos == [len(trs[0][1]), len(trs[1][1])] and batches >= 10
        ms = be.stats()
        assert ms.rx_groups >= 5
    finally:
        be.close()
    # netdevs 0 and 1 have sources: their TX pcaps hold the oracle's frames for them, in order
    # (frames of one netdev from the two input netdevs interleave batch by batch, as sent above)
    assert len(sent[1]) > 300 and len(sent[0]) > 10
    assert mosrx.read_pcap(outs[0]) == sent[0]
    assert mosrx.read_pcap(outs[1]) == sent[1]


def test_view_is_refused_when_it_must_be(tmp_path):
    trs = traces()
    # forwarding off: -1, and forward() hands the -1 on
    be, _ = backend(trs, fwd=False)
    try:
        assert be.recv_pkts(0) > 0
        assert be.fwd_view(0) is None and be.forward(0)[0] == -1
    finally:
        be.close()
    be, _ = backend(trs, group=3)
    try:
        n = be.recv_pkts(0)
        assert n > 0 and be.fwd_view(0) is not None
        dummy = C.c_int(0)
        assert be.ioctl_raw(0, mosrx.PKT_RX_RECLASSIFY, C.byref(dummy)) == 0
        assert be.fwd_view(0) is None and be.forward(0)[0] == -1            # the exposed batch was touched
        assert be.fwd_view(1) is None                                        # nothing exposed on netdev 1
        n2 = be.recv_pkts(0)                                                 # the group's next batch keeps its plan
        assert n2 > 0 and be.fwd_view(0) is not None
        assert be.set_params(0, mosrx.default_params(**PARAMS)) == 0
        assert be.fwd_view(0) is None                                        # SET_PARAMS touched it
        n3 = be.recv_pkts(0)                                                 # classified again under the new state, armed again
        assert n3 > 0
        want = expected(trs[0], 0, n + n2, n3, mosrx.fwd_tables(**TABLES))
        got = be.fwd_view(0)
        assert got is not None and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
        assert got[4].tobytes() == want[4].tobytes()
    finally:
        be.close()
    # bad tables: refused, the setting stays as it was
    L = mosrx.lib()
    L.mosrx_gpu_module_set_fwd.restype = C.c_int
    L.mosrx_gpu_module_set_fwd.argtypes = [C.POINTER(mosrx.FwdTables), C.c_int]
    bad = mosrx.fwd_tables(**TABLES)
    bad.routes[0].nif = 9
    assert L.mosrx_gpu_module_set_fwd(C.byref(bad), 0) == -22
    bad = mosrx.fwd_tables(**TABLES)
    bad.num_arp = mosrx.FWD_MAX_ARP + 1
    assert L.mosrx_gpu_module_set_fwd(C.byref(bad), 0) == -22
    assert L.mosrx_gpu_module_set_fwd(None, 0) == 0


def test_hub_endpoint_has_no_view():
    trs = traces()[:1]
    be, _ = backend(trs, steer=2)
    hub = None
    try:
        hub = mosrx.Hub(C.addressof(be.m), be.ctx, 1, 2)
        ioctl = mosrx._IOCTLFN(hub.m.dev_ioctl)
        answers = []

        def consumer(c):
            ep = hub.endpoint(c)

            def consume(arg, ifidx, index, pkt, ln, res):
                if index == 0:
                    v = mosrx.FwdView()
                    answers.append(ioctl(ep, ifidx, mosrx.PKT_RX_FWD, C.byref(v)))
            return mosrx._PKTFN(consume)

        fns = [consumer(c) for c in range(2)]
        v = mosrx.FwdView()
        assert ioctl(hub.endpoint(0), 0, mosrx.PKT_RX_FWD, C.byref(v)) == -1
        for _ in range(2000):
            h0 = hub.stats()
            for c in range(2):
                rc, st = hub.run_loop(c, fns[c])
                assert rc == 0
            hs = hub.stats()
            if hs.frames == len(trs[0][1]) and hs.delivered == hs.frames and hs.batches == h0.batches:
                break
        else:
            pytest.fail("the hub never drained the backend")
        assert answers and all(a == -1 for a in answers)
        assert hub.close() == 0
        hub = None
    finally:
        if hub is not None:
            hub.close()
        be.close()


@pytest.mark.parametrize("compact", [False, True])
def test_everything_else_answers_as_with_forwarding_unset(compact):
    """Records, RSS, state, flow hashes and the steer view of every batch: the same bytes with forwarding set and unset."""
    trs = traces()

    def run(fwd):
        be, _ = backend(trs, fwd=fwd, compact=compact, steer=1, flowhash=True)
        out = []
        try:
            while True:
                any_rx = False
                for i in (0, 1):
                    n = be.recv_pkts(i)
                    assert n >= 0
                    if not n:
                        continue
                    any_rx = True
                    st = (C.c_uint32 * 6)()                    # mosrx_rx_state
                    assert be.ioctl_raw(i, mosrx.PKT_RX_STATE, C.byref(st)) == 0
                    idx, qs, nq = be.steer_view(i)
                    rec = be.results8(i, n) if compact else be.results(i, n)
                    p = C.c_void_p()
                    other = be.ioctl_raw(i, mosrx.PKT_RX_RESULTS if compact else mosrx.PKT_RX_RESULTS8, C.byref(p))
                    out.append((i, n, rec.tobytes(), be.fhashes(i, n).tobytes(), idx.tobytes(), qs.tobytes(), nq,
                                be.rss_of(i, 0), be.rss_of(i, n - 1), be.get_rptr(i, n - 1), bytes(st), other,
                                be.ioctl_raw(i, mosrx.PKT_RX_MATCH, C.byref(p)),
                                be.ioctl_raw(i, mosrx.PKT_RX_TCPINFO, C.byref(p)), be.queue_view(i, 0)))
                if not any_rx:
                    break
        finally:
            be.close()
        return out

    a, b = run(False), run(True)
    assert len(a) >= 10 and a == b
