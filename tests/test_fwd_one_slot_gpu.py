"""The one-launch forwarding form armed on a host group submit (mosrx_slot_fwd
with mosrx_set_fwd_one's limit set) and on the drop-in backend
(GpuBackend(fwd_one=)): the same checks as the four launches' tests
(tests/test_fwd_desc_slot_gpu.py, tests/test_fwd_desc_backend_gpu.py), against
the same restatements applied to each batch alone, with mosrx_fwd_one_count
saying which form ran.  A steer arm rides along with steer_one set -- three
dispatches a group -- and its outputs and the records are the bytes a submit
without forwarding leaves.  Expected values never come from the GPU."""
import ctypes as C

import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_oracle as F
import mosrx
import oracle_py as O
from test_direct_gpu import _pinned_like, _stage
from test_fwd_desc_backend_gpu import PARAMS, TABLES, backend, expected, traces
from test_fwd_desc_slot_gpu import IFS, NB, trace
from test_fwd_gpu import PAD, WALK, ee
from test_steer_gpu import BIG, GUARD, QS, SENT, expect

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("steer", [False, True])
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("compact", [False, True])
def test_slot_fwd_group_one_launch(gpu_ctx, direct, compact, steer):
    ctx = gpu_ctx
    t = trace()
    tab = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    params = dict(num_msp=1, forward=1, num_queues=4)
    frees = []
    rdt = mosrx.RESULT8_DTYPE if compact else mosrx.RESULT_DTYPE
    rb = rdt.itemsize

    def arr(dtype, k):
        if not direct:
            return np.zeros(k, dtype)
        p, a = _pinned_like(ctx, dtype, k)
        frees.append(p)
        return a

    try:
        ctx.set_params(mosrx.default_params(**params))
        ctx.fwd_set_listener(False)
        ctx.fwd_set(tab)
        base, blk = ctx.host_alloc(t.frames_bytes + 8 * t.n + 256 * (NB + 1))
        frees.append(base)
        batches, parts = _stage(blk, base, t, NB)
        assert max(b.n for b in batches) <= 512
        recs = [arr(rdt, b.n) for b in batches]
        shapes = ((np.uint64, lambda n: n + 1), (np.uint32, lambda n: n + PAD), (np.uint16, lambda n: n + PAD),
                  (np.uint8, lambda n: 12 * (n + PAD)), (mosrx.FWD_RING_DTYPE, lambda n: 4 + 2))
        outs = [[arr(dt, f(b.n)) for b in batches] for dt, f in shapes]           # plan, tx_src, tx_len, tx_mac, rings
        sizes_of = (lambda b: 4 * b.n, lambda b: 4 * QS, lambda b: rb * b.n, lambda b: 4 * b.n, lambda b: 2 * b.n)
        souts = [[arr(np.uint8, f(b) + GUARD) for b in batches] for f in sizes_of]
        ctx.set_direct(BIG if direct else 0)
        ctx.set_steer_one(2048 if steer else 0)

        def fill():
            for a in (a for g in outs for a in g):
                a.view(np.uint8)[...] = 0xEE
            for a in (a for g in souts for a in g):
                a[...] = SENT
            for r in recs:
                r.view(np.uint8)[...] = 0xEE

        def submit(fwd, with_plan=True):
            if steer:
                ctx.slot_steer_gather(1, *[[a.ctypes.data for a in g] for g in souts])
            if fwd:
                ctx.slot_fwd(1, ptrs[1], ptrs[2], ptrs[3], ptrs[4], nrings=4, in_ifidx=IFS, plan=ptrs[0] if with_plan else None)
            o = [r.ctypes.data for r in recs]
            if compact:
                ctx.group_submit_c8(1, batches, o)
            else:
                ctx.group_submit_ex(1, batches, o)
            ctx.group_wait(1)
            assert ctx.slot_direct(1) == direct

        ptrs = [[a.ctypes.data for a in g] for g in outs]
        # forwarding disarmed: the records and the steer outputs every armed submit below must leave as well
        fill()
        submit(False)
        plain = [r.tobytes() for r in recs], [a.tobytes() for g in souts for a in g]
        assert all((a.view(np.uint8) == 0xEE).all() for g in outs for a in g)
        for limit, one in ((512, True), (mosrx.FWD_ONE_MAX, True), (max(b.n for b in batches) - 1, False)):
            for with_plan in (True, False):
                ctx.set_fwd_one(limit)
                fill()
                c0, s0 = ctx.fwd_one_count(), ctx.steer_one_count()
                submit(True, with_plan)
                assert ctx.fwd_one_count() == c0 + (1 if one else 0), (limit, with_plan)
                assert ctx.steer_one_count() == s0 + (1 if steer else 0)
                assert ([r.tobytes() for r in recs], [a.tobytes() for g in souts for a in g]) == plain
                sent_total = 0
                for i, b in enumerate(batches):
                    fr, o, ln, fb = parts[i]
                    fr, o, ln = np.asarray(fr[:fb]), np.asarray(o), np.asarray(ln)
                    rec = O.classify(fr, o, ln, O.params(**params))
                    want = F.plan(fr, o, ln, rec["reason"], tab, IFS[i], forward=1, num_msp=1)
                    init = [ee(b.n + PAD, np.uint32), ee(b.n + PAD, np.uint16), ee(12 * (b.n + PAD), np.uint8),
                            ee(4 + 2, mosrx.FWD_RING_DTYPE)]
                    exp = FD.build(fr, o, want, tab, 4, *init)
                    m = int(exp[3]["count"][:4].sum())
                    sent_total += m
                    if with_plan:
                        assert outs[0][i][b.n] == 0xEEEEEEEEEEEEEEEE
                        assert np.array_equal(outs[0][i][:b.n], want.view(np.uint64)), (limit, i)
                    else:
                        assert (outs[0][i] == 0xEEEEEEEEEEEEEEEE).all()
                    assert outs[4][i].tobytes() == exp[3].tobytes(), (limit, i, outs[4][i], exp[3])
                    for k, per in ((1, 1), (2, 1), (3, 12)):
                        got, e = outs[k][i], exp[k - 1]
                        if direct:                                  # in place: exact, untouched past the sent count
                            assert got.tobytes() == e.tobytes(), (limit, k, i)
                        else:
                            assert np.array_equal(got[:m * per], e[:m * per]), (limit, k, i)
                            assert (got[b.n * per:].view(np.uint8) == 0xEE).all(), (limit, k, i)
                    if steer:
                        eidx, eqs = expect(rec["queue"])
                        np.testing.assert_array_equal(souts[0][i][:4 * b.n].view(np.uint32), eidx)
                        np.testing.assert_array_equal(souts[1][i][:4 * QS].view(np.uint32), eqs)
                assert sent_total > 300
        # refusals come before anything is submitted, as with the limit at 0
        ctx.set_fwd_one(512)
        c0 = ctx.fwd_one_count()
        ctx.slot_fwd(1, ptrs[1], ptrs[2], ptrs[3], ptrs[4], nrings=4)
        ctx.fwd_set(None)
        fill()
        with pytest.raises(mosrx.MosrxError) as e:
            ctx.group_submit_c8(1, batches, [r.ctypes.data for r in recs]) if compact else \
                ctx.group_submit_ex(1, batches, [r.ctypes.data for r in recs])
        assert e.value.errno == 2 and ctx.fwd_one_count() == c0                # ENOENT: no tables
        assert all((a.view(np.uint8) == 0xEE).all() for g in outs for a in g)
        assert all((r.view(np.uint8) == 0xEE).all() for r in recs)
    finally:
        ctx.set_fwd_one(0)
        ctx.set_steer_one(0)
        ctx.set_direct(0)
        ctx.set_params(mosrx.default_params())
        for p in frees:
            ctx.host_free(p)


def drain(be, trs, tab, check=True):
    """Every batch of both netdevs: its view against the restatement, then forward(); the frames sent per netdev."""
    sent, pos = [[], []], [0, 0]
    while True:
        any_rx = False
        for i in (0, 1):
            n = be.recv_pkts(i)
            assert n >= 0
            if not n:
                continue
            any_rx = True
            want, src, tl, mac, rings, lists, rec = expected(trs[i], i, pos[i], n, tab)
            got = be.fwd_view(i)
            assert got is not None
            if check:
                assert np.array_equal(got[0].view(np.uint64), want.view(np.uint64)), (i, pos[i])
                assert got[4].tobytes() == rings.tobytes(), (i, pos[i], got[4], rings)
                assert np.array_equal(got[1], src) and np.array_equal(got[2], tl) and np.array_equal(got[3], mac)
            rc, st = be.forward(i)
            assert rc == int(rings["count"][:2].sum()) == st.sent
            for q in range(2):
                sent[q] += lists[q]
            pos[i] += n
        if not any_rx:
            break
    assert pos == [len(trs[0][1]), len(trs[1][1])]
    return sent


@pytest.mark.parametrize("steer", [False, True])
@pytest.mark.parametrize("compact", [False, True])
def test_backend_view_and_forward(tmp_path, compact, steer):
    trs = traces()
    tab = mosrx.fwd_tables(**TABLES)
    pcaps = {}
    for fwd_one in (2048, 0):
        d = tmp_path / f"one{fwd_one}"
        d.mkdir()
        be, outs = backend(trs, d, compact=compact, steer=2 if steer else False, steer_one=2048 if steer else 0,
                           fwd_one=fwd_one)
        try:
            assert mosrx.lib().mosrx_gpu_module_get_fwd_one() == fwd_one
            sent = drain(be, trs, tab)
            count = be.fwd_one_count()
            assert (count > 0) if fwd_one else (count == 0)
            if fwd_one:
                assert count >= be.stats().rx_groups >= 5         # every group's batches fit: every group took it
        finally:
            be.close()
        assert len(sent[1]) > 300 and len(sent[0]) > 10
        pcaps[fwd_one] = [mosrx.read_pcap(o) for o in outs]
        assert pcaps[fwd_one] == sent                              # the restatement's frames per netdev, in order
    assert pcaps[2048] == pcaps[0]                                 # the same TX pcaps as with the option off
    assert mosrx.lib().mosrx_gpu_module_set_fwd_one(0) == 0


def test_backend_reclassified_batch_still_answers_minus_one():
    trs = traces()
    be, _ = backend(trs, group=3, fwd_one=2048)
    try:
        n = be.recv_pkts(0)
        assert n > 0 and be.fwd_view(0) is not None and be.fwd_one_count() > 0
        dummy = C.c_int(0)
        assert be.ioctl_raw(0, mosrx.PKT_RX_RECLASSIFY, C.byref(dummy)) == 0
        assert be.fwd_view(0) is None and be.forward(0)[0] == -1            # the exposed batch was touched
        n2 = be.recv_pkts(0)                                                 # the group's next batch keeps its plan
        assert n2 > 0 and be.fwd_view(0) is not None
        assert be.set_params(0, mosrx.default_params(**PARAMS)) == 0
        assert be.fwd_view(0) is None
        n3 = be.recv_pkts(0)                                                 # classified and armed again: one launch again
        want = expected(trs[0], 0, n + n2, n3, mosrx.fwd_tables(**TABLES))
        got = be.fwd_view(0)
        assert got is not None and np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
        assert got[4].tobytes() == want[4].tobytes()
    finally:
        be.close()
        mosrx.lib().mosrx_gpu_module_set_fwd_one(0)


def test_backend_hub_endpoint_still_has_no_view(monkeypatch):
    """A hub endpoint answers MOSRX_PKT_RX_FWD with -1, with the option set as without it."""
    import test_fwd_desc_backend_gpu as B
    made = []

    def with_option(*a, **kw):
        made.append(backend(*a, fwd_one=2048, **kw))
        return made[-1]
    monkeypatch.setattr(B, "backend", with_option)
    try:
        B.test_hub_endpoint_has_no_view()
        assert len(made) == 1
    finally:
        mosrx.lib().mosrx_gpu_module_set_fwd_one(0)
