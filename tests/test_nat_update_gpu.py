"""NAT bindings added and removed in place on the GPU (mosrx_nat_update) against
the restatement (tests/nat_oracle.py) over the resulting binding list, the list
index it reports mapped to the ids the updates gave.  Frames are NC.mix(n) packed
as tests/test_nat_gpu.py packs them; plans and xlat records are compared byte
for byte over 0xEE images with canaries.  Expected values never come from the
GPU."""
import ctypes as C

import numpy as np
import pytest

import fwd_rings_oracle as FR
import hostile as H
import mosrx
import nat_cases as NC
import nat_oracle as N
from test_nat import big
from test_nat_gpu import NatRun, same_records, trace
from test_nat_queue_gpu import Xlat, check_rings
from test_fwd_queue_gpu import Setup, split

pytestmark = pytest.mark.gpu

EINVAL, EEXIST, ENOENT = 22, 17, 2
NR = 4
# the flows of NC.mix's MISS frames (frame 25 g + 20): not bound by NC.bindings()
NEW = [("10.1.0.200", 5000 + g, "198.51.100.1", 80, 4000 + g) for g in range(21)]


class Model:
    """The binding list the updates leave, with the ids they gave."""

    def __init__(self, b):
        self.b, self.ids = [x.copy() for x in b], list(range(len(b)))

    def ops(self, adds=(), dels=()):
        """NAT_OP_DTYPE records (deletes first) and their effect on the list."""
        adds = [(mosrx.nat_bindings([f], NC.NAT_IP)[0] if isinstance(f, tuple) else f, i) for f, i in adds]
        for d in dels:
            k = [x.tobytes() for x in self.b].index(d.tobytes())
            del self.b[k], self.ids[k]
        for f, i in adds:
            self.b.append(f.copy())
            self.ids.append(i)
        return mosrx.nat_ops(adds=adds, dels=list(dels))

    def bindings(self):
        return np.array([x.item() for x in self.b], mosrx.NAT_BINDING_DTYPE)


def expect(tr, b, ids, t):
    """(xlat, plan, translated frames) of the restatement for bindings b under the ids."""
    buf, off, ln, rec = tr
    x, pl, out = N.plan(buf, off, ln, rec["reason"], b, t, 0)
    m = np.isin(x["kind"], [N.SNAT, N.DNAT])
    x["bind"][m] = np.asarray(ids, np.uint32)[x["bind"][m]]
    return x, pl, out


def prepare(ctx, b):
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    ctx.fwd_set_listener(False)
    t = mosrx.fwd_tables(**NC.TABLES)
    ctx.fwd_set(t)
    ctx.nat_set(b)
    return t


def run_check(r, want, what, **kw):
    """plan-nat over r's batch equals (xlat, plan) of want, canaries included."""
    r.d_xlat.upload(r.x_init)
    r.ctx.fwd_plan_nat_dev(r.db.batch(), r.d_rec.ptr, r.rb, 0, r.d_plan.ptr, r.d_xlat.ptr, **kw)
    verify(r, want, what)


def verify(r, want, what):
    same_records(r.plan_result(), want[1], (what, "plan"))
    ex = r.x_init.copy()
    ex[:r.n] = want[0]
    same_records(r.xlat(), ex, (what, "xlat"))


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("n", [1, 257, 513])
def test_basic_update(gpu_ctx, n, rec_bytes):
    ctx, tr = gpu_ctx, trace(n)
    a = NC.bindings()[:60]                                           # 256 slots, 120 keys: room for the adds in place
    t = prepare(ctx, a)
    m, st0 = Model(a), ctx.nat_stats()
    assert (st0.live, st0.tombs, st0.slots) == (60, 0, 256) and ctx.nat_count() == 60
    r = NatRun(ctx, *tr, rec_bytes)
    try:
        run_check(r, expect(tr, a, m.ids, t), "before")
        ops = m.ops(adds=[(NEW[0], 500), (NEW[1], 0xFFFFFFFE), (NEW[10], 7)], dels=[a[7], a[3], a[41], a[57]])
        ctx.nat_update(ops)
        st = ctx.nat_stats()
        assert (st.live, st.slots, st.rebuilds - st0.rebuilds, st.updates - st0.updates) == (59, 256, 0, 1)
        assert 2 <= st.tombs <= 8 and st.probe >= st0.probe and ctx.nat_count() == 59
        want = expect(tr, m.bindings(), m.ids, t)
        run_check(r, want, "after")
        if n == 513:
            x = want[0]
            assert {500, 0xFFFFFFFE, 7} <= set(x["bind"].tolist()) and not {3, 41, 57} & set(x["bind"][x["kind"] != 0].tolist())
        if n >= 257:
            assert want[0]["kind"][1] == N.MISS and want[0]["kind"][0] == N.SNAT     # binding 7's frame; binding 0's
    finally:
        r.free()


def test_collision_chain_on_the_device(gpu_ctx):
    ctx, tr = gpu_ctx, trace(513)
    a = NC.bindings()
    t = prepare(ctx, a)
    m, st0 = Model(a), ctx.nat_stats()
    head = NC.NPLAIN                                                 # first in: nearest the chain's home slot
    r = NatRun(ctx, *tr)
    try:
        before = expect(tr, a, m.ids, t)[0]
        ctx.nat_update(m.ops(dels=[a[head]]))
        st = ctx.nat_stats()
        assert (st.live, st.tombs, st.rebuilds - st0.rebuilds) == (63, 2, 0)
        want = expect(tr, m.bindings(), m.ids, t)
        run_check(r, want, "head deleted")
        x = want[0]
        was = np.isin(before["kind"], [N.SNAT, N.DNAT]) & (before["bind"] == head)
        assert was.sum() >= 4 and (x["kind"][was] == N.MISS).all()
        rest = np.isin(x["kind"], [N.SNAT, N.DNAT]) & (x["bind"] > head) & (x["bind"] < head + NC.NCOLL)
        assert set(x["bind"][rest].tolist()) == set(range(head + 1, head + NC.NCOLL))
        assert {int(k) for k in x["kind"][rest]} == {N.SNAT, N.DNAT}
    finally:
        r.free()


@pytest.mark.parametrize("own_first", [False, True], ids=["one_stream", "update_on_a_callers_stream"])
def test_stream_order_without_a_host_wait(gpu_ctx, own_first):
    """plan-nat, update, plan-nat with one synchronisation at the end: the first launch answers by
    the old table, the second by the new.  own_first: the first launch on the context's stream, the
    update and the second launch on a caller's."""
    hip = C.CDLL("libamdhip64.so")
    ctx, tr = gpu_ctx, trace(513)
    a = NC.bindings()[:60]
    t = prepare(ctx, a)
    m = Model(a)
    s = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(s), 1) == 0            # hipStreamNonBlocking
    r1, r2 = NatRun(ctx, *tr), NatRun(ctx, *tr)
    try:
        old = expect(tr, a, m.ids, t)
        ops = m.ops(adds=[(NEW[2], 900)], dels=[a[14]])                  # frame 2 is binding 14's; frame 70 the new flow's
        new = expect(tr, m.bindings(), m.ids, t)
        assert old[0]["kind"][2] == N.SNAT and new[0]["kind"][2] == N.MISS
        assert old[0]["kind"][70] == N.MISS and new[0]["kind"][70] == N.SNAT and new[0]["bind"][70] == 900
        first = None if own_first else s.value
        ctx.fwd_plan_nat_dev(r1.db.batch(), r1.d_rec.ptr, 16, 0, r1.d_plan.ptr, r1.d_xlat.ptr, sync=False, stream=first)
        ctx.nat_update(ops, stream=s.value)
        ctx.fwd_plan_nat_dev(r2.db.batch(), r2.d_rec.ptr, 16, 0, r2.d_plan.ptr, r2.d_xlat.ptr, sync=False, stream=s.value)
        assert hip.hipStreamSynchronize(s) == 0                          # the one wait (the second launch waited for the first's stream)
        mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
        verify(r1, old, "before the update")
        verify(r2, new, "after the update")
        assert ctx.nat_stats().live == 60
    finally:
        mosrx.lib().mosrx_sync(ctx.handle)
        hip.hipStreamSynchronize(s)
        r1.free()
        r2.free()
        hip.hipStreamDestroy(s)


def test_rebuild_path(gpu_ctx):
    ctx, tr = gpu_ctx, trace(257)
    a = NC.bindings()
    t = prepare(ctx, a[:4])
    m, st0 = Model(a[:4]), ctx.nat_stats()
    assert st0.slots == 16
    r = NatRun(ctx, *tr)
    try:
        for call in range(6):
            ids = [1000 + 6 * call + k for k in range(6)]
            ctx.nat_update(m.ops(adds=[(a[4 + 6 * call + k], ids[k]) for k in range(6)]))
            st = ctx.nat_stats()
            assert st.live == 10 + 6 * call == ctx.nat_count() and st.updates - st0.updates == call + 1
            if call in (0, 2):                                           # 4 -> 10 bindings: 16 slots cannot hold them; 16 -> 22: nor 64
                assert st.rebuilds - st0.rebuilds == (1, 2)[call // 2] and st.tombs == 0 and st.slots == (64, 128)[call // 2]
            assert st.slots >= 4 * st.live or st.slots == mosrx.lib().mosrx_nat_slots(st.live)
            want = expect(tr, m.bindings(), m.ids, t)
            run_check(r, want, ("call", call))
        x = want[0]
        assert st.rebuilds - st0.rebuilds >= 2 and {0, 1, 2, 3} <= set(x["bind"][np.isin(x["kind"], [1, 2])].tolist())
        assert set(x["bind"][np.isin(x["kind"], [1, 2])].tolist()) - {0, 1, 2, 3} <= set(range(1000, 1036))   # the ids survived
        # churn with flows that are new every time leaves tombstones until a call no longer fits: the rebuild holds none
        fresh = mosrx.nat_bindings([(f"10.77.{i // 200}.{1 + i % 200}", 10000 + i, "198.51.100.1", 80, 10000 + i) for i in range(96)],
                                   NC.NAT_IP)
        prev, rebuilt = [], False
        for cycle in range(12):
            cur, before = list(fresh[8 * cycle:8 * cycle + 8]), ctx.nat_stats()
            ctx.nat_update(m.ops(adds=[(f, 3000 + 8 * cycle + k) for k, f in enumerate(cur)], dels=prev))
            st, prev = ctx.nat_stats(), cur
            assert st.live == 40 + 8 and 2 * st.live + st.tombs <= st.slots // 2
            if st.rebuilds > before.rebuilds:
                assert st.tombs == 0 and st.slots == mosrx.lib().mosrx_nat_slots(st.live) and before.tombs > 0
                rebuilt = True
                break
            assert st.tombs > 0 or cycle == 0                            # (the first call deletes nothing)
        assert rebuilt
        run_check(r, expect(tr, m.bindings(), m.ids, t), "after the tombstones")
    finally:
        r.free()


def test_full_pool_in_place(gpu_ctx):
    ctx, tr = gpu_ctx, trace(513)
    rest = big(mosrx.NAT_MAX_BINDINGS - NC.NBIND + 500)
    rest["svr_ip"] = mosrx.ip_raw("203.0.113.7")                         # another server: every key apart from the trace's
    rest["svr_ip"][-500:] = mosrx.ip_raw("203.0.113.8")                  # (and the 500 to come apart from those,
    rest["nat_port"][-500:] = [mosrx._htons(20000 + k) for k in range(500)]   # with NAT ports of their own: big()'s run past 65535)
    b = np.concatenate([NC.bindings(), rest[:-500]])
    t = prepare(ctx, b)
    st0 = ctx.nat_stats()
    assert (st0.live, st0.slots) == (mosrx.NAT_MAX_BINDINGS, 1 << 18)
    # 500 out: 20 of the trace's own and 480 others; 500 in: the trace's new flows and others
    dels = [b[i] for i in range(0, 60, 3)] + [b[i] for i in range(1000, 1480)]
    new = mosrx.nat_bindings(NEW, NC.NAT_IP)
    adds = [(new[i], 70000 + i) for i in range(len(new))] + [(rest[len(rest) - 500 + i], 80000 + i) for i in range(500 - len(new))]
    assert len(dels) == len(adds) == 500
    keep = np.ones(len(b), bool)
    keep[list(range(0, 60, 3)) + list(range(1000, 1480))] = False
    after = np.concatenate([b[keep], np.array([f.item() for f, _ in adds], mosrx.NAT_BINDING_DTYPE)])
    ids = np.concatenate([np.nonzero(keep)[0], [i for _, i in adds]]).astype(np.uint32)
    r = NatRun(ctx, *tr)
    try:
        ctx.nat_update(mosrx.nat_ops(adds=adds, dels=dels))
        st = ctx.nat_stats()
        assert st.rebuilds == st0.rebuilds and st.live == mosrx.NAT_MAX_BINDINGS and st.slots == 1 << 18   # in place
        assert 0 < st.tombs <= 1000 and 2 * st.live + st.tombs <= 1 << 17
        want = expect(tr, after, ids, t)
        x = want[0]
        xl = np.isin(x["kind"], [N.SNAT, N.DNAT])
        assert (x["bind"][xl] >= 70000).sum() >= 15 and (x["bind"][xl] < 64).sum() > 200      # added and untouched flows
        old = expect(tr, NC.bindings(), np.arange(64), t)[0]
        assert (np.isin(old["kind"], [N.SNAT, N.DNAT]) & (x["kind"] == N.MISS)).sum() > 50        # deleted ones
        run_check(r, want, "full pool")
    finally:
        r.free()
        ctx.nat_set(None)


def test_queue_run_after_an_update(gpu_ctx):
    ctx, ns = gpu_ctx, [257, 1]
    s = Setup(ctx, split(NC.mix(sum(ns)), ns, (2, 7, 0, 13, 1, 11)))
    xl = None
    try:
        a = NC.bindings()[:60]
        t = prepare(ctx, a)
        m = Model(a)

        def answers():
            return [expect((b, o, l, rec), m.bindings(), m.ids, t) for (b, o, l), rec in zip(s.batches, s.rec)]
        want = answers()
        cap = max(int(FR.need_units(w[1], NR).max()) for w in want) * 16
        q, out, xl = s.queue(), s.outputs(cap, NR), Xlat(ctx, ns)
        out.attach(q)
        q.set_nat(xl.ptrs())
        q.run()
        check_rings(s, out, t, want)
        xl.check([w[0] for w in want])
        # frame 257 (the second batch's only one) is binding (10 * 20 + 7) * 7 % 64 = 41's: deleted; frame 20's flow bound
        ctx.nat_update(m.ops(adds=[(NEW[0], 321)], dels=[a[41], a[0]]))
        want2 = answers()
        assert want[1][0]["kind"][0] == N.DNAT and want2[1][0]["kind"][0] == N.MISS and want2[0][0]["bind"][20] == 321
        out.fill()
        xl.fill()
        q.run()
        check_rings(s, out, t, want2)
        xl.check([w[0] for w in want2])
    finally:
        s.close()
        if xl:
            xl.free()


def test_refused_updates_launch_nothing(gpu_ctx):
    ctx, tr = gpu_ctx, trace(257)
    a = NC.bindings()[:60]
    t = prepare(ctx, a)
    m = Model(a)
    ctx.nat_update(m.ops(dels=[a[9]]))                                   # (a tombstone in the table)
    st0, want = ctx.nat_stats(), expect(tr, m.bindings(), m.ids, t)
    new = mosrx.nat_bindings(NEW[:4], NC.NAT_IP)
    ok = mosrx.nat_ops(adds=[(new[0], 1), (new[1], 2)], dels=[a[5]])
    zero_port = new[2].copy()
    zero_port["nat_port"] = 0
    r = NatRun(ctx, *tr)
    try:
        for bad, errno in ((mosrx.nat_ops(adds=[(a[20], 5)]), EEXIST), (mosrx.nat_ops(dels=[a[9]]), ENOENT),
                           (mosrx.nat_ops(dels=[new[3]]), ENOENT), (mosrx.nat_ops(adds=[(new[2], mosrx.NAT_NO_BIND)]), EINVAL),
                           (mosrx.nat_ops(adds=[(zero_port, 5)]), EINVAL), (mosrx.nat_ops(adds=[(new[0], 9)]), EEXIST)):
            ops = np.concatenate([ok, bad])
            with pytest.raises(mosrx.MosrxError) as e:
                ctx.nat_update(ops)
            assert e.value.errno == errno, (bad, errno)
            assert ctx.nat_stats() == st0 and ctx.nat_count() == 59
        bad_op = ok.copy()
        bad_op["op"][1] = 3
        with pytest.raises(mosrx.MosrxError) as e:
            ctx.nat_update(bad_op)
        assert e.value.errno == EINVAL and ctx.nat_stats() == st0
        ctx.nat_update(ok[:0])                                           # no ops: nothing done
        assert ctx.nat_stats() == st0
        run_check(r, want, "after the refusals")                         # still the old table
        with mosrx.Context(0) as fresh:                                  # never set: as the empty table
            with pytest.raises(mosrx.MosrxError) as e:
                fresh.nat_update(mosrx.nat_ops(dels=[a[0]]))
            assert e.value.errno == ENOENT and fresh.nat_stats().slots == 0
            # more adds than the empty table's 16 slots hold, then an op to refuse: still nothing installed
            with pytest.raises(mosrx.MosrxError) as e:
                fresh.nat_update(np.concatenate([mosrx.nat_ops(adds=[(a[i], i) for i in range(5)]), mosrx.nat_ops(dels=[a[9]])]))
            assert e.value.errno == ENOENT and fresh.nat_stats() == (0, 0, 0, 0, 0, 0) and fresh.nat_count() == 0
            with pytest.raises(mosrx.MosrxError) as e:                   # more ops than MOSRX_NAT_UPDATE_MAX_OPS
                fresh.nat_update(np.zeros(mosrx.NAT_UPDATE_MAX_OPS + 1, mosrx.NAT_OP_DTYPE))
            assert e.value.errno == EINVAL and fresh.nat_stats().slots == 0
            fresh.nat_update(mosrx.nat_ops(adds=[(a[0], 11)]))
            assert fresh.nat_stats()[:3] == (1, 0, 16) and fresh.nat_count() == 1
            mosrx._chk(mosrx.lib().mosrx_sync(fresh.handle), "sync")
    finally:
        r.free()


def test_hostile_frames_after_churn(gpu_ctx):
    ctx, h = gpu_ctx, H.batch()
    a = H.bindings()                                                     # 40 of the 80 flows: 256 slots, 80 keys
    t = prepare(ctx, a)
    m, rng = Model(a), np.random.default_rng(0xC4021)
    free = [(c, cp, s, sp, 2000 + i) for i, (c, cp, s, sp) in enumerate(H.COMBOS) if not H.bound(i)]
    free = list(mosrx.nat_bindings(free, H.NAT_IP))
    st0, next_id = ctx.nat_stats(), 100
    for call in range(6):                                                # at most 24 deletes: 80 keys and 48 tombstones fit
        k = int(rng.integers(1, 5))
        dels = [m.b[i] for i in rng.choice(len(m.b), k, replace=False)]
        adds = [(free.pop(int(rng.integers(len(free)))), next_id + j) for j in range(min(k, len(free)))]
        ctx.nat_update(m.ops(adds=adds, dels=dels))
        free += dels
        next_id += k
    st = ctx.nat_stats()
    assert st.tombs > 0 and st.rebuilds == st0.rebuilds and st.live == len(m.b) == 40
    tr = (h.buf, h.off, h.ln, h.rec)
    want = expect(tr, m.bindings(), m.ids, t)
    for rb in (16, 8):
        r = NatRun(ctx, *tr, rb)
        try:
            run_check(r, want, ("hostile", rb))
            got = r.xlat()[:r.n]
        finally:
            r.free()
        assert set(got["bind"][got["kind"] != N.NONE].tolist()) <= set(m.ids) | {mosrx.NAT_NO_BIND}
        assert {int(k) for k in got["kind"]} == {N.NONE, N.SNAT, N.DNAT, N.MISS, N.HOST}
        assert (got["bind"][np.isin(got["kind"], [N.SNAT, N.DNAT])] >= 100).any()
