"""mosrx_slot_fwd: the plan and the descriptor form of the ring build armed on a
host group submit, against the restatements applied to each batch alone
(fwd_oracle.plan on oracle_py.classify's reasons, fwd_desc_oracle.build).

Direct groups with pinned outputs are written in place and compared exactly
over 0xEE images with canaries; copied groups overwrite all n entries of each
array, so there the entries below the sent count, the rings and the canaries
are compared.  Expected values never come from the GPU."""
import ctypes as C
import types

import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_direct_gpu import _pinned_like, _stage
from test_fwd_desc_gpu import mixed
from test_fwd_gpu import PAD, WALK, ee, pack_at
from test_steer_gpu import BIG, GUARD, QS, SENT, expect

pytestmark = pytest.mark.gpu

EINVAL, ENOENT, EBUSY = 22, 2, 16
NB = 3
IFS = [0, 1, 0]


def trace():
    buf, off, ln = pack_at(mixed(2 * 256 + 100), [0])          # 16-byte aligned frames: a direct group reads them in place
    return types.SimpleNamespace(frames=buf, off=off, len=ln, n=len(off), frames_bytes=len(buf))


@pytest.mark.parametrize("steer", [False, True])
@pytest.mark.parametrize("direct", [False, True])
@pytest.mark.parametrize("compact", [False, True])
def test_slot_fwd_group(gpu_ctx, direct, compact, steer):
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
        recs = [arr(rdt, b.n) for b in batches]
        shapes = ((np.uint64, lambda n: n + 1), (np.uint32, lambda n: n + PAD), (np.uint16, lambda n: n + PAD),
                  (np.uint8, lambda n: 12 * (n + PAD)), (mosrx.FWD_RING_DTYPE, lambda n: 4 + 2))
        outs = [[arr(dt, f(b.n)) for b in batches] for dt, f in shapes]           # plan, tx_src, tx_len, tx_mac, rings
        sizes_of = (lambda b: 4 * b.n, lambda b: 4 * QS, lambda b: rb * b.n, lambda b: 4 * b.n, lambda b: 2 * b.n)
        souts = [[arr(np.uint8, f(b) + GUARD) for b in batches] for f in sizes_of]
        ctx.set_direct(BIG if direct else 0)

        def fill():
            for a in (a for g in outs for a in g):
                a.view(np.uint8)[...] = 0xEE
            for a in (a for g in souts for a in g):
                a[...] = SENT

        def submit():
            o = [r.ctypes.data for r in recs]
            if compact:
                ctx.group_submit_c8(1, batches, o)
            else:
                ctx.group_submit_ex(1, batches, o)
            ctx.group_wait(1)
            assert ctx.slot_direct(1) == direct

        ptrs = [[a.ctypes.data for a in g] for g in outs]
        for with_plan in (True, False):
            fill()
            if steer:
                ctx.slot_steer_gather(1, *[[a.ctypes.data for a in g] for g in souts])
            ctx.slot_fwd(1, ptrs[1], ptrs[2], ptrs[3], ptrs[4], nrings=4, in_ifidx=IFS, plan=ptrs[0] if with_plan else None)
            submit()
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
                    assert np.array_equal(outs[0][i][:b.n], want.view(np.uint64))
                else:
                    assert (outs[0][i] == 0xEEEEEEEEEEEEEEEE).all()
                assert outs[4][i].tobytes() == exp[3].tobytes(), (i, outs[4][i], exp[3])
                for k, per in ((1, 1), (2, 1), (3, 12)):
                    got, e = outs[k][i], exp[k - 1]
                    if direct:                                  # in place: exact, untouched past the sent count
                        assert got.tobytes() == e.tobytes(), (k, i)
                    else:
                        assert np.array_equal(got[:m * per], e[:m * per]), (k, i)
                        assert (got[b.n * per:].view(np.uint8) == 0xEE).all(), (k, i)
                if steer:
                    eidx, eqs = expect(rec["queue"])
                    np.testing.assert_array_equal(souts[0][i][:4 * b.n].view(np.uint32), eidx)
                    np.testing.assert_array_equal(souts[1][i][:4 * QS].view(np.uint32), eqs)
                    np.testing.assert_array_equal(souts[3][i][:4 * b.n].view(np.uint32), o[eidx])
            assert sent_total > 300
        # one-shot: the next submit leaves everything untouched; so does a disarmed one
        for disarm in (False, True):
            fill()
            if disarm:
                ctx.slot_fwd(1, ptrs[1], ptrs[2], ptrs[3], ptrs[4], nrings=4)
                ctx.slot_fwd(1, None)
            submit()
            assert all((a.view(np.uint8) == 0xEE).all() for g in outs for a in g)
            assert all((a == SENT).all() for g in souts for a in g)
    finally:
        ctx.set_direct(0)
        ctx.set_params(mosrx.default_params())
        for p in frees:
            ctx.host_free(p)


def test_slot_fwd_refusals(gpu_ctx):
    ctx = gpu_ctx
    L, h = mosrx.lib(), gpu_ctx.handle
    t = trace()
    frees = []
    try:
        ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
        base, blk = ctx.host_alloc(t.frames_bytes + 8 * t.n + 256 * (NB + 1))
        frees.append(base)
        batches, parts = _stage(blk, base, t, NB)
        recs = [np.zeros(b.n, mosrx.RESULT_DTYPE) for b in batches]
        outs = [[ee(f(b.n), dt) for b in batches] for dt, f in
                ((np.uint32, lambda n: n), (np.uint16, lambda n: n), (np.uint8, lambda n: 12 * n),
                 (mosrx.FWD_RING_DTYPE, lambda n: 4))]
        ptrs = [[a.ctypes.data for a in g] for g in outs]
        one = (C.c_void_p * NB)(*ptrs[0])

        def arm(**kw):
            a = dict(tx_src=ptrs[0], tx_len=ptrs[1], tx_mac=ptrs[2], rings=ptrs[3], nrings=4)
            a.update(kw)
            with pytest.raises(mosrx.MosrxError) as e:
                ctx.slot_fwd(1, **a)
            return e.value.errno

        ctx.fwd_set(None)
        assert arm() == ENOENT
        ctx.fwd_set(mosrx.fwd_tables(**WALK))
        assert arm(nrings=3) == EINVAL and arm(nrings=0) == EINVAL and arm(nrings=17) == EINVAL
        assert arm(tx_len=None) == EINVAL and arm(tx_mac=None) == EINVAL and arm(rings=None) == EINVAL
        assert L.mosrx_slot_fwd(h, 2, None) == -EINVAL and L.mosrx_slot_fwd(h, 0, None) == 0
        o = [r.ctypes.data for r in recs]

        def refused_submit(errno, **kw):
            a = dict(tx_src=ptrs[0], tx_len=ptrs[1], tx_mac=ptrs[2], rings=ptrs[3], nrings=4)
            a.update(kw)
            ctx.slot_fwd(1, **a)
            for r in recs:
                r.view(np.uint8)[...] = 0xEE
            with pytest.raises(mosrx.MosrxError) as e:
                ctx.group_submit_ex(1, batches, o)
            assert e.value.errno == errno
            mosrx._chk(L.mosrx_sync(h), "sync")
            assert all((r.view(np.uint8) == 0xEE).all() for r in recs)                       # nothing was submitted
            assert all((a.view(np.uint8) == 0xEE).all() for g in outs for a in g)

        refused_submit(EINVAL, tx_src=[None] + ptrs[0][1:])
        refused_submit(EINVAL, tx_mac=[ptrs[2][0] + 2] + ptrs[2][1:])
        refused_submit(EINVAL, rings=[ptrs[3][0], None, ptrs[3][2]])
        refused_submit(EINVAL, in_ifidx=[0, 16, 0])
        # the tables in effect at the submit count: cleared after the arm
        ctx.slot_fwd(1, ptrs[0], ptrs[1], ptrs[2], ptrs[3], nrings=4)
        ctx.fwd_set(None)
        with pytest.raises(mosrx.MosrxError) as e:
            ctx.group_submit_ex(1, batches, o)
        assert e.value.errno == ENOENT
        ctx.fwd_set(mosrx.fwd_tables(**WALK))
        # busy slot: the arm is refused, the running submit is not disturbed
        ctx.group_submit_ex(1, batches, o)
        assert L.mosrx_slot_fwd(h, 1, None) == -EBUSY
        ctx.group_wait(1)
        rec0 = O.classify(np.asarray(parts[0][0][:parts[0][3]]), np.asarray(parts[0][1]), np.asarray(parts[0][2]),
                          O.params(num_msp=1, forward=1))
        assert recs[0].tobytes() == rec0.tobytes()
        assert all((a.view(np.uint8) == 0xEE).all() for g in outs for a in g)
    finally:
        ctx.set_params(mosrx.default_params())
        for p in frees:
            ctx.host_free(p)
