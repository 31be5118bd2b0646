"""NAT attached to a batch queue (mosrx_queue_set_nat): 5 batches, one of them
empty, with byte rings and with descriptor rings.  Every batch's plan, xlat
records and TX outputs equal what the single-batch calls give for that batch
alone, which is the restatement's answer (tests/nat_oracle.py) laid over copies
of the same 0xEE images.  The records are the queue's own classify output, equal
to the oracle's.  Expected values never come from the GPU."""
import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_rings_oracle as FR
import mosrx
import nat_cases as NC
import nat_oracle as N
from test_fwd_desc_gpu import DescOutputs
from test_fwd_desc_gpu import assert_same as desc_same
from test_fwd_desc_gpu import download as desc_download
from test_fwd_gpu import ee
from test_fwd_queue_gpu import Setup, split
from test_fwd_rings_gpu import assert_same as rings_same

pytestmark = pytest.mark.gpu

EINVAL, ENOENT = 22, 2
NS = [257, 0, 63, 513, 100]
NR = 4
PHASES = (2, 7, 0, 13, 1, 11)


class Xlat:
    """Per-batch xlat images on the device (two canary records behind each)."""

    def __init__(self, ctx, ns):
        self.ns = ns
        self.init = [ee(n + 2, mosrx.NAT_XLAT_DTYPE) for n in ns]
        self.dev = [mosrx.DevBuffer(ctx, a.nbytes) for a in self.init]
        self.fill()

    def fill(self):
        for d, a in zip(self.dev, self.init):
            d.upload(a)

    def ptrs(self):
        return [d.ptr for d in self.dev]

    def check(self, want):
        for i, (d, a, w) in enumerate(zip(self.dev, self.init, want)):
            e = a.copy()
            e[:self.ns[i]] = w
            assert d.download(np.zeros_like(a)).tobytes() == e.tobytes(), ("xlat of batch", i)

    def untouched(self):
        for d, a in zip(self.dev, self.init):
            assert d.download(np.zeros_like(a)).tobytes() == a.tobytes()

    def free(self):
        for d in self.dev:
            d.free()


def make(ctx):
    s = Setup(ctx, split(NC.mix(sum(NS)), NS, PHASES))
    t = mosrx.fwd_tables(**NC.TABLES)
    ctx.fwd_set(t)
    return s, t


def answers(s, t, bindings):
    """Per batch (xlat, plan, translated frames)."""
    return [N.plan(b, o, l, r["reason"], bindings, t, 0) for (b, o, l), r in zip(s.batches, s.rec)]


def check_plans(out, want):
    for i, w in enumerate(want):
        got = out.plan(i)
        bad = np.nonzero(got.view(np.uint64) != w[1].view(np.uint64))[0]
        assert not len(bad), (i, [(int(k), got[k].tolist(), w[1][k].tolist()) for k in bad[:6]])


def check_rings(s, out, t, want):
    check_plans(out, want)
    for i, ((b, o, l), (x, pl, tr)) in enumerate(zip(s.batches, want)):
        rings_same(out.tx(i), FR.build(tr, o, pl, t, out.cap, out.nrings, *out.init[i]), ("batch", i))


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_queue_of_5_with_byte_rings(gpu_ctx, rec_bytes):
    ctx = gpu_ctx
    s, t = make(ctx)
    xl = None
    try:
        b1 = NC.bindings()
        ctx.nat_set(b1)
        want = answers(s, t, b1)
        assert sum(int(np.isin(w[0]["kind"], [N.SNAT, N.DNAT]).sum()) for w in want) > 600
        cap = max(int(FR.need_units(w[1], NR).max()) for w in want) * 16
        q, out, xl = s.queue(rec_bytes), s.outputs(cap, NR), Xlat(ctx, NS)
        out.attach(q)
        q.set_nat(xl.ptrs())
        # under mosrx_set_fwd_one the multi-launch path is taken all the same
        ctx.set_fwd_one(1024)
        before = ctx.fwd_one_count()
        q.run()
        assert ctx.fwd_one_count() == before
        check_rings(s, out, t, want)
        xl.check([w[0] for w in want])
        # a table replaced between two runs: half of the flows are gone
        b2 = b1[::2].copy()
        ctx.nat_set(b2)
        want2 = answers(s, t, b2)
        assert sum(int((w[0]["kind"] == N.MISS).sum()) for w in want2) > 300
        out.fill()
        xl.fill()
        q.run()
        check_rings(s, out, t, want2)
        xl.check([w[0] for w in want2])
        # a ring too small for the fullest batch: dropped entries are not patched
        small = s.outputs(cap // 2 // 16 * 16, NR)
        small.attach(q)
        q.run()
        check_rings(s, small, t, want2)
        # detached: the queue forwards the received frames as before
        q.set_nat(None)
        out.attach(q)
        out.fill()
        xl.fill()
        q.run()
        s.check(out, t, s.want_plans(t))
        xl.untouched()
    finally:
        ctx.set_fwd_one(0)
        s.close()
        if xl:
            xl.free()


def test_queue_of_5_with_descriptor_rings(gpu_ctx):
    ctx = gpu_ctx
    s, t = make(ctx)
    out = xl = None
    try:
        b1 = NC.bindings()
        ctx.nat_set(b1)
        want = answers(s, t, b1)
        q, out, xl = s.queue(), DescOutputs(ctx, NS, NR), Xlat(ctx, NS)
        out.attach(q)
        q.set_nat(xl.ptrs())
        ctx.set_fwd_one(1024)
        before = ctx.fwd_one_count()
        q.run()
        assert ctx.fwd_one_count() == before
        check_plans(out, want)
        for i, ((b, o, l), (x, pl, tr)) in enumerate(zip(s.batches, want)):
            desc_same(desc_download(out.dev[i], out.init[i]), FD.build(tr, o, pl, t, NR, *out.init[i]), ("batch", i))
        xl.check([w[0] for w in want])
    finally:
        ctx.set_fwd_one(0)
        s.close()
        for o in (out, xl):
            if o:
                o.free()


def test_refusals(gpu_ctx):
    ctx, L = gpu_ctx, mosrx.lib()
    s, t = make(ctx)
    xl = hit = None
    try:
        ctx.nat_set(NC.bindings())
        q, xl = s.queue(), Xlat(ctx, NS)
        with pytest.raises(mosrx.MosrxError) as e:                   # no forwarding attached
            q.set_nat(xl.ptrs())
        assert e.value.errno == EINVAL
        out = s.outputs()                                            # a plan-only attachment will do
        out.attach(q)
        with pytest.raises(mosrx.MosrxError) as e:                   # a misaligned array
            q.set_nat([p + 8 for p in xl.ptrs()])
        assert e.value.errno == EINVAL
        hit = [mosrx.DevBuffer(ctx, 2 * n + 16) for n in NS]
        ctx.acl_set([("DROP", "10.21.0.0/12", "0.0.0.0")])
        q.set_acl([h.ptr for h in hit])
        with pytest.raises(mosrx.MosrxError) as e:                   # firewall rules attached
            q.set_nat(xl.ptrs())
        assert e.value.errno == EINVAL
        q.set_acl(None)
        q.set_nat(xl.ptrs())
        q.set_acl([h.ptr for h in hit])                              # ... attached afterwards: the run refuses
        with pytest.raises(mosrx.MosrxError) as e:
            q.run()
        assert e.value.errno == EINVAL
        q.set_acl(None)
        ctx.set_params(mosrx.default_params(num_msp=1, forward=1, skip_tcp_csum=1))
        with pytest.raises(mosrx.MosrxError) as e:                   # skip_tcp_csum: no exact incremental check
            q.run()
        assert e.value.errno == EINVAL
        ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        out.untouched()
        xl.untouched()
        q.run()                                                      # and with everything in order it runs
        check_plans(out, answers(s, t, NC.bindings()))
    finally:
        ctx.acl_set(None)
        ctx.set_params(mosrx.default_params())
        s.close()
        for o in [xl] + (hit or []):
            if o:
                o.free()
