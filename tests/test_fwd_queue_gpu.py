"""Forwarding over a whole batch queue (mosrx_queue_set_fwd): every batch's
plan, ring block, entry arrays and rings row against the restatements applied to
that batch alone (fwd_oracle.plan on oracle_py.classify's reasons, then
fwd_rings_oracle.build).

As in test_fwd_rings_gpu.py every buffer is a 0xEE image with canary entries
behind it, the restatement writes into copies of the same images, and the
comparison is exact: padding, ring tails, dropped frames' entries, entries past
the last ring, d_rings[nrings ..] and everything of an empty batch but its
zeroed rings are part of it.  Expected values never come from the GPU."""
import os

import numpy as np
import pytest

import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_fwd_gpu import DEVS4, DSTS, PAD, WALK, base_frames, ee, eth_frame, ip_frame, pack_at
from test_fwd_rings_gpu import NAMES, RingRun, assert_same, download, round_robin_16, runs_of_300
from test_oracle_golden import GOLDEN
from test_steer_gpu import QS, SENT, Guarded, expect

pytestmark = pytest.mark.gpu

EINVAL, ENOENT = 22, 2
PARAMS = dict(num_msp=1, forward=1)
SWAPPED = dict(WALK, routes=[("10.0.0.0/8", 3), ("192.168.0.0/16", 0), ("0.0.0.0/0", 2)],
               netdevs=[f"02:00:00:00:cc:{i:02x}" for i in range(4)])


def images(n, nrings, cap):
    """The 0xEE images of one batch's TX outputs, in the order of NAMES."""
    return [ee(nrings * cap + 64, np.uint8), ee(n + PAD, np.uint32), ee(n + PAD, np.uint16), ee(n + PAD, np.uint32),
            ee(nrings + 2, mosrx.FWD_RING_DTYPE)]


class Outputs:
    """One set of per-batch forwarding outputs on the device: a plan array per
    batch (one canary entry behind it) and, with a ring_cap, the TX images."""

    def __init__(self, ctx, ns, ring_cap=None, nrings=0):
        self.ctx, self.ns, self.cap, self.nrings = ctx, ns, ring_cap, nrings
        self.plan_init = [ee(n + 1, np.uint64) for n in ns]
        self.d_plan = [mosrx.DevBuffer(ctx, a.nbytes) for a in self.plan_init]
        self.init = [images(n, nrings, ring_cap) for n in ns] if ring_cap is not None else []
        self.dev = [[mosrx.DevBuffer(ctx, a.nbytes) for a in im] for im in self.init]
        self.fill()

    def fill(self):
        for d, a in zip(self.d_plan, self.plan_init):
            d.upload(a)
        for ds, im in zip(self.dev, self.init):
            for d, a in zip(ds, im):
                d.upload(a)

    def attach(self, q, in_ifidx=None, **over):
        kw = dict(plan=[d.ptr for d in self.d_plan], in_ifidx=in_ifidx)
        if self.cap is not None:
            kw.update(ring_cap=self.cap, nrings=self.nrings)
            for k, name in enumerate(("tx_frames", "tx_off", "tx_len", "tx_src", "rings")):
                kw[name] = [ds[k].ptr for ds in self.dev]
        kw.update(over)
        q.set_fwd(**kw)

    def plan(self, i):
        raw = self.d_plan[i].download(np.zeros(self.ns[i] + 1, np.uint64))
        assert raw[self.ns[i]] == 0xEEEEEEEEEEEEEEEE
        return raw[:self.ns[i]].view(mosrx.FWD_DTYPE)

    def tx(self, i):
        return download(self.dev[i], self.init[i])

    def untouched(self):
        for i in range(len(self.ns)):
            assert (self.d_plan[i].download(np.zeros_like(self.plan_init[i])) == self.plan_init[i]).all(), ("plan", i)
            if self.init:
                assert_same(self.tx(i), self.init[i], ("untouched", i))

    def free(self):
        for d in self.d_plan + [d for ds in self.dev for d in ds]:
            d.free()


class Setup:
    """Batches (buf, off, len) uploaded once, the oracle's records of each, and
    queues / outputs made over them; everything freed by close()."""

    def __init__(self, ctx, batches, params=PARAMS, local=()):
        self.ctx, self.batches, self.ns = ctx, batches, [len(b[1]) for b in batches]
        ctx.set_params(mosrx.default_params(**params, local=list(local) or None))
        ctx.fwd_set_listener(False)
        self.rec = [O.classify(b, o, l, O.params(**params, local=local)) for b, o, l in batches]
        self.dbs = [ctx.upload(b, o, l) for b, o, l in batches]
        self.queues, self.outs = [], []

    def queue(self, rec_bytes=16):
        self.queues.append(self.ctx.queue_ex(self.dbs, compact=rec_bytes == 8))
        return self.queues[-1]

    def outputs(self, ring_cap=None, nrings=0):
        self.outs.append(Outputs(self.ctx, self.ns, ring_cap, nrings))
        return self.outs[-1]

    def want_plans(self, tables, in_ifidx=None):
        return [F.plan(b, o, l, r["reason"], tables, in_ifidx[i] if in_ifidx else 0, forward=1, num_msp=1)
                for i, ((b, o, l), r) in enumerate(zip(self.batches, self.rec))]

    def check(self, out, tables, want, what=""):
        """Every output of every batch equals the restatement; returns the expected rings per batch."""
        rings = []
        for i, ((b, o, l), w) in enumerate(zip(self.batches, want)):
            got = out.plan(i)
            bad = np.nonzero(got.view(np.uint64) != w.view(np.uint64))[0]
            assert not len(bad), (what, i, [(int(k), got[k].tolist(), w[k].tolist()) for k in bad[:6]])
            if out.cap is None:
                continue
            exp = FR.build(b, o, w, tables, out.cap, out.nrings, *out.init[i])
            assert_same(out.tx(i), exp, (what, "batch", i, "cap", out.cap))
            rings.append(exp[4])
            if not len(o):   # an empty batch: zeroed rings, nothing else
                assert exp[4][:out.nrings].view(np.uint32).sum() == 0
                assert all((e.view(np.uint8) == 0xEE).all() for e in exp[:4])
        return rings

    def close(self):
        mosrx.lib().mosrx_sync(self.ctx.handle)
        for q in self.queues:
            q.destroy()
        for o in self.outs:
            o.free()
        for d in self.dbs:
            d.free()


def split(frames, ns, phases=(2, 7, 0, 13)):
    """Consecutive slices of `frames`, one packed batch per entry of ns."""
    lo, out = 0, []
    for n in ns:
        out.append(pack_at(frames[lo:lo + n], list(phases)))
        lo += n
    return out


def top_cap(want, nrings):
    """The fullest ring's need over all batches, in bytes."""
    return max(int(FR.need_units(w, nrings).max()) for w in want) * 16


def run_caps(ctx, batches, tables, nrings, in_ifidx=None, rec_bytes=16, caps=("exact", "minus16")):
    """Queue run per cap against the restatement; returns (wanted plans, expected rings at the first cap)."""
    s = Setup(ctx, batches)
    try:
        ctx.fwd_set(tables)
        want = s.want_plans(tables, in_ifidx)
        q = s.queue(rec_bytes)
        top, first = top_cap(want, nrings), None
        for name in caps:
            out = s.outputs(top if name == "exact" else max(top - 16, 0), nrings)
            out.attach(q, in_ifidx)
            q.run()
            rings = s.check(out, tables, want, name)
            first = rings if first is None else first
        return want, first
    finally:
        s.close()


SIZES = {"as_listed": [0, 1, 255, 256, 257, 700, 0, 513], "empty_second": [1, 0, 255, 256, 257, 700, 0, 513],
         "empty_last": [1, 255, 256, 257, 700, 0, 513, 0]}


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("order", sorted(SIZES))
def test_batch_sizes(gpu_ctx, order, rec_bytes):
    """Tile edges and empty batches first, second, in the middle and last; with
    the cap one unit short of the fullest ring some batches drop and others do not."""
    ns = SIZES[order]
    want, rings = run_caps(gpu_ctx, split(base_frames(sum(ns)), ns), mosrx.fwd_tables(**WALK), 4, rec_bytes=rec_bytes)
    assert [int(r["count"][:4].sum()) for r in rings] == [int(FR.sent_mask(w, 4).sum()) for w in want]
    assert sum(int(r["count"][:4].sum()) > 0 for r in rings) >= 5


def test_per_batch_in_ifidx(gpu_ctx):
    """nic_fwd = {0: 2}: batches with in_ifidx 0 take the shortcut (everything to
    netdev 2, no walk), those with in_ifidx 1 walk the tables and leave non-IPv4 frames NO_NIC."""
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 29) % 300, pad=i % 4, seed=i) for i in range(960)]
    for i in range(5, 960, 11):
        fr[i] = eth_frame(14 + (i * 3) % 90, i)
    ns, ifs = [300, 257, 303, 100], [0, 1, 0, 1]
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    for rb in (16, 8):
        want, rings = run_caps(gpu_ctx, split(fr, ns, (2, 9)), t, 4, in_ifidx=ifs, rec_bytes=rb)
        for w, r, n, i in zip(want, rings, ns, ifs):
            if i == 0:
                assert r["count"][:4].tolist() == [0, 0, n, 0] and (w["kind"] == F.ETH).any()
            else:
                assert (w["kind"] == F.NO_NIC).any() and not (w["kind"] == F.ETH).any() and (r["count"][:4] > 0).all()


@pytest.mark.parametrize("name,ns", [("round_robin_16", [400, 257, 443]), ("runs_of_300", [1500, 2100, 1200])])
def test_16_rings(gpu_ctx, name, ns):
    fr, t, nrings = {"round_robin_16": round_robin_16, "runs_of_300": runs_of_300}[name](sum(ns))
    want, rings = run_caps(gpu_ctx, split(fr, ns, (2, 11)), t, nrings)
    assert sum(int(r["count"][:16].sum()) for r in rings) == sum(ns)
    assert all((r["count"][:16] > 0).sum() >= 4 for r in rings)


def test_16_rings_over_4_netdevs(gpu_ctx):
    ns = [300, 0, 300]
    want, rings = run_caps(gpu_ctx, split(base_frames(600), ns, (2, 5)), mosrx.fwd_tables(**WALK), 16)
    for r in (rings[0], rings[2]):
        m = int(r["count"][:4].sum())
        assert m > 0 and [x.tolist() for x in r[4:16]] == [(m, 0, 0, 0)] * 12


def test_plan_only(gpu_ctx):
    """TX arrays NULL: the plans are written, a set of TX images that is not attached stays as it was."""
    ns = [257, 0, 64]
    s = Setup(gpu_ctx, split(base_frames(sum(ns)), ns))
    try:
        t = mosrx.fwd_tables(**WALK)
        gpu_ctx.fwd_set(t)
        q, out, spare = s.queue(), s.outputs(), s.outputs(4096, 4)
        out.attach(q)
        q.run()
        s.check(out, t, s.want_plans(t))
        spare.untouched()
    finally:
        s.close()


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_queue_of_one(gpu_ctx, rec_bytes):
    """One batch in a queue: the restatement's outputs, which are the single form's, byte for byte."""
    buf, off, ln = pack_at(base_frames(700), [2, 7, 0, 13])
    t = mosrx.fwd_tables(**WALK)
    want, rings = run_caps(gpu_ctx, [(buf, off, ln)], t, 4, rec_bytes=rec_bytes)
    cap = top_cap(want, 4)
    r = RingRun(gpu_ctx, buf, off, ln, rec_bytes)
    try:
        r.plan(0)
        assert np.array_equal(r.plan_result().view(np.uint64), want[0].view(np.uint64))
        dev, init = r.build_rings(cap, 4)
        assert_same(download(dev, init), FR.build(buf, off, want[0], t, cap, 4, *init), "single form")
    finally:
        r.free()


def test_steer_and_fwd_on_one_queue(gpu_ctx):
    ns = [300, 0, 257]
    params = dict(PARAMS, num_queues=8)
    s = Setup(gpu_ctx, split(base_frames(sum(ns)), ns), params=params)
    groups = []
    try:
        t = mosrx.fwd_tables(**WALK)
        gpu_ctx.fwd_set(t)
        want = s.want_plans(t)
        q, out = s.queue(), s.outputs(top_cap(want, 4), 4)
        groups = [[Guarded(gpu_ctx, f(n)) for n in ns] for f in
                  (lambda n: 4 * n, lambda n: 4 * QS, lambda n: 16 * n, lambda n: 4 * n, lambda n: 2 * n)]
        q.set_steer_gather(*[[g.ptr for g in gs] for gs in groups])
        out.attach(q)
        q.run()
        s.check(out, t, want)
        assert sum(int(FR.sent_mask(w, 4).sum()) for w in want) > 100 and len(np.unique(s.rec[0]["queue"])) > 1
        for i, ((b, o, l), n) in enumerate(zip(s.batches, ns)):
            if n == 0:
                assert all((gs[i].read(np.uint8) == SENT).all() for gs in groups)
                continue
            rec = s.dbs[i].results()
            assert rec.tobytes() == s.rec[i].tobytes()
            eidx, eqs = expect(s.rec[i]["queue"])
            np.testing.assert_array_equal(groups[0][i].read(), eidx)
            np.testing.assert_array_equal(groups[1][i].read(), eqs)
            np.testing.assert_array_equal(groups[2][i].read(np.uint8).reshape(n, 16), rec.view(np.uint8).reshape(n, 16)[eidx])
            np.testing.assert_array_equal(groups[3][i].read(np.uint32), o[eidx])
            np.testing.assert_array_equal(groups[4][i].read(np.uint16), l[eidx])
    finally:
        s.close()
        for g in (g for gs in groups for g in gs):
            g.free()
        gpu_ctx.set_params(mosrx.default_params())


def test_detach(gpu_ctx):
    ns = [300, 0, 257]
    s = Setup(gpu_ctx, split(base_frames(sum(ns)), ns))
    try:
        t = mosrx.fwd_tables(**WALK)
        gpu_ctx.fwd_set(t)
        want = s.want_plans(t)
        q, out = s.queue(), s.outputs(top_cap(want, 4), 4)
        out.attach(q)
        q.run()
        s.check(out, t, want)
        q.set_fwd(None)
        out.fill()
        for d in s.dbs:
            d.d_out.upload(ee(max(d.n, 1) * 16, np.uint8))
        gpu_ctx.fwd_set(None)          # a detached queue needs no tables either
        q.run()
        out.untouched()
        for d, r in zip(s.dbs, s.rec):
            assert d.results().tobytes() == r.tobytes()
    finally:
        s.close()


def test_tables_at_run_time(gpu_ctx):
    """Two runs on one stream with a mosrx_fwd_set between them, no sync: each keeps
    the tables it was enqueued under.  Then the run-time refusals, which enqueue nothing."""
    ctx = gpu_ctx
    ns = [300, 257]
    fr = [ip_frame(DSTS[i % len(DSTS)], 40 + i % 50, seed=i) for i in range(sum(ns))]
    s = Setup(ctx, split(fr, ns, (2,)))
    try:
        t1, t2 = mosrx.fwd_tables(**WALK), mosrx.fwd_tables(**SWAPPED)
        w1, w2 = s.want_plans(t1), s.want_plans(t2)
        assert not np.array_equal(w1[0].view(np.uint64), w2[0].view(np.uint64))
        q1, q2 = s.queue(), s.queue()
        o1, o2 = s.outputs(top_cap(w1, 4), 4), s.outputs(top_cap(w2, 4), 4)
        o1.attach(q1)
        o2.attach(q2)
        ctx.fwd_set(t1)
        q1.run(sync=False)
        ctx.fwd_set(t2)
        q2.run(sync=False)
        mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
        s.check(o1, t1, w1, "first tables")
        s.check(o2, t2, w2, "second tables")

        def refused(q, out, errno):
            out.fill()
            for d in s.dbs:
                d.d_out.upload(ee(d.n * 16, np.uint8))
            with pytest.raises(mosrx.MosrxError) as e:
                q.run()
            assert e.value.errno == errno
            mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
            out.untouched()
            for d in s.dbs:     # not even the classify launch
                assert (d.d_out.download(np.zeros(d.n * 16, np.uint8)) == 0xEE).all()

        ctx.fwd_set(None)
        refused(q1, o1, ENOENT)
        ctx.fwd_set(t1)
        o3 = s.outputs(top_cap(w1, 4), 3)
        o3.attach(q1)
        refused(q1, o3, EINVAL)         # 4 netdevs installed, 3 rings attached
    finally:
        s.close()


def test_attach_validation(gpu_ctx):
    """Each refused attach leaves the previous attachment in place."""
    ns = [300, 0, 257]
    s = Setup(gpu_ctx, split(base_frames(sum(ns)), ns))
    try:
        t = mosrx.fwd_tables(**WALK)
        gpu_ctx.fwd_set(t)
        want = s.want_plans(t)
        cap = top_cap(want, 4)
        q, out, other = s.queue(), s.outputs(cap, 4), s.outputs(cap, 4)
        out.attach(q)
        good = dict(plan=[d.ptr for d in other.d_plan])
        for k, name in enumerate(("tx_frames", "tx_off", "tx_len", "tx_src", "rings")):
            good[name] = [ds[k].ptr for ds in other.dev]

        def bumped(name, by, i=0):
            return {name: [p + by if k == i else p for k, p in enumerate(good[name])]}

        def nulled(name, i=0):
            return {name: [None if k == i else p for k, p in enumerate(good[name])]}

        bad = [nulled("plan"), bumped("plan", 4), nulled("tx_frames"), bumped("tx_frames", 8), nulled("tx_off"),
               bumped("tx_off", 2), nulled("tx_len"), bumped("tx_len", 1), nulled("tx_src"), bumped("tx_src", 2),
               nulled("rings"), bumped("rings", 8), nulled("rings", 1),       # rings of the empty batch, too
               dict(in_ifidx=[0, 16, 0]), dict(in_ifidx=[255, 0, 0]),
               dict(tx_frames=None), dict(rings=None), dict(tx_off=None, tx_len=None, tx_src=None, rings=None),
               dict(nrings=0), dict(nrings=17), dict(ring_cap=cap + 8), dict(ring_cap=(1 << 30) + 16),
               dict(ring_cap=1 << 33)]
        for kw in bad:
            with pytest.raises(mosrx.MosrxError) as e:
                other.attach(q, **kw)
            assert e.value.errno == EINVAL, kw
        # an empty batch's plan and entry arrays may be NULL
        other.attach(q, **nulled("plan", 1), **nulled("tx_off", 1))
        out.attach(q)
        for kw in bad[:3]:
            with pytest.raises(mosrx.MosrxError):
                other.attach(q, **kw)
        q.run()
        s.check(out, t, want)
        other.untouched()
    finally:
        s.close()


def test_mos_fixture(gpu_ctx):
    """golden/fwd_plan.npz's traces as the batches of one queue per table set: the
    plans are mOS's, and ring 0 of each batch holds the frames mOS itself sent."""
    z = np.load(os.path.join(GOLDEN, "fwd_plan.npz"))
    by_tables = {}
    for name in ("conv_walk", "edge_walk", "conv_nicfwd"):
        by_tables.setdefault(z[name + "__tables"].tobytes(), []).append(name + "__")
    assert sum(len(v) for v in by_tables.values()) == 3
    for raw, keys in by_tables.items():
        t = mosrx.FwdTables.from_buffer_copy(raw)
        nrings = max(t.num_netdevs, 1)
        s = Setup(gpu_ctx, [(z[k + "frames"], z[k + "off"], z[k + "len"]) for k in keys], local=["127.0.0.1"])
        try:
            gpu_ctx.fwd_set(t)
            cap = max((len(z[k + "tx"]) + 15) // 16 * 16 for k in keys)
            for rb in (16, 8):
                q, out = s.queue(rb), s.outputs(cap, nrings)
                out.attach(q)
                q.run()
                s.check(out, t, [z[k + "plan"].view(mosrx.FWD_DTYPE).reshape(-1) for k in keys], "mOS's plans")
                for i, k in enumerate(keys):
                    tx, toff, tlen, tsrc, rings = out.tx(i)
                    m = len(z[k + "tx_off"])
                    assert rings[0].tolist()[:3] == (0, m, 0)
                    assert FR.ring_list(tx, toff, tlen, rings, 0) == F.tx_list(z[k + "tx"], z[k + "tx_off"], z[k + "tx_len"], m)
                    np.testing.assert_array_equal(tsrc[:m], z[k + "tx_src"])
        finally:
            s.close()


def test_queue_time(gpu_ctx):
    ns = [300, 1000]
    s = Setup(gpu_ctx, split(base_frames(sum(ns)), ns))
    try:
        t = mosrx.fwd_tables(**WALK)
        gpu_ctx.fwd_set(t)
        q, out = s.queue(), s.outputs(top_cap(s.want_plans(t), 4), 4)
        out.attach(q)
        tot, avg = q.time(4)
        assert tot > 0 and avg > 0
    finally:
        s.close()
