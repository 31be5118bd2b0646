"""The descriptor form of the ring build on the GPU (mosrx_fwd_desc_rings_dev,
mosrx_queue_set_fwd_desc) against its restatement (tests/fwd_desc_oracle.py).

Every output is a 0xEE image with canary entries behind it; the restatement
writes into copies of the same images and the comparison is exact, so entries
at and past the sent count and d_rings[nrings ..] are part of it.  The plan given
to the single-batch build is the GPU's own mosrx_fwd_plan_dev output, asserted
equal to the restatement's plan first (or a hand-made plan, for records the plan
kernel never writes).  Expected values never come from the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_fwd_gpu import DEVS4, DSTS, PAD, WALK, Run, base_frames, ee, eth_frame, ip_frame, pack_at
from test_fwd_queue_gpu import PARAMS, Setup, split
from test_fwd_rings_gpu import SPREADS
from test_oracle_golden import GOLDEN
from test_steer_gpu import QS, Guarded, expect

pytestmark = pytest.mark.gpu

T = 256                # mosrx_fwd_tile(), checked in test_tile
NAMES = ("tx_src", "tx_len", "tx_mac", "rings")
EINVAL, ENOENT = 22, 2
HOLES = dict(routes=[("10.0.0.0/8", 1), ("192.168.0.0/16", 2)], arp=[("10.0.0.0/8", "02:00:00:00:00:01")], netdevs=DEVS4)


def images(n, nrings):
    return [ee(n + PAD, np.uint32), ee(n + PAD, np.uint16), ee(12 * (n + PAD), np.uint8),
            ee(nrings + 2, mosrx.FWD_RING_DTYPE)]


def download(dev, init):
    return [d.download(np.zeros_like(i0)) for d, i0 in zip(dev, init)]


def assert_same(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        g, e = g.view(np.uint8), e.view(np.uint8)
        diff = np.nonzero(g != e)[0]
        assert not len(diff), (name, what, len(diff), diff[:8].tolist(), g[diff[:8]].tolist(), e[diff[:8]].tolist())


class DescRun(Run):
    def build_desc(self, nrings, sync=True):
        n, ctx = self.n, self.ctx
        init = images(n, nrings)
        dev = [mosrx.DevBuffer(ctx, a.nbytes) for a in init]
        for d, a in zip(dev, init):
            d.upload(a)
        sb = mosrx.lib().mosrx_fwd_desc_scratch_bytes(n, nrings)
        scr = mosrx.DevBuffer(ctx, sb)
        self.bufs += dev + [scr]
        ctx.fwd_desc_rings_dev(self.db.batch(), self.d_plan.ptr, nrings, dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr,
                               scr.ptr, sb, sync=sync)
        return dev, init


def check(ctx, buf, off, ln, tables, nrings=None, in_ifidx=0, rec_bytes=16, mutate=None):
    """Plan + descriptor build on the GPU equal the restatement; returns (plan, expected rings).
    mutate(plan): a hand-made plan replaces the GPU's own before the build."""
    nrings = tables.num_netdevs if nrings is None else nrings
    ctx.set_params(mosrx.default_params(**PARAMS))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(tables)
    rec = O.classify(buf, off, ln, O.params(**PARAMS))
    want = F.plan(buf, off, ln, rec["reason"], tables, in_ifidx, forward=1, num_msp=1)
    r = DescRun(ctx, buf, off, ln, rec_bytes)
    try:
        r.plan(in_ifidx)
        got = r.plan_result()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]]
        if mutate is not None:
            want = mutate(want.copy())
            r.d_plan.upload(want.view(np.uint64))
        dev, init = r.build_desc(nrings)
        exp = FD.build(buf, off, want, tables, nrings, *init)
        assert_same(download(dev, init), exp, (len(off), nrings, in_ifidx, rec_bytes))
        return want, exp[3]
    finally:
        r.free()


def test_tile():
    assert mosrx.lib().mosrx_fwd_tile() == T


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("n", [1, T - 1, T, T + 1, 3 * T + 1])
def test_frame_counts(gpu_ctx, n, rec_bytes):
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 37) % 240, pad=(i % 5) * 3, ok=i % 3 != 1, seed=i) for i in range(n)]
    buf, off, ln = pack_at(fr, [2, 7, 0, 13])
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), rec_bytes=rec_bytes)
    assert rings["count"][:4].sum() == FR.sent_mask(want, 4).sum() > 0
    if n >= T - 1:
        assert (rings["count"][:4] > 0).all()


@pytest.mark.parametrize("name", ["one_netdev_of_4", "round_robin_16", "middle_gets_nothing", "runs_of_300"])
def test_spreads(gpu_ctx, name):
    make, n = SPREADS[name]
    fr, t, nrings = make(n)
    buf, off, ln = pack_at(fr, [2, 11])
    want, rings = check(gpu_ctx, buf, off, ln, t, nrings=nrings)
    c = rings["count"][:nrings]
    assert rings["units"][:nrings].tolist() == FR.need_units(want, nrings).tolist()
    if name == "one_netdev_of_4":
        assert c.tolist() == [0, n, 0, 0] and rings["start"][:4].tolist() == [0, 0, n, n]
    if name == "round_robin_16":
        assert c.min() >= n // 16 and c.sum() == n
    if name == "middle_gets_nothing":
        assert c[2] == 0 and c[0] > 0 and c[1] > 0 and c[3] > 0 and rings["start"][3] == rings["start"][2]
    if name == "runs_of_300":
        assert c.tolist() == [300] * 16


def mixed(n=600):
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 29) % 300, pad=i % 4, ok=i % 7 != 3, seed=i) for i in range(n)]
    for i in range(5, n, 11):
        fr[i] = eth_frame(14 + (i * 3) % 90, i)
    return fr


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_mixed_traffic(gpu_ctx, rec_bytes):
    buf, off, ln = pack_at(mixed(), [2, 9, 0, 7])
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    # in_ifidx 0: the nic_forward_table shortcut -- arp_idx 0xFFFF keeps the frame's own h_dest; ETH kinds are sent
    want, rings = check(gpu_ctx, buf, off, ln, t, in_ifidx=0, rec_bytes=rec_bytes)
    sent = FR.sent_mask(want, 4)
    assert (want["kind"] == F.ETH).sum() > 20 and (want["arp_idx"][sent & (want["kind"] == F.IP)] == 0xFFFF).all()
    assert rings["count"][:4].tolist() == [0, 0, int(sent.sum()), 0]
    # in_ifidx 1 has no entry: IP frames walk the tables, the others are NO_NIC
    want, rings = check(gpu_ctx, buf, off, ln, t, in_ifidx=1, rec_bytes=rec_bytes)
    assert (want["kind"] == F.NO_NIC).sum() > 20 and (rings["count"][:4] > 0).all()
    # tables with holes: NO_ROUTE and NO_ARP frames take no entry
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**HOLES), rec_bytes=rec_bytes)
    assert (want["kind"] == F.NO_ROUTE).sum() > 20 and (want["kind"] == F.NO_ARP).sum() > 20
    assert rings["count"][:4].tolist() == [0, int((want["kind"] == F.IP).sum()), 0, 0]


def test_hand_made_plan(gpu_ctx):
    """Records the plan kernel never writes: tx_len < 14 and out_ifidx >= nrings are not sent."""
    buf, off, ln = pack_at(mixed(700), [2, 9, 0, 7])

    def mutate(pl):
        s = np.nonzero(FR.sent_mask(pl, 4))[0]
        pl["tx_len"][s[::5]] = 13
        pl["tx_len"][s[1::15]] = 0
        pl["out_ifidx"][s[2::5]] = 4
        pl["out_ifidx"][s[3::15]] = 15
        pl["out_ifidx"][s[4::15]] = -1
        return pl
    clean, whole = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK))
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), mutate=mutate)
    assert 0 < rings["count"][:4].sum() < whole["count"][:4].sum() * 0.6


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_offsets_mod_4_and_exact_end(gpu_ctx, shift):
    """Frame starts at every offset mod 4; the last frame, 14 bytes at offset (shift + 3) mod 4, ends exactly at
    frames_bytes: the dword that holds its byte 11 may end past the frame."""
    fr = mixed(2 * T + 3) + [eth_frame(14, 99)]
    buf, off, ln = pack_at(fr, [(shift + k) % 4 + 4 * k for k in range(4)])
    buf = buf[:int(off[-1]) + int(ln[-1])].copy()
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3} and len(buf) == int(off[-1]) + 14
    assert int(off[-1]) % 4 == (shift + 3) % 4
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 1}))
    for rb in (16, 8):
        want, rings = check(gpu_ctx, buf, off, ln, t, rec_bytes=rb)
        assert want[-1]["kind"] == F.ETH and want[-1]["tx_len"] == 14
    check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), in_ifidx=0)


def test_more_rings_than_netdevs(gpu_ctx):
    buf, off, ln = pack_at(base_frames(600), [2, 5])
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), nrings=16)
    m = int(rings["count"][:4].sum())
    assert m > 0 and [r.tolist() for r in rings[4:16]] == [(m, 0, 0, 0)] * 12


@pytest.mark.parametrize("name", ["conv_walk", "edge_walk", "conv_nicfwd"])
@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_mos_fixture(gpu_ctx, name, rec_bytes):
    """Ring 0's entries laid over the received frames are the frames mOS itself sent (tests/golden/fwd_plan.npz)."""
    z = np.load(os.path.join(GOLDEN, "fwd_plan.npz"))
    k = name + "__"
    t = mosrx.FwdTables.from_buffer_copy(z[k + "tables"].tobytes())
    buf, off, ln = z[k + "frames"], z[k + "off"], z[k + "len"]
    ctx = gpu_ctx
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1, local=["127.0.0.1"]))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(t)
    r = DescRun(ctx, buf, off, ln, rec_bytes)
    try:
        r.plan()
        pl = z[k + "plan"].view(mosrx.FWD_DTYPE).reshape(-1)
        np.testing.assert_array_equal(r.plan_result().view(np.uint64), pl.view(np.uint64))
        nrings = max(t.num_netdevs, 1)
        dev, init = r.build_desc(nrings)
        got = download(dev, init)
        assert_same(got, FD.build(buf, off, pl, t, nrings, *init), name)
        tsrc, tlen, tmac, rings = got
        m = len(z[k + "tx_off"])
        assert rings[0].tolist()[:3] == (0, m, 0)
        assert FD.ring_list(buf, off, tsrc, tlen, tmac, rings, 0) == F.tx_list(z[k + "tx"], z[k + "tx_off"], z[k + "tx_len"], m)
        np.testing.assert_array_equal(tsrc[:m], z[k + "tx_src"])
    finally:
        r.free()


def test_empty_batch_zeroes_the_rings(gpu_ctx):
    ctx = gpu_ctx
    buf, off, ln = pack_at(base_frames(10), [2])
    ctx.set_params(mosrx.default_params(**PARAMS))
    ctx.fwd_set(mosrx.fwd_tables(**WALK))
    r = DescRun(ctx, buf, off[:0], ln[:0])
    try:
        dev, init = r.build_desc(4)
        exp = [a.copy() for a in init]
        exp[3][:4] = (0, 0, 0, 0)
        assert_same(download(dev, init), exp, "n == 0")
    finally:
        r.free()


def test_errors_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    buf, off, ln = pack_at(base_frames(100), [2])
    ctx.set_params(mosrx.default_params(**PARAMS))
    r = DescRun(ctx, buf, off, ln)
    L, b = mosrx.lib(), r.db.batch()
    try:
        n = r.n
        init = images(n, 4)
        bufs = [mosrx.DevBuffer(ctx, a.nbytes) for a in init] + [mosrx.DevBuffer(ctx, 256)]
        r.bufs += bufs
        for d, a in zip(bufs, init):
            d.upload(a)
        tsrc, tlen, tmac, rings, scr = (x.ptr for x in bufs)

        def build(**kw):
            return L.mosrx_fwd_desc_rings_dev(ctx.handle, C.byref(b), kw.get("plan", r.d_plan.ptr), kw.get("nrings", 4),
                                              kw.get("tsrc", tsrc), kw.get("tlen", tlen), kw.get("tmac", tmac),
                                              kw.get("rings", rings), kw.get("scr", scr), kw.get("sb", 256), None)
        ctx.fwd_set(None)
        assert build() == -ENOENT                                     # no tables
        ctx.fwd_set(mosrx.fwd_tables(**WALK))
        assert L.mosrx_fwd_desc_scratch_bytes(n, 4) == 64
        for kw in (dict(plan=None), dict(plan=r.d_plan.ptr + 4), dict(tsrc=None), dict(tsrc=tsrc + 2), dict(tlen=None),
                   dict(tlen=tlen + 1), dict(tmac=None), dict(tmac=tmac + 2), dict(rings=None), dict(rings=rings + 8),
                   dict(scr=None), dict(scr=scr + 8), dict(sb=63), dict(nrings=0), dict(nrings=17), dict(nrings=3)):
            assert build(**kw) == -EINVAL, kw
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        for d, a in zip(bufs, init):                                  # nothing ran
            assert np.array_equal(d.download(np.zeros_like(a)).view(np.uint8), a.view(np.uint8))
    finally:
        L.mosrx_sync(ctx.handle)
        r.free()


def test_timing_op(gpu_ctx):
    ctx = gpu_ctx
    ctx.set_params(mosrx.default_params(**PARAMS))
    ctx.fwd_set(mosrx.fwd_tables(**WALK))
    dbs = []
    try:
        for n in (300, 1000):
            buf, off, ln = pack_at(base_frames(n), [2, 7])
            db = ctx.upload(buf, off, ln)
            ctx.classify_dev(db)
            dbs.append(db)
        tot, avg = ctx.time_op(mosrx.OP_FWD_DESC, dbs, 4, arg=16)
        assert tot > 0 and avg > 0
        bs = (mosrx.Batch * 2)(*[d.batch() for d in dbs])
        outs = (C.c_void_p * 2)(*[d.d_out.ptr for d in dbs])
        aux = (C.c_void_p * 2)(*[d.d_fplan.ptr for d in dbs])
        ms = C.c_float()
        assert mosrx.lib().mosrx_time_op_dispatch(ctx.handle, mosrx.OP_FWD_DESC, 16, bs, 2, outs, aux, 2,
                                                  C.byref(ms)) == -95    # ENOTSUP
    finally:
        for d in dbs:
            d.free()


# ---- the queue form -------------------------------------------------------------

class DescOutputs:
    """Per-batch plan arrays (one canary entry behind each) and descriptor images on the device."""

    def __init__(self, ctx, ns, nrings):
        self.ctx, self.ns, self.nrings = ctx, ns, nrings
        self.plan_init = [ee(n + 1, np.uint64) for n in ns]
        self.d_plan = [mosrx.DevBuffer(ctx, a.nbytes) for a in self.plan_init]
        self.init = [images(n, nrings) for n in ns]
        self.dev = [[mosrx.DevBuffer(ctx, a.nbytes) for a in im] for im in self.init]
        self.fill()

    def fill(self):
        for d, a in zip(self.d_plan, self.plan_init):
            d.upload(a)
        for ds, im in zip(self.dev, self.init):
            for d, a in zip(ds, im):
                d.upload(a)

    def kwargs(self, in_ifidx=None):
        kw = dict(plan=[d.ptr for d in self.d_plan], in_ifidx=in_ifidx, nrings=self.nrings)
        for k, name in enumerate(NAMES):
            kw[name] = [ds[k].ptr for ds in self.dev]
        return kw

    def attach(self, q, in_ifidx=None, **over):
        kw = self.kwargs(in_ifidx)
        kw.update(over)
        q.set_fwd_desc(**kw)

    def plan(self, i):
        raw = self.d_plan[i].download(np.zeros(self.ns[i] + 1, np.uint64))
        assert raw[self.ns[i]] == 0xEEEEEEEEEEEEEEEE
        return raw[:self.ns[i]].view(mosrx.FWD_DTYPE)

    def untouched(self):
        for i in range(len(self.ns)):
            assert (self.d_plan[i].download(np.zeros_like(self.plan_init[i])) == self.plan_init[i]).all(), ("plan", i)
            assert_same(download(self.dev[i], self.init[i]), self.init[i], ("untouched", i))

    def check(self, s, tables, want, what=""):
        rings = []
        for i, ((b, o, l), w) in enumerate(zip(s.batches, want)):
            got = self.plan(i)
            bad = np.nonzero(got.view(np.uint64) != w.view(np.uint64))[0]
            assert not len(bad), (what, i, [(int(k), got[k].tolist(), w[k].tolist()) for k in bad[:6]])
            exp = FD.build(b, o, w, tables, self.nrings, *self.init[i])
            assert_same(download(self.dev[i], self.init[i]), exp, (what, "batch", i))
            rings.append(exp[3])
            if not len(o):   # an empty batch: zeroed rings, nothing else
                assert exp[3][:self.nrings].view(np.uint32).sum() == 0
                assert all((e.view(np.uint8) == 0xEE).all() for e in exp[:3])
        return rings

    def free(self):
        for d in self.d_plan + [d for ds in self.dev for d in ds]:
            d.free()


def run_queue(ctx, batches, tables, nrings, in_ifidx=None, rec_bytes=16):
    s = Setup(ctx, batches)
    out = None
    try:
        ctx.fwd_set(tables)
        want = s.want_plans(tables, in_ifidx)
        q = s.queue(rec_bytes)
        out = DescOutputs(ctx, s.ns, nrings)
        out.attach(q, in_ifidx)
        q.run()
        return want, out.check(s, tables, want)
    finally:
        s.close()
        if out:
            out.free()


SIZES = {"empty_first": [0, 1, T - 1, T, T + 1, 0, 3 * T + 1], "empty_second": [1, 0, T - 1, T, T + 1, 3 * T + 1, 0],
         "empty_last": [T + 1, T, 0, 0, 1, T - 1, 0]}


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("order", sorted(SIZES))
def test_queue_batch_sizes(gpu_ctx, order, rec_bytes):
    ns = SIZES[order]
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 37) % 240, pad=(i % 5) * 3, ok=i % 3 != 1, seed=i) for i in range(sum(ns))]
    want, rings = run_queue(gpu_ctx, split(fr, ns), mosrx.fwd_tables(**WALK), 4, rec_bytes=rec_bytes)
    assert [int(r["count"][:4].sum()) for r in rings] == [int(FR.sent_mask(w, 4).sum()) for w in want]
    assert sum(int(r["count"][:4].sum()) > 0 for r in rings) >= 4


def test_queue_per_batch_in_ifidx(gpu_ctx):
    ns, ifs = [300, 257, 303, 100], [0, 1, 0, 1]
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    for rb in (16, 8):
        want, rings = run_queue(gpu_ctx, split(mixed(960), ns, (2, 9)), t, 4, in_ifidx=ifs, rec_bytes=rb)
        for w, r, i in zip(want, rings, ifs):
            if i == 0:
                assert r["count"][:4].tolist() == [0, 0, int(FR.sent_mask(w, 4).sum()), 0] and (w["kind"] == F.ETH).any()
            else:
                assert (w["kind"] == F.NO_NIC).any() and not (w["kind"] == F.ETH).any() and (r["count"][:4] > 0).all()


def test_queue_16_rings(gpu_ctx):
    make, _ = SPREADS["runs_of_300"]
    ns = [1500, 2100, 1200]
    fr, t, nrings = make(sum(ns))
    want, rings = run_queue(gpu_ctx, split(fr, ns, (2, 11)), t, nrings)
    assert sum(int(r["count"][:16].sum()) for r in rings) == sum(ns)


def test_queue_with_steering(gpu_ctx):
    ns = [300, 0, 257]
    s = Setup(gpu_ctx, split(base_frames(sum(ns)), ns), params=dict(PARAMS, num_queues=8))
    groups, out = [], None
    try:
        t = mosrx.fwd_tables(**WALK)
        gpu_ctx.fwd_set(t)
        want = s.want_plans(t)
        q, out = s.queue(), DescOutputs(gpu_ctx, ns, 4)
        groups = [[Guarded(gpu_ctx, f(n)) for n in ns] for f in
                  (lambda n: 4 * n, lambda n: 4 * QS, lambda n: 16 * n, lambda n: 4 * n, lambda n: 2 * n)]
        q.set_steer_gather(*[[g.ptr for g in gs] for gs in groups])
        out.attach(q)
        q.run()
        out.check(s, t, want)
        for i, ((b, o, l), n) in enumerate(zip(s.batches, ns)):
            if n == 0:
                continue
            rec = s.dbs[i].results()
            assert rec.tobytes() == s.rec[i].tobytes()
            eidx, eqs = expect(s.rec[i]["queue"])
            np.testing.assert_array_equal(groups[0][i].read(), eidx)
            np.testing.assert_array_equal(groups[1][i].read(), eqs)
            np.testing.assert_array_equal(groups[3][i].read(np.uint32), o[eidx])
    finally:
        s.close()
        if out:
            out.free()
        for g in (g for gs in groups for g in gs):
            g.free()
        gpu_ctx.set_params(mosrx.default_params())


def test_queue_detach_refusals_and_exclusion(gpu_ctx):
    ctx = gpu_ctx
    ns = [300, 0, 257]
    s = Setup(ctx, split(base_frames(sum(ns)), ns))
    out = other = None
    try:
        t = mosrx.fwd_tables(**WALK)
        ctx.fwd_set(t)
        want = s.want_plans(t)
        q, out, other = s.queue(), DescOutputs(ctx, ns, 4), DescOutputs(ctx, ns, 4)
        out.attach(q)
        good = other.kwargs()

        def bumped(name, by, i=0):
            return {name: [p + by if k == i else p for k, p in enumerate(good[name])]}

        def nulled(name, i=0):
            return {name: [None if k == i else p for k, p in enumerate(good[name])]}

        bad = [nulled("plan"), bumped("plan", 4), nulled("tx_src"), bumped("tx_src", 2), nulled("tx_len"),
               bumped("tx_len", 1), nulled("tx_mac"), bumped("tx_mac", 2), nulled("rings"), bumped("rings", 8),
               nulled("rings", 1), dict(in_ifidx=[0, 16, 0]), dict(tx_src=None), dict(tx_mac=None), dict(rings=None),
               dict(nrings=0), dict(nrings=17)]
        for kw in bad:                       # each refused attach leaves the previous attachment in place
            with pytest.raises(mosrx.MosrxError) as e:
                other.attach(q, **kw)
            assert e.value.errno == EINVAL, kw
        # mutual exclusion with the byte-ring attachment, both ways
        with pytest.raises(mosrx.MosrxError) as e:
            q.set_fwd(plan=good["plan"])
        assert e.value.errno == EINVAL
        q.run()
        out.check(s, t, want)
        other.untouched()

        def refused(errno):
            out.fill()
            for d in s.dbs:
                d.d_out.upload(ee(max(d.n, 1) * 16, np.uint8))
            with pytest.raises(mosrx.MosrxError) as e:
                q.run()
            assert e.value.errno == errno
            mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
            out.untouched()
            for d in s.dbs:     # not even the classify launch
                assert (d.d_out.download(np.zeros(max(d.n, 1) * 16, np.uint8)) == 0xEE).all()

        ctx.fwd_set(None)
        refused(ENOENT)
        ctx.fwd_set(t)
        out.attach(q, nrings=3)
        refused(EINVAL)                      # 4 netdevs installed, 3 rings attached
        out.attach(q)
        # detach: the queue runs exactly as before, and needs no tables
        q.set_fwd_desc(None)
        out.fill()
        ctx.fwd_set(None)
        q.run()
        out.untouched()
        for d, r in zip(s.dbs, s.rec):
            assert d.results().tobytes() == r.tobytes()
        # now the byte-ring attachment may take the queue, and then refuses this one
        ctx.fwd_set(t)
        q.set_fwd(plan=good["plan"])
        with pytest.raises(mosrx.MosrxError) as e:
            out.attach(q)
        assert e.value.errno == EINVAL
        q.set_fwd_desc(None)                 # (not attached: nothing changes)
        q.run()
        assert np.array_equal(other.plan(0).view(np.uint64), want[0].view(np.uint64))
        q.set_fwd(None)
        out.attach(q)
        q.run()
        out.check(s, t, want)
    finally:
        s.close()
        for o in (out, other):
            if o:
                o.free()
