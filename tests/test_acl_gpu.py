"""The firewall launch on the GPU (mosrx_acl_apply_dev, mosrx_queue_set_acl)
against its restatement (tests/acl_oracle.py) and the sample's own answers
(tests/golden/acl_firewall.npz).

hit, counts and the plan are 0xEE images with canary entries behind them; the
restatement's answers are laid over copies of the same images and the
comparison is exact.  Expected values never come from the GPU: the records the
restatement reads are the oracle's (or hand-made), the plan it amends is
fwd_oracle's, and the downstream builds are compared with fwd_desc_oracle /
fwd_rings_oracle fed that amended plan."""
import ctypes as C
import os

import numpy as np
import pytest

import acl_oracle as A
import acl_pin as P
import fwd_desc_oracle as FD
import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from pktlib import R, tcp_frame
from test_fwd_desc_gpu import DescOutputs, images as desc_images
from test_fwd_desc_gpu import assert_same as desc_same
from test_fwd_desc_gpu import download
from test_fwd_gpu import Run, ee, pack_at
from test_fwd_queue_gpu import Setup
from test_fwd_rings_gpu import RingRun
from test_fwd_rings_gpu import assert_same as rings_same

pytestmark = pytest.mark.gpu

T = 256
EINVAL, ENOENT = 22, 2
PARAMS = dict(num_msp=1, forward=1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acl_firewall.npz")
DEVS2 = ["02:00:00:00:aa:00", "02:00:00:00:aa:01"]
# 10/8 goes out of netdev 1 behind an ARP entry, 9.9.9.9's destinations too; the rest has no route
TABLES = dict(routes=[("10.0.0.0/8", 1)], arp=[("10.0.0.0/8", "02:00:00:00:00:01")], netdevs=DEVS2)
PHASES = [2, 7, 0, 13, 1, 11]     # frames at odd offsets, every offset mod 4

SRC = ["10.37.1.1", "10.5.2.2", "10.22.1.1", "10.8.1.5", "10.8.1.6", "9.9.9.9", "10.8.1.77"]
DST = ["10.7.0.9", "10.7.3.3", "10.9.13.1", "10.9.69.7", "10.10.10.10", "10.9.64.1"]
SPORT = [40000, 4000, 5000, 1111]
DPORT = [80, 443, 25, 22, 23]


def frame(i):
    """Frame i of the mix: SYNs over the rule files' addresses and ports (plain, behind IP options of
    ihl 6 and 15, with a bad TCP checksum), SYN-ACKs, data segments, UDP."""
    s, d = SRC[i % len(SRC)], DST[(i // 2) % len(DST)]
    sp, dp = SPORT[(i // 3) % len(SPORT)], DPORT[(i // 5) % len(DPORT)]
    k = i % 11
    if k == 3:
        return tcp_frame(s, d, sp, dp, flags=0x12, seq=i)                          # SYN-ACK
    if k == 5:
        return tcp_frame(s, d, sp, dp, b"udp" * (i % 7), proto=17)                 # not TCP
    if k == 6:
        return tcp_frame(s, d, sp, dp, flags=0x02, seq=i, tcp_csum=0x1)            # bad TCP checksum: not eligible
    if k == 7:
        return tcp_frame(s, d, sp, dp, flags=0x02, seq=i, ihl=6)
    if k == 8:
        return tcp_frame(s, d, sp, dp, flags=0x02, seq=i, ihl=15, doff=6)
    if k == 9:
        return tcp_frame(s, d, sp, dp, b"x" * (i % 40), flags=0x18, seq=i)
    return tcp_frame(s, d, sp, dp, flags=0x02, seq=i, pad_to=60 + i % 9)


_mix = {}


def mix(n):
    if "f" not in _mix:
        _mix["f"] = [frame(i) for i in range(2 * T + 1)]
    return _mix["f"][:n]


def never(i):
    """A rule no frame of the mix matches (rule i of the long tables)."""
    return ("DROP" if i % 2 else "ACCEPT", f"172.{16 + i // 250}.{i % 250}.1", "0.0.0.0", 0, 1 + i % 7)


RULES = {
    "one": [("DROP", "10.21.0.0/12", "0.0.0.0")],
    "five": A.parse_rules(P.MASKS_RULES),
    "last_of_1024": [never(i) for i in range(1023)] + [("DROP", "0.0.0.0", "0.0.0.0")],      # the loop's full length
    "first_of_1024": [("DROP", "0.0.0.0", "0.0.0.0")] + [never(i) for i in range(1023)],     # the early exit
}
_rules = {}


def rules_of(name):
    if name not in _rules:
        _rules[name] = mosrx.acl_rules(RULES[name])
    return _rules[name]


def rec8_of(rec):
    r8 = np.zeros(len(rec), mosrx.RESULT8_DTYPE)
    for k in ("rss", "reason", "queue", "verdict", "tcp_flags"):
        r8[k] = rec[k]
    return r8


class AclRun(RingRun):
    """A batch on the GPU with its hit / counts images; the records are the GPU's own classify
    output (Run) unless given."""

    def __init__(self, ctx, buf, off, ln, rec_bytes=16, frames_bytes=None, rec=None):
        Run.__init__(self, ctx, buf, off, ln, rec_bytes, frames_bytes)
        if rec is not None and self.n:
            self.d_rec.upload(rec if rec_bytes == 16 else rec8_of(rec))
        self.hit_init, self.cnt_init = ee(self.n + 8, np.uint16), ee(mosrx.ACL_MAX_RULES + 8, np.uint32)
        self.cnt_init[:mosrx.ACL_MAX_RULES] = 0                      # the caller zeroes the counts
        self.d_hit, self.d_cnt = mosrx.DevBuffer(ctx, self.hit_init.nbytes), mosrx.DevBuffer(ctx, self.cnt_init.nbytes)
        self.d_hit.upload(self.hit_init)
        self.d_cnt.upload(self.cnt_init)
        self.bufs += [self.d_hit, self.d_cnt]

    def apply(self, plan=True, counts=True):
        self.ctx.acl_apply_dev(self.db.batch(), self.d_rec.ptr, self.rb, self.d_plan.ptr if plan else None,
                               self.d_hit.ptr, self.d_cnt.ptr if counts else None)

    def hit(self):
        return self.d_hit.download(np.zeros_like(self.hit_init))

    def counts(self):
        return self.d_cnt.download(np.zeros_like(self.cnt_init))

    def build_desc(self, nrings):
        n, ctx = self.n, self.ctx
        init = desc_images(n, nrings)
        dev = [mosrx.DevBuffer(ctx, a.nbytes) for a in init]
        for d, a in zip(dev, init):
            d.upload(a)
        sb = mosrx.lib().mosrx_fwd_desc_scratch_bytes(n, nrings)
        scr = mosrx.DevBuffer(ctx, sb)
        self.bufs += dev + [scr]
        ctx.fwd_desc_rings_dev(self.db.batch(), self.d_plan.ptr, nrings, dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr,
                               scr.ptr, sb)
        return dev, init


def setup(ctx, rules, forward=1, listener=False, tables=TABLES):
    ctx.set_params(mosrx.default_params(num_msp=1, forward=forward))
    ctx.fwd_set_listener(listener)
    t = mosrx.fwd_tables(**tables)
    ctx.fwd_set(t)
    ctx.acl_set(rules)
    return t


def expect_images(r, hit, cnt):
    eh, ec = r.hit_init.copy(), r.cnt_init.copy()
    eh[:r.n] = hit
    ec[:mosrx.ACL_MAX_RULES] = cnt
    return eh, ec


def check(ctx, buf, off, ln, rules, rec_bytes=16, forward=1, listener=False, frames_bytes=None, rec=None, launches=1,
          downstream=False, tables=TABLES, nrings=2):
    """Plan + firewall launch on the GPU equal the restatement: hit, counts (after `launches`
    launches into the same array) and the amended plan, canaries included; returns (hit, plan)."""
    t = setup(ctx, rules, forward, listener, tables)
    orec = O.classify(buf, off, ln, O.params(num_msp=1, forward=forward)) if rec is None else rec
    base = F.plan(buf, off, ln, orec["reason"], t, 0, forward=forward, num_msp=1, listener=listener,
                  frames_bytes=frames_bytes)
    hit, cnt, want = A.apply(buf, off, ln, orec, rules, base, listener=listener, forward=forward,
                             frames_bytes=frames_bytes)
    r = AclRun(ctx, buf, off, ln, rec_bytes, frames_bytes, rec)
    try:
        for k in range(launches):
            r.plan(0)
            got = r.plan_result()
            assert got.tobytes() == base.tobytes(), "the plan launch itself"
            r.apply()
        eh, ec = expect_images(r, hit, cnt * np.uint32(launches))
        np.testing.assert_array_equal(r.hit(), eh)
        np.testing.assert_array_equal(r.counts(), ec)
        got = r.plan_result()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]]
        if downstream:
            # the builds omit exactly the dropped SYNs: the restatements fed the amended plan
            dev, init = r.build_desc(nrings)
            desc_same(download(dev, init), FD.build(buf, off, want, t, nrings, *init), "descriptor rings")
            cap = max(int(FR.need_units(want, nrings).max()) * 16, 16)
            dev, init = r.build_rings(cap, nrings)
            rings_same(download(dev, init), FR.build(buf, off, want, t, cap, nrings, *init), "byte rings")
            sent = FR.sent_mask(want, nrings)
            assert not sent[A.dropped(hit, rules)].any() and \
                sent.sum() == FR.sent_mask(base, nrings).sum() - A.dropped(hit, rules).sum()
        return hit, want
    finally:
        r.free()


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("name", sorted(RULES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2 * T + 1])
def test_sizes_and_tables(gpu_ctx, n, name, rec_bytes):
    buf, off, ln = pack_at(mix(n), PHASES)
    rules = rules_of(name)
    hit, pl = check(gpu_ctx, buf, off, ln, rules, rec_bytes, downstream=n in (65, 2 * T + 1))
    if n >= 63:
        looked = hit != A.NOT_LOOKED_UP
        assert 0 < looked.sum() < n
        if name == "last_of_1024":
            assert (hit[looked] == 1023).all() and (pl["kind"][looked] == mosrx.FWD_DROP).all()
        if name == "first_of_1024":
            assert (hit[looked] == 0).all()
        if name == "five" and n >= 257:
            assert {0, 1, 2, 4, A.NO_MATCH} <= set(hit[looked].tolist()) and 3 not in hit     # rule 4 is shadowed


def test_counts_accumulate_over_two_launches(gpu_ctx):
    """... over the whole mix, which holds every kind of frame the launch must tell apart."""
    buf, off, ln = pack_at(mix(2 * T + 1), PHASES)
    rec = O.classify(buf, off, ln, O.params(**PARAMS))
    syn = (rec["tcp_flags"] & 0x12) == 0x02
    assert (rec["reason"][syn] == R["TCP_BADCSUM"]).sum() > 20 and (rec["reason"] == R["NOT_TCP"]).sum() > 20
    assert ((rec["tcp_flags"] & 0x12) == 0x12).sum() > 20
    ihl = buf[off.astype(np.int64) + 14] & 0xF
    assert (ihl[syn] == 6).sum() > 20 and (ihl[syn] == 15).sum() > 20 and {int(o) % 4 for o in off} == {0, 1, 2, 3}
    hit, pl = check(gpu_ctx, buf, off, ln, rules_of("five"), launches=2)
    assert (hit[syn & (rec["reason"] == R["TCP_BADCSUM"])] == A.NOT_LOOKED_UP).all()


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_listener_and_forward_off(gpu_ctx, rec_bytes):
    buf, off, ln = pack_at(mix(300), PHASES)
    try:
        hit, pl = check(gpu_ctx, buf, off, ln, rules_of("five"), rec_bytes, listener=True)
        assert (hit == A.NOT_LOOKED_UP).all() and not (pl["kind"] == mosrx.FWD_DROP).any()
        # forward = 0: looked up and counted all the same, the plan stays NONE
        hit, pl = check(gpu_ctx, buf, off, ln, rules_of("five"), rec_bytes, forward=0)
        assert (hit < 5).sum() > 20 and not pl["kind"].any()
    finally:
        gpu_ctx.fwd_set_listener(False)
        gpu_ctx.set_params(mosrx.default_params())


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_ports_past_the_buffer_end(gpu_ctx, rec_bytes):
    """Hand-made records: the last frame says ihl 15 with a 40-byte packet, and the buffer ends two bytes
    behind that packet -- its ports' dword lies past the end and reads zero, so only rules with both ports
    wild match it; a frame cut inside its packet is not looked up at all."""
    fr = mix(70) + [tcp_frame("10.37.1.1", "10.7.0.9", 40000, 80, flags=0x02, ihl=15)] * 2
    buf, off, ln = pack_at(fr, PHASES)
    for i in (70, 71):
        o = int(off[i])
        buf[o + 16:o + 18] = (0, 40)                                  # tot_len 40 (the checksums are the records' business)
    fb = int(off[71]) + 14 + 40 + 2
    assert fb % 16 and int(off[71]) + 74 >= (fb + 15) // 16 * 16
    rec = O.classify(buf, off, ln, O.params(**PARAMS))
    rec["reason"][70:], rec["tcp_flags"][70:] = R["TCP_OK"], 0x02
    rules = mosrx.acl_rules([("ACCEPT", "10.21.0.0/12", "10.7.0.0/16", 0, 80), ("DROP", "10.21.0.0/12", "10.7.0.0/16")])
    hit, pl = check(gpu_ctx, buf, off, ln, rules, rec_bytes, frames_bytes=fb, rec=rec)
    assert hit[70] == 0 and hit[71] == 1 and pl["kind"][71] == mosrx.FWD_DROP       # frame 70's ports are in the buffer
    hit, pl = check(gpu_ctx, buf, off, ln, rules, rec_bytes, frames_bytes=fb - 3, rec=rec)
    assert hit[70] == 0 and hit[71] == A.NOT_LOOKED_UP


def test_fixture_from_the_sample(gpu_ctx):
    """The "masks" scenario as the sample itself counted and forwarded it."""
    z, k = np.load(GOLDEN), "masks__"
    buf, off, ln, rules = z[k + "frames"], z[k + "off"], z[k + "len"], z[k + "rules"]
    t = setup(gpu_ctx, rules, tables=dict(routes=[("0.0.0.0/0", 0)], arp=[("0.0.0.0/0", "02:00:00:00:00:aa")],
                                          netdevs=["00:00:00:00:00:00"], nic_fwd={0: 0}))
    assert bytes(t) == bytes(P.tables())
    for rb in (16, 8):
        r = AclRun(gpu_ctx, buf, off, ln, rb)
        try:
            r.plan(0)
            r.apply()
            eh, ec = expect_images(r, z[k + "hit"], np.concatenate([z[k + "counts"], np.zeros(1024 - len(rules), np.uint32)]))
            np.testing.assert_array_equal(r.hit(), eh)
            np.testing.assert_array_equal(r.counts(), ec)
            got = r.plan_result()
            assert got.tobytes() == z[k + "plan"].tobytes()
            np.testing.assert_array_equal(np.nonzero(np.isin(got["kind"], [F.IP, F.ETH]))[0], z[k + "tx_src"])
        finally:
            r.free()


def test_refusals_launch_nothing(gpu_ctx):
    ctx, L = gpu_ctx, mosrx.lib()
    buf, off, ln = pack_at(mix(100), PHASES)
    setup(ctx, rules_of("five"))
    r = AclRun(ctx, buf, off, ln)
    try:
        b = r.db.batch()

        def call(**kw):
            return L.mosrx_acl_apply_dev(ctx.handle, C.byref(kw.get("b", b)), kw.get("rec", r.d_rec.ptr), kw.get("rb", 16),
                                         kw.get("plan", r.d_plan.ptr), kw.get("hit", r.d_hit.ptr),
                                         kw.get("cnt", r.d_cnt.ptr), None)
        ctx.acl_set(None)
        assert ctx.acl_count() == 0 and call() == -ENOENT                       # cleared
        empty = mosrx.Batch(b.frames, b.frames_bytes, b.off, b.len, 0, 0)
        assert call(b=empty) == -ENOENT
        ctx.acl_set(rules_of("five"))
        assert ctx.acl_count() == 5 and call(b=empty) == 0                      # n == 0: nothing to launch
        for kw in (dict(rec=None), dict(rec=r.d_rec.ptr + 8), dict(rb=4), dict(rb=0), dict(plan=r.d_plan.ptr + 4),
                   dict(hit=None), dict(hit=r.d_hit.ptr + 1), dict(cnt=r.d_cnt.ptr + 2)):
            assert call(**kw) == -EINVAL, kw
        bad = np.zeros(2, mosrx.ACL_RULE_DTYPE)
        assert L.mosrx_acl_set(ctx.handle, bad.ctypes.data, 2) == -EINVAL       # action 0
        assert L.mosrx_acl_set(ctx.handle, bad.ctypes.data, 1025) == -EINVAL and ctx.acl_count() == 5
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        np.testing.assert_array_equal(r.hit(), r.hit_init)                      # nothing ran
        np.testing.assert_array_equal(r.counts(), r.cnt_init)
        # plan and counts are optional; the pool rotates: more sets than it has copies
        for _ in range(6):
            ctx.acl_set(rules_of("one"))
            ctx.acl_set(rules_of("five"))
        r.apply(plan=False, counts=False)
        rec = O.classify(buf, off, ln, O.params(**PARAMS))
        np.testing.assert_array_equal(r.hit()[:r.n], A.apply(buf, off, ln, rec, rules_of("five"))[0])
        np.testing.assert_array_equal(r.counts(), r.cnt_init)
        assert r.plan_result().view(np.uint64).tolist() == [0xEEEEEEEEEEEEEEEE] * r.n
    finally:
        L.mosrx_sync(ctx.handle)
        r.free()


def test_timing_op(gpu_ctx):
    ctx = gpu_ctx
    setup(ctx, rules_of("five"))
    buf, off, ln = pack_at(mix(300), PHASES)
    db = ctx.upload(buf, off, ln)
    hit = mosrx.DevBuffer(ctx, 2 * 300)
    try:
        ctx.classify_dev(db)
        bs = (mosrx.Batch * 1)(db.batch())
        outs, aux = (C.c_void_p * 1)(db.d_out.ptr), (C.c_void_p * 1)(hit.ptr)
        tot, avg = C.c_float(), C.c_float()
        L = mosrx.lib()
        assert L.mosrx_time_op(ctx.handle, mosrx.OP_ACL, 16, bs, 1, outs, aux, 4, 1, C.byref(tot), C.byref(avg)) == 0
        assert tot.value > 0 and avg.value > 0
        rec = O.classify(buf, off, ln, O.params(**PARAMS))
        np.testing.assert_array_equal(hit.download(np.zeros(300, np.uint16)), A.apply(buf, off, ln, rec, rules_of("five"))[0])
        assert L.mosrx_time_op(ctx.handle, mosrx.OP_ACL, 12, bs, 1, outs, aux, 4, 1, C.byref(tot), None) == -EINVAL
        assert L.mosrx_time_op_dispatch(ctx.handle, mosrx.OP_ACL, 16, bs, 1, outs, aux, 2, C.byref(avg)) == -95   # ENOTSUP
    finally:
        hit.free()
        db.free()


# ---- the queue form -------------------------------------------------------------

def split(frames, ns):
    out, pos = [], 0
    for n in ns:
        out.append(pack_at(frames[pos:pos + n], PHASES))
        pos += n
    return out


class QueueAcl:
    """Per-batch hit images and the queue's counts image on the device."""

    def __init__(self, ctx, ns):
        self.ctx, self.ns = ctx, ns
        self.hit_init = [ee(n + 8, np.uint16) for n in ns]
        self.cnt_init = ee(mosrx.ACL_MAX_RULES + 8, np.uint32)
        self.cnt_init[:mosrx.ACL_MAX_RULES] = 0
        self.d_hit = [mosrx.DevBuffer(ctx, a.nbytes) for a in self.hit_init]
        self.d_cnt = mosrx.DevBuffer(ctx, self.cnt_init.nbytes)
        self.fill()

    def fill(self):
        for d, a in zip(self.d_hit, self.hit_init):
            d.upload(a)
        self.d_cnt.upload(self.cnt_init)

    def check(self, hits, cnt):
        for i, (d, a, h) in enumerate(zip(self.d_hit, self.hit_init, hits)):
            e = a.copy()
            e[:self.ns[i]] = h
            np.testing.assert_array_equal(d.download(np.zeros_like(a)), e, err_msg=f"hit of batch {i}")
        e = self.cnt_init.copy()
        e[:mosrx.ACL_MAX_RULES] = cnt
        np.testing.assert_array_equal(self.d_cnt.download(np.zeros_like(e)), e)

    def untouched(self):
        for d, a in zip(self.d_hit, self.hit_init):
            np.testing.assert_array_equal(d.download(np.zeros_like(a)), a)
        np.testing.assert_array_equal(self.d_cnt.download(np.zeros_like(self.cnt_init)), self.cnt_init)

    def free(self):
        for d in self.d_hit + [self.d_cnt]:
            d.free()


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_queue_of_5_with_descriptor_rings(gpu_ctx, rec_bytes):
    """set_fwd_desc + set_acl over 5 batches, one empty: batch by batch what the single-batch calls give
    (the restatements), and with the one-launch limit set the outputs are the same and that form is not taken."""
    ctx = gpu_ctx
    ns = [T + 1, 0, 63, 2 * T + 1, 100]
    s = Setup(ctx, split([frame(i) for i in range(sum(ns))], ns))
    out = acl = None
    try:
        rules = rules_of("five")
        t = setup(ctx, rules)
        base = s.want_plans(t)
        res = [A.apply(b, o, l, r, rules, p) for (b, o, l), r, p in zip(s.batches, s.rec, base)]
        want = [x[2] for x in res]
        cnt = sum(x[1].astype(np.uint64) for x in res).astype(np.uint32)
        assert sum(int((w["kind"] == mosrx.FWD_DROP).sum()) for w in want) > 20
        q, out, acl = s.queue(rec_bytes), DescOutputs(ctx, ns, 2), QueueAcl(ctx, ns)
        out.attach(q)
        q.set_acl([d.ptr for d in acl.d_hit], acl.d_cnt.ptr)
        q.run()
        out.check(s, t, want)
        acl.check([x[0] for x in res], cnt)
        # under mosrx_set_fwd_one the multi-launch path is taken all the same
        ctx.set_fwd_one(1024)
        before = ctx.fwd_one_count()
        out.fill()
        acl.fill()
        q.run()
        assert ctx.fwd_one_count() == before
        out.check(s, t, want)
        acl.check([x[0] for x in res], cnt)
        # no rules installed: the run is refused before it enqueues anything
        ctx.acl_set(None)
        out.fill()
        acl.fill()
        with pytest.raises(mosrx.MosrxError) as e:
            q.run()
        assert e.value.errno == ENOENT
        mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
        out.untouched()
        acl.untouched()
        # detached: the queue forwards as it did before, dropped SYNs included
        ctx.acl_set(rules)
        q.set_acl(None)
        q.run()
        out.check(s, t, base)
        acl.untouched()
    finally:
        ctx.set_fwd_one(0)
        s.close()
        for o in (out, acl):
            if o:
                o.free()


def test_queue_without_forwarding(gpu_ctx):
    """No forwarding attached: the launch runs behind the classify launch, with no plan."""
    ctx = gpu_ctx
    ns = [0, 300, T]
    s = Setup(ctx, split([frame(i) for i in range(sum(ns))], ns))
    acl = None
    try:
        rules = rules_of("last_of_1024")
        setup(ctx, rules)
        res = [A.apply(b, o, l, r, rules) for (b, o, l), r in zip(s.batches, s.rec)]
        q, acl = s.queue(), QueueAcl(ctx, ns)
        q.set_acl([d.ptr for d in acl.d_hit], None)                   # no counts either
        q.run()
        for i, (d, a) in enumerate(zip(acl.d_hit, acl.hit_init)):
            e = a.copy()
            e[:ns[i]] = res[i][0]
            np.testing.assert_array_equal(d.download(np.zeros_like(a)), e)
        np.testing.assert_array_equal(acl.d_cnt.download(np.zeros_like(acl.cnt_init)), acl.cnt_init)
        for d, r in zip(s.dbs, s.rec):
            assert d.results().tobytes() == r.tobytes()
        with pytest.raises(mosrx.MosrxError) as e:
            q.set_acl([d.ptr + 1 for d in acl.d_hit], None)
        assert e.value.errno == EINVAL
    finally:
        s.close()
        if acl:
            acl.free()
