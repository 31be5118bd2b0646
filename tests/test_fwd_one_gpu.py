"""The one-launch forwarding form on the GPU (mosrx_set_fwd_one): the plan and
the descriptor rings of a batch by one workgroup, against the same restatements
the four launches are held to (tests/fwd_oracle.py `plan`, tests/fwd_desc_oracle.py
`build`) -- the contract is "the same outputs as the four launches".

Every output is a 0xEE image with canary entries behind it and the comparison is
exact, so entries at and past the sent count, rings[nrings ..] and -- in this
form -- the whole scratch buffer are part of it.  Which form ran is read from
mosrx_fwd_one_count.  Expected values never come from the GPU."""
import ctypes as C

import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_fwd_desc_gpu import HOLES, DescOutputs, DescRun, assert_same, download, images, mixed
from test_fwd_gpu import DEVS4, DSTS, WALK, base_frames, ee, eth_frame, ip_frame, pack_at
from test_fwd_queue_gpu import PARAMS, Setup, split
from test_fwd_rings_gpu import SPREADS

pytestmark = pytest.mark.gpu

T = 256
MAX = mosrx.FWD_ONE_MAX
EINVAL, ENOENT = 22, 2


@pytest.fixture
def ctx(gpu_ctx):
    """The session's context, its limit back at 0 afterwards."""
    gpu_ctx.set_fwd_one(0)
    yield gpu_ctx
    gpu_ctx.set_fwd_one(0)


class OneRun(DescRun):
    """DescRun whose scratch is a 0xEE image too: the one launch leaves it untouched."""

    def build_desc(self, nrings, sync=True):
        n, ctx = self.n, self.ctx
        init = images(n, nrings)
        dev = [mosrx.DevBuffer(ctx, a.nbytes) for a in init]
        for d, a in zip(dev, init):
            d.upload(a)
        sb = mosrx.lib().mosrx_fwd_desc_scratch_bytes(n, nrings)
        self.scr_init = ee(sb, np.uint8)
        self.scr = mosrx.DevBuffer(ctx, sb)
        self.scr.upload(self.scr_init)
        self.bufs += dev + [self.scr]
        ctx.fwd_desc_rings_dev(self.db.batch(), self.d_plan.ptr, nrings, dev[0].ptr, dev[1].ptr, dev[2].ptr, dev[3].ptr,
                               self.scr.ptr, sb, sync=sync)
        return dev, init

    def scratch_untouched(self):
        return bool((self.scr.download(np.zeros_like(self.scr_init)) == 0xEE).all())


def check(ctx, buf, off, ln, tables, nrings=None, in_ifidx=0, rec_bytes=16, mutate=None, limit=MAX, one=True,
          frames_bytes=None):
    """mosrx_fwd_plan_dev (as it was), then mosrx_fwd_desc_rings_dev under `limit`: the outputs equal the
    restatement, and the form that ran is the one expected.  Returns (plan, expected rings)."""
    fb = len(buf) if frames_bytes is None else frames_bytes
    nrings = tables.num_netdevs if nrings is None else nrings
    ctx.set_params(mosrx.default_params(**PARAMS))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(tables)
    rec = O.classify(buf[:fb], off, ln, O.params(**PARAMS))
    want = F.plan(buf, off, ln, rec["reason"], tables, in_ifidx, forward=1, num_msp=1, frames_bytes=fb)
    r = OneRun(ctx, buf, off, ln, rec_bytes, frames_bytes=fb)
    try:
        ctx.set_fwd_one(limit)
        c0 = ctx.fwd_one_count()
        r.plan(in_ifidx)
        assert ctx.fwd_one_count() == c0                    # mosrx_fwd_plan_dev is unchanged
        got = r.plan_result()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]]
        if mutate is not None:
            want = mutate(want.copy())
            r.d_plan.upload(want.view(np.uint64))
        dev, init = r.build_desc(nrings)
        assert ctx.fwd_one_count() == c0 + (1 if one else 0)
        exp = FD.build(buf, off, want, tables, nrings, *init)
        assert_same(download(dev, init), exp, (len(off), nrings, in_ifidx, rec_bytes, limit))
        assert r.scratch_untouched() == one
        assert r.plan_result().view(np.uint64).tobytes() == want.view(np.uint64).tobytes()   # PLAN = false: read only
        return want, exp[3]
    finally:
        ctx.set_fwd_one(0)
        r.free()


def varied(n):
    return [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 37) % 240, pad=(i % 5) * 3, ok=i % 3 != 1, seed=i) for i in range(n)]


def test_setting_round_trip(ctx):
    L = mosrx.lib()
    assert ctx.get_fwd_one() == 0                           # off at open (and after every test here)
    for v in (0, 1, 256, MAX):
        ctx.set_fwd_one(v)
        assert ctx.get_fwd_one() == v
    ctx.set_fwd_one(256)
    for bad in (MAX + 1, 0xFFFFFFFF):
        assert L.mosrx_set_fwd_one(ctx.handle, bad) == -EINVAL
        assert ctx.get_fwd_one() == 256                     # the old value is kept
    with pytest.raises(mosrx.MosrxError):
        ctx.set_fwd_one(MAX + 1)
    assert ctx.fwd_one_count() == mosrx.lib().mosrx_fwd_one_count(ctx.handle)


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, 32 * T])
def test_frame_counts(ctx, n, rec_bytes):
    buf, off, ln = pack_at(varied(max(n, 1)), [2, 7, 0, 13])
    want, rings = check(ctx, buf, off[:n], ln[:n], mosrx.fwd_tables(**WALK), rec_bytes=rec_bytes)
    assert rings["count"][:4].sum() == FR.sent_mask(want, 4).sum()
    assert (n == 0) == (rings["count"][:4].sum() == 0)
    if n == 0:
        assert [r.tolist() for r in rings[:4]] == [(0, 0, 0, 0)] * 4
    if n >= T - 1:
        assert (rings["count"][:4] > 0).all()


@pytest.mark.parametrize("name", ["one_netdev_of_4", "round_robin_16", "middle_gets_nothing", "runs_of_300"])
def test_spreads(ctx, name):
    make, n = SPREADS[name]
    fr, t, nrings = make(n)
    buf, off, ln = pack_at(fr, [2, 11])
    want, rings = check(ctx, buf, off, ln, t, nrings=nrings)
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


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_nic_fwd_and_eth_kinds(ctx, rec_bytes):
    buf, off, ln = pack_at(mixed(), [2, 9, 0, 7])
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    want, rings = check(ctx, buf, off, ln, t, in_ifidx=0, rec_bytes=rec_bytes)
    sent = FR.sent_mask(want, 4)
    assert (want["kind"] == F.ETH).sum() > 20 and (want["arp_idx"][sent & (want["kind"] == F.IP)] == 0xFFFF).all()
    assert rings["count"][:4].tolist() == [0, 0, int(sent.sum()), 0]
    want, rings = check(ctx, buf, off, ln, t, in_ifidx=1, rec_bytes=rec_bytes)
    assert (want["kind"] == F.NO_NIC).sum() > 20 and (rings["count"][:4] > 0).all()
    want, rings = check(ctx, buf, off, ln, mosrx.fwd_tables(**HOLES), rec_bytes=rec_bytes)
    assert (want["kind"] == F.NO_ROUTE).sum() > 20 and (want["kind"] == F.NO_ARP).sum() > 20


def test_more_rings_than_netdevs(ctx):
    buf, off, ln = pack_at(base_frames(600), [2, 5])
    want, rings = check(ctx, buf, off, ln, mosrx.fwd_tables(**WALK), nrings=16)
    m = int(rings["count"][:4].sum())
    assert m > 0 and [r.tolist() for r in rings[4:16]] == [(m, 0, 0, 0)] * 12


def test_hand_made_plan(ctx):
    """Records the plan kernel never writes: out_ifidx >= nrings, kinds outside the enum and tx_len < 14 are not sent."""
    buf, off, ln = pack_at(mixed(700), [2, 9, 0, 7])

    def mutate(pl):
        s = np.nonzero(FR.sent_mask(pl, 4))[0]
        pl["tx_len"][s[::7]] = 13
        pl["tx_len"][s[1::21]] = 0
        pl["out_ifidx"][s[2::7]] = 4
        pl["out_ifidx"][s[3::21]] = 15
        pl["out_ifidx"][s[4::21]] = -1
        pl["kind"][s[5::7]] = 7
        pl["kind"][s[6::21]] = 255
        return pl
    clean, whole = check(ctx, buf, off, ln, mosrx.fwd_tables(**WALK))
    want, rings = check(ctx, buf, off, ln, mosrx.fwd_tables(**WALK), mutate=mutate)
    assert 0 < rings["count"][:4].sum() < whole["count"][:4].sum() * 0.6


@pytest.mark.parametrize("shift", [0, 3])
def test_exact_end_and_cut_frames(ctx, shift):
    """The last frame, 14 bytes, ends exactly at frames_bytes; then frames_bytes 3 and 40 bytes earlier: the cut
    Ethernet frame is not sent (under 14 bytes are left), cut IPv4 frames before it are not forwarded."""
    fr = mixed(2 * T + 3) + [eth_frame(14, 99)]
    buf, off, ln = pack_at(fr, [(shift + k) % 4 + 4 * k for k in range(4)])
    buf = buf[:int(off[-1]) + int(ln[-1])].copy()
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 1}))
    for rb in (16, 8):
        want, _ = check(ctx, buf, off, ln, t, rec_bytes=rb)
        assert want[-1]["kind"] == F.ETH and want[-1]["tx_len"] == 14
    for short in (3, 40):
        want, _ = check(ctx, buf, off, ln, t, frames_bytes=len(buf) - short)
        assert want[-1]["kind"] == F.NONE
        want, _ = check(ctx, buf, off, ln, mosrx.fwd_tables(**WALK), frames_bytes=len(buf) - short)


def test_limit(ctx):
    t = mosrx.fwd_tables(**WALK)
    buf, off, ln = pack_at(varied(32 * T + 1), [2, 7, 0, 13])
    check(ctx, buf, off[:T], ln[:T], t, limit=T, one=True)
    check(ctx, buf, off[:T + 1], ln[:T + 1], t, limit=T, one=False)      # the three launches: the scratch is written
    check(ctx, buf, off[:T + 1], ln[:T + 1], t, limit=0, one=False)
    check(ctx, buf, off, ln, t, limit=MAX, one=False)                    # 32 T + 1 frames: above the hard cap


# ---- the queue form (PLAN = true) ------------------------------------------------

def run_queue(ctx, ns, tables, nrings=4, in_ifidx=None, rec_bytes=16, limit=MAX, one=True, frames=None):
    fr = frames if frames is not None else varied(sum(ns))
    s = Setup(ctx, split(fr, ns))
    out = None
    try:
        ctx.fwd_set(tables)
        want = s.want_plans(tables, in_ifidx)
        q = s.queue(rec_bytes)
        out = DescOutputs(ctx, s.ns, nrings)
        out.attach(q, in_ifidx)
        ctx.set_fwd_one(limit)
        for _ in range(2):                                  # a run is one launch, every time
            out.fill()
            c0 = ctx.fwd_one_count()
            q.run()
            assert ctx.fwd_one_count() == c0 + (1 if one else 0)
            rings = out.check(s, tables, want, (ns, rec_bytes, limit))
        return want, rings
    finally:
        ctx.set_fwd_one(0)
        s.close()
        if out:
            out.free()


QUEUES = {"one": [T + 1], "one_empty": [0], "three": [0, 5 * T + 3, 1],
          "forty": [0, 0, 1, T - 1, T, T + 1, 5 * T + 3, 0, 0, 1] + [T + 1, 0, T - 1, 1, T, 0] * 4 + [5 * T + 3, T, 1, 0, 0, 0]}


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("name", sorted(QUEUES))
def test_queue(ctx, name, rec_bytes):
    ns = QUEUES[name]
    assert len(ns) in (1, 3, 40)
    ifs = [i % 2 for i in range(len(ns))]
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    want, rings = run_queue(ctx, ns, t, in_ifidx=ifs, rec_bytes=rec_bytes, frames=mixed(sum(ns)))
    assert [int(r["count"][:4].sum()) for r in rings] == [int(FR.sent_mask(w, 4).sum()) for w in want]
    for w, r, i, n in zip(want, rings, ifs, ns):
        if i == 0 and n:                                    # the nic_forward_table shortcut, per batch
            assert r["count"][:4].tolist() == [0, 0, int(FR.sent_mask(w, 4).sum()), 0]


def test_queue_limit(ctx):
    t = mosrx.fwd_tables(**WALK)
    ns = [T, 0, T - 1, T + 1, 1]
    run_queue(ctx, ns, t, limit=T, one=False)               # one batch of T + 1: the whole run takes four launches
    run_queue(ctx, ns, t, limit=T + 1, one=True)
    run_queue(ctx, ns, t, limit=0, one=False)
    run_queue(ctx, [T, 32 * T + 1], t, limit=MAX, one=False)
    run_queue(ctx, [T, 32 * T], t, limit=MAX, one=True, rec_bytes=8)


def test_queue_16_rings(ctx):
    make, _ = SPREADS["runs_of_300"]
    ns = [1500, 2100, 1200]
    fr, t, nrings = make(sum(ns))
    want, rings = run_queue(ctx, ns, t, nrings=nrings, frames=fr)
    assert sum(int(r["count"][:16].sum()) for r in rings) == sum(ns)


# ---- refusals: unchanged with the limit set, and nothing is launched -------------

def test_refusals_launch_nothing(ctx):
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
        ctx.set_fwd_one(MAX)
        c0 = ctx.fwd_one_count()

        def build(**kw):
            return L.mosrx_fwd_desc_rings_dev(ctx.handle, C.byref(b), kw.get("plan", r.d_plan.ptr), kw.get("nrings", 4),
                                              kw.get("tsrc", tsrc), kw.get("tlen", tlen), kw.get("tmac", tmac),
                                              kw.get("rings", rings), kw.get("scr", scr), kw.get("sb", 256), None)
        ctx.fwd_set(None)
        assert build() == -ENOENT                                     # no tables
        ctx.fwd_set(mosrx.fwd_tables(**WALK))
        for kw in (dict(plan=None), dict(plan=r.d_plan.ptr + 4), dict(tsrc=tsrc + 2), dict(tlen=tlen + 1),
                   dict(tmac=tmac + 2), dict(rings=None), dict(rings=rings + 8), dict(scr=None), dict(scr=scr + 8),
                   dict(sb=63), dict(nrings=0), dict(nrings=17), dict(nrings=3)):
            assert build(**kw) == -EINVAL, kw
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        assert ctx.fwd_one_count() == c0
        for d, a in zip(bufs, init):                                  # nothing ran
            assert np.array_equal(d.download(np.zeros_like(a)).view(np.uint8), a.view(np.uint8))
    finally:
        L.mosrx_sync(ctx.handle)
        ctx.set_fwd_one(0)
        r.free()


def test_queue_refusals_launch_nothing(ctx):
    ns = [300, 0, 257]
    s = Setup(ctx, split(base_frames(sum(ns)), ns))
    out = None
    try:
        t = mosrx.fwd_tables(**WALK)
        ctx.fwd_set(t)
        q, out = s.queue(), DescOutputs(ctx, ns, 4)
        out.attach(q)
        ctx.set_fwd_one(MAX)
        c0 = ctx.fwd_one_count()

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
        assert ctx.fwd_one_count() == c0
    finally:
        ctx.set_fwd_one(0)
        s.close()
        if out:
            out.free()


# ---- MOSRX_OP_FWD_DESC -----------------------------------------------------------

@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_timing_op(ctx, rec_bytes):
    """The op's plan (the output it leaves where a caller can read it) equals the restatement's in both forms;
    with the limit set each batch under it is one launch (PLAN = true), the larger one the four."""
    ctx.set_params(mosrx.default_params(**PARAMS))
    ctx.fwd_set_listener(False)
    t = mosrx.fwd_tables(**WALK)
    ctx.fwd_set(t)
    dbs, want = [], []
    try:
        for n in (300, 1000):
            buf, off, ln = pack_at(base_frames(n), [2, 7])
            db = ctx.upload(buf, off, ln)
            ctx.classify_dev(db) if rec_bytes == 16 else ctx.classify_dev_compact(db)
            dbs.append(db)
            want.append(F.plan(buf, off, ln, O.classify(buf, off, ln, O.params(**PARAMS))["reason"], t, 0, forward=1, num_msp=1))
        grew = {}
        for limit in (0, MAX, 512):
            ctx.set_fwd_one(limit)
            for d in dbs:
                if d.d_fplan is not None:
                    d.d_fplan.upload(ee(d.n, np.uint64))
            c0 = ctx.fwd_one_count()
            tot, avg = ctx.time_op(mosrx.OP_FWD_DESC, dbs, 4, arg=rec_bytes)
            assert tot > 0 and avg > 0
            grew[limit] = ctx.fwd_one_count() - c0
            for d, w in zip(dbs, want):
                got = d.d_fplan.download(np.zeros(d.n, np.uint64))
                assert got.tobytes() == w.view(np.uint64).tobytes(), limit
        # 4 launches in the stream timing and 4 in the kernel timing, the batches taking turns: every one of them
        # with the limit at the cap, those of the 300-frame batch alone with it at 512, none with it at 0
        assert grew[0] == 0 and grew[MAX] >= 8 and 0 < grew[512] < grew[MAX], grew
    finally:
        ctx.set_fwd_one(0)
        for d in dbs:
            d.free()
