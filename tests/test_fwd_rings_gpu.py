"""The ring form of the forwarding build on the GPU (mosrx_fwd_build_rings_dev)
against its restatement (tests/fwd_rings_oracle.py).

Every buffer is filled with 0xEE before the launches and has canary entries
after it; the restatement writes into copies of the same images and the
comparison is exact, so padding, ring tails, dropped frames' entries, entries
past the last ring and d_rings[nrings ..] are all part of it.  The plan given to
the build is the GPU's own mosrx_fwd_plan_dev output, asserted equal to the
restatement's plan first.  Expected values never come from the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_fwd_gpu import DEVS4, DSTS, PAD, TILE, WALK, Run, base_frames, ee, eth_frame, ip_frame, pack_at
from test_fwd_rings_oracle import NET16
from test_oracle_golden import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = ("tx_frames", "tx_off", "tx_len", "tx_src", "rings")
BY_NIF = ["8.8.8.8", "10.1.2.3", "192.168.1.7", "192.168.9.9"]      # WALK: netdev 0, 1, 2, 3


class RingRun(Run):
    def build_rings(self, ring_cap, nrings, sync=True):
        """Returns the device buffers and their initial host images."""
        n, ctx = self.n, self.ctx
        init = [ee(nrings * ring_cap + 64, np.uint8), ee(n + PAD, np.uint32), ee(n + PAD, np.uint16),
                ee(n + PAD, np.uint32), ee(nrings + 2, mosrx.FWD_RING_DTYPE)]
        dev = [mosrx.DevBuffer(ctx, a.nbytes) for a in init]
        for d, a in zip(dev, init):
            d.upload(a)
        sb = mosrx.lib().mosrx_fwd_rings_scratch_bytes(n, nrings)
        scr = mosrx.DevBuffer(ctx, sb)
        self.bufs += dev + [scr]
        ctx.fwd_build_rings_dev(self.db.batch(), self.d_plan.ptr, dev[0].ptr, ring_cap, nrings, dev[1].ptr, dev[2].ptr,
                                dev[3].ptr, dev[4].ptr, scr.ptr, sb, sync=sync)
        return dev, init


def download(dev, init):
    return [d.download(np.zeros_like(i0)) for d, i0 in zip(dev, init)]


def assert_same(got, exp, what):
    for name, g, e in zip(NAMES, got, exp):
        g, e = g.view(np.uint8) if name == "rings" else g, e.view(np.uint8) if name == "rings" else e
        diff = np.nonzero(g != e)[0]
        assert not len(diff), (name, what, len(diff), diff[:8].tolist(), g[diff[:8]].tolist(), e[diff[:8]].tolist())


def caps_of(need, which):
    """Ring caps from the rings' needs (16-byte units): names, or byte counts as given."""
    top = int(need.max()) * 16
    return [{"exact": top, "minus16": max(top - 16, 0), "half": top // 2 // 16 * 16}.get(w, w) for w in which]


def check(ctx, buf, off, ln, tables, nrings=None, in_ifidx=0, rec_bytes=16, caps=("exact",)):
    """Plan + ring build on the GPU equal the restatement for each cap; returns (plan, rings at the first cap)."""
    nrings = tables.num_netdevs if nrings is None else nrings
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(tables)
    rec = O.classify(buf, off, ln, O.params(num_msp=1, forward=1))
    want = F.plan(buf, off, ln, rec["reason"], tables, in_ifidx, forward=1, num_msp=1)
    r = RingRun(ctx, buf, off, ln, rec_bytes)
    first = None
    try:
        r.plan(in_ifidx)
        got = r.plan_result()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]]
        for cap in caps_of(FR.need_units(want, nrings), caps):
            dev, init = r.build_rings(cap, nrings)
            exp = FR.build(buf, off, want, tables, cap, nrings, *init)
            assert_same(download(dev, init), exp, ("cap", cap))
            first = exp[4] if first is None else first
        return want, first
    finally:
        r.free()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5003])
def test_frame_counts_every_third(gpu_ctx, n):
    buf, off, ln = pack_at(base_frames(n), [2, 7, 0, 13])
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), caps=("exact", "minus16"))
    if n >= 64:
        assert (rings["count"][:4] > 0).all() and rings["count"][:4].sum() <= (n + 2) // 3


def one_netdev(n):
    return [ip_frame("10.1.2.3", 20 + (i * 13) % 100, seed=i) for i in range(n)], mosrx.fwd_tables(**WALK), 4


def one_ring(n):
    t = dict(routes=[("0.0.0.0/0", 0)], arp=[(f"{a}.0.0.0/2", "02:00:00:00:00:01") for a in (0, 64, 128, 192)],
             netdevs=DEVS4[:1])
    return [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 13) % 100, seed=i) for i in range(n)], mosrx.fwd_tables(**t), 1


def round_robin_16(n):
    return ([ip_frame(f"10.{i % 16}.3.{i % 250}", 20 + (i * 29) % 300, pad=i % 4, seed=i) for i in range(n)],
            mosrx.fwd_tables(**NET16), 16)


def middle_gets_nothing(n):
    d = [BY_NIF[0], BY_NIF[1], BY_NIF[3]]
    return [ip_frame(d[(i * 5) % 3], 20 + (i * 31) % 200, pad=i % 3, seed=i) for i in range(n)], mosrx.fwd_tables(**WALK), 4


def runs_of_300(n):
    return ([ip_frame(f"10.{(i // 300) % 16}.0.{i % 250}", 20 + (i * 7) % 90, seed=i) for i in range(n)],
            mosrx.fwd_tables(**NET16), 16)


SPREADS = {"one_netdev_of_4": (one_netdev, 700), "one_ring": (one_ring, 700), "round_robin_16": (round_robin_16, 1100),
           "middle_gets_nothing": (middle_gets_nothing, 700), "runs_of_300": (runs_of_300, 4800)}


@pytest.mark.parametrize("name", sorted(SPREADS))
def test_spreads(gpu_ctx, name):
    make, n = SPREADS[name]
    fr, t, nrings = make(n)
    buf, off, ln = pack_at(fr, [2, 11])
    want, rings = check(gpu_ctx, buf, off, ln, t, nrings=nrings, caps=("exact", "minus16"))
    c = rings["count"][:nrings]
    if name == "one_netdev_of_4":
        assert c.tolist() == [0, n, 0, 0] and rings["start"][:4].tolist() == [0, 0, n, n]
    if name == "one_ring":
        assert c.tolist() == [n]
    if name == "round_robin_16":
        assert c.min() >= n // 16 and c.sum() == n
    if name == "middle_gets_nothing":
        assert c[2] == 0 and c[0] > 0 and c[1] > 0 and c[3] > 0 and rings["start"][3] == rings["start"][2]
    if name == "runs_of_300":
        assert c.tolist() == [300] * 16


def test_more_rings_than_netdevs(gpu_ctx):
    buf, off, ln = pack_at(base_frames(600), [2, 5])
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), nrings=16, caps=("exact", "minus16"))
    m = int(rings["count"][:4].sum())
    assert m > 0 and [r.tolist() for r in rings[4:16]] == [(m, 0, 0, 0)] * 12


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_ring_bounds(gpu_ctx, rec_bytes):
    """ring_cap exactly the fullest ring's need, one unit less, half, one unit, and 0."""
    buf, off, ln = pack_at(base_frames(900), [2, 5])
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), rec_bytes=rec_bytes,
                        caps=("exact", "minus16", "half", 16, 0))
    assert (rings["dropped"][:4] == 0).all()


def test_mixed_traffic_nic_fwd(gpu_ctx):
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 29) % 300, pad=i % 4, seed=i) for i in range(300)]
    for i in range(5, 300, 11):
        fr[i] = eth_frame(14 + (i * 3) % 90, i)
    buf, off, ln = pack_at(fr, [2, 9])
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    want, rings = check(gpu_ctx, buf, off, ln, t, in_ifidx=0, caps=("exact", "half"))
    assert rings["count"][:4].tolist() == [0, 0, 300, 0] and (want["kind"] == F.ETH).sum() == 27
    # in_ifidx 1 has no nic_forward_table entry (-1): IP frames walk the tables, the others stay
    want, rings = check(gpu_ctx, buf, off, ln, t, in_ifidx=1, rec_bytes=8, caps=("exact", "half"))
    assert (want["kind"] == F.NO_NIC).sum() == 27 and (rings["count"][:4] > 0).all()


def test_alignments_ip(gpu_ctx):
    """Every source off mod 16 x every tx_len mod 16 (test_fwd_gpu's input), the frames spread over 4 rings."""
    fr, ph = [], []
    for a in range(16):
        for m in range(16):
            fr += [ip_frame(BY_NIF[(a + m) % 4], 20 + m, seed=a), ip_frame(BY_NIF[(a + m + 1) % 4], 100 + m, seed=a),
                   ip_frame(BY_NIF[(a + m + 2) % 4], 52 + m, pad=1 + (a + m) % 9, seed=a)]
            ph += [a, a, a]
    buf, off, ln = pack_at(fr, ph)
    assert {(int(o) % 16, (14 + 20 + m) % 16) for o, m in zip(off[::3], list(range(16)) * 16)} == \
        {(a, (34 + m) % 16) for a in range(16) for m in range(16)}
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK))
    assert rings["count"][:4].sum() == len(fr) and (rings["count"][:4] > 0).all()
    check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(netdevs=DEVS4, nic_fwd={0: 2}), rec_bytes=8)


def test_alignments_jumbo(gpu_ctx):
    fr = [ip_frame(BY_NIF[a % 4], 8986 + a, seed=a) for a in range(16)]
    buf, off, ln = pack_at(fr, list(range(16)))
    want, rings = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), caps=("exact", "minus16"))
    assert rings["count"][:4].tolist() == [4] * 4 and want["tx_len"].max() == 9000 + 15


@pytest.mark.parametrize("name", ["conv_walk", "edge_walk", "conv_nicfwd"])
@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_mos_fixture(gpu_ctx, name, rec_bytes):
    """Ring 0 holds the frames mOS itself sent (tests/golden/fwd_plan.npz)."""
    z = np.load(os.path.join(GOLDEN, "fwd_plan.npz"))
    k = name + "__"
    t = mosrx.FwdTables.from_buffer_copy(z[k + "tables"].tobytes())
    buf, off, ln = z[k + "frames"], z[k + "off"], z[k + "len"]
    ctx = gpu_ctx
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1, local=["127.0.0.1"]))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(t)
    r = RingRun(ctx, buf, off, ln, rec_bytes)
    try:
        r.plan()
        np.testing.assert_array_equal(r.plan_result().view(np.uint64), z[k + "plan"].view(np.uint64))
        cap = (len(z[k + "tx"]) + 15) // 16 * 16
        nrings = max(t.num_netdevs, 1)
        dev, init = r.build_rings(cap, nrings)
        tx, toff, tlen, tsrc, rings = download(dev, init)
        m = len(z[k + "tx_off"])
        assert rings[0].tolist()[:3] == (0, m, 0)
        assert FR.ring_list(tx, toff, tlen, rings, 0) == F.tx_list(z[k + "tx"], z[k + "tx_off"], z[k + "tx_len"], m)
        np.testing.assert_array_equal(tsrc[:m], z[k + "tx_src"])
        np.testing.assert_array_equal(toff[:m], z[k + "tx_off"])
    finally:
        r.free()


def test_two_table_sets_on_one_stream(gpu_ctx):
    """Ring builds submitted before a set keep the tables they were given."""
    ctx = gpu_ctx
    fr = [ip_frame(DSTS[i % len(DSTS)], 40 + i % 50, seed=i) for i in range(700)]
    buf, off, ln = pack_at(fr, [2])
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    ctx.fwd_set_listener(False)
    rec = O.classify(buf, off, ln, O.params(num_msp=1, forward=1))
    swapped = dict(WALK, routes=[("10.0.0.0/8", 3), ("192.168.0.0/16", 0), ("0.0.0.0/0", 2)],
                   netdevs=[f"02:00:00:00:cc:{i:02x}" for i in range(4)])
    t1, t2 = mosrx.fwd_tables(**WALK), mosrx.fwd_tables(**swapped)
    runs = [RingRun(ctx, buf, off, ln), RingRun(ctx, buf, off, ln)]
    try:
        outs = []
        for r, t in zip(runs, (t1, t2)):
            ctx.fwd_set(t)
            r.plan(sync=False)
            want = F.plan(buf, off, ln, rec["reason"], t, 0)
            cap = int(FR.need_units(want, 4).max()) * 16
            outs.append((r, t, want, cap, r.build_rings(cap, 4, sync=False)))
        ctx.fwd_set(None)
        with pytest.raises(mosrx.MosrxError) as e:
            runs[0].build_rings(outs[0][3], 4, sync=False)
        assert e.value.errno == 2                                   # ENOENT
        mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
        for r, t, want, cap, (dev, init) in outs:
            np.testing.assert_array_equal(r.plan_result().view(np.uint64), want.view(np.uint64))
            assert_same(download(dev, init), FR.build(buf, off, want, t, cap, 4, *init), "stream")
        assert not np.array_equal(outs[0][2].view(np.uint64), outs[1][2].view(np.uint64))
    finally:
        for r in runs:
            r.free()


def test_errors_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    buf, off, ln = pack_at(base_frames(100), [2])
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    r = RingRun(ctx, buf, off, ln)
    L, b = mosrx.lib(), r.db.batch()
    try:
        n, cap = r.n, 4096
        init = [ee(4 * cap, np.uint8), ee(n, np.uint32), ee(n, np.uint16), ee(n, np.uint32), ee(4, mosrx.FWD_RING_DTYPE)]
        bufs = [mosrx.DevBuffer(ctx, a.nbytes) for a in init] + [mosrx.DevBuffer(ctx, 256)]
        r.bufs += bufs
        for d, a in zip(bufs, init):
            d.upload(a)
        tx, toff, tlen, tsrc, rings, scr = (x.ptr for x in bufs)

        def build(**kw):
            return L.mosrx_fwd_build_rings_dev(ctx.handle, C.byref(b), kw.get("plan", r.d_plan.ptr), kw.get("tx", tx),
                                               kw.get("cap", cap), kw.get("nrings", 4), kw.get("toff", toff),
                                               kw.get("tlen", tlen), kw.get("tsrc", tsrc), kw.get("rings", rings),
                                               kw.get("scr", scr), kw.get("sb", 256), None)
        ctx.fwd_set(None)
        assert build() == -2                                          # ENOENT: no tables
        ctx.fwd_set(mosrx.fwd_tables(**WALK))
        assert L.mosrx_fwd_rings_scratch_bytes(n, 4) == 64
        for kw in (dict(plan=None), dict(plan=r.d_plan.ptr + 4), dict(tx=None), dict(tx=tx + 8), dict(toff=None),
                   dict(toff=toff + 2), dict(tlen=None), dict(tlen=tlen + 1), dict(tsrc=None), dict(tsrc=tsrc + 2),
                   dict(rings=None), dict(rings=rings + 8), dict(scr=None), dict(scr=scr + 8), dict(sb=63),
                   dict(nrings=0), dict(nrings=17), dict(nrings=3), dict(cap=4088), dict(cap=(1 << 30) + 16),
                   dict(cap=1 << 33)):
            assert build(**kw) == -22, kw                             # EINVAL
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        for d, a in zip(bufs, init):                                  # nothing ran
            assert np.array_equal(d.download(np.zeros_like(a)).view(np.uint8), a.view(np.uint8))
    finally:
        L.mosrx_sync(ctx.handle)
        r.free()


def test_timing_op(gpu_ctx):
    ctx = gpu_ctx
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    ctx.fwd_set(mosrx.fwd_tables(**WALK))
    dbs = []
    try:
        for n in (300, 1000):
            buf, off, ln = pack_at(base_frames(n), [2, 7])
            db = ctx.upload(buf, off, ln)
            ctx.classify_dev(db)
            dbs.append(db)
        tot, avg = ctx.time_op(mosrx.OP_FWD_RINGS, dbs, 4, arg=16)
        assert tot > 0 and avg > 0
        bs = (mosrx.Batch * 2)(*[d.batch() for d in dbs])
        outs = (C.c_void_p * 2)(*[d.d_out.ptr for d in dbs])
        aux = (C.c_void_p * 2)(*[d.d_fplan.ptr for d in dbs])
        ms = C.c_float()
        assert mosrx.lib().mosrx_time_op_dispatch(ctx.handle, mosrx.OP_FWD_RINGS, 16, bs, 2, outs, aux, 2,
                                                  C.byref(ms)) == -95    # ENOTSUP
    finally:
        for d in dbs:
            d.free()
