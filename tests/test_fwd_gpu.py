"""Forwarding on the GPU (mosrx_fwd_plan_dev / mosrx_fwd_build_dev) against the
restatement (tests/fwd_oracle.py) and mOS's own TX frames (golden/fwd_plan.npz).

The plan records and every TX array are compared exactly, over buffers filled
with 0xEE before the launches: the restatement writes into copies of the same
buffers, so canaries after each array, entries past m and every padding byte
are part of the comparison.  Expected values never come from the GPU: the
records the restatement plans from are the oracle's."""
import os
import struct

import numpy as np
import pytest

import fwd_oracle as F
import mosrx
import oracle_py as O
from test_forwarding import FSTATES
from test_oracle_golden import GOLDEN

pytestmark = pytest.mark.gpu

TILE = 256           # MOSRX_FWD_TILE (checked below)
PAD = 8              # canary entries after each tx_* array
DEVS4 = [f"02:00:00:00:aa:{i:02x}" for i in range(4)]


def ip_frame(dst, tot_len, pad=0, ok=True, seed=0):
    """Ethernet + IPv4 (protocol 253, no options) with tot_len bytes of packet and
    `pad` trailing bytes; ok=False breaks the IP checksum (IP_BADCSUM: not forwarded)."""
    rng = np.random.default_rng(seed * 7919 + tot_len * 31 + pad)
    eth = bytes([0x02, 0xD0, 0, 0, 0, seed & 0xFF, 0x02, 0x50, 0, 0, 0, 1, 0x08, 0x00])
    h = bytearray(struct.pack("!BBHHHBBH4s4s", 0x45, 0, tot_len, seed & 0xFFFF, 0, 64, 253, 0,
                              bytes([10, 0, 0, 1]), bytes(int(x) for x in dst.split("."))))
    s = sum(struct.unpack("!10H", bytes(h)))
    s = (s & 0xFFFF) + (s >> 16)
    s = (s & 0xFFFF) + (s >> 16)
    struct.pack_into("!H", h, 10, (~s & 0xFFFF) ^ (0 if ok else 0x5A5A))
    return eth + bytes(h) + rng.integers(0, 256, tot_len - 20 + pad, dtype=np.uint8).tobytes()


def eth_frame(n, seed=0):
    """A non-IPv4 frame of n >= 14 bytes."""
    rng = np.random.default_rng(1000 + seed + n)
    return bytes([0x02, 0xE0, 0, 0, 0, 1, 0x02, 0xE0, 0, 0, 0, 2, 0x88, 0xB5]) + \
        rng.integers(0, 256, n - 14, dtype=np.uint8).tobytes()


def pack_at(frames, phases):
    """Frame i at the next 16-byte boundary + phases[i % len(phases)]."""
    off, pos, parts = [], 0, []
    for i, f in enumerate(frames):
        o = (pos + 15) // 16 * 16 + phases[i % len(phases)]
        parts.append(b"\0" * (o - pos) + f)
        off.append(o)
        pos = o + len(f)
    buf = np.frombuffer(b"".join(parts) + b"\0" * 64, np.uint8).copy()
    return buf, np.array(off, np.uint32), np.array([len(f) for f in frames], np.uint16)


def ee(n, dtype):
    return np.frombuffer(b"\xEE" * (n * np.dtype(dtype).itemsize), dtype).copy()


def cap_for(pl):
    s = np.isin(pl["kind"], [F.IP, F.ETH])
    return int(((pl["tx_len"][s].astype(np.int64) + 2 + 15) // 16).sum()) * 16


class Run:
    """One batch on the GPU: classify, plan, build; download everything."""

    def __init__(self, ctx, buf, off, ln, rec_bytes=16, frames_bytes=None):
        self.ctx, self.buf, self.off, self.ln, self.rb = ctx, buf, off, ln, rec_bytes
        self.n = len(off)
        self.db = ctx.upload(buf, off, ln, frames_bytes=frames_bytes)
        if rec_bytes == 16:
            ctx.classify_dev(self.db)
            self.d_rec = self.db.d_out
        else:
            ctx.classify_dev_compact(self.db)
            self.d_rec = self.db.d_out8
        self.d_plan = mosrx.DevBuffer(ctx, max(self.n * 8, 8) + 8)
        self.d_plan.upload(ee(self.n + 1, np.uint64))
        self.bufs = []

    def plan(self, in_ifidx=0, sync=True):
        b = self.db.batch()
        self.ctx.fwd_plan_dev(b, self.d_rec.ptr, self.rb, in_ifidx, self.d_plan.ptr, sync=sync)

    def plan_result(self):
        raw = self.d_plan.download(np.zeros(self.n + 1, np.uint64))
        assert raw[self.n] == 0xEEEEEEEEEEEEEEEE
        return raw[:self.n].view(mosrx.FWD_DTYPE)

    def build(self, tx_cap, sync=True):
        """Returns the device buffers and their initial host images."""
        n, ctx = self.n, self.ctx
        init = [ee(tx_cap + 64, np.uint8), ee(n + PAD, np.uint32), ee(n + PAD, np.uint16), ee(n + PAD, np.int8),
                ee(n + PAD, np.uint32), ee(2 + PAD, np.uint32)]
        dev = [mosrx.DevBuffer(ctx, a.nbytes) for a in init]
        for d, a in zip(dev, init):
            d.upload(a)
        sb = mosrx.lib().mosrx_fwd_scratch_bytes(n)
        scr = mosrx.DevBuffer(ctx, sb)
        self.bufs += dev + [scr]
        ctx.fwd_build_dev(self.db.batch(), self.d_plan.ptr, dev[0].ptr, tx_cap, dev[1].ptr, dev[2].ptr, dev[3].ptr,
                          dev[4].ptr, dev[5].ptr, scr.ptr, sb, sync=sync)
        return dev, init

    def free(self):
        for b in self.bufs + [self.d_plan]:
            b.free()
        self.db.free()


def check(ctx, buf, off, ln, tables, in_ifidx=0, rec_bytes=16, caps=(None,), msp=1, esp=0, listener=False,
          local=(), expect_sent=None):
    """Plan + build on the GPU equal the restatement, for each tx_cap in caps (None: exactly what is needed)."""
    ctx.set_params(mosrx.default_params(num_msp=msp, num_esp=esp, forward=1, local=list(local) or None))
    ctx.fwd_set_listener(listener)
    ctx.fwd_set(tables)
    rec = O.classify(buf, off, ln, O.params(num_msp=msp, num_esp=esp, forward=1, local=local))
    want = F.plan(buf, off, ln, rec["reason"], tables, in_ifidx, forward=1, num_msp=msp, listener=listener)
    r = Run(ctx, buf, off, ln, rec_bytes)
    try:
        r.plan(in_ifidx)
        got = r.plan_result()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]]
        need = cap_for(want)
        for cap in caps:
            cap = need if cap is None else max(need + cap, 0) if cap < 0 else cap
            dev, init = r.build(cap)
            exp = F.build(buf, off, want, tables, cap, *init[:5])
            cnt = init[5].copy()
            cnt[:2] = exp[5]
            names = ("tx_frames", "tx_off", "tx_len", "tx_nif", "tx_src", "tx_count")
            for name, d, i0, e in zip(names, dev, init, list(exp[:5]) + [cnt]):
                g = d.download(np.zeros_like(i0))
                diff = np.nonzero(g != e)[0]
                assert not len(diff), (name, cap, len(diff), diff[:8].tolist(), g[diff[:8]].tolist(), e[diff[:8]].tolist())
            if expect_sent is not None and cap == need:
                assert int(exp[5][0]) == expect_sent and int(exp[5][1]) == 0
        return want
    finally:
        r.free()


DSTS = ["10.1.2.3", "10.200.0.9", "192.168.1.77", "192.168.9.9", "172.16.5.5", "8.8.8.8", "10.1.2.4", "192.168.2.27"]
WALK = dict(routes=[("10.0.0.0/8", 1), ("192.168.0.0/16", 2), ("192.168.9.9/32", 3), ("0.0.0.0/0", 0)],
            arp=[("10.0.0.0/8", "02:00:00:00:00:01"), ("192.168.0.0/16", "02:00:00:00:00:02"),
                 ("192.168.2.27/1", "02:00:00:00:00:05"), ("192.168.2.27/32", "02:00:00:00:00:09"),
                 ("192.168.1.0/24", "02:00:00:00:00:03"), ("8.0.0.0/7", "02:00:00:00:00:04"),
                 ("0.0.0.0/0", "02:00:00:00:00:06")], netdevs=DEVS4)

_base = {}


def base_frames(n):
    """n frames, lengths and destinations mixed, every third forwarded (the others fail the IP checksum)."""
    if "f" not in _base:
        _base["f"] = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 37) % 240, pad=(i % 5) * 3, ok=i % 3 == 0, seed=i)
                      for i in range(5003)]
    return _base["f"][:n]


def test_tile_constant():
    assert mosrx.lib().mosrx_fwd_tile() == TILE


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5003])
def test_frame_counts_every_third(gpu_ctx, n):
    buf, off, ln = pack_at(base_frames(n), [2, 7, 0, 13])
    want = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), caps=(None, -16))
    if n >= 64:
        assert 0 < np.isin(want["kind"], [F.IP]).sum() <= (n + 2) // 3


@pytest.mark.parametrize("n", [1, TILE + 1, 1500])
@pytest.mark.parametrize("all_fwd", [True, False])
def test_all_or_none_forwarded(gpu_ctx, n, all_fwd):
    fr = [ip_frame("10.1.2.3", 20 + (i * 13) % 100, ok=all_fwd, seed=i) for i in range(n)]
    buf, off, ln = pack_at(fr, [2])
    check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), expect_sent=n if all_fwd else 0)


def test_alignments_ip(gpu_ctx):
    """Every source off mod 16 x every tx_len mod 16: the shortest packets (tot_len 20..35),
    packets filling the capture, and padded ones."""
    fr, ph = [], []
    for a in range(16):
        for m in range(16):
            fr += [ip_frame("10.1.2.3", 20 + m, seed=a), ip_frame("192.168.1.7", 100 + m, seed=a),
                   ip_frame("10.9.9.9", 52 + m, pad=1 + (a + m) % 9, seed=a)]
            ph += [a, a, a]
    buf, off, ln = pack_at(fr, ph)
    assert {(int(o) % 16, (14 + 20 + m) % 16) for o, m in zip(off[::3], list(range(16)) * 16)} == \
        {(a, (34 + m) % 16) for a in range(16) for m in range(16)}
    check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), expect_sent=len(fr))
    check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(netdevs=DEVS4, nic_fwd={0: 2}), rec_bytes=8, expect_sent=len(fr))


def test_alignments_jumbo_and_eth(gpu_ctx):
    fr, ph = [], []
    for a in range(16):
        fr += [ip_frame("10.1.2.3", 8986 + a, seed=a), eth_frame(14, a), eth_frame(15, a), eth_frame(60, a),
               eth_frame(61 + a, a)]
        ph += [a] * 5
    buf, off, ln = pack_at(fr, ph)
    want = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(netdevs=DEVS4, nic_fwd={0: 1}), expect_sent=len(fr))
    assert (want["kind"] == F.ETH).sum() == 64 and want["tx_len"].max() == 9000 + 15
    want = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), expect_sent=16)     # no table: non-IPv4 frames stay
    assert (want["kind"] == F.NO_NIC).sum() == 64


def big_tables():
    """128 routes and 1024 ARP entries, the matching ones last."""
    routes = [(f"11.{i}.0.0/16", i % 4) for i in range(127)] + [("10.0.0.0/8", 3)]
    arp = [(f"12.{i // 250}.{i % 250}.1/32", f"02:00:00:00:{i >> 8:02x}:{i & 255:02x}") for i in range(1022)]
    arp += [("10.1.2.3/1", "02:00:00:00:ff:01"), ("10.0.0.0/8", "02:00:00:00:ff:02")]
    return dict(routes=routes, arp=arp, netdevs=DEVS4)


TABLES = {
    "empty_routes": (dict(arp=WALK["arp"], netdevs=DEVS4), 0),
    "only_default_route": (dict(routes=[("0.0.0.0/0", 2)], arp=WALK["arp"], netdevs=DEVS4), 0),
    "equal_prefix_ties": (dict(routes=[("10.0.0.0/8", 2), ("10.0.0.0/8", 1), ("0.0.0.0/0", 3), ("0.0.0.0/0", 0)],
                               arp=[("10.0.0.0/8", "02:00:00:00:00:01"), ("10.0.0.0/8", "02:00:00:00:00:02"),
                                    ("0.0.0.0/1", "02:00:00:00:00:03")], netdevs=DEVS4), 0),
    "full_tables_match_last": (big_tables(), 0),
    "prefix1_override": (dict(routes=[("0.0.0.0/0", 0)],
                              arp=[("10.1.2.3/32", "02:00:00:00:00:01"), ("10.1.2.3/1", "02:00:00:00:00:02"),
                                   ("10.1.2.3/32", "02:00:00:00:00:03"), ("10.0.0.0/8", "02:00:00:00:00:04")],
                              netdevs=DEVS4), 0),
    "default_arp_only": (dict(routes=[("0.0.0.0/0", 0)], arp=[("0.0.0.0/0", "02:00:00:00:00:01")], netdevs=DEVS4), 0),
    "nic_fwd_in0": (dict(WALK, nic_fwd={0: 3}), 0),
    "nic_fwd_in1_none": (dict(WALK, nic_fwd={0: 3}), 1),
    "four_netdevs": (WALK, 0),
}


@pytest.mark.parametrize("name", sorted(TABLES))
@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_tables(gpu_ctx, name, rec_bytes):
    kw, in_ifidx = TABLES[name]
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 29) % 300, pad=i % 4, seed=i) for i in range(300)]
    fr[5], fr[77] = eth_frame(60, 1), eth_frame(99, 2)
    buf, off, ln = pack_at(fr, [2, 9])
    want = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**kw), in_ifidx=in_ifidx, rec_bytes=rec_bytes)
    k = np.bincount(want["kind"], minlength=6)
    if name == "empty_routes":
        assert k[F.NO_ROUTE] == 298 and k[F.NO_NIC] == 2
    if name == "four_netdevs":
        assert set(want["out_ifidx"][want["kind"] == F.IP].tolist()) == {0, 1, 2, 3}
    if name == "prefix1_override":
        assert set(want["arp_idx"][want["kind"] == F.IP].tolist()) == {1, 3}
    if name == "full_tables_match_last":
        assert set(want["arp_idx"][want["kind"] == F.IP].tolist()) == {1022, 1023} and k[F.NO_ROUTE] > 0
    if name == "default_arp_only":
        assert k[F.NO_ARP] == 298
    if name == "nic_fwd_in0":
        assert k[F.IP] == 298 and k[F.ETH] == 2
    if name == "nic_fwd_in1_none":
        assert k[F.NO_NIC] == 2 and k[F.IP] > 0 and k[F.NO_ARP] > 0


def test_set_replace_clear_on_one_stream(gpu_ctx):
    """Launches submitted before a set keep the tables they were given."""
    ctx = gpu_ctx
    fr = [ip_frame(DSTS[i % len(DSTS)], 40 + i % 50, seed=i) for i in range(700)]
    buf, off, ln = pack_at(fr, [2])
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    ctx.fwd_set_listener(False)
    rec = O.classify(buf, off, ln, O.params(num_msp=1, forward=1))
    t1, t2 = mosrx.fwd_tables(**WALK), mosrx.fwd_tables(**TABLES["prefix1_override"][0])
    runs = [Run(ctx, buf, off, ln), Run(ctx, buf, off, ln)]
    try:
        outs = []
        for r, t in zip(runs, (t1, t2)):
            ctx.fwd_set(t)
            r.plan(sync=False)
            want = F.plan(buf, off, ln, rec["reason"], t, 0)
            outs.append((r, t, want, r.build(cap_for(want), sync=False)))
        ctx.fwd_set(None)
        with pytest.raises(mosrx.MosrxError) as e:
            runs[0].plan(sync=False)
        assert e.value.errno == 2                                   # ENOENT
        mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")
        for r, t, want, (dev, init) in outs:
            np.testing.assert_array_equal(r.plan_result().view(np.uint64), want.view(np.uint64))
            exp = F.build(buf, off, want, t, cap_for(want), *init[:5])
            for d, i0, e0 in zip(dev[:5], init[:5], exp[:5]):
                np.testing.assert_array_equal(d.download(np.zeros_like(i0)), e0)
    finally:
        for r in runs:
            r.free()


def test_buffer_bounds(gpu_ctx):
    """tx_cap exactly what is needed, one unit less, half, 15 bytes short of a unit, and 0."""
    buf, off, ln = pack_at(base_frames(900), [2, 5])
    need = cap_for(F.plan(buf, off, ln, O.classify(buf, off, ln, O.params(num_msp=1, forward=1))["reason"],
                          mosrx.fwd_tables(**WALK), 0))
    check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), caps=(None, -16, -1, need // 2, 17, 0))


@pytest.mark.parametrize("name", ["conv_walk", "edge_walk", "conv_nicfwd"])
@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_mos_fixture(gpu_ctx, name, rec_bytes):
    """The frames mOS itself sent (tests/golden/fwd_plan.npz)."""
    z = np.load(os.path.join(GOLDEN, "fwd_plan.npz"))
    k = name + "__"
    t = mosrx.FwdTables.from_buffer_copy(z[k + "tables"].tobytes())
    buf, off, ln = z[k + "frames"], z[k + "off"], z[k + "len"]
    ctx = gpu_ctx
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1, local=["127.0.0.1"]))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(t)
    r = Run(ctx, buf, off, ln, rec_bytes)
    try:
        r.plan()
        np.testing.assert_array_equal(r.plan_result().view(np.uint64), z[k + "plan"].view(np.uint64))
        cap = (len(z[k + "tx"]) + 15) // 16 * 16
        dev, init = r.build(cap)
        m = len(z[k + "tx_off"])
        assert dev[5].download(np.zeros(2, np.uint32)).tolist() == [m, 0]
        got = [d.download(np.zeros_like(i0)) for d, i0 in zip(dev[:5], init[:5])]
        sent = F.tx_list(got[0], got[1], got[2], m)
        assert sent == F.tx_list(z[k + "tx"], z[k + "tx_off"], z[k + "tx_len"], m)
        for g, key in zip(got[1:], ("tx_off", "tx_len", "tx_nif", "tx_src")):
            np.testing.assert_array_equal(g[:m], z[k + key])
    finally:
        r.free()


@pytest.mark.parametrize("fix", ["edge", "rand_small", "rand_mid", "rand_large"])
@pytest.mark.parametrize("state", sorted(FSTATES))
def test_golden_frames_under_fstates(gpu_ctx, fix, state):
    z = np.load(os.path.join(GOLDEN, f"{fix}.npz"))
    msp, esp, loc, listen = FSTATES[state]
    check(gpu_ctx, z["frames"], z["off"], z["len"], mosrx.fwd_tables(**WALK), msp=msp, esp=esp, listener=listen,
          local=loc, rec_bytes=8 if state == "msp1" else 16)


def test_errors_launch_nothing(gpu_ctx):
    ctx = gpu_ctx
    buf, off, ln = pack_at(base_frames(100), [2])
    ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
    r = Run(ctx, buf, off, ln)
    L, b = mosrx.lib(), r.db.batch()
    import ctypes as C
    try:
        n = r.n
        bufs = [mosrx.DevBuffer(ctx, s) for s in (4096 * 4, n * 4, n * 2, n, n * 4, 8, 64)]
        r.bufs += bufs
        tx, toff, tlen, tnif, tsrc, cnt, scr = (x.ptr for x in bufs)
        bufs[5].upload(ee(2, np.uint32))
        r.d_plan.upload(ee(n + 1, np.uint64))
        ctx.fwd_set(None)
        assert L.mosrx_fwd_plan_dev(ctx.handle, C.byref(b), r.d_rec.ptr, 16, 0, r.d_plan.ptr, None) == -2
        assert L.mosrx_fwd_build_dev(ctx.handle, C.byref(b), r.d_plan.ptr, tx, 4096, toff, tlen, tnif, tsrc, cnt, scr,
                                     64, None) == -2
        ctx.fwd_set(mosrx.fwd_tables(**WALK))
        plan = lambda **kw: L.mosrx_fwd_plan_dev(ctx.handle, C.byref(b), kw.get("rec", r.d_rec.ptr), kw.get("rb", 16),
                                                 kw.get("ifi", 0), kw.get("plan", r.d_plan.ptr), None)
        assert plan(plan=r.d_plan.ptr + 4) == -22 and plan(plan=None) == -22 and plan(rec=r.d_rec.ptr + 8) == -22
        assert plan(rb=12) == -22 and plan(ifi=16) == -22 and plan(ifi=-1) == -22 and plan(rec=None) == -22
        build = lambda **kw: L.mosrx_fwd_build_dev(ctx.handle, C.byref(b), r.d_plan.ptr, kw.get("tx", tx), 4096,
                                                   kw.get("toff", toff), kw.get("tlen", tlen), tnif, tsrc,
                                                   kw.get("cnt", cnt), kw.get("scr", scr), kw.get("sb", 64), None)
        assert build(tx=tx + 8) == -22 and build(toff=toff + 2) == -22 and build(tlen=tlen + 1) == -22
        assert build(cnt=None) == -22 and build(scr=scr + 4) == -22 and build(sb=8) == -22 and build(tx=None) == -22
        assert L.mosrx_fwd_scratch_bytes(n) == 16 and L.mosrx_fwd_scratch_bytes(0) == 16
        assert L.mosrx_fwd_scratch_bytes(TILE + 1) == 32
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        assert (r.d_plan.download(np.zeros(n + 1, np.uint64)) == 0xEEEEEEEEEEEEEEEE).all()    # nothing ran
        assert (bufs[5].download(np.zeros(2, np.uint32)) == 0xEEEEEEEE).all()
        t = mosrx.fwd_tables(**WALK)
        t.num_routes = 129
        assert L.mosrx_fwd_set(ctx.handle, C.byref(t)) == -22
        t = mosrx.fwd_tables(**WALK)
        t.routes[1].nif = 4
        assert L.mosrx_fwd_set(ctx.handle, C.byref(t)) == -22
        t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 9}))
        assert L.mosrx_fwd_set(ctx.handle, C.byref(t)) == -22
        assert plan() == 0                                           # the tables of the last good set are still in
    finally:
        mosrx.lib().mosrx_sync(ctx.handle)
        r.free()
