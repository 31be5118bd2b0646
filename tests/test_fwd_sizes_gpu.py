"""Forwarding at the batch sizes it is timed at, at the end of the batch buffer
and over hostile descriptors: what the other forwarding tests cannot reach,
because their largest batch has 5,003 frames (20 tiles of MOSRX_FWD_TILE = 256),
their frame buffer always ends in 64 spare bytes and their descriptors are sane.

  * the ring build's scan (mosrx_fwd_rings_body.inc, FWD_BODY == 2, single-batch
    and queue kernels) gives each lane per = ceil(tiles / 64) tiles:
        n = 64 * 256 + 1  = 16385   65 tiles, per 2: lanes 0..31 own 2, lane 32 one
        n = 129 * 256 + 5 = 33029  130 tiles, per 3: lanes 0..42 own 3, lane 43 one
  * mosrx_fwd_scan_kernel (arrival-order build) gives each of 1024 lanes
    per = ceil(tiles / 1024) tiles:
        n = 1026 * 256 + 1 = 262657  1027 tiles, per 2: lanes 0..512 own 2, lane 513 one
  * the queue forms' batch lookup (fwd_queue_batch) over 40 batches: 6 steps.

Expected values are the restatements' (fwd_oracle.plan on oracle_py.classify's
reasons, fwd_oracle.build, fwd_rings_oracle.build), written into copies of the
same 0xEE images the GPU writes into and compared exactly, canaries and padding
included.  They never come from the GPU."""
import numpy as np
import pytest

import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_fwd_gpu import DEVS4, DSTS, TILE, WALK, cap_for, check, eth_frame, ip_frame, pack_at
from test_fwd_queue_gpu import run_caps
from test_fwd_rings_gpu import RingRun, assert_same, caps_of, download
from test_fwd_rings_gpu import check as check_rings
from test_fwd_rings_oracle import NET16

pytestmark = pytest.mark.gpu

BLOCK = 4099          # distinct frames per block: a prime, so block and tile edges never line up
N_RING = (64 * TILE + 1, 129 * TILE + 5)
N_ARRIVAL = 1026 * TILE + 1
SHARE = 8             # one frame in SHARE is forwarded (the others fail the IP checksum)
SHARE_BIG = 16        # ... in the batch of N_ARRIVAL frames: fwd_oracle.build's loop is per sent frame
_blocks = {}


def block(kind, share=SHARE):
    """BLOCK short IPv4 frames (tot_len 20..60, 0..3 trailing bytes), one in `share`
    forwarded; the forwarded ones go round the destinations of WALK's four
    netdevs ("walk") or of NET16's sixteen ("net16") within every tile."""
    if (kind, share) not in _blocks:
        dst = (lambda i: DSTS[(i // share) % len(DSTS)]) if kind == "walk" else \
            (lambda i: f"10.{(i // share) % 16}.3.{i % 250}")
        _blocks[kind, share] = [ip_frame(dst(i), 20 + (i * 37) % 41, pad=i % 4, ok=i % share == 3, seed=i)
                                for i in range(BLOCK)]
    return _blocks[kind, share]


def frames_of(kind, n, first=0):
    """n frames from the block, the last one forwarded: the ragged last tile's scratch row is not zero."""
    b = block(kind)
    fr = [b[(first + i) % BLOCK] for i in range(n)]
    if n:
        fr[-1] = ip_frame("10.1.2.3", 40, seed=n)
    return fr


def scan_runs(tiles, lanes):
    """Tiles owned per lane of a scan kernel (the kernels' own formulas)."""
    per = -(-tiles // lanes)
    return [min(l * per + per, tiles) - min(l * per, tiles) for l in range(lanes)]


def test_sizes_reach_the_branches():
    assert mosrx.lib().mosrx_fwd_tile() == TILE
    r = scan_runs(-(-N_RING[0] // TILE), 64)
    assert r[:32] == [2] * 32 and r[32] == 1 and not any(r[33:])
    r = scan_runs(-(-N_RING[1] // TILE), 64)
    assert r[:43] == [3] * 43 and r[43] == 1 and not any(r[44:])
    r = scan_runs(-(-N_ARRIVAL // TILE), 1024)
    assert r[:513] == [2] * 513 and r[513] == 1 and not any(r[514:])


def rings_per_tile(want, nrings):
    """Per full tile: how many rings get a sent frame of it."""
    s = FR.sent_mask(want, nrings) & (np.arange(len(want)) < len(want) // TILE * TILE)
    tiles = len(want) // TILE
    hit = np.zeros((tiles, nrings), bool)
    i = np.nonzero(s)[0]
    hit[i // TILE, want["out_ifidx"][i].astype(np.int64)] = True
    return hit.sum(axis=1)


@pytest.mark.parametrize("n,rec_bytes", [(N_RING[0], 16), (N_RING[0], 8), (N_RING[1], 16)])
@pytest.mark.parametrize("net", ["walk", "net16"])
def test_ring_build_one_batch(gpu_ctx, net, n, rec_bytes):
    """65 and 130 tiles into 4 rings (WALK) and 16 rings (NET16), the cap exactly the
    fullest ring's need and one unit less."""
    tables, nrings = (mosrx.fwd_tables(**WALK), 4) if net == "walk" else (mosrx.fwd_tables(**NET16), 16)
    buf, off, ln = pack_at(frames_of(net, n), [2, 7, 0, 13])
    want, rings = check_rings(gpu_ctx, buf, off, ln, tables, nrings=nrings, rec_bytes=rec_bytes,
                              caps=("exact", "minus16"))
    # every full tile's scratch row matters in at least two columns, and the ragged last tile's (1 or 5 frames) in one
    assert rings_per_tile(want, nrings).min() >= 2 and FR.sent_mask(want, nrings)[-1]
    assert (rings["count"][:nrings] > 0).all() and (rings["dropped"][:nrings] == 0).all()
    assert n // SHARE // 2 < int(rings["count"][:nrings].sum()) <= n // SHARE + 2


def tiled_batch(n, share):
    """n frames as repeats of one packed block of BLOCK frames (np.tile), the offsets shifted."""
    bbuf, boff, bln = pack_at(block("walk", share), [2, 7, 0, 13])
    body = bbuf[:-64]                                     # pack_at's spare bytes
    step = (len(body) + 15) // 16 * 16
    body = np.concatenate([body, np.zeros(step - len(body), np.uint8)])
    reps = -(-n // BLOCK)
    off = (np.arange(reps, dtype=np.int64)[:, None] * step + boff[None, :].astype(np.int64)).ravel()[:n]
    ln = np.tile(bln, reps)[:n]
    buf = np.concatenate([np.tile(body, reps)[:int(off[-1]) + int(ln[-1])], np.zeros(64, np.uint8)])
    assert len(buf) < 1 << 31
    return buf, off.astype(np.uint32), ln


def test_arrival_build_over_262144_frames(gpu_ctx):
    """1027 tiles: mosrx_fwd_scan_kernel's lanes own two tiles each.  tx_cap exactly
    what is needed and 16 bytes less; every TX array and tx_count as test_fwd_gpu.check compares them."""
    buf, off, ln = tiled_batch(N_ARRIVAL, SHARE_BIG)
    want = check(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**WALK), caps=(None, -16))
    sent = np.isin(want["kind"], [F.IP, F.ETH])
    per_tile = np.bincount(np.nonzero(sent)[0] // TILE, minlength=1027)
    assert per_tile[:1026].min() >= 8 and len(per_tile) == 1027   # no full tile's scratch row is zero (the last tile holds one frame)
    assert N_ARRIVAL // SHARE_BIG // 2 < sent.sum() <= N_ARRIVAL // SHARE_BIG + 1


def queue_sizes():
    ns = [0, 1, 255, 256, 257, N_RING[0], 0, 700, N_RING[1], 0] + [1 + (i * 53) % 300 for i in range(29)] + [0]
    assert len(ns) == 40
    return ns


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_queue_of_40_batches(gpu_ctx, rec_bytes):
    """40 batches, the 65-tile and the 130-tile one among them behind non-zero
    tile bases, empty ones first, in the middle and last; in_ifidx alternates
    between 0 (nic_fwd: everything to netdev 2) and 1 (the walk)."""
    ns = queue_sizes()
    batches = [pack_at(frames_of("walk", n, first=37 * k), [2, 7, 0, 13]) for k, n in enumerate(ns)]
    ifs = [k % 2 for k in range(len(ns))]
    t = mosrx.fwd_tables(**dict(WALK, nic_fwd={0: 2}))
    want, rings = run_caps(gpu_ctx, batches, t, 4, in_ifidx=ifs, rec_bytes=rec_bytes)
    assert [int(r["count"][:4].sum()) for r in rings] == [int(FR.sent_mask(w, 4).sum()) for w in want]
    assert ns[5] == N_RING[0] and ifs[5] == 1 and rings_per_tile(want[5], 4).min() >= 2
    assert ns[8] == N_RING[1] and ifs[8] == 0 and rings[8]["count"][:4].tolist()[:2] == [0, 0] and rings[8]["count"][2] > 4000
    assert sum(int(r["count"][:4].sum()) > 0 for r in rings) >= 20


def run_all(ctx, buf, off, ln, tables, msp=1, rec_bytes=16, frames_bytes=None, caps=(None,), ring_caps=("exact",)):
    """Classify, plan, arrival-order build and ring build of one batch whose buffer
    ends, for the library, at frames_bytes: each equal to the restatement.
    caps: None (exactly what is needed) or "half".  Returns (records, plan) of the restatement."""
    fb = len(buf) if frames_bytes is None else frames_bytes
    ctx.set_params(mosrx.default_params(num_msp=msp, forward=1))
    ctx.fwd_set_listener(False)
    ctx.fwd_set(tables)
    rec = O.classify(buf[:fb], off, ln, O.params(num_msp=msp, forward=1))
    want = F.plan(buf, off, ln, rec["reason"], tables, 0, forward=1, num_msp=msp, frames_bytes=fb)
    nrings = tables.num_netdevs
    r = RingRun(ctx, buf, off, ln, rec_bytes, frames_bytes=fb)
    try:
        if rec_bytes == 16:
            assert r.db.results().tobytes() == rec.tobytes(), "records"
        r.plan(0)
        got = r.plan_result()
        bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
        assert not len(bad), [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]]
        need = cap_for(want)
        for cap in caps:
            cap = need if cap is None else need // 2
            dev, init = r.build(cap)
            exp = F.build(buf, off, want, tables, cap, *init[:5])
            cnt = init[5].copy()
            cnt[:2] = exp[5]
            for name, d, i0, e in zip(("tx_frames", "tx_off", "tx_len", "tx_nif", "tx_src", "tx_count"), dev, init,
                                      list(exp[:5]) + [cnt]):
                g = d.download(np.zeros_like(i0))
                diff = np.nonzero(g != e)[0]
                assert not len(diff), (name, cap, len(diff), diff[:8].tolist(), g[diff[:8]].tolist(), e[diff[:8]].tolist())
        for cap in caps_of(FR.need_units(want, nrings), ring_caps):
            dev, init = r.build_rings(cap, nrings)
            assert_same(download(dev, init), FR.build(buf, off, want, tables, cap, nrings, *init), ("ring cap", cap))
        return rec, want
    finally:
        r.free()


def end_batch(kind, a, m):
    """Two frames, the second at off % 16 == a with tx_len % 16 == m, the last
    thing in the buffer: an IPv4 frame that ends with its packet ("ip") or a
    non-IPv4 frame of 14..29 bytes ("eth")."""
    f1 = ip_frame("192.168.1.7", 20 + (m - 34) % 16, seed=m) if kind == "ip" else eth_frame(14 + (m - 14) % 16, a)
    buf, off, ln = pack_at([ip_frame("10.1.2.3", 77, seed=a), f1], [2, a])
    end = int(off[1]) + int(ln[1])
    assert int(off[1]) % 16 == a and int(ln[1]) % 16 == m
    return buf[:end].copy(), off, ln


@pytest.mark.parametrize("short", [0, 1, 3, 17])
@pytest.mark.parametrize("kind", ["ip", "eth"])
def test_buffer_end(gpu_ctx, kind, short):
    """Every (off % 16, tx_len % 16) of a frame that is the last thing in the
    uploaded buffer, frames_bytes its end (no byte is lost) and 1, 3 and 17
    bytes before it (no byte past frames_bytes goes out: the cut IPv4 frame is
    not forwarded, the cut Ethernet frame goes out as captured)."""
    tables = mosrx.fwd_tables(**WALK) if kind == "ip" else mosrx.fwd_tables(netdevs=DEVS4, nic_fwd={0: 1})
    cut_sent = 0
    for a in range(16):
        for m in range(16):
            buf, off, ln = end_batch(kind, a, m)
            fb = len(buf) - short
            rec, want = run_all(gpu_ctx, buf, off, ln, tables, frames_bytes=fb)
            assert want["kind"][0] == F.IP and want["tx_len"][0] == 14 + 77
            left = int(ln[1]) - short
            if short == 0:
                assert want["kind"][1] == (F.IP if kind == "ip" else F.ETH) and want["tx_len"][1] == ln[1]
            elif kind == "ip" or left < 14:
                assert want["kind"][1] == F.NONE and want["tx_len"][1] == 0
            else:
                assert want["kind"][1] == F.ETH and want["tx_len"][1] == left
                cut_sent += 1
    if kind == "eth":
        assert cut_sent == {0: 0, 1: 16 * 15, 3: 16 * 13, 17: 0}[short]


_hostile = {}
HOSTILE_TABLES = {"walk": WALK, "nic_fwd": dict(netdevs=DEVS4, nic_fwd={0: 2})}


def hostile():
    """test_parity_gpu.test_random_offsets_and_garbage's buffer and descriptors
    (300,000 random bytes, 5,000 random descriptors, every second one made to look
    like IPv4) and test_bogus_offsets_after_sorted_frames' three entries behind
    them: past the end, 0xFFFF0000, and zero length at 0xFFFFFFF0."""
    if not _hostile:
        rng = np.random.default_rng(11)
        buf = rng.integers(0, 256, 300_000, dtype=np.uint8)
        n = 5000
        off = rng.integers(0, len(buf), n).astype(np.uint32)
        ln = rng.integers(0, 2000, n).astype(np.uint16)
        for i in range(0, n, 2):
            o = int(off[i])
            if o + 40 < len(buf):
                buf[o + 12:o + 14] = (0x08, 0x00)
                buf[o + 14] = 0x40 | rng.integers(0, 16)
                tl = int(rng.integers(0, 1600))
                buf[o + 16:o + 18] = (tl >> 8, tl & 0xFF)
                buf[o + 23] = 6 if rng.random() < 0.8 else 17
        off = np.concatenate([off, np.array([len(buf) + 5, 0xFFFF0000, 0xFFFFFFF0], np.uint32)])
        ln = np.concatenate([ln, np.array([1500, 1500, 0], np.uint16)])
        _hostile["in"] = (buf, off, ln)
    return _hostile["in"]


def test_hostile_input_is_useful():
    """The restatement's own output over the hostile descriptors.  A refusal's
    reason is the plan's kind (NO_ROUTE, NO_ARP, NO_NIC) or, for a frame the rule
    does not forward, its record's reason code: every setting has two reasons
    with 50 frames or more.  Frames are sent where there is a way out: with the
    nic_forward_table always; under the walk random destination addresses almost
    never have an ARP entry (NO_ARP), and non-IPv4 frames have no netdev (NO_NIC),
    so those settings are about the refusals."""
    buf, off, ln = hostile()
    sent_of = {}
    for msp in (1, 0):
        rec = O.classify(buf, off, ln, O.params(num_msp=msp, forward=1))
        for name, kw in HOSTILE_TABLES.items():
            pl = F.plan(buf, off, ln, rec["reason"], mosrx.fwd_tables(**kw), 0, forward=1, num_msp=msp)
            assert not pl["kind"][-3:].any()                       # the three bogus entries
            sent = np.isin(pl["kind"], [F.IP, F.ETH])
            why = np.where(pl["kind"] == F.NONE, rec["reason"].astype(np.int64), 100 + pl["kind"].astype(np.int64))
            reasons = np.bincount(why[~sent])
            assert (reasons >= 50).sum() >= 2, (msp, name, reasons.tolist())
            sent_of[msp, name] = int(sent.sum())
    assert sent_of[1, "nic_fwd"] >= 50 and sent_of[0, "nic_fwd"] >= 50
    assert sum(sent_of.values()) >= 50 and sent_of[0, "walk"] > 0


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("tables", sorted(HOSTILE_TABLES))
@pytest.mark.parametrize("msp", [1, 0])
def test_hostile_descriptors(gpu_ctx, msp, tables, rec_bytes):
    """Random and overlapping offsets, offsets past the buffer, zero lengths: plan,
    arrival-order build (tx_cap exact and half) and ring build (cap exact and half)."""
    buf, off, ln = hostile()
    try:
        run_all(gpu_ctx, buf, off, ln, mosrx.fwd_tables(**HOSTILE_TABLES[tables]), msp=msp, rec_bytes=rec_bytes,
                caps=(None, "half"), ring_caps=("exact", "half"))
    finally:
        gpu_ctx.set_params(mosrx.default_params())
