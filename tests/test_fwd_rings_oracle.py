"""The restatement of the ring build (tests/fwd_rings_oracle.py) pinned to what is
already pinned: with nrings = num_netdevs and caps that drop nothing, ring q
holds exactly the frames of fwd_oracle.build's arrival-order run whose tx_nif
is q, in order, byte for byte -- and for tests/golden/fwd_plan.npz those are
mOS's own tx.pcap frames.  Then the drop rule and the scratch size (no GPU)."""
import os

import numpy as np
import pytest

import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
import oracle_py as O
from test_fwd_gpu import DEVS4, DSTS, WALK, ee, ip_frame, pack_at
from test_oracle_golden import GOLDEN

DEVS16 = [f"02:00:00:00:bb:{i:02x}" for i in range(16)]
NET16 = dict(routes=[(f"10.{q}.0.0/16", q) for q in range(16)], arp=[("10.0.0.0/8", "02:00:00:00:00:77")],
             netdevs=DEVS16)


def walk4_input():
    fr = [ip_frame(DSTS[i % len(DSTS)], 20 + (i * 37) % 240, pad=(i % 5) * 3, ok=i % 3 != 1, seed=i) for i in range(700)]
    return pack_at(fr, [2, 7, 0, 13]), mosrx.fwd_tables(**WALK)


def net16_input():
    fr = [ip_frame(f"10.{(i * 7) % 16}.{i % 200}.9", 20 + (i * 29) % 300, pad=i % 4, ok=i % 5 != 4, seed=i)
          for i in range(900)]
    return pack_at(fr, [2, 9]), mosrx.fwd_tables(**NET16)


def planned(buf, off, ln, t):
    rec = O.classify(buf, off, ln, O.params(num_msp=1, forward=1))
    return F.plan(buf, off, ln, rec["reason"], t, 0, forward=1, num_msp=1)


def arrival_run(buf, off, pl, t):
    n = len(off)
    cap = int(FR.units_of(pl)[np.isin(pl["kind"], [F.IP, F.ETH])].sum()) * 16
    tx, toff, tlen, tnif, tsrc, cnt = F.build(buf, off, pl, t, cap, ee(cap + 64, np.uint8), ee(n + 8, np.uint32),
                                              ee(n + 8, np.uint16), ee(n + 8, np.int8), ee(n + 8, np.uint32))
    assert int(cnt[1]) == 0
    m = int(cnt[0])
    return F.tx_list(tx, toff, tlen, m), tnif[:m], tsrc[:m]


def rings_run(buf, off, pl, t, nrings, ring_cap):
    n = len(off)
    return FR.build(buf, off, pl, t, ring_cap, nrings, ee(nrings * ring_cap + 64, np.uint8), ee(n + 8, np.uint32),
                    ee(n + 8, np.uint16), ee(n + 8, np.uint32), ee(nrings + 2, mosrx.FWD_RING_DTYPE))


def assert_rings_equal_run(buf, off, pl, t):
    nrings = t.num_netdevs
    frames, tnif, tsrc = arrival_run(buf, off, pl, t)
    need = FR.need_units(pl, nrings)
    cap = int(need.max()) * 16
    tx, toff, tlen, rsrc, rings = rings_run(buf, off, pl, t, nrings, cap)
    start = 0
    for q in range(nrings):
        sel = np.nonzero(tnif == q)[0]
        assert rings[q].tolist() == (start, len(sel), 0, int(need[q]))
        assert FR.ring_list(tx, toff, tlen, rings, q) == [frames[i] for i in sel]
        assert rsrc[start:start + len(sel)].tolist() == tsrc[sel].tolist()
        a = toff[start:start + len(sel)].astype(np.int64)
        assert ((a >= q * cap) & (a + tlen[start:start + len(sel)] <= q * cap + 16 * int(need[q]))).all()
        start += len(sel)
    assert start == len(frames)
    assert (toff[start:] == 0xEEEEEEEE).all() and (rings[nrings:].view(np.uint8) == 0xEE).all()
    return rings


def test_rings_equal_arrival_run_4_netdevs():
    (buf, off, ln), t = walk4_input()
    rings = assert_rings_equal_run(buf, off, planned(buf, off, ln, t), t)
    assert (rings["count"][:4] > 0).all()                 # no ring empty: the input reaches every netdev


def test_rings_equal_arrival_run_16_netdevs():
    (buf, off, ln), t = net16_input()
    rings = assert_rings_equal_run(buf, off, planned(buf, off, ln, t), t)
    assert (rings["count"][:16] > 0).all()                # all 16 rings reached


@pytest.mark.parametrize("name", ["conv_walk", "edge_walk", "conv_nicfwd"])
def test_rings_equal_mos_fixture(name):
    """fwd_plan.npz: one netdev, so ring 0 is mOS's own tx.pcap list."""
    z = np.load(os.path.join(GOLDEN, "fwd_plan.npz"))
    k = name + "__"
    t = mosrx.FwdTables.from_buffer_copy(z[k + "tables"].tobytes())
    buf, off, pl = z[k + "frames"], z[k + "off"], z[k + "plan"].view(mosrx.FWD_DTYPE).reshape(-1)
    assert_rings_equal_run(buf, off, pl, t)
    m = len(z[k + "tx_off"])
    assert set(z[k + "tx_nif"].tolist()) <= {0}
    cap = (len(z[k + "tx"]) + 15) // 16 * 16
    tx, toff, tlen, rsrc, rings = rings_run(buf, off, pl, t, t.num_netdevs, cap)
    assert rings[0].tolist()[:3] == (0, m, 0)
    assert FR.ring_list(tx, toff, tlen, rings, 0) == F.tx_list(z[k + "tx"], z[k + "tx_off"], z[k + "tx_len"], m)
    np.testing.assert_array_equal(rsrc[:m], z[k + "tx_src"])


@pytest.mark.parametrize("make", [walk4_input, net16_input])
def test_drop_rule(make):
    """One unit under the fullest ring's need: exactly that ring drops, from the
    first frame that does not fit onward; every other ring is complete."""
    (buf, off, ln), t = make()
    pl = planned(buf, off, ln, t)
    nrings = t.num_netdevs
    need = FR.need_units(pl, nrings)
    full = int(np.argmax(need))
    assert (need == need[full]).sum() == 1
    cap = (int(need[full]) - 1) * 16
    whole = rings_run(buf, off, pl, t, nrings, int(need[full]) * 16)
    tx, toff, tlen, rsrc, rings = rings_run(buf, off, pl, t, nrings, cap)
    for q in range(nrings):
        w = whole[4][q]
        assert rings[q]["start"] == w["start"]
        if q != full:
            assert rings[q].tolist() == w.tolist()
            assert FR.ring_list(tx, toff, tlen, rings, q) == FR.ring_list(*whole[:3], whole[4], q)
            continue
        # the ring's frames in order: the first whose padded end passes the cap, and all after it, are dropped
        mine = np.nonzero(FR.sent_mask(pl, nrings) & (pl["out_ifidx"] == q))[0]
        ends = np.cumsum(FR.units_of(pl)[mine]) * 16
        first = int(np.argmax(ends > cap))
        assert ends[first] > cap and (ends[:first] <= cap).all()
        assert rings[q].tolist() == (int(w["start"]), first, len(mine) - first, int(ends[first - 1]) // 16)
        assert FR.ring_list(tx, toff, tlen, rings, q) == FR.ring_list(*whole[:3], whole[4], q)[:first]
        a = int(w["start"])
        assert (toff[a + first:a + len(mine)] == 0xEEEEEEEE).all() and (rsrc[a + first:a + len(mine)] == 0xEEEEEEEE).all()
        assert (tx[q * cap + int(ends[first - 1]):(q + 1) * cap] == 0xEE).all()


def test_scratch_bytes_needs_no_context():
    L = mosrx.lib()
    f = L.mosrx_fwd_rings_scratch_bytes
    ns = [0, 1, 255, 256, 257, 5003, 65536, 1 << 24, 0xFFFFFFFF]
    qs = [0, 1, 2, 4, 15, 16, 17, 0xFFFFFFFF]
    v = np.array([[f(n, q) for q in qs] for n in ns], np.uint64)
    assert (v > 0).all() and (v % 16 == 0).all()
    assert (np.diff(v.astype(np.int64), axis=0) >= 0).all() and (np.diff(v.astype(np.int64), axis=1) >= 0).all()
    assert f(0, 1) == 16 and f(256, 4) == 64 and f(257, 4) == 128 and f(5003, 16) == 20 * 16 * 16
    assert f(100, 1) == L.mosrx_fwd_scratch_bytes(100)
