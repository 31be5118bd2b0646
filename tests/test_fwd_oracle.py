"""The forwarding restatement (tests/fwd_oracle.py) on the CPU: hand-worked cases
for each quirk of the two walks and of the TX layout, the committed fixture
(tests/golden/fwd_plan.npz, made from mOS's own tx.pcap), and -- where
oracle/_ref/mos_app_emul is built -- mOS itself again, live."""
import ctypes as C
import os

import numpy as np
import pytest

import fwd_oracle as F
import fwd_pin as P
import mosrx
from pktlib import R, pack_frames, tcp_frame

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def ip(a):
    return np.array([mosrx.ip_raw(a)], np.uint32)


def T(**kw):
    return F.tables_np(mosrx.fwd_tables(**kw))


def test_conf_masks_as_config_c():
    t = mosrx.fwd_tables(routes=[("10.1.2.3/8", 0), ("1.2.3.4/0", 0), ("1.2.3.4/32", 0)],
                         arp=[("192.168.7.9/20", "02:00:00:00:00:01")], netdevs=["02:00:00:00:00:aa"])
    assert (t.routes[0].mask, t.routes[0].masked_ip) == (0x000000FF, 0x0000000A)    # network order, LE host
    assert (t.routes[1].mask, t.routes[1].masked_ip) == (0, 0)
    assert (t.routes[2].mask, t.routes[2].masked_ip) == (0xFFFFFFFF, mosrx.ip_raw("1.2.3.4"))
    assert t.arp[0].mask == mosrx.conf_mask(20) == 0x00F0FFFF
    assert t.arp[0].masked_ip == mosrx.ip_raw("192.168.0.0") and t.arp[0].ip == mosrx.ip_raw("192.168.7.9")


def test_route_walk_quirks():
    assert F.get_output_interface(T(), ip("10.0.0.1"))[0] == -1                     # empty table: no route
    only0 = T(routes=[("0.0.0.0/0", 2)], netdevs=["02:00:00:00:00:01"] * 3)
    assert F.get_output_interface(only0, ip("8.8.8.8"))[0] == 2                      # from prefix -1: a /0 matches
    ties = T(routes=[("10.0.0.0/8", 1), ("10.0.0.0/8", 2), ("10.1.0.0/16", 0), ("10.1.0.0/16", 2)],
             netdevs=["02:00:00:00:00:01"] * 3)
    assert F.get_output_interface(ties, ip("10.2.0.1"))[0] == 1                      # first of equal prefixes kept
    assert F.get_output_interface(ties, ip("10.1.0.1"))[0] == 0
    assert F.get_output_interface(ties, ip("11.0.0.1"))[0] == -1


def test_arp_walk_quirks():
    t = T(arp=[("0.0.0.0/0", "02:00:00:00:00:00")])
    assert F.get_destination_hwaddr(t, ip("10.0.0.1"))[0] == -1                      # from prefix 0: a /0 never wins
    t = T(arp=[("10.0.0.0/8", "02:00:00:00:00:01"), ("10.1.0.0/16", "02:00:00:00:00:02"),
               ("10.1.2.3/1", "02:00:00:00:00:03"), ("10.1.2.3/32", "02:00:00:00:00:04")])
    assert F.get_destination_hwaddr(t, ip("10.1.2.3"))[0] == 2       # the prefix-1 entry ends the walk: the /32 is never seen
    assert F.get_destination_hwaddr(t, ip("10.1.2.4"))[0] == 1       # prefix 1 is an exact address, not a /1 mask
    assert F.get_destination_hwaddr(t, ip("10.9.9.9"))[0] == 0
    assert F.get_destination_hwaddr(t, ip("200.1.2.3"))[0] == -1     # (a /1 mask would have matched 128.0.0.0/1)
    t = T(arp=[("10.1.0.0/16", "02:00:00:00:00:01"), ("10.1.0.0/16", "02:00:00:00:00:02")])
    assert F.get_destination_hwaddr(t, ip("10.1.0.1"))[0] == 0


def frames3():
    """An IP frame padded past its packet, a non-IPv4 frame, a frame to an unknown address."""
    return [tcp_frame("10.0.0.1", "10.1.2.3", payload=b"abc", pad_to=80),
            tcp_frame(ethertype=0x86DD, payload=b"x", pad_to=61),
            tcp_frame("10.0.0.1", "99.1.2.3", payload=b"abcdef")]


def test_plan_and_layout_by_hand():
    fr = frames3()
    buf, off, ln = pack_frames(fr, phase=5)
    reason = np.array([R["TCP_OK"], R["NON_IPV4"], R["TCP_OK"]], np.uint8)
    t = mosrx.fwd_tables(routes=[("10.0.0.0/8", 1)], arp=[("10.1.0.0/16", "02:00:00:00:00:07")],
                         netdevs=["02:00:00:00:00:a0", "02:00:00:00:00:a1"])
    pl = F.plan(buf, off, ln, reason, t, 0)
    assert pl["kind"].tolist() == [F.IP, F.NO_NIC, F.NO_ROUTE]
    assert pl["tx_len"].tolist() == [14 + 43, 0, 0]                   # the IP length, not the 80 captured
    assert pl["out_ifidx"].tolist() == [1, -1, -1] and pl["arp_idx"].tolist() == [0, 0xFFFF, 0xFFFF]
    assert not pl["reserved"].any()
    # forward off, no monitor, a listener, TRUNCATED: nothing is forwarded
    assert not F.plan(buf, off, ln, reason, t, 0, forward=0)["kind"].any()
    assert not F.plan(buf, off, ln, reason, t, 0, num_msp=0)["kind"].any()
    assert F.plan(buf, off, ln, reason, t, 0, listener=True)["kind"].tolist() == [F.NONE, F.NO_NIC, F.NONE]
    assert not F.plan(buf, off, ln, np.full(3, R["TRUNCATED"], np.uint8), t, 0)["kind"].any()
    # with a nic_forward_table: the fast path keeps h_dest, non-IPv4 frames go out as captured
    tn = mosrx.fwd_tables(netdevs=["02:00:00:00:00:a0", "02:00:00:00:00:a1"], nic_fwd={0: 1})
    pn = F.plan(buf, off, ln, reason, tn, 0)
    assert pn["kind"].tolist() == [F.IP, F.ETH, F.IP] and pn["tx_len"].tolist() == [57, 61, 60]
    assert (pn["arp_idx"] == 0xFFFF).all() and (pn["out_ifidx"] == 1).all()
    assert F.plan(buf, off, ln, reason, tn, 1)["kind"].tolist() == [F.NO_ROUTE, F.NO_NIC, F.NO_ROUTE]   # entry -1
    # layout: 57 bytes -> 4 units, 61 -> 4, 60 -> 4
    cap = 12 * 16
    z = lambda n, d: np.frombuffer(b"\xEE" * (n * np.dtype(d).itemsize), d).copy()   # every byte 0xEE
    tx, toff, tlen, tnif, tsrc, cnt = F.build(buf, off, pn, tn, cap, z(cap + 16, np.uint8), z(3, np.uint32),
                                              z(3, np.uint16), z(3, np.int8), z(3, np.uint32))
    assert cnt.tolist() == [3, 0] and toff.tolist() == [2, 66, 130] and tsrc.tolist() == [0, 1, 2]
    f0 = bytes(tx[2:2 + 57])
    assert f0[0:6] == fr[0][0:6] and f0[6:12] == bytes.fromhex("0200000000a1") and f0[12:] == fr[0][12:57]
    assert bytes(tx[66:66 + 61]) == fr[1]                             # unchanged, source MAC included
    assert (tx[:2] == 0xEE).all() and (tx[59:66] == 0xEE).all() and (tx[190:] == 0xEE).all()   # padding untouched
    # one unit less: the last frame is dropped and counted, its slots untouched
    tx, toff, tlen, tnif, tsrc, cnt = F.build(buf, off, pn, tn, cap - 16, z(cap + 16, np.uint8), z(3, np.uint32),
                                              z(3, np.uint16), z(3, np.int8), z(3, np.uint32))
    assert cnt.tolist() == [2, 1] and toff[2] == 0xEEEEEEEE and (tx[127:] == 0xEE).all()
    assert F.build(buf, off, pn, tn, 0, z(16, np.uint8), z(3, np.uint32), z(3, np.uint16), z(3, np.int8),
                   z(3, np.uint32))[5].tolist() == [0, 3]
    # the ARP entry's haddr replaces h_dest on the walked path
    tx = F.build(buf, off, pl, t, cap, z(cap, np.uint8), z(3, np.uint32), z(3, np.uint16), z(3, np.int8),
                 z(3, np.uint32))[0]
    assert bytes(tx[2:14]) == bytes.fromhex("020000000007" "0200000000a1")


def test_rule_equals_library_rule():
    """forwards() against mosrx_mos_forwards (pinned to ProcessPacket by forward.npz)."""
    rec = np.zeros(mosrx.NREASON, mosrx.RESULT_DTYPE)
    rec["reason"] = np.arange(mosrx.NREASON)
    L = mosrx.lib()
    for fwd in (0, 1):
        for msp in (0, 1, 2):
            for listen in (0, 1):
                lib = [L.mosrx_mos_forwards(C.c_void_p(rec.ctypes.data + 16 * i), fwd, msp, listen)
                       for i in range(len(rec))]
                assert F.forwards(rec["reason"], fwd, msp, listen).astype(int).tolist() == lib


def load_golden():
    return np.load(os.path.join(GOLDEN, "fwd_plan.npz"))


def golden_tables(z, name):
    return mosrx.FwdTables.from_buffer_copy(z[name + "__tables"].tobytes())


@pytest.mark.parametrize("name", sorted(P.SCENARIOS))
def test_restatement_matches_fixture(name):
    """fwd_plan.npz holds mOS's own TX frames: the restatement reproduces them."""
    z = load_golden()
    k = name + "__"
    t = golden_tables(z, name)
    assert bytes(t) == bytes(P.tables(P.SCENARIOS[name][1]))
    pl = F.plan(z[k + "frames"], z[k + "off"], z[k + "len"], z[k + "reason"], t, 0)
    np.testing.assert_array_equal(pl, z[k + "plan"])
    n, m = len(pl), len(z[k + "tx_off"])
    cap = (len(z[k + "tx"]) + 15) // 16 * 16
    tx, toff, tlen, tnif, tsrc, cnt = F.build(z[k + "frames"], z[k + "off"], pl, t, cap, np.zeros(cap, np.uint8),
                                              np.zeros(n, np.uint32), np.zeros(n, np.uint16), np.zeros(n, np.int8),
                                              np.zeros(n, np.uint32))
    assert cnt.tolist() == [m, 0]
    np.testing.assert_array_equal(tx[:len(z[k + "tx"])], z[k + "tx"])
    for a, b in ((toff, "tx_off"), (tlen, "tx_len"), (tnif, "tx_nif"), (tsrc, "tx_src")):
        np.testing.assert_array_equal(a[:m], z[k + b])


def test_fixture_covers_the_walks():
    z = load_golden()
    kinds = np.bincount(z["conv_walk__plan"]["kind"], minlength=6) + np.bincount(z["edge_walk__plan"]["kind"], minlength=6)
    assert kinds[F.IP] > 100 and kinds[F.NO_ARP] > 0 and kinds[F.NO_NIC] > 0 and kinds[F.NONE] > 0
    used = set(z["conv_walk__plan"]["arp_idx"].tolist())
    assert {0, 1, 2, 3, 4} <= used and 5 not in used           # /8, /16, the prefix-1 entry, /24, /32; never the /0
    assert np.bincount(z["conv_nicfwd__plan"]["kind"], minlength=6)[F.ETH] > 0


def test_frames_bytes_default_changes_nothing():
    """frames_bytes left out is the buffer's length: every plan is what it was
    (mOS's own in fwd_plan.npz, the hand-worked one, the golden frame sets), and
    no descriptor of those sets, bogus ones included, makes _field index past the buffer."""
    z = load_golden()
    for name in sorted(P.SCENARIOS):
        k = name + "__"
        t = golden_tables(z, name)
        args = (z[k + "frames"], z[k + "off"], z[k + "len"], z[k + "reason"], t, 0)
        np.testing.assert_array_equal(F.plan(*args), z[k + "plan"])
        np.testing.assert_array_equal(F.plan(*args, frames_bytes=len(z[k + "frames"])), z[k + "plan"])
    buf, off, ln = pack_frames(frames3(), phase=5)
    reason = np.array([R["TCP_OK"], R["NON_IPV4"], R["TCP_OK"]], np.uint8)
    tn = mosrx.fwd_tables(netdevs=["02:00:00:00:00:a0", "02:00:00:00:00:a1"], nic_fwd={0: 1})
    for pl in (F.plan(buf, off, ln, reason, tn, 0), F.plan(buf, off, ln, reason, tn, 0, frames_bytes=len(buf))):
        assert pl["kind"].tolist() == [F.IP, F.ETH, F.IP] and pl["tx_len"].tolist() == [57, 61, 60]
    for fix in ("edge", "rand_small"):
        g = np.load(os.path.join(GOLDEN, f"{fix}.npz"))
        # frames inside the buffer: the capture is len[], the rule the restatement had before
        inside = g["off"].astype(np.int64) + g["len"] <= len(g["frames"])
        reason = np.where(inside, R["NON_IPV4"], R["TRUNCATED"]).astype(np.uint8)
        pl = F.plan(g["frames"], g["off"], g["len"], reason, tn, 0)
        np.testing.assert_array_equal(pl["tx_len"][inside & (g["len"] >= 14)], g["len"][inside & (g["len"] >= 14)])
        assert not pl["kind"][~inside].any()


def test_frames_bytes_by_hand():
    """Four descriptors over a 200-byte buffer that ends, for the batch, at byte 140:
    a 60-byte frame ending exactly there, one cut to 40 bytes, one starting at
    the end and one at 0xFFFFFFF0 (off + len wraps)."""
    ipb = bytes.fromhex("02d000000001" "025000000001" "0800") + \
        bytes.fromhex("4500002e" "00000000" "40fd0000" "0a000001" "0a010203") + bytes(26)   # tot_len 46, payload zeros
    assert len(ipb) == 60
    buf = np.full(200, 0xAB, np.uint8)
    buf[80:140] = np.frombuffer(ipb, np.uint8)
    off = np.array([80, 100, 140, 0xFFFFFFF0], np.uint32)
    ln = np.full(4, 60, np.uint16)
    np.testing.assert_array_equal(F.capture(off, ln, 140), [60, 40, 0, 0])
    np.testing.assert_array_equal(F.capture(off, ln, 139), [59, 39, 0, 0])
    tn = mosrx.fwd_tables(netdevs=["02:00:00:00:00:a0", "02:00:00:00:00:a1"], nic_fwd={0: 1})
    eth = np.full(4, R["NON_IPV4"], np.uint8)
    tcp = np.full(4, R["TCP_OK"], np.uint8)
    # the same answers from frames_bytes = 140 and from a buffer that is 140 bytes long
    for fr, kw in ((buf, dict(frames_bytes=140)), (buf[:140], {})):
        pl = F.plan(fr, off, ln, eth, tn, 0, **kw)
        assert pl["kind"].tolist() == [F.ETH, F.ETH, F.NONE, F.NONE]
        assert pl["tx_len"].tolist() == [60, 40, 0, 0] and pl["out_ifidx"].tolist() == [1, 1, -1, -1]
        # as IPv4: the whole packet (14 + 46) lies inside the first capture; the second
        # reads tot_len 0 from the first's payload: not a packet
        pl = F.plan(fr, off, ln, tcp, tn, 0, **kw)
        assert pl["kind"].tolist() == [F.IP, F.NONE, F.NONE, F.NONE] and pl["tx_len"].tolist() == [60, 0, 0, 0]
    # one byte less: the packet passes the capture (whatever the record says); as Ethernet it goes out cut
    assert not F.plan(buf, off, ln, tcp, tn, 0, frames_bytes=139)["kind"].any()
    pl = F.plan(buf, off, ln, eth, tn, 0, frames_bytes=139)
    assert pl["kind"].tolist() == [F.ETH, F.ETH, F.NONE, F.NONE] and pl["tx_len"].tolist() == [59, 39, 0, 0]
    # a capture under an Ethernet header is not forwarded: 80 + 13, and nothing at all
    assert F.plan(buf, off, ln, eth, tn, 0, frames_bytes=93)["kind"].tolist() == [F.NONE] * 4
    assert F.plan(buf, off, ln, eth, tn, 0, frames_bytes=94)["tx_len"].tolist() == [14, 0, 0, 0]
    assert not F.plan(buf, off, ln, eth, tn, 0, frames_bytes=0)["kind"].any()
    # the TX bytes of the cut frame are the captured ones only
    z = lambda n, d: np.frombuffer(b"\xEE" * (n * np.dtype(d).itemsize), d).copy()
    tx, toff, tlen, tnif, tsrc, cnt = F.build(buf, off, pl, tn, 128, z(128, np.uint8), z(4, np.uint32), z(4, np.uint16),
                                              z(4, np.int8), z(4, np.uint32))
    assert cnt.tolist() == [2, 0] and toff[:2].tolist() == [2, 66] and tlen[:2].tolist() == [59, 39]
    assert bytes(tx[2:61]) == ipb[:59] and bytes(tx[66:105]) == ipb[20:59] and (tx[105:] == 0xEE).all()


@pytest.mark.skipif(not os.access(P.APP, os.X_OK), reason="needs oracle/_ref/mos_app_emul (make -C oracle ref)")
@pytest.mark.parametrize("name", sorted(P.SCENARIOS))
def test_restatement_matches_mos(tmp_path, name):
    kind, nicfwd = P.SCENARIOS[name]
    frames = P.scenario_frames(kind)
    tx = P.restated(frames, nicfwd)[5]
    mos = P.run_mos(tmp_path, name, frames, nicfwd)
    assert len(mos) == len(tx) and mos == tx
