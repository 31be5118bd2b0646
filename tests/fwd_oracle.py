"""numpy restatement of what mOS does with a frame it passes on (forward = 1).

Written from the reference's lines, not from the GPU path:
  * which frames are forwarded: the rule pinned to ProcessPacket by
    tests/golden/forward.npz (test_forwarding.py), restated here over reason codes;
  * ForwardEthernetFrame (core/src/eth_out.c:104-134): nic_forward_table or nothing;
  * ForwardIPPacket (core/src/ip_out.c:39-110): the nic_forward_table fast path,
    else GetOutputInterface (ip_out.c:11-37: from prefix -1, strictly greater
    wins) and GetDestinationHWaddr (arp.c:88-119: from prefix 0; an entry with
    prefix 1 compares the whole address, ends the walk and overrides an earlier
    longer match); no ARP request with forward = 1 (ip_out.c:69);
  * EthernetOutput (eth_out.c:62-102) + memcpy of ip_len bytes: h_dest, h_source
    = the output netdev's haddr, the ethertype, then the IP packet unchanged;
  * the library's TX layout: sent frame j at 16 k + 2, k the exclusive scan of
    ceil((2 + tx_len) / 16); a frame whose padded end passes tx_cap and every
    later one are dropped; nothing but frame bytes is written.
Both walks run over the tables' entries in order with the frames as vectors.
"""
import numpy as np

import mosrx

R = mosrx.R
NONE, IP, ETH, NO_ROUTE, NO_ARP, NO_NIC = range(6)


def forwards(reason, forward, num_msp, listener):
    """1 where mOS forwards a frame with this reason code (eth_in.c:60-77, ip_in.c:67-93, tcp.c:453-510)."""
    reason = np.asarray(reason)
    if not forward:
        return np.zeros(len(reason), bool)
    with_msp = np.isin(reason, [R["NON_IPV4"], R["ARP"], R["NOT_TCP"], R["TCP_BADCSUM"]]) & (num_msp != 0)
    tcp = np.isin(reason, [R["TCP_OK"], R["TCP_LEN_OK"]]) & (num_msp != 0) & (not listener)
    return with_msp | tcp | (reason == R["NOVERIFY_PASS"])


def tables_np(t):
    """A mosrx.FwdTables as numpy arrays (fields verbatim)."""
    nr, na, nd = t.num_routes, t.num_arp, t.num_netdevs
    return dict(
        r_mask=np.array([t.routes[i].mask for i in range(nr)], np.uint32),
        r_masked=np.array([t.routes[i].masked_ip for i in range(nr)], np.uint32),
        r_prefix=np.array([t.routes[i].prefix for i in range(nr)], np.int64),
        r_nif=np.array([t.routes[i].nif for i in range(nr)], np.int64),
        a_ip=np.array([t.arp[i].ip for i in range(na)], np.uint32),
        a_mask=np.array([t.arp[i].mask for i in range(na)], np.uint32),
        a_masked=np.array([t.arp[i].masked_ip for i in range(na)], np.uint32),
        a_prefix=np.array([t.arp[i].prefix for i in range(na)], np.int64),
        a_haddr=np.array([list(t.arp[i].haddr) for i in range(na)], np.uint8).reshape(na, 6),
        dev_haddr=np.array([list(t.netdev_haddr[i]) for i in range(nd)], np.uint8).reshape(nd, 6),
        has_nic_fwd=bool(t.has_nic_fwd), nic_fwd=np.array(list(t.nic_fwd), np.int64))


def get_output_interface(T, daddr):
    """ip_out.c:11-37 for a vector of daddr (raw u32 as mOS loads it): nif or -1."""
    nif = np.full(len(daddr), -1, np.int64)
    prefix = np.full(len(daddr), -1, np.int64)
    for i in range(len(T["r_mask"])):
        hit = ((daddr & T["r_mask"][i]) == T["r_masked"][i]) & (T["r_prefix"][i] > prefix)
        nif[hit] = T["r_nif"][i]
        prefix[hit] = T["r_prefix"][i]
    return nif


def get_destination_hwaddr(T, dip):
    """arp.c:88-119 for a vector of addresses: the entry's index or -1."""
    idx = np.full(len(dip), -1, np.int64)
    prefix = np.zeros(len(dip), np.int64)
    live = np.ones(len(dip), bool)           # the walk has not hit its break
    for i in range(len(T["a_ip"])):
        if T["a_prefix"][i] == 1:
            hit = live & (T["a_ip"][i] == dip)
            idx[hit] = i
            live &= ~hit
        else:
            hit = live & ((dip & T["a_mask"][i]) == T["a_masked"][i]) & (T["a_prefix"][i] > prefix)
            idx[hit] = i
            prefix[hit] = T["a_prefix"][i]
    return idx


def capture(off, ln, frames_bytes):
    """A frame's capture inside the batch buffer (include/mosrx.h, mosrx_batch.frames_bytes:
    no frame byte is read at or past it): min(len, max(frames_bytes - off, 0))."""
    room = np.maximum(int(frames_bytes) - np.asarray(off, np.uint32).astype(np.int64), 0)
    return np.minimum(np.asarray(ln, np.uint16).astype(np.int64), room)


def _field(frames, off, ln, at, nbytes):
    """Frame bytes at..at+nbytes per frame (zeros where the capture ends before them);
    `ln` is the capture, so no index passes the buffer."""
    out = np.zeros((len(off), nbytes), np.uint8)
    ok = np.asarray(ln).astype(np.int64) >= at + nbytes
    pos = off.astype(np.int64)[ok, None] + at + np.arange(nbytes)
    out[ok] = frames[pos]
    return out, ok


def plan(frames, off, ln, reason, t, in_ifidx, forward=1, num_msp=1, listener=False, frames_bytes=None):
    """One mosrx.FWD_DTYPE record per frame.  frames_bytes (default: the buffer's
    length) ends the batch buffer: a frame is what `capture` leaves of it."""
    T = tables_np(t)
    frames = np.asarray(frames, np.uint8)
    off = np.asarray(off, np.uint32)
    frames_bytes = len(frames) if frames_bytes is None else int(frames_bytes)
    assert 0 <= frames_bytes <= len(frames)
    ln = capture(off, ln, frames_bytes)
    n = len(off)
    out = np.zeros(n, mosrx.FWD_DTYPE)
    out["out_ifidx"] = -1
    out["arp_idx"] = 0xFFFF
    fwd = forwards(reason, forward, num_msp, listener) & (np.asarray(reason) != R["TRUNCATED"])
    eth = np.isin(reason, [R["NON_IPV4"], R["ARP"]])
    nicout = int(T["nic_fwd"][in_ifidx]) if T["has_nic_fwd"] else -1
    # ForwardEthernetFrame
    e = fwd & eth & (ln >= 14)
    if nicout == -1:
        out["kind"][e] = NO_NIC
    else:
        out["kind"][e] = ETH
        out["tx_len"][e] = ln[e].astype(np.uint16)
        out["out_ifidx"][e] = nicout
    # ForwardIPPacket
    tl, ok1 = _field(frames, off, ln, 16, 2)
    da, ok2 = _field(frames, off, ln, 30, 4)
    ip_len = tl[:, 0].astype(np.int64) * 256 + tl[:, 1]
    daddr = da.view("<u4")[:, 0]
    # (a forwarded IPv4 frame is never TRUNCATED / IP_SHORT: its packet lies inside the capture)
    p = fwd & ~eth & ok1 & ok2 & (ip_len >= 20) & (14 + ip_len <= ln)
    if nicout != -1:
        out["kind"][p] = IP
        out["out_ifidx"][p] = nicout
    else:
        nif = get_output_interface(T, daddr)
        arp = get_destination_hwaddr(T, daddr)
        noroute = p & (nif < 0)
        noarp = p & (nif >= 0) & (arp < 0)
        good = p & (nif >= 0) & (arp >= 0)
        out["kind"][noroute] = NO_ROUTE
        out["kind"][noarp] = NO_ARP
        out["out_ifidx"][noarp] = nif[noarp]
        out["kind"][good] = IP
        out["out_ifidx"][good] = nif[good]
        out["arp_idx"][good] = arp[good]
    sent_ip = out["kind"] == IP
    out["tx_len"][sent_ip] = (14 + ip_len[sent_ip]).astype(np.uint16)
    return out


def tx_frame(frames, o, pl, T):
    """The bytes mOS puts on the wire for one planned frame."""
    n = int(pl["tx_len"])
    src = frames[int(o):int(o) + n]
    if pl["kind"] == ETH:
        return src.copy()
    f = src.copy()
    if pl["arp_idx"] != 0xFFFF:
        f[0:6] = T["a_haddr"][int(pl["arp_idx"])]
    f[6:12] = T["dev_haddr"][int(pl["out_ifidx"])]
    return f


def build(frames, off, pl, t, tx_cap, tx_init, off_init, len_init, nif_init, src_init):
    """The TX run over copies of the given initial buffers:
    (tx_frames, tx_off, tx_len, tx_nif, tx_src, [m, dropped])."""
    T = tables_np(t)
    frames = np.asarray(frames, np.uint8)
    tx, toff, tlen, tnif, tsrc = (a.copy() for a in (tx_init, off_init, len_init, nif_init, src_init))
    k = m = dropped = 0
    full = False
    for i in np.nonzero(np.isin(pl["kind"], [IP, ETH]))[0]:
        units = (2 + int(pl["tx_len"][i]) + 15) // 16
        if full or (k + units) * 16 > tx_cap:
            full = True                    # offsets only grow: every later frame is dropped too
            dropped += 1
            k += units
            continue
        o = 16 * k + 2
        f = tx_frame(frames, off[i], pl[i], T)
        tx[o:o + len(f)] = f
        toff[m], tlen[m], tnif[m], tsrc[m] = o, len(f), pl["out_ifidx"][i], i
        m += 1
        k += units
    return tx, toff, tlen, tnif, tsrc, np.array([m, dropped], np.uint32)


def tx_list(tx, toff, tlen, m):
    return [bytes(tx[int(o):int(o) + int(n)]) for o, n in zip(toff[:m], tlen[:m])]
