"""numpy restatement of what samples/nat does to a frame ahead of forwarding.

Written from the sample's lines, not from the GPU path:
  * translate_addr (samples/nat/nat.c:91-155): on a TCP frame of a monitored flow
    two memcpy overwrites through mtcp_setlastpkt -- the source address and port
    become the NAT's (client side), or the destination address and port the
    client's (server side) -- and MOS_UPDATE_IP_CHKSUM | MOS_UPDATE_TCP_CHKSUM
    recompute both checks in full (mos_api.c:1179-1194): here oracle_py.tx_csum,
    which is pinned to mOS by tests/golden/tx_*.npz;
  * ForwardIPPacket then routes the translated packet: fwd_oracle.plan and
    fwd_rings_oracle.build on the translated frames;
  * which side a frame is on: the explicit bindings (include/mosrx.h).  A frame is
    eligible when its reason is TCP_OK, num_msp != 0, no listener, and its IPv4
    packet lies inside the capture; doff < 5 or a segment under 20 bytes is for
    the host (mtcp_setlastpkt refuses the port write, or the check word lies
    outside the segment); an eligible frame without a binding is a MISS.
MISS and HOST frames leave the plan with their own kinds (forward != 0).
"""
import numpy as np

import fwd_oracle as F
import mosrx
import oracle_py as O

R = mosrx.R
NONE, SNAT, DNAT, MISS, HOST = range(5)


def lookup_table(bindings):
    """{(saddr, daddr, ports): (kind, addr, port, index)} -- both keys of every binding."""
    tab = {}
    for i, b in enumerate(bindings):
        ck = (int(b["cli_ip"]), int(b["svr_ip"]), int(b["cli_port"]) | int(b["svr_port"]) << 16)
        sk = (int(b["svr_ip"]), int(b["nat_ip"]), int(b["svr_port"]) | int(b["nat_port"]) << 16)
        assert ck not in tab and sk not in tab and ck != sk
        tab[ck] = (SNAT, int(b["nat_ip"]), int(b["nat_port"]), i)
        tab[sk] = (DNAT, int(b["cli_ip"]), int(b["cli_port"]), i)
    return tab


def translate(frames, off, ln, reason, bindings, num_msp=1, listener=False, frames_bytes=None):
    """(xlat records, the translated copy of `frames`)."""
    frames = np.asarray(frames, np.uint8)
    off = np.asarray(off, np.uint32)
    fb = len(frames) if frames_bytes is None else int(frames_bytes)
    cap = F.capture(off, ln, fb)
    # what a load sees: the buffer up to its end rounded up to 16, zero behind it
    seen = np.concatenate([frames[:min((fb + 15) // 16 * 16, len(frames))], np.zeros(256, np.uint8)])
    tab = lookup_table(bindings)
    x = np.zeros(len(off), mosrx.NAT_XLAT_DTYPE)
    tr = frames.copy()
    done = []
    for i in np.nonzero((np.asarray(reason) == R["TCP_OK"]) & bool(num_msp) & (not listener) & (cap >= 34))[0]:
        o = int(off[i])
        ip_len = int(seen[o + 16]) * 256 + int(seen[o + 17])
        if ip_len < 20 or 14 + ip_len > cap[i]:
            continue
        ihl = int(seen[o + 14]) & 0xF
        th = o + 14 + 4 * ihl
        x[i]["ihl"], x[i]["bind"] = ihl, mosrx.NAT_NO_BIND
        if (int(seen[th + 12]) >> 4) < 5 or ip_len - 4 * ihl < 20:
            x[i]["kind"] = HOST
            continue
        key = tuple(int(seen[a:a + 4].view("<u4")[0]) for a in (o + 26, o + 30, th))
        if key not in tab:
            x[i]["kind"] = MISS
            continue
        kind, addr, port, idx = tab[key]
        # the sample's two overwrites
        tr[o + (26 if kind == SNAT else 30):][:4] = np.frombuffer(np.uint32(addr).tobytes(), np.uint8)
        tr[th + (0 if kind == SNAT else 2):][:2] = np.frombuffer(np.uint16(port).tobytes(), np.uint8)
        x[i]["kind"], x[i]["addr"], x[i]["port"], x[i]["bind"] = kind, addr, port, idx
        done.append(i)
    if done:
        d = np.array(done)
        tr = O.tx_csum(tr, off[d], cap[d].astype(np.uint16), mosrx.TX_IP_CSUM | mosrx.TX_TCP_CSUM)
        for i in done:
            o = int(off[i])
            x[i]["ip_check"] = tr[o + 24:o + 26].view("<u2")[0]
            x[i]["tcp_check"] = tr[o + 14 + 4 * int(x[i]["ihl"]) + 16:][:2].view("<u2")[0]
    return x, tr


def plan(frames, off, ln, reason, bindings, t, in_ifidx, forward=1, num_msp=1, listener=False, frames_bytes=None):
    """(xlat, plan, translated frames): ForwardIPPacket's plan over the translated frames,
    MISS / HOST frames taken out with their own kinds."""
    x, tr = translate(frames, off, ln, reason, bindings, num_msp, listener, frames_bytes)
    pl = F.plan(tr, off, ln, reason, t, in_ifidx, forward=forward, num_msp=num_msp, listener=listener,
                frames_bytes=frames_bytes)
    if forward:
        for kind, fk in ((MISS, mosrx.FWD_NAT_MISS), (HOST, mosrx.FWD_NAT_HOST)):
            m = x["kind"] == kind
            pl["kind"][m], pl["tx_len"][m], pl["out_ifidx"][m], pl["arp_idx"][m] = fk, 0, -1, 0xFFFF
    return x, pl, tr
