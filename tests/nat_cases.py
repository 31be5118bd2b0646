"""The NAT tests' shared trace: bindings, forwarding tables and a mixed batch.

Per 25 frames: 20 of established flows (SNAT and DNAT alternating; plain, behind
IP options of ihl 6 and 15, with TCP options, with payloads of odd and even
length; some from the 16 bindings whose client-side keys share one slot; DNATs
whose client has no ARP entry), one TCP frame of an unknown flow (MISS), one with
doff 4 and one with a 12-byte segment (HOST; the latter needs its record forced
to TCP_OK: the classify pass calls it TCP_SHORT), one with a bad TCP checksum, and
one that is UDP or ARP.  So 20 of every 24 TCP frames are translated.
"""
import numpy as np

import mosrx
from pktlib import tcp_frame

NAT_IP = "192.0.2.1"
DEVS4 = [f"02:00:00:00:aa:{i:02x}" for i in range(4)]
# clients 10/8 behind netdev 1, the NAT's own net on netdev 0, servers on netdev 2; 172.16/12 routes to 3 without ARP
TABLES = dict(routes=[("10.0.0.0/8", 1), ("192.0.2.0/24", 0), ("198.51.100.0/24", 2), ("172.16.0.0/12", 3)],
              arp=[("10.0.0.0/8", "02:00:00:00:00:01"), ("192.0.2.0/24", "02:00:00:00:00:02"),
                   ("198.51.100.0/24", "02:00:00:00:00:03")], netdevs=DEVS4)
NPLAIN, NCOLL, NNOARP = 40, 16, 8
NBIND = NPLAIN + NCOLL + NNOARP          # 64 bindings: a table of 256 slots

_cache = {}


def flows():
    """[(cli_ip, cli_port, svr_ip, svr_port, nat_port)]: 40 plain, 16 whose client-side keys
    mosrx_nat_hash sends to one slot of the 256, 8 whose client has a route but no ARP entry."""
    if "flows" in _cache:
        return _cache["flows"]
    out = [(f"10.1.{i % 7}.{10 + i}", 30000 + 7 * i, f"198.51.100.{1 + i % 5}", (80, 443, 8080)[i % 3], 1025 + i)
           for i in range(NPLAIN)]
    L, mask = mosrx.lib(), mosrx.lib().mosrx_nat_slots(NBIND) - 1
    assert mask == 255
    cip, sip, sport, port, target = "10.9.9.9", "198.51.100.77", 80, 1024, None
    while len(out) < NPLAIN + NCOLL:
        port += 1
        h = L.mosrx_nat_hash(mosrx.ip_raw(cip), mosrx.ip_raw(sip), mosrx._htons(port) | mosrx._htons(sport) << 16) & mask
        target = h if target is None else target
        if h == target:
            out.append((cip, port, sip, sport, 2000 + len(out)))
    out += [(f"172.16.5.{5 + i}", 41000 + i, "198.51.100.9", 25, 3000 + i) for i in range(NNOARP)]
    _cache["flows"] = out
    return out


def bindings():
    return mosrx.nat_bindings(flows(), nat_ip=NAT_IP)


def frame(i):
    fl = flows()
    k, g = i % 25, i // 25
    if k < 20:
        j = (g * 20 + k) * 7 % NBIND
        cip, cport, sip, sport, nport = fl[j]
        v = (i // 2) % 5
        kw = [dict(), dict(ihl=6), dict(ihl=15, doff=6), dict(doff=8), dict()][v]
        pay = b"p" * ((i * 3) % 41) if v else b""
        if k % 2 == 0:
            return tcp_frame(cip, sip, cport, sport, pay, flags=0x18, seq=i, **kw)           # client side: SNAT
        return tcp_frame(sip, NAT_IP, sport, nport, pay, flags=0x18, seq=i, **kw)            # server side: DNAT
    if k == 20:
        return tcp_frame("10.1.0.200", "198.51.100.1", 5000 + g, 80, b"new", flags=0x02, seq=i)   # no binding yet
    if k == 21:
        cip, cport, sip, sport, _ = fl[g % NPLAIN]
        return tcp_frame(cip, sip, cport, sport, flags=0x10, seq=i, doff=4)
    if k == 22:
        cip, cport, sip, sport, _ = fl[g % NPLAIN]
        return tcp_frame(cip, sip, cport, sport, flags=0x10, seq=i)[:14 + 20 + 12]            # a 12-byte segment, cut below
    if k == 23:
        cip, cport, sip, sport, _ = fl[g % NPLAIN]
        return tcp_frame(cip, sip, cport, sport, b"bad", flags=0x18, seq=i, tcp_csum=0x1)
    if g % 2:
        return tcp_frame("10.1.0.1", "198.51.100.1", 53, 53, b"udp" * (g % 5), proto=17)
    return tcp_frame(ethertype=0x0806)


def short_fix(f):
    """Frame k == 22 as the wire would hold it: tot_len 32, a valid IP checksum."""
    import struct
    from pktlib import csum16
    b = bytearray(f)
    struct.pack_into("!H", b, 16, 32)
    b[24:26] = b"\0\0"
    struct.pack_into("!H", b, 24, csum16(bytes(b[14:34])))
    return bytes(b)


def mix(n):
    have = _cache.setdefault("mix", [])
    have += [short_fix(frame(i)) if i % 25 == 22 else frame(i) for i in range(len(have), n)]
    return have[:n]


def forced(rec, n):
    """The records with the short-segment frames' reason forced to TCP_OK (see the module's text)."""
    rec = rec.copy()
    idx = np.arange(n)
    rec["reason"][idx[idx % 25 == 22]] = mosrx.R["TCP_OK"]
    return rec
