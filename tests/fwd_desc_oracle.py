"""numpy restatement of the descriptor form of the ring build
(mosrx_fwd_desc_rings_dev, include/mosrx.h), on top of the two restatements that
are pinned to mOS's own tx.pcap:

  * fwd_rings_oracle.build with a ring_cap that drops nothing gives rings
    (dropped == 0, units the ring's whole need), tx_src and tx_len exactly;
  * tx_mac[e] is the first 12 bytes of fwd_oracle.tx_frame for entry e.
Everything is written into copies of the initial buffers given; entries at and
past the total sent count stay as they were.
"""
import numpy as np

import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx


def build(frames, off, pl, t, nrings, src_init, len_init, mac_init, rings_init):
    """(tx_src, tx_len, tx_mac, rings) over copies of the initial buffers; mac_init
    is a uint8 array of 12 bytes per entry."""
    n = len(off)
    assert mac_init.dtype == np.uint8 and len(mac_init) >= 12 * n
    cap = int(FR.need_units(pl, nrings).max(initial=0)) * 16
    _, _, tlen, tsrc, rings = FR.build(frames, off, pl, t, cap, nrings, np.zeros(nrings * cap + 64, np.uint8),
                                       np.zeros(len(src_init), np.uint32), len_init, src_init, rings_init)
    assert (rings["dropped"][:nrings] == 0).all()
    mac = mac_init.copy()
    T = F.tables_np(t)
    frames = np.asarray(frames, np.uint8)
    total = int(rings["count"][:nrings].sum())
    assert total == int(rings[nrings - 1]["start"]) + int(rings[nrings - 1]["count"])
    for e in range(total):
        i = int(tsrc[e])
        mac[12 * e:12 * e + 12] = np.frombuffer(bytes(F.tx_frame(frames, off[i], pl[i], T))[:12], np.uint8)
    return tsrc, tlen, mac, rings


def ring_list(frames, off, tsrc, tlen, mac, rings, q):
    """The frames a host sends for ring q, in order: each entry's source frame,
    tx_len bytes of it, with tx_mac laid over the start."""
    frames = np.asarray(frames, np.uint8)
    a, c = int(rings[q]["start"]), int(rings[q]["count"])
    out = []
    for e in range(a, a + c):
        o, n = int(off[int(tsrc[e])]), int(tlen[e])
        out.append(bytes(mac[12 * e:12 * e + 12]) + bytes(frames[o + 12:o + n]))
    return out
