"""numpy restatement of the ring form of the forwarding build
(mosrx_fwd_build_rings_dev, include/mosrx.h): the frames fwd_oracle.tx_frame
gives, each in the TX ring of its output netdev.

  * sent: kind IP or ETH, tx_len >= 14, out_ifidx in 0 .. nrings - 1;
  * ring q is tx[q * ring_cap .. (q + 1) * ring_cap); its r-th sent frame, in
    arrival order, starts at q * ring_cap + 16 k + 2, k the exclusive scan of
    ceil((2 + tx_len) / 16) over netdev q's sent frames alone;
  * its entry is rings[q].start + r, start the sent frames of the netdevs below
    q whether they fit or not;
  * a frame whose padded end passes ring_cap is dropped, and so is every later
    frame of that netdev; its entry is left as it was;
  * rings[0 .. nrings) is written whole; nothing else but frame bytes and live
    entries is.
Everything is written into copies of the initial buffers given.
"""
import numpy as np

import fwd_oracle as F
import mosrx


def sent_mask(pl, nrings):
    return np.isin(pl["kind"], [F.IP, F.ETH]) & (pl["tx_len"] >= 14) & (pl["out_ifidx"] >= 0) & \
        (pl["out_ifidx"].astype(np.int64) < nrings)


def units_of(pl):
    return (pl["tx_len"].astype(np.int64) + 2 + 15) // 16


def need_units(pl, nrings):
    """Per ring: the 16-byte units its sent frames take."""
    s = sent_mask(pl, nrings)
    return np.bincount(pl["out_ifidx"][s].astype(np.int64), weights=units_of(pl)[s], minlength=nrings).astype(np.int64)


def build(frames, off, pl, t, ring_cap, nrings, tx_init, off_init, len_init, src_init, rings_init):
    """(tx_frames, tx_off, tx_len, tx_src, rings) over copies of the initial buffers;
    rings_init is an array of mosrx.FWD_RING_DTYPE with at least nrings records."""
    T = F.tables_np(t)
    frames = np.asarray(frames, np.uint8)
    tx, toff, tlen, tsrc, rings = (a.copy() for a in (tx_init, off_init, len_init, src_init, rings_init))
    assert rings.dtype == mosrx.FWD_RING_DTYPE and ring_cap % 16 == 0
    s = sent_mask(pl, nrings)
    start = 0
    for q in range(nrings):
        k = count = dropped = 0
        full = False
        mine = np.nonzero(s & (pl["out_ifidx"] == q))[0]
        for r, i in enumerate(mine):
            units = (2 + int(pl["tx_len"][i]) + 15) // 16
            if full or (k + units) * 16 > ring_cap:
                full = True                    # offsets only grow: every later frame of the ring is dropped too
                dropped += 1
                continue
            o = q * ring_cap + 16 * k + 2
            f = F.tx_frame(frames, off[i], pl[i], T)
            tx[o:o + len(f)] = f
            j = start + r
            toff[j], tlen[j], tsrc[j] = o, len(f), i
            count += 1
            k += units
        rings[q] = (start, count, dropped, k)
        start += len(mine)
    return tx, toff, tlen, tsrc, rings


def ring_list(tx, toff, tlen, rings, q):
    """The frames written to ring q, in order."""
    a, c = int(rings[q]["start"]), int(rings[q]["count"])
    return [bytes(tx[int(o):int(o) + int(n)]) for o, n in zip(toff[a:a + c], tlen[a:a + c])]
