"""The firewall scenarios pinned to samples/simple_firewall itself, shared by
test_acl_oracle.py and golden/make_golden_acl.py.

oracle/_ref/simple_firewall_emul in "pp" mode is the sample, unmodified, over
mOS's own ProcessPacket with everything it sends dumped to tx.pcap
(tests/test_simple_firewall.py, whose trace, conf and runner are used as they
are).  Two scenarios: that test's trace under its rules file ("firewall"), and a
short trace under a rules file that has what the first lacks ("masks"): a mask
that is no multiple of 8 bits on each side, a port wildcard on each side, a
rule shadowed by an earlier one, a SYN no rule matches.
"""
import numpy as np

import acl_oracle as A
import fwd_oracle as F
import mosrx
import oracle_py as O
import pktlib
import test_simple_firewall as SF

# IP_NETMASK keeps the LOW bits of the last partial octet: 10.21.0.0/12 is "first
# octet 10, second octet's low nibble 5" (10.5.x.x, 10.37.x.x; not 10.22.x.x), and
# 10.9.69.0/19 is "10.9, third octet's low three bits 5" (10.9.13.x, 10.9.69.x)
MASKS_RULES = """# act   src            dst            ports
DROP    10.21.0.0/12   10.7.0.0/16    dport:80
ACCEPT  10.8.1.0/24    10.9.69.0/19   sport:4000
DROP    10.8.1.0/24    10.9.69.0/19
ACCEPT  10.8.1.5       10.9.13.1      sport:4000
DROP    0.0.0.0        10.10.10.10    dport:22
"""
MASKS_COUNTS = [2, 1, 1, 0, 1]   # by hand: rule 4 is shadowed by rule 2


def masks_frames():
    t = mosrx.Trace(mosrx.TRACE_FW64, 300)
    base = [bytes(t.frames[int(o):int(o) + int(n)]) for o, n in zip(t.off, t.len)]
    flows = [SF.handshake("10.37.1.1", "10.7.0.9", 40000, 80, 100),      # rule 1 (low nibble 5 of 37): DROP
             SF.handshake("10.5.2.2", "10.7.3.3", 40001, 80, 150),       # rule 1 again
             SF.handshake("10.22.1.1", "10.7.0.9", 40002, 80, 200),      # inside a true 10.16/12, not the sample's: no rule
             SF.handshake("10.8.1.5", "10.9.13.1", 4000, 443, 300),      # rule 2 (any dport); rule 4 never sees it
             SF.handshake("10.8.1.6", "10.9.69.7", 5000, 25, 400),       # rule 3 (both ports any): DROP
             SF.handshake("9.9.9.9", "10.10.10.10", 1111, 22, 500),      # rule 5 (any source, any sport): DROP
             SF.handshake("9.9.9.9", "10.10.10.10", 1112, 23, 600)]      # no rule: ACCEPT
    out, k = [], 0
    for i, fr in enumerate(base):
        out.append(fr)
        if i % 30 == 29 and k < max(len(f) for f in flows):
            out += [f[k] for f in flows if k < len(f)]
            k += 1
    return out


SCENARIOS = {"firewall": (SF.firewall_frames, SF.RULES), "masks": (masks_frames, MASKS_RULES)}


def tables():
    """The tables of test_simple_firewall's conf: everything goes lo -> lo."""
    return mosrx.fwd_tables(routes=[("0.0.0.0/0", 0)], arp=[("0.0.0.0/0", "02:00:00:00:00:aa")],
                            netdevs=["00:00:00:00:00:00"], nic_fwd={0: 0})


def restated(frames, rules_text):
    """(buf, off, len, records, rules, hit, counts, amended plan, tx list) of the restatement."""
    buf, off, ln = pktlib.pack_frames(frames)
    rec = O.classify(buf, off, ln, O.params())
    rules = mosrx.acl_rules(A.parse_rules(rules_text))
    t = tables()
    pl = F.plan(buf, off, ln, rec["reason"], t, 0, forward=1, num_msp=1, listener=False)
    hit, cnt, pl = A.apply(buf, off, ln, rec, rules, pl)
    n = len(off)
    cap = int(ln.astype(np.int64).sum()) + 32 * n + 16
    tx, toff, tlen, tnif, tsrc, c = F.build(buf, off, pl, t, cap, np.zeros(cap, np.uint8), np.zeros(n, np.uint32),
                                            np.zeros(n, np.uint16), np.zeros(n, np.int8), np.zeros(n, np.uint32))
    assert c[1] == 0
    return buf, off, ln, rec, rules, hit, cnt, pl, F.tx_list(tx, toff, tlen, int(c[0]))


def run_sample(tmp, name, frames, rules_text):
    """The sample's own run: its printed rule table's counts and the frames it sent (ARP aside)."""
    import os
    exe = os.path.join(SF.REF, "simple_firewall_emul")
    d = tmp / name
    d.mkdir()
    # SF.run_sample takes no rules argument: it writes its module's RULES to <dir>/pp/fw.conf.  That module is
    # not ours to edit, so the text is swapped in around the call; test_acl_oracle reads fw.conf back and fails
    # if the sample was not given these rules (should SF ever write the file another way).
    keep = SF.RULES
    SF.RULES = rules_text
    try:
        r = SF.run_sample(exe, "pp", d, frames)
    finally:
        SF.RULES = keep
    assert r["result"]["done"] == len(frames)
    return [c for _, c, _ in r["table"]], [a for _, _, a in r["table"]], [f for f in r["tx"] if not SF.is_arp(f)]
