"""numpy restatement of what samples/simple_firewall does to the frames a
forward = 1 stack passes on, over a classified batch (include/mosrx.h, the
firewall rules section).  Builds on tests/fwd_oracle.py.

Written from the sample's lines, not from the GPU path:
  * which frames are looked up: CatchInitSYN (simple_firewall.c:362-372),
    tcph->syn && !tcph->ack, on the frames mOS hands to its stream engine --
    restated as the TCP arm of fwd_oracle.forwards with `forward` left out (the
    sample looks up and counts either way) and the plan's condition that the
    IPv4 packet lies inside the capture;
  * the key as ApplyActionPerFlow reads it (:346-347): iph->saddr, iph->daddr,
    tcph->source, tcph->dest, raw values of a little-endian host, tcph at
    14 + 4 * ihl; a byte at or past the batch buffer's end rounded up to 16
    reads zero (include/mosrx.h);
  * FWRLookup (:307-330): rules in order, first match wins, its fr_count bumped;
    MatchAddr (:291-298): fw_ip == 0 || (ip & (0xFFFFFFFF >> (32 - bits))) == fw_ip;
    MatchPort (:300-305): fw_port == 0 || port == fw_port; no match: ACCEPT;
  * DROP (:349-350): mtcp_setlastpkt(MOS_DROP), the frame is not forwarded --
    its plan record becomes the MOSRX_FWD_DROP record; ACCEPT (:351-359) does
    nothing to forwarding.
`parse_rules` restates ParseConfigFile (:217-289) for the rule files the tests
write, through mosrx.acl_rules.
"""
import numpy as np

import fwd_oracle as F
import mosrx

R = mosrx.R
NOT_LOOKED_UP, NO_MATCH = 0xFFFF, 0xFFFE
SYN, ACK = 0x02, 0x10


def parse_rules(text):
    """A rule file's lines as the tuples mosrx.acl_rules takes."""
    out = []
    for line in text.splitlines():
        line = line.split("#")[0].strip()
        if not line:
            continue
        act, src, dst, *ports = line.split()
        sp = dp = 0
        for p in ports:
            k, v = p.split(":")
            if k == "sport":
                sp = int(v)
            else:
                assert k == "dport", p
                dp = int(v)
        out.append((act, src, dst, sp, dp))
    return out


def eligible(frames, off, ln, reason, tcp_flags, num_msp=1, listener=False, frames_bytes=None):
    """1 where the frame is looked up."""
    frames = np.asarray(frames, np.uint8)
    off = np.asarray(off, np.uint32)
    frames_bytes = len(frames) if frames_bytes is None else int(frames_bytes)
    cap = F.capture(off, ln, frames_bytes)
    tl, ok = F._field(frames, off, cap, 16, 2)
    ip_len = tl[:, 0].astype(np.int64) * 256 + tl[:, 1]
    ip_ok = ok & (cap >= 34) & (ip_len >= 20) & (14 + ip_len <= cap)
    reason = np.asarray(reason)
    tcp = np.isin(reason, [R["TCP_OK"], R["TCP_LEN_OK"]]) & (num_msp != 0) & (not listener)
    syn = (np.asarray(tcp_flags) & (SYN | ACK)) == SYN
    return tcp & syn & ip_ok


def keys(frames, off, elig, frames_bytes=None):
    """(saddr, daddr, sport, dport) of the eligible frames, raw little-endian loads; 0 elsewhere."""
    frames = np.asarray(frames, np.uint8)
    frames_bytes = len(frames) if frames_bytes is None else int(frames_bytes)
    end = (frames_bytes + 15) // 16 * 16
    assert len(frames) >= min(end, frames_bytes), "the buffer holds its own bytes"
    img = np.zeros(max(end, len(frames)) + 128, np.uint8)
    k = min(end, len(frames))
    img[:k] = frames[:k]                       # readable up to the rounded end, zero past it
    o = np.asarray(off, np.uint32).astype(np.int64)[elig]

    def ld(at, nbytes):
        return img[at[:, None] + np.arange(nbytes)]
    n = len(off)
    sa, da = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    sp, dp = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    sa[elig] = ld(o + 26, 4).copy().view("<u4")[:, 0]
    da[elig] = ld(o + 30, 4).copy().view("<u4")[:, 0]
    ihl = (img[o + 14] & 0xF).astype(np.int64)
    pt = ld(o + 14 + 4 * ihl, 4).copy().view("<u2")
    sp[elig], dp[elig] = pt[:, 0], pt[:, 1]
    return sa, da, sp, dp


def lookup(rules, elig, sa, da, sp, dp):
    """FWRLookup per frame: the matched rule's index, NO_MATCH, or NOT_LOOKED_UP."""
    hit = np.where(elig, NO_MATCH, NOT_LOOKED_UP).astype(np.uint16)
    looking = np.asarray(elig, bool).copy()
    for j, r in enumerate(rules):
        m = looking
        m = m & ((r["src_ip"] == 0) | ((sa & r["src_mask"]) == r["src_ip"]))
        m = m & ((r["dst_ip"] == 0) | ((da & r["dst_mask"]) == r["dst_ip"]))
        m = m & ((r["sport"] == 0) | (sp == r["sport"])) & ((r["dport"] == 0) | (dp == r["dport"]))
        hit[m] = j
        looking = looking & ~m
        if not looking.any():
            break
    return hit


def counts(hit, nrules, into=None):
    """fr_count of every rule after these lookups, added to `into` (MOSRX_ACL_MAX_RULES u32)."""
    out = np.zeros(mosrx.ACL_MAX_RULES, np.uint32) if into is None else into.copy()
    h = np.asarray(hit).astype(np.int64)
    out += np.bincount(h[h < nrules], minlength=mosrx.ACL_MAX_RULES).astype(np.uint32)
    return out


def dropped(hit, rules):
    h = np.asarray(hit).astype(np.int64)
    d = np.zeros(len(h), bool)
    m = h < len(rules)
    d[m] = rules["action"][h[m]] == mosrx.ACL_DROP
    return d


def amend(plan, hit, rules, forward=1):
    """The plan after the launch: DROP rules' frames get the MOSRX_FWD_DROP record (forward != 0)."""
    out = plan.copy()
    if forward:
        d = dropped(hit, rules)
        out["tx_len"][d] = 0
        out["out_ifidx"][d] = -1
        out["kind"][d] = mosrx.FWD_DROP
        out["arp_idx"][d] = 0xFFFF
        out["reserved"][d] = 0
    return out


def apply(frames, off, ln, rec, rules, plan=None, num_msp=1, listener=False, forward=1, frames_bytes=None,
          counts_in=None):
    """(hit, counts, amended plan or None) for a batch and its records (reason, tcp_flags)."""
    el = eligible(frames, off, ln, rec["reason"], rec["tcp_flags"], num_msp, listener, frames_bytes)
    hit = lookup(rules, el, *keys(frames, off, el, frames_bytes))
    return hit, counts(hit, len(rules), counts_in), None if plan is None else amend(plan, hit, rules, forward)
