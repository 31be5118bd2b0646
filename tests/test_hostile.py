"""The hostile inputs (tests/hostile.py) do what they claim, by the oracles alone:
the condition that keeps tests/test_hostile_gpu.py from passing on easy input.
Also mosrx_nat_patch_frame (host product code) against nat_oracle.translate over
every hostile frame, and the three edits of the launches' conditions that the
inputs must tell apart, each evaluated in numpy against the oracle's answer."""
import numpy as np
import pytest

import acl_oracle as A
import fwd_oracle as F
import hostile as H
import mosrx
import nat_oracle as N
from test_nat import keys_of, walk

R = mosrx.R
IHLS = set(range(5, 16))


@pytest.fixture(scope="module")
def hb():
    h = H.batch(H.N)
    x, tr = N.translate(h.buf, h.off, h.ln, h.rec["reason"], H.bindings())
    el = A.eligible(h.buf, h.off, h.ln, h.rec["reason"], h.rec["tcp_flags"])
    o = h.off.astype(np.int64)
    cap = F.capture(h.off, h.ln, len(h.buf))
    tot = h.buf[o + 16].astype(np.int64) * 256 + h.buf[o + 17]
    ihl = (h.buf[o + 14] & 0xF).astype(np.int64)
    return dict(h=h, x=x, tr=tr, el=el, cap=cap, tot=tot, ihl=ihl, xl=np.isin(x["kind"], [N.SNAT, N.DNAT]))


def test_the_generator_is_seeded():
    a, b = H.generate(64), H.generate(64)
    assert a[0] == b[0] and a[1] == b[1] and (a[2] == b[2]).all()
    h = H.batch(H.N)
    assert len(h.off) == H.N == 1025 and h.rec8.tobytes() == H.rec8_of(h.rec).tobytes()
    assert h.rec.tobytes() == H.classify(h.buf, h.off, h.ln).tobytes()            # the oracle's, unforced


def test_nat_kinds_and_what_the_translated_frames_cover(hb):
    h, x, xl = hb["h"], hb["x"], hb["xl"]
    kinds = np.bincount(x["kind"], minlength=5)
    print("kinds NONE SNAT DNAT MISS HOST", kinds.tolist())
    print("translated per ihl 5..15", np.bincount(x["ihl"][xl], minlength=16)[5:].tolist())
    assert (kinds > 0).all()
    o = h.off.astype(np.int64)
    doff = h.buf[o + 14 + 4 * hb["ihl"] + 12] >> 4
    seg = hb["tot"] - 4 * hb["ihl"]
    host = x["kind"] == N.HOST
    assert (h.rec["reason"][host] == R["TCP_OK"]).all()                             # as classified: nothing forced
    assert (host & (doff < 5) & (seg >= 20)).sum() >= 5                             # HOST through doff alone
    assert (host & (seg < 20)).sum() >= 5                                           # HOST through a short segment
    assert {int(v) for v in seg[host & (seg < 20)]} >= {4, 12, 16, 19}
    assert {int(v) for v in x["ihl"][xl]} == IHLS
    assert {int(v) % 2 for v in seg[xl]} == {0, 1}
    assert {int(v) % 4 for v in h.off[xl]} == {0, 1, 2, 3}
    assert {int(v) % 16 for v in h.off} == set(range(16))
    assert {int(v) for v in doff[xl]} == set(range(5, 16))
    # about half of the TCP frames the launch looks up belong to a binding
    looked = xl.sum() + kinds[N.MISS]
    assert 0.35 * looked <= xl.sum() <= 0.65 * looked and xl.sum() >= 100
    # the edges of ip_ok among the translated frames: tot_len equal to the capture, and shorter (trailing pad)
    assert (xl & (14 + hb["tot"] == hb["cap"])).sum() >= 5 and (xl & (14 + hb["tot"] < hb["cap"])).sum() >= 5
    assert set(h.meta.flags.tolist()) == set(range(256))


def test_firewall_eligibility_tiles_and_rules(hb):
    h, el = hb["h"], hb["el"]
    print("firewall-eligible per ihl 5..15", np.bincount(hb["ihl"][el], minlength=16)[5:].tolist())
    assert {int(v) for v in hb["ihl"][el]} == IHLS
    per_tile = [el[k:k + H.T] for k in range(0, H.N, H.T)]
    assert any(t.sum() == 0 and len(t) == H.T for t in per_tile)                    # no eligible lane
    assert any(t.sum() == 1 and len(t) == H.T for t in per_tile)                    # exactly one
    assert per_tile[2].sum() == 1 and el[H.LONE_SYN] and el[1024]
    assert any(len(t) == H.T and all(t[w:w + 64].any() for w in range(0, H.T, 64)) for t in per_tile)   # all four waves
    # SYNs whose packet does not lie inside the capture, or whose record is not an accepted segment, are not looked up
    syn = (h.rec["tcp_flags"] & 0x12) == 0x02
    assert (syn & ~el).sum() >= 20
    for name, rules in H.rule_sets().items():
        hit, cnt, _ = A.apply(h.buf, h.off, h.ln, h.rec, rules)
        matched = (hit < len(rules)).sum()
        print(name, "eligible", int(el.sum()), "matched", int(matched), "rules hit", sorted(set(hit[hit < len(rules)].tolist())))
        assert 0.25 * el.sum() <= matched <= 0.75 * el.sum(), name                  # about half of the SYNs hit a rule
    rs = H.rule_sets()
    assert len(rs["last_of_full"]) == mosrx.ACL_MAX_RULES and len(rs["n257"]) == 257
    hit = A.apply(h.buf, h.off, h.ln, h.rec, rs["last_of_full"])[0]
    assert set(hit[el].tolist()) == {mosrx.ACL_MAX_RULES - 1, A.NO_MATCH}
    hit = A.apply(h.buf, h.off, h.ln, h.rec, rs["n257"])[0]
    assert set(hit[el].tolist()) == {100, 255, 256, A.NO_MATCH}
    hit = A.apply(h.buf, h.off, h.ln, h.rec, rs["overlap"])[0]
    assert set(hit[el].tolist()) == {0, 1, 2, 3, A.NO_MATCH}                        # rule 4 is never reached
    acts = rs["overlap"]["action"]
    assert (acts[0], acts[1], acts[2], acts[3]) == (mosrx.ACL_ACCEPT, mosrx.ACL_DROP, mosrx.ACL_DROP, mosrx.ACL_ACCEPT)


def test_every_reason_occurs_and_a_third_is_tcp_ok(hb):
    h = hb["h"]
    census = {k: int((h.rec["reason"] == v).sum()) for k, v in R.items()}
    print("reasons", {k: v for k, v in census.items() if v})
    # num_msp = 1, forward = 1, checksums verified, no local address: what mo_classify_one can return
    can = {"TCP_OK", "ARP", "NON_IPV4", "IP_SHORT", "IP_BADVER", "IP_BADCSUM", "NOT_TCP", "TCP_SHORT", "TCP_BADCSUM",
           "TRUNCATED"}
    assert {k for k, v in census.items() if v} == can
    assert 3 * census["TCP_OK"] >= H.N
    # every kind of damage is there, and each cut of len[] left its value
    assert set(h.meta.damage.tolist()) == set(range(-1, len(H.DAMAGE)))
    d = h.meta.damage
    for k, want in ((6, 33), (7, 34)):
        assert (h.ln[d == k] == want).all()
    cut = d == 10
    assert (h.ln[cut] == 14 + hb["tot"][cut] - 1).all() and (h.rec["reason"][cut] == R["TRUNCATED"]).all()


@pytest.mark.parametrize("nslots", [16, 256])
def test_probe_edge_tables(nslots):
    pe = H.probe_edge_bindings(nslots)
    slots, probe = mosrx.nat_table(pe.bindings)                                     # mosrx_nat_build itself
    mask = nslots - 1
    assert len(slots) == nslots and pe.start >= nslots - 2
    assert probe == pe.k                                                            # the run is the longest
    run = [(pe.start + j) & mask for j in range(pe.k)]
    assert run[-1] < run[0] and 0 in run                                            # it wraps past slot 0
    L = mosrx.lib()
    for j, s in enumerate(run):                                                     # binding j's client key at depth j + 1
        assert slots[s]["kind"] == N.SNAT and slots[s]["bind"] == j
        b = pe.bindings[j]
        assert L.mosrx_nat_hash(int(b["cli_ip"]), int(b["svr_ip"]), int(b["cli_port"]) | int(b["svr_port"]) << 16) & mask == pe.start
    assert slots[(run[-1] + 1) & mask]["kind"] == 0 and slots[(run[0] - 1) & mask]["kind"] == 0
    assert pe.last == pe.flows[pe.k - 1] and slots[run[-1]]["port"] == pe.bindings[pe.k - 1]["nat_port"]
    keys, idx = keys_of(pe.bindings)
    at = walk(slots, probe, keys)
    assert (at >= 0).all() and (slots[at]["bind"] == idx).all()
    short = walk(slots, probe - 1, keys)                                            # one step less loses the last-in-run key only
    assert np.nonzero(short < 0)[0].tolist() == [pe.k - 1]
    c, cp, s, sp = pe.absent
    ak = np.array([[mosrx.ip_raw(c), mosrx.ip_raw(s), mosrx._htons(cp) | mosrx._htons(sp) << 16, 0, 0, 0]], np.uint32)
    assert L.mosrx_nat_hash(int(ak[0, 0]), int(ak[0, 1]), int(ak[0, 2])) & mask == pe.start
    assert walk(slots, probe, ak)[0] < 0 and walk(slots, nslots, ak)[0] < 0         # absent, behind the longest run
    # and the oracle's answers for the two keys' frames
    buf, off, ln = H.pack(H.probe_edge_frames(pe))
    x, _ = N.translate(buf, off, ln, H.classify(buf, off, ln)["reason"], pe.bindings)
    assert x["kind"][-1] == N.SNAT and x["bind"][-1] == pe.k - 1 and x["kind"][-2] == N.MISS
    assert np.isin(x["kind"][:-2], [N.SNAT, N.DNAT]).all()


def test_patch_frame_against_the_restatement(hb):
    h, x, tr, xl = hb["h"], hb["x"], hb["tr"], hb["xl"]
    for i in range(H.N):
        o, n = int(h.off[i]), len(h.frames[i])
        got = mosrx.nat_patch_frame(h.buf[o:o + n], x[i])
        assert got.tobytes() == tr[o:o + n].tobytes(), (i, x[i])
        if not xl[i]:
            assert got.tobytes() == bytes(h.frames[i])
    again = H.classify(tr, h.off, h.ln)                                             # valid TCP again, by mOS's own sums
    assert (again["reason"][xl] == R["TCP_OK"]).all()


def test_cuts_and_special_frames():
    a, z = H.eligible_frame(), H.zero_segment_frame()
    assert a[14] & 0xF == 7 and a[16] * 256 + a[17] == 28 + 45 == len(a) - 14
    assert z[14] & 0xF == 5 and z[16] * 256 + z[17] == 20 and len(z) == 60
    ks = H.cut_ks(a)
    assert {0, 13, 14, 33, 34, 14 + 73 - 1, 14 + 73, len(a)} <= set(ks) and {42 + j for j in H.IHL_J} <= set(ks)
    cp = H.cut_points(a, 1000)
    assert all(1000 + k in cp and (1000 + k) // 16 * 16 in cp and (1000 + k + 15) // 16 * 16 in cp for k in ks)
    for last in (a, z):
        c = H.cut_batch(last)
        assert len(c.off) == 257 and c.frames[255] == a and c.frames[256] == last
        assert (int(c.off[256]) + 14 + 4 * (last[14] & 0xF)) % 16 == 14             # the ports' dword straddles a 16-byte line
        assert (c.rec["reason"][255:] == R["TCP_OK"]).all() and (c.rec["tcp_flags"][255:] == 0x02).all()
        cuts = H.cut_points(last, int(c.off[256]), len(last))
        assert min(cuts) >= int(c.off[255]) + int(c.ln[255]) and max(cuts) <= len(c.buf)   # frame 255 stays whole
        el = [A.eligible(c.buf, c.off, c.ln, c.rec["reason"], c.rec["tcp_flags"], frames_bytes=fb)[255:].tolist() for fb in cuts]
        assert [True, False] in el and [True, True] in el
        # the ports rule set tells apart what a lookup saw of the last frame's ports
        hits = {int(A.apply(c.buf, c.off, c.ln, c.rec, H.rule_sets()["ports"], frames_bytes=fb)[0][256]) for fb in cuts}
        # (an eligible frame's ports lie inside its packet unless the packet ends before them: the empty segment)
        assert hits == ({A.NOT_LOOKED_UP, 0} if last is a else {A.NOT_LOOKED_UP, 0, 1}), hits
    # the empty segment's packet ending on a 16-byte line: a buffer ending there shows neither port
    c = H.cut_batch(z, H.end_phase(z))
    assert (int(c.off[256]) + 34) % 16 == 0
    hits = [int(A.apply(c.buf, c.off, c.ln, c.rec, H.rule_sets()["ports"], frames_bytes=int(c.off[256]) + k)[0][256])
            for k in (33, 34, 35)]
    assert hits == [A.NOT_LOOKED_UP, 3, 0]
    s = H.len_sweep()
    assert (s.rec_whole["reason"] == R["TCP_OK"]).all() and R["TRUNCATED"] in s.rec["reason"] and R["TCP_OK"] in s.rec["reason"]


def test_the_inputs_tell_three_edits_apart(hb):
    """Each edit of a launch's condition, evaluated in numpy, differs from the oracle at a named frame."""
    h, x, xl = hb["h"], hb["x"], hb["xl"]
    # 1. plan-nat's `14u + k_len <= k_cap` as `<`: a translated frame whose packet ends with its capture
    edited = xl & (14 + hb["tot"] < hb["cap"])
    lost = np.nonzero(xl & ~edited)[0]
    print("plan-nat `<`: first frames lost", lost[:4].tolist())
    assert len(lost) >= 5
    # 2. the probe loop's bound as probe - 1: the last-in-run key of either table (test_probe_edge_tables' walk)
    # 3. the firewall's `cap >= 34u` as `> 34u`: the empty-segment SYN with its capture or the buffer ending at byte 34
    s = H.len_sweep()
    el = A.eligible(s.buf, s.off, s.ln, s.rec_whole["reason"], s.rec_whole["tcp_flags"])
    at34 = np.nonzero(el & (s.ln == 34))[0]
    print("firewall `> 34`: len sweep frames lost", at34.tolist())
    assert len(at34) == 1 and s.frames[at34[0]] == H.zero_segment_frame()
    c = H.cut_batch(H.zero_segment_frame())
    fb = int(c.off[256]) + 34
    assert fb in H.cut_points(c.frames[256], int(c.off[256]))
    assert A.eligible(c.buf, c.off, c.ln, c.rec["reason"], c.rec["tcp_flags"], frames_bytes=fb)[256]
    assert F.capture(c.off, c.ln, fb)[256] == 34
