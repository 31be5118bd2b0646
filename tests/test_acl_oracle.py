"""The firewall restatement (tests/acl_oracle.py) on the CPU: hand-worked cases of
the sample's mask arithmetic and first-match walk, the committed fixture
(tests/golden/acl_firewall.npz, made from the sample's own rule table and
tx.pcap), and -- where oracle/_ref/simple_firewall_emul is built -- the sample
itself again, live, on test_simple_firewall's trace and on the "masks" rules
file (tests/acl_pin.py)."""
import os

import numpy as np
import pytest

import acl_oracle as A
import acl_pin as P
import fwd_oracle as F
import mosrx
from pktlib import R, pack_frames, tcp_frame
from test_simple_firewall import REF, firewall_frames, pcap_frames, rule_table, run_sample

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acl_firewall.npz")
EXE = os.path.join(REF, "simple_firewall_emul")


def one(rules, src, dst, sport, dport, flags=0x02, **kw):
    """The hit of one frame under the rules (tuples)."""
    buf, off, ln = pack_frames([tcp_frame(src, dst, sport, dport, flags=flags, **kw)])
    rec = np.zeros(1, mosrx.RESULT_DTYPE)
    rec["reason"], rec["tcp_flags"] = R["TCP_OK"], flags
    return int(A.apply(buf, off, ln, rec, mosrx.acl_rules(rules))[0][0])


def test_masks_as_the_sample_computes_them():
    # /12 on the stored (network-order) address keeps the first octet and the LOW nibble of the second
    r = [("DROP", "10.21.0.0/12", "0.0.0.0")]
    assert [one(r, s, "1.1.1.1", 1, 2) for s in ("10.5.0.1", "10.37.9.9", "10.21.0.0", "10.22.0.1", "10.16.0.1", "11.5.0.1")] \
        == [0, 0, 0, A.NO_MATCH, A.NO_MATCH, A.NO_MATCH]
    # /19 on the destination: 10.9 and the third octet's low three bits
    r = [("DROP", "0.0.0.0", "10.9.69.0/19")]
    assert [one(r, "1.1.1.1", d, 1, 2) for d in ("10.9.13.200", "10.9.69.1", "10.9.5.5", "10.9.64.1", "10.9.70.1")] \
        == [0, 0, 0, A.NO_MATCH, A.NO_MATCH]
    # a rule address whose masked value is 0 is the wildcard, whatever was written (MatchAddr: fw_ip == 0)
    assert one([("DROP", "0.16.0.0/12", "0.0.0.0")], "200.1.2.3", "1.1.1.1", 1, 2) == 0


def test_first_match_ports_and_wildcards():
    r = [("ACCEPT", "10.0.0.0/8", "0.0.0.0", 1000, 0), ("DROP", "10.0.0.0/8", "0.0.0.0", 0, 80),
         ("ACCEPT", "10.1.1.1", "10.2.2.2", 1000, 80), ("DROP", "0.0.0.0", "0.0.0.0")]
    assert one(r, "10.1.1.1", "10.2.2.2", 1000, 80) == 0       # rule 3 is shadowed by rule 1
    assert one(r, "10.1.1.1", "10.2.2.2", 1001, 80) == 1
    assert one(r, "10.1.1.1", "10.2.2.2", 1001, 81) == 3       # the catch-all
    assert one(r[:3], "10.1.1.1", "10.2.2.2", 1001, 81) == A.NO_MATCH
    assert one(r, "10.1.1.1", "10.2.2.2", 0x1234, 0x5678, ihl=6) == 3   # ports behind IP options
    assert one([("DROP", "0.0.0.0", "0.0.0.0", 0x1234, 0x5678)], "1.1.1.1", "2.2.2.2", 0x1234, 0x5678, ihl=15) == 0
    assert one([("DROP", "0.0.0.0", "0.0.0.0", 0x1234, 0x5678)], "1.1.1.1", "2.2.2.2", 0x3412, 0x7856) == A.NO_MATCH


def test_eligibility():
    r = [("DROP", "0.0.0.0", "0.0.0.0")]
    assert one(r, "1.1.1.1", "2.2.2.2", 1, 2, flags=0x12) == A.NOT_LOOKED_UP     # SYN-ACK
    assert one(r, "1.1.1.1", "2.2.2.2", 1, 2, flags=0x10) == A.NOT_LOOKED_UP
    assert one(r, "1.1.1.1", "2.2.2.2", 1, 2, flags=0xC2) == 0                   # SYN with ECE | CWR: still syn && !ack
    buf, off, ln = pack_frames([tcp_frame(flags=0x02)] * 3)
    rec = np.zeros(3, mosrx.RESULT_DTYPE)
    rec["tcp_flags"] = 0x02
    rec["reason"] = [R["TCP_OK"], R["TCP_BADCSUM"], R["TCP_LEN_OK"]]
    rules = mosrx.acl_rules(r)
    assert A.apply(buf, off, ln, rec, rules)[0].tolist() == [0, A.NOT_LOOKED_UP, 0]
    assert (A.apply(buf, off, ln, rec, rules, listener=True)[0] == A.NOT_LOOKED_UP).all()
    assert (A.apply(buf, off, ln, rec, rules, num_msp=0)[0] == A.NOT_LOOKED_UP).all()
    # the packet must lie inside the capture: a buffer that ends inside the second frame
    fb = int(off[1]) + 40
    assert A.apply(buf, off, ln, rec, rules, frames_bytes=fb)[0].tolist() == [0, A.NOT_LOOKED_UP, A.NOT_LOOKED_UP]


def test_counts_and_plan_amendment():
    fr = [tcp_frame("10.0.0.1", "10.0.0.2", 1, 80, flags=0x02), tcp_frame("10.0.0.1", "10.0.0.2", 1, 81, flags=0x02),
          tcp_frame("10.0.0.1", "10.0.0.2", 1, 80, flags=0x12), tcp_frame("10.0.0.1", "10.0.0.2", 2, 80, flags=0x02)]
    buf, off, ln = pack_frames(fr)
    rec = np.zeros(4, mosrx.RESULT_DTYPE)
    rec["reason"], rec["tcp_flags"] = R["TCP_OK"], [0x02, 0x02, 0x12, 0x02]
    rules = mosrx.acl_rules([("DROP", "0.0.0.0", "0.0.0.0", 0, 80), ("ACCEPT", "0.0.0.0", "0.0.0.0", 0, 81)])
    t = mosrx.fwd_tables(netdevs=["02:00:00:00:00:a0"], nic_fwd={0: 0})
    pl = F.plan(buf, off, ln, rec["reason"], t, 0)
    hit, cnt, out = A.apply(buf, off, ln, rec, rules, pl)
    assert hit.tolist() == [0, 1, A.NOT_LOOKED_UP, 0] and cnt[:3].tolist() == [2, 1, 0] and cnt.sum() == 3
    assert out["kind"].tolist() == [mosrx.FWD_DROP, F.IP, F.IP, mosrx.FWD_DROP]
    assert out[0].tolist() == (0, -1, 6, 0xFFFF, 0) and out[1] == pl[1] and out[2] == pl[2]
    # counts accumulate; forward = 0: looked up and counted all the same, the plan stays NONE
    pl0 = F.plan(buf, off, ln, rec["reason"], t, 0, forward=0)
    hit0, cnt0, out0 = A.apply(buf, off, ln, rec, rules, pl0, forward=0, counts_in=cnt)
    assert hit0.tolist() == hit.tolist() and cnt0[:2].tolist() == [4, 2] and not out0["kind"].any()


def test_acl_rules_refuses_slash_zero_and_bad_input():
    with pytest.raises(ValueError):
        mosrx.acl_rules([("DROP", "10.0.0.0/0", "0.0.0.0")])
    with pytest.raises(ValueError):
        mosrx.acl_rules([("DROP", "0.0.0.0", "10.0.0.0/33")])
    with pytest.raises(ValueError):
        mosrx.acl_rules([("REJECT", "0.0.0.0", "0.0.0.0")])
    with pytest.raises(ValueError):
        mosrx.acl_rules([("DROP", "0.0.0.0", "0.0.0.0")] * (mosrx.ACL_MAX_RULES + 1))
    assert A.parse_rules(P.MASKS_RULES)[0] == ("DROP", "10.21.0.0/12", "10.7.0.0/16", 0, 80)


def load():
    return np.load(GOLDEN)


@pytest.mark.parametrize("name", sorted(P.SCENARIOS))
def test_restatement_matches_fixture(name):
    """acl_firewall.npz holds what the sample counted and sent: the restatement reproduces it."""
    z, k = load(), name + "__"
    make, text = P.SCENARIOS[name]
    buf, off, ln, rec, rules, hit, cnt, pl, tx = P.restated(make(), text)
    assert rules.tobytes() == z[k + "rules"].tobytes() and int(z[k + "n"][0]) == len(off)
    assert cnt[:len(rules)].tolist() == z[k + "counts"].tolist() and cnt[len(rules):].sum() == 0
    sent = np.isin(pl["kind"], [F.IP, F.ETH])
    if name == "masks":
        assert z[k + "counts"].tolist() == P.MASKS_COUNTS
        np.testing.assert_array_equal(buf, z[k + "frames"])
        np.testing.assert_array_equal(hit, z[k + "hit"])
        np.testing.assert_array_equal(pl, z[k + "plan"].view(mosrx.FWD_DTYPE).reshape(-1))
        np.testing.assert_array_equal(np.nonzero(sent)[0], z[k + "tx_src"])
        # the fixture's own inputs give the same answer without the frame generator
        r2 = np.zeros(len(off), mosrx.RESULT_DTYPE)
        r2["reason"], r2["tcp_flags"] = z[k + "reason"], z[k + "tcp_flags"]
        np.testing.assert_array_equal(A.apply(z[k + "frames"], z[k + "off"], z[k + "len"], r2, z[k + "rules"])[0], hit)
        assert (hit == A.NO_MATCH).sum() == 3 and (pl["kind"] == mosrx.FWD_DROP).sum() == 4
    else:
        np.testing.assert_array_equal(np.nonzero(hit != A.NOT_LOOKED_UP)[0], z[k + "hit_idx"])
        np.testing.assert_array_equal(hit[hit != A.NOT_LOOKED_UP], z[k + "hit_val"])
        np.testing.assert_array_equal(np.nonzero(~sent)[0], z[k + "not_sent"])
        assert (pl["kind"] == mosrx.FWD_DROP).sum() == 2


def test_fixture_is_small_and_data_only():
    assert os.path.getsize(GOLDEN) < 64 << 10
    z = load()
    assert all(z[k].dtype.kind in "uiV" for k in z.files)


@pytest.mark.skipif(not os.access(EXE, os.X_OK), reason="needs oracle/_ref/simple_firewall_emul (make -C oracle ref)")
@pytest.mark.parametrize("name", sorted(P.SCENARIOS))
def test_restatement_matches_the_sample(tmp_path, name):
    """The sample's printed rule table equals the restatement's per-rule counts, and its tx.pcap the
    restatement's sent frames, one for one."""
    make, text = P.SCENARIOS[name]
    frames = make()
    buf, off, ln, rec, rules, hit, cnt, pl, tx = P.restated(frames, text)
    # the runner, trace, table parser and pcap reader are test_simple_firewall's own, used as they are
    assert (P.SF.run_sample, P.SF.rule_table, P.SF.pcap_frames) == (run_sample, rule_table, pcap_frames)
    assert P.SCENARIOS["firewall"][0] is firewall_frames
    flows, acts, sent = P.run_sample(tmp_path, name, frames, text)
    # ... and the sample read the rules file meant for it (acl_pin.run_sample hands it over through SF.RULES)
    assert (tmp_path / name / "pp" / "fw.conf").read_text() == text
    assert flows == cnt[:len(rules)].tolist()
    assert acts == ["DROP" if a == mosrx.ACL_DROP else "ACCEPT" for a in rules["action"]]
    assert len(sent) == len(tx) and sent == tx
