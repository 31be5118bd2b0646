"""Generate tests/golden/acl_firewall.npz: the firewall scenarios of tests/acl_pin.py
with what samples/simple_firewall ITSELF counted and sent for them.

Run where the reference build exists (oracle/_ref):
    make -C oracle ref && python tests/golden/make_golden_acl.py

"masks" (a few hundred frames) is stored whole: the packed frames, the records'
reason and tcp_flags, the rule fields (mosrx_acl_rule records), the hit per
frame, the counts per rule, the amended plan and the indices of the frames
sent.  "firewall" is test_simple_firewall's 10 046-frame trace, which that
module rebuilds from its seed: only the rule fields, the looked-up frames'
indices and hits, the counts and the indices of the frames NOT sent are stored.
The run refuses to write a fixture where the sample's printed rule table or its
tx.pcap differ from the restatement (tests/acl_oracle.py).  Only data.
"""
from __future__ import annotations

import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "mos-networking-stack_amd"))

import acl_pin as P  # noqa: E402
import fwd_oracle as F  # noqa: E402


def main():
    out = {}
    for name, (make, rules_text) in P.SCENARIOS.items():
        frames = make()
        buf, off, ln, rec, rules, hit, cnt, pl, tx = P.restated(frames, rules_text)
        flows, acts, sent = P.run_sample(pathlib.Path(tempfile.mkdtemp()), name, frames, rules_text)
        if flows != cnt[:len(rules)].tolist() or sent != tx:
            sys.exit(f"{name}: the sample counted {flows} and sent {len(sent)} frames; the restatement "
                     f"{cnt[:len(rules)].tolist()} and {len(tx)}, or their bytes differ")
        sent_mask = np.isin(pl["kind"], [F.IP, F.ETH])
        k = name + "__"
        out[k + "rules"] = rules
        out[k + "counts"] = cnt[:len(rules)]
        out[k + "n"] = np.array([len(off)], np.uint32)
        if name == "masks":
            out[k + "frames"], out[k + "off"], out[k + "len"] = buf, off, ln
            out[k + "reason"] = np.ascontiguousarray(rec["reason"])
            out[k + "tcp_flags"] = np.ascontiguousarray(rec["tcp_flags"])
            out[k + "hit"], out[k + "plan"] = hit, pl
            out[k + "tx_src"] = np.nonzero(sent_mask)[0].astype(np.uint32)
        else:
            out[k + "hit_idx"] = np.nonzero(hit != 0xFFFF)[0].astype(np.uint32)
            out[k + "hit_val"] = hit[hit != 0xFFFF]
            out[k + "not_sent"] = np.nonzero(~sent_mask)[0].astype(np.uint32)
        print(f"{name}: {len(off)} frames, {int((hit != 0xFFFF).sum())} looked up, counts {flows}, {len(sent)} sent")
    np.savez_compressed(os.path.join(HERE, "acl_firewall.npz"), **out)


if __name__ == "__main__":
    main()
