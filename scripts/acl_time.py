#!/usr/bin/env python3
"""Cost of the firewall launch (mosrx_queue_set_acl) inside the
queue form it is inserted into: device time between events on one stream, median
of 5 windows, the forms alternating in one run (scripts/fwd_time.py's method,
scripts/fwd_rings_time.py's rows and tables).

Per row, trace and window, one pass over all batches of
    queue                  mosrx_queue_run, nothing attached (the classify launch)
    queue+plan             ... with the plan attached
    queue+plan+desc        ... with plan and descriptor rings (what the parent runs)
    queue+plan+acl+desc    ... with the firewall launch between them
"acl alone" is the last less the third; "plan alone" the second less the first.
The traces: each row's own against 5 rules (the 64 B trace has next to no SYN, so
every workgroup ends after its records; the 1500 B trace's segments are nearly
all lone SYNs, so there every workgroup walks the five rules); and for the 64 B
row the same frames with TCP flags bytes turned into a lone SYN (checksum
adjusted) against 1024 rules none of which matches -- every frame (each lane
walks the whole table: the bounded worst case), and one frame in 256 (one
eligible lane a workgroup, which still copies the whole table into LDS).

    python scripts/acl_time.py [--windows 5] > profiles/acl/acl_time.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mos-networking-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402

import mosrx  # noqa: E402
from fwd_rings_time import ROWS, tables  # noqa: E402

RULES_5 = [("DROP", "10.5.0.0/24", "10.5.0.0/24", 0, 80), ("ACCEPT", "10.5.1.7", "10.5.1.9", 1024, 0),
           ("ACCEPT", "10.5.2.7", "10.5.2.9"), ("DROP", "10.5.3.0/24", "10.5.4.0/24"), ("DROP", "0.0.0.0", "10.10.10.10", 0, 22)]
# no frame of the generated traces comes from 203.0.113.0/24 port 7: none of these matches
RULES_1024 = [("DROP", f"203.0.113.{i % 250 + 1}", "0.0.0.0", 7, 1 + i) for i in range(1024)]


def all_syn(t, every=1):
    """The trace's frames with the flags byte of every `every`-th plain IPv4 / TCP frame made a lone SYN,
    the TCP checksum adjusted for the changed word (RFC 1624)."""
    buf = np.array(t.frames, np.uint8, copy=True)
    o = np.asarray(t.off).astype(np.int64)
    o = o[np.asarray(t.len) >= 54]
    o = o[(buf[o + 12] == 8) & (buf[o + 13] == 0) & (buf[o + 14] == 0x45) & (buf[o + 23] == 6)][::every]
    hi = buf[o + 46].astype(np.int64) << 8
    old, new = hi | buf[o + 47], hi | 0x02
    c = (buf[o + 50].astype(np.int64) << 8) | buf[o + 51]
    x = (~c & 0xFFFF) + (~old & 0xFFFF) + new
    x = (x & 0xFFFF) + (x >> 16)
    x = (x & 0xFFFF) + (x >> 16)
    c = ~x & 0xFFFF
    buf[o + 47] = 0x02
    buf[o + 50], buf[o + 51] = c >> 8, c & 0xFF
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch counts (a quick run)")
    a = ap.parse_args()
    print(f"# the firewall launch inside the descriptor queue form, median of {a.windows} windows, "
          "ms per pass over the row's batches")
    with mosrx.Context(0, mosrx.default_params(num_msp=1, forward=1)) as ctx:
        tab = tables(False)
        nrings = tab.num_netdevs
        ctx.fwd_set(tab)
        for row, (kind, n, nb, rb) in ROWS.items():
            nb = max(nb // a.scale, 1)
            tr = [mosrx.Trace(kind, n, seed=1 + i) for i in range(min(nb, 8))]
            cases = [("the row's own trace, 5 rules", 0, RULES_5)]
            if kind == mosrx.TRACE_S64:
                cases.append(("every TCP frame a SYN, 1024 rules, none matching", 1, RULES_1024))
                cases.append(("one TCP frame in 256 a SYN, 1024 rules, none matching", 256, RULES_1024))
            for what, syn, rules in cases:
                ctx.acl_set(rules)
                dbs = [ctx.upload(all_syn(t, syn) if syn else t.frames, t.off, t.len, frames_bytes=t.frames_bytes,
                                  max_len=t.max_len) for t in (tr[i % len(tr)] for i in range(nb))]
                bufs = [[mosrx.DevBuffer(ctx, sz(d.n)) for d in dbs] for sz in
                        (lambda m: 8 * m, lambda m: 4 * m, lambda m: 2 * m, lambda m: 12 * m, lambda m: 16 * nrings,
                         lambda m: 2 * m)]
                p = [[b.ptr for b in bs] for bs in bufs]
                cnt = mosrx.DevBuffer(ctx, 4 * mosrx.ACL_MAX_RULES)
                cnt.upload(np.zeros(mosrx.ACL_MAX_RULES, np.uint32))
                names = ("queue", "queue+plan", "queue+plan+desc", "queue+plan+acl+desc")
                qs = {k: ctx.queue_ex(dbs, compact=rb == 8) for k in names}
                qs["queue+plan"].set_fwd(p[0])
                qs["queue+plan+desc"].set_fwd_desc(p[0], None, nrings, p[1], p[2], p[3], p[4])
                qs["queue+plan+acl+desc"].set_fwd_desc(p[0], None, nrings, p[1], p[2], p[3], p[4])
                qs["queue+plan+acl+desc"].set_acl(p[5], cnt.ptr)
                for q in qs.values():
                    q.run()                                                             # warm up
                hit = bufs[5][0].download(np.zeros(dbs[0].n, np.uint16))
                looked, matched = int((hit != mosrx.ACL_NOT_LOOKED_UP).sum()), int((hit < len(rules)).sum())
                ms = {k: [] for k in qs}
                for _ in range(a.windows):
                    for k, q in qs.items():
                        ms[k].append(q.time(1, kernels=False)[0])
                med = {k: statistics.median(v) for k, v in ms.items()}
                acl = med["queue+plan+acl+desc"] - med["queue+plan+desc"]
                plan = med["queue+plan"] - med["queue"]
                print(f"\n{row}, {what}: {nb * n} frames in {nb} batches; batch 0: {looked} of {dbs[0].n} frames looked up, "
                      f"{matched} matched")
                for k, v in ms.items():
                    print(f"  {k:<20} median {med[k]:8.3f}  windows {' '.join(f'{x:.3f}' for x in v)}")
                print(f"  acl alone {acl:8.3f} ms   plan alone {plan:8.3f} ms   acl / plan {acl / plan:.2f}   "
                      f"classify + plan + acl + descriptors {nb * n / med['queue+plan+acl+desc'] / 1e3:8.1f} Mpps "
                      f"(without acl {nb * n / med['queue+plan+desc'] / 1e3:8.1f})")
                for q in qs.values():
                    q.destroy()
                for b in [b for bs in bufs for b in bs] + [cnt]:
                    b.free()
                for d in dbs:
                    d.free()


if __name__ == "__main__":
    main()
