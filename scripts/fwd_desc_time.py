#!/usr/bin/env python3
"""Cost of the descriptor form of the ring build (mosrx_queue_set_fwd_desc,
DESIGN.md §4.13) next to the byte-ring form it stands beside: device time
between events on one stream, median of 5 windows, the forms alternating in one
run (scripts/fwd_queue_time.py's method, rows and tables).

Per row and window, one pass over all batches of
    queue                  mosrx_queue_run, nothing attached (the classify launch)
    queue+plan             ... with the plan attached
    queue+plan+desc        ... with plan and the descriptor outputs attached
    queue+plan+rings       ... with plan and the byte rings attached (the yardstick)
"alone" is a form's median less queue+plan's.  By bytes the descriptor form
writes 18 B per sent frame (tx_src, tx_len, tx_mac) and reads 16 B of the frame;
the byte ring reads tx_len and writes the padded frame plus 10 B.

    python scripts/fwd_desc_time.py [--windows 5] > profiles/fwd/desc_time.txt
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch counts (a quick run)")
    a = ap.parse_args()
    print(f"# descriptor form against the byte-ring form over a batch queue, median of {a.windows} windows, "
          "ms per pass over the row's batches")
    with mosrx.Context(0, mosrx.default_params(num_msp=1, forward=1)) as ctx:
        for row, (kind, n, nb, rb) in ROWS.items():
            nb = max(nb // a.scale, 1)
            tr = [mosrx.Trace(kind, n, seed=1 + i) for i in range(min(nb, 8))]
            dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
                   for t in (tr[i % len(tr)] for i in range(nb))]
            for d in dbs:
                ctx.classify_dev(d, sync=False)
                if rb == 8:
                    ctx.classify_dev_compact(d, sync=False)
            for spread in (False, True):
                tab = tables(spread)
                nrings = tab.num_netdevs
                ctx.fwd_set(tab)
                plan = np.zeros(n, mosrx.FWD_DTYPE)
                tx_bytes = pad_bytes = sent = need = 0
                for i, d in enumerate(dbs[:len(tr)]):
                    ctx.time_op(mosrx.OP_FWD_PLAN, [d], 1, arg=rb, kernels=False)
                    d.d_fplan.download(plan)
                    s = np.isin(plan["kind"], [mosrx.FWD_IP, mosrx.FWD_ETH])
                    units = (plan["tx_len"][s].astype(np.int64) + 2 + 15) // 16
                    mult = len([j for j in range(nb) if j % len(tr) == i])
                    sent += int(s.sum()) * mult
                    tx_bytes += int(plan["tx_len"][s].astype(np.int64).sum()) * mult
                    pad_bytes += int(units.sum()) * 16 * mult
                    need = max(need, int(np.bincount(plan["out_ifidx"][s].astype(np.int64), weights=units,
                                                     minlength=nrings).max()))
                cap = need * 16
                bufs = [[mosrx.DevBuffer(ctx, sz(d.n)) for d in dbs] for sz in
                        (lambda m: 8 * m, lambda m: nrings * cap, lambda m: 4 * m, lambda m: 2 * m, lambda m: 4 * m,
                         lambda m: 16 * nrings, lambda m: 12 * m, lambda m: 16 * nrings)]
                p = [[b.ptr for b in bs] for bs in bufs]
                qs = {k: ctx.queue_ex(dbs, compact=rb == 8) for k in ("queue", "queue+plan", "queue+plan+desc",
                                                                        "queue+plan+rings")}
                qs["queue+plan"].set_fwd(p[0])
                qs["queue+plan+desc"].set_fwd_desc(p[0], None, nrings, p[4], p[3], p[6], p[7])
                qs["queue+plan+rings"].set_fwd(p[0], None, cap, nrings, p[1], p[2], p[3], p[4], p[5])
                for q in qs.values():
                    q.run()                                                             # warm up
                rd, rr = np.zeros(nrings, mosrx.FWD_RING_DTYPE), np.zeros(nrings, mosrx.FWD_RING_DTYPE)
                bufs[7][0].download(rd)
                bufs[5][0].download(rr)
                ms = {k: [] for k in qs}
                for _ in range(a.windows):
                    for k, q in qs.items():
                        ms[k].append(q.time(1, kernels=False)[0])
                med = {k: statistics.median(v) for k, v in ms.items()}
                desc, ring = med["queue+plan+desc"] - med["queue+plan"], med["queue+plan+rings"] - med["queue+plan"]
                print(f"\n{row}, {nrings} netdev{'s' if spread else ''}: {nb * n} frames in {nb} batches, {sent} sent, "
                      f"{tx_bytes / 1e6:.1f} MB of TX frames; batch 0 counts desc {rd['count'].tolist()} rings "
                      f"{rr['count'].tolist()}, units equal: {rd['units'].tolist() == rr['units'].tolist()}")
                for k, v in ms.items():
                    print(f"  {k:<20} median {med[k]:8.3f}  windows {' '.join(f'{x:.3f}' for x in v)}")
                print(f"  descriptor form alone {desc:8.3f} ms ({34 * sent / 1e6:.1f} MB read + written)   byte-ring form alone "
                      f"{ring:8.3f} ms ({(tx_bytes + pad_bytes + 10 * sent) / 1e6:.1f} MB)   desc / rings {desc / ring:.2f}")
                print(f"  classify + plan + descriptors {med['queue+plan+desc']:8.3f} ms "
                      f"{nb * n / med['queue+plan+desc'] / 1e3:8.1f} Mpps   classify + plan + byte rings "
                      f"{med['queue+plan+rings']:8.3f} ms {nb * n / med['queue+plan+rings'] / 1e3:8.1f} Mpps")
                for q in qs.values():
                    q.destroy()
                for b in (b for bs in bufs for b in bs):
                    b.free()
            for d in dbs:
                d.free()


if __name__ == "__main__":
    main()
