#!/usr/bin/env python3
"""Cost of forwarding over a whole batch queue (mosrx_queue_set_fwd, DESIGN.md
§4.13) next to the batch-by-batch forms: device time between events on one
stream, median of 5 windows, the forms alternating in one run.

Rows: the 1500 B row (8 batches of 64K frames) and the 64 B ring (256 batches
of 32K frames, 8-byte records), each with every frame routed to one netdev and
with the frames spread over 4 netdevs (scripts/fwd_rings_time.py's tables).
Per row and window, one pass over all batches of
    queue                         mosrx_queue_run, nothing attached (the classify launch)
    queue+plan                    ... with the plan attached            (1 more launch)
    queue+plan+rings              ... with plan and TX rings attached   (4 more launches)
    plan by batch                 MOSRX_OP_FWD_PLAN   (nb launches: the yardstick)
    plan+rings by batch           MOSRX_OP_FWD_RINGS  (4 nb launches: the yardstick)
    memcpy                        a device-to-device copy of the bytes the build moves
The build's own bytes are tx_len read + padded tx_len + 10 written (tx_off,
tx_len, tx_src) per sent frame.

    python scripts/fwd_queue_time.py [--windows 5] > profiles/fwd/queue_time.txt
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
from fwd_time import copy_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch counts (a quick run)")
    a = ap.parse_args()
    import torch
    print(f"# forwarding over a batch queue against batch by batch, median of {a.windows} windows, "
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
                ctx.time_op(mosrx.OP_FWD_RINGS, dbs[:1], 1, arg=rb, kernels=False)      # allocate, warm up
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
                algo = tx_bytes + pad_bytes + 10 * sent
                cap = need * 16
                bufs = [[mosrx.DevBuffer(ctx, sz(d.n)) for d in dbs] for sz in
                        (lambda m: 8 * m, lambda m: nrings * cap, lambda m: 4 * m, lambda m: 2 * m, lambda m: 4 * m,
                         lambda m: 16 * nrings)]
                ptrs = [[b.ptr for b in bs] for bs in bufs]
                qs = {"queue": ctx.queue_ex(dbs, compact=rb == 8), "queue+plan": ctx.queue_ex(dbs, compact=rb == 8),
                      "queue+plan+rings": ctx.queue_ex(dbs, compact=rb == 8)}
                qs["queue+plan"].set_fwd(ptrs[0])
                qs["queue+plan+rings"].set_fwd(ptrs[0], None, cap, nrings, *ptrs[1:])
                ops = {"plan by batch": (mosrx.OP_FWD_PLAN, rb), "plan+rings by batch": (mosrx.OP_FWD_RINGS, rb)}
                for q in qs.values():
                    q.run()                                                             # warm up
                rings = np.zeros(nrings, mosrx.FWD_RING_DTYPE)
                bufs[5][0].download(rings)
                copy = copy_ms(torch, tx_bytes)
                ms = {k: [] for k in list(qs) + list(ops) + ["memcpy"]}
                for _ in range(a.windows):
                    for k, q in qs.items():
                        ms[k].append(q.time(1, kernels=False)[0])
                    for k, (op, arg) in ops.items():
                        ms[k].append(ctx.time_op(op, dbs, len(dbs), arg=arg, kernels=False)[0])
                    ms["memcpy"].append(copy())
                med = {k: statistics.median(v) for k, v in ms.items()}
                qplan, qbuild = med["queue+plan"] - med["queue"], med["queue+plan+rings"] - med["queue+plan"]
                bplan, bbuild = med["plan by batch"], med["plan+rings by batch"] - med["plan by batch"]
                copy_rate = 2 * tx_bytes / med["memcpy"]
                print(f"\n{row}, {nrings} netdev{'s' if spread else ''}: {nb * n} frames in {nb} batches, {sent} sent, "
                      f"{tx_bytes / 1e6:.1f} MB of TX frames, ring_cap {cap}; batch 0 rings: count "
                      f"{rings['count'].tolist()} dropped {rings['dropped'].tolist()}")
                for k, v in ms.items():
                    print(f"  {k:<20} median {med[k]:8.3f}  windows {' '.join(f'{x:.3f}' for x in v)}")
                print(f"  plan alone        queue {qplan:8.3f} ms   by batch {bplan:8.3f} ms   queue / by batch {qplan / bplan:.2f}")
                print(f"  ring build alone  queue {qbuild:8.3f} ms   by batch {bbuild:8.3f} ms   queue / by batch {qbuild / bbuild:.2f}")
                print(f"  classify + plan + ring build  queue {med['queue+plan+rings']:8.3f} ms "
                      f"{nb * n / med['queue+plan+rings'] / 1e3:8.1f} Mpps   by batch "
                      f"{med['queue'] + med['plan+rings by batch']:8.3f} ms "
                      f"{nb * n / (med['queue'] + med['plan+rings by batch']) / 1e3:8.1f} Mpps")
                print(f"  memcpy d2d        {med['memcpy']:8.3f} ms  {copy_rate / 1e6:8.1f} GB/s on {2 * tx_bytes / 1e6:.1f} MB "
                      "(read + written)")
                print(f"  build on its own {algo / 1e6:.1f} MB: queue {algo / qbuild / 1e6:8.1f} GB/s = "
                      f"{algo / qbuild / copy_rate:.2f} of the copy's rate   by batch {algo / bbuild / 1e6:8.1f} GB/s = "
                      f"{algo / bbuild / copy_rate:.2f}")
                for q in qs.values():
                    q.destroy()
                for b in (b for bs in bufs for b in bs):
                    b.free()
            for d in dbs:
                d.free()


if __name__ == "__main__":
    main()
