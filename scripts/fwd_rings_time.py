#!/usr/bin/env python3
"""Cost of the ring form of the forwarding build next to the
arrival-order build: device time between events on one stream, median of 5
windows, the forms alternating in one run.

Rows: the 1500 B row (8 batches of 64K frames) and the 64 B ring (256 batches
of 32K frames, 8-byte records).  Per row and window, one pass over all batches of
    classify                      MOSRX_OP_CLASSIFY (16-byte records)
    plan                          MOSRX_OP_FWD_PLAN
    plan + build                  MOSRX_OP_FWD        (the arrival-order build: the yardstick)
    plan + ring build             MOSRX_OP_FWD_RINGS  (nrings = the tables' num_netdevs)
Each row runs twice: every frame routed to one netdev (one ring), and the frames
spread over 4 netdevs by the low two bits of the destination address.  Every
frame of both rows is forwarded (TCP_OK, one monitor, forward = 1).  The 64 B
trace has one destination address: its 4-netdev pass is 4 rings with every
frame in one of them (the "per ring" counts printed with each pass say so).

    python scripts/fwd_rings_time.py [--windows 5] > profiles/fwd/rings_time.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mos-networking-stack_amd"))

import numpy as np  # noqa: E402

import mosrx  # noqa: E402

ROWS = {"M1500 8x64K": (mosrx.TRACE_M1500, 65536, 8, 16), "S64 256x32K c8": (mosrx.TRACE_S64, 32768, 256, 8)}
ANY = [(f"{a}.0.0.0/2", "02:00:00:00:00:aa") for a in (0, 64, 128, 192)]


def tables(spread):
    devs = [f"02:00:00:00:00:{i + 1:02x}" for i in range(4 if spread else 1)]
    t = mosrx.fwd_tables(routes=[("0.0.0.0/0", q) for q in range(len(devs))], arp=ANY, netdevs=devs)
    for q in range(len(devs)) if spread else ():
        # route q: the destination's last octet has low bits q (the address as mOS loads it: that octet is the top byte)
        t.routes[q].mask, t.routes[q].masked_ip, t.routes[q].prefix = 0x03000000, q << 24, 2
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch counts (a quick run)")
    a = ap.parse_args()
    print(f"# ring build against the arrival-order build, median of {a.windows} windows, ms per pass over the row's batches")
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
                ctx.fwd_set(tab)
                ctx.time_op(mosrx.OP_FWD_RINGS, dbs[:1], 1, arg=rb, kernels=False)      # allocate, warm up
                ctx.time_op(mosrx.OP_FWD, dbs[:1], 1, arg=rb, kernels=False)
                plan = np.zeros(n, mosrx.FWD_DTYPE)
                dbs[0].d_fplan.download(plan)
                s = np.isin(plan["kind"], [mosrx.FWD_IP, mosrx.FWD_ETH])
                per = np.bincount(plan["out_ifidx"][s].astype(np.int64), minlength=tab.num_netdevs).tolist()
                forms = {"classify": (mosrx.OP_CLASSIFY, 0), "plan": (mosrx.OP_FWD_PLAN, rb),
                         "plan+build": (mosrx.OP_FWD, rb), "plan+rings": (mosrx.OP_FWD_RINGS, rb)}
                ms = {k: [] for k in forms}
                for _ in range(a.windows):
                    for k, (op, arg) in forms.items():
                        ms[k].append(ctx.time_op(op, dbs, len(dbs), arg=arg, kernels=False)[0])
                med = {k: statistics.median(v) for k, v in ms.items()}
                build, rings = med["plan+build"] - med["plan"], med["plan+rings"] - med["plan"]
                print(f"\n{row}, {tab.num_netdevs} netdev{'s' if spread else ''}: {nb * n} frames, "
                      f"batch 0 sends {int(s.sum())} of {n}, per ring {per}")
                for k, v in ms.items():
                    print(f"  {k:<12} median {med[k]:8.3f}  windows {' '.join(f'{x:.3f}' for x in v)}")
                print(f"  classify + plan                {med['classify'] + med['plan']:8.3f} ms")
                print(f"  classify + plan + build        {med['classify'] + med['plan+build']:8.3f} ms  "
                      f"{nb * n / (med['classify'] + med['plan+build']) / 1e3:8.1f} Mpps")
                print(f"  classify + plan + ring build   {med['classify'] + med['plan+rings']:8.3f} ms  "
                      f"{nb * n / (med['classify'] + med['plan+rings']) / 1e3:8.1f} Mpps")
                print(f"  build alone {build:8.3f} ms   ring build alone {rings:8.3f} ms   ring / arrival-order {rings / build:.2f}")
            for d in dbs:
                d.free()


if __name__ == "__main__":
    main()
