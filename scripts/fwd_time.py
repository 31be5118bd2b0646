#!/usr/bin/env python3
"""Cost of the forwarding path: device time between events on
one stream, median of 5 windows, the forms alternating in one run.

Rows: the 1500 B row (8 batches of 64K frames) and the 64 B ring (256 batches
of 32K frames; the plan and build read 8-byte records there).  Per row and
window, one pass over all batches of
    classify                      MOSRX_OP_CLASSIFY (16-byte records)
    plan                          MOSRX_OP_FWD_PLAN
    plan + build                  MOSRX_OP_FWD
    memcpy                        a device-to-device copy of the bytes the build moves
and from their medians: classify, classify + plan, classify + plan + build,
the build alone (plan + build minus plan) and its rate on its algorithmic bytes
(tx_len read + padded tx_len + 11 written per sent frame) next to the copy's
(bytes read + bytes written).  Every frame of both rows is forwarded
(TCP_OK, one monitor, forward = 1); `--tables walk` plans through the route and
ARP walks (4 + 4 entries), `nicfwd` through the nic_forward_table.

    python scripts/fwd_time.py [--windows 5] [--tables walk] > profiles/fwd/fwd_time.txt
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
QUARTERS = [(f"{a}.0.0.0/2", "02:00:00:00:00:aa") for a in (0, 64, 128, 192)]


def copy_ms(torch, nbytes):
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def once():
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    once()
    return once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--tables", choices=("walk", "nicfwd"), default="walk")
    ap.add_argument("--scale", type=int, default=1, help="divide the batch counts (a quick run)")
    a = ap.parse_args()
    import torch
    tab = (mosrx.fwd_tables(routes=[(c, 0) for c, _ in QUARTERS], arp=QUARTERS, netdevs=["02:00:00:00:00:01"])
           if a.tables == "walk" else mosrx.fwd_tables(netdevs=["02:00:00:00:00:01"], nic_fwd={0: 0}))
    print(f"# forwarding cost, tables={a.tables}, median of {a.windows} windows, ms per pass over the row's batches")
    with mosrx.Context(0, mosrx.default_params(num_msp=1, forward=1)) as ctx:
        ctx.fwd_set(tab)
        for row, (kind, n, nb, rb) in ROWS.items():
            nb = max(nb // a.scale, 1)
            tr = [mosrx.Trace(kind, n, seed=1 + i) for i in range(min(nb, 8))]
            dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
                   for t in (tr[i % len(tr)] for i in range(nb))]
            for d in dbs:
                ctx.classify_dev(d, sync=False)
                if rb == 8:
                    ctx.classify_dev_compact(d, sync=False)
            ctx.time_op(mosrx.OP_FWD, dbs[:1], 1, arg=rb, kernels=False)           # allocate, warm up
            plan = np.zeros(n, mosrx.FWD_DTYPE)
            tx_bytes = pad_bytes = sent = 0
            for i, d in enumerate(dbs[:len(tr)]):
                ctx.time_op(mosrx.OP_FWD_PLAN, [d], 1, arg=rb, kernels=False)
                d.d_fplan.download(plan)
                s = np.isin(plan["kind"], [mosrx.FWD_IP, mosrx.FWD_ETH])
                mult = len([j for j in range(nb) if j % len(tr) == i])
                sent += int(s.sum()) * mult
                tx_bytes += int(plan["tx_len"][s].astype(np.int64).sum()) * mult
                pad_bytes += int(((plan["tx_len"][s].astype(np.int64) + 2 + 15) // 16 * 16).sum()) * mult
            algo = tx_bytes + pad_bytes + 11 * sent
            copy = copy_ms(torch, tx_bytes)
            forms = {"classify": (mosrx.OP_CLASSIFY, 0), "plan": (mosrx.OP_FWD_PLAN, rb), "plan+build": (mosrx.OP_FWD, rb)}
            ms = {k: [] for k in list(forms) + ["memcpy"]}
            for _ in range(a.windows):
                for k, (op, arg) in forms.items():
                    ms[k].append(ctx.time_op(op, dbs, len(dbs), arg=arg, kernels=False)[0])
                ms["memcpy"].append(copy())
            med = {k: statistics.median(v) for k, v in ms.items()}
            build = med["plan+build"] - med["plan"]
            print(f"\n{row}: {nb * n} frames, {sent} sent, {tx_bytes / 1e6:.1f} MB of TX frames")
            for k, v in ms.items():
                print(f"  {k:<12} median {med[k]:8.3f}  windows {' '.join(f'{x:.3f}' for x in v)}")
            print(f"  classify                 {med['classify']:8.3f} ms  {nb * n / med['classify'] / 1e3:8.1f} Mpps")
            print(f"  classify + plan          {med['classify'] + med['plan']:8.3f} ms")
            print(f"  classify + plan + build  {med['classify'] + med['plan+build']:8.3f} ms  "
                  f"{nb * n / (med['classify'] + med['plan+build']) / 1e3:8.1f} Mpps")
            print(f"  build alone              {build:8.3f} ms  {algo / build / 1e6:8.1f} GB/s on {algo / 1e6:.1f} MB")
            print(f"  memcpy d2d               {med['memcpy']:8.3f} ms  {2 * tx_bytes / med['memcpy'] / 1e6:8.1f} GB/s "
                  f"on {2 * tx_bytes / 1e6:.1f} MB (read + written)")
            print(f"  build rate / copy rate   {(algo / build) / (2 * tx_bytes / med['memcpy']):.2f}")
            for d in dbs:
                d.free()


if __name__ == "__main__":
    main()
