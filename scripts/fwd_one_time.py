#!/usr/bin/env python3
"""The one-launch forwarding form against the four launches.

Part A, device rows: MOSRX_OP_FWD_DESC (plan + descriptor rings) through
mosrx_time_op, batch by batch on one stream, device time between events, median
of --repeats windows.  Within every repeat the limit is set to 0 (the four
launches: the code as it was) and then to MOSRX_FWD_ONE_MAX (the one launch),
so both columns come from one run.  64 B and 1500 B frames, 16-byte records,
n = 256 .. 8192, scripts/fwd_rings_time.py's spread tables (four netdevs).

Part B, group rows: one direct group (a single batch of 64 B frames, every
output pinned) submitted and waited in a loop, host time submit -> outputs
visible: nothing armed, mosrx_slot_fwd armed with the limit off (four launches)
and on (one), and the last two again with a mosrx_slot_steer_gather arm under
mosrx_set_steer_one -- eight dispatches a group against three.

  python scripts/fwd_one_time.py [--steps K] [--repeats R] > profiles/fwd/one_time.txt
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mos-networking-stack_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import mosrx  # noqa: E402
from fwd_rings_time import tables  # noqa: E402

SIZES = (256, 1024, 2048, 4096, 8192)
NBATCH = 8
MAX = mosrx.FWD_ONE_MAX


def med(xs, nd=3):
    return round(statistics.median(xs), nd)


def device_row(ctx, kind, name, n, steps, repeats):
    trs = [mosrx.Trace(kind, n, seed=1 + i) for i in range(NBATCH)]
    dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len) for t in trs]
    try:
        for d in dbs:
            ctx.classify_dev(d)

        def us(limit):
            ctx.set_fwd_one(limit)
            c0 = ctx.fwd_one_count()
            ms = ctx.time_op(mosrx.OP_FWD_DESC, dbs, steps * NBATCH, nstreams=1, arg=16, kernels=False)[0]
            assert (ctx.fwd_one_count() > c0) == (limit != 0)
            return ms * 1e3 / (steps * NBATCH)
        us(0), us(MAX)                                            # warm-up: both forms' code objects, the buffers
        four, one = [], []
        for _ in range(repeats):
            four.append(us(0))
            one.append(us(MAX))
        return {"frames": name, "n": n, "steps": steps, "repeats": repeats, "four_launch_us": med(four), "one_launch_us": med(one),
                "one_faster_in_every_window": bool(max(one) < min(four)),
                "four_all": [round(x, 3) for x in four], "one_all": [round(x, 3) for x in one]}
    finally:
        ctx.set_fwd_one(0)
        for d in dbs:
            d.free()


def group_row(ctx, n, steps, repeats):
    t = mosrx.Trace(mosrx.TRACE_S64, n, nflows=100_000)
    frees = []

    def pinned(dtype, k):
        p, a = ctx.host_alloc(max(k, 1) * np.dtype(dtype).itemsize)
        frees.append(p)
        return a.view(dtype)[:k]

    try:
        fb = t.frames_bytes
        fa = (fb + 15) & ~15
        base, blk = ctx.host_alloc(fa + 6 * n + 256)
        frees.append(base)
        blk[:fb] = t.frames[:fb]
        blk[fa:fa + 4 * n].view(np.uint32)[:] = t.off
        blk[fa + 4 * n:fa + 6 * n].view(np.uint16)[:] = t.len
        batches = [mosrx.Batch(base, fb, base + fa, base + fa + 4 * n, n, int(t.len.max()))]
        rec = pinned(mosrx.RESULT8_DTYPE, n)
        souts = [[a.ctypes.data] for a in (pinned(np.uint32, n), pinned(np.uint32, mosrx.STEER_QSLOTS),
                                           pinned(np.uint8, 8 * n), pinned(np.uint32, n), pinned(np.uint16, n))]
        fouts = [[a.ctypes.data] for a in (pinned(np.uint32, n), pinned(np.uint16, n), pinned(np.uint32, 3 * n),
                                           pinned(mosrx.FWD_RING_DTYPE, 4), pinned(np.uint64, n))]
        ctx.set_direct(1 << 30)

        def us(fwd, limit, steer):
            ctx.set_fwd_one(limit)
            ctx.set_steer_one(2048 if steer and n <= 2048 else mosrx.STEER_ONE_MAX if steer else 0)
            c0 = ctx.fwd_one_count()
            t0 = time.perf_counter()
            for _ in range(steps):
                if steer:
                    ctx.slot_steer_gather(1, *souts)
                if fwd:
                    ctx.slot_fwd(1, fouts[0], fouts[1], fouts[2], fouts[3], nrings=4, plan=fouts[4])
                ctx.group_submit_c8(1, batches, [rec.ctypes.data])
                ctx.group_wait(1)
            dt = time.perf_counter() - t0
            assert ctx.slot_direct(1) and ctx.fwd_one_count() - c0 == (steps if fwd and limit else 0)
            return dt * 1e6 / steps
        forms = {"plain": (False, 0, False), "fwd_four": (True, 0, False), "fwd_one": (True, MAX, False),
                 "steer_one+fwd_four": (True, 0, True), "steer_one+fwd_one": (True, MAX, True)}
        for f in forms.values():
            us(*f)
        got = {k: [] for k in forms}
        for _ in range(repeats):
            for k, f in forms.items():
                got[k].append(us(*f))
        out = {"direct_group_frames": n, "steps": steps, "repeats": repeats}
        for k in forms:
            out[k + "_us"] = med(got[k], 2)
        out["all"] = {k: [round(x, 2) for x in v] for k, v in got.items()}
        return out
    finally:
        ctx.set_fwd_one(0)
        ctx.set_steer_one(0)
        ctx.set_direct(0)
        for p in frees:
            ctx.host_free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="passes (device rows: over 8 batches) per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    with mosrx.Context(0, mosrx.default_params(num_msp=1, forward=1, num_queues=8)) as ctx:
        ctx.fwd_set(tables(True))
        rows = []
        for kind, name in ((mosrx.TRACE_S64, "64B"), (mosrx.TRACE_M1500, "1500B")):
            for n in SIZES:
                rows.append(device_row(ctx, kind, name, n, a.steps, a.repeats))
                print(json.dumps(rows[-1]), flush=True)
        for name in ("64B", "1500B"):
            ok = [r["n"] for r in rows if r["frames"] == name and r["one_faster_in_every_window"]]
            # the limit worth setting: the largest size up to which the one launch won every window at every size
            run = [n for n in SIZES if all(m in ok for m in SIZES if m <= n)]
            print(json.dumps({"frames": name, "sizes_one_launch_faster_in_every_window": ok,
                              "limit_worth_setting": max(run) if run else 0}), flush=True)
        for n in (256, 4096):
            print(json.dumps(group_row(ctx, n, a.steps * 5, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
