#!/usr/bin/env python3
"""The one-launch steer form against the three launches.

Device rows: MOSRX_OP_STEER, _GATHER and _GATHER_SIDE (all three side arrays)
through mosrx_time_op, batch by batch on one stream, device time between events,
median of --repeats windows.  Within every repeat the limit is set to 0 (the
three launches: the code as it was) and then to MOSRX_STEER_ONE_MAX (the one
launch), so both columns come from one run.  8-byte records of 64 B frames at
n = 256 .. 32768, 16-byte records of IMIX frames at 2048 and 8192.

Group rows: one direct group (a single batch of 64 B frames, every output
pinned) armed with mosrx_slot_steer_gather_side (records, descriptors, flow
hashes), submitted and waited in a loop; host time submit -> outputs visible,
limit off against limit on, alternating the same way.  `plain` is the same
group with nothing armed.

  python scripts/steer_one_time.py [--steps K] [--repeats R] > profiles/steer/one_time.txt
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

import mosrx  # noqa: E402

NQ = 8
OPS = (("steer", mosrx.OP_STEER, 0), ("gather", mosrx.OP_STEER_GATHER, 0),
       ("gather_side", mosrx.OP_STEER_GATHER_SIDE, (mosrx.SIDE_FHASH | mosrx.SIDE_MATCH | mosrx.SIDE_TCPINFO) << 8))
DEVICE_ROWS = [(mosrx.TRACE_S64, n, 8) for n in (256, 1024, 2048, 4096, 8192, 16384, 32768)] + \
              [(mosrx.TRACE_IMIX, 2048, 16), (mosrx.TRACE_IMIX, 8192, 16)]
NBATCH = 8


def device_row(ctx, kind, n, rb, steps, repeats):
    t = mosrx.Trace(kind, n, nflows=100_000)
    dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len) for _ in range(NBATCH)]
    try:
        for d in dbs:
            ctx.classify_dev(d)
            ctx.classify_dev_compact(d)
        keys = (dbs[0].results8() if rb == 8 else dbs[0].results())["queue"]
        out = {"rec_bytes": rb, "n": n, "queues_used": int(len(set(keys.tolist()))), "steps": steps, "repeats": repeats}
        for name, op, bits in OPS:
            def us(limit):
                ctx.set_steer_one(limit)
                ms = ctx.time_op(op, dbs, steps * NBATCH, nstreams=1, arg=rb | bits, kernels=False)[0]
                return ms * 1e3 / (steps * NBATCH)
            us(0), us(mosrx.STEER_ONE_MAX)                      # warm-up: both forms' code objects, the scratch
            three, one = [], []
            for _ in range(repeats):
                three.append(us(0))
                one.append(us(mosrx.STEER_ONE_MAX))
            out[name] = {"three_launch_us": round(statistics.median(three), 3), "one_launch_us": round(statistics.median(one), 3),
                         "three_all": [round(x, 3) for x in three], "one_all": [round(x, 3) for x in one]}
        return out
    finally:
        ctx.set_steer_one(0)
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
        rec, fh = pinned(mosrx.RESULT8_DTYPE, n), pinned(np.uint32, n)
        outs = [[a.ctypes.data] for a in (pinned(np.uint32, n), pinned(np.uint32, mosrx.STEER_QSLOTS),
                                          pinned(np.uint8, 8 * n), pinned(np.uint32, n), pinned(np.uint16, n),
                                          pinned(np.uint32, n))]
        ctx.set_direct(1 << 30)

        def us(limit, armed=True):
            ctx.set_steer_one(limit)
            t0 = time.perf_counter()
            for _ in range(steps):
                if armed:
                    ctx.slot_steer_gather_side(1, *outs, None, None)
                ctx.group_submit_c8(1, batches, [rec.ctypes.data], [fh.ctypes.data])
                ctx.group_wait(1)
            dt = time.perf_counter() - t0
            assert ctx.slot_direct(1)
            return dt * 1e6 / steps

        us(0), us(mosrx.STEER_ONE_MAX), us(0, False)
        three, one, plain = [], [], []
        for _ in range(repeats):
            plain.append(us(0, False))
            three.append(us(0))
            one.append(us(mosrx.STEER_ONE_MAX))
        return {"direct_group_frames": n, "steps": steps, "repeats": repeats,
                "plain_us": round(statistics.median(plain), 2), "three_launch_us": round(statistics.median(three), 2),
                "one_launch_us": round(statistics.median(one), 2),
                "three_all": [round(x, 2) for x in three], "one_all": [round(x, 2) for x in one]}
    finally:
        ctx.set_steer_one(0)
        ctx.set_direct(0)
        for p in frees:
            ctx.host_free(p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="passes (device rows: over 8 batches) per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    with mosrx.Context(0, mosrx.default_params(num_queues=NQ)) as ctx:
        rows = []
        for kind, n, rb in DEVICE_ROWS:
            rows.append(device_row(ctx, kind, n, rb, a.steps, a.repeats))
            print(json.dumps(rows[-1]), flush=True)
        for name, _, _ in OPS:
            ok = [r["n"] for r in rows if r["rec_bytes"] == 8 and r[name]["one_launch_us"] <= r[name]["three_launch_us"]]
            print(json.dumps({"op": name, "rec_bytes": 8, "largest_n_one_launch_no_slower": max(ok) if ok else None}),
                  flush=True)
        for n in (256, 4096):
            print(json.dumps(group_row(ctx, n, a.steps * 5, a.repeats)), flush=True)


if __name__ == "__main__":
    main()
