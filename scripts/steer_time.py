#!/usr/bin/env python3
"""Cost of queue steering next to the classify launch it follows.

Two rows, each in one process on resident batches:
  S64_c8   the 64 B compact ring: 256 batches of 32K frames, 8-byte records
  M1500    the 1500 B row: 8 batches of 64K frames, 16-byte records

Per row, device time between events on the launch stream (ms per pass over the
row's batches, median of --repeats after a warm-up pass of every shape):
  classify         mosrx_time_queue of the row's batch queue, nothing attached
  steer_op         MOSRX_OP_STEER (mosrx_time_op): the three steer launches per
                   batch, one batch after the other on one stream
  classify+steer   mosrx_time_queue of the same queue with steer outputs attached
                   (three launches over all batches behind the classify launch);
                   steer_queue = classify+steer - classify
The plain and the attached queue runs alternate within a repeat.  The context
maps onto 8 queues; the 1500 B trace carries --flows flows (1M: all 8 queues
used), the 64 B trace is config #2's single flow whatever --flows says (every
frame on one queue; `queues_used` in the output says which).  Not called by
bench.py.

  python scripts/steer_time.py [--steps K] [--repeats R] [--flows N] [--rows S64_c8,M1500]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mos-networking-stack_amd"))

import mosrx  # noqa: E402

ROWS = {
    # kind, frames per batch, batches per pass, rings resident, compact
    "S64_c8": (mosrx.TRACE_S64, 32_768, 256, 2, True),
    "M1500": (mosrx.TRACE_M1500, 65_536, 8, 1, False),
}
NQ = 8


def row(ctx, key, steps, repeats, flows):
    kind, batch, ring, rings, compact = ROWS[key]
    rb = 8 if compact else 16
    t = mosrx.Trace(kind, batch, nflows=flows)
    dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
           for _ in range(ring * rings)]
    qs = [ctx.queue_ex(dbs[i:i + ring], compact=compact) for i in range(0, len(dbs), ring)]
    idx = [mosrx.DevBuffer(ctx, 4 * batch) for _ in dbs]
    qst = [mosrx.DevBuffer(ctx, 4 * mosrx.STEER_QSLOTS) for _ in dbs]

    def attach(on):
        for k, q in enumerate(qs):
            lo = k * ring
            q.set_steer([b.ptr for b in idx[lo:lo + ring]] if on else None,
                        [b.ptr for b in qst[lo:lo + ring]] if on else None)

    def queue_ms():
        return qs[0].time(steps, qs[1:], kernels=False)[0] / steps

    def op_ms():
        return ctx.time_op(mosrx.OP_STEER, dbs, steps * ring, nstreams=1, arg=rb, kernels=False)[0] / steps

    try:
        # warm-up: every shape once (code objects loaded, records made, scratch allocated)
        attach(False)
        queue_ms()
        attach(True)
        queue_ms()
        op_ms()
        ctx.device_sync()
        plain, both, op = [], [], []
        for _ in range(repeats):
            attach(False)
            plain.append(queue_ms())
            attach(True)
            both.append(queue_ms())
            op.append(op_ms())
        attach(False)
        keys = dbs[0].results8()["queue"] if compact else dbs[0].results()["queue"]
        c, b, o = statistics.median(plain), statistics.median(both), statistics.median(op)
        frames = batch * ring
        return {
            "row": key, "frames_per_pass": frames, "batches": ring, "rec_bytes": rb, "flows": flows,
            "queues_used": int(len(set(keys.tolist()))), "steps": steps, "repeats": repeats,
            "classify_ms": round(c, 5), "classify_steer_ms": round(b, 5), "steer_queue_ms": round(b - c, 5),
            "steer_op_ms": round(o, 5),
            "steer_queue_share_of_classify": round((b - c) / c, 4), "steer_op_share_of_classify": round(o / c, 4),
            "steer_queue_GBps": round(frames * (2 * rb + 4) / ((b - c) * 1e6), 1) if b > c else None,
            "classify_ms_all": [round(x, 5) for x in plain],
            "classify_steer_ms_all": [round(x, 5) for x in both],
            "steer_op_ms_all": [round(x, 5) for x in op],
        }
    finally:
        for q in qs:
            q.destroy()
        for b in idx + qst + dbs:
            b.free()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="passes over the row's batches per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--flows", type=int, default=1_000_000)
    ap.add_argument("--rows", default="S64_c8,M1500")
    a = ap.parse_args()
    with mosrx.Context(0, mosrx.default_params(num_queues=NQ)) as ctx:
        for key in a.rows.split(","):
            print(json.dumps(row(ctx, key, a.steps, a.repeats, a.flows)), flush=True)


if __name__ == "__main__":
    main()
