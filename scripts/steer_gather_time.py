#!/usr/bin/env python3
"""Cost of the queue-major gather next to the steer pass it rides on and the
classify launch both follow.  The method of steer_time.py:

Two rows, each in one process on resident batches:
  S64_c8   the 64 B compact ring: 256 batches of 32K frames, 8-byte records
  M1500    the 1500 B row: 8 batches of 64K frames, 16-byte records

Per row, device time between events on the launch stream (ms per pass over the
row's batches, median of --repeats windows of --steps passes after a warm-up
pass of every shape), the three forms alternating within a repeat:
  classify                 mosrx_time_queue of the row's batch queue, nothing attached
  classify+steer           the same queue with steer outputs attached
                           (mosrx_queue_set_steer: the plain scatter pass)
  classify+steer+gather    ... with gather outputs attached
                           (mosrx_queue_set_steer_gather: records, offsets, lengths)
steer = classify+steer - classify; gather = classify+steer+gather - classify+steer.
Achieved rates are on the bytes of DESIGN §4.12: the steer pass moves
2 * rec_bytes + 4 B per frame, the gather adds 6 B read and rec_bytes + 6 B
written.  Not called by bench.py.

  python scripts/steer_gather_time.py [--steps K] [--repeats R] [--flows N] [--rows S64_c8,M1500]
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
FORMS = ("plain", "steer", "gather")


def row(ctx, key, steps, repeats, flows):
    kind, batch, ring, rings, compact = ROWS[key]
    rb = 8 if compact else 16
    t = mosrx.Trace(kind, batch, nflows=flows)
    dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
           for _ in range(ring * rings)]
    qs = [ctx.queue_ex(dbs[i:i + ring], compact=compact) for i in range(0, len(dbs), ring)]
    idx = [mosrx.DevBuffer(ctx, 4 * batch) for _ in dbs]
    qst = [mosrx.DevBuffer(ctx, 4 * mosrx.STEER_QSLOTS) for _ in dbs]
    qrec = [mosrx.DevBuffer(ctx, rb * batch) for _ in dbs]
    qoff = [mosrx.DevBuffer(ctx, 4 * batch) for _ in dbs]
    qlen = [mosrx.DevBuffer(ctx, 2 * batch) for _ in dbs]

    def attach(form):
        for k, q in enumerate(qs):
            sl = slice(k * ring, (k + 1) * ring)
            if form == "plain":
                q.set_steer(None, None)
            elif form == "steer":
                q.set_steer([b.ptr for b in idx[sl]], [b.ptr for b in qst[sl]])
            else:
                q.set_steer_gather(*[[b.ptr for b in arr[sl]] for arr in (idx, qst, qrec, qoff, qlen)])

    def queue_ms():
        return qs[0].time(steps, qs[1:], kernels=False)[0] / steps

    try:
        for f in FORMS:      # warm-up: every shape once
            attach(f)
            queue_ms()
        ctx.device_sync()
        ms = {f: [] for f in FORMS}
        for _ in range(repeats):
            for f in FORMS:
                attach(f)
                ms[f].append(queue_ms())
        attach("plain")
        keys = dbs[0].results8()["queue"] if compact else dbs[0].results()["queue"]
        c, s, g = (statistics.median(ms[f]) for f in FORMS)
        frames = batch * ring
        steer_bytes, gather_bytes = frames * (2 * rb + 4), frames * (rb + 12)
        steer_rate = steer_bytes / ((s - c) * 1e6) if s > c else None
        gather_rate = gather_bytes / ((g - s) * 1e6) if g > s else None
        return {
            "row": key, "frames_per_pass": frames, "batches": ring, "rec_bytes": rb, "flows": flows,
            "queues_used": int(len(set(keys.tolist()))), "steps": steps, "repeats": repeats,
            "classify_ms": round(c, 5), "classify_steer_ms": round(s, 5), "classify_steer_gather_ms": round(g, 5),
            "steer_ms": round(s - c, 5), "gather_ms": round(g - s, 5),
            "steer_share_of_classify": round((s - c) / c, 4), "gather_share_of_classify": round((g - s) / c, 4),
            "steer_GBps": round(steer_rate, 1) if steer_rate else None,
            "gather_GBps": round(gather_rate, 1) if gather_rate else None,
            "gather_rate_over_steer_rate": round(gather_rate / steer_rate, 3) if steer_rate and gather_rate else None,
            "classify_ms_all": [round(x, 5) for x in ms["plain"]],
            "classify_steer_ms_all": [round(x, 5) for x in ms["steer"]],
            "classify_steer_gather_ms_all": [round(x, 5) for x in ms["gather"]],
        }
    finally:
        for q in qs:
            q.destroy()
        for b in idx + qst + qrec + qoff + qlen + dbs:
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
