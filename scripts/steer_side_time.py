#!/usr/bin/env python3
"""Cost of the gather's side form next to the gather it rides on (DESIGN.md
§4.12).  The method of steer_gather_time.py: two rows, each in one process on
resident batches,
  S64_c8   the 64 B compact ring: 256 batches of 32K frames, 8-byte records
  M1500    the 1500 B row: 8 batches of 64K frames, 16-byte records
device time between events on the launch stream, ms per pass over the row's
batches, median of --repeats windows of --steps passes after a warm-up pass of
every shape, the forms alternating within a repeat.

Part A, behind the classify launch (the row's batch queue, made with flow
hashes): classify | +steer | +steer+gather | +steer+gather+fhash
(mosrx_queue_set_steer_gather_side).  gather = the third minus the second, the
column of steer_gather_time.py, through the same kernel instantiation;
side(fhash) = the fourth minus the third.

Part B, the steer launches alone over the records part A left (mosrx_time_op:
MOSRX_OP_STEER_GATHER against MOSRX_OP_STEER_GATHER_SIDE with fhash only, match
only, all three): the batch queue makes no pkt_info, so the 12-byte array is
measured here, with the two u32 arrays beside it for comparison with part A.

Rates are on each form's own added bytes: 8 B per frame (4 read, 4 written) for
a u32 array, 24 B for tcpinfo; the yardstick is the record gather's rate on its
own rec_bytes + 12 B in the same run.  Not called by bench.py.

  python scripts/steer_side_time.py [--steps K] [--repeats R] [--flows N] [--rows S64_c8,M1500]
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
QFORMS = ("plain", "steer", "gather", "gather_fhash")
OFORMS = {"gather": None, "fhash": mosrx.SIDE_FHASH, "match": mosrx.SIDE_MATCH,
          "all": mosrx.SIDE_FHASH | mosrx.SIDE_MATCH | mosrx.SIDE_TCPINFO}
SIDE_BYTES = {"fhash": 8, "match": 8, "all": 40}


def rate(nbytes, ms):
    return round(nbytes / (ms * 1e6), 1) if ms > 0 else None


def row(ctx, key, steps, repeats, flows):
    kind, batch, ring, rings, compact = ROWS[key]
    rb = 8 if compact else 16
    t = mosrx.Trace(kind, batch, nflows=flows)
    dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
           for _ in range(ring * rings)]
    qs = [ctx.queue_ex(dbs[i:i + ring], flow_hash=True, compact=compact) for i in range(0, len(dbs), ring)]
    idx = [mosrx.DevBuffer(ctx, 4 * batch) for _ in dbs]
    qst = [mosrx.DevBuffer(ctx, 4 * mosrx.STEER_QSLOTS) for _ in dbs]
    qrec = [mosrx.DevBuffer(ctx, rb * batch) for _ in dbs]
    qoff = [mosrx.DevBuffer(ctx, 4 * batch) for _ in dbs]
    qlen = [mosrx.DevBuffer(ctx, 2 * batch) for _ in dbs]
    qfh = [mosrx.DevBuffer(ctx, 4 * batch) for _ in dbs]

    def attach(form):
        for k, q in enumerate(qs):
            sl = slice(k * ring, (k + 1) * ring)
            if form == "plain":
                q.set_steer(None, None)
            elif form == "steer":
                q.set_steer([b.ptr for b in idx[sl]], [b.ptr for b in qst[sl]])
            elif form == "gather":
                q.set_steer_gather(*[[b.ptr for b in arr[sl]] for arr in (idx, qst, qrec, qoff, qlen)])
            else:
                q.set_steer_gather_side(*[[b.ptr for b in arr[sl]] for arr in (idx, qst, qrec, qoff, qlen, qfh)])

    def queue_ms():
        return qs[0].time(steps, qs[1:], kernels=False)[0] / steps

    def op_ms(which):
        op = mosrx.OP_STEER_GATHER if which is None else mosrx.OP_STEER_GATHER_SIDE
        arg = rb if which is None else rb | which << 8
        return ctx.time_op(op, dbs[:ring], steps * ring, nstreams=1, arg=arg, kernels=False)[0] / steps

    try:
        for f in QFORMS:     # warm-up: every shape once (and the records part B reads)
            attach(f)
            queue_ms()
        attach("plain")
        for w in OFORMS.values():
            op_ms(w)
        ctx.device_sync()
        ms = {f: [] for f in QFORMS}
        for _ in range(repeats):
            for f in QFORMS:
                attach(f)
                ms[f].append(queue_ms())
        attach("plain")
        oms = {f: [] for f in OFORMS}
        for _ in range(repeats):
            for f, w in OFORMS.items():
                oms[f].append(op_ms(w))
        c, s, g, gf = (statistics.median(ms[f]) for f in QFORMS)
        og = statistics.median(oms["gather"])
        frames = batch * ring
        gather_bytes = frames * (rb + 12)
        out = {
            "row": key, "frames_per_pass": frames, "batches": ring, "rec_bytes": rb, "flows": flows,
            "steps": steps, "repeats": repeats,
            "classify_ms": round(c, 5), "classify_steer_ms": round(s, 5), "classify_steer_gather_ms": round(g, 5),
            "classify_steer_gather_fhash_ms": round(gf, 5),
            "gather_ms": round(g - s, 5), "gather_GBps": rate(gather_bytes, g - s),
            "side_fhash_ms": round(gf - g, 5), "side_fhash_GBps": rate(frames * 8, gf - g),
            "side_fhash_rate_over_gather_rate": (round(rate(frames * 8, gf - g) / rate(gather_bytes, g - s), 3)
                                                 if gf > g and g > s else None),
            "op_steer_gather_ms": round(og, 5),
        }
        for f in ("fhash", "match", "all"):
            d = statistics.median(oms[f]) - og
            out[f"op_side_{f}_ms"] = round(d, 5)
            out[f"op_side_{f}_GBps"] = rate(frames * SIDE_BYTES[f], d)
        for f in QFORMS:
            out[f"{f}_ms_all"] = [round(x, 5) for x in ms[f]]
        for f in OFORMS:
            out[f"op_{f}_ms_all"] = [round(x, 5) for x in oms[f]]
        return out
    finally:
        for q in qs:
            q.destroy()
        for b in idx + qst + qrec + qoff + qlen + qfh + dbs:
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
