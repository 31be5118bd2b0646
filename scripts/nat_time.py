#!/usr/bin/env python3
"""Cost of NAT translation (mosrx_queue_set_nat) inside the byte-
ring queue form: device time between events on one stream, median of 5 windows,
the forms alternating in one run (scripts/fwd_time.py's method,
scripts/fwd_rings_time.py's rows and tables).

Per row, case and window, one pass over all batches of
    queue                 mosrx_queue_run, nothing attached (the classify launch)
    queue+plan            ... with the plan attached
    queue+plan+rings      ... with plan and byte rings (what the parent runs)
    queue+natplan         ... with plan-nat in the plan's place
    queue+natplan+rings   ... with plan-nat, byte rings and the patch
"plan" is the second less the first, "plan-nat" the fourth less the first, "build"
the third less the second, "patch" the fifth less the fourth less the build.
The cases: the row's trace as generated with its first flow bound (1 binding: the
64 B trace is one flow, so every TCP_OK frame is translated; the 1500 B trace has
a flow per frame, so one frame a batch is) and with an unrelated binding (none);
the same frames spread over 64510 flows by their source ports, with 64510 of the
flows bound (all translated, but for the 1500 B row's flows past the pool) and
with 64510 unrelated bindings (none).  With none translated every TCP_OK frame
is a MISS and leaves the plan, so the build behind plan-nat has next to nothing
to copy: "patch" is then no measurement (negative), and the row shows what a
table of first frames costs.  The byte bound to hold
plan-nat against: the plan's bytes plus 16 B written and one 32 B slot read per
eligible frame.

    python scripts/nat_time.py [--windows 5] > profiles/nat/nat_time.txt
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

NAT_IP = mosrx.ip_raw("192.0.2.1")


def flows_of(traces, limit):
    """Bindings for the distinct (saddr, daddr, sport, dport) of the traces' plain IPv4 / TCP frames, at most `limit`."""
    keys = []
    for t in traces:
        o = np.asarray(t.off).astype(np.int64)[np.asarray(t.len) >= 54]
        buf = t.frames
        o = o[(buf[o + 12] == 8) & (buf[o + 13] == 0) & (buf[o + 14] == 0x45) & (buf[o + 23] == 6)]
        k = np.stack([buf[o + j] for j in range(26, 38)], 1)
        keys.append(np.unique(np.ascontiguousarray(k).view("V12")))
    rest = np.setdiff1d(np.unique(np.concatenate(keys)), keys[0])
    k = np.concatenate([keys[0], rest])[:limit]                    # batch 0's flows first: it is the batch reported
    raw = np.frombuffer(k.tobytes(), np.uint8).reshape(-1, 12)
    b = np.zeros(len(raw), mosrx.NAT_BINDING_DTYPE)
    b["cli_ip"] = raw[:, 0:4].copy().view("<u4")[:, 0]
    b["svr_ip"] = raw[:, 4:8].copy().view("<u4")[:, 0]
    b["cli_port"] = raw[:, 8:10].copy().view("<u2")[:, 0]
    b["svr_port"] = raw[:, 10:12].copy().view("<u2")[:, 0]
    b["nat_ip"] = NAT_IP
    i = np.arange(len(b)) + 1025
    b["nat_port"] = (i & 0xFF) << 8 | i >> 8
    return b


def spread(t, nflows):
    """The trace's frames (the generator gives one flow) with the source port of plain IPv4 / TCP frame i made
    1025 + i % nflows, the TCP checksum adjusted for the changed word (RFC 1624): nflows flows."""
    buf = np.array(t.frames, np.uint8, copy=True)
    o = np.asarray(t.off).astype(np.int64)[np.asarray(t.len) >= 54]
    o = o[(buf[o + 12] == 8) & (buf[o + 13] == 0) & (buf[o + 14] == 0x45) & (buf[o + 23] == 6)]
    new = 1025 + np.arange(len(o)) % nflows
    old = (buf[o + 34].astype(np.int64) << 8) | buf[o + 35]
    c = (buf[o + 50].astype(np.int64) << 8) | buf[o + 51]
    x = (~c & 0xFFFF) + (~old & 0xFFFF) + new
    x = (x & 0xFFFF) + (x >> 16)
    x = (x & 0xFFFF) + (x >> 16)
    c = ~x & 0xFFFF
    buf[o + 34], buf[o + 35] = new >> 8, new & 0xFF
    buf[o + 50], buf[o + 51] = c >> 8, c & 0xFF
    t.frames = buf
    return t


def unrelated(n):
    """n bindings no frame of the generated traces matches (203.0.113.0/24 clients)."""
    i = np.arange(n)
    b = np.zeros(n, mosrx.NAT_BINDING_DTYPE)
    b["cli_ip"] = 203 | 0 << 8 | 113 << 16 | (i % 250 + 1) << 24
    b["svr_ip"], b["nat_ip"] = mosrx.ip_raw("198.51.100.7"), NAT_IP
    p = 1 + i // 250
    b["cli_port"] = (p & 0xFF) << 8 | p >> 8
    b["svr_port"] = 7 << 8
    b["nat_port"] = ((i + 1025) & 0xFF) << 8 | (i + 1025) >> 8
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide the batch counts (a quick run)")
    a = ap.parse_args()
    print(f"# NAT translation inside the byte-ring queue form, median of {a.windows} windows, ms per pass over the row's batches")
    with mosrx.Context(0, mosrx.default_params(num_msp=1, forward=1)) as ctx:
        tab = tables(False)
        nrings = tab.num_netdevs
        ctx.fwd_set(tab)
        for row, (kind, n, nb, rb) in ROWS.items():
            nb = max(nb // a.scale, 1)
            for nflows in (1, mosrx.NAT_MAX_BINDINGS):
                # one trace for every batch (each uploaded on its own): the bindings of batch 0 are then everyone's
                tr = [spread(mosrx.Trace(kind, n, seed=1), nflows)]
                bound = flows_of(tr, 1 if nflows == 1 else mosrx.NAT_MAX_BINDINGS)
                if nflows > 1:                                                          # the full pool, whatever the batch holds
                    bound = np.concatenate([bound, unrelated(mosrx.NAT_MAX_BINDINGS - len(bound))])
                dbs = [ctx.upload(t.frames, t.off, t.len, frames_bytes=t.frames_bytes, max_len=t.max_len)
                       for t in (tr[i % len(tr)] for i in range(nb))]
                cap = (max(t.frames_bytes for t in tr) + 32 * n + 255) // 256 * 256
                bufs = [[mosrx.DevBuffer(ctx, sz(d.n)) for d in dbs] for sz in
                        (lambda m: 8 * m, lambda m: nrings * cap, lambda m: 4 * m, lambda m: 2 * m, lambda m: 4 * m,
                         lambda m: 16 * nrings, lambda m: 16 * m)]
                p = [[b.ptr for b in bs] for bs in bufs]
                names = ("queue", "queue+plan", "queue+plan+rings", "queue+natplan", "queue+natplan+rings")
                for what, bind in ((f"{len(bound)} bindings, the trace's own flows", bound),
                                   (f"{len(bound)} bindings, none of the trace's", unrelated(len(bound)))):
                    ctx.nat_set(bind)
                    qs = {k: ctx.queue_ex(dbs, compact=rb == 8) for k in names}
                    qs["queue+plan"].set_fwd(p[0])
                    qs["queue+plan+rings"].set_fwd(p[0], None, cap, nrings, p[1], p[2], p[3], p[4], p[5])
                    qs["queue+natplan"].set_fwd(p[0])
                    qs["queue+natplan"].set_nat(p[6])
                    qs["queue+natplan+rings"].set_fwd(p[0], None, cap, nrings, p[1], p[2], p[3], p[4], p[5])
                    qs["queue+natplan+rings"].set_nat(p[6])
                    for q in qs.values():
                        q.run()                                                         # warm up
                    x = bufs[6][0].download(np.zeros(dbs[0].n, mosrx.NAT_XLAT_DTYPE))
                    kinds = np.bincount(x["kind"], minlength=5).tolist()
                    ms = {k: [] for k in qs}
                    for _ in range(a.windows):
                        for k, q in qs.items():
                            ms[k].append(q.time(1, kernels=False)[0])
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    plan, natplan = med["queue+plan"] - med["queue"], med["queue+natplan"] - med["queue"]
                    build = med["queue+plan+rings"] - med["queue+plan"]
                    patch = med["queue+natplan+rings"] - med["queue+natplan"] - build
                    _, probe = mosrx.nat_table(bind)
                    print(f"\n{row}, {nflows} flows, {what} (longest probe run {probe}): {nb * n} frames in {nb} batches; "
                          f"batch 0 xlat kinds none/snat/dnat/miss/host {kinds}")
                    for k, v in ms.items():
                        print(f"  {k:<20} median {med[k]:8.3f}  windows {' '.join(f'{v_:.3f}' for v_ in v)}")
                    print(f"  plan {plan:8.3f} ms   plan-nat {natplan:8.3f} ms   plan-nat / plan {natplan / plan:.2f}   "
                          f"build {build:8.3f} ms   patch {patch:8.3f} ms   patch / build {patch / build:.2f}")
                    print(f"  classify + plan + rings {nb * n / med['queue+plan+rings'] / 1e3:8.1f} Mpps   "
                          f"classify + plan-nat + rings + patch {nb * n / med['queue+natplan+rings'] / 1e3:8.1f} Mpps")
                    for q in qs.values():
                        q.destroy()
                for b in [b for bs in bufs for b in bs]:
                    b.free()
                for d in dbs:
                    d.free()


if __name__ == "__main__":
    main()
