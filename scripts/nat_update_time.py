#!/usr/bin/env python3
"""Cost of handing the GPU a changed NAT table: mosrx_nat_update
of 1, 64 and 4096 ops against the mosrx_nat_set that reaches the same table, at
64510 and at 1024 bindings.

Per table size and op count one pair of op lists: `there` deletes half of the
ops' worth of installed bindings and adds as many new ones, `back` undoes it, so
the table returns and every window measures the same work.  Host wall time per
call (perf_counter around the call; for the update that is the arithmetic on the
mirror and the enqueue, for the set the build, the blocking upload and whatever
drain the pool asks for) and, for the update, device time between two events
around its launch on the context's stream.  The two forms alternate in one run;
median of 5 windows of `reps` calls each.  At 1024 bindings 4096 ops cannot be
half deletes: the list is 1024 deletes and 3072 adds, which no longer fits the
table in place, so that row times the rebuild path (the stats say so).

The set that is timed is this tree's mosrx_nat_set, not the parent commit's: it
builds and uploads exactly as the parent's does and then keeps the host table it
built as the mirror where the parent frees it, one free() less per call.  For a
call that rebuilds, the "device" figure is not device work: the rebuild runs on
the host between the two event records (its upload is a blocking copy), so the
events merely span it.

Then the rebuild that churn forces at the full pool: calls of 8 deletes and 8 adds
of flows never seen before until the stats count a rebuild; that call's wall time,
the calls and deletes it took to get there, and the cost spread over them.

    python scripts/nat_update_time.py [--windows 5] > profiles/nat/update_time.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mos-networking-stack_amd"))

import numpy as np  # noqa: E402

import mosrx  # noqa: E402

NAT_IP = mosrx.ip_raw("192.0.2.1")


def flows(lo, n):
    """Bindings lo .. lo + n of one endless family of distinct flows."""
    i = np.arange(lo, lo + n)
    b = np.zeros(n, mosrx.NAT_BINDING_DTYPE)
    b["cli_ip"] = 10 | (i // 62500 % 250) << 8 | (i // 250 % 250) << 16 | (i % 250 + 1) << 24
    b["svr_ip"] = 198 | 51 << 8 | 100 << 16 | (7 + i // 15625000) << 24
    b["nat_ip"] = NAT_IP
    p = 1024 + i % 60000
    b["cli_port"] = (p & 0xFF) << 8 | p >> 8
    b["svr_port"] = (80 + i // 60000) << 8
    q = 1025 + i % 64510
    b["nat_port"] = (q & 0xFF) << 8 | q >> 8
    return b


def ops_of(adds, ids, dels):
    o = np.zeros(len(dels) + len(adds), mosrx.NAT_OP_DTYPE)
    o["b"][:len(dels)], o["op"][:len(dels)] = dels, mosrx.NAT_OP_DEL
    o["b"][len(dels):], o["op"][len(dels):], o["bind"][len(dels):] = adds, mosrx.NAT_OP_ADD, ids
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    hip = C.CDLL("libamdhip64.so")
    e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_float()
    print(f"# mosrx_nat_update against mosrx_nat_set, median of {a.windows} windows of {a.reps} calls, microseconds per call")
    with mosrx.Context(0, mosrx.default_params(num_msp=1, forward=1)) as ctx:
        assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
        stream = C.c_void_p(mosrx.lib().mosrx_stream(ctx.handle))
        sync = lambda: mosrx._chk(mosrx.lib().mosrx_sync(ctx.handle), "sync")   # noqa: E731
        for nbind in (mosrx.NAT_MAX_BINDINGS, 1024):
            for nops in (1, 64, 4096):
                base = flows(0, nbind - (nops == 1))                   # (the lone op is an ADD: one port of the pool left for it)
                nd = min(nops // 2, nbind)
                na = max(nops - nd, 1) if nops > 1 else 1
                nd = 0 if nops == 1 else nd
                new = flows(1 << 20, na)
                there = ops_of(new, np.arange(na) + (1 << 20), base[:nd])
                back = ops_of(base[:nd], np.arange(nd), new)
                after = np.concatenate([base[nd:], new])
                ctx.nat_set(base)
                s0 = ctx.nat_stats()
                wall = {"update": [], "set": []}
                dev = []
                for _ in range(a.windows):
                    w = d = 0.0
                    for _ in range(a.reps):
                        for o in (there, back):
                            hip.hipEventRecord(e0, stream)
                            t = time.perf_counter()
                            ctx.nat_update(o)
                            w += time.perf_counter() - t
                            hip.hipEventRecord(e1, stream)
                            sync()
                            hip.hipEventElapsedTime(C.byref(ms), e0, e1)
                            d += ms.value
                    wall["update"].append(w / (2 * a.reps) * 1e6)
                    dev.append(d / (2 * a.reps) * 1e3)
                    s1 = ctx.nat_stats()
                    w = 0.0
                    for _ in range(max(a.reps // 4, 1)):
                        for b in (after, base):
                            t = time.perf_counter()
                            ctx.nat_set(b)
                            w += time.perf_counter() - t
                    wall["set"].append(w / (2 * max(a.reps // 4, 1)) * 1e6)
                mu, msd, md = (statistics.median(v) for v in (wall["update"], wall["set"], dev))
                print(f"\n{nbind} bindings ({s0.slots} slots), {nops} ops ({nd} deletes, {na} adds): "
                      f"rebuilds over all windows {s1.rebuilds - s0.rebuilds} of {2 * a.reps * a.windows} calls, tombstones at the end {s1.tombs}")
                print(f"  nat_update wall   median {mu:10.1f}  windows {' '.join(f'{v:.1f}' for v in wall['update'])}")
                print(f"  nat_update device median {md:10.1f}  windows {' '.join(f'{v:.1f}' for v in dev)}")
                print(f"  nat_set    wall   median {msd:10.1f}  windows {' '.join(f'{v:.1f}' for v in wall['set'])}")
                print(f"  nat_set / nat_update (wall) {msd / mu:8.1f}")
        # the rebuild churn forces at the full pool
        ctx.nat_set(flows(0, mosrx.NAT_MAX_BINDINGS))
        s0, lo, calls, spent, prev = ctx.nat_stats(), 1 << 21, 0, 0.0, flows(0, 8)
        while True:
            cur = flows(lo, 8)
            o = ops_of(cur, np.arange(8) + lo, prev)
            t = time.perf_counter()
            ctx.nat_update(o)
            dt = time.perf_counter() - t
            calls, lo, prev = calls + 1, lo + 8, cur
            if ctx.nat_stats().rebuilds > s0.rebuilds:
                break
            spent += dt
        sync()
        print(f"\nfull pool, calls of 8 deletes + 8 adds of new flows: rebuild at call {calls} ({8 * calls} deletes); "
              f"in-place calls {spent / max(calls - 1, 1) * 1e6:.1f} us each, the rebuilding call {dt * 1e3:.2f} ms, "
              f"spread over the {calls} calls {dt / calls * 1e6:.1f} us a call, {dt / (8 * calls) * 1e6:.2f} us a delete")


if __name__ == "__main__":
    main()
