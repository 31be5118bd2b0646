#!/usr/bin/env python3
"""The drop-in backend's rx loop with forwarding off and on:
recv_pkts over a looping memory source, and with forwarding on one
mosrx_backend_forward per batch (MOSRX_PKT_RX_FWD + mosrx_fwd_desc_send into the
module's own get_wptr / send_pkts; the source has no TX sink, so the frames are
discarded after the copy).  Wall-clock Mpkt/s of the loop, median of 5 windows,
off and on alternating in one run, and the classify launch's device time per
group beside it (the module's timing; the plan and descriptor launches are
timed on the device by scripts/fwd_desc_time.py).

    python scripts/fwd_desc_backend_time.py > profiles/fwd/desc_backend_time.txt
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mos-networking-stack_amd"))

import mosrx  # noqa: E402

ROWS = {"S64": (mosrx.TRACE_S64, 32768, 64), "M1500": (mosrx.TRACE_M1500, 32768, 16)}
DEV = ["02:00:00:00:aa:00"]


def window(kind, n, batches, fwd):
    t = mosrx.Trace(kind, n, seed=3)
    src = mosrx.mem_source(t.frames, t.off, t.len, loops=batches)
    tab = mosrx.fwd_tables(netdevs=DEV, nic_fwd={0: 0}) if fwd else None
    be = mosrx.GpuBackend([src], params=mosrx.default_params(num_msp=1, forward=1), batch=n, group=4, cpu=3,
                          compact=True, timing=True, fwd=tab)
    frames = sent = 0
    try:
        t0 = time.perf_counter()
        while True:
            k = be.recv_pkts(0)
            if k <= 0:
                break
            frames += k
            if fwd:
                rc, st = be.forward(0)
                assert rc >= 0
                sent += rc
        dt = time.perf_counter() - t0
        ms = be.stats()
        per = ms.kernel_ms / max(ms.kernel_launches, 1)
    finally:
        be.close()
    return frames / dt / 1e6, per, frames, sent


def main():
    print("# gpu_module_func rx loop, forwarding off / on, median of 5 windows (off and on alternating)")
    for row, (kind, n, batches) in ROWS.items():
        res = {False: [], True: []}
        for _ in range(5):
            for fwd in (False, True):
                res[fwd].append(window(kind, n, batches, fwd))
        for fwd in (False, True):
            mp = [r[0] for r in res[fwd]]
            kms = [r[1] for r in res[fwd]]
            print(f"{row} {n} frames x {batches} batches, forwarding {'on ' if fwd else 'off'}: "
                  f"{statistics.median(mp):8.2f} Mpkt/s (windows {' '.join(f'{x:.2f}' for x in mp)}), classify launch "
                  f"{statistics.median(kms) * 1e3:7.1f} us per group, frames {res[fwd][0][2]}, sent {res[fwd][0][3]}")


if __name__ == "__main__":
    main()
