"""Generate tests/golden/fwd_plan.npz: the forwarding scenarios of tests/fwd_pin.py
with the frames mOS's OWN ProcessPacket sent for them.

Run where the reference build exists (oracle/_ref):
    make -C oracle ref && python tests/golden/make_golden_fwd.py

Per scenario: the frames (packed), the tables (a mosrx_fwd_tables, raw bytes),
whether the conf had a nic_forward_table, the restatement's plan records, and
mOS's tx.pcap frames laid out as the library stages them (tx bytes, tx_off,
tx_len, tx_nif, tx_src).  The run refuses to write a fixture whose TX frames
from mOS differ from the restatement's (tests/fwd_oracle.py).  Only data.
"""
from __future__ import annotations

import os
import pathlib
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "mos-networking-stack_amd"))

import fwd_oracle as F  # noqa: E402
import fwd_pin as P  # noqa: E402


def main():
    if not os.access(P.APP, os.X_OK):
        sys.exit(f"{P.APP} missing: run `make -C oracle ref` first")
    out = {}
    for name, (kind, nicfwd) in P.SCENARIOS.items():
        frames = P.scenario_frames(kind)
        buf, off, ln, rec, pl, tx = P.restated(frames, nicfwd)
        mos = P.run_mos(pathlib.Path(tempfile.mkdtemp()), name, frames, nicfwd)
        if mos != tx:
            sys.exit(f"{name}: mOS sent {len(mos)} frames, the restatement {len(tx)}, or their bytes differ")
        t = P.tables(nicfwd)
        n = len(off)
        cap = int(ln.astype(np.int64).sum()) + 32 * n + 16
        txb, toff, tlen, tnif, tsrc, cnt = F.build(buf, off, pl, t, cap, np.zeros(cap, np.uint8),
                                                   np.zeros(n, np.uint32), np.zeros(n, np.uint16),
                                                   np.zeros(n, np.int8), np.zeros(n, np.uint32))
        m = int(cnt[0])
        # the TX bytes as mOS sent them, at the restatement's offsets
        assert [bytes(txb[int(o):int(o) + int(k)]) for o, k in zip(toff[:m], tlen[:m])] == mos
        end = int(toff[m - 1]) + int(tlen[m - 1]) if m else 0
        k = name + "__"
        out[k + "frames"], out[k + "off"], out[k + "len"] = buf, off, ln
        out[k + "reason"] = np.ascontiguousarray(rec["reason"])
        out[k + "tables"] = np.frombuffer(bytes(t), np.uint8).copy()
        out[k + "plan"] = pl
        out[k + "tx"], out[k + "tx_off"], out[k + "tx_len"] = txb[:end], toff[:m], tlen[:m]
        out[k + "tx_nif"], out[k + "tx_src"] = tnif[:m], tsrc[:m]
        print(f"{name}: {n} frames, {m} sent, kinds {np.bincount(pl['kind'], minlength=6).tolist()}, "
              f"arp entries used {sorted(set(pl['arp_idx'][pl['arp_idx'] != 0xFFFF].tolist()))}")
    np.savez_compressed(os.path.join(HERE, "fwd_plan.npz"), **out)


if __name__ == "__main__":
    main()
