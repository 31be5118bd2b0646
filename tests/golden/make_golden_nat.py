"""Generate tests/golden/nat.npz: one trace's NAT answers as the restatement
(tests/nat_oracle.py) gives them -- the sample's two overwrites, both checks
recomputed in full by the oracle's mo_tx_csum, the plan of the translated frames.

    python tests/golden/make_golden_nat.py

The trace is tests/nat_cases.py's mixed batch of 513 frames at odd offsets, with
its 64 bindings (16 of them in one slot) and its tables.  Stored: the packed
frames, the records' reason (the short-segment frames forced to TCP_OK), the
bindings, and per frame the xlat record and the plan record; the translated
buffer too, which the ring comparison copies from.  No build of the nat sample
exists here: the equivalence with it rests on the reading of nat.c / mos_api.c
stated in nat_oracle.py, on fwd_plan.npz and on tx_*.npz.  Only data.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "mos-networking-stack_amd"))

import mosrx  # noqa: E402
import nat_cases as NC  # noqa: E402
import nat_oracle as N  # noqa: E402
import oracle_py as O  # noqa: E402
from test_fwd_gpu import pack_at  # noqa: E402

N_FRAMES = 513
PHASES = [2, 7, 0, 13, 1, 11]


def main():
    buf, off, ln = pack_at(NC.mix(N_FRAMES), PHASES)
    rec = NC.forced(O.classify(buf, off, ln, O.params(num_msp=1, forward=1)), N_FRAMES)
    b = NC.bindings()
    x, pl, tr = N.plan(buf, off, ln, rec["reason"], b, mosrx.fwd_tables(**NC.TABLES), 0)
    np.savez_compressed(os.path.join(HERE, "nat.npz"), n=np.array([N_FRAMES], np.uint32), frames=buf, off=off, len=ln,
                        reason=np.ascontiguousarray(rec["reason"]), bindings=b, xlat=x, plan=pl, translated=tr)
    print(f"{N_FRAMES} frames: xlat kinds {np.bincount(x['kind']).tolist()}, plan kinds {np.bincount(pl['kind']).tolist()}")


if __name__ == "__main__":
    main()
