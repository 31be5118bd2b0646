"""The restatement of the descriptor form (tests/fwd_desc_oracle.py) pinned to
what is already pinned: each entry's source frame with tx_mac laid over it
reproduces the byte rings' ring_list, and for tests/golden/fwd_plan.npz ring 0
is mOS's own recorded TX frames.  Then the scratch size (no GPU)."""
import os

import numpy as np
import pytest

import fwd_desc_oracle as FD
import fwd_oracle as F
import fwd_rings_oracle as FR
import mosrx
from test_fwd_gpu import ee
from test_fwd_rings_oracle import net16_input, planned, rings_run, walk4_input
from test_oracle_golden import GOLDEN


def desc_run(buf, off, pl, t, nrings):
    n = len(off)
    return FD.build(buf, off, pl, t, nrings, ee(n + 8, np.uint32), ee(n + 8, np.uint16), ee(12 * (n + 8), np.uint8),
                    ee(nrings + 2, mosrx.FWD_RING_DTYPE))


def assert_desc_equal_rings(buf, off, pl, t, nrings):
    need = FR.need_units(pl, nrings)
    cap = int(need.max()) * 16
    tx, toff, tlen, rsrc, rings = rings_run(buf, off, pl, t, nrings, cap)
    dsrc, dlen, dmac, drings = desc_run(buf, off, pl, t, nrings)
    assert drings.tobytes() == rings.tobytes() and (rings["dropped"][:nrings] == 0).all()
    assert drings["units"][:nrings].tolist() == need.tolist()
    total = int(rings["count"][:nrings].sum())
    assert dsrc.tobytes() == rsrc.tobytes() and dlen.tobytes() == tlen.tobytes()
    for q in range(nrings):
        assert FD.ring_list(buf, off, dsrc, dlen, dmac, drings, q) == FR.ring_list(tx, toff, tlen, rings, q)
    assert (dmac[12 * total:] == 0xEE).all() and (dsrc[total:] == 0xEEEEEEEE).all() and (dlen[total:] == 0xEEEE).all()
    return drings


def test_desc_equals_rings_4_netdevs():
    (buf, off, ln), t = walk4_input()
    rings = assert_desc_equal_rings(buf, off, planned(buf, off, ln, t), t, 4)
    assert (rings["count"][:4] > 0).all()


def test_desc_equals_rings_16_netdevs():
    (buf, off, ln), t = net16_input()
    rings = assert_desc_equal_rings(buf, off, planned(buf, off, ln, t), t, 16)
    assert (rings["count"][:16] > 0).all()


@pytest.mark.parametrize("name", ["conv_walk", "edge_walk", "conv_nicfwd"])
def test_desc_equals_mos_fixture(name):
    """fwd_plan.npz: one netdev, so ring 0 is mOS's own tx.pcap list."""
    z = np.load(os.path.join(GOLDEN, "fwd_plan.npz"))
    k = name + "__"
    t = mosrx.FwdTables.from_buffer_copy(z[k + "tables"].tobytes())
    buf, off, pl = z[k + "frames"], z[k + "off"], z[k + "plan"].view(mosrx.FWD_DTYPE).reshape(-1)
    nrings = max(t.num_netdevs, 1)
    assert_desc_equal_rings(buf, off, pl, t, nrings)
    m = len(z[k + "tx_off"])
    dsrc, dlen, dmac, drings = desc_run(buf, off, pl, t, nrings)
    assert drings[0].tolist()[:3] == (0, m, 0) and m > 0
    assert FD.ring_list(buf, off, dsrc, dlen, dmac, drings, 0) == F.tx_list(z[k + "tx"], z[k + "tx_off"], z[k + "tx_len"], m)
    np.testing.assert_array_equal(dsrc[:m], z[k + "tx_src"])


def test_scratch_bytes_needs_no_context():
    L = mosrx.lib()
    f = L.mosrx_fwd_desc_scratch_bytes
    for n in (0, 1, 255, 256, 257, 5003, 65536, 0xFFFFFFFF):
        for q in (0, 1, 4, 16, 17):
            assert f(n, q) == L.mosrx_fwd_rings_scratch_bytes(n, q) and f(n, q) > 0 and f(n, q) % 16 == 0
    assert f(0, 1) == 16 and f(257, 4) == 128
