"""The firewall rules on the drop-in backend (mosrx_gpu_module_set_acl, the group
submits armed with mosrx_slot_acl, MOSRX_PKT_RX_ACL): GpuBackend over a memory
source of test_acl_gpu's mix of frames, batches small enough for several batches
and groups.  Every batch's forwarding view equals the restatements applied to
that batch alone with the firewall's amendment between them (fwd_oracle.plan,
acl_oracle.apply, fwd_desc_oracle.build), its ACL view the restatement's hits,
and the counts the restatement's sums.  Expected values never come from the GPU."""
import numpy as np
import pytest

import acl_oracle as A
import fwd_desc_oracle as FD
import fwd_oracle as F
import mosrx
import oracle_py as O
from test_acl_gpu import PHASES, TABLES, frame, rules_of
from test_fwd_gpu import PAD, ee, pack_at

pytestmark = pytest.mark.gpu

PARAMS = dict(num_msp=1, forward=1)
BATCH = 96
N = 700


def expected(tr, lo, n, tab, rules):
    """The restatement's (amended plan, tx_src, tx_len, tx_mac, rings, hit, counts) for frames lo .. lo + n."""
    buf, off, ln = tr
    o, l = off[lo:lo + n], ln[lo:lo + n]
    rec = O.classify(buf, o, l, O.params(**PARAMS))
    base = F.plan(buf, o, l, rec["reason"], tab, 0, forward=1, num_msp=1)
    hit, cnt, want = A.apply(buf, o, l, rec, rules, base)
    init = [ee(n + PAD, np.uint32), ee(n + PAD, np.uint16), ee(12 * (n + PAD), np.uint8), ee(2 + 2, mosrx.FWD_RING_DTYPE)]
    src, tl, mac, rings = FD.build(buf, o, want, tab, 2, *init)
    m = int(rings["count"][:2].sum())
    return want, src[:m], tl[:m], mac[:12 * m], rings[:2], hit, cnt[:len(rules)], base


def drain(direct_kb, compact, fwd_one=0, acl="five"):
    """Every batch of the trace through the backend, each view checked; returns (batches, fwd_one_count, drops)."""
    tr = pack_at([frame(i) for i in range(N)], PHASES)
    tab, rules = mosrx.fwd_tables(**TABLES), rules_of(acl)
    be = mosrx.GpuBackend([mosrx.mem_source(*tr, loops=1)], params=mosrx.default_params(**PARAMS), batch=BATCH, group=2,
                          cpu=9, compact=compact, fwd=tab, acl=rules, direct_kb=direct_kb, fwd_one=fwd_one)
    pos = batches = drops = 0
    cum = np.zeros(len(rules), np.uint32)
    total = A.apply(tr[0], tr[1], tr[2], O.classify(*tr, O.params(**PARAMS)), rules)[1][:len(rules)]
    try:
        assert be.acl_view(0) is None and be.fwd_view(0) is None            # no batch exposed yet
        while True:
            n = be.recv_pkts(0)
            assert n >= 0
            if not n:
                break
            want, src, tl, mac, rings, hit, cnt, base = expected(tr, pos, n, tab, rules)
            got = be.fwd_view(0)
            assert got is not None
            assert np.array_equal(got[0].view(np.uint64), want.view(np.uint64)), pos
            assert got[4].tobytes() == rings.tobytes(), (pos, got[4], rings)
            assert np.array_equal(got[1], src) and np.array_equal(got[2], tl) and np.array_equal(got[3], mac)
            av = be.acl_view(0)
            assert av is not None
            np.testing.assert_array_equal(av[0], hit)
            cum += cnt
            # the counts are those of every group waited for: this batch's group may hold later batches too
            assert (av[1] >= cum).all() and (av[1] <= total).all(), (pos, av[1], cum)
            drops += int((want["kind"] == mosrx.FWD_DROP).sum())
            assert not np.isin(np.nonzero(want["kind"] == mosrx.FWD_DROP)[0], src).any()
            last = av[1]
            pos += n
            batches += 1
        assert pos == N and batches >= 7 and be.stats().rx_groups >= 4
        np.testing.assert_array_equal(last, total)
        np.testing.assert_array_equal(cum, total)
        return batches, be.fwd_one_count(), drops
    finally:
        be.close()


@pytest.mark.parametrize("direct_kb", [None, 0])
@pytest.mark.parametrize("compact", [False, True])
def test_views_equal_the_restatement(compact, direct_kb):
    """direct_kb None: the default, small groups written in place; 0: every group copied back."""
    batches, ones, drops = drain(direct_kb, compact)
    assert drops > 20 and ones == 0


@pytest.mark.parametrize("direct_kb", [None, 0])
def test_fwd_one_limit_changes_nothing(direct_kb):
    """Every batch fits the one-launch limit, and the groups still take the multi-launch path: the
    same views (checked inside), and the one-launch count does not advance."""
    batches, ones, drops = drain(direct_kb, False, fwd_one=256)
    assert ones == 0 and drops > 20


def test_without_rules_the_ioctl_answers_minus_one_and_one_launch_is_taken():
    tr = pack_at([frame(i) for i in range(200)], PHASES)
    be = mosrx.GpuBackend([mosrx.mem_source(*tr, loops=1)], params=mosrx.default_params(**PARAMS), batch=BATCH, group=2,
                          cpu=9, fwd=mosrx.fwd_tables(**TABLES), fwd_one=256)
    try:
        assert be.recv_pkts(0) > 0
        assert be.acl_view(0) is None and be.fwd_view(0) is not None
        assert be.fwd_one_count() > 0
    finally:
        be.close()
    L = mosrx.lib()
    bad = np.zeros(2, mosrx.ACL_RULE_DTYPE)
    assert L.mosrx_gpu_module_set_acl(bad.ctypes.data, 2) == -22 and L.mosrx_gpu_module_set_acl(None, 3) == -22
    assert L.mosrx_gpu_module_set_acl(bad.ctypes.data, 1025) == -22 and L.mosrx_gpu_module_set_acl(None, 0) == 0
