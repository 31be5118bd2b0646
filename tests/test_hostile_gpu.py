"""The plan, firewall and NAT launches over hostile inputs (tests/hostile.py;
tests/test_hostile.py asserts what those inputs cover): frames whose header
fields run over their whole ranges, the buffer end and len[] cut at and around
every byte count a condition of the launches names, binding tables whose longest
probe run wraps past slot 0, rule tables matched at their edges, and a queue of
empty batches and batches of exactly one and two tiles.

Every comparison is exact, over 0xEE images with canary entries, through the
runs and checks of test_acl_gpu.py / test_nat_gpu.py / test_nat_queue_gpu.py.
Expected values never come from the GPU: the records uploaded are
oracle_py.classify's of the same bytes, unforced (in the cut tests: of the whole
buffer, so that the launch's own capture conditions decide), and the answers are
fwd_oracle / acl_oracle / nat_oracle / fwd_rings_oracle's."""
import numpy as np
import pytest

import acl_oracle as A
import fwd_oracle as F
import fwd_rings_oracle as FR
import hostile as H
import mosrx
import nat_oracle as N
import oracle_py as O
import test_acl_gpu as TA
import test_nat_gpu as TN
from test_acl_gpu import QueueAcl
from test_fwd_desc_gpu import DescOutputs
from test_fwd_queue_gpu import Setup
from test_nat_queue_gpu import Xlat, check_rings

pytestmark = pytest.mark.gpu

NS = [0, 256, 0, 0, 1, 512, 0]
STARTS = [0, 0, 0, 0, 256, 513, 0]           # tile 0; frame 256; the lone SYN's tile from 513, tile 3 and frame 1024
NR = 4
FW = dict(tables=H.TABLES, nrings=NR)     # the firewall checks over the NAT tests' forwarding tables: frames are sent


@pytest.fixture(autouse=True)
def default_params_afterwards(gpu_ctx):
    yield
    gpu_ctx.fwd_set_listener(False)
    gpu_ctx.set_params(mosrx.default_params())


# ---- the mixed batch ------------------------------------------------------------------

@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_plan(gpu_ctx, rec_bytes):
    """mosrx_fwd_plan_dev alone: plan-nat includes the same body, so a difference here is the plan's."""
    h = H.batch()
    t = TN.setup(gpu_ctx, H.bindings())
    want = F.plan(h.buf, h.off, h.ln, h.rec["reason"], t, 0)
    assert {F.NONE, F.IP, F.NO_ROUTE, F.NO_NIC} <= set(want["kind"].tolist())
    r = TN.NatRun(gpu_ctx, h.buf, h.off, h.ln, h.rec, rec_bytes)
    try:
        r.plan(0)
        TN.same_records(r.plan_result(), want, "plan")
        assert r.xlat().tobytes() == r.x_init.tobytes()
    finally:
        r.free()


@pytest.mark.parametrize("forward", [1, 0])
@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("name", ["last_of_full", "n257", "overlap"])
def test_firewall(gpu_ctx, name, rec_bytes, forward):
    h, rules = H.batch(), H.rule_sets()[name]
    rec = h.rec if forward else O.classify(h.buf, h.off, h.ln, O.params(num_msp=1, forward=0))
    hit, pl = TA.check(gpu_ctx, h.buf, h.off, h.ln, rules, rec_bytes, forward=forward, rec=rec,
                       downstream=bool(forward) and rec_bytes == 16, **FW)
    looked = hit != A.NOT_LOOKED_UP
    assert looked[2 * H.T:3 * H.T].sum() == 1 and not looked[H.T:2 * H.T].any() and looked[1024]
    want = {"last_of_full": {1023}, "n257": {100, 255, 256}, "overlap": {0, 1, 2, 3}}[name] | {A.NO_MATCH}
    assert set(hit[looked].tolist()) == want
    assert (pl["kind"] == mosrx.FWD_DROP).sum() == (A.dropped(hit, rules).sum() if forward else 0)
    assert A.dropped(hit, rules).sum() >= 15


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_nat(gpu_ctx, rec_bytes):
    h = H.batch()
    x, pl = TN.check(gpu_ctx, h.buf, h.off, h.ln, h.rec, H.bindings(), rec_bytes)
    assert {int(k) for k in x["kind"]} == {N.NONE, N.SNAT, N.DNAT, N.MISS, N.HOST}
    assert (pl["kind"][x["kind"] == N.MISS] == mosrx.FWD_NAT_MISS).all()
    assert (pl["kind"][x["kind"] == N.HOST] == mosrx.FWD_NAT_HOST).all()


@pytest.mark.parametrize("nslots", [16, 256])
def test_nat_probe_edge(gpu_ctx, nslots):
    """The longest run starts in the table's last two slots and wraps: the key at depth `probe` is found,
    an absent key behind the same run is a MISS after `probe` steps."""
    pe = H.probe_edge_bindings(nslots)
    buf, off, ln = H.pack(H.probe_edge_frames(pe))
    rec = H.classify(buf, off, ln)
    for rb in (16, 8):
        x, pl = TN.check(gpu_ctx, buf, off, ln, rec, pe.bindings, rb)
        assert gpu_ctx.nat_count() == len(pe.bindings)
        assert x["kind"][-1] == N.SNAT and x["bind"][-1] == pe.k - 1             # the last-in-run key translated
        assert x["kind"][-2] == N.MISS and pl["kind"][-2] == mosrx.FWD_NAT_MISS     # the absent key
        assert np.isin(x["kind"][:-2], [N.SNAT, N.DNAT]).all()


# ---- the buffer end and len[] ------------------------------------------------------------

def cut_case(which):
    a, z = H.eligible_frame(), H.zero_segment_frame()
    c = {"eligible": lambda: H.cut_batch(a), "empty_segment": lambda: H.cut_batch(z),
         "empty_segment_on_a_line": lambda: H.cut_batch(z, H.end_phase(z))}[which]()
    cuts = H.cut_points(c.frames[256], int(c.off[256]), int(c.ln[256]))
    assert 20 <= len(cuts) <= 64 and min(cuts) >= int(c.off[255]) + int(c.ln[255])
    return c, cuts


@pytest.mark.parametrize("which", ["eligible", "empty_segment", "empty_segment_on_a_line"])
def test_firewall_cut_by_frames_bytes(gpu_ctx, which):
    """One launch per buffer end and record size; the last frame's packet, then its ports, fall behind it."""
    c, cuts = cut_case(which)
    seen = set()
    for fb in cuts:
        for rb in (16, 8):
            hit, pl = TA.check(gpu_ctx, c.buf, c.off, c.ln, H.rule_sets()["ports"], rb, frames_bytes=fb, rec=c.rec, **FW)
            assert hit[255] == 0 and pl["kind"][255] != mosrx.FWD_DROP, fb          # frame 255 stays whole
            seen.add(int(hit[256]))
    assert seen == {"eligible": {A.NOT_LOOKED_UP, 0}, "empty_segment": {A.NOT_LOOKED_UP, 0, 1},
                    "empty_segment_on_a_line": {A.NOT_LOOKED_UP, 0, 3}}[which]


@pytest.mark.parametrize("which", ["eligible", "empty_segment"])
def test_nat_cut_by_frames_bytes(gpu_ctx, which):
    c, cuts = cut_case(which)
    seen = set()
    for fb in cuts:
        for rb in (16, 8):
            x, pl = TN.check(gpu_ctx, c.buf, c.off, c.ln, c.rec, H.bindings(), rb, frames_bytes=fb)
            assert x["kind"][255] == N.SNAT and pl["kind"][255] == F.IP, fb
            seen.add(int(x["kind"][256]))
    assert seen == {N.NONE, N.SNAT if which == "eligible" else N.HOST}


@pytest.mark.parametrize("records", ["of_these_lens", "of_the_whole_frames"])
@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_len_sweep(gpu_ctx, rec_bytes, records):
    """One launch each: copies of the eligible and of the empty-segment frame, every one with another len."""
    s = H.len_sweep()
    rec = s.rec if records == "of_these_lens" else s.rec_whole
    hit, _ = TA.check(gpu_ctx, s.buf, s.off, s.ln, H.rule_sets()["ports"], rec_bytes, rec=rec, **FW)
    x, _ = TN.check(gpu_ctx, s.buf, s.off, s.ln, rec, H.bindings(), rec_bytes)
    whole = s.ln >= np.array([14 + f[16] * 256 + f[17] for f in s.frames])
    looked, taken = hit != A.NOT_LOOKED_UP, x["kind"] != N.NONE
    assert 2 <= whole.sum() < len(whole) and not looked[~whole].any() and not taken[~whole].any()
    if records == "of_the_whole_frames":
        assert (looked == whole).all() and (taken == whole).all()
        assert looked[s.ln == 34].tolist().count(True) == 1                          # looked up at len 34: the empty segment
    else:   # a capture that does not hold 20 bytes behind the IP header is TRUNCATED to the classify pass
        assert 2 <= looked.sum() < whole.sum() and (looked == taken).all() and not looked[s.ln == 34].any()


# ---- queue shapes ----------------------------------------------------------------------

def queue_setup(ctx):
    s = Setup(ctx, H.split(NS, STARTS))
    assert s.ns == NS
    return s


def classified_as_the_oracle(s):
    for d, r in zip(s.dbs, s.rec):
        assert d.results().tobytes() == r.tobytes()


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_queue_shapes_nat_byte_rings(gpu_ctx, rec_bytes):
    ctx = gpu_ctx
    s = queue_setup(ctx)
    xl = None
    try:
        t = mosrx.fwd_tables(**H.TABLES)
        ctx.fwd_set(t)
        b = H.bindings()
        ctx.nat_set(b)
        want = [N.plan(f, o, l, r["reason"], b, t, 0) for (f, o, l), r in zip(s.batches, s.rec)]
        assert all(np.isin(w[0]["kind"], [N.SNAT, N.DNAT]).sum() > 0 for w, n in zip(want, NS) if n >= 256)
        cap = max(int(FR.need_units(w[1], NR).max()) for w in want) * 16
        q, out, xl = s.queue(rec_bytes), s.outputs(cap, NR), Xlat(ctx, NS)
        out.attach(q)
        q.set_nat(xl.ptrs())
        q.run()
        if rec_bytes == 16:
            classified_as_the_oracle(s)
        check_rings(s, out, t, want)
        xl.check([w[0] for w in want])
        for i, n in enumerate(NS):
            if n == 0:      # an empty batch: zeroed rings, nothing else
                tx = out.tx(i)
                assert all((a.view(np.uint8) == 0xEE).all() for a in tx[:4]) and (tx[4][NR:].view(np.uint8) == 0xEE).all()
                assert not tx[4][:NR].view(np.uint32).any()
    finally:
        s.close()
        if xl:
            xl.free()


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_queue_shapes_firewall_descriptor_rings(gpu_ctx, rec_bytes):
    ctx = gpu_ctx
    s = queue_setup(ctx)
    out = acl = None
    try:
        rules = H.rule_sets()["last_of_full"]
        t = TA.setup(ctx, rules, tables=H.TABLES)
        base = s.want_plans(t)
        res = [A.apply(f, o, l, r, rules, p) for (f, o, l), r, p in zip(s.batches, s.rec, base)]
        want = [x[2] for x in res]
        cnt = sum(x[1].astype(np.uint64) for x in res).astype(np.uint32)
        assert [int((w["kind"] == mosrx.FWD_DROP).sum()) >= 10 for w in want] == [n >= 256 for n in NS]
        q, out, acl = s.queue(rec_bytes), DescOutputs(ctx, NS, NR), QueueAcl(ctx, NS)
        out.attach(q)
        q.set_acl([d.ptr for d in acl.d_hit], acl.d_cnt.ptr)
        q.run()
        if rec_bytes == 16:
            classified_as_the_oracle(s)
        out.check(s, t, want)           # (an empty batch: zeroed rings, nothing else)
        acl.check([x[0] for x in res], cnt)
    finally:
        s.close()
        for o in (out, acl):
            if o:
                o.free()
