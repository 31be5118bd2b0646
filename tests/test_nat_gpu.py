"""NAT translation on the GPU (mosrx_fwd_plan_nat_dev, mosrx_nat_patch_rings_dev)
against its restatement (tests/nat_oracle.py) and the recorded answers of
tests/golden/nat.npz.

The plan, the xlat records and every TX array are 0xEE images with canary entries
behind them; the restatement's answers are laid over copies of the same images
and the comparison is exact, so padding, ring tails, dropped frames' entries and
entries past the last ring are part of it.  Expected values never come from the
GPU: the records are the oracle's (the short-segment frames forced to TCP_OK, see
tests/nat_cases.py), the checks are the oracle's full recompute, the rings are
fwd_rings_oracle.build over the translated frames."""
import ctypes as C
import os

import numpy as np
import pytest

import fwd_rings_oracle as FR
import mosrx
import nat_cases as NC
import nat_oracle as N
import oracle_py as O
from test_acl_gpu import rec8_of
from test_fwd_gpu import Run, ee, pack_at
from test_fwd_rings_gpu import RingRun, assert_same, download

pytestmark = pytest.mark.gpu

EINVAL, ENOENT = 22, 2
PHASES = [2, 7, 0, 13, 1, 11]     # frames at odd offsets, every offset mod 4
NR = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nat.npz")


class NatRun(RingRun):
    """A batch on the GPU with its xlat image; the records are uploaded as given."""

    def __init__(self, ctx, buf, off, ln, rec, rec_bytes=16, frames_bytes=None):
        Run.__init__(self, ctx, buf, off, ln, rec_bytes, frames_bytes)
        if self.n:
            self.d_rec.upload(rec if rec_bytes == 16 else rec8_of(rec))
        self.x_init = ee(self.n + 2, mosrx.NAT_XLAT_DTYPE)
        self.d_xlat = mosrx.DevBuffer(ctx, self.x_init.nbytes)
        self.d_xlat.upload(self.x_init)
        self.bufs.append(self.d_xlat)

    def plan_nat(self, in_ifidx=0):
        self.ctx.fwd_plan_nat_dev(self.db.batch(), self.d_rec.ptr, self.rb, in_ifidx, self.d_plan.ptr, self.d_xlat.ptr)

    def xlat(self):
        return self.d_xlat.download(np.zeros_like(self.x_init))

    def patch(self, dev, nrings=NR):
        self.ctx.nat_patch_rings_dev(self.d_xlat.ptr, dev[0].ptr, dev[1].ptr, dev[3].ptr, dev[4].ptr, nrings, self.n)


def setup(ctx, bindings, forward=1, listener=False):
    ctx.set_params(mosrx.default_params(num_msp=1, forward=forward))
    ctx.fwd_set_listener(listener)
    t = mosrx.fwd_tables(**NC.TABLES)
    ctx.fwd_set(t)
    ctx.nat_set(bindings)
    return t


def same_records(got, want, what):
    bad = np.nonzero(got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1))[0]
    bad = np.unique(bad)
    assert not len(bad), (what, [(int(i), got[i].tolist(), want[i].tolist()) for i in bad[:6]])


def check(ctx, buf, off, ln, rec, bindings, rec_bytes=16, frames_bytes=None, caps=("exact",), forward=1, listener=False,
          translated=None):
    """plan-nat, the ring build and the patch on the GPU equal the restatement; returns (xlat, plan)."""
    t = setup(ctx, bindings, forward, listener)
    x, pl, tr = N.plan(buf, off, ln, rec["reason"], bindings, t, 0, forward=forward, listener=listener,
                       frames_bytes=frames_bytes)
    if translated is not None:
        assert tr.tobytes() == translated.tobytes()
    other = ~np.isin(x["kind"], [N.SNAT, N.DNAT])
    assert not (x["addr"][other].any() or x["port"][other].any() or x["ip_check"][other].any() or x["tcp_check"][other].any())
    r = NatRun(ctx, buf, off, ln, rec, rec_bytes, frames_bytes)
    try:
        r.plan_nat(0)
        same_records(r.plan_result(), pl, "plan")
        ex = r.x_init.copy()
        ex[:r.n] = x
        same_records(r.xlat(), ex, "xlat")
        need = FR.need_units(pl, NR)
        for cap in caps:
            cap = max(int(need.max()) * 16, 16) if cap == "exact" else cap
            dev, init = r.build_rings(cap, NR)
            r.patch(dev)
            exp = FR.build(tr, off, pl, t, cap, NR, *init)
            assert_same(download(dev, init), exp, ("cap", cap))
        return x, pl
    finally:
        r.free()


def trace(n):
    buf, off, ln = pack_at(NC.mix(n), PHASES)
    return buf, off, ln, NC.forced(O.classify(buf, off, ln, O.params(num_msp=1, forward=1)), n)


@pytest.mark.parametrize("rec_bytes", [16, 8])
@pytest.mark.parametrize("n", [1, 255, 257, 513])
def test_mixed_batches(gpu_ctx, n, rec_bytes):
    buf, off, ln, rec = trace(n)
    x, pl = check(gpu_ctx, buf, off, ln, rec, NC.bindings(), rec_bytes)
    if n == 1:
        assert x["kind"][0] == N.SNAT
        return
    tcp = (buf[off.astype(np.int64) + 12] == 8) & (buf[off.astype(np.int64) + 23] == 6)
    xl = np.isin(x["kind"], [N.SNAT, N.DNAT])
    assert xl.sum() >= 0.8 * tcp.sum()
    assert {int(k) for k in x["kind"]} == {N.NONE, N.SNAT, N.DNAT, N.MISS, N.HOST}
    assert {5, 6, 15} <= {int(v) for v in x["ihl"][xl]} and {int(o) % 4 for o in off} == {0, 1, 2, 3}
    coll = xl & (x["bind"] >= NC.NPLAIN) & (x["bind"] < NC.NPLAIN + NC.NCOLL)
    assert len(set(x["bind"][coll].tolist())) == NC.NCOLL                           # the 16-way collision set, all found
    dn = x["kind"] == N.DNAT
    assert (pl["kind"][dn] == 4).any() and (pl["out_ifidx"][dn & (pl["kind"] == 1)] == 1).all()   # NO_ARP; clients' netdev
    assert (pl["kind"][x["kind"] == N.MISS] == mosrx.FWD_NAT_MISS).all() and (pl["kind"][x["kind"] == N.HOST] == mosrx.FWD_NAT_HOST).all()
    inv = mosrx.R
    assert (x["kind"][np.isin(rec["reason"], [inv["TCP_BADCSUM"], inv["NOT_TCP"], inv["ARP"]])] == N.NONE).all()


def test_dnat_leaves_by_another_netdev_than_the_received_daddr(gpu_ctx):
    """The received daddr (the NAT's) routes to netdev 0, the translated one to netdev 1."""
    buf, off, ln, rec = trace(50)
    import fwd_oracle as F
    t = mosrx.fwd_tables(**NC.TABLES)
    base = F.plan(buf, off, ln, rec["reason"], t, 0)
    x, pl = check(gpu_ctx, buf, off, ln, rec, NC.bindings())
    dn = (x["kind"] == N.DNAT) & (pl["kind"] == 1)
    assert dn.sum() > 5 and (base["out_ifidx"][dn] == 0).all() and (pl["out_ifidx"][dn] == 1).all()


def test_ring_overflow_leaves_dropped_entries_alone(gpu_ctx):
    buf, off, ln, rec = trace(257)
    t = mosrx.fwd_tables(**NC.TABLES)
    _, pl, _ = N.plan(buf, off, ln, rec["reason"], NC.bindings(), t, 0)
    half = int(FR.need_units(pl, NR).max()) * 16 // 2 // 16 * 16
    check(gpu_ctx, buf, off, ln, rec, NC.bindings(), caps=("exact", half, 16))


@pytest.mark.parametrize("rec_bytes", [16, 8])
def test_frame_cut_by_frames_bytes(gpu_ctx, rec_bytes):
    """The last frame (a client-side frame of a bound flow, its record TCP_OK) is cut inside its packet, and
    then ends with its packet exactly at the buffer's end."""
    buf, off, ln, rec = trace(257)
    assert rec["reason"][256] == mosrx.R["TCP_OK"]
    x, _ = check(gpu_ctx, buf, off, ln, rec, NC.bindings(), rec_bytes, frames_bytes=int(off[256]) + 40)
    assert x["kind"][256] == N.NONE and x["kind"][254] != N.NONE
    x, _ = check(gpu_ctx, buf, off, ln, rec, NC.bindings(), rec_bytes, frames_bytes=int(off[256]) + int(ln[256]))
    assert x["kind"][256] == N.SNAT


def test_listener_forward_off_and_empty_table(gpu_ctx):
    buf, off, ln, rec = trace(300)
    try:
        x, pl = check(gpu_ctx, buf, off, ln, rec, NC.bindings(), listener=True)
        assert not x["kind"].any()
        x, pl = check(gpu_ctx, buf, off, ln, rec, NC.bindings(), forward=0)
        assert (x["kind"] == N.SNAT).sum() > 50 and not pl["kind"].any()             # translated all the same, the plan stays NONE
        x, pl = check(gpu_ctx, buf, off, ln, rec, np.zeros(0, mosrx.NAT_BINDING_DTYPE))
        assert gpu_ctx.nat_count() == 0 and set(x["kind"].tolist()) == {N.NONE, N.MISS, N.HOST}
        x, pl = check(gpu_ctx, buf, off, ln, rec, NC.bindings()[:1])
        assert gpu_ctx.nat_count() == 1 and 0 < np.isin(x["kind"], [N.SNAT, N.DNAT]).sum() < 20
    finally:
        gpu_ctx.fwd_set_listener(False)
        gpu_ctx.set_params(mosrx.default_params())


def test_fixture(gpu_ctx):
    z = np.load(GOLDEN)
    buf, off, ln = z["frames"], z["off"], z["len"]
    rec = np.zeros(len(off), mosrx.RESULT_DTYPE)
    rec["reason"] = z["reason"]
    for rb in (16, 8):
        x, pl = check(gpu_ctx, buf, off, ln, rec, z["bindings"], rb, translated=z["translated"])
        assert x.tobytes() == z["xlat"].tobytes() and pl.tobytes() == z["plan"].tobytes()


def test_full_pool_of_bindings(gpu_ctx):
    """64510 bindings (8 MiB of slots, the longest probe run the host recorded) around the trace's own."""
    from test_nat import big
    b = np.concatenate([NC.bindings(), big(mosrx.NAT_MAX_BINDINGS - NC.NBIND)])
    b["svr_ip"][NC.NBIND:] = mosrx.ip_raw("203.0.113.7")            # another server: every key apart from the trace's
    assert mosrx.lib().mosrx_nat_check(b.ctypes.data, len(b)) == 0
    buf, off, ln, rec = trace(257)
    x, _ = check(gpu_ctx, buf, off, ln, rec, b)
    assert gpu_ctx.nat_count() == mosrx.NAT_MAX_BINDINGS and np.isin(x["kind"], [N.SNAT, N.DNAT]).sum() > 190
    # the pool rotates: more sets than it has copies, tables of different sizes, then the launch again
    for _ in range(3):
        gpu_ctx.nat_set(NC.bindings())
        gpu_ctx.nat_set(b)
    check(gpu_ctx, buf, off, ln, rec, NC.bindings())


def test_refusals_launch_nothing(gpu_ctx):
    ctx, L = gpu_ctx, mosrx.lib()
    buf, off, ln, rec = trace(100)
    setup(ctx, NC.bindings())
    r = NatRun(ctx, buf, off, ln, rec)
    try:
        b = r.db.batch()
        empty = mosrx.Batch(b.frames, b.frames_bytes, b.off, b.len, 0, 0)

        def call(c=ctx, **kw):
            return L.mosrx_fwd_plan_nat_dev(c.handle, C.byref(kw.get("b", b)), kw.get("rec", r.d_rec.ptr), kw.get("rb", 16),
                                            kw.get("nif", 0), kw.get("plan", r.d_plan.ptr), kw.get("xlat", r.d_xlat.ptr), None)
        for kw in (dict(rec=None), dict(rec=r.d_rec.ptr + 8), dict(rb=4), dict(rb=0), dict(nif=-1), dict(nif=16),
                   dict(plan=None), dict(plan=r.d_plan.ptr + 4), dict(xlat=None), dict(xlat=r.d_xlat.ptr + 8)):
            assert call(**kw) == -EINVAL, kw
        ctx.set_params(mosrx.default_params(num_msp=1, forward=1, skip_tcp_csum=1))
        assert call() == -EINVAL and call(b=empty) == -EINVAL                       # never summed: no incremental check
        ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
        ctx.fwd_set(None)
        assert call() == -ENOENT and call(b=empty) == -ENOENT                       # no forwarding tables
        with mosrx.Context(0) as fresh:                                             # tables, but mosrx_nat_set never called
            fresh.set_params(mosrx.default_params(num_msp=1, forward=1))
            fresh.fwd_set(mosrx.fwd_tables(**NC.TABLES))
            assert fresh.nat_count() == 0 and call(c=fresh) == -ENOENT
            mosrx._chk(L.mosrx_sync(fresh.handle), "sync")
        setup(ctx, NC.bindings())
        assert call(b=empty) == 0                                                   # n == 0: nothing to launch
        bad = NC.bindings().copy()
        bad["nat_port"][3] = 0
        assert L.mosrx_nat_set(ctx.handle, bad.ctypes.data, len(bad)) == -EINVAL and ctx.nat_count() == NC.NBIND
        dev, init = r.build_rings(4096, NR)                                          # (over the 0xEE plan: nothing is sent)

        def patch(**kw):
            return L.mosrx_nat_patch_rings_dev(ctx.handle, kw.get("xlat", r.d_xlat.ptr), kw.get("tx", dev[0].ptr),
                                               kw.get("off", dev[1].ptr), kw.get("src", dev[3].ptr),
                                               kw.get("rings", dev[4].ptr), kw.get("nr", NR), kw.get("n", r.n), None)
        for kw in (dict(xlat=None), dict(xlat=r.d_xlat.ptr + 8), dict(tx=None), dict(tx=dev[0].ptr + 4), dict(off=None),
                   dict(off=dev[1].ptr + 2), dict(src=None), dict(src=dev[3].ptr + 2), dict(rings=None),
                   dict(rings=dev[4].ptr + 8), dict(nr=0), dict(nr=17)):
            assert patch(**kw) == -EINVAL, kw
        assert patch(n=0) == 0
        mosrx._chk(L.mosrx_sync(ctx.handle), "sync")
        assert r.xlat().tobytes() == r.x_init.tobytes()                              # nothing ran
        assert r.plan_result().view(np.uint64).tolist() == [0xEEEEEEEEEEEEEEEE] * r.n
    finally:
        L.mosrx_sync(ctx.handle)
        ctx.set_params(mosrx.default_params())
        r.free()


def test_timing_op(gpu_ctx):
    ctx = gpu_ctx
    t = setup(ctx, NC.bindings())
    buf, off, ln, rec = trace(300)
    db = ctx.upload(buf, off, ln)
    plan = mosrx.DevBuffer(ctx, 8 * 300)
    try:
        ctx.classify_dev(db)
        db.d_out.upload(rec)                                        # (the short-segment frames' forced reason)
        bs =(mosrx.Batch * 1)(db.batch())
        outs, aux = (C.c_void_p * 1)(db.d_out.ptr), (C.c_void_p * 1)(plan.ptr)
        tot, avg = C.c_float(), C.c_float()
        L = mosrx.lib()
        assert L.mosrx_time_op(ctx.handle, mosrx.OP_FWD_NAT, 16, bs, 1, outs, aux, 4, 1, C.byref(tot), C.byref(avg)) == 0
        assert tot.value > 0 and avg.value > 0
        _, pl, _ = N.plan(buf, off, ln, rec["reason"], NC.bindings(), t, 0)
        assert plan.download(np.zeros(300, mosrx.FWD_DTYPE)).tobytes() == pl.tobytes()
        assert L.mosrx_time_op(ctx.handle, mosrx.OP_FWD_NAT, 12, bs, 1, outs, aux, 4, 1, C.byref(tot), None) == -EINVAL
        assert L.mosrx_time_op_dispatch(ctx.handle, mosrx.OP_FWD_NAT, 16, bs, 1, outs, aux, 2, C.byref(avg)) == -95   # ENOTSUP
    finally:
        plan.free()
        db.free()
