"""Every refusal of the forwarding entry points, as one table: an entry point,
one defect, the expected code -- the four *_dev calls, the two queue attaches
with mosrx_queue_run, mosrx_slot_fwd with a group submit, and mosrx_time_op
(MOSRX_OP_FWD_DESC) under mosrx_set_fwd_one.

The shapes are the smallest that reach every clause: one 64-byte frame, a
2-batch queue / group whose second batch is empty (an empty batch's arrays are
not looked at, its ring rows are), 2 rings with 2 netdevs installed.  Every row
also checks that nothing was launched: all outputs are 0xEE images that must
still be 0xEE after mosrx_sync, and mosrx_fwd_one_count must not move.  An
attach row is followed by a run, which must behave as the attachment in place
before the row does.  The expected codes were read from the host code, not
taken from a run."""
import ctypes as C

import numpy as np
import pytest

import mosrx
from test_fwd_gpu import DEVS4, ip_frame, pack_at

pytestmark = pytest.mark.gpu

OK, ENOENT, E2BIG, EINVAL = 0, 2, 7, 22
NR = 2                       # rings, and netdevs installed
CAP = 256                    # ring_cap of the byte rings
SLOT = 1024                  # bytes per named output in the arenas
NAMES = ["plan0", "plan1", "tx0", "tx1", "toff0", "toff1", "tlen0", "tlen1", "tsrc0", "tsrc1", "tmac0", "tmac1",
         "rings0", "rings1", "tnif0", "tcnt0", "scr", "rec0", "rec1"]
ALIGN = dict(plan=8, tx=16, toff=4, tlen=2, tsrc=4, tmac=4, rings=16, scr=16, tcnt=4, rec=16)


def tables(netdevs=NR):
    return mosrx.fwd_tables(routes=[("10.0.0.0/8", 1), ("0.0.0.0/0", 0)], arp=[("10.0.0.0/8", "02:00:00:00:00:01")],
                            netdevs=DEVS4[:netdevs])


class Env:
    """The session's context with forwarding parameters, the two device batches and
    their queue, the two host batches, and one arena of named outputs on each side."""

    def __init__(self, ctx):
        self.ctx, self.L, self.h = ctx, mosrx.lib(), ctx.handle
        ctx.set_params(mosrx.default_params(num_msp=1, forward=1))
        ctx.fwd_set_listener(False)
        ctx.set_direct(0)
        buf, off, ln = pack_at([ip_frame("10.1.2.3", 50)], [0])
        assert int(ln[0]) == 64
        self.host = (buf, off, ln)                                  # kept alive: the host batch points into them
        self.db = ctx.upload(buf, off, ln)
        self.de = ctx.upload(np.zeros(16, np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint16))
        self.q = ctx.queue([self.db, self.de])
        self.arena = mosrx.DevBuffer(ctx, SLOT * len(NAMES))
        self.image = np.full(SLOT * len(NAMES), 0xEE, np.uint8)
        raw = np.zeros(SLOT * len(NAMES) + 64, np.uint8)
        self.hbase = (raw.ctypes.data + 63) // 64 * 64
        self.harena = raw[self.hbase - raw.ctypes.data:][:SLOT * len(NAMES)]
        self.state = "?"
        self.sb = dict(build_dev=self.L.mosrx_fwd_scratch_bytes(1), build_rings_dev=self.L.mosrx_fwd_rings_scratch_bytes(1, NR),
                       desc_rings_dev=self.L.mosrx_fwd_desc_scratch_bytes(1, NR))
        assert self.sb == dict(build_dev=16, build_rings_dev=32, desc_rings_dev=32)

    def close(self):
        self.L.mosrx_sync(self.h)
        self.ctx.set_fwd_one(0)
        self.ctx.fwd_set(None)
        self.ctx.set_params(mosrx.default_params())
        self.q.destroy()
        self.arena.free()
        self.db.free()
        self.de.free()

    def p(self, name, host=False):
        return (self.hbase if host else self.arena.ptr) + SLOT * NAMES.index(name)

    def tables(self, state):
        """'tab': 2 netdevs installed, 'tab3': 3, 'none': no tables."""
        if state != self.state:
            self.ctx.fwd_set(None if state == "none" else tables(3 if state == "tab3" else NR))
            self.state = state

    def fill(self):
        self.arena.upload(self.image)
        self.db.d_out.upload(self.image[:16])
        self.harena[...] = 0xEE

    def touched(self):
        """The names of the outputs, device and host, that are no longer 0xEE images."""
        mosrx._chk(self.L.mosrx_sync(self.h), "mosrx_sync")
        dev = self.arena.download(np.zeros_like(self.image)).reshape(len(NAMES), SLOT)
        hst = self.harena.reshape(len(NAMES), SLOT)
        out = [n for i, n in enumerate(NAMES) if (dev[i] != 0xEE).any()] + \
              ["h_" + n for i, n in enumerate(NAMES) if (hst[i] != 0xEE).any()]
        if (self.db.d_out.download(np.zeros(16, np.uint8)) != 0xEE).any():
            out.append("records")
        return out

    def refused(self, what, call, want):
        """`call` returns -want (or 0 for a row that is admitted) having launched nothing."""
        self.fill()
        c0 = self.ctx.fwd_one_count()
        rc = call()
        assert rc == -want, (what, rc, -want)
        assert self.touched() == [], what
        assert self.ctx.fwd_one_count() == c0, what


@pytest.fixture(scope="module")
def env(gpu_ctx):
    e = Env(gpu_ctx)
    yield e
    e.close()


def defects(key, base, batch=None):
    """NULL, and misaligned by half its alignment and by one byte."""
    a = ALIGN[key.rstrip("01")] if batch is None else ALIGN[key]
    k = key if batch is None else f"{key}[{batch}]"
    return [(f"{k} NULL", {k: None})] + [(f"{k} + {d}", {k: base + d}) for d in sorted({a // 2, 1})]


def patched(base, over):
    """base with the overrides applied; 'name[i]' replaces element i of a per-batch list."""
    a = {k: (list(v) if isinstance(v, list) else v) for k, v in base.items()}
    for k, v in over.items():
        if k.endswith("]"):
            name, i = k[:-1].split("[")
            a[name][int(i)] = v
        else:
            a[k] = v
    return a


def bad_batch(b, how):
    """A copy of b that mosrx__check_batch refuses with -E2BIG ('big') or whose off[] is misaligned ('off')."""
    c = mosrx.Batch.from_buffer_copy(b)
    if how == "big":
        c.frames_bytes = 1 << 40
    else:
        c.off = c.off + 2
    return c


# ---- the four *_dev calls ------------------------------------------------------------

def dev_args(e):
    return dict(b=e.db.batch(), rec=e.db.d_out.ptr, rec_bytes=16, in_ifidx=0, plan=e.p("plan0"), tx=e.p("tx0"), cap=CAP,
                nrings=NR, toff=e.p("toff0"), tlen=e.p("tlen0"), tnif=e.p("tnif0"), tsrc=e.p("tsrc0"), tcnt=e.p("tcnt0"),
                tmac=e.p("tmac0"), rings=e.p("rings0"), scr=e.p("scr"))


def dev_call(e, entry, a):
    L, h, b, sb = e.L, e.h, C.byref(a["b"]), a.get("sb", e.sb.get(entry, 0))
    if entry == "plan_dev":
        return L.mosrx_fwd_plan_dev(h, b, a["rec"], a["rec_bytes"], a["in_ifidx"], a["plan"], None)
    if entry == "build_dev":
        return L.mosrx_fwd_build_dev(h, b, a["plan"], a["tx"], a["cap"], a["toff"], a["tlen"], a["tnif"], a["tsrc"],
                                     a["tcnt"], a["scr"], sb, None)
    if entry == "build_rings_dev":
        return L.mosrx_fwd_build_rings_dev(h, b, a["plan"], a["tx"], a["cap"], a["nrings"], a["toff"], a["tlen"], a["tsrc"],
                                           a["rings"], a["scr"], sb, None)
    return L.mosrx_fwd_desc_rings_dev(h, b, a["plan"], a["nrings"], a["tsrc"], a["tlen"], a["tmac"], a["rings"], a["scr"],
                                      sb, None)


POINTERS = dict(plan_dev=["plan", "rec"], build_dev=["plan", "tx", "toff", "tlen", "tsrc", "tcnt", "scr"],
                build_rings_dev=["plan", "tx", "toff", "tlen", "tsrc", "rings", "scr"],
                desc_rings_dev=["plan", "tsrc", "tlen", "tmac", "rings", "scr"])


def dev_rows(e, entry):
    """(what, overrides, tables, expected code)."""
    base, b = dev_args(e), e.db.batch()
    rows = [(w, o, "tab", EINVAL) for k in POINTERS[entry] for w, o in defects(k, base[k])]
    rows += [("batch NULL frames", {"b": mosrx.Batch(0, 64, b.off, b.len, 1, 64)}, "tab", EINVAL),
             ("batch off + 2", {"b": bad_batch(b, "off")}, "tab", EINVAL),
             ("batch too big", {"b": bad_batch(b, "big")}, "tab", E2BIG),
             ("no tables", {}, "none", ENOENT),
             # precedence: the arguments, then the batch, then the tables
             ("plan NULL, no tables", {"plan": None}, "none", EINVAL),
             ("batch too big, no tables", {"b": bad_batch(b, "big")}, "none", E2BIG),
             ("batch off + 2, no tables", {"b": bad_batch(b, "off")}, "none", EINVAL),
             ("plan NULL, batch too big", {"plan": None, "b": bad_batch(b, "big")}, "tab", EINVAL)]
    if entry == "plan_dev":
        rows += [("rec_bytes 12", {"rec_bytes": 12}, "tab", EINVAL), ("in_ifidx 16", {"in_ifidx": 16}, "tab", EINVAL),
                 ("in_ifidx -1", {"in_ifidx": -1}, "tab", EINVAL), ("rec + 4, rec_bytes 8", {"rec": base["rec"] + 4, "rec_bytes": 8}, "tab", EINVAL),
                 ("in_ifidx 16, no tables", {"in_ifidx": 16}, "none", EINVAL)]
    else:
        rows += [("scratch one byte short", {"sb": e.sb[entry] - 1}, "tab", EINVAL),
                 ("scratch one byte short, no tables", {"sb": e.sb[entry] - 1}, "none", EINVAL)]
    if entry == "build_dev":
        rows += [("tnif NULL", {"tnif": None}, "tab", EINVAL)]
    if entry in ("build_rings_dev", "desc_rings_dev"):
        rows += [("nrings 0", {"nrings": 0}, "tab", EINVAL), ("nrings 17", {"nrings": 17}, "tab", EINVAL),
                 ("nrings 1 of 2 netdevs", {"nrings": 1}, "tab", EINVAL),
                 ("nrings 2 of 3 netdevs", {}, "tab3", EINVAL),
                 # ... then nrings against the tables' netdevs
                 ("nrings 1, no tables", {"nrings": 1}, "none", ENOENT), ("nrings 0, no tables", {"nrings": 0}, "none", EINVAL),
                 ("nrings 1, batch too big", {"nrings": 1, "b": bad_batch(b, "big")}, "tab", E2BIG)]
    if entry == "build_rings_dev":
        rows += [("ring_cap 24", {"cap": 24}, "tab", EINVAL), ("ring_cap 2^32 + 16", {"cap": (1 << 32) + 16}, "tab", EINVAL),
                 ("ring_cap 2^32 x 2 rings", {"cap": 1 << 32}, "tab", EINVAL),
                 ("ring_cap 24, no tables", {"cap": 24}, "none", EINVAL)]
    return rows


@pytest.mark.parametrize("limit", [0, mosrx.FWD_ONE_MAX])
@pytest.mark.parametrize("entry", sorted(POINTERS))
def test_dev_calls(env, entry, limit):
    e = env
    e.ctx.set_fwd_one(limit)
    try:
        for what, over, state, want in dev_rows(e, entry):
            e.tables(state)
            a = patched(dev_args(e), over)
            e.refused((entry, what), lambda: dev_call(e, entry, a), want)
        # an empty batch is planned by no launch, and its tables are not noted as read
        e.tables("tab")
        a = patched(dev_args(e), {"b": e.de.batch(), "rec": None})
        if entry == "plan_dev":
            e.refused((entry, "n == 0"), lambda: dev_call(e, entry, a), OK)
    finally:
        e.ctx.set_fwd_one(0)


# ---- MOSRX_OP_FWD_DESC under mosrx_set_fwd_one ----------------------------------------

def op_call(e, a):
    bs = (mosrx.Batch * 1)(a["b"])
    outs = (C.c_void_p * 1)(a["rec"])
    aux = (C.c_void_p * 1)(a["plan"])
    tot = C.c_float()
    return e.L.mosrx_time_op(e.h, mosrx.OP_FWD_DESC, a["rec_bytes"] | (a["in_ifidx"] << 8), bs, 1,
                             outs if a.get("outs", 1) else None, aux if a.get("aux", 1) else None, 1, 1, C.byref(tot), None)


def test_time_op_one_launch(env):
    e = env
    base, b = dev_args(e), e.db.batch()
    rows = [(w, o, "tab", EINVAL) for k in ("plan", "rec") for w, o in defects(k, base[k])]
    rows += [("rec_bytes 12", {"rec_bytes": 12}, "tab", EINVAL), ("in_ifidx 16", {"in_ifidx": 16}, "tab", EINVAL),
             ("in_ifidx -1", {"in_ifidx": -1}, "tab", EINVAL), ("no outs", {"outs": 0}, "tab", EINVAL),
             ("no aux", {"aux": 0}, "tab", EINVAL), ("batch off + 2", {"b": bad_batch(b, "off")}, "tab", EINVAL),
             ("batch NULL frames", {"b": mosrx.Batch(0, 64, b.off, b.len, 1, 64)}, "tab", EINVAL),
             ("no tables", {}, "none", ENOENT),
             # the op asks for the tables before it sizes its outputs: ahead of what the launch path refuses
             ("plan NULL, no tables", {"plan": None}, "none", ENOENT),
             ("batch off + 2, no tables", {"b": bad_batch(b, "off")}, "none", ENOENT),
             ("rec_bytes 12, no tables", {"rec_bytes": 12}, "none", EINVAL)]
    e.ctx.set_fwd_one(mosrx.FWD_ONE_MAX)
    try:
        for what, over, state, want in rows:
            e.tables(state)
            a = patched(base, over)
            e.refused(("time_op", what), lambda: op_call(e, a), want)
    finally:
        e.ctx.set_fwd_one(0)


# ---- the queue attaches and mosrx_queue_run -----------------------------------------

def lists(e, names, host=False):
    return {k: [e.p(k + "0", host), e.p(k + "1", host)] for k in names}


def ptr_array(v):
    return None if v is None else (C.c_void_p * len(v))(*v)


def attach(e, form, a):
    """mosrx_queue_set_fwd_desc ('desc') or mosrx_queue_set_fwd ('ring': with the byte rings, 'plan': plan only)."""
    ifs = (C.c_uint8 * 2)(*a["in_ifidx"]) if a["in_ifidx"] is not None else None
    if form == "desc":
        keep = [ptr_array(a[k]) for k in ("plan", "tsrc", "tlen", "tmac", "rings")]
        f = mosrx.QueueFwdDesc(C.cast(ifs, C.c_void_p), C.cast(keep[0], C.c_void_p), a["nrings"],
                               *[C.cast(x, C.c_void_p) for x in keep[1:]])
        return e.L.mosrx_queue_set_fwd_desc(e.h, e.q.handle, C.byref(f))
    keep = [ptr_array(a[k]) for k in ("plan", "tx", "toff", "tlen", "tsrc", "rings")]
    f = mosrx.QueueFwd(C.cast(ifs, C.c_void_p), C.cast(keep[0], C.c_void_p), a["cap"], a["nrings"],
                       *[C.cast(x, C.c_void_p) for x in keep[1:]])
    return e.L.mosrx_queue_set_fwd(e.h, e.q.handle, C.byref(f))


def attach_args(e, form):
    a = dict(lists(e, ["plan", "tx", "toff", "tlen", "tsrc", "tmac", "rings"]), in_ifidx=None, nrings=NR, cap=CAP)
    if form == "plan":
        a.update(tx=None, toff=None, tlen=None, tsrc=None, rings=None, nrings=0, cap=0)
    return a


def run(e):
    return e.L.mosrx_queue_run(e.h, e.q.handle, None)


WRITES = {"desc": {"plan0", "tsrc0", "tlen0", "tmac0", "rings0", "rings1", "records"},
          "ring": {"plan0", "tx0", "toff0", "tlen0", "tsrc0", "rings0", "rings1", "records"}, "plan": {"plan0", "records"}}


def runs_as(e, form, what):
    """A run forwards in `form`: the plan and both batches' ring rows are written, and of the outputs
    only one form has (tx_mac: the descriptor form, the byte rings' tx_off: the ring form) only that form's."""
    e.tables("tab")
    e.fill()
    assert run(e) == 0, what
    t = set(e.touched())
    assert WRITES[form] <= t, (what, form, t)
    assert ("tmac0" in t) == (form == "desc") and ("toff0" in t) == (form == "ring"), (what, form, t)
    assert not t & {"plan1", "tsrc1", "tlen1", "tmac1", "tx1", "toff1"}, (what, t)      # the empty batch's arrays


def attach_rows(e, form):
    base = attach_args(e, form)
    arrays = dict(desc=["plan", "tsrc", "tlen", "tmac", "rings"], ring=["plan", "tx", "toff", "tlen", "tsrc", "rings"])[form]
    rows = [(f"{k} array NULL", {k: None}, EINVAL) for k in arrays]
    for k in arrays:
        rows += [(w, o, EINVAL) for w, o in defects(k, base[k][0], 0)]
        # the empty batch: its ring rows are checked, its arrays are not looked at
        rows += [(w, o, EINVAL if k == "rings" else OK) for w, o in defects(k, base[k][1], 1)]
    rows += [("nrings 0", {"nrings": 0}, EINVAL), ("nrings 17", {"nrings": 17}, EINVAL),
             ("in_ifidx 16", {"in_ifidx": [16, 0]}, EINVAL), ("in_ifidx 16, empty batch", {"in_ifidx": [0, 16]}, EINVAL),
             ("in_ifidx 15", {"in_ifidx": [15, 15]}, OK)]
    if form == "ring":
        rows += [("ring_cap 24", {"cap": 24}, EINVAL), ("ring_cap 2^32 + 16", {"cap": (1 << 32) + 16}, EINVAL),
                 ("ring_cap 2^32 x 2 rings", {"cap": 1 << 32}, EINVAL), ("ring_cap 2^32, 1 ring", {"cap": 1 << 32, "nrings": 1}, OK)]
    return rows


@pytest.mark.parametrize("limit", [0, mosrx.FWD_ONE_MAX])
@pytest.mark.parametrize("form", ["desc", "ring"])
def test_queue_attach(env, form, limit):
    e = env
    other = "ring" if form == "desc" else "desc"
    e.ctx.set_fwd_one(limit)
    try:
        e.tables("tab")
        assert attach(e, form, attach_args(e, form)) == 0
        for what, over, want in attach_rows(e, form):
            a = patched(attach_args(e, form), over)
            e.refused((form, what), lambda: attach(e, form, a), want)
            if want:                                            # refused: the earlier attachment is in place
                runs_as(e, form, (form, what))
            else:                                               # admitted: it replaced it; back to the good one
                assert attach(e, form, attach_args(e, form)) == 0
        # attached without tables, the attach does not ask for them; the run does, and enqueues nothing
        e.tables("none")
        e.refused((form, "attach, no tables"), lambda: attach(e, form, attach_args(e, form)), OK)
        e.refused((form, "run, no tables"), lambda: run(e), ENOENT)
        e.tables("tab3")
        e.refused((form, "run, 2 rings of 3 netdevs"), lambda: run(e), EINVAL)
        e.tables("tab")
        assert attach(e, form, patched(attach_args(e, form), {"nrings": 1})) == 0
        e.refused((form, "run, 1 ring of 2 netdevs"), lambda: run(e), EINVAL)
        assert attach(e, form, attach_args(e, form)) == 0
        # the two forms exclude each other: the other's attach is refused, its detach detaches nothing
        e.refused((form, "the other form over it"), lambda: attach(e, other, attach_args(e, other)), EINVAL)
        runs_as(e, form, "after the other form's attach")
        detach_other = e.L.mosrx_queue_set_fwd if form == "desc" else e.L.mosrx_queue_set_fwd_desc
        e.refused((form, "the other form's detach"), lambda: detach_other(e.h, e.q.handle, None), OK)
        runs_as(e, form, "after the other form's detach")
        if form == "ring":                                      # the plan-only attach is the same call: it replaces
            e.refused((form, "plan only over it"), lambda: attach(e, "plan", attach_args(e, "plan")), OK)
            runs_as(e, "plan", "plan only")
            e.refused((form, "desc over plan only"), lambda: attach(e, "desc", attach_args(e, "desc")), EINVAL)
            e.refused((form, "plan only, plan[0] + 4"),
                      lambda: attach(e, "plan", patched(attach_args(e, "plan"), {"plan[0]": e.p("plan0") + 4})), EINVAL)
            e.refused((form, "tx given, rings not"),
                      lambda: attach(e, "plan", patched(attach_args(e, "plan"), {"tx": [e.p("tx0"), e.p("tx1")]})), EINVAL)
            runs_as(e, "plan", "plan only, after refusals")
    finally:
        e.ctx.set_fwd_one(0)
        e.L.mosrx_sync(e.h)
        e.L.mosrx_queue_set_fwd(e.h, e.q.handle, None)
        e.L.mosrx_queue_set_fwd_desc(e.h, e.q.handle, None)


# ---- mosrx_slot_fwd and the group submit ------------------------------------------------

def host_batches(e):
    buf, off, ln = e.host
    return [mosrx.Batch(buf.ctypes.data, len(buf), off.ctypes.data, ln.ctypes.data, 1, 64), mosrx.Batch()]


def group_args(e):
    return dict(lists(e, ["plan", "tsrc", "tlen", "tmac", "rings"], host=True), in_ifidx=None, nrings=NR, bs=host_batches(e))


def arm(e, a):
    keep = [ptr_array(a[k]) for k in ("plan", "tsrc", "tlen", "tmac", "rings")]
    ifs = (C.c_uint8 * 2)(*a["in_ifidx"]) if a["in_ifidx"] is not None else None
    o = mosrx.SlotFwdOut(C.cast(ifs, C.c_void_p), a["nrings"], *[C.cast(x, C.c_void_p) for x in keep])
    return e.L.mosrx_slot_fwd(e.h, 1, C.byref(o)), (keep, ifs, o)


def submit(e, a, between=None):
    """Arm (admitted: the per-batch pointers are the submit's to refuse), then submit and, if taken, wait."""
    rc, keep = arm(e, a)
    assert rc == 0, rc
    if between:
        e.tables(between)
    bs = (mosrx.Batch * 2)(*a["bs"])
    outs = (C.c_void_p * 2)(e.p("rec0", True), e.p("rec1", True))
    rc = e.L.mosrx_classify_host_group_submit_ex(e.h, 1, bs, 2, outs, None, None)
    if rc == 0:
        assert e.L.mosrx_classify_host_wait(e.h, 1) == 0
    del keep
    return rc


def test_slot_arm(env):
    e = env
    base = group_args(e)
    rows = [(f"{k} array NULL", {k: None}, "tab", EINVAL) for k in ("tsrc", "tlen", "tmac", "rings")]
    rows += [("nrings 0", {"nrings": 0}, "tab", EINVAL), ("nrings 17", {"nrings": 17}, "tab", EINVAL),
             ("nrings 1 of 2 netdevs", {"nrings": 1}, "tab", EINVAL), ("nrings 2 of 3 netdevs", {}, "tab3", EINVAL),
             ("no tables", {}, "none", ENOENT), ("nrings 0, no tables", {"nrings": 0}, "none", EINVAL),
             ("nrings 1, no tables", {"nrings": 1}, "none", ENOENT), ("rings array NULL, no tables", {"rings": None}, "none", EINVAL),
             # the per-batch pointers are the submit's to look at, h_plan may be absent
             ("rings[0] NULL", {"rings[0]": None}, "tab", OK), ("no h_plan", {"plan": None}, "tab", OK)]
    try:
        for what, over, state, want in rows:
            e.tables(state)
            a = patched(base, over)
            e.refused(("slot_fwd", what), lambda: arm(e, a)[0], want)
            assert e.L.mosrx_slot_fwd(e.h, 1, None) == 0
    finally:
        e.L.mosrx_slot_fwd(e.h, 1, None)


def test_group_submit(env):
    e = env
    base = group_args(e)
    big = [bad_batch(base["bs"][0], "big"), base["bs"][1]]
    late = [base["bs"][0], bad_batch(base["bs"][0], "big")]
    rows = []
    for k in ("plan", "tsrc", "tlen", "tmac"):
        rows += [(w, o, "tab", None, EINVAL) for w, o in defects(k, base[k][0], 0)]
        rows += [(w, o, "tab", None, OK) for w, o in defects(k, base[k][1], 1)]      # the empty batch's arrays
    rows += [("rings[0] NULL", {"rings[0]": None}, "tab", None, EINVAL), ("rings[1] NULL", {"rings[1]": None}, "tab", None, EINVAL),
             ("rings[0] + 2", {"rings[0]": base["rings"][0] + 2}, "tab", None, EINVAL),
             ("rings[0] + 1", {"rings[0]": base["rings"][0] + 1}, "tab", None, EINVAL),
             ("rings[1] + 2", {"rings[1]": base["rings"][1] + 2}, "tab", None, EINVAL),
             # rows aligned to 4 bytes but not 16 are admitted: they are copied back, not written in place
             ("rings[0] + 4", {"rings[0]": base["rings"][0] + 4}, "tab", None, OK),
             ("rings[1] + 8", {"rings[1]": base["rings"][1] + 8}, "tab", None, OK),
             ("in_ifidx 16", {"in_ifidx": [16, 0]}, "tab", None, EINVAL),
             ("in_ifidx 16, empty batch", {"in_ifidx": [0, 16]}, "tab", None, EINVAL),
             ("no h_plan", {"plan": None}, "tab", None, OK),
             # the tables in effect at the submit count
             ("tables cleared after the arm", {}, "tab", "none", ENOENT),
             ("3 netdevs installed after the arm", {}, "tab", "tab3", EINVAL),
             # precedence: the tables, then batch by batch its own check ahead of its forwarding outputs
             ("tables cleared, batch too big", {"bs": big}, "tab", "none", ENOENT),
             ("tables cleared, rings[0] NULL", {"rings[0]": None}, "tab", "none", ENOENT),
             ("batch 0 too big, rings[0] NULL", {"bs": big, "rings[0]": None}, "tab", None, E2BIG),
             ("batch 0 too big, rings[1] NULL", {"bs": big, "rings[1]": None}, "tab", None, E2BIG),
             ("rings[0] NULL, batch 1 too big", {"bs": late, "rings[0]": None}, "tab", None, EINVAL),
             ("batch 1 too big", {"bs": late}, "tab", None, E2BIG)]
    try:
        for limit in (0, mosrx.FWD_ONE_MAX):
            e.ctx.set_fwd_one(limit)
            for what, over, state, between, want in rows:
                e.tables(state)
                a = patched(base, over)
                if want:
                    e.refused(("group", what, limit), lambda: submit(e, a, between), want)
                    # a refused submit leaves the slot free: the arm comes off without -EBUSY
                    assert e.L.mosrx_slot_fwd(e.h, 1, None) == 0, what
                    continue
                e.fill()
                c0 = e.ctx.fwd_one_count()
                assert submit(e, a, between) == 0, what
                t = set(e.touched())
                assert {"h_rec0", "h_tsrc0", "h_tlen0", "h_tmac0", "h_rings0", "h_rings1"} <= t, (what, t)
                assert ("h_plan0" in t) == (a["plan"] is not None), (what, t)
                assert not t & {"h_plan1", "h_tsrc1", "h_tlen1", "h_tmac1", "h_rec1"}, (what, t)
                assert not [n for n in t if not n.startswith("h_")], (what, t)
                assert e.ctx.fwd_one_count() == c0 + (1 if limit else 0), what
            # a group without a frame: its ring rows zeroed on the host, nothing launched
            e.tables("tab")
            e.fill()
            c0 = e.ctx.fwd_one_count()
            assert submit(e, patched(base, {"bs": [mosrx.Batch(), mosrx.Batch()]})) == 0
            assert set(e.touched()) == {"h_rings0", "h_rings1"}
            rows_of = e.harena.reshape(len(NAMES), SLOT)
            for n in ("rings0", "rings1"):
                r = rows_of[NAMES.index(n)]
                assert not r[:16 * NR].any() and (r[16 * NR:] == 0xEE).all()
            assert e.ctx.fwd_one_count() == c0
    finally:
        e.ctx.set_fwd_one(0)
        e.L.mosrx_slot_fwd(e.h, 1, None)
