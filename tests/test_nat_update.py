"""NAT bindings added and removed in place, the parts that need no GPU: the new
ABI records against the Python mirrors, mosrx_nat_apply against a dict model
under churn (every live key found by a walk written here that steps over the
delete marker, every deleted key not found, the touch list equal to the table's
change), the 16-way collision chain with its head deleted, every refusal with
the table's bytes unchanged, -ENOSPC at exactly half of a 16-slot table, the same
churn as a stand-alone C program (plain and under -fsanitize=address,undefined),
and the update launch function's refusals that come before any launch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mosrx
import nat_cases as NC
from test_nat import big

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EEXIST, ENOENT, ENOSPC = 22, 17, 2, 28
NAT_IP = "192.0.2.1"


def keys_of(b):
    """((saddr, daddr, ports) client side, (...) server side) of one binding record."""
    return ((int(b["cli_ip"]), int(b["svr_ip"]), int(b["cli_port"]) | int(b["svr_port"]) << 16),
            (int(b["svr_ip"]), int(b["nat_ip"]), int(b["svr_port"]) | int(b["nat_port"]) << 16))


_hash = {}


def walk(slots, probe, key):
    """The lookup as the kernel makes it after this change: from the key's hash at most `probe`
    slots; kind 0 ends it, 0xFF is stepped over, SNAT / DNAT slots are compared.  The slot, or -1."""
    if key not in _hash:
        _hash[key] = mosrx.lib().mosrx_nat_hash(*key)
    h, mask = _hash[key], len(slots) - 1
    for d in range(probe):
        s = slots[(h + d) & mask]
        k = int(s["kind"])
        if k == 0xFF:
            continue
        if k not in (mosrx.NAT_SNAT, mosrx.NAT_DNAT):
            return -1
        if (int(s["saddr"]), int(s["daddr"]), int(s["ports"])) == key:
            return (h + d) & mask
    return -1


def found(slots, probe, b, bind):
    """Both keys of binding b are found, with their kind, value and id."""
    ck, sk = keys_of(b)
    a, z = walk(slots, probe, ck), walk(slots, probe, sk)
    if a < 0 or z < 0:
        return False
    a, z = slots[a], slots[z]
    return ((int(a["kind"]), int(a["addr"]), int(a["port"]), int(a["bind"])) == (mosrx.NAT_SNAT, int(b["nat_ip"]), int(b["nat_port"]), bind)
            and (int(z["kind"]), int(z["addr"]), int(z["port"]), int(z["bind"])) == (mosrx.NAT_DNAT, int(b["cli_ip"]), int(b["cli_port"]), bind))


def absent(slots, probe, b):
    return all(walk(slots, probe, k) < 0 for k in keys_of(b))


def refused(slots, st, ops, errno):
    """The ops are refused with -errno and leave the table and the state as they were."""
    before, L = slots.tobytes(), mosrx.lib()
    o = np.ascontiguousarray(ops, mosrx.NAT_OP_DTYPE)
    s = np.array(tuple(st), np.uint32)
    touch, m = np.zeros(4 * len(o), mosrx.NAT_TOUCH_DTYPE), C.c_uint32(12345)
    assert L.mosrx_nat_apply(slots.ctypes.data, s.ctypes.data, o.ctypes.data, len(o), touch.ctypes.data, C.byref(m)) == -errno
    assert slots.tobytes() == before and tuple(int(v) for v in s) == tuple(st)
    with pytest.raises(mosrx.MosrxError) as e:
        mosrx.nat_apply(slots, st, ops)
    assert e.value.errno == errno and slots.tobytes() == before


def pool(n):
    """n distinct candidate flows as binding records."""
    return mosrx.nat_bindings([(f"10.{3 + i // 200}.{i % 7}.{1 + i % 200}", 20000 + i, f"198.51.100.{1 + i % 4}", (80, 443)[i % 2],
                                1025 + i) for i in range(n)], nat_ip=NAT_IP)


def test_abi_records_and_constants():
    assert mosrx.NAT_TOMB == 0xFF and (mosrx.NAT_OP_ADD, mosrx.NAT_OP_DEL) == (1, 2)
    assert mosrx.NAT_UPDATE_MAX_OPS == 2 * mosrx.NAT_MAX_BINDINGS
    assert mosrx.NAT_OP_DTYPE.itemsize == 28 and [mosrx.NAT_OP_DTYPE.fields[k][1] for k in ("b", "op", "bind")] == [0, 20, 24]
    assert mosrx.NAT_TOUCH_DTYPE.itemsize == 48 and [mosrx.NAT_TOUCH_DTYPE.fields[k][1] for k in ("slot", "pad", "image")] == [0, 4, 16]
    assert mosrx.NAT_TOUCH_DTYPE.fields["image"][0] == mosrx.NAT_SLOT_DTYPE
    assert mosrx.NAT_STATS_DTYPE.itemsize == 32 and [mosrx.NAT_STATS_DTYPE.fields[k][1] for k in
                                                     ("live", "tombs", "slots", "probe", "updates", "rebuilds")] == [0, 4, 8, 12, 16, 24]
    L = mosrx.lib()
    assert L.mosrx_abi_version() == 3                                       # additive: the ABI version stands
    for name in ("mosrx_nat_apply", "mosrx_nat_update", "mosrx_nat_get_stats", "mosrx_launch_nat_update"):
        assert hasattr(L, name), name
    for name in ("nat_update", "nat_stats"):
        assert callable(getattr(mosrx.Context, name)), name
    f = ("10.0.0.1", 1234, "8.8.8.8", 80, 1025)
    o = mosrx.nat_ops(adds=[(f, 7)], dels=[f, mosrx.nat_bindings([f], NAT_IP)[0]], nat_ip=NAT_IP)
    assert o["op"].tolist() == [2, 2, 1] and o["bind"].tolist() == [0, 0, 7]  # the deletes first
    assert all(o["b"][i].tobytes() == mosrx.nat_bindings([f], NAT_IP)[0].tobytes() for i in range(3))
    assert o[2].tobytes() == bytes([10, 0, 0, 1, 8, 8, 8, 8, 192, 0, 2, 1, 0x04, 0xD2, 0, 80, 0x04, 0x01, 0, 0, 1, 0, 0, 0, 7, 0, 0, 0])
    assert L.mosrx_nat_get_stats(None, None) == -EINVAL and L.mosrx_nat_update(None, None, 0, None) == -EINVAL


def test_churn_against_a_dict_model():
    rng = np.random.default_rng(0x4E4154)
    cand = pool(120)
    slots, probe = mosrx.nat_table(cand[:8])
    st = mosrx.nat_state(slots, probe)
    assert st == (32, 16, 0, probe)
    live, gone, next_id = {i: i for i in range(8)}, set(), 1000     # candidate -> bind id; candidates deleted and not bound again
    rebuilds = reuse = spoilt = 0

    def rebuild():
        """An empty table with room, the live bindings added again under their ids."""
        t = np.zeros(1 << int(np.ceil(np.log2(4 * (len(live) + 24)))), mosrx.NAT_SLOT_DTYPE)
        s = mosrx.NatState(len(t), 0, 0, 0)
        if live:
            _, s = mosrx.nat_apply(t, s, mosrx.nat_ops(adds=[(cand[i], v) for i, v in live.items()]))
        return t, s

    for call in range(300):
        picks = rng.choice(len(cand), int(rng.integers(1, 17)), replace=False)
        model, dead, ops = dict(live), set(gone), np.zeros(len(picks), mosrx.NAT_OP_DTYPE)
        for k, i in enumerate(int(i) for i in picks):
            # a live candidate is deleted, another added; with 60 live the ADD is one the call must be refused for
            if i in model:
                ops[k] = (cand[i], mosrx.NAT_OP_DEL, 0)
                del model[i]
                dead.add(i)
            elif len(model) < 60:
                ops[k] = (cand[i], mosrx.NAT_OP_ADD, next_id + k)
                model[i] = next_id + k
                dead.discard(i)
            else:
                ops[k] = (cand[i], mosrx.NAT_OP_ADD, mosrx.NAT_NO_BIND)
        if (ops["bind"] == mosrx.NAT_NO_BIND).any():                       # (a full model: the ADD was made one to refuse)
            refused(slots, st, ops, EINVAL)
            spoilt += 1
            continue
        prev = slots.copy()
        try:
            touch, new = mosrx.nat_apply(slots, st, ops)
        except mosrx.MosrxError as e:
            assert e.errno == ENOSPC and slots.tobytes() == prev.tobytes()
            slots, st = rebuild()
            rebuilds += 1
            prev = slots.copy()
            touch, new = mosrx.nat_apply(slots, st, ops)
        # the touch list: distinct ascending slots whose images over the old table give the new one
        assert (np.diff(touch["slot"].astype(np.int64)) > 0).all() and len(touch) <= 2 * len(ops)
        prev[touch["slot"]] = touch["image"]
        assert prev.tobytes() == slots.tobytes()
        assert not touch["pad"].any()
        reuse += int(new.tombs < st.tombs)
        assert new.probe >= st.probe and new.slots == st.slots
        live, gone, st, next_id = model, dead, new, next_id + len(ops)
        kinds = slots["kind"]
        assert st.keys == 2 * len(live) == int(np.isin(kinds, [1, 2]).sum()) and st.tombs == int((kinds == 0xFF).sum())
        assert set(kinds.tolist()) <= {0, 1, 2, 0xFF} and st.keys + st.tombs <= st.slots // 2
        tomb = slots[kinds == 0xFF].copy()
        tomb["kind"] = 0
        assert not tomb.view(np.uint8).any()                                # a tombstone: every other byte zero
        for i, v in live.items():
            assert found(slots, st.probe, cand[i], v), (call, i)
        for i in gone:
            assert absent(slots, st.probe, cand[i]), (call, i)
    assert rebuilds >= 2 and reuse >= 5 and spoilt >= 1 and len(gone) > 20


def collision_table():
    b = NC.bindings()
    slots, probe = mosrx.nat_table(b)
    return b, slots, mosrx.nat_state(slots, probe)


def test_collision_chain_with_its_head_deleted():
    b, slots, st = collision_table()
    coll = list(range(NC.NPLAIN, NC.NPLAIN + NC.NCOLL))
    # the chain's head: the binding whose client-side key lies nearest its home slot
    home = mosrx.lib().mosrx_nat_hash(*keys_of(b[coll[0]])[0]) & 255
    head = min(coll, key=lambda i: (walk(slots, st.probe, keys_of(b[i])[0]) - home) & 255)
    assert head == coll[0] and all(found(slots, st.probe, b[i], i) for i in coll)
    touch, st1 = mosrx.nat_apply(slots, st, mosrx.nat_ops(dels=[b[head]]))
    assert len(touch) == 2 and (touch["image"]["kind"] == 0xFF).all() and (st1.keys, st1.tombs) == (st.keys - 2, 2)
    assert all(found(slots, st1.probe, b[i], i) for i in coll[1:])          # a freed slot would cut the chain here
    assert absent(slots, st1.probe, b[head]) and st1.probe == st.probe
    assert all(found(slots, st1.probe, b[i], i) for i in range(NC.NBIND) if i != head)
    # a duplicate ADD of a key that lies behind the tombstone in its own chain
    refused(slots, st1, mosrx.nat_ops(adds=[(b[coll[5]], 99)]), EEXIST)
    refused(slots, st1, mosrx.nat_ops(adds=[(b[coll[15]], 99)]), EEXIST)
    # the head again: into the tombstones it left, under a new id
    touch, st2 = mosrx.nat_apply(slots, st1, mosrx.nat_ops(adds=[(b[head], 777)]))
    assert st2.tombs < st1.tombs and st2.tombs == 0 and st2.keys == st.keys and st2.probe >= st1.probe
    assert found(slots, st2.probe, b[head], 777) and all(found(slots, st2.probe, b[i], i) for i in coll[1:])
    # the last of the chain deleted, then one added whose walk passes that tombstone and ends behind it
    tail = max(coll, key=lambda i: (walk(slots, st2.probe, keys_of(b[i])[0]) - home) & 255)
    _, st3 = mosrx.nat_apply(slots, st2, mosrx.nat_ops(dels=[b[tail]]))
    assert absent(slots, st3.probe, b[tail]) and st3.probe == st2.probe    # probe never shrinks
    assert all(found(slots, st3.probe, b[i], 777 if i == head else i) for i in coll if i != tail)


def test_every_refusal_inside_a_longer_list():
    cand = pool(12)
    slots, probe = mosrx.nat_table(cand[:6])                                # 32 slots, 12 keys
    st = mosrx.nat_state(slots, probe)
    ok_a, ok_b = (cand[6], 60), (cand[7], 70)

    def around(bad):
        o = np.concatenate([mosrx.nat_ops(adds=[ok_a], dels=[cand[0]]), bad, mosrx.nat_ops(adds=[ok_b])])
        return o

    def one(b, op, bind=5):
        o = np.zeros(1, mosrx.NAT_OP_DTYPE)
        o[0] = (b, op, bind)
        return o

    for op in (0, 3, 0xFFFFFFFF):
        refused(slots, st, around(one(cand[8], op)), EINVAL)
    for field in ("nat_ip", "nat_port"):
        for op in (mosrx.NAT_OP_ADD, mosrx.NAT_OP_DEL):
            bad = cand[8 if op == mosrx.NAT_OP_ADD else 1].copy()
            bad[field] = 0
            refused(slots, st, around(one(bad, op)), EINVAL)
    refused(slots, st, around(one(cand[8], mosrx.NAT_OP_ADD, mosrx.NAT_NO_BIND)), EINVAL)
    same_client = cand[8].copy()                                            # the client-side key of a live binding, another NAT port
    for k in ("cli_ip", "cli_port", "svr_ip", "svr_port"):
        same_client[k] = cand[2][k]
    refused(slots, st, around(one(same_client, mosrx.NAT_OP_ADD)), EEXIST)
    same_server = cand[8].copy()                                            # the server-side key of a live binding, another client
    for k in ("svr_ip", "svr_port", "nat_port"):
        same_server[k] = cand[2][k]
    refused(slots, st, around(one(same_server, mosrx.NAT_OP_ADD)), EEXIST)
    refused(slots, st, around(one(cand[6], mosrx.NAT_OP_ADD)), EEXIST)      # added earlier in the same list
    refused(slots, st, around(one(cand[9], mosrx.NAT_OP_DEL)), ENOENT)      # never bound
    refused(slots, st, around(one(cand[0], mosrx.NAT_OP_DEL)), ENOENT)      # deleted earlier in the same list
    other_port = cand[1].copy()                                             # the binding is named in full
    other_port["nat_port"] = cand[9]["nat_port"]
    refused(slots, st, around(one(other_port, mosrx.NAT_OP_DEL)), ENOENT)
    other_client = cand[1].copy()
    other_client["cli_port"] = cand[9]["cli_port"]
    refused(slots, st, around(one(other_client, mosrx.NAT_OP_DEL)), ENOENT)
    refused(slots, st, mosrx.nat_ops(adds=[(cand[i], i) for i in (6, 7, 8)]), ENOSPC)   # 18 keys in 32 slots
    for bad in (mosrx.NatState(24, 0, 0, 0), mosrx.NatState(8, 0, 0, 0), mosrx.NatState(32, 17, 0, 3), mosrx.NatState(32, 12, 5, 3)):
        refused(slots, bad, around(one(cand[8], mosrx.NAT_OP_ADD)), EINVAL)  # no table's state
    # and with the bad op taken out the list is accepted
    _, st1 = mosrx.nat_apply(slots, st, around(np.zeros(0, mosrx.NAT_OP_DTYPE)))
    assert st1.keys == 14 and st1.keys + st1.tombs <= 16


def test_more_than_the_port_pool_is_refused():
    b = big(mosrx.NAT_MAX_BINDINGS)
    slots, probe = mosrx.nat_table(b)
    st = mosrx.nat_state(slots, probe)
    assert st == (1 << 18, 2 * mosrx.NAT_MAX_BINDINGS, 0, probe)
    extra = pool(2)
    refused(slots, st, mosrx.nat_ops(dels=[b[5]], adds=[(extra[0], 1), (extra[1], 2)]), EINVAL)
    _, st1 = mosrx.nat_apply(slots, st, mosrx.nat_ops(dels=[b[5]], adds=[(extra[0], 1)]))
    assert st1.keys == st.keys and st1.tombs <= 2 and found(slots, st1.probe, extra[0], 1) and absent(slots, st1.probe, b[5])


def test_enospc_exactly_at_half_of_16_slots():
    cand = pool(8)
    slots, probe = mosrx.nat_table(cand[:0])
    st = mosrx.nat_state(slots, probe)
    assert st == (16, 0, 0, 0)
    _, st = mosrx.nat_apply(slots, st, mosrx.nat_ops(adds=[(cand[i], i) for i in range(3)]))
    assert (st.keys, st.tombs) == (6, 0)
    refused(slots, st, mosrx.nat_ops(adds=[(cand[3], 3), (cand[4], 4)]), ENOSPC)       # 10 > 8
    _, st = mosrx.nat_apply(slots, st, mosrx.nat_ops(adds=[(cand[3], 3)]))            # 8: exactly half
    assert (st.keys, st.tombs) == (8, 0)
    refused(slots, st, mosrx.nat_ops(adds=[(cand[4], 4)]), ENOSPC)
    # tombstones count: a delete makes no room, except for a key whose walk passes a tombstone
    _, st = mosrx.nat_apply(slots, st, mosrx.nat_ops(dels=[cand[1]]))
    assert (st.keys, st.tombs) == (6, 2)
    # cand[4]: its client-side key's home slot is one of the two tombstones, its server-side key's walk passes none
    # and needs a free slot: 7 + 1 + 1 > 8, and the first key's write is undone
    homes = [mosrx.lib().mosrx_nat_hash(*k) & 15 for k in keys_of(cand[4])]
    assert int(slots[homes[0]]["kind"]) == 0xFF and walk(slots, 16, keys_of(cand[4])[1]) < 0
    assert all(int(slots[(homes[1] + d) & 15]["kind"]) != 0xFF for d in range(2)) and int(slots[(homes[1] + 1) & 15]["kind"]) == 0
    refused(slots, st, mosrx.nat_ops(adds=[(cand[4], 4)]), ENOSPC)
    _, st = mosrx.nat_apply(slots, st, mosrx.nat_ops(adds=[(cand[1], 11)]))           # its own tombstones lie on its walks
    assert (st.keys, st.tombs) == (8, 0) and found(slots, st.probe, cand[1], 11)
    # a delete and an add in one call: the sum is held at every op, not at the end
    refused(slots, st, mosrx.nat_ops(dels=[cand[0], cand[2], cand[3]], adds=[(cand[i], i) for i in (0, 2, 3, 4)]), ENOSPC)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_update_arithmetic_standalone(tmp_path, flags):
    exe = tmp_path / "nat_update_driver"
    csrc = os.path.join(ROOT, "mos-networking-stack_amd", "csrc")
    b = subprocess.run(["gcc", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + csrc,
                        os.path.join(ROOT, "tests", "csrc", "nat_update_driver.c"), os.path.join(csrc, "nat_table.c"),
                        "-o", str(exe)], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert r.stdout.startswith("checked ") and int(words[1]) >= 200000 and int(words[6]) > 0 and int(words[8]) > 0


def test_update_launch_refuses_before_any_launch():
    L = mosrx.lib()
    buf = (C.c_uint8 * 1024)()
    a = (C.addressof(buf) + 15) & ~15
    assert L.mosrx_launch_nat_update(None, 15, a, 1, None) == -EINVAL
    assert L.mosrx_launch_nat_update(a, 15, None, 1, None) == -EINVAL
    assert L.mosrx_launch_nat_update(a + 8, 15, a + 512, 1, None) == -EINVAL
    assert L.mosrx_launch_nat_update(a, 15, a + 512 + 4, 1, None) == -EINVAL
    for mask in (0, 7, 14, 16, 0xFFFFFFFE, 0xFFFFFFFF):
        assert L.mosrx_launch_nat_update(a, mask, a + 512, 1, None) == -EINVAL, mask
    assert L.mosrx_launch_nat_update(None, 15, None, 0, None) == -EINVAL     # m == 0 excuses nothing
    assert L.mosrx_nat_update(None, a, 1, None) == -EINVAL and L.mosrx_nat_get_stats(None, a) == -EINVAL
