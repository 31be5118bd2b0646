"""mosrx — Python mirror of the MI355X rx classifier's C ABI (include/mosrx.h).

Thin ctypes binding over the in-tree ``libmosrx.so``; every call goes to the
HIP path.  There is no CPU fallback: when the library or a gfx950 GPU is
missing, ``Context()`` raises.

The names mirror mOS's receive path: ``classify`` is ProcessPacket
(core/src/eth_in.c:27) over a batch, records carry the verdict it returns plus
the raw ip_fast_csum / TCPCalcChecksum values and the GetRSSHash /
GetRSSCPUCore outputs (core/src/util.c:61-131).
"""
from __future__ import annotations

import collections
import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(PKG_DIR, "libmosrx.so")

RESULT_DTYPE = np.dtype([
    ("rss", "<u4"), ("ip_csum", "<u2"), ("tcp_csum", "<u2"), ("payloadlen", "<u2"),
    ("payload_off", "u1"), ("verdict", "i1"), ("reason", "u1"), ("queue", "u1"),
    ("tcp_flags", "u1"), ("ihl_doff", "u1"),
])
assert RESULT_DTYPE.itemsize == 16

REASONS = ["TCP_OK", "ARP", "NON_IPV4", "IP_SHORT", "IP_BADVER", "NOVERIFY_PASS", "IP_BADCSUM",
           "NOT_TCP", "TCP_SHORT", "TCP_BADCSUM", "TRUNCATED", "TCP_LEN_OK", "ICMP_LOCAL"]
R = {name: i for i, name in enumerate(REASONS)}
NREASON = len(REASONS)
MAX_LOCAL = 16

# mosrx_tcpinfo: pkt_info's TCP fields (FillPacketContextTCPInfo, tcp.c:258-270), host order
TCPINFO_DTYPE = np.dtype([("seq", "<u4"), ("ack_seq", "<u4"), ("window", "<u2"), ("ip_len", "<u2")])
assert TCPINFO_DTYPE.itemsize == 12
# mosrx_result8: the compact record (rss, reason, queue, verdict, tcp_flags)
RESULT8_DTYPE = np.dtype([("rss", "<u4"), ("reason", "u1"), ("queue", "u1"), ("verdict", "i1"),
                          ("tcp_flags", "u1")])
assert RESULT8_DTYPE.itemsize == 8
QUEUE_COMPACT = 1
HOST_PINNED = 1
KIND_SMALL, KIND_S13 = 0, 1


def shape_variant(kind: int, nt_tails: bool = True) -> int:
    """mosrx_set_variant value forcing a kernel shape (bits 2-6 = kind + 1; bit 1 = nt tails)."""
    return ((kind + 1) << 2) | (2 if nt_tails else 0)

QMAP_I40E, QMAP_IXGBE = 1, 0
TRACE_FW64, TRACE_S64, TRACE_M1500, TRACE_IMIX = 0, 1, 2, 3
TRACE_SEED_BASE = 0x6D4F5321   # MOSRX_TRACE_SEED: seed 0 selects TRACE_SEED_BASE + kind
WINDOW_END = 78       # MOSRX_WINDOW_END_SMALL: batches whose frames all fit take the SMALL tile

MS_KEY = bytes([0x6d, 0x5a, 0x56, 0xda, 0x25, 0x5b, 0x0e, 0xc2, 0x41, 0x67, 0x25, 0x3d, 0x43, 0xa3,
                0x8f, 0xb0, 0xd0, 0xca, 0x2b, 0xcb, 0xae, 0x7b, 0x30, 0xb4, 0x77, 0xcb, 0x2d, 0xa3,
                0x80, 0x30, 0xf2, 0x0c, 0x6a, 0x42, 0xb7, 0x3b, 0xbe, 0xac, 0x01, 0xfa])


class Params(C.Structure):
    """mosrx_params: the mOS stack state the verdict depends on."""
    _fields_ = [("num_msp", C.c_uint32), ("num_esp", C.c_uint32), ("forward", C.c_int32),
                ("num_queues", C.c_int32), ("queue_mode", C.c_int32), ("skip_tcp_csum", C.c_int32),
                ("rss_key_len", C.c_uint32), ("rss_key", C.c_uint8 * 52),
                ("num_local", C.c_uint32), ("local_ip", C.c_uint32 * MAX_LOCAL)]


def ip_raw(a: str) -> int:
    """Dotted quad -> the raw u32 mOS keeps in netdev ip_addr (network order, loaded little-endian)."""
    return int.from_bytes(bytes(int(x) for x in a.split(".")), "little")


class Batch(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("frames_bytes", C.c_uint64), ("off", C.c_void_p),
                ("len", C.c_void_p), ("n", C.c_uint32), ("max_len", C.c_uint32),
                ("layout", C.c_uint32), ("off0", C.c_uint32), ("stride", C.c_uint32), ("reserved", C.c_uint32)]


BATCH_UNIFORM = 1   # mosrx_batch.layout: frame i expected at off0 + i * stride (a hint; off[] decides)


def uniform_layout(off: np.ndarray):
    """(off0, stride) when off[i] == off[0] + i * stride for every i (a fixed-stride
    packing, as a ring of equal-size frames has), else None."""
    off = np.asarray(off)
    if len(off) < 2:
        return None
    st = int(off[1]) - int(off[0])
    if st <= 0 or not (np.diff(off.astype(np.int64)) == st).all():
        return None
    return int(off[0]), st


def with_hint(b: Batch, hint) -> Batch:
    """b with the layout hint (off0, stride) set (None: no hint)."""
    if hint is not None:
        b.layout, b.off0, b.stride = BATCH_UNIFORM, int(hint[0]), int(hint[1])
    return b


BPF_INSN = np.dtype([("code", "<u2"), ("jt", "u1"), ("jf", "u1"), ("k", "<u4")])   # mosrx_bpf_insn
BPF_LEN_FRAME, BPF_LEN_IP = 0, 1
TX_IP_CSUM, TX_TCP_CSUM = 1 << 4, 1 << 5   # MOS_UPDATE_IP_CHKSUM / MOS_UPDATE_TCP_CHKSUM
OP_CLASSIFY, OP_CLASSIFY_FH, OP_BPF, OP_TX_CSUM, OP_CLASSIFY_BPF, OP_CLASSIFY_TI, OP_TX_CHECKS = 0, 1, 2, 3, 4, 5, 6
OP_STEER = 7           # MOSRX_OP_STEER: the steer sequence over a batch's records (arg = rec_bytes)
OP_STEER_GATHER = 8    # MOSRX_OP_STEER_GATHER: ... with the scatter launch in its gather form
OP_STEER_GATHER_SIDE = 9   # MOSRX_OP_STEER_GATHER_SIDE: ... in its side form (arg = rec_bytes | SIDE_* bits << 8)
SIDE_FHASH, SIDE_MATCH, SIDE_TCPINFO = 1, 2, 4   # MOSRX_SIDE_*
STEER_QSLOTS = 257     # MOSRX_STEER_QSLOTS: qstart entries per batch
STEER_ONE_MAX = 65536  # MOSRX_STEER_ONE_MAX: the most frames per batch the one-launch steer form takes
FWD_ONE_MAX = 8192     # MOSRX_FWD_ONE_MAX: the most frames per batch the one-launch forwarding form takes
# include/mosrx.h mosrx_tx_check: the TX checks of a frame, the frame untouched
TX_CHECK_DTYPE = np.dtype([("ip_check", "<u2"), ("tcp_check", "<u2"), ("what", "u1"), ("ihl", "u1"),
                           ("pad", "<u2")])
BPF_MAX_PROGS = 32

# ---- forwarding (include/mosrx.h: mosrx_fwd_tables, mosrx_fwd) ----
OP_FWD_PLAN = 10       # MOSRX_OP_FWD_PLAN: the forwarding plan (arg = rec_bytes | in_ifidx << 8)
OP_FWD = 11            # MOSRX_OP_FWD: plan + build
OP_FWD_RINGS = 12      # MOSRX_OP_FWD_RINGS: plan + the ring form of the build (one ring per netdev)
OP_FWD_DESC = 13       # MOSRX_OP_FWD_DESC: plan + the descriptor form of the ring build
FWD_MAX_ROUTES, FWD_MAX_ARP, FWD_MAX_NETDEVS = 128, 1024, 16
FWD_NONE, FWD_IP, FWD_ETH, FWD_NO_ROUTE, FWD_NO_ARP, FWD_NO_NIC = range(6)   # MOSRX_FWD_*
# mosrx_fwd: the plan of one frame
FWD_DTYPE = np.dtype([("tx_len", "<u2"), ("out_ifidx", "i1"), ("kind", "u1"), ("arp_idx", "<u2"),
                      ("reserved", "<u2")])
assert FWD_DTYPE.itemsize == 8
# mosrx_fwd_ring: one TX ring (output netdev) of mosrx_fwd_build_rings_dev
FWD_RING_DTYPE = np.dtype([("start", "<u4"), ("count", "<u4"), ("dropped", "<u4"), ("units", "<u4")])
assert FWD_RING_DTYPE.itemsize == 16


class FwdRoute(C.Structure):
    _fields_ = [("mask", C.c_uint32), ("masked_ip", C.c_uint32), ("prefix", C.c_int32), ("nif", C.c_int32)]


class FwdArp(C.Structure):
    _fields_ = [("ip", C.c_uint32), ("mask", C.c_uint32), ("masked_ip", C.c_uint32), ("prefix", C.c_int32),
                ("haddr", C.c_uint8 * 6), ("pad", C.c_uint8 * 2)]


class FwdTables(C.Structure):
    """mosrx_fwd_tables: the route / ARP / netdev / nic_forward fields mOS holds after mos.conf."""
    _fields_ = [("num_routes", C.c_uint32), ("num_arp", C.c_uint32), ("num_netdevs", C.c_uint32),
                ("has_nic_fwd", C.c_int32), ("nic_fwd", C.c_int8 * FWD_MAX_NETDEVS),
                ("netdev_haddr", (C.c_uint8 * 6) * FWD_MAX_NETDEVS), ("routes", FwdRoute * FWD_MAX_ROUTES),
                ("arp", FwdArp * FWD_MAX_ARP)]


class QueueFwd(C.Structure):
    """mosrx_queue_fwd: forwarding outputs attached to a batch queue (Queue.set_fwd)."""
    _fields_ = [("in_ifidx", C.c_void_p), ("d_plan", C.c_void_p), ("ring_cap", C.c_uint64), ("nrings", C.c_uint32),
                ("d_tx_frames", C.c_void_p), ("d_tx_off", C.c_void_p), ("d_tx_len", C.c_void_p),
                ("d_tx_src", C.c_void_p), ("d_rings", C.c_void_p)]


class QueueFwdDesc(C.Structure):
    """mosrx_queue_fwd_desc: the descriptor form attached to a batch queue (Queue.set_fwd_desc)."""
    _fields_ = [("in_ifidx", C.c_void_p), ("d_plan", C.c_void_p), ("nrings", C.c_uint32), ("d_tx_src", C.c_void_p),
                ("d_tx_len", C.c_void_p), ("d_tx_mac", C.c_void_p), ("d_rings", C.c_void_p)]


class SlotFwdOut(C.Structure):
    """mosrx_slot_fwd_out: forwarding outputs armed on a slot's next group submit (Context.slot_fwd)."""
    _fields_ = [("in_ifidx", C.c_void_p), ("nrings", C.c_uint32), ("h_plan", C.c_void_p), ("h_tx_src", C.c_void_p),
                ("h_tx_len", C.c_void_p), ("h_tx_mac", C.c_void_p), ("h_rings", C.c_void_p)]


def conf_mask(prefix: int) -> int:
    """htonl((prefix == 0) ? 0 : ((-1) << (32 - prefix))) as config.c:316, :346 store it
    (network order, the raw u32 of a little-endian host)."""
    host = 0 if prefix == 0 else (0xFFFFFFFF << (32 - prefix)) & 0xFFFFFFFF
    return int.from_bytes(host.to_bytes(4, "big"), "little")


def mac_bytes(m: str) -> bytes:
    b = bytes(int(x, 16) for x in m.split(":"))
    assert len(b) == 6, m
    return b


def fwd_tables(routes=(), arp=(), netdevs=(), nic_fwd=None) -> FwdTables:
    """The tables of a mos.conf: routes [("10.0.0.0/8", nif)], arp [("10.1.0.0/16",
    "02:00:00:00:00:01")], netdevs ["02:..", ...] (each netdev's haddr), nic_fwd
    None (no nic_forward_table) or {in_ifidx: out_ifidx} (the others -1).  mask
    and masked_ip exactly as FeedArpConfLine / FeedRouteConfLine compute them
    (config.c:314-317, 345-348); prefixes 0..32."""
    t = FwdTables()
    assert len(routes) <= FWD_MAX_ROUTES and len(arp) <= FWD_MAX_ARP and len(netdevs) <= FWD_MAX_NETDEVS
    t.num_routes, t.num_arp, t.num_netdevs = len(routes), len(arp), len(netdevs)
    for i, m in enumerate(netdevs):
        t.netdev_haddr[i][:] = list(mac_bytes(m))
    for i, (cidr, nif) in enumerate(routes):
        a, p = cidr.split("/")
        p = int(p)
        assert 0 <= p <= 32, cidr
        r = t.routes[i]
        r.mask = conf_mask(p)
        r.masked_ip = r.mask & ip_raw(a)
        r.prefix, r.nif = p, int(nif)
    for i, (cidr, mac) in enumerate(arp):
        a, p = cidr.split("/")
        p = int(p)
        assert 0 <= p <= 32, cidr
        e = t.arp[i]
        e.ip = ip_raw(a)
        e.prefix = p
        e.mask = conf_mask(p)
        e.masked_ip = e.mask & e.ip
        e.haddr[:] = list(mac_bytes(mac))
    t.has_nic_fwd = 0 if nic_fwd is None else 1
    for i in range(FWD_MAX_NETDEVS):
        t.nic_fwd[i] = -1 if nic_fwd is None else int(dict(nic_fwd).get(i, -1))
    return t


# ---- firewall rules on SYN frames (include/mosrx.h: mosrx_acl_rule) ----
OP_ACL = 14            # MOSRX_OP_ACL: the firewall launch (arg = rec_bytes; aux = the u16 hit arrays)
ACL_MAX_RULES = 1024   # MOSRX_ACL_MAX_RULES (the sample's MAX_RULES)
ACL_ACCEPT, ACL_DROP = 1, 2                       # MOSRX_ACL_*: FRA_ACCEPT, FRA_DROP
ACL_NOT_LOOKED_UP, ACL_NO_MATCH = 0xFFFF, 0xFFFE  # d_hit values that are no rule index
FWD_DROP = 6           # MOSRX_FWD_DROP: the plan kind of a SYN a DROP rule matched
ACL_RULE_DTYPE = np.dtype([("src_ip", "<u4"), ("src_mask", "<u4"), ("dst_ip", "<u4"), ("dst_mask", "<u4"),
                           ("sport", "<u2"), ("dport", "<u2"), ("action", "u1"), ("pad", "u1", 3)])
assert ACL_RULE_DTYPE.itemsize == 24


class AclRule(C.Structure):
    """mosrx_acl_rule: one rule as struct FirewallRule holds it after ParseConfigFile."""
    _fields_ = [("src_ip", C.c_uint32), ("src_mask", C.c_uint32), ("dst_ip", C.c_uint32), ("dst_mask", C.c_uint32),
                ("sport", C.c_uint16), ("dport", C.c_uint16), ("action", C.c_uint8), ("pad", C.c_uint8 * 3)]


def acl_mask(bits: int) -> int:
    """What IP_NETMASK (simple_firewall.c:39) ands the stored, network-order address
    with: 0xFFFFFFFF >> (32 - bits).  For bits that are no multiple of 8 this keeps
    the LOW bits of the last partial octet -- the sample's behaviour, reproduced.
    /0 is a shift by 32 there (undefined) and is refused: 0.0.0.0 is the wildcard."""
    if not 1 <= bits <= 32:
        raise ValueError(f"/{bits}: a prefix of 1..32 (0.0.0.0 is the wildcard; /0 is undefined in the sample)")
    return 0xFFFFFFFF >> (32 - bits)


def _acl_addr(cidr: str) -> tuple[int, int]:
    a, _, p = cidr.partition("/")
    m = acl_mask(int(p) if p else 32)
    return ip_raw(a) & m, m                # ExtractIPAddress (:204) stores the masked address


def acl_rules(rules) -> np.ndarray:
    """The rules of a simple_firewall rule file as ACL_RULE_DTYPE records:
    [("DROP" | "ACCEPT", "10.1.0.0/16", "10.2.0.1", sport, dport), ...], ports in
    host order, 0 (or omitted) the wildcard, as is the address 0.0.0.0."""
    if len(rules) > ACL_MAX_RULES:
        raise ValueError(f"{len(rules)} rules: at most {ACL_MAX_RULES}")
    out = np.zeros(len(rules), ACL_RULE_DTYPE)
    for i, r in enumerate(rules):
        act, src, dst = r[0], r[1], r[2]
        sport, dport = (tuple(r[3:]) + (0, 0))[:2]
        if act not in ("ACCEPT", "DROP"):
            raise ValueError(f"rule {i}: action {act!r}")
        if not (0 <= int(sport) <= 0xFFFF and 0 <= int(dport) <= 0xFFFF):
            raise ValueError(f"rule {i}: port out of range")
        out[i]["src_ip"], out[i]["src_mask"] = _acl_addr(src)
        out[i]["dst_ip"], out[i]["dst_mask"] = _acl_addr(dst)
        out[i]["sport"] = int.from_bytes(int(sport).to_bytes(2, "big"), "little")   # htons
        out[i]["dport"] = int.from_bytes(int(dport).to_bytes(2, "big"), "little")
        out[i]["action"] = ACL_ACCEPT if act == "ACCEPT" else ACL_DROP
    return out


# ---- NAT: established flows translated ahead of forwarding (include/mosrx.h) ----
OP_FWD_NAT = 15              # MOSRX_OP_FWD_NAT: plan-nat, ring build, patch (arg / aux as OP_FWD_RINGS)
NAT_MAX_BINDINGS = 64510     # MOSRX_NAT_MAX_BINDINGS (the sample's port pool)
NAT_NONE, NAT_SNAT, NAT_DNAT, NAT_MISS, NAT_HOST = range(5)   # MOSRX_NAT_*
NAT_NO_BIND = 0xFFFFFFFF
FWD_NAT_MISS, FWD_NAT_HOST = 7, 8                              # MOSRX_FWD_NAT_*: plan kinds handed to the host
NAT_BINDING_DTYPE = np.dtype([("cli_ip", "<u4"), ("svr_ip", "<u4"), ("nat_ip", "<u4"), ("cli_port", "<u2"),
                              ("svr_port", "<u2"), ("nat_port", "<u2"), ("pad", "<u2")])
NAT_XLAT_DTYPE = np.dtype([("addr", "<u4"), ("port", "<u2"), ("ip_check", "<u2"), ("tcp_check", "<u2"), ("kind", "u1"),
                           ("ihl", "u1"), ("bind", "<u4")])
NAT_SLOT_DTYPE = np.dtype([("saddr", "<u4"), ("daddr", "<u4"), ("ports", "<u4"), ("port", "<u2"), ("kind", "u1"),
                           ("pad", "u1"), ("addr", "<u4"), ("bind", "<u4"), ("reserved", "<u4", 2)])
assert NAT_BINDING_DTYPE.itemsize == 20 and NAT_XLAT_DTYPE.itemsize == 16 and NAT_SLOT_DTYPE.itemsize == 32


def _htons(x: int) -> int:
    return int.from_bytes(int(x).to_bytes(2, "big"), "little")


def nat_bindings(flows, nat_ip: str) -> np.ndarray:
    """Established flows as NAT_BINDING_DTYPE records: [(cli_ip, cli_port, svr_ip,
    svr_port, nat_port), ...] with dotted quads and host-order ports; nat_ip the
    NAT's own address (the sample's g_NATIP).  Stored network order, as the frame
    holds them."""
    if len(flows) > NAT_MAX_BINDINGS:
        raise ValueError(f"{len(flows)} bindings: at most {NAT_MAX_BINDINGS}")
    out = np.zeros(len(flows), NAT_BINDING_DTYPE)
    for i, (cip, cport, sip, sport, nport) in enumerate(flows):
        if not all(0 <= int(x) <= 0xFFFF for x in (cport, sport, nport)):
            raise ValueError(f"binding {i}: port out of range")
        out[i] = (ip_raw(cip), ip_raw(sip), ip_raw(nat_ip), _htons(cport), _htons(sport), _htons(nport), 0)
    return out


def nat_table(bindings: np.ndarray):
    """mosrx_nat_build: (slots as NAT_SLOT_DTYPE, the longest probe run) -- the lookup
    table mosrx_nat_set uploads, built on the host.  Raises MosrxError as mosrx_nat_check."""
    b = np.ascontiguousarray(bindings, NAT_BINDING_DTYPE)
    slots = np.zeros(lib().mosrx_nat_slots(len(b)), NAT_SLOT_DTYPE)
    probe = C.c_uint32()
    _chk(lib().mosrx_nat_build(b.ctypes.data if len(b) else None, len(b), slots.ctypes.data, C.byref(probe)),
         "mosrx_nat_build")
    return slots, int(probe.value)


NAT_TOMB = 0xFF                     # MOSRX_NAT_TOMB: a slot whose key was deleted (a slot's kind only)
NAT_OP_ADD, NAT_OP_DEL = 1, 2       # MOSRX_NAT_OP_*
NAT_UPDATE_MAX_OPS = 2 * NAT_MAX_BINDINGS   # MOSRX_NAT_UPDATE_MAX_OPS: more ops in one nat_update are refused
NAT_OP_DTYPE = np.dtype([("b", NAT_BINDING_DTYPE), ("op", "<u4"), ("bind", "<u4")])
NAT_TOUCH_DTYPE = np.dtype([("slot", "<u4"), ("pad", "<u4", 3), ("image", NAT_SLOT_DTYPE)])
NAT_STATS_DTYPE = np.dtype([("live", "<u4"), ("tombs", "<u4"), ("slots", "<u4"), ("probe", "<u4"), ("updates", "<u8"),
                            ("rebuilds", "<u8")])
assert NAT_OP_DTYPE.itemsize == 28 and NAT_TOUCH_DTYPE.itemsize == 48 and NAT_STATS_DTYPE.itemsize == 32
NatState = collections.namedtuple("NatState", "slots keys tombs probe")    # mosrx_nat_tstate
NatStats = collections.namedtuple("NatStats", "live tombs slots probe updates rebuilds")


def nat_ops(adds=(), dels=(), nat_ip: str = None) -> np.ndarray:
    """NAT_OP_DTYPE records for mosrx_nat_update / mosrx_nat_apply: the deletes first,
    in their order, then the adds in theirs (so a flow may be deleted and bound again
    in one call).  adds: [(flow, bind), ...], dels: [flow, ...]; a flow is nat_bindings'
    tuple (cli_ip, cli_port, svr_ip, svr_port, nat_port) or one NAT_BINDING_DTYPE
    record (nat_ip then not needed)."""
    def rec(f):
        if isinstance(f, (np.void, np.ndarray)):
            return np.asarray(f, NAT_BINDING_DTYPE).reshape(())
        return nat_bindings([f], nat_ip)[0]
    out = np.zeros(len(dels) + len(adds), NAT_OP_DTYPE)
    for i, f in enumerate(dels):
        out[i]["b"], out[i]["op"] = rec(f), NAT_OP_DEL
    for i, (f, bind) in enumerate(adds, len(dels)):
        out[i]["b"], out[i]["op"], out[i]["bind"] = rec(f), NAT_OP_ADD, bind
    return out


def nat_state(slots: np.ndarray, probe: int) -> NatState:
    """The NatState of a table as nat_table returns it (or as nat_apply left it)."""
    k = slots["kind"]
    return NatState(len(slots), int(((k == NAT_SNAT) | (k == NAT_DNAT)).sum()), int((k == NAT_TOMB).sum()), int(probe))


def nat_apply(slots: np.ndarray, state, ops):
    """mosrx_nat_apply: the ops applied in their order to the host table `slots` (a
    contiguous NAT_SLOT_DTYPE array, changed in place) whose NatState is `state`;
    returns (touch, the new NatState) -- touch the final image of every slot that
    changed, NAT_TOUCH_DTYPE, slots ascending.  Raises MosrxError on a refusal, the
    table then as it was."""
    if slots.dtype != NAT_SLOT_DTYPE or not slots.flags.c_contiguous or not slots.flags.writeable:
        raise ValueError("slots: a writable contiguous NAT_SLOT_DTYPE array")
    o = np.ascontiguousarray(ops, NAT_OP_DTYPE)
    st = np.array(tuple(state), np.uint32)
    touch = np.zeros(4 * len(o), NAT_TOUCH_DTYPE)
    m = C.c_uint32()
    _chk(lib().mosrx_nat_apply(slots.ctypes.data, st.ctypes.data, o.ctypes.data if len(o) else None, len(o),
                               touch.ctypes.data if len(o) else None, C.byref(m)), "mosrx_nat_apply")
    return touch[:m.value].copy(), NatState(*(int(v) for v in st))


def nat_patch_frame(frame, xlat) -> np.ndarray:
    """mosrx_nat_patch_frame: a copy of one host frame (from its Ethernet header) with
    one NAT_XLAT_DTYPE record applied."""
    f = np.array(np.frombuffer(bytes(frame), np.uint8), copy=True)
    x = np.ascontiguousarray(np.asarray(xlat, NAT_XLAT_DTYPE).reshape(1))
    lib().mosrx_nat_patch_frame(f.ctypes.data, x.ctypes.data)
    return f


class BpfProg(C.Structure):
    _fields_ = [("insns", C.c_void_p), ("len", C.c_uint32), ("len_mode", C.c_int32)]


class TraceC(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("frames_bytes", C.c_uint64), ("off", C.c_void_p),
                ("len", C.c_void_p), ("n", C.c_uint32), ("max_len", C.c_uint32),
                ("caplen_sum", C.c_uint64)]


class RxStats(C.Structure):
    _fields_ = [("rx_packets", C.c_uint64), ("rx_bytes", C.c_uint64), ("rx_errors", C.c_uint64),
                ("rounds", C.c_uint64), ("batches", C.c_uint64), ("by_reason", C.c_uint64 * NREASON),
                ("recv_errors", C.c_uint64)]


class ModuleCfg(C.Structure):
    _fields_ = [("num_ifs", C.c_uint32), ("if_names", (C.c_char * 16) * 16),
                ("src", C.c_void_p * 16), ("batch", C.c_uint32), ("max_frame", C.c_uint32),
                ("gpu_base", C.c_int32), ("ngpu", C.c_int32), ("pipeline", C.c_int32),
                ("params", Params), ("bpf_progs", C.c_void_p), ("bpf_nprog", C.c_uint32),
                ("tx_batch", C.c_uint32), ("tcpinfo", C.c_int32), ("group", C.c_uint32),
                ("group_bytes", C.c_uint64), ("flowhash", C.c_int32), ("tx_csum", C.c_int32),
                ("numa", C.c_int32), ("compact", C.c_int32), ("group_max_us", C.c_uint32),
                ("direct_kb", C.c_uint32), ("direct_frames", C.c_uint32), ("steer", C.c_int32)]


class SteerView(C.Structure):
    """mosrx_steer_view (dev_ioctl(MOSRX_PKT_RX_STEER))."""
    _fields_ = [("idx", C.c_void_p), ("qstart", C.c_void_p), ("n", C.c_uint32), ("num_queues", C.c_uint32)]


class QueueView(C.Structure):
    """mosrx_queue_view (dev_ioctl(MOSRX_PKT_RX_QUEUE))."""
    _fields_ = [("q", C.c_uint32), ("n", C.c_uint32), ("rec", C.c_void_p), ("rec_bytes", C.c_uint32),
                ("off", C.c_void_p), ("len", C.c_void_p), ("idx", C.c_void_p), ("frames", C.c_void_p)]


class QueueSide(C.Structure):
    """mosrx_queue_side (dev_ioctl(MOSRX_PKT_RX_QUEUE_SIDE))."""
    _fields_ = [("q", C.c_uint32), ("n", C.c_uint32), ("fhash", C.c_void_p), ("match", C.c_void_p),
                ("tcpinfo", C.c_void_p)]


class HubStats(C.Structure):
    """mosrx_hub_stats."""
    _fields_ = [("batches", C.c_uint64), ("frames", C.c_uint64), ("delivered", C.c_uint64),
                ("unowned", C.c_uint64), ("owner_waits", C.c_uint64)]


class ModuleStats(C.Structure):
    _fields_ = [("rx_batches", C.c_uint64), ("rx_frames", C.c_uint64), ("tx_packets", C.c_uint64),
                ("tx_bytes", C.c_uint64), ("tx_errors", C.c_uint64), ("kernel_launches", C.c_uint64),
                ("kernel_ms", C.c_double), ("rx_drops", C.c_uint64),
                ("rx_reclassified", C.c_uint64), ("cpu", C.c_int32), ("device", C.c_int32),
                ("tx_csum_offloaded", C.c_uint64), ("cpu_node", C.c_int32), ("gpu_node", C.c_int32),
                ("rx_groups", C.c_uint64), ("max_group_frames", C.c_uint64), ("group_cap_frames", C.c_uint64),
                ("ns_per_frame_host", C.c_double), ("ns_per_byte_dev", C.c_double),
                ("rx_direct_groups", C.c_uint64)]


LAT_BINS = 1024


class LatencyProbe(C.Structure):
    """mosrx_latency_probe (include/mosrx_io_module.h): residency histograms of
    frames from a paced source, filled by the rx loop (RxLoopOpts.probe)."""
    _fields_ = [("src", C.c_void_p), ("t0_ns", C.c_uint64), ("ns_per_frame", C.c_double),
                ("skip", C.c_uint64), ("seen", C.c_uint64), ("recorded", C.c_uint64), ("batches", C.c_uint64),
                ("avail_max_ns", C.c_uint64), ("done_max_ns", C.c_uint64),
                ("avail_hist", C.c_uint64 * LAT_BINS), ("done_hist", C.c_uint64 * LAT_BINS)]

    @staticmethod
    def bin_ns(b: int) -> float:
        """The middle of histogram bin b, ns (16 bins per octave above 16 ns)."""
        if b < 16:
            return float(b)
        e, m = b // 16, b % 16
        return ((16 + m) + 0.5) * 2.0 ** (e - 4)

    def percentiles(self, which: str = "avail", ps=(50, 99, 99.9)) -> dict:
        h = np.array(getattr(self, which + "_hist")[:], dtype=np.float64)
        tot = h.sum()
        if tot == 0:
            return {}
        cum = np.cumsum(h) / tot
        return {f"p{p:g}_us": round(self.bin_ns(int(np.searchsorted(cum, p / 100.0))) / 1e3, 2) for p in ps}


class RxLoopOpts(C.Structure):
    _fields_ = [("max_pkts", C.c_uint64), ("idle_rounds", C.c_uint32), ("idle_us", C.c_uint32),
                ("max_us", C.c_uint64), ("probe", C.c_void_p)]


class AfpOpts(C.Structure):
    _fields_ = [("ring_blocks", C.c_uint32), ("retire_ms", C.c_uint32), ("fanout_group", C.c_uint32),
                ("copy", C.c_int32)]


class AfpInfo(C.Structure):
    _fields_ = [("zero_copy", C.c_int32), ("ring_bytes", C.c_uint64), ("dropped_outgoing", C.c_uint64),
                ("ring_packets", C.c_uint64), ("ring_drops", C.c_uint64)]


class Forwarder(C.Structure):
    _fields_ = [("iom", C.c_void_p), ("ctx", C.c_void_p), ("out_if", C.c_int32 * 16),
                ("forwarded", C.c_uint64), ("dropped", C.c_uint64),
                ("forward", C.c_int32), ("num_msp", C.c_uint32), ("listener", C.c_uint32)]


class MosrxError(OSError):
    pass


_lib = None


def build():
    """Compile libmosrx.so in-tree (hipcc --offload-arch=gfx950 + gcc)."""
    subprocess.check_call(["make", "-s", "-C", PKG_DIR])


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MosrxError(2, f"{LIB_PATH} missing: run build() / `make -C {PKG_DIR}`")
        L = C.CDLL(LIB_PATH)
        P, U32, U64, I = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        sig = {
            "mosrx_abi_version": (I, []),
            "mosrx_strerror": (C.c_char_p, [I]),
            "mosrx_params_default": (None, [C.POINTER(Params)]),
            "mosrx_params_set_ms_key": (None, [C.POINTER(Params)]),
            "mosrx_open": (I, [I, C.POINTER(Params), C.POINTER(P)]),
            "mosrx_set_params": (I, [P, C.POINTER(Params)]),
            "mosrx_set_variant": (I, [P, I]),
            "mosrx_close": (None, [P]),
            "mosrx_classify_dev": (I, [P, C.POINTER(Batch), P, P]),
            "mosrx_classify_host": (I, [P, C.POINTER(Batch), P]),
            "mosrx_classify_dev_fh": (I, [P, C.POINTER(Batch), P, P, P]),
            "mosrx_classify_host_fh": (I, [P, C.POINTER(Batch), P, P]),
            "mosrx_classify_dev_ex": (I, [P, C.POINTER(Batch), P, P, P, P]),
            "mosrx_classify_host_ex": (I, [P, C.POINTER(Batch), P, P, P]),
            "mosrx_classify_host_submit": (I, [P, I, C.POINTER(Batch), P]),
            "mosrx_classify_host_wait": (I, [P, I]),
            "mosrx_last_counters": (I, [P, C.POINTER(U64)]),
            "mosrx_sync": (I, [P]),
            "mosrx_dev_alloc": (I, [P, C.c_size_t, C.POINTER(P)]),
            "mosrx_dev_free": (I, [P, P]),
            "mosrx_host_alloc": (I, [P, C.c_size_t, C.POINTER(P)]),
            "mosrx_host_free": (I, [P, P]),
            "mosrx_memcpy_h2d": (I, [P, P, P, C.c_size_t]),
            "mosrx_memcpy_d2h": (I, [P, P, P, C.c_size_t]),
            "mosrx_memcpy_h2d_pull": (I, [P, P, P, C.c_size_t]),
            "mosrx_stream": (P, [P]),
            "mosrx_time_dev": (I, [P, C.POINTER(Batch), U32, C.POINTER(P), U32, C.POINTER(C.c_float)]),
            "mosrx_time_dev_kernels": (I, [P, C.POINTER(Batch), U32, C.POINTER(P), U32, C.POINTER(C.c_float)]),
            "mosrx_device_sync": (I, [P]),
            "mosrx_time_op": (I, [P, I, I, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P), U32, U32,
                                  C.POINTER(C.c_float), C.POINTER(C.c_float)]),
            "mosrx_time_dev_streams": (I, [P, C.POINTER(Batch), U32, C.POINTER(P), U32, U32, C.POINTER(C.c_float)]),
            "mosrx_time_op_dispatch": (I, [P, I, I, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P), U32,
                                           C.POINTER(C.c_float)]),
            "mosrx_time_queue_dispatch": (I, [P, C.POINTER(P), U32, U32, C.POINTER(C.c_float)]),
            "mosrx_probe_read_bw": (I, [P, U64, U32, U32, C.POINTER(C.c_float)]),
            "mosrx_probe_stamp_floor": (I, [P, C.POINTER(Batch), U32, C.POINTER(C.c_float)]),
            "mosrx_queue_create": (I, [P, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P)]),
            "mosrx_queue_run": (I, [P, P, P]),
            "mosrx_queue_destroy": (None, [P, P]),
            "mosrx_time_queue": (I, [P, C.POINTER(P), U32, U32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
            "mosrx_time_host": (I, [P, C.POINTER(Batch), U32, C.POINTER(P), U32, C.POINTER(C.c_float)]),
            "mosrx_rss_tables": (I, [C.c_char_p, U32, C.POINTER(U32)]),
            "mosrx_tx_csum_dev": (I, [P, C.POINTER(Batch), I, P]),
            "mosrx_tx_csum_host": (I, [P, C.POINTER(Batch), I]),
            "mosrx_tx_csum_dev_checks": (I, [P, C.POINTER(Batch), I, P, P]),
            "mosrx_bpf_check": (I, [P, U32]),
            "mosrx_bpf_set": (I, [P, C.POINTER(BpfProg), U32]),
            "mosrx_bpf_dev": (I, [P, C.POINTER(Batch), P, P]),
            "mosrx_bpf_host": (I, [P, C.POINTER(Batch), P]),
            "mosrx_bpf_set_engine": (I, [P, I]),
            "mosrx_bpf_engine": (I, [P]),
            "mosrx_bpf_jit_log": (C.c_char_p, [P]),
            "mosrx_bpf_jit_source": (I, [C.POINTER(BpfProg), U32, C.POINTER(P)]),
            "mosrx_bpf_jit_hook_source": (I, [C.POINTER(BpfProg), U32, C.POINTER(P)]),
            "mosrx_bpf_jit_compile": (I, [C.POINTER(BpfProg), U32, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
            "mosrx_bpf_jit_compile_fused": (I, [C.POINTER(BpfProg), U32, C.c_char_p, C.c_size_t,
                                                C.POINTER(C.c_size_t)]),
            "mosrx_classify_bpf_dev": (I, [P, C.POINTER(Batch), P, P, P]),
            "mosrx_bpf_fused": (I, [P]),
            "mosrx_classify_bpf_host": (I, [P, C.POINTER(Batch), P, P]),
            "mosrx_classify_bpf_host_submit": (I, [P, I, C.POINTER(Batch), P, P]),
            "mosrx_trace_gen": (I, [I, U32, U32, U64, C.POINTER(TraceC)]),
            "mosrx_trace_free": (None, [C.POINTER(TraceC)]),
            "mosrx_source_mem": (P, [P, P, P, U32, U32]),
            "mosrx_source_pcap": (P, [C.c_char_p, U32]),
            "mosrx_source_afpacket": (P, [C.c_char_p]),
            "mosrx_source_close": (None, [P]),
            "mosrx_source_next": (I, [P, P, U32]),
            "mosrx_source_fill": (I, [P, P, U64, P, P, U32, U32, C.POINTER(U64)]),
            "mosrx_source_borrow": (I, [P, U32, U32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), P, P]),
            "mosrx_source_give_back": (I, [P]),
            "mosrx_source_mem_set_mode": (I, [P, I]),
            "mosrx_gpu_module_cfg_default": (None, [C.POINTER(ModuleCfg)]),
            "mosrx_gpu_module_configure": (I, [C.POINTER(ModuleCfg)]),
            "mosrx_gpu_module_bind": (I, [P, I]),
            "mosrx_rx_loop": (I, [P, P, I, U64, P, P, C.POINTER(RxStats)]),
            "mosrx_rx_loop_ex": (I, [P, P, I, C.POINTER(RxLoopOpts), P, P, C.POINTER(RxStats)]),
            "mosrx_source_paced": (P, [P, C.c_double]),
            "mosrx_source_paced_info": (I, [P, C.POINTER(U64), C.POINTER(C.c_double), C.POINTER(U64)]),
            "mosrx_classify_host_ready": (I, [P, I]),
            "mosrx_classify_host_reserve": (I, [P, U64, U32]),
            "mosrx_set_counters": (I, [P, I]),
            "mosrx_set_direct": (I, [P, U64, U32]),
            "mosrx_slot_direct": (I, [P, I]),
            "mosrx_mos_forwards": (I, [P, I, U32, U32]),
            "mosrx_device_count": (I, []),
            "mosrx_classify_host_submit_ex": (I, [P, I, C.POINTER(Batch), P, P]),
            "mosrx_classify_host_group_submit": (I, [P, I, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P)]),
            "mosrx_classify_host_group_submit_ex": (I, [P, I, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P),
                                                        C.POINTER(P)]),
            "mosrx_set_timing": (I, [P, I]),
            "mosrx_last_kernel_ms": (I, [P, C.POINTER(C.c_float)]),
            "mosrx_source_afpacket_ex": (P, [C.c_char_p, C.POINTER(AfpOpts)]),
            "mosrx_source_afpacket_info": (I, [P, C.POINTER(AfpInfo)]),
            "mosrx_source_tpacket_v3": (P, [P, U32, U32]),
            "mosrx_source_send": (I, [P, P, U32]),
            "mosrx_source_tx_pcap": (I, [P, C.c_char_p]),
            "mosrx_source_tx_flush": (I, [P]),
            "mosrx_source_tx_stats": (I, [P, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
            "mosrx_gpu_module_bind_source": (I, [I, I, P]),
            "mosrx_gpu_module_device_of": (I, [I, I]),
            "mosrx_gpu_module_stats_of": (I, [P, C.POINTER(ModuleStats)]),
            "mosrx_gpu_module_set_timing": (I, [P, I]),
            "mosrx_bpf_set_async": (I, [P, C.POINTER(BpfProg), U32]),
            "mosrx_bpf_wait": (I, [P]),
            "mosrx_bpf_pending": (I, [P]),
            "mosrx_classify_dev_compact": (I, [P, C.POINTER(Batch), P, P]),
            "mosrx_queue_create_ex": (I, [P, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P), C.POINTER(P), I,
                                          C.POINTER(P)]),
            "mosrx_classify_host_group_submit_bpf": (I, [P, I, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P),
                                                         C.POINTER(P)]),
            "mosrx_classify_host_group_submit_c8": (I, [P, I, C.POINTER(Batch), U32, C.POINTER(P), C.POINTER(P)]),
            "mosrx_classify_host_group_submit_bpf_c8": (I, [P, I, C.POINTER(Batch), U32, C.POINTER(P),
                                                            C.POINTER(P), C.POINTER(P)]),
            "mosrx_host_register": (I, [P, P, C.c_size_t, I]),
            "mosrx_host_unregister": (I, [P, P]),
            "mosrx_pci_numa_node": (I, [C.c_char_p]),
            "mosrx_cpu_numa_node": (I, [I]),
            "mosrx_gpu_numa_node": (I, [I]),
            "mosrx_numa_pick": (I, [I, C.POINTER(C.c_int), I]),
            "mosrx_topology_set_root": (I, [C.c_char_p]),
            "mosrx_steer_scratch_bytes": (C.c_size_t, [U32]),
            "mosrx_steer_tile": (U32, []),
            "mosrx_steer_dev": (I, [P, P, U32, I, P, P, P, C.c_size_t, P]),
            "mosrx_queue_set_steer": (I, [P, P, C.POINTER(P), C.POINTER(P)]),
            "mosrx_slot_steer": (I, [P, I, C.POINTER(P), C.POINTER(P)]),
            "mosrx_steer_gather_dev": (I, [P, P, P, P, U32, I, P, P, P, P, P, P, C.c_size_t, P]),
            "mosrx_queue_set_steer_gather": (I, [P, P, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P),
                                                 C.POINTER(P)]),
            "mosrx_slot_steer_gather": (I, [P, I, C.POINTER(P), C.POINTER(P), C.POINTER(P), C.POINTER(P),
                                            C.POINTER(P)]),
            "mosrx_steer_gather_side_dev": (I, [P, P, P, P, U32, I, P, P, P, P, P, P, P, P, P, P, P, P, C.c_size_t,
                                                P]),
            "mosrx_queue_set_steer_gather_side": (I, [P, P] + [C.POINTER(P)] * 7),
            "mosrx_slot_steer_gather_side": (I, [P, I] + [C.POINTER(P)] * 8),
            "mosrx_set_steer_one": (I, [P, U32]),
            "mosrx_get_steer_one": (U32, [P]),
            "mosrx_steer_one_count": (U64, [P]),
            "mosrx_gpu_module_steer_one_count": (U64, [P]),
            "mosrx_gpu_module_set_steer_one": (I, [C.c_int32]),
            "mosrx_gpu_module_get_steer_one": (C.c_int32, []),
            "mosrx_set_fwd_one": (I, [P, U32]),
            "mosrx_get_fwd_one": (U32, [P]),
            "mosrx_fwd_one_count": (U64, [P]),
            "mosrx_gpu_module_fwd_one_count": (U64, [P]),
            "mosrx_gpu_module_set_fwd_one": (I, [C.c_int32]),
            "mosrx_gpu_module_get_fwd_one": (C.c_int32, []),
            "mosrx_fwd_set": (I, [P, C.POINTER(FwdTables)]),
            "mosrx_fwd_set_listener": (I, [P, I]),
            "mosrx_fwd_plan_dev": (I, [P, C.POINTER(Batch), P, I, I, P, P]),
            "mosrx_fwd_build_dev": (I, [P, C.POINTER(Batch), P, P, U64, P, P, P, P, P, P, C.c_size_t, P]),
            "mosrx_fwd_scratch_bytes": (C.c_size_t, [U32]),
            "mosrx_fwd_build_rings_dev": (I, [P, C.POINTER(Batch), P, P, U64, U32, P, P, P, P, P, C.c_size_t, P]),
            "mosrx_fwd_rings_scratch_bytes": (C.c_size_t, [U32, U32]),
            "mosrx_fwd_tile": (U32, []),
            "mosrx_queue_set_fwd": (I, [P, P, C.POINTER(QueueFwd)]),
            "mosrx_fwd_desc_rings_dev": (I, [P, C.POINTER(Batch), P, U32, P, P, P, P, P, C.c_size_t, P]),
            "mosrx_fwd_desc_scratch_bytes": (C.c_size_t, [U32, U32]),
            "mosrx_queue_set_fwd_desc": (I, [P, P, C.POINTER(QueueFwdDesc)]),
            "mosrx_slot_fwd": (I, [P, I, C.POINTER(SlotFwdOut)]),
            "mosrx_gpu_module_set_fwd": (I, [C.POINTER(FwdTables), I]),
            "mosrx_backend_forward": (I, [P, P, I, P]),
            "mosrx_acl_check": (I, [P, U32]),
            "mosrx_acl_set": (I, [P, P, U32]),
            "mosrx_acl_count": (U32, [P]),
            "mosrx_acl_apply_dev": (I, [P, C.POINTER(Batch), P, I, P, P, P, P]),
            "mosrx_queue_set_acl": (I, [P, P, C.POINTER(P), P]),
            "mosrx_slot_acl": (I, [P, I, C.POINTER(P), P]),
            "mosrx_gpu_module_set_acl": (I, [P, U32]),
            "mosrx_nat_hash": (U32, [U32, U32, U32]),
            "mosrx_nat_slots": (U32, [U32]),
            "mosrx_nat_build": (I, [P, U32, P, C.POINTER(U32)]),
            "mosrx_nat_check": (I, [P, U32]),
            "mosrx_nat_set": (I, [P, P, U32]),
            "mosrx_nat_count": (U32, [P]),
            "mosrx_nat_apply": (I, [P, P, P, U32, P, C.POINTER(U32)]),
            "mosrx_nat_update": (I, [P, P, U32, P]),
            "mosrx_nat_get_stats": (I, [P, P]),
            "mosrx_launch_nat_update": (I, [P, U32, P, U32, P]),
            "mosrx_fwd_plan_nat_dev": (I, [P, C.POINTER(Batch), P, I, I, P, P, P]),
            "mosrx_nat_patch_rings_dev": (I, [P, P, P, P, P, P, U32, U32, P]),
            "mosrx_nat_patch_frame": (None, [P, P]),
            "mosrx_queue_set_nat": (I, [P, P, C.POINTER(P)]),
            "mosrx_hub_open": (I, [P, P, I, U32, C.POINTER(P)]),
            "mosrx_hub_endpoint": (P, [P, U32]),
            "mosrx_hub_stats_get": (I, [P, P]),
            "mosrx_hub_close": (I, [P]),
            "mosrx_rx_loop_queues": (I, [P, P, I, U32, P, C.POINTER(P), U64, C.POINTER(RxStats)]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
        _sigs.update(sig)
    return _lib


_sigs = {}


def module_lib(path: str):
    """Another build of gpu_module_func (e.g. the CPU test suite's build of the
    module over a stand-in for the GPU): a CDLL whose mosrx_gpu_module_*
    functions carry libmosrx's signatures, for GpuBackend(module_lib=...)."""
    lib()
    L = C.CDLL(path)
    for name, (res, args) in _sigs.items():
        if name.startswith("mosrx_gpu_module_"):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
    return L


def _chk(rc: int, what: str):
    if rc:
        raise MosrxError(-rc, f"{what}: {lib().mosrx_strerror(rc).decode()}")


def default_params(**kw) -> Params:
    """simple_firewall's state (mosrx_params_default) with fields overridden; `key`
    = RSS key bytes, `local` = the netdevs' IPv4 addresses (dotted quads)."""
    p = Params()
    lib().mosrx_params_default(C.byref(p))
    key = kw.pop("key", None)
    local = kw.pop("local", None)
    if local is not None:
        if len(local) > MAX_LOCAL:
            raise ValueError("at most 16 local addresses")
        p.num_local = len(local)
        for i, a in enumerate(local):
            p.local_ip[i] = ip_raw(a) if isinstance(a, str) else int(a)
    for k, v in kw.items():
        setattr(p, k, v)
    if key is not None:
        if not 16 <= len(key) <= 52:
            raise ValueError("rss key must be 16..52 bytes")
        for i in range(52):
            p.rss_key[i] = key[i] if i < len(key) else 0
        p.rss_key_len = len(key)
    return p


BPF_ENGINE_INTERP, BPF_ENGINE_JIT = 0, 1


def _bpf_progs(progs):
    keep = [np.ascontiguousarray(i if i is not None else [], BPF_INSN) for i, _ in progs]
    arr = (BpfProg * max(1, len(progs)))()
    for j, ((_, mode), ins) in enumerate(zip(progs, keep)):
        arr[j].insns = ins.ctypes.data if len(ins) else None
        arr[j].len = len(ins)
        arr[j].len_mode = mode
    return arr, keep


def bpf_jit_source(progs) -> str:
    """mosrx_bpf_jit_source: the gfx950 kernel source generated for a program set."""
    arr, _keep = _bpf_progs(progs)
    out = C.c_void_p()
    _chk(lib().mosrx_bpf_jit_source(arr, len(progs), C.byref(out)), "mosrx_bpf_jit_source")
    try:
        return C.string_at(out.value).decode()
    finally:
        C.CDLL(None).free(out)


def bpf_jit_hook_source(progs) -> str:
    """mosrx_bpf_jit_hook_source: the fused kernel's generated hook for a program set."""
    arr, _keep = _bpf_progs(progs)
    out = C.c_void_p()
    _chk(lib().mosrx_bpf_jit_hook_source(arr, len(progs), C.byref(out)), "mosrx_bpf_jit_hook_source")
    try:
        return C.string_at(out.value).decode()
    finally:
        C.CDLL(None).free(out)


def bpf_jit_compile(progs):
    """mosrx_bpf_jit_compile: (rc, code-object bytes, hipRTC log); no GPU needed."""
    arr, _keep = _bpf_progs(progs)
    log = C.create_string_buffer(4096)
    sz = C.c_size_t(0)
    rc = lib().mosrx_bpf_jit_compile(arr, len(progs), log, len(log), C.byref(sz))
    return rc, int(sz.value), log.value.decode(errors="replace")


def bpf_jit_compile_fused(progs):
    """mosrx_bpf_jit_compile_fused: (rc, code-object bytes, hipRTC log) of the fused
    classify + BPF kernel; no GPU needed."""
    arr, _keep = _bpf_progs(progs)
    log = C.create_string_buffer(8192)
    sz = C.c_size_t(0)
    rc = lib().mosrx_bpf_jit_compile_fused(arr, len(progs), log, len(log), C.byref(sz))
    return rc, int(sz.value), log.value.decode(errors="replace")


def bpf_check(insns) -> int:
    """mosrx_bpf_check: 0 if mosrx_bpf_set would admit the program, else -errno."""
    ins = np.ascontiguousarray(insns, BPF_INSN)
    return lib().mosrx_bpf_check(ins.ctypes.data if len(ins) else None, len(ins))


class Trace:
    """A seeded synthetic batch (include/mosrx_trace.h) held as numpy arrays."""

    def __init__(self, kind: int, n: int, nflows: int = 1_000_000, seed: int = 0):
        t = TraceC()
        _chk(lib().mosrx_trace_gen(kind, n, nflows, seed, C.byref(t)), "mosrx_trace_gen")
        try:
            fb = int(t.frames_bytes)
            self.frames = np.ctypeslib.as_array(C.cast(t.frames, C.POINTER(C.c_uint8)), (fb + 64,)).copy()
            self.off = np.ctypeslib.as_array(C.cast(t.off, C.POINTER(C.c_uint32)), (t.n,)).copy() if t.n else np.zeros(0, np.uint32)
            self.len = np.ctypeslib.as_array(C.cast(t.len, C.POINTER(C.c_uint16)), (t.n,)).copy() if t.n else np.zeros(0, np.uint16)
            self.frames_bytes = fb
            self.n = int(t.n)
            self.max_len = int(t.max_len)
            self.caplen_sum = int(t.caplen_sum)
        finally:
            lib().mosrx_trace_free(C.byref(t))


class DevBuffer:
    """Device allocation owned by a Context (hipMalloc through the C ABI)."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, int(nbytes)
        p = C.c_void_p()
        _chk(lib().mosrx_dev_alloc(ctx.handle, max(self.nbytes, 1), C.byref(p)), "mosrx_dev_alloc")
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        _chk(lib().mosrx_memcpy_h2d(self.ctx.handle, self.ptr, a.ctypes.data, a.nbytes), "h2d")

    def download(self, arr: np.ndarray):
        assert arr.flags.c_contiguous and arr.nbytes <= self.nbytes
        _chk(lib().mosrx_memcpy_d2h(self.ctx.handle, arr.ctypes.data, self.ptr, arr.nbytes), "d2h")
        return arr

    def free(self):
        if self.ptr:
            lib().mosrx_dev_free(self.ctx.handle, self.ptr)
            self.ptr = None


class DevBatch:
    """A batch resident in HBM: frames + off + len, and its result buffer."""

    def __init__(self, ctx: "Context", frames: np.ndarray, off: np.ndarray, ln: np.ndarray,
                 frames_bytes: int | None = None, max_len: int | None = None, hint="auto"):
        frames = np.ascontiguousarray(frames, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        self.n = len(off)
        # the layout hint the batch is handed over with: "auto" = its own fixed
        # stride if it has one (the producer knows how it packed the frames),
        # None = none, or an explicit (off0, stride) -- tests give wrong ones
        self.hint = uniform_layout(off) if isinstance(hint, str) else hint
        self.frames_bytes = int(frames_bytes if frames_bytes is not None else len(frames))
        self.d_frames = DevBuffer(ctx, max(len(frames), 16))
        self.d_frames.upload(frames)
        self.d_off = DevBuffer(ctx, max(off.nbytes, 4))
        self.d_off.upload(off)
        self.d_len = DevBuffer(ctx, max(ln.nbytes, 2))
        self.d_len.upload(ln)
        self.d_out = DevBuffer(ctx, max(self.n * 16, 16))
        self.d_fhash = None   # allocated on the first classify_dev(..., flow_hash=True)
        self.d_tinfo = None   # allocated on the first classify_dev(..., tcpinfo=True)
        self.d_match = None   # allocated on the first bpf_dev
        self.d_out8 = None    # compact records, allocated on the first classify_dev_compact
        self.d_sidx = None    # steered frame indices, allocated on the first time_op(OP_STEER)
        self.d_fplan = None   # forwarding plan records, allocated on the first time_op(OP_FWD_PLAN / OP_FWD)
        self.max_len = int(max_len if max_len is not None else (int(ln.max()) if self.n else 0))
        self.caplen_sum = int(ln.astype(np.uint64).sum())

    def batch(self) -> Batch:
        return with_hint(Batch(self.d_frames.ptr, self.frames_bytes, self.d_off.ptr, self.d_len.ptr, self.n,
                               self.max_len), self.hint)

    def results(self) -> np.ndarray:
        out = np.zeros(self.n, RESULT_DTYPE)
        if self.n:
            self.d_out.download(out)
        return out

    def frames(self, nbytes: int | None = None) -> np.ndarray:
        """The frame buffer as it is now in HBM (e.g. after tx_csum_dev)."""
        out = np.zeros(self.frames_bytes if nbytes is None else nbytes, np.uint8)
        return self.d_frames.download(out)

    def matches(self) -> np.ndarray:
        out = np.zeros(self.n, np.uint32)
        if self.n:
            self.d_match.download(out)
        return out

    def results8(self) -> np.ndarray:
        out = np.zeros(self.n, RESULT8_DTYPE)
        if self.n:
            self.d_out8.download(out)
        return out

    def flow_hashes(self) -> np.ndarray:
        out = np.zeros(self.n, np.uint32)
        if self.n:
            self.d_fhash.download(out)
        return out

    def tcpinfo(self) -> np.ndarray:
        out = np.zeros(self.n, TCPINFO_DTYPE)
        if self.n:
            self.d_tinfo.download(out)
        return out

    def free(self):
        for b in (self.d_frames, self.d_off, self.d_len, self.d_out, self.d_fhash, self.d_match, self.d_tinfo,
                  self.d_out8, self.d_sidx, self.d_fplan):
            if b is not None:
                b.free()


class Context:
    """mosrx_ctx: one per host thread, bound to one GPU."""

    def __init__(self, device: int = 0, params: Params | None = None):
        self.params = params or default_params()
        h = C.c_void_p()
        _chk(lib().mosrx_open(device, C.byref(self.params), C.byref(h)), "mosrx_open")
        self.handle = h.value
        self.device = device

    def close(self):
        if self.handle:
            lib().mosrx_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_variant(self, variant: int):
        _chk(lib().mosrx_set_variant(self.handle, variant), "mosrx_set_variant")

    def set_params(self, params: Params):
        _chk(lib().mosrx_set_params(self.handle, C.byref(params)), "mosrx_set_params")
        self.params = params

    # ---- end-to-end from host memory ----
    def classify_host(self, frames, off, ln, frames_bytes=None, max_len=0) -> np.ndarray:
        frames = np.ascontiguousarray(frames, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        out = np.zeros(len(off), RESULT_DTYPE)
        b = Batch(frames.ctypes.data, int(frames_bytes if frames_bytes is not None else len(frames)),
                  off.ctypes.data, ln.ctypes.data, len(off), max_len)
        _chk(lib().mosrx_classify_host(self.handle, C.byref(b), out.ctypes.data), "mosrx_classify_host")
        return out

    def classify_host_ex(self, frames, off, ln, frames_bytes=None, max_len=0):
        """(records, flow hashes, pkt_info TCP fields) of a host batch in one GPU pass."""
        frames = np.ascontiguousarray(frames, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        out = np.zeros(len(off), RESULT_DTYPE)
        fh = np.zeros(len(off), np.uint32)
        ti = np.zeros(len(off), TCPINFO_DTYPE)
        b = Batch(frames.ctypes.data, int(frames_bytes if frames_bytes is not None else len(frames)),
                  off.ctypes.data, ln.ctypes.data, len(off), max_len)
        _chk(lib().mosrx_classify_host_ex(self.handle, C.byref(b), out.ctypes.data, fh.ctypes.data,
                                          ti.ctypes.data), "mosrx_classify_host_ex")
        return out, fh, ti

    def classify_host_fh(self, frames, off, ln, frames_bytes=None, max_len=0):
        """Records plus the per-frame flow hash (HashFlow before the NUM_BINS mask)."""
        frames = np.ascontiguousarray(frames, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        out = np.zeros(len(off), RESULT_DTYPE)
        fh = np.zeros(len(off), np.uint32)
        b = Batch(frames.ctypes.data, int(frames_bytes if frames_bytes is not None else len(frames)),
                  off.ctypes.data, ln.ctypes.data, len(off), max_len)
        _chk(lib().mosrx_classify_host_fh(self.handle, C.byref(b), out.ctypes.data, fh.ctypes.data),
             "mosrx_classify_host_fh")
        return out, fh

    # ---- TX checksum rewrite (mosrx_tx_csum_*) ----
    def tx_csum_host(self, frames, off, ln, flags=TX_IP_CSUM | TX_TCP_CSUM, frames_bytes=None) -> np.ndarray:
        """A rewritten copy of `frames` (the input array is left as it is)."""
        out = np.array(frames, np.uint8, copy=True)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        b = Batch(out.ctypes.data, int(frames_bytes if frames_bytes is not None else len(out)),
                  off.ctypes.data, ln.ctypes.data, len(off), 0)
        _chk(lib().mosrx_tx_csum_host(self.handle, C.byref(b), flags), "mosrx_tx_csum_host")
        return out

    def tx_csum_dev_checks(self, db: "DevBatch", flags=TX_IP_CSUM | TX_TCP_CSUM) -> np.ndarray:
        """mosrx_tx_csum_dev_checks into the batch's record buffer: one
        TX_CHECK_DTYPE record per frame, the frames left as they are."""
        b = db.batch()
        _chk(lib().mosrx_tx_csum_dev_checks(self.handle, C.byref(b), flags, db.d_out.ptr, None),
             "mosrx_tx_csum_dev_checks")
        _chk(lib().mosrx_sync(self.handle), "mosrx_sync")
        raw = np.empty(max(db.n, 1) * 8, np.uint8)
        db.d_out.download(raw)
        return raw.view(TX_CHECK_DTYPE)[:db.n].copy()

    def tx_csum_dev(self, db: "DevBatch", flags=TX_IP_CSUM | TX_TCP_CSUM, sync: bool = True) -> None:
        b = db.batch()
        _chk(lib().mosrx_tx_csum_dev(self.handle, C.byref(b), flags, None), "mosrx_tx_csum_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    # ---- batched BPF (mosrx_bpf_*) ----
    def bpf_set(self, progs) -> None:
        """progs: list of (insns, len_mode); insns None/empty = no filter (matches)."""
        arr, _keep = _bpf_progs(progs)
        _chk(lib().mosrx_bpf_set(self.handle, arr, len(progs)), "mosrx_bpf_set")

    def bpf_set_async(self, progs) -> None:
        """mosrx_bpf_set_async: in effect at once (interpreter), compiled behind."""
        arr, _keep = _bpf_progs(progs)
        _chk(lib().mosrx_bpf_set_async(self.handle, arr, len(progs)), "mosrx_bpf_set_async")

    def bpf_wait(self) -> None:
        _chk(lib().mosrx_bpf_wait(self.handle), "mosrx_bpf_wait")

    def bpf_pending(self) -> bool:
        rc = lib().mosrx_bpf_pending(self.handle)
        if rc < 0:
            _chk(rc, "mosrx_bpf_pending")
        return rc == 1

    def bpf_set_engine(self, engine: int) -> None:
        """Engine of the next bpf_set: BPF_ENGINE_JIT (hipRTC-compiled set) or BPF_ENGINE_INTERP."""
        _chk(lib().mosrx_bpf_set_engine(self.handle, engine), "mosrx_bpf_set_engine")

    def bpf_engine(self) -> int:
        """Engine of the installed set."""
        return lib().mosrx_bpf_engine(self.handle)

    def bpf_fused(self) -> bool:
        """The installed set has a fused classify + BPF kernel."""
        return lib().mosrx_bpf_fused(self.handle) == 1

    def classify_bpf_dev(self, db: "DevBatch", sync: bool = True, stream: int | None = None) -> None:
        """Records into db.d_out and match masks into db.d_match in one pass."""
        if db.d_match is None:
            db.d_match = DevBuffer(self, max(db.n * 4, 4))
        b = db.batch()
        _chk(lib().mosrx_classify_bpf_dev(self.handle, C.byref(b), db.d_out.ptr, db.d_match.ptr, stream),
             "mosrx_classify_bpf_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def classify_bpf_host(self, frames, off, ln, frames_bytes=None):
        """(records, match masks) of a host batch in one GPU pass."""
        frames = np.ascontiguousarray(frames, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        out = np.zeros(len(off), RESULT_DTYPE)
        match = np.zeros(len(off), np.uint32)
        b = Batch(frames.ctypes.data, int(frames_bytes if frames_bytes is not None else len(frames)),
                  off.ctypes.data, ln.ctypes.data, len(off), 0)
        _chk(lib().mosrx_classify_bpf_host(self.handle, C.byref(b), out.ctypes.data, match.ctypes.data),
             "mosrx_classify_bpf_host")
        return out, match

    def bpf_jit_log(self) -> str:
        return (lib().mosrx_bpf_jit_log(self.handle) or b"").decode(errors="replace")

    def bpf_host(self, frames, off, ln, frames_bytes=None) -> np.ndarray:
        frames = np.ascontiguousarray(frames, np.uint8)
        off = np.ascontiguousarray(off, np.uint32)
        ln = np.ascontiguousarray(ln, np.uint16)
        out = np.zeros(len(off), np.uint32)
        b = Batch(frames.ctypes.data, int(frames_bytes if frames_bytes is not None else len(frames)),
                  off.ctypes.data, ln.ctypes.data, len(off), 0)
        _chk(lib().mosrx_bpf_host(self.handle, C.byref(b), out.ctypes.data), "mosrx_bpf_host")
        return out

    def bpf_dev(self, db: "DevBatch", sync: bool = True, stream: int | None = None) -> None:
        """Match masks into db.d_match; `stream`: a caller's hipStream_t (None: the context's)."""
        if db.d_match is None:
            db.d_match = DevBuffer(self, max(db.n * 4, 4))
        b = db.batch()
        _chk(lib().mosrx_bpf_dev(self.handle, C.byref(b), db.d_match.ptr, stream), "mosrx_bpf_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def last_counters(self) -> np.ndarray:
        c = (C.c_uint64 * NREASON)()
        _chk(lib().mosrx_last_counters(self.handle, c), "mosrx_last_counters")
        return np.array(c[:], np.uint64)

    # ---- device resident ----
    def upload(self, frames, off, ln, frames_bytes=None, max_len=None, hint="auto") -> DevBatch:
        return DevBatch(self, frames, off, ln, frames_bytes, max_len, hint)

    def classify_dev(self, db: DevBatch, sync: bool = True, flow_hash: bool = False, tcpinfo: bool = False) -> None:
        b = db.batch()
        if flow_hash and db.d_fhash is None:
            db.d_fhash = DevBuffer(self, max(db.n * 4, 4))
        if tcpinfo and db.d_tinfo is None:
            db.d_tinfo = DevBuffer(self, max(db.n * 12, 12))
        if tcpinfo:
            _chk(lib().mosrx_classify_dev_ex(self.handle, C.byref(b), db.d_out.ptr,
                                             db.d_fhash.ptr if flow_hash else None, db.d_tinfo.ptr, None),
                 "mosrx_classify_dev_ex")
        elif flow_hash:
            _chk(lib().mosrx_classify_dev_fh(self.handle, C.byref(b), db.d_out.ptr, db.d_fhash.ptr, None),
                 "mosrx_classify_dev_fh")
        else:
            _chk(lib().mosrx_classify_dev(self.handle, C.byref(b), db.d_out.ptr, None), "mosrx_classify_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def classify_dev_compact(self, db: DevBatch, sync: bool = True) -> None:
        """8-byte records (mosrx_result8) into db.d_out8."""
        if db.d_out8 is None:
            db.d_out8 = DevBuffer(self, max(db.n * 8, 8))
        b = db.batch()
        _chk(lib().mosrx_classify_dev_compact(self.handle, C.byref(b), db.d_out8.ptr, None),
             "mosrx_classify_dev_compact")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def group_submit_bpf(self, slot: int, batches: list, outs: list, fhash: list | None, match: list) -> None:
        """mosrx_classify_host_group_submit_bpf over host batches (Batch structs);
        outs / fhash / match: lists of host pointers (wait with group_wait)."""
        n = len(batches)
        bs = (Batch * n)(*batches)
        o = (C.c_void_p * n)(*outs)
        f = (C.c_void_p * n)(*fhash) if fhash is not None else None
        m = (C.c_void_p * n)(*match)
        _chk(lib().mosrx_classify_host_group_submit_bpf(self.handle, slot, bs, n, o, f, m),
             "mosrx_classify_host_group_submit_bpf")

    def group_submit_c8(self, slot: int, batches: list, outs8: list, fhash: list | None = None,
                        match: list | None = None) -> None:
        """mosrx_classify_host_group_submit_c8 (match None) or _bpf_c8: 8-byte records
        into outs8 (host pointers), flow hashes and the installed set's masks."""
        n = len(batches)
        bs = (Batch * n)(*batches)
        o = (C.c_void_p * n)(*outs8)
        f = (C.c_void_p * n)(*fhash) if fhash is not None else None
        if match is None:
            _chk(lib().mosrx_classify_host_group_submit_c8(self.handle, slot, bs, n, o, f),
                 "mosrx_classify_host_group_submit_c8")
        else:
            m = (C.c_void_p * n)(*match)
            _chk(lib().mosrx_classify_host_group_submit_bpf_c8(self.handle, slot, bs, n, o, f, m),
                 "mosrx_classify_host_group_submit_bpf_c8")

    def group_submit_ex(self, slot: int, batches: list, outs: list, tinfo: list | None = None,
                        fhash: list | None = None) -> None:
        """mosrx_classify_host_group_submit_ex: 16-byte records into outs (host
        pointers), pkt_info TCP fields and flow hashes when given."""
        n = len(batches)
        bs = (Batch * n)(*batches)
        o = (C.c_void_p * n)(*outs)
        ti = (C.c_void_p * n)(*tinfo) if tinfo is not None else None
        f = (C.c_void_p * n)(*fhash) if fhash is not None else None
        _chk(lib().mosrx_classify_host_group_submit_ex(self.handle, slot, bs, n, o, ti, f),
             "mosrx_classify_host_group_submit_ex")

    def steer_dev(self, d_rec: int, n: int, rec_bytes: int, d_idx: int, d_qstart: int, d_scratch: int,
                  scratch_bytes: int, sync: bool = True, stream: int | None = None) -> None:
        """mosrx_steer_dev: the stable partition of a device-resident batch's frame
        indices by its records' queue byte (device pointers; the caller owns all)."""
        _chk(lib().mosrx_steer_dev(self.handle, d_rec, n, rec_bytes, d_idx, d_qstart, d_scratch, scratch_bytes,
                                   stream), "mosrx_steer_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    # ---- forwarding ----
    def fwd_set(self, tables: FwdTables | None) -> None:
        """mosrx_fwd_set: install the forwarding tables (None clears them)."""
        _chk(lib().mosrx_fwd_set(self.handle, C.byref(tables) if tables is not None else None), "mosrx_fwd_set")

    def fwd_set_listener(self, listener: bool) -> None:
        _chk(lib().mosrx_fwd_set_listener(self.handle, int(bool(listener))), "mosrx_fwd_set_listener")

    def fwd_plan_dev(self, b: Batch, d_rec: int, rec_bytes: int, in_ifidx: int, d_plan: int, sync: bool = True,
                     stream: int | None = None) -> None:
        """mosrx_fwd_plan_dev: one mosrx_fwd (FWD_DTYPE) per frame of a device-resident
        batch from its records (device pointers; the caller owns all)."""
        _chk(lib().mosrx_fwd_plan_dev(self.handle, C.byref(b), d_rec, rec_bytes, in_ifidx, d_plan, stream),
             "mosrx_fwd_plan_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def fwd_build_dev(self, b: Batch, d_plan: int, d_tx_frames: int, tx_cap: int, d_tx_off: int, d_tx_len: int,
                      d_tx_nif: int, d_tx_src: int, d_tx_count: int, d_scratch: int, scratch_bytes: int,
                      sync: bool = True, stream: int | None = None) -> None:
        """mosrx_fwd_build_dev: the TX frames of a planned batch, in arrival order."""
        _chk(lib().mosrx_fwd_build_dev(self.handle, C.byref(b), d_plan, d_tx_frames, tx_cap, d_tx_off, d_tx_len,
                                       d_tx_nif, d_tx_src, d_tx_count, d_scratch, scratch_bytes, stream),
             "mosrx_fwd_build_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def fwd_build_rings_dev(self, b: Batch, d_plan: int, d_tx_frames: int, ring_cap: int, nrings: int, d_tx_off: int,
                            d_tx_len: int, d_tx_src: int, d_rings: int, d_scratch: int, scratch_bytes: int,
                            sync: bool = True, stream: int | None = None) -> None:
        """mosrx_fwd_build_rings_dev: the TX frames of a planned batch, each in the ring
        of its output netdev (d_rings: nrings records of FWD_RING_DTYPE)."""
        _chk(lib().mosrx_fwd_build_rings_dev(self.handle, C.byref(b), d_plan, d_tx_frames, ring_cap, nrings, d_tx_off,
                                             d_tx_len, d_tx_src, d_rings, d_scratch, scratch_bytes, stream),
             "mosrx_fwd_build_rings_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def fwd_desc_rings_dev(self, b: Batch, d_plan: int, nrings: int, d_tx_src: int, d_tx_len: int, d_tx_mac: int,
                           d_rings: int, d_scratch: int, scratch_bytes: int, sync: bool = True,
                           stream: int | None = None) -> None:
        """mosrx_fwd_desc_rings_dev: per sent frame of a planned batch its source index,
        TX length and 12 rewritten address bytes, sorted by output netdev (d_rings:
        nrings records of FWD_RING_DTYPE); the frames themselves stay where they are."""
        _chk(lib().mosrx_fwd_desc_rings_dev(self.handle, C.byref(b), d_plan, nrings, d_tx_src, d_tx_len, d_tx_mac,
                                            d_rings, d_scratch, scratch_bytes, stream), "mosrx_fwd_desc_rings_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    # ---- firewall rules ----
    def acl_set(self, rules) -> None:
        """mosrx_acl_set: install the firewall rules (ACL_RULE_DTYPE records, or the
        tuples acl_rules takes); None or an empty list clears them."""
        if rules is None or len(rules) == 0:
            _chk(lib().mosrx_acl_set(self.handle, None, 0), "mosrx_acl_set")
            return
        r = rules if isinstance(rules, np.ndarray) else acl_rules(rules)
        r = np.ascontiguousarray(r, ACL_RULE_DTYPE)
        _chk(lib().mosrx_acl_set(self.handle, r.ctypes.data, len(r)), "mosrx_acl_set")

    def acl_count(self) -> int:
        return int(lib().mosrx_acl_count(self.handle))

    def acl_apply_dev(self, b: Batch, d_rec: int, rec_bytes: int, d_plan: int | None, d_hit: int,
                      d_counts: int | None = None, sync: bool = True, stream: int | None = None) -> None:
        """mosrx_acl_apply_dev: the installed rules over a device-resident batch's SYN
        frames -- a u16 hit per frame, counts added per rule, DROP rules' frames
        taken out of the plan (device pointers; the caller owns all)."""
        _chk(lib().mosrx_acl_apply_dev(self.handle, C.byref(b), d_rec, rec_bytes, d_plan, d_hit, d_counts, stream),
             "mosrx_acl_apply_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    # ---- NAT ----
    def nat_set(self, bindings) -> None:
        """mosrx_nat_set: install the bindings (NAT_BINDING_DTYPE records); None or an
        empty array installs the empty table (every eligible frame is then a MISS)."""
        if bindings is None or len(bindings) == 0:
            _chk(lib().mosrx_nat_set(self.handle, None, 0), "mosrx_nat_set")
            return
        b = np.ascontiguousarray(bindings, NAT_BINDING_DTYPE)
        _chk(lib().mosrx_nat_set(self.handle, b.ctypes.data, len(b)), "mosrx_nat_set")

    def nat_count(self) -> int:
        return int(lib().mosrx_nat_count(self.handle))

    def nat_update(self, ops, stream: int = 0) -> None:
        """mosrx_nat_update: NAT_OP_DTYPE records (nat_ops) applied to the installed table
        in place, in `stream`'s order (0: the context's own stream); returns before the
        device has applied them.  A table too full of tombstones is rebuilt instead."""
        o = np.ascontiguousarray(ops, NAT_OP_DTYPE)
        _chk(lib().mosrx_nat_update(self.handle, o.ctypes.data if len(o) else None, len(o), stream), "mosrx_nat_update")

    def nat_stats(self) -> NatStats:
        """mosrx_nat_get_stats: live bindings, tombstones, slots and loop bound of the
        installed table; successful nat_update calls and those that rebuilt."""
        st = np.zeros(1, NAT_STATS_DTYPE)
        _chk(lib().mosrx_nat_get_stats(self.handle, st.ctypes.data), "mosrx_nat_get_stats")
        return NatStats(*(int(v) for v in st[0]))

    def fwd_plan_nat_dev(self, b: Batch, d_rec: int, rec_bytes: int, in_ifidx: int, d_plan: int, d_xlat: int,
                         sync: bool = True, stream: int | None = None) -> None:
        """mosrx_fwd_plan_nat_dev: fwd_plan_dev with the installed bindings applied -- one
        NAT_XLAT_DTYPE record per frame besides the plan (device pointers; the caller owns all)."""
        _chk(lib().mosrx_fwd_plan_nat_dev(self.handle, C.byref(b), d_rec, rec_bytes, in_ifidx, d_plan, d_xlat, stream),
             "mosrx_fwd_plan_nat_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def nat_patch_rings_dev(self, d_xlat: int, d_tx_frames: int, d_tx_off: int, d_tx_src: int, d_rings: int,
                            nrings: int, n: int, sync: bool = True, stream: int | None = None) -> None:
        """mosrx_nat_patch_rings_dev: the translations stored into the frames
        fwd_build_rings_dev built from the same plan."""
        _chk(lib().mosrx_nat_patch_rings_dev(self.handle, d_xlat, d_tx_frames, d_tx_off, d_tx_src, d_rings, nrings, n,
                                             stream), "mosrx_nat_patch_rings_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def slot_acl(self, slot: int, hit: list | None, counts: int | None = None) -> None:
        """mosrx_slot_acl: arm the slot's next group submit with the firewall launch (host
        pointers: a u16 hit array per batch, one counts array or None); hit None disarms."""
        self._acl_arm = (C.c_void_p * len(hit))(*hit) if hit is not None else None   # must outlive the submit
        _chk(lib().mosrx_slot_acl(self.handle, slot, self._acl_arm, counts), "mosrx_slot_acl")

    def slot_fwd(self, slot: int, tx_src: list | None, tx_len: list | None = None, tx_mac: list | None = None,
                 rings: list | None = None, nrings: int = 0, in_ifidx: list | None = None,
                 plan: list | None = None) -> None:
        """mosrx_slot_fwd: arm the slot's next group submit with the plan and the
        descriptor form of the ring build (host pointers per batch); tx_src None disarms."""
        if tx_src is None:
            self._fwd_arm = None
            _chk(lib().mosrx_slot_fwd(self.handle, slot, None), "mosrx_slot_fwd")
            return
        keep = [(C.c_void_p * len(a))(*a) if a is not None else None for a in (plan, tx_src, tx_len, tx_mac, rings)]
        ifs = (C.c_uint8 * len(in_ifidx))(*in_ifidx) if in_ifidx is not None else None
        o = SlotFwdOut(C.cast(ifs, C.c_void_p), nrings, *[C.cast(a, C.c_void_p) for a in keep])
        self._fwd_arm = (keep, ifs, o)   # the pointer arrays must outlive the submit
        _chk(lib().mosrx_slot_fwd(self.handle, slot, C.byref(o)), "mosrx_slot_fwd")

    def slot_steer(self, slot: int, idx: list | None, qstart: list | None) -> None:
        """mosrx_slot_steer: arm the slot's next group submit (host pointers per
        batch: n indices, STEER_QSLOTS queue starts); None, None disarms."""
        if idx is None:
            self._steer_arm = None
            _chk(lib().mosrx_slot_steer(self.handle, slot, None, None), "mosrx_slot_steer")
            return
        # the pointer arrays must outlive the submit
        self._steer_arm = ((C.c_void_p * len(idx))(*idx), (C.c_void_p * len(qstart))(*qstart))
        _chk(lib().mosrx_slot_steer(self.handle, slot, *self._steer_arm), "mosrx_slot_steer")

    def steer_gather_dev(self, d_rec: int, d_off: int | None, d_len: int | None, n: int, rec_bytes: int, d_idx: int,
                         d_qstart: int, d_qrec: int, d_qoff: int | None, d_qlen: int | None, d_scratch: int,
                         scratch_bytes: int, sync: bool = True, stream: int | None = None) -> None:
        """mosrx_steer_gather_dev: steer_dev, with the records (and, with d_qoff /
        d_qlen, the batch's offsets and lengths) also stored in the order of idx."""
        _chk(lib().mosrx_steer_gather_dev(self.handle, d_rec, d_off, d_len, n, rec_bytes, d_idx, d_qstart, d_qrec,
                                          d_qoff, d_qlen, d_scratch, scratch_bytes, stream),
             "mosrx_steer_gather_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def steer_gather_side_dev(self, d_rec: int, d_off: int | None, d_len: int | None, n: int, rec_bytes: int,
                              d_idx: int, d_qstart: int, d_qrec: int, d_qoff: int | None, d_qlen: int | None,
                              d_scratch: int, scratch_bytes: int, fhash: tuple | None = None,
                              match: tuple | None = None, tcpinfo: tuple | None = None, sync: bool = True,
                              stream: int | None = None) -> None:
        """mosrx_steer_gather_side_dev: steer_gather_dev, with each side array given
        as a (source, destination) pair of device pointers also stored in the order of idx."""
        pairs = [p if p is not None else (None, None) for p in (fhash, match, tcpinfo)]
        _chk(lib().mosrx_steer_gather_side_dev(self.handle, d_rec, d_off, d_len, n, rec_bytes, d_idx, d_qstart, d_qrec,
                                               d_qoff, d_qlen, *pairs[0], *pairs[1], *pairs[2], d_scratch,
                                               scratch_bytes, stream), "mosrx_steer_gather_side_dev")
        if sync:
            _chk(lib().mosrx_sync(self.handle), "mosrx_sync")

    def slot_steer_gather_side(self, slot: int, idx: list | None, qstart: list | None = None,
                               qrec: list | None = None, qoff: list | None = None, qlen: list | None = None,
                               qfhash: list | None = None, qmatch: list | None = None,
                               qtcpinfo: list | None = None) -> None:
        """mosrx_slot_steer_gather_side: slot_steer_gather with per-batch host
        destinations for the flow hashes, match masks and pkt_info (any may be None)."""
        if idx is None:
            self._steer_arm = None
            _chk(lib().mosrx_slot_steer_gather_side(self.handle, slot, *([None] * 8)), "mosrx_slot_steer_gather_side")
            return
        self._steer_arm = tuple((C.c_void_p * len(a))(*a) if a is not None else None
                                for a in (idx, qstart, qrec, qoff, qlen, qfhash, qmatch, qtcpinfo))
        _chk(lib().mosrx_slot_steer_gather_side(self.handle, slot, *self._steer_arm), "mosrx_slot_steer_gather_side")

    def slot_steer_gather(self, slot: int, idx: list | None, qstart: list | None = None, qrec: list | None = None,
                          qoff: list | None = None, qlen: list | None = None) -> None:
        """mosrx_slot_steer_gather: slot_steer with per-batch gather outputs (host
        pointers: n records, and n offsets / n lengths or neither); idx None disarms."""
        if idx is None:
            self._steer_arm = None
            _chk(lib().mosrx_slot_steer_gather(self.handle, slot, None, None, None, None, None),
                 "mosrx_slot_steer_gather")
            return
        # the pointer arrays must outlive the submit
        self._steer_arm = tuple((C.c_void_p * len(a))(*a) if a is not None else None
                                for a in (idx, qstart, qrec, qoff, qlen))
        _chk(lib().mosrx_slot_steer_gather(self.handle, slot, *self._steer_arm), "mosrx_slot_steer_gather")

    def group_wait(self, slot: int) -> None:
        _chk(lib().mosrx_classify_host_wait(self.handle, slot), "mosrx_classify_host_wait")

    def set_direct(self, max_bytes: int, max_frames: int = 0xFFFFFFFF) -> None:
        """mosrx_set_direct: group submits of at most max_frames frames and max_bytes of
        pinned input run copy-free."""
        _chk(lib().mosrx_set_direct(self.handle, int(max_bytes), int(max_frames)), "mosrx_set_direct")

    def set_steer_one(self, max_frames: int) -> None:
        """mosrx_set_steer_one: steer launches whose batches all have at most
        max_frames frames (up to STEER_ONE_MAX) run as one kernel; 0: the three launches."""
        _chk(lib().mosrx_set_steer_one(self.handle, int(max_frames)), "mosrx_set_steer_one")

    def get_steer_one(self) -> int:
        return int(lib().mosrx_get_steer_one(self.handle))

    def steer_one_count(self) -> int:
        """mosrx_steer_one_count: this context's steer launches that took the one-launch form."""
        return int(lib().mosrx_steer_one_count(self.handle))

    def set_fwd_one(self, max_frames: int) -> None:
        """mosrx_set_fwd_one: forwarding launches whose batches all have at most max_frames
        frames (up to FWD_ONE_MAX) plan and build their descriptor rings in one kernel; 0: the
        four launches."""
        _chk(lib().mosrx_set_fwd_one(self.handle, int(max_frames)), "mosrx_set_fwd_one")

    def get_fwd_one(self) -> int:
        return int(lib().mosrx_get_fwd_one(self.handle))

    def fwd_one_count(self) -> int:
        """mosrx_fwd_one_count: this context's forwarding launches that took the one-launch form."""
        return int(lib().mosrx_fwd_one_count(self.handle))

    def slot_direct(self, slot: int) -> bool:
        """mosrx_slot_direct: the slot's last group submit ran copy-free."""
        rc = lib().mosrx_slot_direct(self.handle, slot)
        if rc < 0:
            _chk(rc, "mosrx_slot_direct")
        return rc == 1

    def host_register(self, ptr: int, nbytes: int, flags: int = 0) -> None:
        _chk(lib().mosrx_host_register(self.handle, ptr, nbytes, flags), "mosrx_host_register")

    def host_unregister(self, ptr: int) -> None:
        _chk(lib().mosrx_host_unregister(self.handle, ptr), "mosrx_host_unregister")

    def queue_ex(self, dbs: list[DevBatch], flow_hash: bool = False, match: bool = False,
                 compact: bool = False) -> "Queue":
        return Queue(self, dbs, flow_hash=flow_hash, match=match, compact=compact)

    def time_dev(self, dbs: list[DevBatch], iters: int) -> float:
        bs = (Batch * len(dbs))(*[d.batch() for d in dbs])
        outs = (C.c_void_p * len(dbs))(*[d.d_out.ptr for d in dbs])
        ms = C.c_float()
        _chk(lib().mosrx_time_dev(self.handle, bs, len(dbs), outs, iters, C.byref(ms)), "mosrx_time_dev")
        return float(ms.value)

    def time_op(self, op: int, dbs: list[DevBatch], iters: int, nstreams: int = 1, arg: int = 0,
                total: bool = True, kernels: bool = True):
        """mosrx_time_op: (total ms over `iters` launches on `nstreams` streams,
        average single-launch ms); either is None when not requested."""
        for d in dbs:
            if op == OP_CLASSIFY_FH and d.d_fhash is None:
                d.d_fhash = DevBuffer(self, max(d.n * 4, 4))
            if op == OP_CLASSIFY_TI and d.d_tinfo is None:
                d.d_tinfo = DevBuffer(self, max(d.n * 12, 12))
            if op in (OP_BPF, OP_CLASSIFY_BPF) and d.d_match is None:
                d.d_match = DevBuffer(self, max(d.n * 4, 4))
            if op in (OP_STEER, OP_STEER_GATHER, OP_STEER_GATHER_SIDE) and d.d_sidx is None:
                d.d_sidx = DevBuffer(self, max(d.n * 4, 4))
            if op in (OP_FWD_PLAN, OP_FWD, OP_FWD_RINGS, OP_FWD_DESC) and d.d_fplan is None:
                d.d_fplan = DevBuffer(self, max(d.n * 8, 8))
        bs = (Batch * len(dbs))(*[d.batch() for d in dbs])
        # OP_STEER reads the records a classify call left: the compact ones for arg == 8
        outs = (C.c_void_p * len(dbs))(*[(d.d_match.ptr if op == OP_BPF else
                                          d.d_out8.ptr if op in (OP_STEER, OP_STEER_GATHER, OP_STEER_GATHER_SIDE,
                                                                 OP_FWD_PLAN, OP_FWD, OP_FWD_RINGS, OP_FWD_DESC) and (arg & 0xFF) == 8
                                          else d.d_out.ptr) for d in dbs])
        aux = (C.c_void_p * len(dbs))(*[(d.d_match.ptr if op == OP_CLASSIFY_BPF else
                                         d.d_tinfo.ptr if op == OP_CLASSIFY_TI else
                                         d.d_sidx.ptr if op in (OP_STEER, OP_STEER_GATHER, OP_STEER_GATHER_SIDE) else
                                         d.d_fplan.ptr if op in (OP_FWD_PLAN, OP_FWD, OP_FWD_RINGS, OP_FWD_DESC) else
                                         (d.d_fhash.ptr if d.d_fhash else None)) for d in dbs])
        tot, avg = C.c_float(), C.c_float()
        _chk(lib().mosrx_time_op(self.handle, op, arg, bs, len(dbs), outs, aux, iters, nstreams,
                                 C.byref(tot) if total else None, C.byref(avg) if kernels else None),
             "mosrx_time_op")
        return (float(tot.value) if total else None), (float(avg.value) if kernels else None)

    def time_op_dispatch(self, op: int, dbs: list[DevBatch], iters: int, arg: int = 0):
        """mosrx_time_op_dispatch: the kernel's own average duration (ms), each
        launch stamped by its dispatch; None for an op that is not one kernel."""
        def ptr(buf):
            return buf.ptr if buf is not None else None
        bs = (Batch * len(dbs))(*[d.batch() for d in dbs])
        outs = (C.c_void_p * len(dbs))(*[(ptr(d.d_match) if op == OP_BPF else d.d_out.ptr) for d in dbs])
        aux = (C.c_void_p * len(dbs))(*[(ptr(d.d_match) if op == OP_CLASSIFY_BPF else
                                         ptr(d.d_tinfo) if op == OP_CLASSIFY_TI else
                                         ptr(d.d_fhash) if op == OP_CLASSIFY_FH else None) for d in dbs])
        ms = C.c_float()
        rc = lib().mosrx_time_op_dispatch(self.handle, op, arg, bs, len(dbs), outs, aux, iters, C.byref(ms))
        if rc == -95:   # -ENOTSUP: more than one launch per operation
            return None
        _chk(rc, "mosrx_time_op_dispatch")
        return float(ms.value)

    def time_dev_streams(self, dbs: list[DevBatch], iters: int, nstreams: int) -> float:
        """Total ms for `iters` launches spread round-robin over `nstreams` streams."""
        bs = (Batch * len(dbs))(*[d.batch() for d in dbs])
        outs = (C.c_void_p * len(dbs))(*[d.d_out.ptr for d in dbs])
        ms = C.c_float()
        _chk(lib().mosrx_time_dev_streams(self.handle, bs, len(dbs), outs, iters, nstreams, C.byref(ms)),
             "mosrx_time_dev_streams")
        return float(ms.value)

    def time_dev_kernels(self, dbs: list[DevBatch], iters: int) -> float:
        """Average kernel duration (ms), HIP events around every launch."""
        bs = (Batch * len(dbs))(*[d.batch() for d in dbs])
        outs = (C.c_void_p * len(dbs))(*[d.d_out.ptr for d in dbs])
        ms = C.c_float()
        _chk(lib().mosrx_time_dev_kernels(self.handle, bs, len(dbs), outs, iters, C.byref(ms)),
             "mosrx_time_dev_kernels")
        return float(ms.value)

    def queue(self, dbs: list[DevBatch]) -> "Queue":
        return Queue(self, dbs)

    def probe_read_bw(self, nbytes: int = 128 << 20, nbuf: int = 6, iters: int = 60) -> float:
        """Measured streaming-read ceiling (GB/s) of this device."""
        g = C.c_float()
        _chk(lib().mosrx_probe_read_bw(self.handle, nbytes, nbuf, iters, C.byref(g)), "mosrx_probe_read_bw")
        return float(g.value)

    def probe_stamp_floor(self, db: DevBatch, iters: int = 500) -> float:
        """mosrx_probe_stamp_floor: the dispatch-stamped duration (ms) of an empty
        kernel with the grid a classify launch of `db` has."""
        ms = C.c_float()
        b = db.batch()
        _chk(lib().mosrx_probe_stamp_floor(self.handle, C.byref(b), iters, C.byref(ms)), "mosrx_probe_stamp_floor")
        return float(ms.value)

    def device_sync(self):
        _chk(lib().mosrx_device_sync(self.handle), "mosrx_device_sync")

    def host_alloc(self, nbytes: int) -> tuple[int, np.ndarray]:
        p = C.c_void_p()
        _chk(lib().mosrx_host_alloc(self.handle, max(int(nbytes), 1), C.byref(p)), "mosrx_host_alloc")
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (max(int(nbytes), 1),))
        return p.value, arr

    def host_free(self, ptr: int):
        lib().mosrx_host_free(self.handle, ptr)

    def time_host(self, batches: list[Batch], outs: list[int], iters: int) -> float:
        bs = (Batch * len(batches))(*batches)
        os_ = (C.c_void_p * len(outs))(*outs)
        ms = C.c_float()
        _chk(lib().mosrx_time_host(self.handle, bs, len(batches), os_, iters, C.byref(ms)), "mosrx_time_host")
        return float(ms.value)


class Queue:
    """mosrx_queue: one launch classifies every batch of the queue."""

    def __init__(self, ctx: Context, dbs: list[DevBatch], flow_hash: bool = False, match: bool = False,
                 compact: bool = False):
        self.ctx = ctx
        n = len(dbs)
        for d in dbs:
            if flow_hash and d.d_fhash is None:
                d.d_fhash = DevBuffer(ctx, max(d.n * 4, 4))
            if match and d.d_match is None:
                d.d_match = DevBuffer(ctx, max(d.n * 4, 4))
            if compact and d.d_out8 is None:
                d.d_out8 = DevBuffer(ctx, max(d.n * 8, 8))
        bs = (Batch * n)(*[d.batch() for d in dbs])
        outs = (C.c_void_p * n)(*[(d.d_out8.ptr if compact else d.d_out.ptr) for d in dbs])
        h = C.c_void_p()
        if not (flow_hash or match or compact):
            _chk(lib().mosrx_queue_create(ctx.handle, bs, n, outs, C.byref(h)), "mosrx_queue_create")
        else:
            fh = (C.c_void_p * n)(*[d.d_fhash.ptr for d in dbs]) if flow_hash else None
            mt = (C.c_void_p * n)(*[d.d_match.ptr for d in dbs]) if match else None
            _chk(lib().mosrx_queue_create_ex(ctx.handle, bs, n, outs, fh, mt, QUEUE_COMPACT if compact else 0,
                                             C.byref(h)), "mosrx_queue_create_ex")
        self.handle = h.value

    def set_steer(self, idx: list | None, qstart: list | None) -> None:
        """mosrx_queue_set_steer: attach per-batch steer outputs (device pointers:
        n indices, STEER_QSLOTS queue starts) to every run; None, None detaches."""
        if idx is None:
            _chk(lib().mosrx_queue_set_steer(self.ctx.handle, self.handle, None, None), "mosrx_queue_set_steer")
            return
        i = (C.c_void_p * len(idx))(*idx)
        q = (C.c_void_p * len(qstart))(*qstart)
        _chk(lib().mosrx_queue_set_steer(self.ctx.handle, self.handle, i, q), "mosrx_queue_set_steer")

    def set_steer_gather(self, idx: list | None, qstart: list | None = None, qrec: list | None = None,
                         qoff: list | None = None, qlen: list | None = None) -> None:
        """mosrx_queue_set_steer_gather: set_steer with per-batch gather outputs
        (device pointers: n records, and n offsets / n lengths or neither); idx None detaches."""
        arrs = [(C.c_void_p * len(a))(*a) if a is not None else None for a in (idx, qstart, qrec, qoff, qlen)]
        _chk(lib().mosrx_queue_set_steer_gather(self.ctx.handle, self.handle, *arrs), "mosrx_queue_set_steer_gather")

    def set_steer_gather_side(self, idx: list | None, qstart: list | None = None, qrec: list | None = None,
                              qoff: list | None = None, qlen: list | None = None, qfhash: list | None = None,
                              qmatch: list | None = None) -> None:
        """mosrx_queue_set_steer_gather_side: set_steer_gather with per-batch device
        destinations for the queue's own flow hashes / match masks; idx None detaches."""
        arrs = [(C.c_void_p * len(a))(*a) if a is not None else None
                for a in (idx, qstart, qrec, qoff, qlen, qfhash, qmatch)]
        _chk(lib().mosrx_queue_set_steer_gather_side(self.ctx.handle, self.handle, *arrs),
             "mosrx_queue_set_steer_gather_side")

    def set_fwd(self, plan: list | None, in_ifidx: list | None = None, ring_cap: int = 0, nrings: int = 0,
                tx_frames: list | None = None, tx_off: list | None = None, tx_len: list | None = None,
                tx_src: list | None = None, rings: list | None = None) -> None:
        """mosrx_queue_set_fwd: attach forwarding to every run -- per-batch device
        pointers for the plan arrays and, for the ring build, the five TX outputs
        (all or none); in_ifidx: per-batch input netdevs (None: all 0).  plan None detaches."""
        if plan is None:
            _chk(lib().mosrx_queue_set_fwd(self.ctx.handle, self.handle, None), "mosrx_queue_set_fwd")
            return
        keep = [(C.c_void_p * len(a))(*a) if a is not None else None
                for a in (plan, tx_frames, tx_off, tx_len, tx_src, rings)]
        ifs = (C.c_uint8 * len(in_ifidx))(*in_ifidx) if in_ifidx is not None else None
        f = QueueFwd(C.cast(ifs, C.c_void_p), C.cast(keep[0], C.c_void_p), ring_cap, nrings,
                     *[C.cast(a, C.c_void_p) for a in keep[1:]])
        _chk(lib().mosrx_queue_set_fwd(self.ctx.handle, self.handle, C.byref(f)), "mosrx_queue_set_fwd")

    def set_fwd_desc(self, plan: list | None, in_ifidx: list | None = None, nrings: int = 0,
                     tx_src: list | None = None, tx_len: list | None = None, tx_mac: list | None = None,
                     rings: list | None = None) -> None:
        """mosrx_queue_set_fwd_desc: attach the plan and the descriptor form of the ring
        build to every run -- per-batch device pointers; plan None detaches.  Not
        together with set_fwd."""
        if plan is None:
            _chk(lib().mosrx_queue_set_fwd_desc(self.ctx.handle, self.handle, None), "mosrx_queue_set_fwd_desc")
            return
        keep = [(C.c_void_p * len(a))(*a) if a is not None else None for a in (plan, tx_src, tx_len, tx_mac, rings)]
        ifs = (C.c_uint8 * len(in_ifidx))(*in_ifidx) if in_ifidx is not None else None
        f = QueueFwdDesc(C.cast(ifs, C.c_void_p), C.cast(keep[0], C.c_void_p), nrings,
                         *[C.cast(a, C.c_void_p) for a in keep[1:]])
        _chk(lib().mosrx_queue_set_fwd_desc(self.ctx.handle, self.handle, C.byref(f)), "mosrx_queue_set_fwd_desc")

    def set_acl(self, hit: list | None, counts: int | None = None) -> None:
        """mosrx_queue_set_acl: attach the firewall launch to every run -- per-batch
        device pointers for the u16 hit arrays, one counts array for the queue (or
        None); between the plan and the build when forwarding is attached.  hit None detaches."""
        h = (C.c_void_p * len(hit))(*hit) if hit is not None else None
        _chk(lib().mosrx_queue_set_acl(self.ctx.handle, self.handle, h, counts), "mosrx_queue_set_acl")

    def set_nat(self, xlat: list | None) -> None:
        """mosrx_queue_set_nat: plan-nat in the plan launch's place (and the patch behind
        byte rings) on every run -- per-batch device pointers for the NAT_XLAT_DTYPE
        arrays; needs forwarding attached and no firewall rules.  None detaches."""
        x = (C.c_void_p * len(xlat))(*xlat) if xlat is not None else None
        _chk(lib().mosrx_queue_set_nat(self.ctx.handle, self.handle, x), "mosrx_queue_set_nat")

    def run(self, sync: bool = True):
        _chk(lib().mosrx_queue_run(self.ctx.handle, self.handle, None), "mosrx_queue_run")
        if sync:
            _chk(lib().mosrx_sync(self.ctx.handle), "mosrx_sync")

    def time(self, iters: int, others: list["Queue"] = (), kernels: bool = True) -> tuple[float, float]:
        """(total ms of `iters` back-to-back launches cycling over self + others,
        average isolated-launch ms or None when `kernels` is False)."""
        qs = [self] + list(others)
        arr = (C.c_void_p * len(qs))(*[q.handle for q in qs])
        tot, kern = C.c_float(), C.c_float()
        _chk(lib().mosrx_time_queue(self.ctx.handle, arr, len(qs), iters, C.byref(tot),
                                    C.byref(kern) if kernels else None), "mosrx_time_queue")
        return float(tot.value), (float(kern.value) if kernels else None)

    def time_dispatch(self, iters: int, others: list["Queue"] = ()) -> float:
        """The queue kernel's own average duration (ms) over `iters` back-to-back
        launches cycling over self + others, each stamped by its dispatch."""
        qs = [self] + list(others)
        arr = (C.c_void_p * len(qs))(*[q.handle for q in qs])
        ms = C.c_float()
        _chk(lib().mosrx_time_queue_dispatch(self.ctx.handle, arr, len(qs), iters, C.byref(ms)),
             "mosrx_time_queue_dispatch")
        return float(ms.value)

    def destroy(self):
        if self.handle:
            lib().mosrx_queue_destroy(self.ctx.handle, self.handle)
            self.handle = None


def rss_tables(key: bytes) -> np.ndarray:
    out = (C.c_uint32 * 384)()
    _chk(lib().mosrx_rss_tables(key, len(key), out), "mosrx_rss_tables")
    return np.array(out[:], np.uint32)


# ---------------------------------------------------------------------------
# io_module_func backend (include/mosrx_io_module.h): gpu_module_func behind a
# raw-socket / loopback source, driven by the RunMainLoop-shaped rx loop.
# ---------------------------------------------------------------------------
_VOIDFN = C.CFUNCTYPE(None)
_CTXFN = C.CFUNCTYPE(None, C.c_void_p)
_IOCTLFN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int, C.c_int, C.c_void_p)
_RECVFN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int)
_RPTRFN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint16))
_WPTRFN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_uint16)
_SENDFN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_int)


class ResultC(C.Structure):
    """mosrx_result as a ctypes structure (RESULT_DTYPE's layout)."""
    _fields_ = [("rss", C.c_uint32), ("ip_csum", C.c_uint16), ("tcp_csum", C.c_uint16),
                ("payloadlen", C.c_uint16), ("payload_off", C.c_uint8), ("verdict", C.c_int8),
                ("reason", C.c_uint8), ("queue", C.c_uint8), ("tcp_flags", C.c_uint8), ("ihl_doff", C.c_uint8)]


# mosrx_pkt_fn: the rx loop's per-frame consumer (ProcessPacket's place)
_PKTFN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint16, C.POINTER(ResultC))
PKT_TX_IP_CSUM, PKT_TX_TCP_CSUM = 0x01, 0x02
PKT_RX_RSS, DRV_NAME, PKT_RX_RESULTS, PKT_RX_MATCH = 0x03, 0x08, 0x10, 0x11
PKT_RX_TCPINFO, PKT_SET_PARAMS = 0x12, 0x13
PKT_RX_STATE, PKT_RX_RECLASSIFY, PKT_SET_BPF, PKT_RX_FHASH = 0x14, 0x15, 0x16, 0x17
PKT_RX_RESULTS8 = 0x18
PKT_RX_STEER = 0x19
PKT_RX_QUEUE = 0x1A
PKT_RX_QUEUE_SIDE = 0x1B
PKT_RX_FWD = 0x1C
PKT_RX_ACL = 0x1D


class AclView(C.Structure):
    """mosrx_acl_view: dev_ioctl(MOSRX_PKT_RX_ACL)'s answer for the exposed batch."""
    _fields_ = [("n", C.c_uint32), ("nrules", C.c_uint32), ("hit", C.c_void_p), ("counts", C.c_void_p)]


class FwdView(C.Structure):
    """mosrx_fwd_view: dev_ioctl(MOSRX_PKT_RX_FWD)'s answer for the exposed batch."""
    _fields_ = [("n", C.c_uint32), ("nrings", C.c_uint32), ("frames", C.c_void_p), ("off", C.c_void_p),
                ("plan", C.c_void_p), ("tx_src", C.c_void_p), ("tx_len", C.c_void_p), ("tx_mac", C.c_void_p),
                ("rings", C.c_void_p)]


class FwdSendStats(C.Structure):
    """mosrx_fwd_send_stats."""
    _fields_ = [("sent", C.c_uint64), ("no_buffer", C.c_uint64), ("send_calls", C.c_uint64)]
QUEUE_PROBE = 0xFFFFFFFF


class IoModuleFunc(C.Structure):
    """io_module_func (core/src/include/io_module.h:63-78): 14 function pointers."""
    _fields_ = [(n, C.c_void_p) for n in (
        "load_module_upper_half", "load_module_lower_half", "init_handle", "link_devices",
        "release_pkt", "get_wptr", "set_wptr", "send_pkts", "get_rptr", "get_nif", "recv_pkts",
        "select", "destroy_handle", "dev_ioctl")]


class RssInfo(C.Structure):
    _fields_ = [("pktidx", C.c_int8), ("hash_value", C.c_uint32)]


def gpu_module() -> IoModuleFunc:
    return IoModuleFunc.in_dll(lib(), "gpu_module_func")


class GpuBackend:
    """One mTCP-thread's view of gpu_module_func over in-memory / pcap sources."""

    def __init__(self, sources: list[int], params: Params | None = None, batch: int = 32768,
                 max_frame: int = 2048, pipeline: bool = True, cpu: int = 0, gpu_base: int = 0,
                 ngpu: int = 1, bpf=None, group: int = 1, tcpinfo: bool = False, tx_batch: int = 64,
                 timing: bool = False, flowhash: bool = False, tx_csum: bool = False, compact: bool = False,
                 group_bytes: int = 0, group_max_us: int = 0, direct_kb: int | None = None,
                 direct_frames: int | None = None, module_lib=None, steer: bool | int = False,
                 steer_one: int = 0, fwd: FwdTables | None = None, fwd_listener: bool = False, fwd_one: int = 0,
                 acl=None):
        self.L = L = module_lib or lib()
        cfg = ModuleCfg()
        L.mosrx_gpu_module_cfg_default(C.byref(cfg))
        cfg.num_ifs = len(sources)
        for i, s in enumerate(sources):
            cfg.src[i] = s
            cfg.if_names[i].value = f"gpu{i}".encode()
        cfg.batch, cfg.max_frame, cfg.pipeline = batch, max_frame, int(pipeline)
        cfg.gpu_base, cfg.ngpu = gpu_base, ngpu
        cfg.group, cfg.tcpinfo, cfg.tx_batch, cfg.flowhash = group, int(tcpinfo), tx_batch, int(flowhash)
        cfg.tx_csum = int(tx_csum)
        cfg.compact = int(compact)          # 8-byte records (results8), with or without filters
        cfg.group_bytes = group_bytes       # auto groups' frame bytes per launch (0: MOSRX_GROUP_AUTO_BYTES)
        cfg.group_max_us = group_max_us     # a group's latency budget (0: none)
        if direct_kb is not None:
            cfg.direct_kb = direct_kb       # copy-free groups up to this many KiB (0: none)
        if direct_frames is not None:
            cfg.direct_frames = direct_frames   # ... and up to this many frames
        cfg.steer = int(steer)              # 1: every group steered on the GPU (steer_view, run_loop_queues);
        #                                     2: and gathered queue-major (queue_view, Hub);
        #                                     3: and the side arrays with them (queue_side)
        if params is not None:
            cfg.params = params
        self.params = Params.from_buffer_copy(cfg.params)
        self._bpf = None
        if bpf:
            self._bpf = _bpf_progs(bpf)          # kept alive until init_handle has installed them
            cfg.bpf_progs = C.addressof(self._bpf[0])
            cfg.bpf_nprog = len(bpf)
        _chk(L.mosrx_gpu_module_configure(C.byref(cfg)), "mosrx_gpu_module_configure")
        # steered groups of batches up to this many frames: one steer launch (0: never; always set,
        # so a backend does not inherit an earlier one's)
        _chk(L.mosrx_gpu_module_set_steer_one(int(steer_one)), "mosrx_gpu_module_set_steer_one")
        # forwarded groups of batches up to this many frames: one forwarding launch (0: never; always set)
        _chk(L.mosrx_gpu_module_set_fwd_one(int(fwd_one)), "mosrx_gpu_module_set_fwd_one")
        # forwarding on the GPU with these tables (None: off; always set, for the same reason)
        L.mosrx_gpu_module_set_fwd.restype = C.c_int
        L.mosrx_gpu_module_set_fwd.argtypes = [C.POINTER(FwdTables), C.c_int]
        _chk(L.mosrx_gpu_module_set_fwd(C.byref(fwd) if fwd is not None else None, int(bool(fwd_listener))),
             "mosrx_gpu_module_set_fwd")
        # firewall rules (ACL_RULE_DTYPE records or acl_rules' tuples): every group submit is armed with them
        L.mosrx_gpu_module_set_acl.restype = C.c_int
        L.mosrx_gpu_module_set_acl.argtypes = [C.c_void_p, C.c_uint32]
        r = None if acl is None or len(acl) == 0 else np.ascontiguousarray(
            acl if isinstance(acl, np.ndarray) else acl_rules(acl), ACL_RULE_DTYPE)
        _chk(L.mosrx_gpu_module_set_acl(r.ctypes.data if r is not None else None, len(r) if r is not None else 0),
             "mosrx_gpu_module_set_acl")
        self.nif = len(sources)
        self.sources = list(sources)
        self.m = IoModuleFunc.in_dll(L, "gpu_module_func")
        self._ctx_obj = C.c_uint64(0xC0DE0000 + cpu)      # stands in for struct mtcp_thread_context *
        self.ctx = C.addressof(self._ctx_obj)
        _chk(L.mosrx_gpu_module_bind(self.ctx, cpu), "mosrx_gpu_module_bind")
        _VOIDFN(self.m.load_module_upper_half)()
        _CTXFN(self.m.init_handle)(self.ctx)
        self._recv = _RECVFN(self.m.recv_pkts)
        self._rptr = _RPTRFN(self.m.get_rptr)
        self._ioctl = _IOCTLFN(self.m.dev_ioctl)
        self._wptr = _WPTRFN(self.m.get_wptr)
        self._send = _SENDFN(self.m.send_pkts)
        if timing:
            _chk(L.mosrx_gpu_module_set_timing(self.ctx, 1), "mosrx_gpu_module_set_timing")

    def steer_one_count(self) -> int:
        """mosrx_gpu_module_steer_one_count: steered groups that took the one-launch form."""
        return int(self.L.mosrx_gpu_module_steer_one_count(self.ctx))

    def fwd_one_count(self) -> int:
        """mosrx_gpu_module_fwd_one_count: forwarded groups that took the one-launch form."""
        self.L.mosrx_gpu_module_fwd_one_count.restype = C.c_uint64
        self.L.mosrx_gpu_module_fwd_one_count.argtypes = [C.c_void_p]
        return int(self.L.mosrx_gpu_module_fwd_one_count(self.ctx))

    def recv_pkts(self, ifidx: int = 0) -> int:
        return self._recv(self.ctx, ifidx)

    def get_rptr(self, ifidx: int, index: int) -> bytes | None:
        ln = C.c_uint16()
        p = self._rptr(self.ctx, ifidx, index, C.byref(ln))
        return C.string_at(p, ln.value) if p else None

    def results(self, ifidx: int, n: int) -> np.ndarray:
        p = C.c_void_p()
        if self._ioctl(self.ctx, ifidx, PKT_RX_RESULTS, C.byref(p)):
            raise MosrxError(5, "dev_ioctl(MOSRX_PKT_RX_RESULTS)")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n * 16,)).view(RESULT_DTYPE).copy()

    def results8(self, ifidx: int, n: int) -> np.ndarray:
        """The exposed batch's 8-byte records (a compact backend's batch without filters)."""
        p = C.c_void_p()
        if self._ioctl(self.ctx, ifidx, PKT_RX_RESULTS8, C.byref(p)):
            raise MosrxError(5, "dev_ioctl(MOSRX_PKT_RX_RESULTS8)")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n * 8,)).view(RESULT8_DTYPE).copy()

    def matches(self, ifidx: int, n: int) -> np.ndarray:
        """dev_ioctl(MOSRX_PKT_RX_MATCH): the batch's BPF match masks."""
        p = C.c_void_p()
        if self._ioctl(self.ctx, ifidx, PKT_RX_MATCH, C.byref(p)):
            raise MosrxError(5, "dev_ioctl(MOSRX_PKT_RX_MATCH)")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), (n,)).copy()

    def fhashes(self, ifidx: int, n: int) -> np.ndarray:
        """dev_ioctl(MOSRX_PKT_RX_FHASH): the batch's flow-table hashes (cfg.flowhash)."""
        p = C.c_void_p()
        if self._ioctl(self.ctx, ifidx, PKT_RX_FHASH, C.byref(p)):
            raise MosrxError(5, "dev_ioctl(MOSRX_PKT_RX_FHASH)")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), (n,)).copy()

    def tcpinfo(self, ifidx: int, n: int) -> np.ndarray:
        """dev_ioctl(MOSRX_PKT_RX_TCPINFO): the batch's pkt_info TCP fields."""
        p = C.c_void_p()
        if self._ioctl(self.ctx, ifidx, PKT_RX_TCPINFO, C.byref(p)):
            raise MosrxError(5, "dev_ioctl(MOSRX_PKT_RX_TCPINFO)")
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n * 12,)).view(TCPINFO_DTYPE).copy()

    def steer_view(self, ifidx: int):
        """dev_ioctl(MOSRX_PKT_RX_STEER): (idx[n], qstart[STEER_QSLOTS], num_queues)
        of the exposed batch, or None when the backend does not steer."""
        v = SteerView()
        if self._ioctl(self.ctx, ifidx, PKT_RX_STEER, C.byref(v)):
            return None
        idx = np.ctypeslib.as_array(C.cast(v.idx, C.POINTER(C.c_uint32)), (max(v.n, 1),))[:v.n].copy()
        qs = np.ctypeslib.as_array(C.cast(v.qstart, C.POINTER(C.c_uint32)), (STEER_QSLOTS,)).copy()
        return idx, qs, int(v.num_queues)

    def queue_view(self, ifidx: int, q: int):
        """dev_ioctl(MOSRX_PKT_RX_QUEUE): queue q's share of the exposed batch as
        (rec bytes [n, rec_bytes], off[n], len[n], idx[n], frame base address), or
        None unless the batch was gathered (cfg.steer = 2)."""
        v = QueueView()
        v.q = q
        if self._ioctl(self.ctx, ifidx, PKT_RX_QUEUE, C.byref(v)):
            return None
        return _queue_view_arrays(v)

    def queue_side(self, ifidx: int, q: int):
        """dev_ioctl(MOSRX_PKT_RX_QUEUE_SIDE): queue q's share of the exposed batch's
        side arrays as (fhash[n], match[n], tcpinfo[n]), each None where the batch
        has none; None unless the batch was gathered with cfg.steer = 3."""
        v = QueueSide()
        v.q = q
        if self._ioctl(self.ctx, ifidx, PKT_RX_QUEUE_SIDE, C.byref(v)):
            return None
        return _queue_side_arrays(v)

    def acl_view(self, ifidx: int):
        """dev_ioctl(MOSRX_PKT_RX_ACL): the exposed batch's (hit[n], counts[nrules] so far), or
        None when the ioctl answers -1 (no rules, no batch, the batch was touched)."""
        v = AclView()
        if self._ioctl(self.ctx, ifidx, PKT_RX_ACL, C.byref(v)):
            return None
        hit = np.ctypeslib.as_array(C.cast(v.hit, C.POINTER(C.c_uint16)), (v.n,)).copy() if v.n else np.zeros(0, np.uint16)
        cnt = np.ctypeslib.as_array(C.cast(v.counts, C.POINTER(C.c_uint32)), (ACL_MAX_RULES,)).copy()
        assert not cnt[v.nrules:].any()
        return hit, cnt[:v.nrules]

    def fwd_view(self, ifidx: int):
        """dev_ioctl(MOSRX_PKT_RX_FWD): the exposed batch's (plan[n], tx_src[m], tx_len[m],
        tx_mac[12 m] bytes, rings[nrings]) with m the rings' total count, or None when the
        ioctl answers -1 (forwarding off, no batch, the batch was touched)."""
        v = FwdView()
        if self._ioctl(self.ctx, ifidx, PKT_RX_FWD, C.byref(v)):
            return None

        def arr(p, nbytes, dtype):
            if not nbytes:
                return np.zeros(0, dtype)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (nbytes,)).view(dtype).copy()
        rings = arr(v.rings, 16 * v.nrings, FWD_RING_DTYPE)
        m = int(rings["count"].sum())
        return (arr(v.plan, 8 * v.n, FWD_DTYPE), arr(v.tx_src, 4 * m, np.uint32), arr(v.tx_len, 2 * m, np.uint16),
                arr(v.tx_mac, 12 * m, np.uint8), rings)

    def forward(self, ifidx: int) -> tuple[int, FwdSendStats]:
        """mosrx_backend_forward for the batch exposed on ifidx: (its return -- frames
        sent, or -1 when the view is not there --, the send's stats)."""
        st = FwdSendStats()
        fn = self.L.mosrx_backend_forward
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return int(fn(C.addressof(self.m), self.ctx, ifidx, C.byref(st))), st

    def run_loop_queues(self, nq: int, fn=None, args: list | None = None, max_rounds: int = 0) -> RxStats:
        """mosrx_rx_loop_queues over this backend: fn (a _PKTFN callback) gets
        args[q] (integers passed as the void * argument) for queue q's frames."""
        st = RxStats()
        a = (C.c_void_p * nq)(*(args if args is not None else [None] * nq))
        _chk(lib().mosrx_rx_loop_queues(C.addressof(self.m), self.ctx, self.nif, nq,
                                        C.cast(fn, C.c_void_p) if fn is not None else None, a, max_rounds,
                                        C.byref(st)), "mosrx_rx_loop_queues")
        return st

    def set_params(self, ifidx: int, params: Params) -> int:
        """dev_ioctl(MOSRX_PKT_SET_PARAMS): the stack state changed (0 or -1)."""
        return self._ioctl(self.ctx, ifidx, PKT_SET_PARAMS, C.byref(params))

    def ioctl_raw(self, ifidx: int, cmd: int, argp) -> int:
        return self._ioctl(self.ctx, ifidx, cmd, argp)

    def send(self, ifidx: int, frame: bytes) -> None:
        """get_wptr + copy (EthernetOutput, eth_out.c:80-84): the frame waits for send_pkts."""
        p = self._wptr(self.ctx, ifidx, len(frame))
        if not p:
            raise MosrxError(5, "get_wptr")
        C.memmove(p, frame, len(frame))

    def send_offloaded(self, ifidx: int, frame: bytes, ip: bool, tcp: bool) -> tuple[int, int]:
        """get_wptr + copy, then mOS's TX checksum offload requests for the frame
        (ip_out.c:169-174, tcp_out.c:207-218: dev_ioctl with its IP header):
        the (PKT_TX_IP_CSUM, PKT_TX_TCP_CSUM) returns, None where not asked."""
        p = self._wptr(self.ctx, ifidx, len(frame))
        if not p:
            raise MosrxError(5, "get_wptr")
        C.memmove(p, frame, len(frame))
        iph = C.c_void_p(p + 14)
        ri = self._ioctl(self.ctx, ifidx, PKT_TX_IP_CSUM, iph) if ip else None
        rt = self._ioctl(self.ctx, ifidx, PKT_TX_TCP_CSUM, iph) if tcp else None
        return ri, rt

    def send_pkts(self, ifidx: int) -> int:
        return self._send(self.ctx, ifidx)

    def stats(self) -> ModuleStats:
        st = ModuleStats()
        _chk(self.L.mosrx_gpu_module_stats_of(self.ctx, C.byref(st)), "mosrx_gpu_module_stats_of")
        return st

    def forwarder(self, out_if: list[int], listener: bool = False) -> Forwarder:
        """A mosrx_forwarder for run_loop(forward=...): netdev i -> out_if[i], the
        frames mOS forwards under the backend's stack state (mosrx_mos_forwards);
        `listener`: an end-host socket listens (its orphans get a RST, not forwarded)."""
        f = Forwarder()
        f.iom = C.addressof(self.m)
        f.ctx = self.ctx
        for i in range(16):
            f.out_if[i] = out_if[i] if i < len(out_if) else -1
        f.forward, f.num_msp, f.listener = self.params.forward, self.params.num_msp, int(listener)
        return f

    def rss_of(self, ifidx: int, pktidx: int) -> int | None:
        ri = RssInfo(pktidx, 0)
        return None if self._ioctl(self.ctx, ifidx, PKT_RX_RSS, C.byref(ri)) else ri.hash_value

    def run_loop(self, max_pkts: int = 0, idle_rounds: int = 1, idle_us: int = 0, max_us: int = 0,
                 forward: Forwarder | None = None, probe: LatencyProbe | None = None) -> RxStats:
        """mosrx_rx_loop_ex over this backend; `forward`: the mosrx_forward_frame
        consumer; `probe`: the residency of a paced source's frames (RxLoopOpts.probe)."""
        st = RxStats()
        o = RxLoopOpts(max_pkts, idle_rounds, idle_us, max_us, C.addressof(probe) if probe is not None else None)
        fn, arg = None, None
        if forward is not None:
            fn, arg = C.cast(lib().mosrx_forward_frame, C.c_void_p), C.byref(forward)
        _chk(lib().mosrx_rx_loop_ex(C.addressof(self.m), self.ctx, self.nif, C.byref(o), fn, arg, C.byref(st)),
             "mosrx_rx_loop_ex")
        return st

    def close(self):
        if self.ctx:
            _CTXFN(self.m.destroy_handle)(self.ctx)
            self.ctx = None
            for s in self.sources:
                lib().mosrx_source_close(s)
            self.sources = []


def _queue_view_arrays(v: QueueView):
    n = int(v.n)
    if n == 0:
        return (np.zeros((0, int(v.rec_bytes) or 16), np.uint8), np.zeros(0, np.uint32), np.zeros(0, np.uint16),
                np.zeros(0, np.uint32), v.frames)
    rec = np.ctypeslib.as_array(C.cast(v.rec, C.POINTER(C.c_uint8)), (n * v.rec_bytes,)).reshape(n, -1).copy()
    off = np.ctypeslib.as_array(C.cast(v.off, C.POINTER(C.c_uint32)), (n,)).copy()
    ln = np.ctypeslib.as_array(C.cast(v.len, C.POINTER(C.c_uint16)), (n,)).copy()
    idx = np.ctypeslib.as_array(C.cast(v.idx, C.POINTER(C.c_uint32)), (n,)).copy()
    return rec, off, ln, idx, v.frames


def _queue_side_arrays(v: QueueSide):
    n = int(v.n)

    def arr(p, dtype):
        if not p:
            return None
        if n == 0:
            return np.zeros(0, dtype)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n * dtype.itemsize,)).view(dtype).copy()
    return arr(v.fhash, np.dtype(np.uint32)), arr(v.match, np.dtype(np.uint32)), arr(v.tcpinfo, TCPINFO_DTYPE)


def hub_module(module_lib=None) -> IoModuleFunc:
    return IoModuleFunc.in_dll(module_lib or lib(), "mosrx_hub_module_func")


class Hub:
    """mosrx_hub over one gathering backend (an io_module_func address and its
    context): endpoint(core) is core's context for hub_module().  Open it, and
    run core 0's endpoint, on the thread that opened the backend."""

    def __init__(self, backend_iom: int, backend_ctx: int | None, nif: int, ncores: int):
        h = C.c_void_p()
        _chk(lib().mosrx_hub_open(backend_iom, backend_ctx, nif, ncores, C.byref(h)), "mosrx_hub_open")
        self.handle, self.nif, self.ncores = h.value, nif, ncores
        self.m = hub_module()
        self.iom = C.addressof(self.m)

    def endpoint(self, core: int) -> int:
        p = lib().mosrx_hub_endpoint(self.handle, core)
        if not p:
            raise MosrxError(22, "mosrx_hub_endpoint")
        return p

    def run_loop(self, core: int, fn=None, arg=None, max_pkts: int = 0) -> tuple[int, RxStats]:
        """mosrx_rx_loop over core's endpoint (it ends at the first idle round): (rc, stats)."""
        st = RxStats()
        rc = lib().mosrx_rx_loop(self.iom, self.endpoint(core), self.nif, max_pkts,
                                 C.cast(fn, C.c_void_p) if fn is not None else None, arg, C.byref(st))
        return rc, st

    def stats(self) -> HubStats:
        st = HubStats()
        _chk(lib().mosrx_hub_stats_get(self.handle, C.byref(st)), "mosrx_hub_stats_get")
        return st

    def close(self) -> int:
        """mosrx_hub_close: 0, or -EBUSY (-16) while a share is outstanding (the hub stays open)."""
        if not self.handle:
            return 0
        rc = lib().mosrx_hub_close(self.handle)
        if rc == 0:
            self.handle = None
        return rc


SRC_BEST, SRC_FILL, SRC_PER_FRAME = 0, 1, 2


def paced_source(inner: int, rate_pps: float) -> int:
    """mosrx_source_paced: `inner`'s frames released at rate_pps (takes inner over)."""
    s = lib().mosrx_source_paced(inner, float(rate_pps))
    if not s:
        raise MosrxError(22, "mosrx_source_paced")
    return s


def mem_source(frames: np.ndarray, off: np.ndarray, ln: np.ndarray, loops: int = 1, mode: int = SRC_BEST) -> int:
    frames = np.ascontiguousarray(frames, np.uint8)
    off = np.ascontiguousarray(off, np.uint32)
    ln = np.ascontiguousarray(ln, np.uint16)
    s = lib().mosrx_source_mem(frames.ctypes.data, off.ctypes.data, ln.ctypes.data, len(off), loops)
    if not s:
        raise MosrxError(12, "mosrx_source_mem")
    if mode != SRC_BEST:
        _chk(lib().mosrx_source_mem_set_mode(s, mode), "mosrx_source_mem_set_mode")
    return s


def afpacket_source(ifname: str, ring_blocks: int = 8, retire_ms: int = 1, fanout_group: int = 0,
                    copy: bool = False) -> int:
    """mosrx_source_afpacket_ex (TPACKET_V3 ring; needs CAP_NET_RAW)."""
    o = AfpOpts(ring_blocks, retire_ms, fanout_group, int(copy))
    s = lib().mosrx_source_afpacket_ex(ifname.encode(), C.byref(o))
    if not s:
        raise MosrxError(1, f"mosrx_source_afpacket_ex({ifname})")
    return s


def afpacket_info(src: int) -> AfpInfo:
    i = AfpInfo()
    _chk(lib().mosrx_source_afpacket_info(src, C.byref(i)), "mosrx_source_afpacket_info")
    return i


def source_tx_pcap(src: int, path: str | None) -> None:
    _chk(lib().mosrx_source_tx_pcap(src, path.encode() if path else None), "mosrx_source_tx_pcap")


def source_send(src: int, frame: bytes) -> int:
    return lib().mosrx_source_send(src, frame, len(frame))


def source_tx_stats(src: int) -> tuple[int, int, int]:
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _chk(lib().mosrx_source_tx_stats(src, C.byref(a), C.byref(b), C.byref(c)), "mosrx_source_tx_stats")
    return a.value, b.value, c.value


def source_borrow(src, max_n: int, max_frame: int = 65535):
    """One zero-copy run of the source (mosrx_source_borrow): (frames as bytes
    objects, the run's base address, off, len), or None when nothing is ready.
    The run stays valid until source_give_back."""
    off = np.zeros(max(1, max_n), np.uint32)
    ln = np.zeros(max(1, max_n), np.uint16)
    base, nbytes = C.c_void_p(), C.c_uint64()
    n = lib().mosrx_source_borrow(src, max_n, max_frame, C.byref(base), C.byref(nbytes),
                                  off.ctypes.data, ln.ctypes.data)
    _chk(min(n, 0), "mosrx_source_borrow")
    if n == 0:
        return None
    frames = [C.string_at(base.value + int(o), int(l)) for o, l in zip(off[:n], ln[:n])]
    return frames, base.value, off[:n].copy(), ln[:n].copy()


def source_give_back(src) -> None:
    _chk(lib().mosrx_source_give_back(src), "mosrx_source_give_back")


def read_pcap(path: str) -> list[bytes]:
    """Frames of a classic pcap file through the library's own reader (mosrx_source_pcap)."""
    s = lib().mosrx_source_pcap(path.encode(), 1)
    if not s:
        raise MosrxError(2, f"mosrx_source_pcap({path})")
    buf = np.zeros(65536, np.uint8)
    out = []
    try:
        while True:
            n = lib().mosrx_source_next(s, buf.ctypes.data, len(buf))
            if n <= 0:
                return out
            out.append(bytes(buf[:n]))
    finally:
        lib().mosrx_source_close(s)


def _sysfs_props(path: str) -> dict:
    out = {}
    try:
        with open(path) as fh:
            for line in fh:
                k, _, v = line.strip().partition(" ")
                if v.strip().lstrip("-").isdigit():
                    out[k] = int(v)
    except OSError:
        pass
    return out


def _parse_cpulist(text: str) -> list[int]:
    cpus = []
    for part in text.strip().split(","):
        if not part:
            continue
        lo, _, hi = part.partition("-")
        cpus += list(range(int(lo), int(hi or lo) + 1))
    return cpus


def gpu_numa_cpus(device: int, root: str = "/"):
    """(PCI address, NUMA node, that node's cores) of HIP device `device`, read from
    sysfs without touching the GPU (so a rank can bind itself before its first HIP
    call): the KFD topology's GPU nodes in order -- HIP's device order -- less those
    ROCR_VISIBLE_DEVICES / HIP_VISIBLE_DEVICES hide, the GPU's PCI numa_node, the
    node's cpulist.  None when any of it is unknown."""
    base = os.path.join(root, "sys", "class", "kfd", "kfd", "topology", "nodes")
    try:
        ids = sorted(int(d) for d in os.listdir(base) if d.isdigit())
    except OSError:
        return None
    gpus = []
    for k in ids:
        pr = _sysfs_props(os.path.join(base, str(k), "properties"))
        if pr.get("simd_count", 0) > 0 and "location_id" in pr:
            loc = pr["location_id"]
            gpus.append(f"{pr.get('domain', 0):04x}:{(loc >> 8) & 0xFF:02x}:{(loc >> 3) & 0x1F:02x}.{loc & 7:x}")
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v:
            try:
                gpus = [gpus[int(x)] for x in v.split(",") if x.strip()]
            except (ValueError, IndexError):
                return None
    if not 0 <= device < len(gpus):
        return None
    bdf = gpus[device]
    try:
        with open(os.path.join(root, "sys", "bus", "pci", "devices", bdf, "numa_node")) as fh:
            node = int(fh.read().strip())
        with open(os.path.join(root, "sys", "devices", "system", "node", f"node{node}", "cpulist")) as fh:
            cpus = _parse_cpulist(fh.read())
    except (OSError, ValueError):
        return None
    return (bdf, node, cpus) if node >= 0 and cpus else None


def bind_to_gpu_node(device: int, root: str = "/") -> dict:
    """Bind the calling process to the cores of device's NUMA node (those it may
    run on), as mOS binds each mTCP thread to its core's node (cpu.c:56-87).
    Call before the first GPU call; never re-execs.  Returns what was done."""
    info = gpu_numa_cpus(device, root)
    if not info:
        return {"device": device, "bound": False, "why": "topology unknown"}
    bdf, node, cpus = info
    allowed = os.sched_getaffinity(0)
    mine = sorted(set(cpus) & allowed)
    if not mine:
        return {"device": device, "pci": bdf, "node": node, "bound": False,
                "why": f"none of node {node}'s cores in this process's affinity"}
    if set(mine) != allowed:
        os.sched_setaffinity(0, mine)
    return {"device": device, "pci": bdf, "node": node, "bound": True, "cpus": len(mine)}


def shard_plan(nbatches: int, world: int, rank: int) -> list[int]:
    """Round-robin split of a job's batches over GPUs: batch b -> GPU b % world.

    No exchange step exists between GPUs, so the plan is the whole multi-GPU protocol:
    each rank classifies its own batches; results land in disjoint slices."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("bad world/rank")
    return list(range(rank, nbatches, world))


def split_batches(frames: np.ndarray, off: np.ndarray, ln: np.ndarray, batch: int):
    """Cut a packed trace into consecutive batches of `batch` frames (views re-based
    so every batch is self-contained: its own frames buffer and offsets)."""
    out = []
    for s in range(0, len(off), batch):
        o, l = off[s:s + batch], ln[s:s + batch]
        lo = int(o.min()) & ~15 if len(o) else 0
        hi = int((o.astype(np.uint64) + l).max()) if len(o) else 0
        out.append((frames[lo:hi + 64], (o - lo).astype(np.uint32), l.copy(), hi - lo))
    return out
