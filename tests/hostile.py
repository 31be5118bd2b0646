"""Hostile inputs for the plan, firewall and NAT launches: a seeded generator of
frames whose header fields are drawn over their whole ranges, the buffer cuts
around one frame, binding tables whose longest probe run wraps past slot 0, and
rule tables with their match at the edges.  A helper, not a test:
tests/test_hostile.py asserts that the inputs do what they claim, and
tests/test_hostile_gpu.py puts them through the launches.

Every frame starts from a flow of small pools of addresses and ports (about half
of the TCP frames belong to a binding of `bindings()`, about half of the SYNs
match a rule of each set of `rule_sets()`), gets its header fields set -- ihl
5..15 behind random option bytes, doff 0..15 over a random reserved nibble, a
segment length ip_len - 4 * ihl out of SEGLENS, flags over all 256 values, 0..7
bytes of random trailing pad, on about half of the frames the Ethernet minimum
of 60 bytes on top -- and then its checksums the way mOS verifies them
(tcp.c:429-434: over ip_len - 4 * ihl bytes), so that the classify pass accepts
what the fields allow.  A segment under 18 bytes does not hold its check word:
the sum is then made right through another word of the segment (the sequence
number, the destination port) or, for an empty segment, through the destination
address.  Where the segment is under 20 bytes the rest of the 20-byte TCP header
follows it as pad on half of those frames (the classify pass needs the capture
to hold it) and is left off on the other half (TRUNCATED).  One frame in five is
damaged on purpose (DAMAGE).  Records are never forced: they are what
oracle_py.classify says of these bytes.

Frames sit at offsets of every residue mod 16.  Tile 1 (frames 256..511) holds
no SYN without ACK, tile 2 exactly one (frame LONE_SYN), and frame 1024 is a tile
of one frame, a SYN of a bound flow.
"""
import itertools
import struct
import types

import numpy as np

import mosrx
import nat_cases as NC
import oracle_py as O
from pktlib import csum16, tcp_frame

SEED = 0x4057113
N = 1025
T = 256
NAT_IP = NC.NAT_IP
TABLES = NC.TABLES            # clients 10/8 behind netdev 1, servers on 2, 172.16/12 routed without ARP
PARAMS = dict(num_msp=1, forward=1)

CLI = ["10.1.1.5", "10.1.3.7", "10.2.2.9", "10.2.4.11", "172.16.5.5"]
CPORT = [30000, 30001, 30002, 30003]
SVR = ["198.51.100.1", "198.51.100.9"]
SPORT = [80, 443]
COMBOS = list(itertools.product(CLI, CPORT, SVR, SPORT))     # 80 flows, every other pair of them bound
SEGLENS = ("0", "4", "12", "16", "19", "20", "21", "4*doff-1", "4*doff", "4*doff+odd", "4*doff+even")
SEG_WEIGHTS = (.03, .04, .05, .06, .05, .07, .06, .06, .16, .21, .21)
DAMAGE = (("bad_ip",), ("bad_tcp",), ("version5",), ("tot_len", "0"), ("tot_len", "19"), ("tot_len", "capture-13"),
          ("len", "33"), ("len", "34"), ("len", "14+4*ihl+11"), ("len", "14+4*ihl+19"), ("len", "14+tot_len-1"),
          ("udp",), ("arp",), ("ethertype",))
LONE_SYN = 2 * T + 77         # wave 1 of tile 2
IHL_J = (0, 1, 3, 4, 11, 12, 13, 15, 16, 17, 18, 19, 20)

_cache = {}


def bound(idx):
    return ((idx >> 1) ^ idx) & 1 == 0


def flows():
    """[(cli_ip, cli_port, svr_ip, svr_port, nat_port)] of the bound flows: 40 bindings, a table of 256 slots."""
    return [(c, cp, s, sp, 1025 + i) for i, (c, cp, s, sp) in enumerate(COMBOS) if bound(i)]


def bindings():
    return mosrx.nat_bindings(flows(), nat_ip=NAT_IP)


def rec8_of(rec):
    """The 8-byte form of 16-byte records."""
    r8 = np.zeros(len(rec), mosrx.RESULT8_DTYPE)
    for k in ("rss", "reason", "queue", "verdict", "tcp_flags"):
        r8[k] = rec[k]
    return r8


def ip_fix(b, ihl):
    b[24:26] = b"\0\0"
    struct.pack_into("!H", b, 24, csum16(bytes(b[14:14 + 4 * ihl])))


def tcp_fix(b, ihl, seglen):
    """Make TCPCalcChecksum over `seglen` bytes come out right; returns the frame offset of the word used."""
    th = 14 + 4 * ihl
    at = th + 16 if seglen >= 18 else th + 4 if seglen >= 6 else th + 2 if seglen >= 4 else 32
    b[at:at + 2] = b"\0\0"
    pseudo = bytes(b[26:34]) + struct.pack("!BBH", 0, 6, seglen)
    struct.pack_into("!H", b, at, csum16(pseudo + bytes(b[th:th + seglen])))
    if at == 32:              # the destination address changed
        ip_fix(b, ihl)
    return at


def wire(rng, src, dst, sport, dport, ihl, doff, seglen, flags, pad=0, min60=False, tail=True, proto=6, seq=1):
    """One frame as the module's text describes it; bytearray."""
    body = rng.integers(0, 256, max(seglen - 20, 0), dtype=np.uint8).tobytes()
    f = bytearray(tcp_frame(src, dst, sport, dport, body, ihl=ihl, doff=doff, flags=flags, seq=seq,
                            ack=int(rng.integers(0, 1 << 32)), window=int(rng.integers(0, 1 << 16)),
                            ip_id=int(rng.integers(0, 1 << 16)), ttl=int(rng.integers(1, 256)), proto=proto,
                            ip_opts=rng.integers(0, 256, 4 * ihl - 20, dtype=np.uint8).tobytes(), tcp_opts=b"",
                            tot_len=4 * ihl + seglen))
    th = 14 + 4 * ihl
    f[th + 12] |= int(rng.integers(0, 16))                 # the reserved nibble under doff
    if proto == 6:
        tcp_fix(f, ihl, seglen)
    if seglen < 20 and not tail:
        del f[th + seglen:]
    f += rng.integers(1, 256, pad, dtype=np.uint8).tobytes()
    if min60 and len(f) < 60:
        f += rng.integers(1, 256, 60 - len(f), dtype=np.uint8).tobytes()
    return f


def flow_of(rng):
    """(src, dst, sport, dport) of a frame: client or server side of one of COMBOS."""
    idx = int(rng.integers(0, len(COMBOS)))
    c, cp, s, sp = COMBOS[idx]
    if rng.random() < 0.6:
        return c, s, cp, sp
    return s, NAT_IP, sp, 1025 + idx if bound(idx) else 5000 + idx


def eligible_frame():
    """A SYN of the bound flow COMBOS[0], client side, behind 8 bytes of IP options, with 4 of TCP options
    and 21 of payload: looked up by the firewall, translated (SNAT) by the NAT."""
    c, cp, s, sp = COMBOS[0]
    return bytes(wire(np.random.default_rng(SEED + 1), c, s, cp, sp, ihl=7, doff=6, seglen=24 + 21, flags=0x02))


def zero_segment_frame():
    """tot_len 20 with ihl 5: an empty segment, which TCPCalcChecksum accepts because the destination
    address makes the pseudo header sum right; what follows the packet as pad reads as a TCP header with
    doff 0 and SYN.  TCP_OK to the classify pass; the firewall looks it up (its ports lie behind the packet),
    the NAT leaves it to the host.  The one frame whose packet ends at byte 34."""
    c, cp, s, sp = COMBOS[0]
    return bytes(wire(np.random.default_rng(SEED + 2), c, s, cp, sp, ihl=5, doff=0, seglen=0, flags=0x02, min60=True))


def pack(frames, lens=None, phases=None):
    """Frame i at the next 16-byte boundary + phases[i]; (buf, off, len), the buffer a multiple of 16 with
    at least 64 zero bytes behind the last frame.  `lens` overrides the frames' own lengths."""
    off, pos, parts = [], 0, []
    for i, f in enumerate(frames):
        o = (pos + 15) // 16 * 16 + (int(phases[i]) if phases is not None else (2, 7, 0, 13, 1, 11)[i % 6])
        parts.append(b"\0" * (o - pos) + bytes(f))
        off.append(o)
        pos = o + len(f)
    parts.append(b"\0" * ((pos + 64 + 15) // 16 * 16 - pos))
    buf = np.frombuffer(b"".join(parts), np.uint8).copy()
    ln = [len(f) for f in frames] if lens is None else lens
    return buf, np.array(off, np.uint32), np.array(ln, np.uint16)


def classify(buf, off, ln):
    return O.classify(buf, off, ln, O.params(**PARAMS))


def generate(n=N):
    """(frames, lens, phases, meta): the hostile frames, their len[] values, their offsets mod 16, and what
    was drawn for each (ihl, doff, seglen, pad, flags, damage: index into DAMAGE or -1)."""
    rng = np.random.default_rng(SEED)
    frames, lens, meta = [], [], []
    nd = 0
    flag_perm = None
    for i in range(n):
        if i % T == 0:
            flag_perm = rng.permutation(256)
        flags = int(flag_perm[i % T])
        tile = i // T
        if tile in (1, 2) and (flags & 0x12) == 0x02:
            flags |= 0x10
        ihl, doff = int(rng.integers(5, 16)), int(rng.integers(0, 16))
        dmg = i % 5 == 2 and i != LONE_SYN
        plain = dmg or i in (LONE_SYN, 1024)          # a well-formed frame: the damage alone decides
        if plain:
            doff = max(doff, 5)
        opt = int(rng.choice(len(SEGLENS), p=SEG_WEIGHTS)) if not plain else int(rng.integers(8, 11))
        odd, even = 1 + 2 * int(rng.integers(0, 20)), 2 + 2 * int(rng.integers(0, 20))
        seglen = max([0, 4, 12, 16, 19, 20, 21, 4 * doff - 1, 4 * doff, 4 * doff + odd, 4 * doff + even][opt], 0)
        pad, min60, tail = int(rng.integers(0, 8)), bool(rng.random() < 0.5), bool(rng.random() < 0.5)
        tail = tail or tile in (1, 2)                 # (random pad in the flags' place could read as a SYN)
        src, dst, sp, dp = flow_of(rng)
        if i in (LONE_SYN, 1024):
            (src, sp, dst, dp), flags = COMBOS[3 if i == 1024 else 5], 0x02
            assert bound(3) and not bound(5)
        kind = -1
        if dmg:
            kind = nd % len(DAMAGE)
            nd += 1
        d = DAMAGE[kind] if dmg else ("",)
        proto = 17 if d[0] == "udp" else 6
        f = wire(rng, src, dst, sp, dp, ihl, doff, seglen, flags, pad, min60, tail, proto=proto, seq=i)
        ln = len(f)
        if d[0] == "bad_ip":
            f[24] ^= 0x5A
        elif d[0] == "bad_tcp":
            f[14 + 4 * ihl + 16] ^= 0x01                 # (a plain frame: the segment holds its check word)
        elif d[0] == "version5":
            f[14] = 0x50 | ihl
            ip_fix(f, ihl)
        elif d[0] == "tot_len":
            struct.pack_into("!H", f, 16, {"0": 0, "19": 19, "capture-13": ln - 13}[d[1]])
            ip_fix(f, ihl)
        elif d[0] == "len":
            ln = {"33": 33, "34": 34, "14+4*ihl+11": 14 + 4 * ihl + 11, "14+4*ihl+19": 14 + 4 * ihl + 19,
                  "14+tot_len-1": 14 + 4 * ihl + seglen - 1}[d[1]]
        elif d[0] == "arp":
            f[12:14] = b"\x08\x06"
        elif d[0] == "ethertype":
            f[12:14] = b"\x86\xdd"
        assert ln <= len(f)
        frames.append(bytes(f))
        lens.append(ln)
        meta.append((ihl, doff, seglen, pad, flags, kind))
    phases = rng.integers(0, 16, n)
    m = np.array(meta, np.int64)
    meta = types.SimpleNamespace(ihl=m[:, 0], doff=m[:, 1], seglen=m[:, 2], pad=m[:, 3], flags=m[:, 4], damage=m[:, 5])
    return frames, lens, phases, meta


def batch(n=N):
    """The first n hostile frames packed, with the oracle's records of them:
    .frames .buf .off .ln .rec (16-byte records) .rec8 .meta"""
    if "gen" not in _cache:
        _cache["gen"] = generate(N)
    if n not in _cache:
        frames, lens, phases, meta = _cache["gen"]
        buf, off, ln = pack(frames[:n], lens[:n], phases[:n])
        rec = classify(buf, off, ln)
        _cache[n] = types.SimpleNamespace(frames=frames[:n], buf=buf, off=off, ln=ln, rec=rec, rec8=rec8_of(rec),
                                          meta=types.SimpleNamespace(**{k: v[:n] for k, v in vars(meta).items()}))
    return _cache[n]


def split(ns, starts=None):
    """Slices of the hostile frames, one packed batch (buf, off, len) per entry of ns: consecutive ones, or
    from the given first frames."""
    batch(N)
    frames, lens, phases, _ = _cache["gen"]
    out, lo = [], 0
    for k, n in enumerate(ns):
        lo = lo if starts is None else starts[k]
        assert lo + n <= N
        out.append(pack(frames[lo:lo + n], lens[lo:lo + n], phases[lo:lo + n]))
        lo += n
    return out


# ---- cuts ------------------------------------------------------------------------

def cut_ks(frame, ln=None):
    """Byte counts of a frame at and around which a launch's conditions change."""
    ihl, tot = frame[14] & 0xF, frame[16] * 256 + frame[17]
    ln = len(frame) if ln is None else ln
    return sorted({0, 13, 14, 33, 34, 14 + tot - 1, 14 + tot, ln} | {14 + 4 * ihl + j for j in IHL_J})


def cut_points(frame, off=0, ln=None):
    """The frames_bytes values for a batch whose last frame is `frame` at `off`: off + k for every k of
    cut_ks, each also rounded down and up to 16."""
    out = set()
    for k in cut_ks(frame, ln):
        out |= {off + k, (off + k) // 16 * 16, (off + k + 15) // 16 * 16}
    return sorted(out)


def straddle_phase(frame):
    """The offset mod 16 at which the frame's ports' dword has its source port in one 16-byte block and its
    destination port in the next: a buffer end rounded up to 16 can show one without the other."""
    return (14 - (14 + 4 * (frame[14] & 0xF))) % 16


def end_phase(frame):
    """The offset mod 16 at which the frame's packet ends on a 16-byte line: a buffer that ends with the
    packet shows nothing behind it, one byte more shows the next 16."""
    return -(14 + frame[16] * 256 + frame[17]) % 16


def cut_batch(last, phase=None):
    """257 frames: 255 hostile ones, eligible_frame(), `last`; the last one at `phase` mod 16 (default:
    straddle_phase).  Records of the whole buffer."""
    phase = straddle_phase(last) if phase is None else phase
    key = ("cut", last, phase)
    if key not in _cache:
        h = batch(N)
        frames = h.frames[:T - 1] + [eligible_frame(), last]
        phases = list(_cache["gen"][2][:T]) + [phase]
        buf, off, ln = pack(frames, list(h.ln[:T - 1]) + [len(f) for f in frames[T - 1:]], phases)
        rec = classify(buf, off, ln)
        _cache[key] = types.SimpleNamespace(frames=frames, buf=buf, off=off, ln=ln, rec=rec, rec8=rec8_of(rec))
    return _cache[key]


def len_sweep():
    """Copies of eligible_frame() and of zero_segment_frame(), one per value of cut_ks, each with that value
    as its len; .rec the records of these lens, .rec_whole those of the whole frames."""
    if "sweep" not in _cache:
        frames, lens = [], []
        for f in (eligible_frame(), zero_segment_frame()):
            for k in cut_ks(f):
                frames.append(f)
                lens.append(k)
        phases = np.arange(len(frames)) * 5 % 16
        buf, off, ln = pack(frames, lens, phases)
        whole = np.array([len(f) for f in frames], np.uint16)
        _cache["sweep"] = types.SimpleNamespace(frames=frames, buf=buf, off=off, ln=ln, rec=classify(buf, off, ln),
                                                rec_whole=classify(buf, off, whole), whole=whole)
    return _cache["sweep"]


# ---- binding tables whose longest run wraps ------------------------------------------

def probe_edge_bindings(nslots):
    """Bindings for a table of `nslots` (16 or 256) slots in which the client-side keys of the first k
    bindings (k = 4, resp. 6) hash to one of the last two slots, so that their run wraps past slot 0, and
    every other key sits alone in the slot it hashes to: the run is the table's longest and `probe` is k.
    .flows .bindings .start .k .last (the flow whose client-side key is found at depth k)
    .absent (cli_ip, cli_port, svr_ip, svr_port of a flow without a binding whose key hashes to .start)"""
    key = ("probe", nslots)
    if key in _cache:
        return _cache[key]
    L, mask = mosrx.lib(), nslots - 1
    nbind, k, start = {16: (4, 4, 15), 256: (40, 6, 254)}[nslots]
    assert L.mosrx_nat_slots(nbind) == nslots
    run = {(start + j) & mask for j in range(k)}
    safe = set(range(nslots)) - {(start + j) & mask for j in range(-2, k + 2)}
    used = set()

    def slot(sa, da, sp, dp):
        return L.mosrx_nat_hash(mosrx.ip_raw(sa), mosrx.ip_raw(da), mosrx._htons(sp) | mosrx._htons(dp) << 16) & mask

    def alone(make, first):
        """The first port from `first` on whose key hashes to a safe slot that is still free."""
        for p in range(first, 65535):
            s = slot(*make(p))
            if s in safe and s not in used:
                used.add(s)
                return p
        raise AssertionError("no port found")

    cip, sip, sport = "10.9.9.9", "198.51.100.77", 80
    coll = [p for p in range(1025, 65535) if slot(cip, sip, p, sport) == start][:k + 1]
    assert len(coll) == k + 1
    fl, nport = [], 20000
    for i in range(nbind):
        if i < k:
            c, cp = cip, coll[i]
        else:
            c = f"10.8.{i}.1"
            cp = alone(lambda p: (c, sip, p, sport), 40000)
        nport = alone(lambda p: (sip, NAT_IP, sport, p), nport + 1)
        fl.append((c, cp, sip, sport, nport))
    out = types.SimpleNamespace(flows=fl, bindings=mosrx.nat_bindings(fl, nat_ip=NAT_IP), start=start, k=k, run=run,
                                last=fl[k - 1], absent=(cip, coll[k], sip, sport))
    _cache[key] = out
    return out


def probe_edge_frames(pe):
    """Both sides of every binding of `pe`, the absent key's frame last but one, the last-in-run key's last."""
    fr = []
    for j, (c, cp, s, sp, npt) in enumerate(pe.flows):
        fr.append(tcp_frame(c, s, cp, sp, b"c" * (j % 7), flags=0x18, seq=j))
        fr.append(tcp_frame(s, NAT_IP, sp, npt, b"s" * (j % 5), flags=0x18, seq=j, ihl=5 + j % 11))
    c, cp, s, sp = pe.absent
    fr.append(tcp_frame(c, s, cp, sp, b"absent", flags=0x18))
    c, cp, s, sp, _ = pe.last
    fr.append(tcp_frame(c, s, cp, sp, b"last", flags=0x18, ihl=6))
    return fr


# ---- rule tables --------------------------------------------------------------------

def never(i):
    """A rule no frame of the pools matches."""
    return ("DROP" if i % 2 else "ACCEPT", f"172.{17 + i // 250}.{i % 250}.1", "0.0.0.0", 0, 1 + i % 7)


def rule_sets():
    """name -> ACL_RULE_DTYPE records.
    last_of_full  MOSRX_ACL_MAX_RULES rules, only the last can match
    n257          257 rules: the table's second 256 hold one rule; matches at 100, 255 and 256
    overlap       a later DROP shadowed by an earlier ACCEPT (rules 0, 1), a later ACCEPT shadowed by an
                  earlier DROP (rules 2, 3), and a rule that is never reached (4)
    ports         hit depends on which of the ports a lookup saw (the cut tests' set)"""
    if "rules" not in _cache:
        full = [never(i) for i in range(mosrx.ACL_MAX_RULES - 1)] + [("DROP", "10.0.0.0/8", "0.0.0.0")]
        n257 = [never(i) for i in range(257)]
        n257[100] = ("DROP", "10.1.0.0/16", "0.0.0.0", 0, 80)
        n257[255] = ("ACCEPT", "198.51.100.0/24", "0.0.0.0")
        n257[256] = ("DROP", "10.2.0.0/16", "0.0.0.0")
        overlap = [("ACCEPT", "10.1.1.0/24", "0.0.0.0"), ("DROP", "10.1.0.0/16", "0.0.0.0"),
                   ("DROP", "10.2.2.0/24", "0.0.0.0"), ("ACCEPT", "10.2.0.0/16", "0.0.0.0"),
                   ("ACCEPT", "10.2.2.0/24", "0.0.0.0", 0, 80)]
        ports = [("ACCEPT", "10.1.1.0/24", "0.0.0.0", COMBOS[0][1], COMBOS[0][3]),
                 ("DROP", "10.1.1.0/24", "0.0.0.0", COMBOS[0][1], 0), ("ACCEPT", "10.1.1.0/24", "0.0.0.0", 0, COMBOS[0][3]),
                 ("DROP", "10.0.0.0/8", "0.0.0.0")]
        _cache["rules"] = {k: mosrx.acl_rules(v) for k, v in
                           dict(last_of_full=full, n257=n257, overlap=overlap, ports=ports).items()}
    return _cache["rules"]

