"""Builders for tests/test_bpf_values.py: BPF program sets whose 32-bit match
mask IS the accumulator (pure Python, no GPU).

The probe.  A set holds 32 programs with the same text; program b ends with
`and #(1 << b); ret a`.  Under MOSRX_BPF_LEN_FRAME every frame is evaluated, so
bit b of a frame's match mask is bit b of A after that text: the mask is A at
full width.  A program that returns 0 early (a load out of range, a division by
X == 0) gives mask 0.

Packing.  Every set is a hipRTC compile on the GPU engines, so one set holds
many operations: after a short prefix each program loads a selector byte of the
frame and walks a `jeq` ladder into one block per operation; every block jumps
to the common tail.  A frame therefore runs exactly one block, the one its
selector names, and carries that block's operands.  MOSRX_BPF_MAX_INSNS (4096
per set) leaves 128 instructions per program.

Three families of sets:
  operand  frames of OP_LEN bytes, a at [14], b at [18], selector at [22];
           prefix `ld [14]; st M[0]; ld [18]; tax`: ALU, jumps, register moves
  st, stx  the same frames; the prefix stores 16 distinct values with bit 31 set
           into all 16 scratch slots (through ST, through STX), block s reads
           slot s back
  load     frames of many lengths, selector at [0], X at [2]; prefix
           `ld [2]; tax`: absolute and indexed packet loads, LEN
"""
import random

import numpy as np

import mosrx

I_ = lambda code, k=0, jt=0, jf=0: (code, jt, jf, k & 0xFFFFFFFF)  # noqa: E731
M32 = 0xFFFFFFFF

# the operand set: both sides of every boundary a 32-bit port gets wrong (24-bit multiplies,
# 5-bit shift counts, bit 15 / bit 31 carries, signed compares and divisions)
E = [0, 1, 2, 3, 7, 31, 32, 33, 63, 0xffff, 0x10000, 0x00ffffff, 0x01000001, 0x7fffffff, 0x80000000,
     0x80000001, 0xfffffffe, 0xffffffff, 0xdeadbeef, 0x12345678]
JUMP_K = [0, 1, 0x7fffffff, 0x80000000, 0xffffffff]     # both sides of the signed / unsigned boundary
ALU = {"add": 0x04, "sub": 0x14, "mul": 0x24, "div": 0x34, "or": 0x44, "and": 0x54, "lsh": 0x64, "rsh": 0x74}
JMP = {"jeq": 0x15, "jgt": 0x25, "jge": 0x35, "jset": 0x45}
TAKEN = 0xAAAA0005                                      # what a taken jump loads; the other arm keeps a
SLOT_VALUE = [0x80000000 + 0x01010101 * t for t in range(16)]

MAX_PROG = 4096 // 32                                   # MOSRX_BPF_MAX_INSNS over 32 programs
OP_LEN, OP_A, OP_B, OP_SEL = 32, 14, 18, 22             # operand frames
LD_X, LD_SEL = 2, 0                                     # load frames
STAGE_B = 141                                           # mosrx_bpf.hip: frame bytes [0, 141) are staged in LDS
LENGTHS = [14, 60, 141, 142, 2047, 2048, 9000]

PREFIX = {
    "operand": [I_(0x20, OP_A), I_(0x02, 0), I_(0x20, OP_B), I_(0x07)],
    "st": [i for t in range(16) for i in (I_(0x00, SLOT_VALUE[t]), I_(0x02, t))],
    "stx": [i for t in range(16) for i in (I_(0x01, SLOT_VALUE[t]), I_(0x03, t))],
    "load": [I_(0x20, LD_X), I_(0x07)],
}
SEL_AT = {"operand": OP_SEL, "st": OP_SEL, "stx": OP_SEL, "load": LD_SEL}


def alu_value(op, a, b):
    """The ALU operation in Python (for choosing operands; the oracle is the reference)."""
    return {"add": (a + b) & M32, "sub": (a - b) & M32, "mul": (a * b) & M32, "div": a // b if b else 0,
            "or": a | b, "and": a & b, "lsh": (a << (b & 31)) & M32, "rsh": a >> (b & 31)}[op]


def trivial(v):
    return v == 0 or v == M32


class Block:
    """One operation: its instructions (entered with the family's prefix done, A
    = the selector) and the frames that select it."""

    def __init__(self, family, name, insns, cases, stat=None):
        self.family, self.name, self.insns, self.stat = family, name, insns, stat
        self.cases = cases        # operand: (a, b); load: (frame length, X)


def _dilute(rng, op, base, draw):
    """Operand pairs beyond `base` so that at most a tenth of the opcode's
    results are 0 or 0xffffffff (AND with 0, shifts to nothing, a / b with a < b
    are most of what E x E gives): dense random operands, seeded."""
    bad = sum(trivial(alu_value(op, a, b)) for a, b in base)
    want = max(0, 10 * bad - len(base)) + 8
    out = []
    while len(out) < want:
        a, b = draw(rng)
        if not (op == "div" and b == 0) and not trivial(alu_value(op, a, b)):
            out.append((a, b))
    return out


def operand_blocks():
    rng = random.Random(0xB9F)
    blocks = []
    pairs = [(a, b) for a in E for b in E]
    for op, code in ALU.items():
        extra = _dilute(rng, op, pairs, lambda r: (r.getrandbits(32), r.getrandbits(32) >> r.randint(0, 31)))
        # DIV|X with X == 0 stays in: the program returns 0 there
        blocks.append(Block("operand", f"{op}_x", [I_(0x60, 0), I_(code | 8)], pairs + extra, stat=code | 8))
        ks = [k for k in E if not (op == "div" and k == 0)]      # DIV|K with k == 0 is rejected at set time
        more = _dilute(rng, op, [(a, k) for k in ks for a in E], lambda r: (r.getrandbits(32), r.choice(ks)))
        for k in ks:
            cases = [(a, 0) for a in E] + [(a, 0) for a, kk in more if kk == k]
            blocks.append(Block("operand", f"{op}_k_{k:x}", [I_(0x60, 0), I_(code, k)], cases, stat=code))
    for name, insns in (("neg", [I_(0x60, 0), I_(0x84)]),
                        ("tax_txa", [I_(0x60, 0), I_(0x07), I_(0x00, 0), I_(0x87)]),
                        ("ld_imm", [I_(0x00, 0x80000001)]),
                        ("ld_imm_ones", [I_(0x00, 0xffffffff)]),
                        ("ldx_imm", [I_(0x01, 0x80000001), I_(0x87)])):
        blocks.append(Block("operand", name, insns, [(a, 0) for a in E]))
    blocks.append(Block("operand", "txa", [I_(0x87)], [(0, b) for b in E]))
    for name, code in JMP.items():
        body = [I_(0x00, TAKEN)]
        blocks.append(Block("operand", f"{name}_x", [I_(0x60, 0), I_(code | 8, 0, 0, 1)] + body,
                            [(a, b) for a in E for b in JUMP_K], stat=code | 8))
        for k in JUMP_K:
            blocks.append(Block("operand", f"{name}_k_{k:x}", [I_(0x60, 0), I_(code, k, 0, 1)] + body,
                                [(a, 0) for a in E], stat=code))
    return blocks


def scratch_blocks():
    one = [(0x12345678, 0x9abcdef0)]
    return ([Block("st", f"ld_mem_{s}", [I_(0x60, s)], one) for s in range(16)] +
            [Block("stx", f"ldx_mem_{s}", [I_(0x61, s), I_(0x87)], one) for s in range(16)])


def _ends(length, lo=5):
    return list(range(length - lo, length + 2))


def reads_before_frame(size, x, k):
    """X + k wraps into the offsets where sfbpf_filter's int bounds check passes
    and it reads before the frame (the comment at mosrx_bpf_check, include/mosrx.h)."""
    s = (x + k) & M32
    return (size == 4 and s >= 0xFFFFFFFC) or (size == 2 and s >= 0xFFFFFFFE)


def load_blocks():
    """Few offsets, many frame lengths: a block is compiled code, a frame is data.
    Every absolute offset k meets frames of k - 1 .. k + 6 bytes, so that it lies
    at len - 6 .. len + 1 of some frame, besides much shorter and longer ones."""
    blocks = []

    def lens(k, more):
        return sorted({n for n in range(k - 1, k + 7) if n >= 14} | set(more))

    # absolute loads: around the LDS stage's end (reads that straddle it, with the frame ending inside
    # the stage, at its edge and beyond); k = 30 inside the stage and k = 2044 in memory, at a frame's
    # end; k = 1000 on shorter and longer frames; the first and last offsets the compiled engines read
    # from registers (the fused window holds frame bytes [2, 94), the standalone kernel 35 dwords)
    for name, code, size, stage_lo in (("ldw", 0x20, 4, 136), ("ldh", 0x28, 2, 138), ("ldb", 0x30, 1, 139),
                                       ("msh", 0xb1, 1, 139)):
        ks = {k: lens(k, [60, 2048]) for k in range(stage_lo, 143)}
        ks[30] = lens(30, [14, 60])
        ks[1000] = lens(1000, [142, 2048, 9000])
        ks[2044] = lens(2044, [142])
        if name in ("ldw", "ldb"):
            for k in (1, 2, 86, 87, 132, 133):
                ks[k] = lens(k, [14, 60, 141])
        for k, ns in sorted(ks.items()):
            insns = [I_(code, k)] + ([I_(0x87)] if name == "msh" else [])
            blocks.append(Block("load", f"{name}_abs_{k}", insns, [(n, 0x01020304) for n in ns], stat=code))
    # indexed loads: X from the frame so that X + k lands on the same edges; k = 14 and 0xFFFFFFF0
    # wrap 2^32 (with the latter, X in 16..80 reads frame byte X - 16)
    targets = {14: [0, 9, 10, 11, 12, 13, 14, 15], 60: [0, 1, 2, 3, 31] + _ends(60) + [64, 1000],
               141: [0, 3] + _ends(141) + [1000], 142: [0, 3, 64] + list(range(135, 145)) + [1000],
               2048: [1000] + _ends(2048)}
    for name, code, size in (("ldw", 0x40, 4), ("ldh", 0x48, 2), ("ldb", 0x50, 1)):
        for k in (0, 14, 0xFFFFFFF0):
            cases = []
            for n, ts in targets.items():
                for t in ts + ([0xFFFFFFF0 - 5, 0xFFFFFFFB] if n == 60 else []):   # sums that stay out of range
                    x = (t - k) & M32
                    if not reads_before_frame(size, x, k):
                        cases.append((n, x))
            blocks.append(Block("load", f"{name}_ind_{k:x}", [I_(code, k)], cases, stat=code))
    blocks.append(Block("load", "ld_len", [I_(0x80)], [(n, 0) for n in LENGTHS], stat=0x80))
    blocks.append(Block("load", "ldx_len", [I_(0x81), I_(0x87)], [(n, 0) for n in LENGTHS], stat=0x81))
    return blocks


# blocks per set: the fused module's hipRTC compile grows faster than the number of far loads
MAX_BLOCKS = {"operand": 255, "st": 255, "stx": 255, "load": 8}


class ValueSet:
    """Up to 128 instructions' worth of blocks of one family, as 32 programs."""

    def __init__(self, family, blocks):
        self.family, self.blocks = family, blocks
        self.programs = [(self.program([I_(0x54, 1 << b), I_(0x16)]), mosrx.BPF_LEN_FRAME) for b in range(32)]
        self.bare = self.program([I_(0x16)])          # the same text ending in `ret a`: returns A itself
        self.frames, self.frame_block = [], []
        rng = np.random.RandomState(len(blocks) * 131 + len(family))
        for sel, blk in enumerate(blocks):
            for case in blk.cases:
                self.frames.append(self._frame(rng, sel, case))
                self.frame_block.append(sel)

    @staticmethod
    def size(family, blocks):
        return len(PREFIX[family]) + 1 + len(blocks) + 1 + sum(len(b.insns) + 1 for b in blocks) + 2

    def program(self, tail):
        pre = PREFIX[self.family] + [I_(0x30, SEL_AT[self.family])]
        n = len(self.blocks)
        starts, pos = [], len(pre) + n + 1
        for blk in self.blocks:
            starts.append(pos)
            pos += len(blk.insns) + 1
        ins = list(pre)
        for sel in range(n):
            ins.append(I_(0x15, sel, starts[sel] - (len(ins) + 1), 0))
        ins.append(I_(0x06, 0))                        # no such selector
        for blk in self.blocks:
            ins += blk.insns
            ins.append(I_(0x05, pos - (len(ins) + 1)))
        ins += tail
        assert len(ins) <= MAX_PROG and all(i[1] < 256 and i[2] < 256 for i in ins)
        return np.array(ins, mosrx.BPF_INSN)

    def _frame(self, rng, sel, case):
        if self.family == "load":
            n, x = case
            f = rng.randint(1, 256, n).astype(np.uint8)      # no zero bytes: a load that reads is not 0
            f[12:14] = (0x88, 0xb5)
            f[LD_X:LD_X + 4] = list(x.to_bytes(4, "big"))
            f[LD_SEL] = sel
        else:
            a, b = case
            f = rng.randint(1, 256, OP_LEN).astype(np.uint8)
            f[:12] = 2
            f[12:14] = (0x88, 0xb5)
            f[OP_A:OP_A + 4] = list(a.to_bytes(4, "big"))
            f[OP_B:OP_B + 4] = list(b.to_bytes(4, "big"))
            f[OP_SEL] = sel
        return f.tobytes()


def pack(blocks):
    """Greedy packing of the blocks, family by family, into as few sets as 128 instructions allow."""
    sets = []
    for family in PREFIX:
        cur = []
        for blk in (b for b in blocks if b.family == family):
            if cur and (ValueSet.size(family, cur + [blk]) > MAX_PROG or len(cur) == MAX_BLOCKS[family]):
                sets.append(ValueSet(family, cur))
                cur = []
            cur.append(blk)
        if cur:
            sets.append(ValueSet(family, cur))
    return sets


_SETS = None


def value_sets():
    global _SETS
    if _SETS is None:
        _SETS = pack(operand_blocks() + scratch_blocks() + load_blocks())
    return _SETS

