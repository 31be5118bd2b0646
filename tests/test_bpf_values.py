"""BPF values at full width: A, X, the scratch slots and the
packet loads of all three GPU engines, bit for bit against the oracle.

The other BPF tests see one bit per program per frame (`ret != 0`).  Here a set
of 32 programs with a common text reads the accumulator out: program b ends
with `and #(1 << b); ret a`, so a frame's match mask is A (tests/bpf_values.py).
The oracle's mo_bpf_filter, pinned to mOS's sfbpf_filter by the golden returns
(test_bpf.py), gives the expected value.  A selector byte in each frame picks one
operation of the set, which keeps the number of sets -- each a hipRTC compile --
small.

What the sets hold: every ALU opcode in its X form over all pairs of
bpf_values.E and in its K form with every k of E against every a (plus dense
random operands, so that at most a tenth of an opcode's results are 0 or all
ones); NEG, TAX, TXA, LD|IMM, LDX|IMM with bit 31 set; the four jumps in both
forms on both sides of the signed boundary, both arms visible as values; all 16
scratch slots through ST / LD|MEM and STX / LDX|MEM; absolute and indexed
loads of every width around the frame end, the interpreter's LDS stage (141
bytes), the compiled engines' register windows and far past both, X + k
wrapping 2^32; LEN on frames of 14 to 9000 bytes.  Every batch is packed at
the four frame-offset phases mod 4, and one has frames_bytes cutting its last
frame.

Measured on the oracle with 25 single-point mutants of mo_bpf_filter (24-bit
multiplies, float and signed division, unmasked and arithmetic shifts, a lost
carry, or as xor, 8 scratch slots, bit 31 dropped in moves, LEN cut to 11
bits, a byte-swapped far halfword load, ...): the match bits of test_bpf.py's
golden and random sets change under 10 of them, the values here under all 25.
"""
import numpy as np
import pytest

import bpf_values as V
import mosrx
import oracle_py as O
from pktlib import pack_frames
from test_bpf import bpf_set, engine  # noqa: F401  (the fixture: both GPU engines, JIT restored after)

SETS = V.value_sets()
SET_IDS = [f"{i}-{s.family}" for i, s in enumerate(SETS)]
PHASES = (0, 1, 2, 3)          # the LDS stage loads from o & ~3

_batches = {}


def batch(si, phase):
    """(buf, off, len, expected A per frame) of set si's frames at a phase; built once."""
    if (si, phase) not in _batches:
        buf, off, ln = pack_frames(SETS[si].frames, align=1, phase=phase)
        _batches[si, phase] = (buf, off, ln, O.bpf_eval(SETS[si].programs, buf, off, ln))
    return _batches[si, phase]


# ---------------------------------------------------------------- CPU: the probe is honest
@pytest.mark.parametrize("si", range(len(SETS)), ids=SET_IDS)
def test_probe_mask_is_the_accumulator(si):
    """The 32 masks put together equal what the same text returns through a bare
    `ret a`, on every frame: the probe reads A, all of it."""
    s = SETS[si]
    buf, off, ln, exp = batch(si, 0)
    for p, _ in s.programs:
        assert mosrx.bpf_check(p) == 0 and O.bpf_validate(p) == 1
    assert sum(len(p) for p, _ in s.programs) <= 4096
    np.testing.assert_array_equal(exp, O.bpf_returns(s.bare, mosrx.BPF_LEN_FRAME, buf, off, ln))
    for phase in PHASES[1:]:
        np.testing.assert_array_equal(batch(si, phase)[3], exp)


def results_by_block():
    """{block name: (block, expected A of each of its frames)}"""
    out = {}
    for si, s in enumerate(SETS):
        exp = batch(si, 0)[3]
        fb = np.asarray(s.frame_block)
        for sel, blk in enumerate(s.blocks):
            assert blk.name not in out
            out[blk.name] = (blk, exp[fb == sel])
    return out


def test_matrix_coverage():
    """What the matrix must hold, so that a later edit cannot hollow it out."""
    res = results_by_block()
    # every opcode sfbpf_filter executes is in some block or prefix (test_bpf.test_fixture_coverage's set)
    executable = {0x06, 0x16, 0x20, 0x28, 0x30, 0x80, 0x81, 0x40, 0x48, 0x50, 0xb1, 0x00, 0x01, 0x60, 0x61,
                  0x02, 0x03, 0x05, 0x25, 0x35, 0x15, 0x45, 0x2d, 0x3d, 0x1d, 0x4d, 0x0c, 0x1c, 0x2c, 0x3c,
                  0x5c, 0x4c, 0x6c, 0x7c, 0x04, 0x14, 0x24, 0x34, 0x54, 0x44, 0x64, 0x74, 0x84, 0x07, 0x87}
    in_blocks = {i[0] for blk, _ in res.values() for i in blk.insns}
    in_text = {int(c) for s in SETS for c in s.programs[0][0]["code"]}
    assert executable - in_text == set()
    assert executable - in_blocks <= {0x06, 0x16, 0x02, 0x03, 0x05, 0x15}   # the frame of every program

    # ALU: both forms over E, k == 0 left out only for DIV|K; at least 90 % of an opcode's results
    # are neither 0 nor all ones
    for op, code in V.ALU.items():
        blk, got = res[f"{op}_x"]
        assert set(blk.cases) >= {(a, b) for a in V.E for b in V.E}
        for form, names in ((code | 8, [f"{op}_x"]),
                            (code, [f"{op}_k_{k:x}" for k in V.E if not (op == "div" and k == 0)])):
            assert len(names) in (1, len(V.E) - (op == "div"))
            allv = np.concatenate([res[n][1] for n in names])
            for n in names[1:] + names[:1]:
                assert {a for a, _ in res[n][0].cases} >= set(V.E) and res[n][0].stat == form
            good = np.count_nonzero((allv != 0) & (allv != 0xFFFFFFFF))
            assert good >= 0.9 * len(allv), (op, hex(form), good, len(allv))
    # division: X == 0 returns 0; 0x80000000 / 0xffffffff (where a signed division traps) is 0
    blk, got = res["div_x"]
    for (a, b), v in zip(blk.cases, got):
        assert v == (a // b if b else 0)
    assert (0x80000000, 0xffffffff) in blk.cases and (0x80000000, 0) in res["div_k_ffffffff"][0].cases

    # jumps: both forms on both sides of the signed boundary, both arms taken
    for name, code in V.JMP.items():
        for form in ([f"{name}_x"], [f"{name}_k_{k:x}" for k in V.JUMP_K]):
            arms = set()
            for n in form:
                blk, got = res[n]
                assert {a for a, _ in blk.cases} >= set(V.JUMP_K)
                taken = got == V.TAKEN
                kept = got == np.array([a for a, _ in blk.cases], np.uint32)
                assert np.all(taken | kept)
                arms |= {"taken"} if taken.any() else set()
                arms |= {"kept"} if kept.any() else set()
            assert arms == {"taken", "kept"}, form
        assert {b for _, b in res[f"{name}_x"][0].cases} == set(V.JUMP_K)

    # register moves with bit 31 set
    assert np.all(res["ld_imm"][1] == 0x80000001) and np.all(res["ldx_imm"][1] == 0x80000001)
    np.testing.assert_array_equal(res["tax_txa"][1], np.array(V.E, np.uint32))
    np.testing.assert_array_equal(res["txa"][1], np.array(V.E, np.uint32))
    np.testing.assert_array_equal(res["neg"][1], (-np.array(V.E, np.int64)).astype(np.uint32))

    # all 16 scratch slots, distinct values with bit 31 set, through both store / load pairs
    assert len(set(V.SLOT_VALUE)) == 16 and all(v >> 31 for v in V.SLOT_VALUE)
    for s in range(16):
        assert res[f"ld_mem_{s}"][1].tolist() == [V.SLOT_VALUE[s]]
        assert res[f"ldx_mem_{s}"][1].tolist() == [V.SLOT_VALUE[s]]

    # loads: every width, absolute and indexed, reads on both sides of the frame end, of the LDS
    # stage's end and at k = 1000; no case where the reference reads before the frame
    for kind, size in (("ldw", 4), ("ldh", 2), ("ldb", 1), ("msh", 1)):
        ks = {int(n.rsplit("_", 1)[1]) for n in res if n.startswith(f"{kind}_abs_")}
        assert ks >= set(range(V.STAGE_B - size - 1, V.STAGE_B + 2)) | {1000}
        rel = set()                                        # k - frame length over the absolute cases
        for k in ks:
            blk, got = res[f"{kind}_abs_{k}"]
            rel |= {k - n for n, _ in blk.cases}
            for (n, _), v in zip(blk.cases, got):
                assert (v != 0) == (k + size <= n) or kind == "msh", (blk.name, n)   # (a nibble may be 0)
        assert rel >= set(range(-5, 2))
        lens_at_1000 = {n for n, _ in res[f"{kind}_abs_1000"][0].cases}
        assert min(lens_at_1000) < 1000 < max(lens_at_1000)
    for kind, size in (("ldw", 4), ("ldh", 2), ("ldb", 1)):
        for k in (0, 14, 0xFFFFFFF0):
            blk, got = res[f"{kind}_ind_{k:x}"]
            sums = {(x + k) & 0xFFFFFFFF for _, x in blk.cases}
            assert not any(V.reads_before_frame(size, x, k) for _, x in blk.cases)
            assert k == 0 or any(x + k >= 1 << 32 for _, x in blk.cases)             # X + k wraps 2^32
            assert sums >= set(range(V.STAGE_B - size - 1, V.STAGE_B + 2)) | {1000}
            assert {s - n for (n, x), s in zip(blk.cases, [(x + k) & 0xFFFFFFFF for _, x in blk.cases])} \
                >= set(range(-5, 2))
            inside = np.array([((x + k) & 0xFFFFFFFF) + size <= n for n, x in blk.cases])
            assert not got[~inside].any() and np.count_nonzero(got[inside]) >= 0.8 * inside.sum() > 0   # (the X field holds zero bytes)
            assert 0.25 < inside.mean() < 0.75
    blk, got = res["ldb_ind_fffffff0"]                     # X in 16..80 reads frame byte X - 16
    assert {x for _, x in blk.cases} >= {16, 17, 18, 19, 47, 80}
    for name in ("ld_len", "ldx_len"):
        assert res[name][1].tolist() == V.LENGTHS == [14, 60, 141, 142, 2047, 2048, 9000]


@pytest.mark.parametrize("si", range(len(SETS)), ids=SET_IDS)
def test_value_sets_compile(si):
    """Every set becomes gfx950 code through hipRTC, standalone and fused (compile only, no GPU)."""
    ps = SETS[si].programs
    rc, size, log = mosrx.bpf_jit_compile(ps)
    assert rc == 0 and size > 0, log
    rc, size, log = mosrx.bpf_jit_compile_fused(ps)
    assert rc == 0 and size > 0, log


# ---------------------------------------------------------------- GPU: three engines, full width
def check_all_entry_points(ctx, eng, ps, buf, off, ln, exp, fb=None):
    """bpf_host, bpf_dev and the fused classify + BPF launch (compiled hook on the
    JIT engine, the interpreter behind classify otherwise): A on every frame, and
    the fused records still the oracle's."""
    fb = len(buf) if fb is None else fb
    assert ctx.bpf_fused() == (eng == mosrx.BPF_ENGINE_JIT), ctx.bpf_jit_log()
    got = ctx.bpf_host(buf, off, ln, frames_bytes=fb)
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), ("bpf_host", bad[:5], [hex(int(v)) for v in got[bad[:5]]], [hex(int(v)) for v in exp[bad[:5]]])
    db = ctx.upload(buf, off, ln, frames_bytes=fb)
    ctx.bpf_dev(db)
    np.testing.assert_array_equal(db.matches(), exp, err_msg="bpf_dev")
    db.free()
    db = ctx.upload(buf, off, ln, frames_bytes=fb)
    ctx.classify_bpf_dev(db)
    rec, got = db.results(), db.matches()
    db.free()
    bad = np.nonzero(got != exp)[0]
    assert not len(bad), ("classify_bpf_dev", bad[:5], [hex(int(v)) for v in got[bad[:5]]],
                          [hex(int(v)) for v in exp[bad[:5]]])
    ora = O.classify(buf[:fb], off, ln, O.params())
    assert np.array_equal(rec.view(np.uint8), ora.view(np.uint8)), "records differ from the oracle"


@pytest.mark.gpu
@pytest.mark.parametrize("si", range(len(SETS)), ids=SET_IDS)
def test_bpf_values(gpu_ctx, engine, si):  # noqa: F811
    gpu_ctx.set_params(mosrx.default_params())
    bpf_set(gpu_ctx, engine, SETS[si].programs)
    for phase in PHASES:
        buf, off, ln, exp = batch(si, phase)
        check_all_entry_points(gpu_ctx, engine, SETS[si].programs, buf, off, ln, exp)


@pytest.mark.gpu
def test_bpf_values_truncated_last_frame(gpu_ctx, engine):  # noqa: F811
    """frames_bytes cuts the last frame: loads past the cut return 0, as the
    oracle on buf[:frames_bytes] says (and loads before it still read)."""
    si = next(i for i, s in enumerate(SETS) if any(b.name == "ldw_abs_137" for b in s.blocks))
    s = SETS[si]
    gpu_ctx.set_params(mosrx.default_params())
    bpf_set(gpu_ctx, engine, s.programs)
    last = [i for i, (f, sel) in enumerate(zip(s.frames, s.frame_block))
            if len(f) == 142 and s.blocks[sel].name.split("_")[1] == "abs"]
    assert len(last) >= 8
    seen = set()
    for j, i in enumerate(last):
        frames = s.frames[:i] + s.frames[i + 1:] + [s.frames[i]]
        buf, off, ln = pack_frames(frames, align=1, phase=j % 4)
        fb = int(off[-1]) + 142 - (1 + j % 6)
        exp = O.bpf_eval(s.programs, buf[:fb], off, ln)
        seen.add(bool(exp[-1]))
        check_all_entry_points(gpu_ctx, engine, s.programs, buf, off, ln, exp, fb=fb)
    assert seen == {False, True}
