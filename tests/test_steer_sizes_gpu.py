"""Queue steering at the batch sizes it is timed at: the branches of
mosrx_steer_scan_kernel and of the queue forms' batch lookup that the other
steer tests cannot enter, because no batch of theirs has more than four tiles
and no queue more than eight batches.

With T = mosrx_steer_tile() the scan kernel gives each of its 4 x 256 lanes
per = ceil(tiles / 4) tiles of a column:

    n        tiles  per  segments own
    4T + 1     5     2   2, 2, 1, 0 tiles
    5T         5     2   2, 2, 1, 0 tiles, the last tile full
    9T + 1    10     3   3, 3, 3, 1
    16T + 3   17     5   5, 5, 5, 2
    32T       32     8   8, 8, 8, 8     (MOSRX_STEER_ONE_MAX)

so its loops make more than one trip, `before` sums segments of several tiles
and the split is uneven with per >= 2.  Expected values are test_steer_gpu.py's,
compared exactly and never against another GPU run:

    idx    == argsort(queue, kind="stable")
    qstart == [0] + cumsum(bincount(queue, 256))
    gathered arrays == src[idx]

Every output sits in a sentinel-guarded buffer."""
import numpy as np
import pytest

import mosrx
import oracle_py as O
from test_steer_gather_gpu import _sub
from test_steer_gpu import QS, SENT, Guarded, expect, keys_of, tile
from test_steer_one_gpu import MAX, check_form, run_form
from test_steer_side_gpu import ARRAYS, synthetic

pytestmark = pytest.mark.gpu

RUN = 700   # the `runs` pattern's run length: no divisor of the tile, so runs cross tile edges
FORMS3 = [("plain", False, ()), ("gather", True, ()), ("side", True, ARRAYS)]


def big_sizes():
    T = tile()
    return [4 * T + 1, 5 * T, 9 * T + 1, 16 * T + 3, 32 * T]


def segments(n):
    """The tiles each of the scan kernel's four segments owns (its own formulas)."""
    tiles = -(-n // tile())
    per = -(-tiles // 4)
    return [min(g * per + per, tiles) - min(g * per, tiles) for g in range(4)]


def keys(pattern, n, rng):
    if pattern == "runs":     # every tile has another histogram: a base from the wrong tile or segment cannot cancel out
        return ((np.arange(n) // RUN) % 256).astype(np.uint8)
    return keys_of(pattern, n, rng)


def make(ctx, rng, pattern, n, rb):
    """test_steer_side_gpu.synthetic with this file's key patterns."""
    h, d = synthetic(ctx, rng, "one", n, rb)
    h["key"] = keys(pattern, n, rng)
    h["rec"][:, rb - 3] = h["key"]
    d["rec"].upload(h["rec"])
    return h, d


def test_sizes_reach_the_branches():
    T = tile()
    assert MAX == 32 * T and T % RUN != 0
    assert [segments(n) for n in big_sizes()] == [[2, 2, 1, 0], [2, 2, 1, 0], [3, 3, 3, 1], [5, 5, 5, 2], [8, 8, 8, 8]]
    k = keys("runs", 5 * T, None)
    hists = {np.bincount(k[i * T:(i + 1) * T], minlength=256).tobytes() for i in range(5)}
    assert len(hists) == 5


@pytest.mark.parametrize("rb", [8, 16])
@pytest.mark.parametrize("pattern", ["random", "mod256", "one", "runs"])
def test_steer_sizes_synthetic(gpu_ctx, rb, pattern):
    """mosrx_steer_dev at every size; the gather and side forms (all three side
    arrays) at 9T + 1 and 16T + 3; all through the three launches (limit 0, the
    count of fused launches does not move).  Then the one-launch kernel in its
    three forms at 16T + 3 and 32T with the limit at MOSRX_STEER_ONE_MAX."""
    T = tile()
    rng = np.random.default_rng(8642 + rb)
    try:
        for n in big_sizes():
            h, d = make(gpu_ctx, rng, pattern, n, rb)
            try:
                gpu_ctx.set_steer_one(0)
                forms = FORMS3 if n in (9 * T + 1, 16 * T + 3) else FORMS3[:1]
                for form, descs, which in forms:
                    out = run_form(gpu_ctx, d, n, rb, form, descs, which)
                    assert out[-1] == 0, f"a fused launch with the limit at 0 ({form}, n={n})"
                    check_form(h, n, rb, out, form, descs, which, f"(three launches, {form}, n={n})")
                if n in (16 * T + 3, 32 * T):
                    gpu_ctx.set_steer_one(MAX)
                    for form, descs, which in FORMS3:
                        out = run_form(gpu_ctx, d, n, rb, form, descs, which)
                        assert out[-1] == 1, f"steer_one_count grew by {out[-1]} ({form}, n={n})"
                        check_form(h, n, rb, out, form, descs, which, f"(one launch, {form}, n={n})")
            finally:
                for b in d.values():
                    b.free()
    finally:
        gpu_ctx.set_steer_one(0)


def queue_sizes():
    """40 batches: empty ones first, in the middle and last, tile edges, two
    batches on the per >= 2 path behind a non-zero tile_base, then small ones.
    Unequal tile counts (the classify launch's tpb == 0 path) and a batch lookup
    of 6 steps (ceil(log2 40)) where the other tests make 3."""
    T = tile()
    ns = [0, 1, 63, T - 1, 4 * T + 1, 0, T + 1, 9 * T + 1, 0] + [1 + (i * 53) % 300 for i in range(30)] + [0]
    assert len(ns) == 40 and all(1 <= n <= 300 for n in ns[9:39])
    return ns


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("trace", ["S64", "IMIX"])
def test_queue_of_40_batches(gpu_ctx, trace, compact):
    """set_steer, then set_steer_gather on the same queue; per batch idx, qstart
    and the gathered records, off and len are the oracle's.  S64 is the timed
    64-byte row: one flow, every frame on one queue, every tile's count in one
    column.  IMIX with 3000 flows fills all 8 queues, differently in every tile.
    An empty batch's buffers all keep their sentinel (the library gives it no
    outputs, as test_queue_steer_gather and test_steer_one_queue pin)."""
    ns = queue_sizes()
    rb = 8 if compact else 16
    t = mosrx.Trace(getattr(mosrx, "TRACE_" + trace), sum(ns), nflows=3000, seed=40)
    los = np.concatenate([[0], np.cumsum(ns)]).astype(int)
    subs = [_sub(t, int(lo), n) for lo, n in zip(los, ns)]
    oras = [O.classify(fr, o, ln, O.params(num_queues=8)) if n else None for (fr, o, ln, fb), n in zip(subs, ns)]
    big = [i for i, n in enumerate(ns) if segments(n)[0] >= 2]
    assert len(big) == 2 and all(len(np.unique(oras[i]["queue"])) == (1 if trace == "S64" else 8) for i in big)
    dbs, bufs, q = [], [], None
    try:
        gpu_ctx.set_steer_one(0)
        gpu_ctx.set_params(mosrx.default_params(num_queues=8))
        for fr, o, ln, fb in subs:
            dbs.append(gpu_ctx.upload(fr, o, ln, frames_bytes=fb, hint=None))
        q = gpu_ctx.queue_ex(dbs, compact=compact)
        q.run()
        plain = [(d.results8() if compact else d.results()).tobytes() for d in dbs]
        groups = [[Guarded(gpu_ctx, f(n)) for n in ns] for f in
                  (lambda n: 4 * n, lambda n: 4 * QS, lambda n: rb * n, lambda n: 4 * n, lambda n: 2 * n)]
        idxs, qss, qrs, qos, qls = groups
        bufs = [g for gs in groups for g in gs]
        ptrs = [[g.ptr for g in gs] for gs in groups]
        for form in ("steer", "gather"):
            for g in bufs:
                g.fill()
            if form == "steer":
                q.set_steer(ptrs[0], ptrs[1])
            else:
                q.set_steer_gather(*ptrs)
            q.run()
            recs = [d.results8() if compact else d.results() for d in dbs]
            assert [r.tobytes() for r in recs] == plain
            for i, n in enumerate(ns):
                msg = f"{form} batch {i} (n={n})"
                if n == 0:
                    for gs in groups:
                        assert (gs[i].read(np.uint8) == SENT).all(), f"an empty batch wrote outputs, {msg}"
                    continue
                fr, o, ln, fb = subs[i]
                np.testing.assert_array_equal(recs[i]["queue"], oras[i]["queue"], err_msg=msg)
                eidx, eqs = expect(oras[i]["queue"])
                np.testing.assert_array_equal(qss[i].read(), eqs, err_msg=msg)
                np.testing.assert_array_equal(idxs[i].read(), eidx, err_msg=msg)
                if form == "steer":
                    for gs in (qrs, qos, qls):
                        assert (gs[i].read(np.uint8) == SENT).all(), f"gather outputs written, {msg}"
                    continue
                want = recs[i].view(np.uint8).reshape(n, rb)[eidx]
                np.testing.assert_array_equal(qrs[i].read(np.uint8).reshape(n, rb), want, err_msg=msg)
                np.testing.assert_array_equal(qos[i].read(np.uint32), o[eidx], err_msg=msg)
                np.testing.assert_array_equal(qls[i].read(np.uint16), ln[eidx], err_msg=msg)
    finally:
        gpu_ctx.set_params(mosrx.default_params())
        if q is not None:
            q.destroy()
        for g in bufs:
            g.free()
        for d in dbs:
            d.free()
