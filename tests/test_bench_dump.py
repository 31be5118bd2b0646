"""bench.py --dump-outputs (CPU): the last timed step's records go out one file
per field, float32 / float64 and exact, in the step's batch order; an output past
the size limit is cut to the same seeded sample of frames in every run."""
import os

import numpy as np

import mosrx


class _Batch:
    """Stands in for a resident batch: hands out the records a step left in it."""

    def __init__(self, rec, rec8=None, match=None):
        self._rec, self._rec8, self._match = rec, rec8, match

    def results(self):
        return self._rec

    def results8(self):
        return self._rec8

    def matches(self):
        return self._match


def _records(n, seed, dtype=mosrx.RESULT_DTYPE):
    rng = np.random.default_rng(seed)
    return np.frombuffer(rng.integers(0, 256, n * dtype.itemsize, dtype=np.uint8).tobytes(), dtype).copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_every_field_exact_in_batch_order(tmp_path):
    import bench
    recs = [_records(1000, 1), _records(777, 2)]
    bench.dump_outputs(str(tmp_path / "o"), "M1500", [_Batch(r) for r in recs])
    got = _load(tmp_path / "o")
    want = np.concatenate(recs)
    assert sorted(got) == sorted(mosrx.RESULT_DTYPE.names)
    for f in mosrx.RESULT_DTYPE.names:
        assert got[f].dtype == (np.float64 if want[f].dtype.itemsize > 2 else np.float32)
        np.testing.assert_array_equal(got[f].astype(want[f].dtype), want[f])


def test_compact_and_fused_rows(tmp_path):
    import bench
    r8 = _records(500, 3, mosrx.RESULT8_DTYPE)
    bench.dump_outputs(str(tmp_path / "c"), "S64_c8", [_Batch(None, rec8=r8)])
    assert sorted(_load(tmp_path / "c")) == sorted(mosrx.RESULT8_DTYPE.names)
    m = np.arange(500, dtype=np.uint32) * 8_000_009
    bench.dump_outputs(str(tmp_path / "f"), "IMIX_cls_bpf_ring", [_Batch(_records(500, 4), match=m)])
    got = _load(tmp_path / "f")
    assert got["match"].dtype == np.float64
    np.testing.assert_array_equal(got["match"].astype(np.uint32), m)


def test_large_output_is_the_same_seeded_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64 << 10)
    rec = _records(20_000, 5)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "M1500", [_Batch(rec[:12_000]), _Batch(rec[12_000:])])
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(v.nbytes for v in a.values()) <= 64 << 10
    idx = a["sample_index"].astype(np.int64)
    assert len(idx) > 1000 and (np.diff(idx) > 0).all() and idx[-1] < len(rec)
    for f in a:
        np.testing.assert_array_equal(a[f], b[f])
    np.testing.assert_array_equal(a["rss"].astype(np.uint32), rec["rss"][idx])
