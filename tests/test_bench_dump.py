"""bench.py --dump-outputs: what the timed path computed in its last step, as .npy files of float32 / float64 within 64 MB, the
same entries from one run to the next.  A stand-in batch with the accessors of quasimodo_amd.Batch, so nothing here needs a GPU;
the GPU run of the same option is in test_gpu_shards.py."""
import numpy as np

import bench


class FakeBatch:
    def __init__(self, n_vcf, n, n_bins=256, seed=1):
        rng = np.random.default_rng(seed)
        self.n_vcf, self.n_bins = n_vcf, n_bins
        self.n_records = np.full(n_vcf, n, np.int64)
        self._cls = [rng.integers(0, 4, n).astype(np.uint8) for _ in range(n_vcf)]
        self._scal = np.zeros((n_vcf, 8), np.int64)
        self._scal[:, 1] = [int((c == 3).sum()) for c in self._cls]
        self._scal[:, 2] = [int((c == 1).sum()) for c in self._cls]
        self._roc = rng.integers(0, n, (n_vcf, 3, n_bins)).astype(np.uint64)

    def scalars(self):
        return self._scal.copy()

    def roc(self):
        return self._roc.copy()

    def cls(self, v):
        return self._cls[v].copy()

    def idx(self, v):
        c, n = self._cls[v], int(self.n_records[v])
        out = np.full(n, 12345, np.int32)          # what lies between the two lists is left undefined by the library
        tp, fp = np.nonzero(c == 3)[0], np.nonzero(c == 1)[0]
        out[:len(tp)] = tp
        out[n - len(fp):] = fp
        return out


def _load(d):
    import os
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_output_exactly_and_the_same_twice(tmp_path):
    b = FakeBatch(6, 5000)
    glob = np.arange(2 * 3 * 256, dtype=np.int64).reshape(2, 3, 256) * 100_000     # beyond 2^24: float64
    bench.dump_outputs(b, glob, str(tmp_path / "a"))
    bench.dump_outputs(b, glob, str(tmp_path / "b"))
    a, a2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["cls", "global_counts", "idx", "record_slots", "record_vcfs", "roc", "roc_vcfs", "scalars"]
    assert all(np.array_equal(a[k], a2[k]) for k in a)
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert a["global_counts"].dtype == np.float64 and np.array_equal(a["global_counts"], glob)
    assert a["roc"].dtype == np.float32 and np.array_equal(a["roc"], b.roc()) and np.array_equal(a["scalars"], b.scalars())
    assert a["cls"].shape == (4, 5000) and np.array_equal(a["record_slots"], np.arange(5000))
    for i, v in enumerate(a["record_vcfs"].astype(int)):
        assert np.array_equal(a["cls"][i], b.cls(v))
        tp, fp = b.scalars()[v, 1], b.scalars()[v, 2]
        want = b.idx(v).astype(np.int64)
        want[tp:5000 - fp] = -1
        assert np.array_equal(a["idx"][i], want)


def test_dump_of_large_vcfs_keeps_to_64_mb_with_a_fixed_sample(tmp_path):
    b = FakeBatch(5, 3_000_000)
    bench.dump_outputs(b, np.zeros((1, 3, 256), np.int64), str(tmp_path / "a"))
    bench.dump_outputs(b, np.zeros((1, 3, 256), np.int64), str(tmp_path / "b"))
    a, a2 = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert all(np.array_equal(a[k], a2[k]) for k in a)
    slots = a["record_slots"].astype(np.int64)
    assert 0 < len(slots) < 3_000_000 and (np.diff(slots) > 0).all()
    v = int(a["record_vcfs"][0])
    assert np.array_equal(a["cls"][0], b.cls(v)[slots])
