"""Parity tests proper: the HIP engine (through the C ABI) against the oracle on the same
seeded inputs, and end to end against the reference's golden bytes.  Needs an MI355X."""
import os
import warnings

import numpy as np
import pytest

from conftest import case_id, golden_cases, random_columns, random_truth, read_case

pytestmark = pytest.mark.gpu
CASES = golden_cases()


def check_vcf(oracle, res, cols, truth, n_bins=256, expect_sorted=None):
    cls, roc, sc = oracle.classify_columns(*cols, *truth, n_bins=n_bins)
    assert np.array_equal(res["cls"], cls)
    assert np.array_equal(res["roc"], roc)
    s = res["scalars"]
    for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "truth_unique"):
        assert s[k] == sc[k], (k, s[k], sc[k])
    assert s["n_records"] == len(cols[0])
    if expect_sorted is not None:
        assert s["sorted"] == int(expect_sorted)
    # compacted line-index lists: ascending, exactly the TP / FP lines
    assert np.array_equal(res["tp_idx"], np.nonzero(cls == 3)[0])
    assert np.array_equal(res["fp_idx"], np.nonzero(cls == 1)[0])
    # pinned point of the ROC
    if n_bins > 20:
        assert int(res["roc"][0, 20]) == s["tp_lines"] and int(res["roc"][1, 20]) == s["fp_lines"]


SIZES = [0, 1, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 5000, 16384, 16385, 40000]


@pytest.mark.parametrize("seed", [0, 1])
def test_ragged_sorted_batch(engine, oracle, seed):
    rng = np.random.default_rng(100 + seed)
    L = 60000
    truths = [random_truth(rng, 4000, L), random_truth(rng, 300, L)]
    tids = [engine.truth_load(*t) for t in truths]
    cols, which = [], []
    for i, n in enumerate(SIZES):
        w = i % 2
        cols.append(random_columns(rng, n, L, truths[w], sorted_=True))
        which.append(w)
    res, glob = engine.classify_batch(cols, [tids[w] for w in which])
    for r, c, w in zip(res, cols, which):
        check_vcf(oracle, r, c, truths[w], expect_sorted=True)
    # the single-call entry point (qm_classify_batch on concatenated host buffers) agrees
    res1, glob1 = engine.classify_batch_oneshot(cols, [tids[w] for w in which])
    assert np.array_equal(glob, glob1)
    for a, b in zip(res, res1):
        assert a["scalars"] == b["scalars"] and all(np.array_equal(a[k], b[k]) for k in ("cls", "roc", "tp_idx", "fp_idx"))
    # per-truth sums = sum of the ROC rows of the VCFs that use that truth set
    for w in range(2):
        want = sum((r["roc"] for r, ww in zip(res, which) if ww == w), np.zeros((3, 256), np.uint64))
        assert np.array_equal(glob[tids[w]], want)


def test_ragged_batch_run_twice_with_timing_gives_the_same_answers(engine, oracle):
    """qm_batch_run queues the compaction on the main stream and the rows' k_finalize on the context's second stream.  A small
    ragged batch (empty and one-record VCFs, sizes either side of the bucket path's 16 384), sorted and unsorted VCFs mixed,
    run twice back to back with timing on, agrees with the oracle."""
    rng = np.random.default_rng(502)
    L = 90000
    truth = random_truth(rng, 3000, L)
    tid = engine.truth_load(*truth)
    sizes = [20000, 1, 0, 40000, 333, 17000, 5, 70000, 2048, 16384, 16385, 900]
    cols = [random_columns(rng, n, L, truth, sorted_=(i % 5 != 3)) for i, n in enumerate(sizes)]
    b = engine.batch(sizes, [tid] * len(sizes))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.set_timing(True)
    for _ in range(2):
        b.run()
    b.finish()
    tm = b.timings()
    assert tm["total_ms"] > 0 and tm["classify_ms"] > 0 and tm["compact_ms"] > 0
    roc, scal = b.roc(), b.scalars()
    for v, c in enumerate(cols):
        cls, oroc, sc = oracle.classify_columns(*c, *truth)
        assert np.array_equal(b.cls(v), cls) and np.array_equal(roc[v], oroc)
        assert scal[v][1] == sc["tp_lines"] and scal[v][3] == sc["TP_R"] and scal[v][4] == sc["FP_R"]
        idx = b.idx(v)
        assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0])
        assert np.array_equal(idx[len(c[0]) - sc["fp_lines"]:], np.nonzero(cls == 1)[0])
    assert np.array_equal(b.global_counts()[tid], roc.sum(axis=0))
    b.close()
    engine.truth_release(tid)


def test_unsorted_vcfs_take_the_radix_sort_path(engine, oracle):
    rng = np.random.default_rng(7)
    L = 200000
    truth = random_truth(rng, 5000, L)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, L, truth, sorted_=s) for n, s in
            ((3000, False), (10, False), (5000, True), (2, False), (70000, False), (2048, False), (1, False))]
    res, glob = engine.classify_batch(cols, [tid] * len(cols))
    for r, c in zip(res, cols):
        srt = bool(np.all(np.diff(c[0].astype(np.int64)) >= 0))
        check_vcf(oracle, r, c, truth, expect_sorted=srt)
    want = sum((r["roc"] for r in res), np.zeros((3, 256), np.uint64))
    assert np.array_equal(glob[tid], want)


def test_unsorted_vcfs_too_dense_for_the_bucket_path_fall_back_to_the_radix_sort(engine, oracle):
    """Unsorted VCFs normally take the bucket path (one scatter pass + k_classify_hash).  Buckets that do not fit its LDS
    tables -- here 300 000 records on 16 positions, and a truth set with every allele pair at every position -- flag the
    VCF, and the radix sort redoes it: same answers, many repeated keys."""
    rng = np.random.default_rng(71)
    tpos = np.repeat(np.arange(900, 1300, dtype=np.int32), 16)
    truth = (tpos, np.tile(np.repeat(np.arange(4, dtype=np.int32), 4), 400), np.tile(np.arange(4, dtype=np.int32), 1600))
    tid = engine.truth_load(*truth)
    cols = []
    for n, lo, hi in ((300000, 1000, 1016), (50000, 900, 1300), (9000, 1, 5000)):
        pos = rng.integers(lo, hi, n).astype(np.int32)
        ref = rng.integers(0, 4, n).astype(np.int32)
        alt = rng.integers(0, 4, n).astype(np.int32)
        qual = rng.integers(0, 300, n).astype(np.float32)
        flags = ((qual >= 20).astype(np.uint8) | ((rng.random(n) > 0.1).astype(np.uint8) << 1) | ((rng.random(n) < 0.01).astype(np.uint8) << 2)).astype(np.uint8)
        cols.append((pos, ref, alt, qual, flags))
    res, glob = engine.classify_batch(cols, [tid] * len(cols))
    for r, c in zip(res, cols):
        check_vcf(oracle, r, c, truth, expect_sorted=False)
    assert np.array_equal(glob[tid], sum((r["roc"] for r in res), np.zeros((3, 256), np.uint64)))
    engine.truth_release(tid)


def test_long_equal_position_runs_across_tiles(engine, oracle):
    """Runs of one position longer than a tile: ownership of the truth entries and the
    R-path de-duplication must not double count across tile and span boundaries."""
    rng = np.random.default_rng(11)
    truth = (np.array([50, 50, 50, 77, 90], np.int32), np.array([0, 0, 1, 2, 3], np.int32), np.array([1, 2, 3, 3, 0], np.int32))
    tid = engine.truth_load(*truth)
    n = 9000
    pos = np.concatenate([np.full(20, 10), np.full(n, 50), np.full(2048 * 9, 77), np.full(5, 90), np.full(3, 95)]).astype(np.int32)
    N = len(pos)
    ref = rng.integers(0, 4, N).astype(np.int32)
    alt = rng.integers(0, 4, N).astype(np.int32)
    qual = rng.integers(0, 260, N).astype(np.float32)
    flags = (((qual >= 20).astype(np.uint8)) | ((rng.random(N) > 0.1).astype(np.uint8) << 1)).astype(np.uint8)
    cols = (pos, ref, alt, qual, flags)
    res, _ = engine.classify_batch([cols], [tid])
    check_vcf(oracle, res[0], cols, truth, expect_sorted=True)


def test_dense_truth_slices_are_chunked(engine, oracle):
    """Truth slice of one tile larger than the LDS staging capacity (2048 keys)."""
    rng = np.random.default_rng(13)
    L = 40000
    tp = np.repeat(np.arange(1, L + 1, dtype=np.int32), 3)
    truth = (tp, rng.integers(0, 4, len(tp)).astype(np.int32), rng.integers(0, 4, len(tp)).astype(np.int32))
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, 500, L, truth, frac_truth=0.5), random_columns(rng, 6000, L, truth, frac_truth=0.5)]
    res, _ = engine.classify_batch(cols, [tid, tid])
    for r, c in zip(res, cols):
        check_vcf(oracle, r, c, truth)


def test_empty_truth_and_small_bins(engine, oracle):
    rng = np.random.default_rng(17)
    empty = (np.zeros(0, np.int32),) * 3
    tid = engine.truth_load(*empty)
    cols = random_columns(rng, 3000, 5000, empty)
    for nb in (256, 64, 21):
        res, _ = engine.classify_batch([cols], [tid], n_bins=nb)
        check_vcf(oracle, res[0], cols, empty, n_bins=nb)
        # no truth key: the only TP lines are the ones the host path declared (QM_F_TPLINE)
        assert res[0]["scalars"]["tp_lines"] == int(np.count_nonzero((cols[4] & 9) == 9))


def test_position_out_of_range_is_an_error(engine):
    import quasimodo_amd as q
    tid = engine.truth_load(np.array([5], np.int32), np.array([0], np.int32), np.array([1], np.int32))
    cols = (np.array([1, 1 << 28], np.int32), np.zeros(2, np.int32), np.ones(2, np.int32), np.full(2, 50, np.float32),
            np.full(2, 3, np.uint8))
    with pytest.raises(q.QmvtError) as ei:
        engine.classify_batch([cols], [tid])
    assert ei.value.code == -5
    with pytest.raises(q.QmvtError):
        engine.truth_load(np.array([-1], np.int32), np.array([0], np.int32), np.array([1], np.int32))


def test_position_out_of_range_behind_an_unsorted_stretch(engine):
    """The optimistic pass stops streaming a VCF at its first out-of-order tile; a bad position behind it is found by
    the radix-sort path and is the same error."""
    import quasimodo_amd as q
    tid = engine.truth_load(np.array([5], np.int32), np.array([0], np.int32), np.array([1], np.int32))
    n = 40000
    pos = np.arange(n, 0, -1, dtype=np.int32)       # descending: out of order from the first tile on
    pos[-7] = 1 << 28
    cols = (pos, np.zeros(n, np.int32), np.ones(n, np.int32), np.full(n, 50, np.float32), np.full(n, 3, np.uint8))
    with pytest.raises(q.QmvtError) as ei:
        engine.classify_batch([cols], [tid])
    assert ei.value.code == -5


def test_truth_sets_can_be_released_and_batches_keep_their_layout(engine, oracle):
    """qm_truth_release frees a slot for reuse; a batch created against the released set refuses to run; a truth set
    loaded AFTER a batch was created changes neither the size of its per-truth sums nor what it reads back."""
    import quasimodo_amd as q
    rng = np.random.default_rng(31)
    L = 30000
    t1, t2 = random_truth(rng, 900, L), random_truth(rng, 500, L)
    a = engine.truth_load(*t1)
    cols = random_columns(rng, 7000, L, t1)
    b = engine.batch([7000], [a])
    rows = b.n_truth
    b.upload(0, *cols)
    later = [engine.truth_load(*t2) for _ in range(5)]          # the context's truth table grows past the batch's rows
    assert engine.n_truth >= rows + 5 or min(later) < rows      # (released slots of earlier tests may be reused)
    b.run(); b.finish()
    g = b.global_counts()
    assert g.shape[0] == rows and np.array_equal(g[a], b.roc()[0])
    cls, roc, sc = oracle.classify_columns(*cols, *t1)
    assert np.array_equal(b.cls(0), cls) and np.array_equal(b.roc()[0], roc)
    engine.truth_release(a)
    with pytest.raises(q.QmvtError) as ei:
        b.run()
    assert ei.value.code == -6
    again = engine.truth_load(*t1)                                # the slot comes back ...
    assert again == a
    with pytest.raises(q.QmvtError):                              # ... but it is another truth set to the old batch
        b.run()
    b.close()
    for t in later + [again]:
        engine.truth_release(t)
    with pytest.raises(q.QmvtError):
        engine.truth_release(again)


@pytest.mark.parametrize("shuffled", [False, True])
def test_synthetic_batch_vs_oracle(engine, oracle, shuffled):
    """The on-device generator of the bench workload, at a size the oracle finishes in seconds."""
    L, N, T = 400000, 80000, 8000
    tid = engine.truth_synth(L, T, 3)
    b = engine.batch([N, N, N // 2], [tid] * 3)
    b.synth(L, T, 3, 3000, shuffled=shuffled)
    b.run()
    b.finish()
    roc, scal = b.roc(), b.scalars()
    # the truth keys, regenerated through the engine's own columns: every record drawn from
    # the truth is a hit, so recover T' from the scalars and the keys from a dense probe
    tk = None
    for v in range(3):
        cols = b.columns(v)
        if not shuffled:
            assert np.all(np.diff(cols[0]) > 0)           # distinct, sorted positions
        if tk is None:
            from oracle.synth import synth_truth_keys
            tk = synth_truth_keys(L, T, 3)
        cls, oroc, sc = oracle.classify_columns(*cols, *tk)
        assert np.array_equal(b.cls(v), cls)
        assert np.array_equal(roc[v], oroc)
        assert scal[v][0] == sc["n_pass"] and scal[v][3] == sc["TP_R"] and scal[v][4] == sc["FP_R"]
        assert scal[v][5] == (0 if shuffled else 1)
        hit_frac = sc["tp_lines"] / max(sc["n_pass"], 1)
        expect = 0.8 * T / len(cols[0])                      # 80 % of the strata that hold a truth key
        assert 0.9 * expect < hit_frac < 1.3 * expect       # (+ chance matches of the random records)
        idx = b.idx(v)
        n = len(cols[0])
        assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0])
        assert np.array_equal(idx[n - sc["fp_lines"]:], np.nonzero(cls == 1)[0])
    b.close()


@pytest.mark.parametrize("two_level", [False, True])
def test_config3_shape_ten_million_record_vcfs(engine, oracle, monkeypatch, two_level):
    """BASELINE configs[3] shape per VCF: 10 M records on a 50 Mb reference, 1 M truth keys (611 spans,
    9 766 tiles per VCF), sorted and shuffled, against the oracle.  Shuffled, such a VCF is two partitions of 256 WIDE buckets
    (2^17 positions, up to 32 768 records: k_join_lean<.., BIG>) filled by ONE pass of the 512-digit scatter since round 6
    (`bucket_partitions`); a level-1 scatter and a second one from its entries before (`bucket_two_level`, still there behind
    QM_UNSORTED_PATH=two_level and for wider references)."""
    from oracle.synth import synth_truth_keys
    if two_level:
        monkeypatch.setenv("QM_UNSORTED_PATH", "two_level")
    L, N, T = 50_000_000, 10_000_000, 1_000_000
    tid = engine.truth_synth(L, T, 4)
    tk = synth_truth_keys(L, T, 4)
    for shuffled in (False, True):
        b = engine.batch([N, N // 2], [tid, tid])
        b.synth(L, T, 4, 4000, shuffled=shuffled)
        b.run()
        b.finish()
        if shuffled:
            ps = b.path_stats()
            assert ps["unsorted"] == 2 and ps["radix"] == 0 and ps["radix_after_overflow"] == 0, ps
            assert (ps["bucket_two_level"], ps["bucket_partitions"]) == ((2, 0) if two_level else (0, 2)), ps
        roc, scal = b.roc(), b.scalars()
        for v in range(2):
            cols = b.columns(v)
            cls, oroc, sc = oracle.classify_columns(*cols, *tk)
            assert np.array_equal(b.cls(v), cls)
            assert np.array_equal(roc[v], oroc)
            assert [int(x) for x in scal[v][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
            idx = b.idx(v)
            assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0])
            assert np.array_equal(idx[len(cls) - sc["fp_lines"]:], np.nonzero(cls == 1)[0])
        b.close()


@pytest.mark.parametrize("records, truth, path", [(2_000_000, 100_000, "bucket_partitions"), (1_000_000, 100_000, "bucket_hashed"),
                                                 (1_000_000, 1_000_000, "bucket_partitions")])
def test_shuffled_vcfs_on_a_50_mb_reference_by_size_and_truth_density(engine, oracle, records, truth, path):
    """Which buckets a shuffled default-mode VCF of a 50 Mb reference takes: above the one-level path's 1.31 M records the wide
    ones (round 6; two levels before, 2.8e10 /s against 4.3e10); below, the one-level path with the hashed join -- unless the
    truth set is so dense that a one-level bucket (2^18 positions here) would hold more truth keys than that join stages: then
    the wide buckets as well (the chunk used to overflow and take the radix sort).  Against the oracle and the sorted run."""
    from oracle.synth import synth_truth_keys
    L = 50_000_000
    tid = engine.truth_synth(L, truth, 4)
    tk = synth_truth_keys(L, truth, 4)
    res = {}
    for shuffled in (False, True):
        b = engine.batch([records, records], [tid, tid])
        b.synth(L, truth, 4, 4000, shuffled=shuffled)
        b.run()
        b.finish()
        if shuffled:
            ps = b.path_stats()
            assert ps["unsorted"] == 2 and ps["radix"] == 0 and ps["radix_after_overflow"] == 0 and ps["overflow_chunks"] == 0, ps
            assert ps[path] == 2, ps
            cols = b.columns(0)
            cls, oroc, sc = oracle.classify_columns(*cols, *tk)
            assert np.array_equal(b.cls(0), cls)
            assert np.array_equal(b.roc()[0], oroc)
            assert [int(x) for x in b.scalars()[0][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
        res[shuffled] = (b.roc().copy(), np.array(b.scalars())[:, :5].copy())
        b.close()
    assert np.array_equal(res[False][0], res[True][0]) and np.array_equal(res[False][1], res[True][1])


def test_unsorted_vcfs_of_a_wide_reference_take_every_path_in_one_finish(engine, oracle, monkeypatch):
    """One batch on a 40 Mb reference, uploaded columns with everything random_columns knows (repeats, multi-allelic sites,
    keyless records, non-'.' IDs, infinite QUALs): a 1.5 M-record VCF out of order (wide buckets), one of 200 000 (one level,
    hashed join), one of 5 000 (radix sort), a sorted one, and a second 1.5 M-record VCF with 30 % of its records on 3 000
    positions -- its wide buckets overflow, the two levels behind them as well, and the radix sort redoes it, while the other
    large VCF of the same chunk takes the wide buckets again without it (through round 5 a chunk fell back as a whole).  Twice:
    the second run with the batch's memory of the first.  Every VCF against the oracle, the per-truth sums against the VCFs' rows."""
    from conftest import random_columns, random_truth
    from quasimodo_amd.engine import SCALAR_NAMES
    rng = np.random.default_rng(6061)
    L = 40_000_000
    truth = random_truth(rng, 60_000, L)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, L, truth, sorted_=s) for n, s in ((1_500_000, False), (200_000, False), (5_000, False), (300_000, True))]
    pos, ref, alt, qual, flags = random_columns(rng, 1_500_000, L, truth, sorted_=False)
    crowd = rng.random(len(pos)) < 0.3
    pos = np.where(crowd, 20_000_000 + rng.integers(0, 3000, len(pos)), pos).astype(np.int32)
    cols.append((pos, ref, alt, qual, flags))
    b = engine.batch([len(c[0]) for c in cols], [tid] * len(cols))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    for rep in range(2):
        b.run()
        b.finish()
        want = np.zeros((3, 256), np.uint64)
        for v, c in enumerate(cols):
            sc = dict(zip(SCALAR_NAMES, b.scalars()[v].tolist()))
            reg = b.idx(v)
            res = {"cls": b.cls(v), "roc": b.roc()[v], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[len(c[0]) - sc["fp_lines"]:].copy()}
            check_vcf(oracle, res, c, truth, expect_sorted=(v == 3))
            want += res["roc"]
        assert np.array_equal(b.global_counts()[tid], want)
        ps = b.path_stats()
        assert ps["unsorted"] == 4 and ps["bucket_partitions"] == 1 and ps["bucket_hashed"] == 1 and ps["radix"] == 1 and ps["radix_after_overflow"] == 1, (rep, ps)
    b.close()
    engine.truth_release(tid)


def test_wide_buckets_and_positions_above_what_the_optimistic_pass_saw(engine, oracle):
    """test_positions_above_what_the_optimistic_pass_saw for the wide buckets: a 1.5 M-record VCF out of order whose records the
    optimistic pass looks at (the first round of every span, the 64 samples) lie below 2^25 -- one wide partition by that
    estimate -- while a quarter of the others lie between 2^25 and 60 M.  The scatter flags the records beyond the partition,
    the radix sort redoes the VCF and its key OR corrects the estimate: the second run takes two wide partitions."""
    from quasimodo_amd.engine import SCALAR_NAMES
    rng = np.random.default_rng(6062)
    n, span = 1_500_000, 16384
    seen = np.zeros(n, bool)
    for s0 in range(0, n, span):
        seen[s0:s0 + 256] = True
    seen[(np.arange(64) * n) >> 6] = True
    lo = rng.integers(1, 1 << 25, n - n // 4).astype(np.int32)
    hi = rng.integers(1 << 25, 60_000_000, n // 4).astype(np.int32)
    pos = np.empty(n, np.int32)
    pos[seen] = lo[:seen.sum()]
    rest = np.concatenate([lo[seen.sum():], hi])
    rng.shuffle(rest)
    pos[~seen] = rest
    pos[0], pos[1] = (1 << 25) - 1, 5          # the estimate is 2^25 - 1 exactly; the first span is out of order at once
    ref = rng.integers(0, 4, n).astype(np.int32)
    alt = ((ref + 1 + rng.integers(0, 3, n)) & 3).astype(np.int32)
    qual = rng.integers(0, 256, n).astype(np.float32)
    flags = (2 | (qual >= 20)).astype(np.uint8)
    take = rng.random(n) < 0.2
    tp_, tr_, ta_ = pos[take], ref[take], alt[take]
    o = np.lexsort((ta_, tr_, tp_))
    truth = (tp_[o], tr_[o], ta_[o])
    tid = engine.truth_load(*truth)
    cols = (pos, ref, alt, qual, flags)
    b = engine.batch([n], [tid])
    b.upload(0, *cols)
    for rep in range(3):
        b.run()
        b.finish()
        sc = dict(zip(SCALAR_NAMES, b.scalars()[0].tolist()))
        reg = b.idx(0)
        res = {"cls": b.cls(0), "roc": b.roc()[0], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[n - sc["fp_lines"]:].copy()}
        check_vcf(oracle, res, cols, truth, expect_sorted=False)
        ps = b.path_stats()
        assert ps["radix_after_overflow"] == (1 if rep == 0 else 0) and ps["bucket_partitions"] == (0 if rep == 0 else 1), (rep, ps)
    b.close()
    engine.truth_release(tid)


@pytest.mark.parametrize("knobs", [{}, {"QM_SPECULATE": "0"}, {"QM_UNSORTED_PATH": "two_level"}], ids=["queued", "looked-at", "two-levels"])
def test_one_overflowing_vcf_does_not_take_its_chunk_to_the_radix_sort(engine, oracle, monkeypatch, knobs):
    """Five VCFs out of order in ONE chunk of the one-level bucket path, the third of them 60 000 records on sixteen positions: its
    buckets overflow, nothing of the chunk is handed over -- and (round 6) only that VCF goes through the radix sort, the other
    four take the buckets again among themselves.  Both ways a one-level chunk is settled (queued without a look at its flags;
    looked at), and the two levels (QM_UNSORTED_PATH=two_level: the dense VCF's partition is named before anything is scattered)."""
    from conftest import random_columns, random_truth
    from quasimodo_amd.engine import SCALAR_NAMES
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(6065)
    L = 4_000_000 if knobs.get("QM_UNSORTED_PATH") else 400_000   # (the two levels size a partition's buckets for 128 ... 256 of them in use: 4 M positions are 123)
    truth = random_truth(rng, 8000, L)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, L, truth, sorted_=False) for n in (40_000, 33_000)]
    n = 60_000
    pos = rng.integers(1000, 1016, n).astype(np.int32)
    ref = rng.integers(0, 4, n).astype(np.int32)
    alt = rng.integers(0, 4, n).astype(np.int32)
    qual = rng.integers(0, 300, n).astype(np.float32)
    cols.append((pos, ref, alt, qual, ((qual >= 20).astype(np.uint8) | 2).astype(np.uint8)))
    cols += [random_columns(rng, n, L, truth, sorted_=False) for n in (45_000, 38_000)]
    b = engine.batch([len(c[0]) for c in cols], [tid] * len(cols))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    for rep in range(2):
        b.run()
        b.finish()
        want = np.zeros((3, 256), np.uint64)
        for v, c in enumerate(cols):
            sc = dict(zip(SCALAR_NAMES, b.scalars()[v].tolist()))
            reg = b.idx(v)
            res = {"cls": b.cls(v), "roc": b.roc()[v], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[len(c[0]) - sc["fp_lines"]:].copy()}
            check_vcf(oracle, res, c, truth, expect_sorted=False)
            want += res["roc"]
        assert np.array_equal(b.global_counts()[tid], want)   # nothing was added twice
        st = b.path_stats()
        good = "bucket_two_level" if knobs.get("QM_UNSORTED_PATH") else "bucket_direct"
        assert st["unsorted"] == 5 and st["radix_after_overflow"] == 1 and st[good] == 4, (rep, st)
    b.close()
    engine.truth_release(tid)


def test_a_vcf_too_dense_for_any_bucket_goes_to_the_radix_sort_alone(engine, oracle):
    """Three VCFs out of order on 10.6 M positions (a pair of narrow partitions): 150 000 and 570 000 records, and 3.7 M -- 0.35
    records per position, more than the buckets of such a reference hold.  A chunk falls back as a whole, so the dense VCF used
    to take its neighbours to the radix sort with it; the routing now sends it there alone (tools/gpu_fuzz_big.py, round 6)."""
    from conftest import random_columns, random_truth
    from quasimodo_amd.engine import SCALAR_NAMES
    rng = np.random.default_rng(6064)
    L = 10_600_000
    truth = random_truth(rng, 200_000, L)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, L, truth, frac_truth=0.05, sorted_=False, dup_frac=0.01, near_frac=0.01) for n in (150_000, 3_700_000, 570_000)]
    b = engine.batch([len(c[0]) for c in cols], [tid] * 3)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    for rep in range(2):
        b.run()
        b.finish()
        ps = b.path_stats()
        assert ps["unsorted"] == 3 and ps["radix"] == 1 and ps["radix_after_overflow"] == 0 and ps["bucket_partitions"] == 2, (rep, ps)
        for v, c in enumerate(cols):
            sc = dict(zip(SCALAR_NAMES, b.scalars()[v].tolist()))
            reg = b.idx(v)
            res = {"cls": b.cls(v), "roc": b.roc()[v], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[len(c[0]) - sc["fp_lines"]:].copy()}
            check_vcf(oracle, res, c, truth, expect_sorted=False)
    b.close()
    engine.truth_release(tid)


def test_wide_buckets_up_to_the_end_of_their_regions(engine, oracle):
    """A 1 M-record VCF out of order on 67.1 M positions against 400 000 truth keys (too dense for the hashed join: wide
    buckets): two wide partitions whose LAST bucket is in use, sub-regions of 2 048 entries -- half of what a wave pair of the
    wide join covers.  The lanes of the join that have nothing to fetch read their sub-region's first quad (every lane issues
    every load, k_join_lean); in round 6's first form they read the first quad of the wave's HALF, which for such a sub-region
    lies behind it -- for the last bucket's last sub-region behind the allocation: tools/gpu_fuzz_big.py found the fault."""
    from conftest import random_columns, random_truth
    from quasimodo_amd.engine import SCALAR_NAMES
    rng = np.random.default_rng(6063)
    L, n = 67_100_000, 1_000_000
    truth = random_truth(rng, 400_000, L)
    tid = engine.truth_load(*truth)
    cols = random_columns(rng, n, L, truth, frac_truth=0.3, sorted_=False, near_frac=0.02)
    assert int(cols[0].max()) >= 511 * (1 << 17)
    b = engine.batch([n], [tid])
    b.upload(0, *cols)
    for rep in range(2):
        b.run()
        b.finish()
        ps = b.path_stats()
        assert ps["bucket_partitions"] == 1 and ps["radix_after_overflow"] == 0, ps
        sc = dict(zip(SCALAR_NAMES, b.scalars()[0].tolist()))
        reg = b.idx(0)
        res = {"cls": b.cls(0), "roc": b.roc()[0], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[n - sc["fp_lines"]:].copy()}
        check_vcf(oracle, res, cols, truth, expect_sorted=False)
    b.close()
    engine.truth_release(tid)


def test_shuffled_vcfs_above_the_level_one_index_stay_on_buckets(engine, oracle):
    """Two shuffled VCFs of 32 M records: a level-1 entry of the two-level bucket path holds 24 index bits, so a
    VCF above 16.7 M records used to fall onto the radix sort (4x slower).  It is dealt out in runs of 2^24 records now, level-1
    segments of their own whose entries lie one behind the other inside every partition (BucketScatterParams.l1_half): the
    shuffled run equals the sorted one, one VCF also the oracle, nothing takes the radix sort, and the step is timed."""
    import time
    from oracle.synth import synth_truth_keys
    L, N, N2, T = 256_000_000, 32_000_000, 16_000_000, 1_000_000   # 0.125 records per position, 31 partitions of 2^27 keys; the 32 M-record VCFs are two runs of 2^24 records each, the third VCF one
    tid = engine.truth_synth(L, T, 4)
    res = {}
    for shuffled in (False, True):
        b = engine.batch([N, N, N2], [tid, tid, tid])
        b.synth(L, T, 4, 4100, shuffled=shuffled)
        b.run()
        b.finish()
        res[shuffled] = (b.roc(), b.scalars()[:, :5].copy())
        if shuffled:
            ps = b.path_stats()
            assert ps["unsorted"] == 3 and ps["bucket_two_level"] == 3 and ps["radix"] == 0 and ps["radix_after_overflow"] == 0, ps
            t0 = time.perf_counter()
            for _ in range(3):
                b.run(); b.finish()
            rate = 3 * (2 * N + N2) / (time.perf_counter() - t0)
            print("shuffled 10 M-record VCFs: %.3g classifications/s" % rate)
            if rate < 4e10:   # (5.0-5.5e10 measured; the radix sort: 1.5e10)  rates are judged by bench.py: a slow box must not turn a parity run red
                warnings.warn("shuffled 10 M-record VCFs at %.3g classifications/s: below the 4e10 this path has measured (path counters above say which path ran)" % rate)
            cols = b.columns(1)
            cls, oroc, sc = oracle.classify_columns(*cols, *synth_truth_keys(L, T, 4))
            assert np.array_equal(b.cls(1), cls) and np.array_equal(b.roc()[1], oroc)
            assert [int(x) for x in b.scalars()[1][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
            idx = b.idx(1)
            assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0])
            assert np.array_equal(idx[len(cls) - sc["fp_lines"]:], np.nonzero(cls == 1)[0])
        b.close()
    engine.truth_release(tid)
    assert np.array_equal(res[True][0], res[False][0]) and np.array_equal(res[True][1], res[False][1])


def test_config5_shape_mixed_snp_indel_three_truth_sets(engine, oracle):
    """BASELINE configs[4] under the reference's semantics: 70 % SNP / 30 % indel records, three truth sets
    (VCF v uses truth v mod 3).  The reference drops every indel at the A2 filter
    (extract_TP_FP_SNPs.py:24), so records whose alleles are not single bases are neither kept nor matched;
    matching variable-length alleles would be a build-defined extension and is not built."""
    rng = np.random.default_rng(55)
    L = 300000
    truths = [random_truth(rng, 6000, L) for _ in range(3)]
    tids = [engine.truth_load(*t) for t in truths]
    cols, which = [], []
    for v in range(9):
        w = v % 3
        c = list(random_columns(rng, 20000 + 3000 * v, L, truths[w], weird=False))
        indel = rng.random(len(c[0])) < 0.3
        c[2] = np.where(indel, rng.integers(4, 1 << 20, len(c[0])), c[2]).astype(np.int32)   # allele-pool style codes
        c[1] = np.where(indel & (rng.random(len(c[0])) < 0.5), rng.integers(4, 1 << 20, len(c[0])), c[1]).astype(np.int32)
        snp = (c[1] < 4) & (c[2] < 4)
        c[4] = ((snp & (np.floor(c[3]) >= 20)).astype(np.uint8) | 2).astype(np.uint8)
        cols.append(tuple(c))
        which.append(w)
    res, glob = engine.classify_batch(cols, [tids[w] for w in which])
    for r, c, w in zip(res, cols, which):
        check_vcf(oracle, r, c, truths[w], expect_sorted=True)
        assert not np.any(r["cls"][(c[1] >= 4) | (c[2] >= 4)])            # indel rows are in no output file
    for w in range(3):
        want = sum((r["roc"] for r, ww in zip(res, which) if ww == w), np.zeros((3, 256), np.uint64))
        assert np.array_equal(glob[tids[w]], want)


def test_fp_overlap_vs_sets(engine):
    rng = np.random.default_rng(23)
    sets = []
    for k in range(4):
        n = 3000 + 500 * k
        sets.append((rng.integers(1, 2000, n).astype(np.int32), rng.integers(0, 4, n).astype(np.int32),
                     rng.integers(0, 4, n).astype(np.int32)))
    reg = engine.fp_overlap(sets)
    member = {}
    for k, (p, r, a) in enumerate(sets):
        for key in set(zip(p.tolist(), r.tolist(), a.tolist())):
            member[key] = member.get(key, 0) | (1 << k)
    want = np.zeros(16, np.int64)
    for m in member.values():
        want[m] += 1
    assert np.array_equal(reg, want)


def test_golden_end_to_end_bytes(engine, oracle, tmp_path):
    """BASELINE config 1 + 2 (HCMV-shaped bundle stand-in): the drop-in worker writes exactly the
    bytes the reference wrote, for every caller x sample VCF, in one batch call."""
    import quasimodo_amd as q
    from quasimodo_amd.extract import Job
    jobs, exps = [], []
    for e in CASES:      # the `quirks` family too: its lines are decided on the product's host path
        vcf, truth, exp = read_case(e)
        root = tmp_path / e["family"] / e["mode"]
        vp = root / e["vcf"][len("input/"):]
        tp = root / e["truth"][len("input/"):]
        vp.parent.mkdir(parents=True, exist_ok=True)
        tp.parent.mkdir(parents=True, exist_ok=True)
        vp.write_bytes(vcf)
        tp.write_bytes(truth)
        jobs.append(Job(str(vp), str(tp), e["mode"], str(root / e["outdir"]), e["caller"]))
        exps.append((e, exp, truth))
    q.extract_many(jobs, engine=engine, strict=True)
    n_truth_slots = engine.n_truth
    q.extract_many(jobs[:6], engine=engine, strict=True)
    assert engine.n_truth == n_truth_slots              # a call releases its truth sets: a shared engine reuses the slots
    for job, (e, exp, truth) in zip(jobs, exps):
        assert open(job.filtered_out, "rb").read() == exp["filtered"], case_id(e)
        assert open(job.fp_out, "rb").read() == exp["fp"], case_id(e)
        if e["pure"]:
            assert job.tp_out == ""
            continue
        assert open(job.tp_out, "rb").read() == exp["tp"], case_id(e)
        # declared output paths (extract_TP.smk:6-11 / eval_variant_custom.smk:63-64)
        if e["mode"] == "hcmv":
            assert job.filtered_out.endswith(e["expected"]["filtered"][len("expected/"):])
        rc = oracle.count_text(exp["filtered"], truth, custom=e["mode"] == "custom")
        assert job.stats["n_pass"] == rc["calleridentify"] and job.stats["genomediff"] == rc["genomediff"]
        assert job.stats["TP_R"] == rc["TP"] and job.stats["FP_R"] == rc["FP"], case_id(e)
        assert job.stats["truth_unique"] - job.stats["TP_R"] <= rc["FN"]   # R's FN also counts never-matching rows
        # the line counts are those of the files the reference wrote ('#' lines that pass the filter sit in tp / fp too)
        nl = lambda b: sum(1 for ln in b.split(b"\n") if ln and not ln.startswith(b"#"))
        assert job.stats["tp_lines"] == nl(exp["tp"]) and job.stats["fp_lines"] == nl(exp["fp"]), case_id(e)


def test_cli_dropin(engine, tmp_path):
    """program/extract_TP_FP_SNPs.py: same argv as the reference, non-zero exit on error."""
    import subprocess
    import sys
    from conftest import ROOT
    e = [c for c in CASES if c["family"] == "config1"][0]
    vcf, truth, exp = read_case(e)
    d = tmp_path / "lofreq"
    d.mkdir()
    (d / "TA-1-10.AD169.lofreq.vcf").write_bytes(vcf)
    (tmp_path / "TA.maskrepeat.variants.vcf").write_bytes(truth)
    cli = os.path.join(ROOT, "program", "extract_TP_FP_SNPs.py")
    r = subprocess.run([sys.executable, cli, str(d / "TA-1-10.AD169.lofreq.vcf"), str(tmp_path / "TA.maskrepeat.variants.vcf"),
                        "hcmv", str(d), "lofreq"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (d / "TA-1-10.AD169.lofreq.filtered.vcf").read_bytes() == exp["filtered"]
    assert (d / "tp" / "TA-1-10.AD169.lofreq.tp.vcf").read_bytes() == exp["tp"]
    assert (d / "fp" / "TA-1-10.AD169.lofreq.fp.vcf").read_bytes() == exp["fp"]
    r = subprocess.run([sys.executable, cli, str(d / "missing.vcf"), "x", "hcmv", str(d), "lofreq"], capture_output=True, text=True)
    assert r.returncode != 0 and "extract_TP_FP_SNPs.py" in r.stderr


@pytest.mark.parametrize("shuffled", [False, True], ids=["sorted", "shuffled"])
def test_maximum_sizes_one_vcf_of_133_million_records_up_to_the_position_limit(engine, shuffled):
    """Edge of the encoding: positions up to 2^28 - 2^21 (the key uses all 32 bits), one VCF of 1.3e8
    records (130 048 tiles, 8 128 spans), 2 M truth keys.  Checked with size-independent numpy
    arithmetic on the device's own columns instead of the (slow) oracle."""
    from oracle.synth import synth_truth_keys
    N = (1 << 27) - (1 << 20)
    L, T = 2 * N, N // 64
    assert L < (1 << 28)
    tid = engine.truth_synth(L, T, 9)
    b = engine.batch([N], [tid])
    b.synth(L, T, 9, 9000, shuffled=shuffled)
    b.run()
    b.finish()
    pos, ref, alt, qual, flags = b.columns(0)
    assert int(pos.max()) > (1 << 28) - (1 << 22) and bool((np.diff(pos) > 0).all()) != shuffled
    tp_, tr_, ta_ = synth_truth_keys(L, T, 9)
    tkeys = np.sort((tp_.astype(np.uint32) << 4) | (tr_.astype(np.uint32) << 2) | ta_.astype(np.uint32))
    keys = (pos.astype(np.uint32) << 4) | (ref.astype(np.uint32) << 2) | alt.astype(np.uint32)
    bitmap = np.zeros(1 << 29, np.uint8)            # one bit per possible key: a vectorised gather also when shuffled
    np.bitwise_or.at(bitmap, tkeys >> 3, (1 << (tkeys & 7)).astype(np.uint8))
    hit = ((bitmap[keys >> 3] >> (keys & 7).astype(np.uint8)) & 1).astype(bool)
    del bitmap
    kept = (flags & 1).astype(bool)
    cls = kept.astype(np.uint8) | ((kept & hit).astype(np.uint8) << 1)          # all IDs are '.', all alleles single bases
    got = b.cls(0)
    assert np.array_equal(got, cls)
    sc = dict(zip(("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "sorted", "n", "T"), b.scalars()[0].tolist()))
    assert sc["n_pass"] == int(kept.sum()) and sc["tp_lines"] == int((kept & hit).sum()) and sc["fp_lines"] == int((kept & ~hit).sum())
    assert sc["TP_R"] == sc["tp_lines"] and sc["FP_R"] == sc["fp_lines"]          # positions are distinct: every key is unique
    assert sc["sorted"] == int(not shuffled) and sc["n"] == N and sc["T"] == T
    roc = b.roc()[0]
    bins = np.clip(qual, 0, 255).astype(np.int64)
    for t in (0, 20, 100, 255):
        assert int(roc[0, t]) == int((hit & (bins >= t)).sum()) and int(roc[1, t]) == int((~hit & (bins >= t)).sum())
        assert int(roc[2, t]) == int(roc[0, t])                                    # one record per truth key at most
    idx = b.idx(0)
    assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0].astype(np.int32))
    assert np.array_equal(idx[N - sc["fp_lines"]:], np.nonzero(cls == 1)[0].astype(np.int32))
    b.close()


def test_config3_full_size_properties(engine, oracle):
    """BASELINE configs[2] at its full size on one GPU (1 000 VCFs x 1 M records, 21 GB resident):
    size-independent properties over all VCFs, the oracle on three of them, idempotence, and order
    independence of every counter (the same VCFs shuffled, on a subset)."""
    from oracle.synth import synth_truth_keys
    L, T, N, NV = 5_000_000, 100_000, 1_000_000, 1000
    tid = engine.truth_synth(L, T, 3)
    b = engine.batch([N] * NV, [tid] * NV)
    b.synth(L, T, 3, 3000)
    b.run(); b.finish()
    roc, scal, glob = b.roc(), b.scalars(), b.global_counts()
    assert (scal[:, 6] == N).all() and (scal[:, 5] == 1).all() and (scal[:, 7] == engine.truth_size(tid)).all()
    assert np.array_equal(roc[:, 0, 20].astype(np.int64), scal[:, 1]) and np.array_equal(roc[:, 1, 20].astype(np.int64), scal[:, 2])
    assert (scal[:, 0] == scal[:, 1] + scal[:, 2]).all()
    assert (np.diff(roc.astype(np.int64), axis=2) <= 0).all()                       # cumulative from the top: non-increasing in t
    assert (roc[:, 0, 0] + roc[:, 1, 0] == N).all()                                  # every record has a QUAL >= 0 here
    assert (roc[:, 2, :] <= roc[:, 0, :]).all() and (roc[:, 2, 20].astype(np.int64) == scal[:, 3]).all()   # distinct keys <= TP lines; U(20) = TP_R (all IDs '.')
    assert np.array_equal(glob[tid], roc.sum(axis=0))
    truth = synth_truth_keys(L, T, 3)
    for v in (0, 499, 999):
        cls, oroc, sc = oracle.classify_columns(*b.columns(v), *truth)
        assert np.array_equal(b.cls(v), cls) and np.array_equal(roc[v], oroc)
        assert [int(x) for x in scal[v][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
    b.run(); b.finish()                                                                # idempotent
    assert np.array_equal(b.roc(), roc) and np.array_equal(b.scalars(), scal) and np.array_equal(b.global_counts(), glob)
    b.close()
    ns = 64
    s = engine.batch([N] * ns, [tid] * ns)
    s.synth(L, T, 3, 3000, shuffled=True)
    s.run(); s.finish()
    assert np.array_equal(s.roc(), roc[:ns])
    sc2 = s.scalars()
    assert np.array_equal(sc2[:, :5], scal[:ns, :5]) and (sc2[:, 5] == 0).all()
    s.close()


def test_bench_synth_entry_point(engine):
    """qm_bench_synth (the harness entry point SURVEY.md 8b lists) agrees with the batch API on the same workload"""
    L, T, N, NV = 5_000_000, 100_000, 1_000_000, 8
    r = engine.bench_synth(NV, N, L, T, steps=3)
    tid = engine.truth_synth(L, T, 3)
    b = engine.batch([N] * NV, [tid] * NV)
    b.synth(L, T, 3, 3000)
    b.run(); b.finish()
    sc = b.scalars()
    assert (r["kept"], r["tp_lines"], r["fp_lines"]) == (int(sc[:, 0].sum()), int(sc[:, 1].sum()), int(sc[:, 2].sum()))
    assert r["records"] == NV * N and r["classifications_per_s"] > 1e9 and r["classify_ms"] > 0
    b.close()
    rs = engine.bench_synth(4, N, L, T, steps=2, shuffled=True)
    assert (rs["kept"], rs["tp_lines"]) == (int(sc[:4, 0].sum()), int(sc[:4, 1].sum()))   # VCFs 0..3 of the same seeds, order independent
    ra = engine.bench_synth(4, N, L, T, steps=2, indel_pct=30, truth_seed=5, seed=5000)
    assert ra["kept"] > 0 and ra["tp_lines"] > 0


def test_randomised_adversarial_batches(engine):
    """a short fixed-seed run of tools/gpu_fuzz.py (the long runs are a development tool): runs of equal
    positions across rounds / tiles / spans, oversize truth slices, unsorted VCFs, few bins, both modes"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gpu_fuzz", os.path.join(os.path.dirname(__file__), "..", "tools", "gpu_fuzz.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.run(60, 5, eng=engine) == 0


def test_two_contexts_in_two_threads(oracle):
    """the ABI promises re-entrancy across distinct contexts: two engines on the same GPU, one thread each"""
    import threading
    import quasimodo_amd as q
    out, errs = {}, []

    def work(k):
        try:
            rng = np.random.default_rng(900 + k)
            eng = q.Engine(0)
            truth = random_truth(rng, 3000, 100000)
            tid = eng.truth_load(*truth)
            for rep in range(4):
                cols = [random_columns(rng, n, 100000, truth, sorted_=(rep % 2 == 0)) for n in (5000, 20000, 300)]
                res, _ = eng.classify_batch(cols, [tid] * 3)
                for r, c in zip(res, cols):
                    cls, roc, sc = oracle.classify_columns(*c, *truth)
                    assert np.array_equal(r["cls"], cls) and np.array_equal(r["roc"], roc) and r["scalars"]["FP_R"] == sc["FP_R"]
            eng.close()
            out[k] = True
        except BaseException as e:   # surfaced in the main thread
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    assert out == {0: True, 1: True}


def test_integration_md_ctypes_stub_runs_as_written(tmp_path):
    """the stand-alone ctypes binding shown in INTEGRATION.md is executed verbatim on a golden case"""
    root = os.path.join(os.path.dirname(__file__), "..")
    md = open(os.path.join(root, "INTEGRATION.md")).read()
    sec = md[md.index("## The binding itself"):]
    code = sec[sec.index("```python") + len("```python"):]
    code = code[:code.index("```")]
    e = [c for c in CASES if c["family"] == "config1"][0]
    g = os.path.join(os.path.dirname(__file__), "golden", "config1")
    outs = {k: str(tmp_path / (k + ".vcf")) for k in ("filtered", "tp", "fp")}
    env = {"vcf_path": os.path.join(g, e["vcf"]), "truth_path": os.path.join(g, e["truth"]),
           "filtered_out": outs["filtered"], "tp_out": outs["tp"], "fp_out": outs["fp"]}
    cwd = os.getcwd()
    os.chdir(root)                     # the stub loads quasimodo_amd/csrc/libqmvt.so by relative path
    try:
        exec(compile(code, "INTEGRATION.md", "exec"), env)
    finally:
        os.chdir(cwd)
    for k in ("filtered", "tp", "fp"):
        assert open(outs[k], "rb").read() == open(os.path.join(g, e["expected"][k]), "rb").read(), k


def test_batch_beyond_two_to_the_32_records(engine, oracle):
    """BASELINE configs[3]: one GPU's shard is 1.25e10 records -- global record indices need 64 bits everywhere.
    440 VCFs x 10 M = 4.4e9 records (94 GB resident); the last VCF lies entirely past the 2^32nd record."""
    from oracle.synth import synth_truth_keys
    L, T, N, NV = 50_000_000, 1_000_000, 10_000_000, 440
    assert NV * N > (1 << 32) + N
    tid = engine.truth_synth(L, T, 4)
    b = engine.batch([N] * NV, [tid] * NV)
    b.synth(L, T, 4, 4000)
    b.run(); b.finish()
    roc, scal = b.roc(), b.scalars()
    assert (scal[:, 6] == N).all() and (scal[:, 5] == 1).all()
    assert np.array_equal(roc[:, 0, 20].astype(np.int64), scal[:, 1]) and np.array_equal(roc[:, 1, 20].astype(np.int64), scal[:, 2])
    assert np.array_equal(b.global_counts()[tid], roc.sum(axis=0))
    truth = synth_truth_keys(L, T, 4)
    for v in (0, NV - 1):
        cls, oroc, sc = oracle.classify_columns(*b.columns(v), *truth)
        assert np.array_equal(b.cls(v), cls) and np.array_equal(roc[v], oroc)
        assert [int(x) for x in scal[v][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
        idx = b.idx(v)
        assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0]) and np.array_equal(idx[N - sc["fp_lines"]:], np.nonzero(cls == 1)[0])
    b.close()


def test_error_behaviour_of_the_abi(engine):
    """bad arguments and wrong call order are refused with a code and a message, never guessed at"""
    import ctypes as C
    from quasimodo_amd import QmvtError
    from quasimodo_amd import _lib
    L = _lib.lib()
    tid = engine.truth_load(np.array([5], np.int32), np.array([0], np.int32), np.array([1], np.int32))

    def code(fn):
        with pytest.raises(QmvtError) as e:
            fn()
        assert str(e.value)          # a message, not just a number
        return e.value.code

    assert code(lambda: engine.batch([10], [tid + 1000])) == -1          # unknown truth set
    assert code(lambda: engine.batch([10], [-1])) == -1
    assert code(lambda: engine.batch([-3], [tid])) == -1                 # negative record count
    assert code(lambda: engine.batch([10], [tid], n_bins=0)) == -1
    assert code(lambda: engine.batch([10], [tid], n_bins=257)) == -1
    assert code(lambda: engine.truth_synth(1000, 7, 1)) == -1            # T does not divide L
    assert code(lambda: engine.truth_load(np.array([1 << 28], np.int32), np.array([0], np.int32), np.array([1], np.int32))) == -5
    b = engine.batch([100], [tid])
    assert code(lambda: b.cls(0)) == -6                                   # nothing was run
    assert code(lambda: b.finish()) == -6
    assert code(lambda: b.timings()) == -6
    with pytest.raises(ValueError):
        b.upload(0, np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32), np.zeros(5, np.float32), np.zeros(5, np.uint8))
    assert code(lambda: b._ck(L.qm_batch_upload(b._h, 7, None, None, None, None, None))) == -1      # VCF index out of range
    assert code(lambda: b._ck(L.qm_batch_upload(b._h, 0, None, None, None, None, None))) == -1      # NULL columns
    assert code(lambda: b.synth(1000, 10, 3, 1, indel_pct=30)) == -1                                  # indels need an allele-extended batch
    b.upload(0, np.arange(100, dtype=np.int32), np.zeros(100, np.int32), np.ones(100, np.int32), np.full(100, 30, np.float32), np.full(100, 3, np.uint8))
    b.run()
    assert code(lambda: b.cls(0)) == -6                                   # run but not finished
    b.finish()
    assert int(b.scalars()[0][0]) == 100 and int(b.scalars()[0][1]) == 1      # position 5, A>C is the one true positive
    with pytest.raises(IndexError):
        b.cls(3)
    assert code(lambda: b._ck(L.qm_batch_get_cls(b._h, 3, np.zeros(4, np.uint8).ctypes.data_as(C.c_void_p)))) == -1
    b.close()
    # a second context on a device that does not exist
    h = C.c_void_p()
    assert L.qm_init(99, C.byref(h)) == -1 and b"out of range" in L.qm_last_error(None)
    assert code(lambda: engine.fp_overlap([(np.zeros(1, np.int32),) * 3] * 6)) == -1                    # more than 5 sets


def test_truth_builder_feeds_the_gpu_path(engine, oracle, tmp_path):
    """SURVEY f-2 end to end on the device: a `show-snps -CTHlr` table (SNVs, same-position SNVs that fold into a
    multi-allelic row, insertion and deletion runs, N bases) -> quasimodo_amd.mummer2vcf (the restatement of
    program/mummer2vcf.py: genome_diff.smk:22-24) -> `<sample>.maskrepeat.variants.vcf` -> extractTP on the GPU,
    byte for byte what the oracle's awk / fgrep restatement makes of the same two files."""
    import quasimodo_amd as q
    from quasimodo_amd.extract import Job
    from quasimodo_amd.mummer2vcf import convert
    rng = np.random.default_rng(11)
    L = 60_000
    bases = np.array(list("ACGT"))
    seq = "".join(bases[rng.integers(0, 4, L)])
    fa = tmp_path / "ref.fa"
    fa.write_text(">Merlin\n" + "\n".join(seq[i:i + 70] for i in range(0, L, 70)) + "\n")
    rows, p2 = [], 1
    for p in np.sort(rng.choice(np.arange(2, L - 2), 6000, replace=False)):
        ref = seq[p - 1]
        kind = rng.random()
        p2 += 7
        col = lambda a, b, c: "\t".join([str(a), b, c, str(p2), "5", "100", str(L), str(L), "1", "1", "Merlin", "qry"]) + "\n"
        if kind < 0.80:                      # SNV, sometimes a second allele at the same place, sometimes an N
            alt = "ACGT"[("ACGT".index(ref) + int(rng.integers(1, 4))) & 3]
            rows.append(col(p, ref, "N" if kind < 0.02 else alt))
            if kind > 0.74:
                rows.append(col(p, ref, "ACGT"[("ACGT".index(alt) + 1) & 3] if "ACGT"[("ACGT".index(alt) + 1) & 3] != ref else alt))
        elif kind < 0.90:                    # insertion run: '.' in the reference column, consecutive query positions
            for k in range(int(rng.integers(1, 4))):
                rows.append(col(p, ".", "ACGT"[int(rng.integers(0, 4))]))
                p2 += 1
        else:                                # deletion: '.' in the query column
            rows.append(col(p, ref, "."))
    truth_text = ("\n".join(convert(rows, reference=str(fa), no_ns=True, output_header=True)) + "\n").encode()
    tpath = tmp_path / "TM.maskrepeat.variants.vcf"
    tpath.write_bytes(truth_text)
    tk = q.scan_truth(truth_text)
    assert tk.n_refused == 0 and len(tk.pos) > 3000
    # a caller's VCF over the same genome: half of its records on truth SNVs, PASS and non-PASS, sorted
    n = 20_000
    pos = np.sort(np.where(rng.random(n) < 0.5, tk.pos[rng.integers(0, len(tk.pos), n)], rng.integers(1, L + 1, n)))
    j = np.searchsorted(tk.pos, pos).clip(0, len(tk.pos) - 1)
    on = tk.pos[j] == pos
    ref = np.where(on, tk.ref[j], rng.integers(0, 4, n))
    alt = np.where(on & (rng.random(n) < 0.85), tk.alt[j], (ref + rng.integers(1, 4, n)) & 3)
    lines = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for p, r, a, ql, ps in zip(pos, ref, alt, rng.integers(0, 300, n), rng.random(n) < 0.9):
        lines.append(b"Merlin\t%d\t.\t%s\t%s\t%d\t%s\tDP=50" % (p, b"ACGT"[r:r + 1], b"ACGT"[a:a + 1], ql, b"PASS" if ps else b"q10"))
    vcf_text = b"\n".join(lines) + b"\n"
    d = tmp_path / "lofreq"
    d.mkdir()
    vpath = d / "TM-1-10.Merlin.lofreq.vcf"
    vpath.write_bytes(vcf_text)
    job = Job(str(vpath), str(tpath), "hcmv")
    q.extract_many([job], engine=engine, strict=True)
    want_f, want_t, want_p, _ = oracle.extract_text(vcf_text, truth_text)
    assert open(job.filtered_out, "rb").read() == want_f
    assert open(job.tp_out, "rb").read() == want_t and open(job.fp_out, "rb").read() == want_p
    assert job.stats["tp_lines"] > 5000
    rc = oracle.count_text(want_f, truth_text)
    assert job.stats["TP_R"] == rc["TP"] and job.stats["FP_R"] == rc["FP"] and job.stats["genomediff"] == rc["genomediff"]


def test_unsorted_vcf_behind_stale_mask_words(engine, oracle, monkeypatch):
    """The bucket path's scatter writes the kept mask in 32-bit words, the compaction reads 64-bit ones: the words
    between a VCF's last record and the end of its padding must be written too.  Found by `tools/gpu_fuzz.py 100 8`
    (round 99: an unsorted VCF of 1 025 records whose FP index list picked up bits that had been left in that memory),
    which is the reliable reproducer -- whether this test meets dirty memory depends on the allocator; it pins the
    batch shape and leaves ones behind from a first batch of the same padded sizes."""
    from conftest import random_columns, random_truth
    monkeypatch.setenv("QM_BUCKET_MIN", "0")    # VCFs this small take the radix sort otherwise
    rng = np.random.default_rng(5)
    L = (1 << 28) - 1
    truth = random_truth(rng, 50, L)
    tid = engine.truth_load(*truth)
    sizes = [4096, 4096, 1025, 1024, 1024, 1023]
    # same shapes, every record kept and in order: leaves ones in every mask word of the padded regions
    full = []
    for n in sizes:
        n_pad = (n + 255) // 256 * 256
        pos = np.arange(1, n_pad + 1, dtype=np.int32)
        full.append((pos, np.zeros(n_pad, np.int32), np.ones(n_pad, np.int32), np.full(n_pad, 99, np.float32), np.full(n_pad, 3, np.uint8)))
    engine.classify_batch(full, [tid] * len(sizes))
    cols = [random_columns(rng, n, L, truth, sorted_=False) for n in sizes]
    res, _ = engine.classify_batch(cols, [tid] * len(sizes))
    for r, c in zip(res, cols):
        check_vcf(oracle, r, c, truth)


def test_batch_of_empty_vcfs(engine, oracle):
    """No record at all: k_classify is not launched (its first wave is what clears the per-truth sums), the sums are still zero."""
    from conftest import random_truth
    rng = np.random.default_rng(2)
    truth = random_truth(rng, 100, 10_000)
    tid = engine.truth_load(*truth)
    e = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.uint8))
    for _ in range(2):
        res, glob = engine.classify_batch([e, e, e], [tid] * 3)
        assert not glob[tid].any()
        for r in res:
            check_vcf(oracle, r, e, truth)


def test_many_small_unsorted_vcfs_and_a_few_large_ones(engine, oracle):
    """The unsorted VCFs of a batch are split by size: the bucket path takes the large ones (it costs 256 workgroups and 256
    histogram rows per VCF), the radix sort the small ones -- here 1 500 VCFs of a few hundred records beside three of 40 000."""
    from conftest import random_columns, random_truth
    rng = np.random.default_rng(77)
    L = 300_000
    truth = random_truth(rng, 5000, L)
    tid = engine.truth_load(*truth)
    sizes = [int(x) for x in rng.integers(1, 700, 1500)] + [40_000, 40_001, 39_999]
    order = rng.permutation(len(sizes))
    sizes = [sizes[i] for i in order]
    cols = [random_columns(rng, n, L, truth, sorted_=bool(rng.random() < 0.2)) for n in sizes]
    res, glob = engine.classify_batch(cols, [tid] * len(sizes))
    want = np.zeros((3, 256), np.uint64)
    for i, (r, c) in enumerate(zip(res, cols)):
        want += r["roc"]
        if i % 25 == 0 or len(c[0]) > 30_000:
            check_vcf(oracle, r, c, truth)
    assert np.array_equal(glob[tid], want)
    engine.truth_release(tid)


@pytest.mark.parametrize("shuffled,pct", [(False, 0), (True, 0), (False, 30)], ids=["sorted", "shuffled", "indels"])
def test_synthetic_workload_is_what_the_specification_says(engine, shuffled, pct):
    """DESIGN.md section 4.5 is THE definition of the bench workload: oracle/synth.py restates it in numpy, and the columns the
    device generates (qm_batch_synth) equal that restatement record for record -- a third party can regenerate the
    workload of the bench line from the text alone."""
    from oracle.synth import synth_vcf_columns
    L, T, N = 5_000_000, 100_000, 1_000_000
    tid = engine.truth_synth(L, T, 3, indel_pct=pct)
    b = engine.batch([N, N // 2, N], [tid] * 3, alleles=pct > 0)
    b.synth(L, T, 3, 3000, shuffled=shuffled, indel_pct=pct)
    for v, n in ((0, N), (1, N // 2), (2, N)):
        want = synth_vcf_columns(L, n, T, 3, 3000 + v, indel_pct=pct, shuffled=shuffled, vcf_sizes=[N, N // 2, N])
        got = b.columns(v)
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (v, k)
    b.close()
    engine.truth_release(tid)


@pytest.mark.parametrize("memo", ["1", "0"], ids=["memo", "first-seen"])
def test_vcfs_sorted_per_contig(engine, oracle, monkeypatch, memo):
    """A VCF of several contigs is sorted PER CONTIG: POS restarts with every CHROM, and the reference never compares CHROM
    (extract_TP_FP_SNPs.py:47: the pattern is POS . REF ALT), so the contigs share one position space and a key may repeat across
    them (such input fell to the radix sort -- a bucket's pieces are long, one per contig, and three of them on
    one sub-region were an overflow).  Synthetic VCFs of 24 ascending runs (qm_synth_cfg.shuffled = 24; the device's columns equal
    oracle/synth.py's), ragged hand-made ones with keys REPEATED across the runs (the cross-run counts TP_R / FP_R / U(t)), against the
    oracle; the generated ones also against the same records in one ascending run.  Nothing takes the radix sort."""
    from oracle.synth import synth_truth_keys, synth_vcf_columns
    monkeypatch.setenv("QM_MEMO", memo)
    L, T, N = 5_000_000, 100_000, 1_000_000
    tid = engine.truth_synth(L, T, 3)
    tk = synth_truth_keys(L, T, 3)
    rows = {}
    for runs in (0, 24):
        b = engine.batch([N, N // 2, N], [tid] * 3)
        b.synth(L, T, 3, 3000, shuffled=runs)
        for rep in range(2):
            b.run(); b.finish()
        rows[runs] = (b.roc(), b.scalars()[:, :5].copy(), b.global_counts())
        if runs:
            ps = b.path_stats()
            assert ps["unsorted"] == 3 and ps["radix"] == 0 and ps["radix_after_overflow"] == 0, ps
            want = synth_vcf_columns(L, N // 2, T, 3, 3001, shuffled=24)
            cols = b.columns(1)
            assert all(np.array_equal(g, w) for g, w in zip(cols, want))
            assert int((np.diff(cols[0]) < 0).sum()) == 23
            for v in (0, 1):
                cols = b.columns(v)
                cls, oroc, sc = oracle.classify_columns(*cols, *tk)
                assert np.array_equal(b.cls(v), cls) and np.array_equal(rows[runs][0][v], oroc)
                assert [int(x) for x in rows[runs][1][v]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")]
                idx = b.idx(v)
                assert np.array_equal(idx[:sc["tp_lines"]], np.nonzero(cls == 3)[0]) and np.array_equal(idx[len(cls) - sc["fp_lines"]:], np.nonzero(cls == 1)[0])
        b.close()
    for k in range(3):
        assert np.array_equal(rows[0][k], rows[24][k]), k
    engine.truth_release(tid)
    # hand-made: contigs of ragged sizes whose keys repeat across contigs (and inside one), truth keys hit from several contigs
    rng = np.random.default_rng(77)
    Ls = 300_000
    truth = random_truth(rng, 9_000, Ls)
    tid2 = engine.truth_load(*truth)
    cols = []
    for n_contigs, n in ((2, 20_000), (7, 60_000), (31, 200_000), (3, 4_100)):
        parts = [random_columns(rng, max(1, int(n * w)), Ls, truth) for w in rng.dirichlet(np.ones(n_contigs))]
        parts.append(tuple(a[: len(a) // 2].copy() for a in parts[0]))           # a contig that repeats half of another one's records
        cols.append(tuple(np.concatenate([p[k] for p in parts]) for k in range(5)))
    b = engine.batch([len(c[0]) for c in cols], [tid2] * len(cols))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    for rep in range(2):
        b.run(); b.finish()
        roc, scal = b.roc(), b.scalars()
        for v, c in enumerate(cols):
            cls, oroc, sc = oracle.classify_columns(*c, *truth)
            assert np.array_equal(b.cls(v), cls) and np.array_equal(roc[v], oroc), (rep, v)
            assert [int(x) for x in scal[v][:5]] == [sc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")], (rep, v)
    b.close()
    engine.truth_release(tid2)


@pytest.mark.parametrize("memo", ["1", "0"], ids=["memo", "no-memo"])
def test_a_batch_remembers_which_vcfs_were_out_of_order_until_their_columns_change(engine, oracle, monkeypatch, memo):
    """What a finish found stays known to the batch while the columns stay the same: on the next run the VCFs found out of order
    are not streamed by the optimistic pass and their bucket path (or radix sort) is queued without first waiting for the flags.
    The answers must be the ones of a fresh batch -- after a plain repeat, and after uploads that turn an unsorted VCF into a
    sorted one, a sorted one into an unsorted one, and replace an unsorted one by another unsorted one (QM_MEMO=0: the same
    without the memory)."""
    monkeypatch.setenv("QM_MEMO", memo)
    rng = np.random.default_rng(31)
    L = 500_000
    truth = random_truth(rng, 20_000, L)
    tid = engine.truth_load(*truth)
    sizes = [40_000, 3_000, 50_000, 20_000, 0, 70_000]
    order = [False, False, True, True, True, False]      # sorted?
    cols = [random_columns(rng, n, L, truth, sorted_=s) for n, s in zip(sizes, order)]
    b = engine.batch(sizes, [tid] * len(sizes))

    def check_all(n_unsorted):
        roc, sc = b.roc(), b.scalars()
        want = np.zeros((3, 256), np.uint64)
        for v, c in enumerate(cols):
            cls, oroc, osc = oracle.classify_columns(*c, *truth)
            assert np.array_equal(b.cls(v), cls), v
            assert np.array_equal(roc[v], oroc), v
            assert [int(x) for x in sc[v, :5]] == [osc[k] for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R")], v
            idx = b.idx(v)
            assert np.array_equal(idx[:osc["tp_lines"]], np.nonzero(cls == 3)[0]) and np.array_equal(idx[len(cls) - osc["fp_lines"]:], np.nonzero(cls == 1)[0])
            want += oroc
        assert np.array_equal(b.global_counts()[tid], want)
        assert b.path_stats()["unsorted"] == n_unsorted

    for v, c in enumerate(cols):
        b.upload(v, *c)
    for _ in range(3):                 # the first finish finds them, the others know
        b.run(); b.finish()
        check_all(3)
    cols[0] = random_columns(rng, sizes[0], L, truth, sorted_=True)    # unsorted -> sorted
    cols[2] = random_columns(rng, sizes[2], L, truth, sorted_=False)   # sorted -> unsorted
    cols[5] = random_columns(rng, sizes[5], L, truth, sorted_=False)   # unsorted -> other unsorted records
    for v in (0, 2, 5):
        b.upload(v, *cols[v])
    for _ in range(2):
        b.run(); b.finish()
        check_all(3)
    cols[1] = random_columns(rng, sizes[1], L, truth, sorted_=True)    # the last small one in order too: only the two large ones remain
    b.upload(1, *cols[1])
    for _ in range(2):
        b.run(); b.finish()
        check_all(2)
    b.close()
    engine.truth_release(tid)


def test_unsorted_vcfs_on_a_reference_of_ten_million_positions_take_a_pair_of_partitions(engine, oracle):
    """Default mode, 1 M records on a 10 Mb reference, out of order: the key range needs buckets of 2^20 keys on the one-level path
    (the hashed join); as ONE pair of partitions of 2^27 keys it is one pass of the 512-digit scatter and the bit-map join.  Against
    the sorted run and, for one VCF, the oracle."""
    from oracle.synth import synth_truth_keys
    L, T, N = 10_000_000, 100_000, 1_000_000
    tid = engine.truth_synth(L, T, 9)
    rows = {}
    for shuffled in (False, True):
        b = engine.batch([N] * 3, [tid] * 3)
        b.synth(L, T, 9, 7000, shuffled=shuffled)
        for _ in range(2 if shuffled else 1):
            b.run(); b.finish()
        rows[shuffled] = (b.roc(), b.scalars()[:, :5].copy(), b.global_counts())
        if shuffled:
            ps = b.path_stats()
            assert ps["unsorted"] == 3 and ps["bucket_partitions"] == 3 and ps["bucket_two_level"] == 0 and ps["bucket_hashed"] == 0 and ps["radix"] == 0, ps
            cls, oroc, sc = oracle.classify_columns(*b.columns(2), *synth_truth_keys(L, T, 9))
            assert np.array_equal(b.cls(2), cls) and np.array_equal(rows[True][0][2], oroc)
        b.close()
    for k in range(3):
        assert np.array_equal(rows[True][k], rows[False][k]), k
    engine.truth_release(tid)


def test_positions_above_what_the_optimistic_pass_saw(engine, oracle):
    """The optimistic pass leaves a span at its first ROUND out of order (256 records; its first tile until round 5), so the OR of the
    positions it saw can miss the highest ones; the bucket path sizes its join by that OR.  A shuffled VCF (every span is left at once) whose first tiles
    hold no position with bit 21 or above 0x5fffff -- an OR of 0x5fffff: 192 buckets of 256 -- while a quarter of the other
    records lie at 0x600000 and above (buckets 192..255): those records must be classified (by the radix sort, after the scatter
    flags the VCF), not dropped (the join was trimmed to the buckets below the estimate and nothing noticed).
    Run three times: the first run pays for the radix sort, whose first pass ORs every key of its chunk -- those bits correct the
    estimate the batch remembers the VCF with (round 6, ADVICE 5: until then the same overflow came back on every run), so the
    later runs size the buckets for what the VCF really holds and stay on them."""
    rng = np.random.default_rng(4242)
    n, span = 40000, 16384
    seen = np.zeros(n, bool)
    for s0 in range(0, n, span):
        seen[s0:s0 + 1024] = True   # the first tile of every span: all the optimistic pass ever saw of a shuffled VCF (its first 256 records now)
    seen[(np.arange(64) * n) >> 6] = True   # ... and the sixty-four records every span samples over the whole VCF (round 6)
    lo = rng.choice(np.concatenate([np.arange(1, 0x200000), np.arange(0x400000, 0x600000)]), size=n - n // 4, replace=False)
    hi = rng.choice(np.arange(0x600000, 0x800000), size=n // 4, replace=False)
    pos = np.empty(n, np.int32)
    pos[seen] = lo[:seen.sum()]                                  # shuffled: every first tile is out of order
    rest = np.concatenate([lo[seen.sum():], hi])
    rng.shuffle(rest)
    pos[~seen] = rest
    ref = rng.integers(0, 4, n).astype(np.int32)
    alt = ((ref + 1 + rng.integers(0, 3, n)) & 3).astype(np.int32)
    qual = rng.integers(0, 256, n).astype(np.float32)
    flags = (2 | (qual >= 20)).astype(np.uint8)
    take = rng.random(n) < 0.3                                   # truth: a third of the records' keys, high positions included
    tp_, tr_, ta_ = pos[take], ref[take], alt[take]
    o = np.lexsort((ta_, tr_, tp_))
    truth = (tp_[o], tr_[o], ta_[o])
    assert (truth[0] >= 0x600000).sum() > 100
    tid = engine.truth_load(*truth)
    cols = (pos, ref, alt, qual, flags)
    b = engine.batch([n], [tid])
    b.upload(0, *cols)
    from quasimodo_amd.engine import SCALAR_NAMES
    for rep in range(3):
        b.run()
        b.finish()
        sc = dict(zip(SCALAR_NAMES, b.scalars()[0].tolist()))
        reg = b.idx(0)
        res = {"cls": b.cls(0), "roc": b.roc()[0], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[n - sc["fp_lines"]:].copy()}
        check_vcf(oracle, res, cols, truth, expect_sorted=False)
        ps = b.path_stats()
        assert ps["radix_after_overflow"] == (1 if rep == 0 else 0) and ps["bucket_direct"] == (0 if rep == 0 else 1), (rep, ps)
    b.close()


@pytest.mark.parametrize("knobs", [{}, {"QM_SPECULATE": "0"}, {"QM_NO_MIRRORS": "1"}],
                         ids=["queued", "looked-at", "no-host-mapped-mirrors"])
def test_several_bucket_chunks_in_one_finish_one_of_which_does_not_fit(engine, oracle, monkeypatch, knobs):
    """qm_batch_finish queues the last kernels of a bucket chunk without looking at the chunk's flags first (a round trip through
    the host per chunk) and settles all chunks behind its last wait: a chunk whose buckets did not fit must not have added its
    rows to the per-truth sums, goes through the radix sort then, and the compaction runs again.  Five unsorted VCFs in five
    chunks (QM_SORT_CHUNK_RECORDS), the third of them 60 000 records on 16 positions; twice, the second time with the batch's
    memory of the first; the knobs switch the round trips of round 4 back on: the look at a chunk's flags before its last
    kernels, and (without the mirrors) the wait for the whole stream before the flags are read."""
    from conftest import random_columns, random_truth
    from quasimodo_amd.engine import SCALAR_NAMES
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("QM_SORT_CHUNK_RECORDS", "50000")
    rng = np.random.default_rng(515)
    L = 400_000
    truth = random_truth(rng, 8000, L)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, L, truth, sorted_=False) for n in (40_000, 33_000)]
    n = 60_000
    pos = rng.integers(1000, 1016, n).astype(np.int32)
    ref = rng.integers(0, 4, n).astype(np.int32)
    alt = rng.integers(0, 4, n).astype(np.int32)
    qual = rng.integers(0, 300, n).astype(np.float32)
    cols.append((pos, ref, alt, qual, ((qual >= 20).astype(np.uint8) | 2).astype(np.uint8)))
    cols += [random_columns(rng, n, L, truth, sorted_=s) for n, s in ((45_000, False), (20_000, True), (38_000, False))]
    b = engine.batch([len(c[0]) for c in cols], [tid] * len(cols))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    for _ in range(2):
        b.run()
        b.finish()
        want = np.zeros((3, 256), np.uint64)
        for v, c in enumerate(cols):
            sc = dict(zip(SCALAR_NAMES, b.scalars()[v].tolist()))
            reg = b.idx(v)
            res = {"cls": b.cls(v), "roc": b.roc()[v], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[len(c[0]) - sc["fp_lines"]:].copy()}
            check_vcf(oracle, res, c, truth, expect_sorted=(v == 4))
            want += res["roc"]
        assert np.array_equal(b.global_counts()[tid], want)   # nothing of the chunk that did not fit was added twice
        st = b.path_stats()
        assert st["bucket_chunks"] == 5 and st["overflow_chunks"] == 1 and st["radix_after_overflow"] == 1 and st["bucket_direct"] == 4, st
    b.close()
    engine.truth_release(tid)


def test_the_compaction_on_lists_of_every_density(engine, oracle):
    """k_compact stores a list chunk by chunk: a wave the chunks that begin among its entries, completed from the ONE tile behind
    its own; what lies beyond that reach is stored by the wave whose tiles hold it.  The lists must come out whole
    whatever they hold: dense and sparse, empty, one entry, everything TP, a handful of kept records at the far ends of a long
    VCF (chunks that no wave completes), TP lines in one half only, ragged sizes."""
    rng = np.random.default_rng(77)
    L = 400000
    truth = random_truth(rng, 30000, L)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, L, truth, sorted_=True) for n in (0, 1, 255, 256, 257, 1023, 1025, 4095, 4097, 20000, 70001)]

    def plain(n, keep, hit):   # n sorted records on distinct positions; keep / hit: boolean arrays (kept by the filter; carries a truth key)
        pos = (np.arange(n, dtype=np.int64) * 3 + 5).astype(np.int32)
        ref = np.zeros(n, np.int32)
        alt = np.where(hit, 1, 2).astype(np.int32)
        qual = np.where(keep, 50, 3).astype(np.float32)
        return pos, ref, alt, qual, (2 | keep).astype(np.uint8)

    n = 90000
    tpos = (np.arange(n, dtype=np.int64) * 3 + 5).astype(np.int32)
    truth2 = (tpos, np.zeros(n, np.int32), np.ones(n, np.int32))          # every position with ALT = C: a record hits iff its ALT is C
    tid2 = engine.truth_load(*truth2)
    e = np.zeros(n, bool)
    far = e.copy(); far[[3, n - 2]] = True
    few = e.copy(); few[rng.choice(n, 40, replace=False)] = True
    half = e.copy(); half[: n // 2] = rng.random(n // 2) < 0.3          # a dense list that stops: the chunk at its end is never whole
    thin = rng.random(n) < 0.004                                          # a few entries per tile: chunks span many waves
    edge = e.copy(); edge[np.arange(0, n, 1024)] = True; edge[np.arange(1023, n, 1024)] = True   # the first and last record of every tile
    shapes = [plain(n, ~e, ~e),            # everything kept, everything TP: the FP list is empty
              plain(n, ~e, e),             # everything kept, nothing TP
              plain(n, e, e),              # nothing kept: both lists empty
              plain(n, far, far),          # two TP lines, at the two ends of the VCF: the chunk that holds them is nobody's to complete
              plain(n, ~e, half), plain(n, half, e), plain(n, ~e, thin), plain(n, thin, thin), plain(n, thin, e),
              plain(n, ~e, edge), plain(n, edge, edge), plain(n, edge, e),
              plain(n, ~e, few),           # a dense FP list, forty TP lines somewhere
              plain(n, few, e),            # forty FP lines, nothing else
              plain(n, rng.random(n) < 0.5, rng.random(n) < 0.5)]
    res, _ = engine.classify_batch(cols + shapes, [tid] * len(cols) + [tid2] * len(shapes))
    for r, c in zip(res, cols):
        check_vcf(oracle, r, c, truth)
    for r, c in zip(res[len(cols):], shapes):
        check_vcf(oracle, r, c, truth2, expect_sorted=True)
