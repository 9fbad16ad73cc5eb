"""k_classify_pair (sorted, single-base, column input: two rounds of 256 records joined against the truth keys at once) against
the oracle, through the public batch path, on the seams a pair adds: record 255|256 inside a pair, 511|512 between pairs,
1 023|1 024 between tiles, 16 383|16 384 between spans.  Needs an MI355X."""
import numpy as np
import pytest

from conftest import random_columns, random_truth

pytestmark = pytest.mark.gpu

PASS, IDDOT, NOKEY = 1, 2, 4


def check_vcf(oracle, res, cols, truth, n_bins=256, expect_sorted=None):
    """class bits, ROC row, scalars and both index lists against the oracle (as test_gpu_parity.check_vcf)"""
    cls, roc, sc = oracle.classify_columns(*cols, *truth, n_bins=n_bins)
    assert np.array_equal(res["cls"], cls)
    assert np.array_equal(res["roc"], roc)
    s = res["scalars"]
    for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "truth_unique"):
        assert s[k] == sc[k], (k, s[k], sc[k])
    assert s["n_records"] == len(cols[0])
    if expect_sorted is not None:
        assert s["sorted"] == int(expect_sorted)
    assert np.array_equal(res["tp_idx"], np.nonzero(cls == 3)[0])
    assert np.array_equal(res["fp_idx"], np.nonzero(cls == 1)[0])
    if n_bins > 20:
        assert int(res["roc"][0, 20]) == s["tp_lines"] and int(res["roc"][1, 20]) == s["fp_lines"]


SEAMS = (256, 512, 1024, 16384)


def _cols(pos, ref, alt, qual, flags):
    return (np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(ref, np.int32), np.ascontiguousarray(alt, np.int32),
            np.ascontiguousarray(qual, np.float32), np.ascontiguousarray(flags, np.uint8))


def _truth(keys):
    k = np.array(sorted(set(keys)), np.int64).reshape(-1, 3)
    return k[:, 0].astype(np.int32), k[:, 1].astype(np.int32), k[:, 2].astype(np.int32)


def _run(engine, oracle, cols, truths, n_bins=256, expect_sorted=True):
    """cols[i] against truths[i] (tuples; equal objects are loaded once), one batch, every VCF checked like test_gpu_parity."""
    ids = {}
    for t in truths:
        if id(t) not in ids:
            ids[id(t)] = engine.truth_load(*t)
    res, _ = engine.classify_batch(cols, [ids[id(t)] for t in truths], n_bins=n_bins)
    try:
        for r, c, t in zip(res, cols, truths):
            check_vcf(oracle, r, c, t, n_bins=n_bins, expect_sorted=expect_sorted)
    finally:
        for tid in ids.values():
            engine.truth_release(tid)
    return res


def _ladder(n, step=2, start=100):
    """n records on distinct ascending positions, REF/ALT 0/1, QUAL 50, PASS and '.' ID: every record a TP line iff its key is a truth key"""
    pos = start + step * np.arange(n, dtype=np.int64)
    return [pos.astype(np.int32), np.zeros(n, np.int32), np.ones(n, np.int32), np.full(n, 50, np.float32), np.full(n, PASS | IDDOT, np.uint8)]


LENGTHS = [255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1535, 1537, 16383, 16384, 16385,
           16384 + 511, 16384 + 512, 16384 + 513]


def test_lengths_around_every_seam(engine, oracle):
    """A last pair with only its first half, an empty or ragged second half, a span of one round.  Against a sparse truth set
    (every tile's slice fits: the pair join) and a dense one (the small VCFs' tiles are above the slice cap: round by round)."""
    rng = np.random.default_rng(2701)
    L = 60000
    sparse, dense = random_truth(rng, 150, L), random_truth(rng, 4000, L)
    cols, truths = [], []
    for n in LENGTHS:
        for t in (sparse, dense):
            cols.append(random_columns(rng, n, L, t, sorted_=True))
            truths.append(t)
    _run(engine, oracle, cols, truths)


def _seam_vcf(rng, base_pos, seam, lo, hi):
    """base_pos with records [lo, hi) moved onto ONE position (that of record lo): a run across `seam`.  The run's records carry
    two keys only (0/1 and 0/2), kept and not, '.' IDs and others, so kept keys repeat across the seam."""
    n = len(base_pos)
    pos = base_pos.copy()
    pos[lo:hi] = base_pos[lo]
    ref = rng.integers(0, 4, n).astype(np.int32)
    alt = rng.integers(0, 4, n).astype(np.int32)
    ref[lo:hi] = 0
    alt[lo:hi] = rng.integers(1, 3, hi - lo)
    qual = rng.integers(0, 300, n).astype(np.float32)
    flags = ((qual >= 20).astype(np.uint8) * PASS) | ((rng.random(n) > 0.2).astype(np.uint8) * IDDOT) | ((rng.random(n) < 0.03).astype(np.uint8) * NOKEY)
    # both sides of the seam hold kept '.'-ID records of key 0/1 (TP_R, U(t), ownership) and kept records of key 0/2 (FP_R)
    for i, a in ((seam - 2, 1), (seam - 1, 2), (seam, 2), (seam + 1, 1)):
        if lo <= i < hi:
            alt[i] = a; flags[i] = PASS | IDDOT; qual[i] = 40 + (i & 7)
    return _cols(pos, ref, alt, qual, flags.astype(np.uint8))


def test_runs_of_one_position_across_each_seam(engine, oracle):
    rng = np.random.default_rng(2702)
    n = 16384 + 1500
    base = (50 + np.cumsum(rng.integers(1, 5, n))).astype(np.int32)     # strictly ascending
    runs = [(s, s - 7, s + 9) for s in SEAMS] + [(s, s - 1, s + 1) for s in SEAMS]
    runs += [(512, 300, 900), (256, 200, 800), (1024, 700, 1300), (16384, 16384 - 300, 16384 + 300)]   # 600 records: longer than a pair
    run_pos = sorted({int(base[lo]) for _, lo, _ in runs})
    bg = random_truth(rng, 900, int(base[-1]))
    bg_keys = [(int(p), int(r), int(a)) for p, r, a in zip(*bg) if int(p) not in run_pos]
    t_without = _truth(bg_keys)
    t_with = _truth(bg_keys + [(p, 0, 1) for p in run_pos])
    cols, truths = [], []
    for seam, lo, hi in runs:
        c = _seam_vcf(rng, base, seam, lo, hi)
        cols += [c, c]
        truths += [t_with, t_without]
    _run(engine, oracle, cols, truths)


def test_truth_keys_at_the_edges_of_a_pair(engine, oracle):
    """Keys on the first and the last position of a pair, a pair whose range holds none, a pair with 65..128 keys (the key loop's
    second trip), a tile above the slice cap (chunked, round by round) between ordinary ones."""
    n = 5 * 1024 + 300
    c = _ladder(n)
    p = c[0]
    key = lambda i: (int(p[i]), 0, 1)
    miss = lambda i: (int(p[i]) + 1, 0, 1)          # a position between two records
    edges = [key(i) for k in range(0, n, 512) for i in (k, min(k + 511, n - 1))]
    t_edges = _truth(edges)
    t_first = _truth([key(k) for k in range(0, n, 512)])
    t_last = _truth([key(k + 511) for k in range(0, n - 511, 512)])
    t_hole = _truth([key(i) for i in range(0, 512, 9)] + [key(i) for i in range(1024, 1536, 9)] + [miss(700)])   # pair 1: no key matches, one lies between
    t_none_in_pair = _truth([key(i) for i in range(0, 512, 9)] + [key(i) for i in range(1024, n, 9)])              # pair 1: nothing in its range
    t_loop2 = _truth([key(i) for i in range(512, 1024, 5)] + [key(3), key(1500)])                                     # 103 keys in pair 1
    t_loop2b = _truth([key(i) for i in range(0, 512, 4)] + [key(i) for i in range(512, 1024, 7)])                    # 128 + 74: both pairs of a tile, 202 <= cap
    t_over = _truth([key(i) for i in range(2048, 3072) if i % 5 != 0] + [miss(i) for i in range(2048, 3072, 3)] +
                    [key(i) for i in range(0, n, 37)])                                                               # tile 2: > 1 100 keys, three chunks and more per round
    truths = [t_edges, t_first, t_last, t_hole, t_none_in_pair, t_loop2, t_loop2b, t_over]
    _run(engine, oracle, [_cols(*c)] * len(truths), truths)


def test_hit_set_extremes(engine, oracle):
    n = 2048 + 100
    c = _ladder(n)
    p = c[0]
    key = lambda i: (int(p[i]), 0, 1)
    far = (int(p[-1]) + 1000, 0, 1)
    cols, truths = [], []
    # only record 0 / 255 / 256 / 511 of a pair is a TP (first pair, and the second pair of the second tile)
    for b in (0, 1536):
        for i in (0, 255, 256, 511):
            cols.append(_cols(*c)); truths.append(_truth([key(b + i), far]))
    # none: the truth set lies elsewhere; lies on the same positions with another allele; lies between the records
    cols.append(_cols(*c)); truths.append(_truth([far]))
    cols.append(_cols(*c)); truths.append(_truth([(int(p[i]), 0, 2) for i in range(0, 512, 3)]))
    cols.append(_cols(*c)); truths.append(_truth([(int(p[i]) + 1, 0, 1) for i in range(0, 512, 3)]))
    # all 512 records of a pair: 512 distinct keys (above the slice cap: round by round) ...
    cols.append(_cols(*c)); truths.append(_truth([key(i) for i in range(512, 1024)]))
    # ... and 128 keys carried by four records each (the pair join: every bit of the 16 hit words set)
    d = _ladder(n)
    d[0][512:1024] = np.repeat(d[0][512:1024:4], 4)
    cols.append(_cols(*d)); truths.append(_truth([(int(q), 0, 1) for q in d[0][512:1024:4]]))
    res = _run(engine, oracle, cols, truths)
    assert [r["scalars"]["tp_lines"] for r in res[:8]] == [1] * 8
    assert [r["scalars"]["tp_lines"] for r in res[8:]] == [0, 0, 0, 512, 512]
    assert res[12]["scalars"]["TP_R"] == 128


@pytest.mark.parametrize("n", [3000, 20000])
def test_single_descent_is_flagged_and_redone(engine, oracle, n):
    """One descent exactly at 255->256, at 511->512 and inside each half: the VCF is flagged and redone (the sort below 16 384
    records, the buckets above), every output as the oracle's."""
    rng = np.random.default_rng(2705 + n)
    truth = random_truth(rng, 500, 3 * n)
    cols = []
    for k in (256, 512, 100, 300, 768, 1024, 1280, 1600, n - 1):
        pos = (10 + 3 * np.arange(n)).astype(np.int32)
        pos[k] = pos[k - 1] - 1                      # pos[k - 2] < pos[k] < pos[k - 1] < pos[k + 1]
        c = list(random_columns(rng, n, 3 * n, truth, sorted_=True))
        c[0] = pos
        tk = rng.integers(0, n, n // 8)
        c[1][tk] = 0; c[2][tk] = 1
        c[4][tk] = (c[4][tk] & ~np.uint8(PASS)) | (np.floor(c[3][tk]) >= 20).astype(np.uint8)   # single-base now: kept iff QUAL >= 20, as everywhere
        cols.append(_cols(*c))
    t = _truth([(int(10 + 3 * i), 0, 1) for i in range(0, n, 5)] + [(int(p), int(r), int(a)) for p, r, a in zip(*truth)])
    _run(engine, oracle, cols, [t] * len(cols), expect_sorted=False)


@pytest.mark.parametrize("n,k", [(400, 399), (512, 300), (1024 + 400, 1024 + 399), (16384 + 512, 16384 + 511)])
def test_position_out_of_range_in_the_second_half_only(engine, n, k):
    import quasimodo_amd as q
    tid = engine.truth_load(np.array([5], np.int32), np.array([0], np.int32), np.array([1], np.int32))
    c = _ladder(n)
    c[0][k:] = 1 << 28                               # still ascending
    with pytest.raises(q.QmvtError) as ei:
        engine.classify_batch([_cols(*c)], [tid])
    assert ei.value.code == -5
    engine.truth_release(tid)


@pytest.mark.parametrize("n_bins", [1, 2, 20, 255, 256])
def test_roc_bins(engine, oracle, n_bins):
    """NaN, negative, fractional QUALs, QUALs exactly on a bin edge and far above the top bin; every record in the top bin (the
    ballot-counted path)."""
    rng = np.random.default_rng(2706)
    n = 1537
    L = 9000
    truth = random_truth(rng, 200, L)
    base = random_columns(rng, n, L, truth, sorted_=True)
    special = np.array([np.nan, -1.0, -0.5, -1e30, 0.0, 0.25, 0.999, 1.0, 1.5, 19.0, 19.999, 20.0, 254.0, 254.5, 255.0, 255.5, 256.0,
                        1e9, 3e38, np.inf, -np.inf, 1e-40, -1e-40, -0.0, n_bins - 1, n_bins - 0.5, n_bins, n_bins + 0.5], np.float32)
    mixed = list(base); mixed[3] = special[rng.integers(0, len(special), n)]
    top = list(base); top[3] = np.full(n, n_bins + 7, np.float32)
    edge = list(base); edge[3] = rng.integers(0, n_bins + 2, n).astype(np.float32)
    nan = list(base); nan[3] = np.full(n, np.nan, np.float32)
    snp = (base[1] < 4) & (base[2] < 4)
    for c in (mixed, top, edge, nan):                # kept iff single-base and QUAL >= 20, as everywhere (NaN: not kept)
        with np.errstate(invalid="ignore"):
            c[4] = (base[4] & ~np.uint8(PASS)) | (snp & (np.floor(c[3]) >= 20)).astype(np.uint8)
    _run(engine, oracle, [_cols(*c) for c in (mixed, top, edge, nan)], [truth] * 4, n_bins=n_bins)


def test_shuffled_records_through_the_packed_kernel_give_the_same_rows(engine, oracle):
    """The same records out of order take the radix sort and k_classify on its (key, info) pairs: ROC rows and scalars as the sorted run's."""
    rng = np.random.default_rng(2707)
    L = 40000
    truth = random_truth(rng, 2500, L)
    tid = engine.truth_load(*truth)
    cols, shuf = [], []
    for n in (513, 1537, 5000):
        c = random_columns(rng, n, L, truth, sorted_=True)
        o = rng.permutation(n)
        cols.append(c); shuf.append(tuple(np.ascontiguousarray(a[o]) for a in c))
    res, _ = engine.classify_batch(cols + shuf, [tid] * 6)
    for a, b, c in zip(res[:3], res[3:], cols):
        check_vcf(oracle, a, c, truth, expect_sorted=True)
        assert b["scalars"]["sorted"] == 0
        assert np.array_equal(a["roc"], b["roc"])
        for k in ("n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "truth_unique", "n_records"):
            assert a["scalars"][k] == b["scalars"][k], k
    engine.truth_release(tid)
