"""The filter surface (qm_batch_surface: k_surface_records / k_surface_truth / k_surface_sums) against a numpy
restatement written from the semantics alone: per record the single-base test, the key's index in the truth set (a dict), the
TP rule, the quality bin and the AF bin (one float32 multiply); per truth key the lexicographically largest (qb, ab) of its
'.'-ID records; 2-D suffix sums.  No helper is shared with the binding.  Every count is an integer and compared exactly."""
import numpy as np
import pytest

from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8
STAGE = 4096                      # qmvt_surface.h SF_STAGE: truth sets up to here stage their best codes in LDS
GENOME = 5000
PARAMS = [(1, 256, 8), (4, 64, 50), (1, 1, 1), (7, 3, 64), (1, 64, 64)]
SIZES = [0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 3, 1023, 1024, 1025, 4095, 4096, 16384, 16385]   # 1023 .. 1025: a step of the span walk; 16 384: a span
TRUTH_SIZES = [0, 1, 31, 32, 33, STAGE - 1, STAGE, STAGE + 1]
N_BINS = 256


def _f32_pool():
    """the QUAL and AF values the issue names, for every grid of PARAMS"""
    f = np.float32
    q = [f(np.nan), f(-np.inf), f(-1), f(-0.5), f(0), f(0.99), f(19.99), f(20), f(1e9), f(np.inf)]
    for step in sorted({p[0] for p in PARAMS}):
        for i in range(1, 70):
            v = f(step * i)
            q += [v, np.nextafter(v, f(0))]           # q_step * i and the float just below it
    a = [f(np.nan), f(-0.1), f(0), f(0.999), f(1.0), f(1.5)]
    for na in sorted({p[2] for p in PARAMS}):
        for k in range(na + 1):
            v = f(k) / f(na)
            a += [v, np.nextafter(v, f(0)), np.nextafter(v, f(2))]   # k / na and its two float32 neighbours
    return np.array(q, np.float32), np.array(a, np.float32)


def _truth(rng, t):
    """exactly t distinct single-base keys over positions 1 .. GENOME"""
    k = np.sort(rng.choice(GENOME * 16, size=t, replace=False)).astype(np.int64)
    return ((k >> 4) + 1).astype(np.int32), ((k >> 2) & 3).astype(np.int32), (k & 3).astype(np.int32)


def _vcf(rng, n, truth, qpool, apool, shuffle):
    tpos, tref, talt = truth
    pos = rng.integers(1, GENOME + 1, size=n).astype(np.int32)
    ref = rng.integers(0, 4, size=n).astype(np.int32)
    alt = rng.integers(0, 4, size=n).astype(np.int32)
    cross = len(tpos) >= 4 and n > 12                                # the first two keys and the last are kept for the crossing records
    if len(tpos) and n:
        take = rng.random(n) < 0.45                                  # a truth key, often the same one several times
        j = rng.integers(2, len(tpos) - 1, size=n) if cross else rng.integers(0, len(tpos), size=n)
        pos, ref, alt = (np.where(take, t[j], x).astype(np.int32) for t, x in ((tpos, pos), (tref, ref), (talt, alt)))
    if n:
        alt = np.where(rng.random(n) < 0.08, rng.integers(4, 9, size=n), alt).astype(np.int32)   # not single bases
        ref = np.where(rng.random(n) < 0.03, -1, ref).astype(np.int32)
    qual = qpool[rng.integers(0, len(qpool), size=n)]
    af = apool[rng.integers(0, len(apool), size=n)]
    if cross:
        # keys with two or three records whose (QUAL, AF) cross: high QUAL / low AF, low QUAL / high AF, and one between
        for m, (q, a) in enumerate(((200, 0.05), (30, 0.95), (100, 0.5), (200, 0.02), (30, 0.99), (21, 0.999), (199.5, 0.3), (2, 1.0), (250, 0))):
            k = (m // 3) % len(tpos) if m < 6 else len(tpos) - 1
            pos[m], ref[m], alt[m], qual[m], af[m] = tpos[k], tref[k], talt[k], q, a
    snp = (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4)
    with np.errstate(invalid="ignore"):
        passed = snp & (np.floor(qual.astype(np.float64)) >= 20)
    fl = passed.astype(np.uint8) | ((rng.random(n) > 0.15).astype(np.uint8) << 1) | ((rng.random(n) < 0.04).astype(np.uint8) << 2) | \
        ((rng.random(n) < 0.04).astype(np.uint8) << 3)                # ID '.' or not; NOKEY; TPLINE, with and without a hit
    if cross:
        fl[:9] |= F_IDDOT
        fl[:9] &= ~np.uint8(F_NOKEY)
    o = rng.permutation(n) if shuffle else np.argsort(pos, kind="stable")
    cols = tuple(np.ascontiguousarray(x[o]) for x in (pos, ref, alt, qual.astype(np.float32), fl.astype(np.uint8)))
    return cols, np.ascontiguousarray(af[o].astype(np.float32))


class Case:
    pass


@pytest.fixture(scope="module")
def case(engine):
    """one batch of 48 VCFs over eight truth sets, finished; the per-record facts that no parameter changes are restated once"""
    rng = np.random.default_rng(1615)
    qpool, apool = _f32_pool()
    c = Case()
    c.truths = [_truth(rng, t) for t in TRUTH_SIZES]
    c.tids = [engine.truth_load(*t) for t in c.truths]
    # neighbours of different truth sets, short enough to share a workgroup; the two long VCFs last
    sizes = SIZES + [5, 300, 12, 700, 40, 1000, 3, 129, 513, 31, 90, 17, 2500, 1, 33, 260, 64, 999, 10, 4097, 250, 15, 77, 1500] + [70000, 300000]
    c.which = [v % len(TRUTH_SIZES) for v in range(len(sizes))]
    c.which[-2], c.which[-1] = TRUTH_SIZES.index(STAGE), TRUTH_SIZES.index(STAGE + 1)     # a staged and an unstaged truth set
    made = [_vcf(rng, n, c.truths[w], qpool, apool, shuffle=(v % 2 == 1)) for v, (n, w) in enumerate(zip(sizes, c.which))]
    c.cols, c.af = [m[0] for m in made], [m[1] for m in made]
    c.no_af = 29                                                       # this VCF's frequencies are never uploaded
    c.af[c.no_af] = None
    assert len(sizes) == 48 and len(c.cols[c.no_af][0]) > 0
    b = engine.batch([len(x[0]) for x in c.cols], [c.tids[w] for w in c.which], n_bins=N_BINS)
    for v, x in enumerate(c.cols):
        b.upload(v, *x)
        if c.af[v] is not None:
            b.upload_af(v, c.af[v])
    b.run()
    b.finish()
    c.b = b
    # per record: snp, the key's index j, is_tp, and whether it may be a key's best record
    c.tkeys = [[(int(p) << 4) | (int(r) << 2) | int(a) for p, r, a in zip(*t)] for t in c.truths]
    c.facts = []
    for v, (pos, ref, alt, qual, fl) in enumerate(c.cols):
        index = {k: i for i, k in enumerate(sorted(set(c.tkeys[c.which[v]])))}
        snp = (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4)
        j = np.full(len(pos), -1, np.int64)
        for i in range(len(pos)):
            if snp[i] and not fl[i] & F_NOKEY:
                j[i] = index.get((int(pos[i]) << 4) | (int(ref[i]) << 2) | int(alt[i]), -1)
        dot = (fl & F_IDDOT) != 0
        c.facts.append((snp, j, ((j >= 0) & dot) | (snp & ((fl & F_TPLINE) != 0)), (j >= 0) & dot, len(index)))
    yield c
    b.close()
    for t in c.tids:
        engine.truth_release(t)


def restate(case, v, q_step, nq, na):
    """(S [3][nq][na], extra [4]) of VCF v from the Semantics section"""
    snp, j, is_tp, dot_hit, tn = case.facts[v]
    qual, af = case.cols[v][3], case.af[v]
    n = len(qual)
    limit = nq * q_step
    with np.errstate(invalid="ignore"):
        fq = np.floor(qual.astype(np.float64))
        b = np.where(np.isnan(qual) | (fq < 0), -1, np.minimum(fq, limit - 1)).astype(np.int64)
        qb = b // q_step
        if af is None:
            af = np.full(n, np.nan, np.float32)
        nan_af = np.isnan(af)
        prod = af * np.float32(na)                                      # ONE float32 multiply
        assert prod.dtype == np.float32
        ab = np.where(nan_af | (af < 0), 0, np.minimum(na - 1, np.where(nan_af | (af < 0), 0, prod).astype(np.int64)))
    counted = snp & (b >= 0)
    G = np.zeros((3, nq, na), np.int64)
    i = np.flatnonzero(counted)
    np.add.at(G, (np.where(is_tp[i], 0, 1), qb[i], ab[i]), 1)
    # every truth key at its best record: its '.'-ID records in the order (key, qb, ab), the last of every key
    i = np.flatnonzero(counted & dot_hit)
    i = i[np.lexsort((ab[i], qb[i], j[i]))]
    if len(i):
        i = i[np.append(j[i][1:] != j[i][:-1], True)]
        np.add.at(G[2], (qb[i], ab[i]), 1)
    S = G[:, ::-1, ::-1].cumsum(1).cumsum(2)[:, ::-1, ::-1]
    extra = [int(counted.sum()), int((counted & nan_af).sum()), int((snp & (b < 0)).sum()), tn]
    return S, extra


@pytest.mark.parametrize("q_step,nq,na", PARAMS)
def test_surface_equals_the_restatement(case, q_step, nq, na):
    b = case.b
    S, extra = b.surface(q_step, nq, na)
    assert S.shape == (48, 3, nq, na) and extra.shape == (48, 4) and S.dtype == np.uint64
    roc = b.roc()
    lines = [i for i in range(nq) if i * q_step < N_BINS]
    some_u = some_fp = 0
    for v in range(48):
        wS, wx = restate(case, v, q_step, nq, na)
        g = S[v].astype(np.int64)
        bad = np.argwhere(g != wS)
        assert bad.size == 0, "VCF %d (%d records): S%s is %d, restated %d" % (v, len(case.cols[v][0]), tuple(bad[0]), g[tuple(bad[0])], wS[tuple(bad[0])])
        assert extra[v].tolist() == wx, "VCF %d: extra" % v
        # the QUAL ROC of the classification is the surface's AF >= 0 column
        for c in range(3):
            assert g[c, lines, 0].tolist() == [int(roc[v, c, i * q_step]) for i in lines], "VCF %d grid %d against roc" % (v, c)
        # monotone along both axes, and no more found keys than TP records
        assert (np.diff(g, axis=1) <= 0).all() and (np.diff(g, axis=2) <= 0).all() and (g[2] <= g[0]).all()
        assert int(g[0, 0, 0] + g[1, 0, 0]) == wx[0] and int(g[2, 0, 0]) <= wx[3]
        some_u += int(g[2, 0, 0])
        some_fp += int(g[1, 0, 0])
    assert some_u > 3000 and some_fp > 100000                          # the case is not empty
    assert int(extra[case.no_af, 1]) == int(extra[case.no_af, 0]) > 0 and not S[case.no_af][:, :, 1:].any()   # no upload: every record without AF
    assert not S[0].any() and extra[0].tolist() == [0, 0, 0, 0]                                              # the empty VCF of the empty truth set


def test_crossing_duplicates_are_represented_by_the_higher_qual(case):
    """a key with a (QUAL 200, AF 0.05) and a (QUAL 30, AF 0.95) record is found at (200, 0.05): under QUAL >= 30 and AF >= 0.5
    its low-QUAL record passes, and the key is still not counted there"""
    v = len(SIZES) + 5                                                  # 1 000 records, shuffled, 32 truth keys
    assert len(case.cols[v][0]) == 1000 and case.facts[v][4] == 32
    S, _ = case.b.surface(1, 256, 8)
    wS, _ = restate(case, v, 1, 256, 8)
    assert np.array_equal(S[v].astype(np.int64), wS)
    snp, j, is_tp, dot_hit, tn = case.facts[v]
    pos, ref, alt, qual, fl = case.cols[v]
    key0 = int(j[np.flatnonzero((qual == 200) & np.isclose(case.af[v], 0.05) & dot_hit)[0]])
    recs = np.flatnonzero((j == key0) & dot_hit)
    assert {(float(qual[i]), round(float(case.af[v][i]), 2)) for i in recs} >= {(200.0, 0.05), (30.0, 0.95), (100.0, 0.5)}
    # leave key0's records out: U loses the key exactly where QUAL <= best qb and AF <= best ab, nowhere else
    best_q = max(int(min(np.floor(qual[i]), 255)) for i in recs if qual[i] >= 0)
    best_a = max(min(7, int(np.float32(case.af[v][i]) * np.float32(8))) for i in recs if int(min(np.floor(qual[i]), 255)) == best_q)
    keep = np.ones(len(pos), bool)
    keep[recs] = False
    saved = case.cols[v], case.af[v], case.facts[v]
    try:
        case.cols[v] = tuple(x[keep] for x in saved[0])
        case.af[v] = saved[1][keep]
        case.facts[v] = (snp[keep], j[keep], is_tp[keep], dot_hit[keep], tn)
        without, _ = restate(case, v, 1, 256, 8)
    finally:
        case.cols[v], case.af[v], case.facts[v] = saved
    d = wS[2] - without[2]
    want = np.zeros((256, 8), np.int64)
    want[:best_q + 1, :best_a + 1] = 1
    assert best_q >= 200 and np.array_equal(d, want)
    assert d[30, 4] == 0                                                # QUAL >= 30, AF >= 0.5: a record of the key passes, the key is not counted


def test_counts_survive_a_second_call_and_other_passes(case):
    b = case.b
    S1, x1 = b.surface(4, 64, 50)
    S2, x2 = b.surface(4, 64, 50)
    assert np.array_equal(S1, S2) and np.array_equal(x1, x2)
    b.truth_hits()
    b.nearmiss(3)
    S3, x3 = b.surface_counts()
    assert np.array_equal(S1, S3) and np.array_equal(x1, x3)
    b.set_timing(True)
    try:
        S4, _ = b.surface(4, 64, 50)
        t = b.surface_timings()
    finally:
        b.set_timing(False)
    assert np.array_equal(S1, S4) and sorted(t) == ["surface_records_ms", "surface_sums_ms", "surface_truth_ms"] and all(x >= 0 for x in t.values())
    with pytest.raises(QmvtError) as e:
        b.surface(4, 64, 50)
        b.surface_timings()
    assert e.value.code == QM_E_STATE                                   # timing is off again


def test_device_bytes_grow_by_the_best_array_at_the_first_call_only(engine, case):
    rng = np.random.default_rng(5)
    qpool, apool = _f32_pool()
    w = TRUTH_SIZES.index(33)
    made = [_vcf(rng, n, case.truths[w], qpool, apool, False) for n in (100, 0, 300)]
    b = engine.batch([100, 0, 300], [case.tids[w]] * 3, n_bins=N_BINS)
    try:
        for v, (cols, af) in enumerate(made):
            b.upload(v, *cols)
        b.run()
        b.finish()
        before = b.device_bytes                                         # a batch that never asks has allocated nothing for the pass
        b.surface(4, 64, 50)
        first = b.device_bytes - before
        best = 4 * 3 * 33                                               # one u32 per (VCF, truth key)
        tables = 8 * 3 * (3 * 64 * 50 + 4) + 8 * (3 + 1) + 3            # the grids and extras, the row offsets, the AF marks
        assert first == best + tables
        b.surface(4, 64, 50)
        b.surface(1, 32, 8)                                             # a smaller grid fits what is there
        assert b.device_bytes - before == first
    finally:
        b.close()


def test_refusals(engine, case):
    rng = np.random.default_rng(6)
    qpool, apool = _f32_pool()
    w = TRUTH_SIZES.index(33)
    cols, af = _vcf(rng, 50, case.truths[w], qpool, apool, False)
    b = engine.batch([50], [case.tids[w]], n_bins=N_BINS)
    try:
        b.upload(0, *cols)
        with pytest.raises(QmvtError, match="qm_batch_run") as e:       # an unfinished batch
            b.surface()
        assert e.value.code == QM_E_STATE
        b.run()
        with pytest.raises(QmvtError) as e:
            b.surface()
        assert e.value.code == QM_E_STATE
        b.finish()
        for args, word in (((1, 241, 17), r"nq \* na = 4097"), ((0, 64, 50), "q_step 0"), ((4, 257, 1), "nq 257"), ((4, 1, 65), "na 65"),
                           ((4, 0, 50), "nq 0"), ((4, 64, 0), "na 0"), ((-1, 64, 50), "q_step -1")):
            with pytest.raises(QmvtError, match=word) as e:
                b.surface(*args)
            assert e.value.code == QM_E_INVAL
        with pytest.raises(QmvtError) as e:                             # nothing was made: nothing to get
            b.surface_counts()
        assert e.value.code == QM_E_STATE
        S, x = b.surface(1, 64, 64)                                     # 4096 cells is inside the limit
        assert S.shape == (1, 3, 64, 64) and int(x[0, 3]) == 33
        b.run()
        b.finish()
        with pytest.raises(QmvtError) as e:                             # the batch ran since
            b.surface_counts()
        assert e.value.code == QM_E_STATE
    finally:
        b.close()
    x = engine.batch([50], [case.tids[w]], n_bins=N_BINS, alleles=True)
    try:
        x.upload(0, *cols)
        x.run()
        x.finish()
        with pytest.raises(QmvtError, match="allele-extended") as e:
            x.surface()
        assert e.value.code == QM_E_STATE
    finally:
        x.close()
