"""Near-miss classes of FP lines and missed truth keys (qm_batch_nearmiss, k_nearmiss_records / k_nearmiss_truth)
against a brute-force numpy restatement of the semantics: every record against every truth key, no index and no window walk.
Its inputs are the uploaded columns, the truth rows and the batch's own kept / TP bits (qm_batch_get_cls: the populations are
defined by them).  Equality is exact in counts, per-record bytes and per-key bytes."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, random_columns, random_truth

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_FP_LINES, S_TRUTH = 2, 7
F_PASS, F_IDDOT, F_NOKEY = 1, 2, 4
A, C, G, T = 0, 1, 2, 3
TOP = (1 << 28) - 1
NONE = 255
R_IDCOL, R_ALLELE, R_REFBASE, R_NEAR, R_ISOLATED, R_NOKEY = range(6)
T_FILTERED, T_ALLELE, T_POSITION, T_NEAR, T_UNCALLED = range(5)
KD = F_PASS | F_IDDOT


def span_records():
    """records per span of the batch layout (qmvt_dev.h: SPAN_TILES tiles of 256 * K1_ROUNDS records)"""
    src = open(os.path.join(ROOT, "quasimodo_amd", "csrc", "qmvt_dev.h")).read()
    d = {k: int(re.search(r"#define %s (\d+)" % k, src).group(1)) for k in ("QM_SPAN_TILES", "QM_K1_ROUNDS")}
    return d["QM_SPAN_TILES"] * 256 * d["QM_K1_ROUNDS"]


def truth_keys(truth):
    tp, tr, ta = (np.asarray(x, np.int64) for x in truth)
    ok = (tr >= 0) & (tr < 4) & (ta >= 0) & (ta < 4)
    return np.unique((tp[ok] << 4) | (tr[ok] << 2) | ta[ok])


def restate(cols, cls, tkeys, radius, rows=128):
    """(rcls uint8[n], tcls uint8[T'], hits bool[T'], intruth bool[n]): section 1 of the contract, record by key"""
    pos, ref, alt, _, fl = (np.asarray(x) for x in cols)
    n, nt = len(pos), len(tkeys)
    p = pos.astype(np.int64)
    usable = (fl & F_NOKEY) == 0
    single = (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4)
    cmp_ = usable & single
    nib = np.where(single, (ref.astype(np.int64) << 2) | alt.astype(np.int64), 0)
    kept = (cls & 1) != 0
    fpl = kept & ((cls & 2) == 0)
    tpos, tnib = tkeys >> 4, tkeys & 15
    rcls = np.full(n, NONE, np.uint8)
    intruth = np.zeros(n, bool)
    hit, pf, pa, pp, pn = (np.zeros(nt, bool) for _ in range(5))
    for r0 in range(0, n, rows):
        s = slice(r0, min(r0 + rows, n))
        d = tpos[None, :] - p[s, None]
        same = d == 0
        near = (np.abs(d) >= 1) & (np.abs(d) <= radius)
        c, u, k = cmp_[s, None], usable[s, None], kept[s, None]
        sameref = (tnib[None, :] >> 2) == (nib[s, None] >> 2)
        eq = same & c & (tnib[None, :] == nib[s, None])
        sra = same & c & sameref & ~eq
        # the record side, first class that applies
        r_in = eq.any(1)
        r_allele = sra.any(1)
        r_refbase = same.any(1) & ~(same & sameref).any(1)
        r_near = ~same.any(1) & near.any(1)
        rc = np.where(~cmp_[s], R_NOKEY, np.where(r_in, R_IDCOL, np.where(r_allele, R_ALLELE, np.where(r_refbase, R_REFBASE,
                      np.where(r_near, R_NEAR, R_ISOLATED)))))
        rcls[s] = np.where(fpl[s], rc, NONE)
        intruth[s] = kept[s] & r_in
        # the truth side: what the records say about every key
        hit |= (eq & k).any(0)
        pf |= (eq & ~k).any(0)
        pa |= sra.any(0)
        pp |= (same & u & ((c & ~sameref) | ~single[s, None])).any(0)
        pn |= (near & u).any(0)
    tc = np.where(hit, NONE, np.where(pf, T_FILTERED, np.where(pa, T_ALLELE, np.where(pp, T_POSITION, np.where(pn, T_NEAR, T_UNCALLED)))))
    return rcls, tc.astype(np.uint8), hit, intruth


def run_batch(engine, cols, tids, alleles=False):
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b


def check(b, cols, truths_of_vcf, radius, want=None):
    """one qm_batch_nearmiss against the restatement, every VCF, with the invariants; returns (rec, tru, [rcls], [tcls])"""
    rec, tru = b.nearmiss(radius)
    sc = b.scalars()
    assert rec.shape == (b.n_vcf, 6) and tru.shape == (b.n_vcf, 5)
    rcs, tcs = [], []
    for v, c in enumerate(cols):
        tk = truth_keys(truths_of_vcf[v])
        cls = b.cls(v)
        w_rcls, w_tcls, w_hit, w_intruth = want[v] if want else restate(c, cls, tk, radius)
        hits = b.truth_hit_bits(v)
        assert np.array_equal(hits, w_hit), "VCF %d: the hit bitmap against the restatement" % v
        assert np.array_equal(b.intruth_mask(v), w_intruth & ((c[4] & F_NOKEY) == 0)), "VCF %d: mask_intruth" % v
        g_rcls, g_tcls = b.nearmiss_classes(v), b.nearmiss_truth(v)
        bad = np.flatnonzero(g_rcls != w_rcls)
        assert bad.size == 0, "VCF %d radius %d: record %d is %d, restated %d" % (v, radius, bad[0], g_rcls[bad[0]], w_rcls[bad[0]])
        bad = np.flatnonzero(g_tcls != w_tcls)
        assert bad.size == 0, "VCF %d radius %d: key %d is %d, restated %d" % (v, radius, bad[0], g_tcls[bad[0]], w_tcls[bad[0]])
        assert rec[v].tolist() == np.bincount(w_rcls[w_rcls != NONE], minlength=6).tolist(), "VCF %d: record-side counts" % v
        assert tru[v].tolist() == np.bincount(w_tcls[w_tcls != NONE], minlength=5).tolist(), "VCF %d: truth-side counts" % v
        # the invariants
        assert int(rec[v].sum()) == int(sc[v, S_FP_LINES])
        assert np.array_equal(g_rcls != NONE, ((cls & 1) != 0) & ((cls & 2) == 0))
        assert int(sc[v, S_TRUTH]) == len(tk) and int(tru[v].sum()) == len(tk) - int(hits.sum())
        assert np.array_equal(g_tcls == NONE, hits)
        rcs.append(g_rcls)
        tcs.append(g_tcls)
    return rec, tru, rcs, tcs


def _cols(recs):
    return tuple(np.array([r[k] for r in recs], dt) for k, dt in enumerate((np.int32, np.int32, np.int32, np.float32, np.uint8)))


def _sorted(c):
    o = np.argsort(c[0], kind="stable")
    return tuple(np.ascontiguousarray(x[o]) for x in c)


def _distinct_truth(rng, t, genome_len):
    """exactly t distinct single-base keys over positions 1 .. genome_len"""
    k = rng.choice(genome_len * 16, size=t, replace=False).astype(np.int64)
    return ((k >> 4) + 1).astype(np.int32), ((k >> 2) & 3).astype(np.int32), (k & 3).astype(np.int32)


class Truths:
    """truth sets loaded for one test and released behind it"""

    def __init__(self, engine):
        self.engine, self.ids = engine, []

    def __enter__(self):
        return self

    def load(self, truth):
        self.ids.append(self.engine.truth_load(*truth))
        return self.ids[-1]

    def __exit__(self, *a):
        for t in self.ids:
            self.engine.truth_release(t)


def test_hand_written_case_every_class_once(engine):
    """a dozen records, eight truth keys, radius 2, literal expectations"""
    truth = (np.array([10, 20, 30, 40, 50, 60, 70, 90], np.int32), np.array([A, A, C, G, T, A, C, G], np.int32),
             np.array([C, C, G, T, A, G, T, C], np.int32))
    recs = [(10, A, C, 99, KD),                 # a TP line
            (20, A, C, 99, F_PASS),             # kept, key in the truth set, ID not '.': no TP line -> idcol; the key is hit
            (20, A, C, 99, KD),                 # the same key as a TP line
            (30, C, G, 17, F_IDDOT),            # called and dropped by the filter -> the key is `filtered`
            (40, G, A, 99, KD),                 # the right position and ref, another alt -> allele / allele
            (50, C, A, 99, KD),                 # the right position, another ref base -> refbase / position
            (60, A, 5, 17, F_IDDOT),            # alleles that are not single bases at a truth position -> position
            (72, C, T, 99, KD),                 # two bases off a key -> near / near
            (73, C, T, 99, KD),                 # three off: outside the radius -> isolated
            (80, A, T, 99, KD),                 # nothing around -> isolated
            (85, A, C, 99, KD | F_NOKEY),       # a kept line without a comparable key -> nokey
            (91, G, C, 17, F_IDDOT | F_NOKEY)]  # not kept, no usable position: ignored, key 90 stays `uncalled`
    cols = _cols(recs)
    with Truths(engine) as ts:
        tid = ts.load(truth)
        b = run_batch(engine, [cols], [tid])
        b.truth_hits()
        assert b.cls(0).tolist() == [3, 1, 3, 0, 1, 1, 0, 1, 1, 1, 1, 0]
        rec, tru, rcs, tcs = check(b, [cols], [truth], 2)
        assert rcs[0].tolist() == [NONE, R_IDCOL, NONE, NONE, R_ALLELE, R_REFBASE, NONE, R_NEAR, R_ISOLATED, R_ISOLATED, R_NOKEY, NONE]
        assert tcs[0].tolist() == [NONE, NONE, T_FILTERED, T_ALLELE, T_POSITION, T_POSITION, T_NEAR, T_UNCALLED]
        assert rec[0].tolist() == [1, 1, 1, 1, 2, 1] and tru[0].tolist() == [1, 1, 2, 1, 1]
        b.close()


def test_record_counts_tail_byte_lane_stride_and_more_than_four_spans(engine):
    span = span_records()
    sizes = [0, 1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4 * span + 9]
    rng = np.random.default_rng(141)
    L = 6000
    truth = random_truth(rng, 700, L)
    cols = [random_columns(rng, n, L, truth, frac_truth=0.25, near_frac=0.15) for n in sizes]
    with Truths(engine) as ts:
        tid = ts.load(truth)
        b = run_batch(engine, cols, [tid] * len(cols))
        b.truth_hits()
        rec, _, _, _ = check(b, cols, [truth] * len(cols), 3)
        assert rec[-1].sum() > span and not rec[0].any()
        b.close()


def test_several_truth_sets_inside_one_workgroup_and_a_vcf_without_fp_lines(engine):
    """every VCF here is one span, so the first four share a workgroup: the planes and counts are flushed at every change"""
    rng = np.random.default_rng(142)
    L = 3000
    truths = [random_truth(rng, t, L) for t in (200, 90, 400)]
    order = [0, 1, 0, 2, 1, 2]
    cols = [random_columns(rng, n, L, truths[k], near_frac=0.2) for n, k in zip((300, 200, 0, 500, 100, 257), order)]
    quiet = list(random_columns(rng, 200, L, truths[1], near_frac=0.2))
    quiet[4] = (quiet[4] & ~np.uint8(F_PASS)).astype(np.uint8)   # nothing kept: no FP line, but its records still feed the truth side
    cols[1] = tuple(quiet)
    with Truths(engine) as ts:
        tids = [ts.load(t) for t in truths]
        b = run_batch(engine, cols, [tids[k] for k in order])
        b.truth_hits()
        rec, tru, _, _ = check(b, cols, [truths[k] for k in order], 5)
        assert not rec[1].any() and tru[1][T_FILTERED] > 0 and rec[0].any() and rec[3].any()
        b.close()


def test_truth_sets_of_0_1_31_32_33_keys(engine):
    rng = np.random.default_rng(143)
    L = 400
    sizes = (0, 1, 31, 32, 33)
    truths = [_distinct_truth(rng, t, L) for t in sizes]
    cols = [random_columns(rng, 500, L, t, near_frac=0.1) for t in truths]
    with Truths(engine) as ts:
        tids = [ts.load(t) for t in truths]
        b = run_batch(engine, cols, tids)
        b.truth_hits()
        _, tru, _, tcs = check(b, cols, truths, 4)
        assert [len(t) for t in tcs] == list(sizes) and not tru[0].any()
        b.close()


def test_truth_sets_on_both_sides_of_the_lds_split(engine):
    """32 768 keys stay in the LDS planes, 32 769 take global atomics; one restatement for both"""
    rng = np.random.default_rng(144)
    L = 40000
    truths = [_distinct_truth(rng, t, L) for t in (32768, 32769)]
    cols = [random_columns(rng, 3000, L, t, frac_truth=0.3, near_frac=0.1) for t in truths]
    with Truths(engine) as ts:
        tids = [ts.load(t) for t in truths]
        b = run_batch(engine, cols, tids)
        b.truth_hits()
        _, tru, _, tcs = check(b, cols, truths, 2)
        assert [len(t) for t in tcs] == [32768, 32769] and all(tru[v, :4].all() for v in range(2))
        b.close()


def test_dense_truth_set_bounds_the_walk(engine):
    """all 12 single-base keys at each of 2 * radius + 1 consecutive positions, radius 64"""
    radius, base = 64, 5000
    tp, tr, ta = zip(*[(base + d, r, a) for d in range(2 * radius + 1) for r in range(4) for a in range(4) if r != a])
    truth = (np.array(tp, np.int32), np.array(tr, np.int32), np.array(ta, np.int32))
    rng = np.random.default_rng(145)
    n = 600
    pos = rng.integers(base - 80, base + 2 * radius + 80, n).astype(np.int32)
    pos[:3] = (base + radius, base - radius, base + 3 * radius)
    ref, alt = rng.integers(0, 4, n).astype(np.int32), rng.integers(0, 5, n).astype(np.int32)
    fl = np.where(rng.random(n) < 0.6, KD, F_IDDOT).astype(np.uint8)
    fl[rng.random(n) < 0.1] &= np.uint8(~F_IDDOT & 0xff)
    cols = _sorted((pos, ref, alt, np.full(n, 50, np.float32), fl))
    with Truths(engine) as ts:
        tid = ts.load(truth)
        b = run_batch(engine, [cols], [tid])
        b.truth_hits()
        _, tru, _, tcs = check(b, [cols], [truth], radius)
        assert len(tcs[0]) == 12 * (2 * radius + 1) and tru[0][T_UNCALLED] == 0
        b.close()


def test_windows_across_index_cells_and_at_both_ends_of_the_position_range(engine):
    """radius 64.  With keys up to 2^28 - 1 a cell of the coarse index holds 4 096 positions: windows that straddle a cell
    boundary, start before cell 0 (pos 0, 1) and end beyond the last cell (2^28 - 1, 2^28 - 2); with a low truth set, windows
    that start in its last cell and end beyond it, and records far beyond every cell."""
    wide = [(0, A, C), (1, C, G), (30, G, T), (4090, A, G), (4095, C, T), (4096, T, A), (4100, G, A), (8191, A, T), (8200, C, A),
            (TOP - 70, A, C), (TOP - 64, C, A), (TOP - 1, G, C), (TOP, T, G)]
    low = [(5, A, C), (990, C, G), (1000, G, T)]
    truths = [tuple(np.array(x, np.int32) for x in zip(*t)) for t in (wide, low)]
    rp = [0, 1, 2, 40, 64, 65, 95, 4030, 4031, 4032, 4095, 4096, 4097, 4159, 4160, 4161, 8127, 8128, 8192, 8255, 8264, 8265, 100000,
          TOP - 135, TOP - 134, TOP - 128, TOP - 65, TOP - 64, TOP - 2, TOP - 1, TOP]
    recs = []
    for i, p in enumerate(rp):
        recs.append((p, i & 3, (i + 1 + i // 4) & 3, 99, KD))
        recs.append((p, (i + 2) & 3, 4 if i % 5 == 0 else i & 3, 10, F_IDDOT))          # not kept; some with other alleles
    c_wide = _cols(recs)
    recs = [(p, A, C, 99, KD) for p in (0, 5, 6, 925, 926, 1000, 1001, 1064, 1065, 1100, 5000, TOP)]
    c_low = _cols(recs)
    with Truths(engine) as ts:
        tids = [ts.load(t) for t in truths]
        b = run_batch(engine, [c_wide, c_low], tids)
        b.truth_hits()
        _, tru, rcs, _ = check(b, [c_wide, c_low], truths, 64)
        assert rcs[1].tolist() == [R_NEAR, NONE, R_NEAR, R_ISOLATED, R_NEAR, R_REFBASE, R_NEAR, R_NEAR, R_ISOLATED, R_ISOLATED, R_ISOLATED,
                                   R_ISOLATED]
        b.close()


def test_radius_only_moves_isolated_to_near_and_uncalled_to_near(engine):
    rng = np.random.default_rng(147)
    L = 20000
    truth = random_truth(rng, 400, L)
    cols = [random_columns(rng, 1500, L, truth, near_frac=0.1), random_columns(rng, 700, L, truth, sorted_=False)]
    with Truths(engine) as ts:
        tid = ts.load(truth)
        b = run_batch(engine, cols, [tid, tid])
        b.truth_hits()
        prev = None
        for radius in (0, 1, 10, 64):
            rec, tru, rcs, tcs = check(b, cols, [truth, truth], radius)
            if radius == 0:
                assert not rec[:, R_NEAR].any() and not tru[:, T_NEAR].any()
            if prev is not None:
                prec, ptru, prcs, ptcs = prev
                for v in range(2):
                    moved = prcs[v] != rcs[v]
                    assert (prcs[v][moved] == R_ISOLATED).all() and (rcs[v][moved] == R_NEAR).all()
                    moved = ptcs[v] != tcs[v]
                    assert (ptcs[v][moved] == T_UNCALLED).all() and (tcs[v][moved] == T_NEAR).all()
                assert (rec[:, R_NEAR] >= prec[:, R_NEAR]).all() and (tru[:, T_NEAR] >= ptru[:, T_NEAR]).all()
                assert np.array_equal(np.delete(rec, [R_NEAR, R_ISOLATED], 1), np.delete(prec, [R_NEAR, R_ISOLATED], 1))
                assert np.array_equal(np.delete(tru, [T_NEAR, T_UNCALLED], 1), np.delete(ptru, [T_NEAR, T_UNCALLED], 1))
            prev = (rec, tru, rcs, tcs)
        assert prev[0][:, R_NEAR].all() and prev[1][:, T_NEAR].all()
        b.close()


def test_a_shuffled_vcf_and_its_sorted_copy(engine):
    rng = np.random.default_rng(148)
    L = 9000
    truth = random_truth(rng, 600, L)
    shuffled = random_columns(rng, 5000, L, truth, sorted_=False, near_frac=0.1, weird=False)
    o = np.argsort(shuffled[0], kind="stable")
    ordered = tuple(np.ascontiguousarray(x[o]) for x in shuffled)
    with Truths(engine) as ts:
        tid = ts.load(truth)
        b = run_batch(engine, [shuffled, ordered], [tid, tid])
        b.truth_hits()
        rec, tru, rcs, tcs = check(b, [shuffled, ordered], [truth, truth], 7)
        assert np.array_equal(rec[0], rec[1]) and np.array_equal(tru[0], tru[1])
        assert np.array_equal(rcs[0][o], rcs[1]) and np.array_equal(tcs[0], tcs[1])
        b.close()


def test_refusals_by_their_codes(engine):
    from quasimodo_amd import QmvtError
    rng = np.random.default_rng(149)
    L = 3000
    truth = random_truth(rng, 100, L)
    cols = [random_columns(rng, 400, L, truth, weird=False) for _ in range(2)]

    def code(fn):
        with pytest.raises(QmvtError) as e:
            fn()
        return e.value.code
    with Truths(engine) as ts:
        tid = ts.load(truth)
        b = engine.batch([len(c[0]) for c in cols], [tid, tid])
        for v, c in enumerate(cols):
            b.upload(v, *c)
        assert code(lambda: b.nearmiss(2)) == QM_E_STATE                     # nothing ran
        b.run()
        assert code(lambda: b.nearmiss(2)) == QM_E_STATE                     # not finished
        b.finish()
        assert code(lambda: b.nearmiss(2)) == QM_E_STATE                     # no truth_hits behind the run
        assert code(b.nearmiss_counts) == QM_E_STATE                         # a getter before any pass
        assert code(lambda: b.nearmiss_classes(0)) == QM_E_STATE
        assert code(lambda: b.nearmiss_truth(0)) == QM_E_STATE
        b.truth_hits()
        assert code(b.nearmiss_counts) == QM_E_STATE
        assert code(lambda: b.nearmiss(-1)) == QM_E_INVAL
        assert code(lambda: b.nearmiss(65)) == QM_E_INVAL
        check(b, cols, [truth, truth], 64)
        check(b, cols, [truth, truth], 0)                                    # repeated with another radius
        before = b.device_bytes
        b.nearmiss(3)
        assert b.device_bytes == before                                      # the outputs were allocated once, and counted
        b.run()
        b.finish()
        assert code(b.nearmiss_counts) == QM_E_STATE                         # the batch ran since the pass
        assert code(lambda: b.nearmiss_classes(0)) == QM_E_STATE
        assert code(lambda: b.nearmiss_truth(0)) == QM_E_STATE
        assert code(lambda: b.nearmiss(2)) == QM_E_STATE                     # ... and the hit bitmaps are stale too
        b.truth_hits()
        check(b, cols, [truth, truth], 2)
        b.close()
        bx = run_batch(engine, cols, [tid, tid], alleles=True)               # an allele-extended batch
        assert code(lambda: bx.nearmiss(2)) == QM_E_STATE
        bx.close()
