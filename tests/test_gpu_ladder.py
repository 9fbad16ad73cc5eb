"""The four rescues combined on the device (qm_batch_ladder; k_ladder_records / k_ladder_truth) against the
restatement of quasimodo_amd.ladder: counts, mask bytes and entry bytes, exactly -- on the draws of the rescue-ROC sweep (VCFs of
0 .. 16 385 records, truth sets of 1, 65 and 2000 entries on two genomes, one VCF without a genome, sorted and shuffled) and on
the planted family of ladder_family.py, where every method bit and the pairs are reached; with and without the subset search and
the columns; the identities against the producers' own getters; 4096 lines in one cell; SNVs alone; the state rules."""
import numpy as np
import pytest

from quasimodo_amd import _lib
from quasimodo_amd import haplo as hp
from quasimodo_amd import ladder as ld
from quasimodo_amd import normalize as nz
from quasimodo_amd._lib import QmvtError
from haplo_family import truth_codes
from ladder_family import LadderFamily
import rescueroc_family as fam

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
B = ld.M_B


class Run:
    """one finished allele-extended batch with the four producers (with their columns) behind it"""

    def __init__(self, engine, genomes, truths, cols, which, norm_none=(), hap_none=(), produce=True, gap=None):
        self.engine = engine
        self.tids = [engine.truth_load(*t) for t in truths]
        self.gids = [engine.genome_load(g.encode()) for g in genomes]
        self.b = engine.batch([len(c[0]) for c in cols], [self.tids[w] for w in which], alleles=True)
        try:
            for v, c in enumerate(cols):
                self.b.upload(v, *c)
            self.b.run()
            self.b.finish()
            self.masks = []
            for v in range(self.b.n_vcf):
                m = self.b.cls(v)
                self.masks.append(((m & 1).astype(bool), (m & 2).astype(bool)))
            self.gids_n = [-1 if v in norm_none else self.gids[w] for v, w in enumerate(which)]
            self.gids_h = [-1 if v in hap_none else self.gids[w] for v, w in enumerate(which)]
            self.gap = gap
            if produce:
                self.produce()
        except Exception:
            self.close()
            raise

    def produce(self):
        b = self.b
        self.norm = b.normalize(self.gids_n, columns=True)
        self.atom = b.atomize(columns=True)
        self.hap = b.haplotypes(self.gids_h, gap=self.gap, columns=True)
        self.sub = b.hapsubsets(columns=True)

    def close(self):
        self.b.close()
        for t in self.tids:
            self.engine.truth_release(t)
        for g in self.gids:
            self.engine.genome_release(g)


def compare(run, genomes, truths, cols, which, norm_none=(), hap_none=()):
    """with the subset search and the columns against the restatement; then without the search (the restated bytes less B), and
    without the columns (the same counts, no bytes)"""
    b = run.b
    rec, tru = b.ladder(subsets=True, columns=True)
    assert rec.shape == (b.n_vcf, 18) and rec.dtype == np.uint64 and tru.shape == (b.n_vcf, 18)
    got = [b.laddered(v) for v in range(b.n_vcf)]
    want = []
    for v, (c, w) in enumerate(zip(cols, which)):
        gn = None if v in norm_none else genomes[w]
        gh = None if v in hap_none else genomes[w]
        kept, tp = run.masks[v]
        wrec, wtru, wmask, wemask = ld.masks(gn, gh, truths[w], c[0], c[1], c[2], c[4], kept, tp, gap=run.gap, subsets=True)
        want.append((wmask, wemask))
        np.testing.assert_array_equal(got[v][0], wmask, err_msg="mask bytes of VCF %d" % v)
        np.testing.assert_array_equal(got[v][1], wemask, err_msg="entry bytes of VCF %d" % v)
        np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d" % v)
        np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d" % v)
        # the identities against the producers' own getters
        ld.identities(rec[v], tru[v], got[v][1], norm=None if gn is None else (run.norm[0][v], run.norm[1][v]),
                      atom=(run.atom[0][v], run.atom[1][v]), hap=None if gh is None else (run.hap[0][v], run.hap[1][v]),
                      sub=None if gh is None else run.sub[v],
                      forms_of=None if gn is None else [nz.form_codes(gn, *e)[1:] for e in nz.truth_order(*truths[w])])
    rec2, tru2 = b.ladder(columns=True)
    for v, (wmask, wemask) in enumerate(want):
        m, e = b.laddered(v)
        np.testing.assert_array_equal(m, wmask & ~np.uint8(B), err_msg="mask bytes of VCF %d without the search" % v)
        np.testing.assert_array_equal(e, wemask & ~np.uint8(B), err_msg="entry bytes of VCF %d without the search" % v)
        np.testing.assert_array_equal(rec2[v], ld.count_records(m))
        np.testing.assert_array_equal(tru2[v], ld.count_entries(e))
    rec3, tru3 = b.ladder(subsets=True)
    np.testing.assert_array_equal(rec3, rec)
    np.testing.assert_array_equal(tru3, tru)
    with pytest.raises(QmvtError, match="did not keep the columns"):
        b.laddered(0)
    return rec, tru, got


# ---- the device against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_against_the_restatement(engine, sorted_):
    """VCFs of 0, 1, 2, 1023, 1024, 1025, 16 384, 16 385 and 300 records -- the seams of a span, of a workgroup and of a lane's 16
    records -- on two truth sets (2000 entries on the planted genome, 65 on the 17-base one), several VCFs on each, one VCF that
    names no genome in either call"""
    tvs, truths, cols = fam.family(41, sorted_)
    none = (fam.NO_GENOME,)
    run = Run(engine, fam.GENOMES, truths, cols, fam.WHICH, norm_none=none, hap_none=none)
    try:
        rec, tru, _ = compare(run, fam.GENOMES, truths, cols, fam.WHICH, none, none)
        assert sum(ld.cells_with(r, ld.M_N) for r in rec) > 100 and sum(ld.cells_with(r, ld.M_A) for r in rec) > 100
        assert ld.cells_with(rec[fam.NO_GENOME], ld.M_N | ld.M_H | ld.M_B) == 0 and ld.cells_with(rec[fam.NO_GENOME], ld.M_A) > 0
    finally:
        run.close()


@pytest.mark.parametrize("seed", [7, 8])
def test_planted_family(engine, seed):
    """every method bit alone and the pairs (tests/test_ladder_host.py checks the draw): sorted, shuffled, a VCF that names no
    genome in the normalisation call, one that names none in the haplotype call, all on one truth set"""
    f = LadderFamily(seed)
    truth = truth_codes(f.truth)
    rng = np.random.default_rng(seed)
    cols = [f.columns(), f.columns(rng), f.columns(rng), f.columns(), f.columns(keep=range(0, len(f.recs), 2))]
    run = Run(engine, [f.genome], [truth], cols, [0] * 5, norm_none=(2,), hap_none=(3,))
    try:
        rec, tru, got = compare(run, [f.genome], [truth], cols, [0] * 5, (2,), (3,))
        for m in (ld.M_N, ld.M_A, ld.M_H, ld.M_B, ld.M_N | ld.M_H, ld.M_A | ld.M_H, ld.M_N | ld.M_B):
            assert int(rec[0][ld.CELL0 + m]) >= 1, ld.set_name(m)
        np.testing.assert_array_equal(rec[0], rec[1])               # shuffled: the same counts
        np.testing.assert_array_equal(tru[0], tru[1])
        np.testing.assert_array_equal(got[0][1], got[1][1])
        assert ld.cells_with(rec[2], ld.M_N) == 0 and ld.cells_with(rec[2], ld.M_H) > 0
        assert ld.cells_with(rec[3], ld.M_H | ld.M_B) == 0 and ld.cells_with(rec[3], ld.M_N) > 0
    finally:
        run.close()


@pytest.mark.parametrize("n", [1, 65])
def test_truth_set_sizes(engine, n):
    """truth sets of n entries on both genomes: the last word of the bitmaps holds one bit or two, the tables are the smallest"""
    rng = np.random.default_rng(500 + n)
    tvs = [fam.truth_set(g, rng, n) for g in fam.GENOMES]
    truths = [fam.codes(v) for v in tvs]
    assert all(len(nz.truth_order(*t)) == n for t in truths)
    which = [0, 1, 0, 1]
    cols = [fam.records(fam.GENOMES[w], rng, m, tvs[w], bool(v & 1)) for v, (m, w) in enumerate(zip([400, 400, 257, 1030], which))]
    run = Run(engine, fam.GENOMES, truths, cols, which)
    try:
        compare(run, fam.GENOMES, truths, cols, which)
    finally:
        run.close()


def test_4096_kept_lines_in_one_cell(engine):
    """the deletion of one A from the 70-base run at 101, spelled at sixteen places, 4096 times: one cell takes them all"""
    g = fam.G600
    n = 4096
    pos = np.array([101 + (i * 7) % 16 for i in range(n)], np.int32)
    cols = (pos, np.full(n, nz.code("AA"), np.int32), np.full(n, nz.code("A"), np.int32), np.full(n, 50, np.float32), np.full(n, 3, np.uint8))
    truth = fam.codes([(100, "TA", "T")])
    run = Run(engine, [g], [truth], [cols], [0])
    try:
        rec, tru, got = compare(run, [g], [truth], [cols], [0])
        want = np.zeros(18, np.uint64)
        want[ld.KEPT], want[ld.CELL0 + ld.M_N] = n, n
        np.testing.assert_array_equal(rec[0], want)
        assert (got[0][0] == (ld.M_K | ld.M_N)).all()
        assert int(tru[0][ld.CELL0 + ld.M_N]) == 1 and int(tru[0][ld.KEPT]) == 1
    finally:
        run.close()


def test_snvs_alone(engine):
    """SNVs on both sides: an SNV is its own normal form and its own atom, no site can rescue one -- all 15 cells are zero, TP
    and FOUND are the batch's"""
    rng = np.random.default_rng(5)
    g = fam.G600
    bases = "ACGT"
    tvs = sorted({(int(p), g[p - 1], bases[(bases.index(g[p - 1]) + int(k)) % 4]) for p, k in zip(rng.integers(1, len(g) + 1, 300), rng.integers(1, 4, 300))})
    truth = fam.codes(tvs)
    cols = []
    for n in (2000, 257):
        recs = []
        for i in range(n):
            if rng.random() < 0.5:
                recs.append(tvs[int(rng.integers(0, len(tvs)))])
            else:
                p = int(rng.integers(1, len(g) + 1))
                recs.append((p, g[p - 1], bases[(bases.index(g[p - 1]) + int(rng.integers(1, 4))) % 4]))
        pos, ref, alt = fam.codes(recs)
        flags = (rng.random(n) < 0.8).astype(np.uint8) | ((rng.random(n) < 0.9).astype(np.uint8) << 1)
        cols.append((pos, ref, alt, np.full(n, 30, np.float32), flags.astype(np.uint8)))
    run = Run(engine, [g], [truth], cols, [0, 0])
    try:
        rec, tru, _ = compare(run, [g], [truth], cols, [0, 0])
        for v in range(2):
            assert not rec[v][ld.CELL0 + 1:].any() and not tru[v][ld.CELL0 + 1:].any()
            kept, tp = run.masks[v]
            assert int(rec[v][ld.KEPT]) == int(kept.sum()) and int(rec[v][ld.TP]) == int(tp.sum()) > 100
            assert int(tru[v][ld.TP]) == int(run.hap[1][v][1]) == int(run.atom[1][v][4]) > 50
            assert int(rec[v][ld.CELL0]) == int(kept.sum()) - int(tp.sum())
    finally:
        run.close()


# ---- state and argument errors ------------------------------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    tvs, truths, cols = fam.family(49, True, sizes=[40, 40], which=[0, 0], truth_n=[50, 20])
    run = Run(engine, fam.GENOMES, truths, cols, [0, 0], produce=False)
    b = run.b
    sb = engine.batch([40], [run.tids[0]])                     # a single-base batch
    try:
        code, msg = refused(b.ladder_counts)                    # before the pass
        assert code == QM_E_STATE and "no qm_batch_ladder" in msg
        code, msg = refused(lambda: b.laddered(0))
        assert code == QM_E_STATE and "no qm_batch_ladder" in msg
        # every producer missing in turn: the first one missing is named
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "qm_batch_normalize(.., QM_NORM_COLUMNS)" in msg
        b.normalize(run.gids_n)                                 # without the columns: not the producer
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "qm_batch_normalize(.., QM_NORM_COLUMNS)" in msg
        b.normalize(run.gids_n, columns=True)
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "qm_batch_atomize(QM_ATOM_COLUMNS)" in msg
        b.atomize(columns=True)
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "qm_batch_haplotypes(.., QM_HAP_COLUMNS)" in msg
        b.haplotypes(run.gids_h)
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "qm_batch_haplotypes(.., QM_HAP_COLUMNS)" in msg
        before = b.device_bytes
        b.haplotypes(run.gids_h, columns=True)
        mid = b.device_bytes
        code, msg = refused(lambda: b.ladder(subsets=True))
        assert code == QM_E_STATE and "qm_batch_hapsubsets(QM_HAPSUB_COLUMNS)" in msg
        assert b.device_bytes == mid                            # a refused call allocates nothing
        first = b.ladder(columns=True)                          # three producers suffice without QM_LADDER_SUBSETS
        assert b.device_bytes > mid >= before                   # the pass's arrays are counted
        b.hapsubsets()                                          # without the columns: not the producer; and it forgets the ladder's rows
        code, msg = refused(b.ladder_counts)
        assert code == QM_E_STATE and "no qm_batch_ladder" in msg
        code, msg = refused(lambda: b.ladder(subsets=True))
        assert code == QM_E_STATE and "qm_batch_hapsubsets(QM_HAPSUB_COLUMNS)" in msg
        b.hapsubsets(columns=True)
        full = b.ladder(subsets=True, columns=True)
        for what in (4, 8, 7):
            assert b._L.qm_batch_ladder(b._h, what, None) == QM_E_INVAL
        for x, y in zip(b.ladder_counts(), full):               # a refused call leaves the rows
            np.testing.assert_array_equal(x, y)
        # behind a producer called again: each of the four forgets the ladder's rows
        for again in (lambda: b.normalize(run.gids_n, columns=True), lambda: b.atomize(columns=True), lambda: b.hapsubsets(columns=True)):
            again()
            code, msg = refused(b.ladder_counts)
            assert code == QM_E_STATE and "no qm_batch_ladder" in msg
            for x, y in zip(b.ladder(subsets=True, columns=True), full):
                np.testing.assert_array_equal(x, y)
        b.haplotypes(run.gids_h, columns=True)                  # ... and the haplotype pass the search's too
        code, msg = refused(b.ladder_counts)
        assert code == QM_E_STATE
        code, msg = refused(lambda: b.ladder(subsets=True))
        assert code == QM_E_STATE and "qm_batch_hapsubsets(QM_HAPSUB_COLUMNS)" in msg
        for x, y in zip(b.ladder(), first):
            np.testing.assert_array_equal(x, y)
        code, msg = refused(lambda: b.laddered(0))
        assert code == QM_E_STATE and "QM_LADDER_COLUMNS" in msg
        code, msg = refused(b.ladder_timings)                   # the timings with timing off
        assert code == QM_E_STATE and "timing is off" in msg
        b.set_timing(True)
        b.ladder()
        ms = b.ladder_timings()
        assert set(ms) == {"ladder_records_ms", "ladder_truth_ms"} and all(x >= 0 for x in ms.values())
        b.set_timing(False)
        b.run()                                                 # behind a new run
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "qm_batch_finish first" in msg
        b.finish()
        code, msg = refused(b.ladder)
        assert code == QM_E_STATE and "behind the latest run" in msg
        code, msg = refused(b.ladder_counts)
        assert code == QM_E_STATE
        sb.upload(0, *[x if i < 1 or i > 2 else (x & 3).astype(np.int32) for i, x in enumerate(cols[0])])
        sb.run()
        sb.finish()
        code, msg = refused(sb.ladder)
        assert code == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        assert b._L.qm_batch_get_ladder(None, None, None) == QM_E_INVAL
        assert b._L.qm_batch_get_laddered(b._h, 5, None, None) == QM_E_STATE     # (the rows are gone: the state comes first)
    finally:
        sb.close()
        run.close()
