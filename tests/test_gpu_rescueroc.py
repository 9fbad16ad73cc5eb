"""The QUAL ROC under normal-form and atom matching on the device (qm_batch_rescue_roc; k_rroc_records / k_rroc_units; DESIGN.md
4.22) against the restatement of quasimodo_amd.rescueroc, against the batch's own ROC and against the two producer passes run on
filtered batches.  Every comparison is exact: these are integers."""
import numpy as np
import pytest

from quasimodo_amd import _lib
from quasimodo_amd import normalize as nz
from quasimodo_amd import rescueroc as rr
from quasimodo_amd._lib import QmvtError
import rescueroc_family as fam

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
N_TP_N, N_FOUND = 2, 2            # QM_NORM_R_TP_N, QM_NORM_T_FOUND
A_TP_A, A_FOUND_A = 2, 5          # QM_ATOM_R_TP_A, QM_ATOM_T_FOUND_A
S_TRUTH_UNIQUE = 7


class Run:
    """one finished allele-extended batch with both producers and the sweep behind it"""

    def __init__(self, engine, genomes, truths, cols, which, no_genome=(), n_bins=256, sweep=True):
        self.engine = engine
        self.tids = [engine.truth_load(*t) for t in truths]
        self.gids = [engine.genome_load(g.encode()) for g in genomes]
        self.b = engine.batch([len(c[0]) for c in cols], [self.tids[w] for w in which], n_bins=n_bins, alleles=True)
        try:
            for v, c in enumerate(cols):
                self.b.upload(v, *c)
            self.b.run()
            self.b.finish()
            self.want_gids = [-1 if v in no_genome else self.gids[w] for v, w in enumerate(which)]
            if sweep:
                self.norm = self.b.normalize(self.want_gids, columns=True)
                self.atom = self.b.atomize(columns=True)
                self.roc_n, self.roc_a, self.base = self.b.rescue_roc()
                self.roc = self.b.roc()
        except Exception:
            self.close()
            raise

    def close(self):
        self.b.close()
        for t in self.tids:
            self.engine.truth_release(t)
        for g in self.gids:
            self.engine.genome_release(g)


def identities(roc_x, base_x, roc, what):
    """what holds for every t whatever the draw: the universe is the batch ROC's, a rescue only ever adds TP lines, the found
    units shrink with the threshold and never exceed the baseline"""
    np.testing.assert_array_equal(roc_x[0] + roc_x[1], roc[0] + roc[1], err_msg="TP + FP, " + what)
    assert (roc_x[0] >= roc[0]).all(), what
    assert (np.diff(roc_x[2].astype(np.int64)) <= 0).all(), what
    assert int(roc_x[2][0]) <= int(base_x), what


def compare(run, genomes, truths, cols, which, no_genome=(), n_bins=256):
    for v, (c, w) in enumerate(zip(cols, which)):
        g = None if v in no_genome else genomes[w]
        wn, wa, wb = rr.sweep(g, truths[w], *c, n_bins=n_bins)
        np.testing.assert_array_equal(run.roc_n[v], wn, err_msg="roc_n of VCF %d" % v)
        np.testing.assert_array_equal(run.roc_a[v], wa, err_msg="roc_a of VCF %d" % v)
        np.testing.assert_array_equal(run.base[v], wb, err_msg="base of VCF %d" % v)
        identities(run.roc_a[v], run.base[v][1], run.roc[v], "atoms, VCF %d" % v)
        if g is None:
            assert not run.roc_n[v].any() and int(run.base[v][0]) == 0
        else:
            identities(run.roc_n[v], run.base[v][0], run.roc[v], "normal form, VCF %d" % v)


# ---- the device against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_against_the_restatement(engine, sorted_):
    """VCFs of 0 .. 16 385 records on two truth sets (2000 entries on the planted genome, 65 on the 17-base one), several VCFs on
    each -- the best cells of one VCF are nothing to the next --, one VCF without a genome"""
    tvs, truths, cols = fam.family(41, sorted_)
    run = Run(engine, fam.GENOMES, truths, cols, fam.WHICH, no_genome=(fam.NO_GENOME,))
    try:
        compare(run, fam.GENOMES, truths, cols, fam.WHICH, no_genome=(fam.NO_GENOME,))
        assert int((run.roc_n[:, 0, 0] - run.roc[:, 0, 0])[:fam.NO_GENOME].sum()) > 100      # lines only the normal form makes TP
        assert int((run.roc_a[:, 0, 0] - run.roc[:, 0, 0]).sum()) > 100
        assert len({int(x) for x in run.roc_n[6][2]}) > 20 and len({int(x) for x in run.roc_a[6][2]}) > 20   # many best bins
        # the same sweep again, and one matching alone: the same rows
        again = run.b.rescue_roc()
        for x, y in zip(again, (run.roc_n, run.roc_a, run.base)):
            np.testing.assert_array_equal(x, y)
        rn, ra, base = run.b.rescue_roc(which=_lib.QM_RROC_ATOM)
        assert rn is None
        np.testing.assert_array_equal(ra, run.roc_a)
        np.testing.assert_array_equal(base[:, 1], run.base[:, 1])
        assert not base[:, 0].any()
        code, msg = refused(lambda: run.b.rescue_roc_counts(_lib.QM_RROC_NORM))
        assert code == QM_E_STATE and "did not sweep by normal form" in msg
        run.b.set_timing(True)
        run.b.rescue_roc()
        ms = run.b.rescue_roc_timings()
        assert set(ms) == {"rroc_norm_records_ms", "rroc_norm_units_ms", "rroc_atom_records_ms", "rroc_atom_units_ms"}
        assert all(x >= 0 for x in ms.values())
    finally:
        run.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_truth_set_sizes(engine, n):
    """truth sets of n entries on both genomes: the last word of the best cells is half used or full"""
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


@pytest.mark.parametrize("n_bins", [1, 20, 21])
def test_fewer_bins(engine, n_bins):
    """n_bins = 20: QUAL 20 and 19.999 share the last bin; 21: they do not; 1: one threshold"""
    tvs, truths, cols = fam.family(43, False, sizes=[0, 1, 300, 1025, 700], which=[0, 1, 0, 1, 0], truth_n=[200, 65])
    which = [0, 1, 0, 1, 0]
    run = Run(engine, fam.GENOMES, truths, cols, which, no_genome=(4,), n_bins=n_bins)
    try:
        assert run.roc_n.shape == (5, 3, n_bins)
        compare(run, fam.GENOMES, truths, cols, which, no_genome=(4,), n_bins=n_bins)
    finally:
        run.close()


# ---- contention -----------------------------------------------------------------------------------------------------------------
def one_truth_batch(engine, g, truth_vs, recs, n_bins=256):
    truth = fam.codes(truth_vs)
    cols = (np.array([r[0] for r in recs], np.int32), np.array([nz.code(r[1]) for r in recs], np.int32),
            np.array([nz.code(r[2]) for r in recs], np.int32), np.array([r[3] for r in recs], np.float32),
            np.full(len(recs), 3, np.uint8))
    return Run(engine, [g], [truth], [cols], [0], n_bins=n_bins), truth, cols


def test_4096_records_of_one_form_with_every_bin(engine):
    """the deletion of one A from the 70-base run at 101, spelled at sixteen places: every record raises the same cell"""
    g = fam.G600
    recs = [(101 + (i * 7) % 16, "AA", "A", (i * 37) % 256 + 0.5) for i in range(4096)]
    run, truth, cols = one_truth_batch(engine, g, [(100, "TA", "T")], recs)
    try:
        compare(run, [g], [truth], [cols], [0])
        want = np.zeros(256, np.uint64)
        want[:] = np.cumsum(np.full(256, 16, np.uint64)[::-1])[::-1]
        np.testing.assert_array_equal(run.roc_n[0][0], want)
        assert not run.roc_n[0][1].any() and (run.roc_n[0][2] == 1).all() and int(run.base[0][0]) == 1
        np.testing.assert_array_equal(run.roc_a[0][1], want)              # none of them is spelled like the entry
        assert not run.roc_a[0][2].any()
    finally:
        run.close()


def test_64_consecutive_records_on_one_atom(engine):
    """one wave's records all carry the atom C -> T at 8 of the truth MNP, at 64 distinct bins; one more carries the other atom"""
    g = "GGTTGGACGG" * 3
    order = np.random.default_rng(3).permutation(64)
    recs = [(8, "C", "T", float(4 * k + 1)) for k in order] + [(7, "A", "G", 9.0)]
    run, truth, cols = one_truth_batch(engine, g, [(7, "AC", "GT")], recs)
    try:
        compare(run, [g], [truth], [cols], [0])
        np.testing.assert_array_equal(run.roc_a[0][2], (np.arange(256) <= 9).astype(np.uint64))   # min(253, 9)
        assert int(run.roc_a[0][0][0]) == 65
    finally:
        run.close()


@pytest.mark.parametrize("n_bins", [256, 21])
def test_neighbouring_cells_at_alternating_bins(engine, n_bins):
    """64 SNVs and 128 insertions at 64 consecutive positions: 192 entries, 192 forms, their cells side by side in shared words
    (forms and entries by entry index; the atoms by slot: 64 atoms in 128 slots).  Units of even entry index are hit at bin 0
    alone, those of odd index at the last bin alone, record beside record: an update that touched its neighbour would lift a
    unit out of bin 0 or drop one from the last bin."""
    g, bases = fam.G600, "ACGT"
    K, p0 = 64, 480                                       # outside the planted repeats
    snvs = [(p0 + k, g[p0 + k - 1], bases[(bases.index(g[p0 + k - 1]) + 1 + k % 3) % 4]) for k in range(K)]
    ins = lambda k, s: (p0 + k, g[p0 + k - 1], g[p0 + k - 1] + [b for b in bases if b != g[p0 + k]][s] + "TT")
    truth_vs = snvs + [ins(k, 0) for k in range(K)] + [ins(k, 1) for k in range(K)]
    index = {e: j for j, e in enumerate(nz.truth_order(*fam.codes(truth_vs)))}
    assert len(index) == 3 * K
    recs = []
    for rep in range(6):
        for v in truth_vs:
            odd = index[(v[0], nz.code(v[1]), nz.code(v[2]))] & 1
            recs.append((v[0], v[1], v[2], float(n_bins - 1) + 0.5 if odd else 0.25))
    recs.sort(key=lambda r: r[0])                          # the records of neighbouring entries beside each other
    run, truth, cols = one_truth_batch(engine, g, truth_vs, recs, n_bins=n_bins)
    try:
        compare(run, [g], [truth], [cols], [0], n_bins=n_bins)
        for roc, base in ((run.roc_n[0], run.base[0][0]), (run.roc_a[0], run.base[0][1])):
            assert int(base) == 3 * K and int(roc[2][0]) == 3 * K
            assert (roc[2][1:] == 3 * K // 2).all()
    finally:
        run.close()


# ---- independent of the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_against_the_two_passes_themselves(engine, sorted_):
    """PASS <=> bin >= 20 and every ID is `.`: the sweep at t = 20 is what the passes count.  For five thresholds a second batch
    holds only the records with bin >= t, all PASS: the passes count there what the sweep says at t."""
    sizes, which = [300, 1025, 2000], [0, 1, 0]
    tvs, truths, cols = fam.family(47, sorted_, sizes=sizes, which=which, truth_n=[300, 65], pass_is_bin=True, all_iddot=True)
    run = Run(engine, fam.GENOMES, truths, cols, which)
    try:
        (nrec, ntru), (arec, atru) = run.norm, run.atom
        np.testing.assert_array_equal(run.roc_n[:, 0, 20], nrec[:, N_TP_N])
        np.testing.assert_array_equal(run.roc_n[:, 2, 20], ntru[:, N_FOUND])
        np.testing.assert_array_equal(run.roc_a[:, 0, 20], arec[:, A_TP_A])
        np.testing.assert_array_equal(run.roc_a[:, 2, 20], atru[:, A_FOUND_A])
        assert int(nrec[:, N_TP_N].sum()) > 0 and int(atru[:, A_FOUND_A].sum()) > 0
        roc_n, roc_a = run.roc_n.copy(), run.roc_a.copy()
    finally:
        run.close()
    ok = lambda c: ((c >= 0) & (c < 4)) | (c >= 0x08000000)
    for t in (0, 1, 19, 100, 255):
        sub = []
        for c in cols:
            bins = np.array([rr.qual_bin(q, 256) for q in c[3]], np.int64)
            m = bins >= t
            flags = np.where(ok(c[1][m]) & ok(c[2][m]), c[4][m] | 1, c[4][m]).astype(np.uint8)
            sub.append((c[0][m].copy(), c[1][m].copy(), c[2][m].copy(), c[3][m].copy(), flags))
        run = Run(engine, fam.GENOMES, truths, sub, which, sweep=False)
        try:
            nrec, ntru = run.b.normalize(run.want_gids)
            arec, atru = run.b.atomize()
        finally:
            run.close()
        np.testing.assert_array_equal(roc_n[:, 0, t], nrec[:, N_TP_N], err_msg="TP_N(%d)" % t)
        np.testing.assert_array_equal(roc_n[:, 2, t], ntru[:, N_FOUND], err_msg="U_N(%d)" % t)
        np.testing.assert_array_equal(roc_a[:, 0, t], arec[:, A_TP_A], err_msg="TP_A(%d)" % t)
        np.testing.assert_array_equal(roc_a[:, 2, t], atru[:, A_FOUND_A], err_msg="U_A(%d)" % t)


def test_snvs_alone_give_the_batch_roc(engine):
    """an SNV is its own normal form and its own atom: both sweeps are the batch's ROC bit for bit, both baselines its truth_unique"""
    from conftest import random_columns
    rng = np.random.default_rng(5)
    g = fam.G600
    gcode = np.array(["ACGT".index(ch) for ch in g], np.int32)
    tpos = rng.integers(1, len(g) + 1, 300).astype(np.int32)
    tref = gcode[tpos - 1]
    talt = ((tref + rng.integers(1, 4, 300)) % 4).astype(np.int32)
    cols = []
    for n in (2000, 257):
        pos, ref, alt, qual, flags = random_columns(rng, n, len(g), (tpos, tref, talt), frac_truth=0.5, weird=False)
        alt = np.where(alt == ref, (ref + 1) % 4, alt).astype(np.int32)      # (any REF: a mismatch with the genome is its own form too)
        qual = np.where(rng.random(n) < 0.1, np.float32(np.nan), qual + np.float32(0.5)).astype(np.float32)
        flags = (flags | (rng.random(n) < 0.03).astype(np.uint8) << 3 | (rng.random(n) < 0.03).astype(np.uint8) << 2).astype(np.uint8)
        flags = np.where(rng.random(n) < 0.1, flags & ~np.uint8(2), flags).astype(np.uint8)
        cols.append((pos, ref, alt, qual, flags))
    run = Run(engine, [g], [(tpos, tref, talt)], cols, [0, 0])
    try:
        np.testing.assert_array_equal(run.roc_n, run.roc)
        np.testing.assert_array_equal(run.roc_a, run.roc)
        scal = run.b.scalars()
        assert (run.base[:, 0] == scal[:, S_TRUTH_UNIQUE]).all() and (run.base[:, 1] == scal[:, S_TRUTH_UNIQUE]).all()
        assert int(run.roc[0][0][0]) > 100 and int(run.roc[0][2][0]) > 50
    finally:
        run.close()


# ---- state and argument errors ------------------------------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    tvs, truths, cols = fam.family(49, True, sizes=[40, 40], which=[0, 0], truth_n=[50, 20])
    run = Run(engine, fam.GENOMES, truths, cols, [0, 0], sweep=False)
    b = run.b
    sb = engine.batch([40], [run.tids[0]])                     # a single-base batch
    try:
        before = b.device_bytes
        code, msg = refused(b.rescue_roc)                       # no producer yet: the first one missing is named
        assert code == QM_E_STATE and "qm_batch_normalize(.., QM_NORM_COLUMNS)" in msg
        code, msg = refused(lambda: b.rescue_roc(which=_lib.QM_RROC_ATOM))
        assert code == QM_E_STATE and "qm_batch_atomize(QM_ATOM_COLUMNS)" in msg
        code, msg = refused(b.rescue_roc_counts)
        assert code == QM_E_STATE and "no qm_batch_rescue_roc" in msg
        b.normalize(run.want_gids)                              # without the columns: not the producer
        code, msg = refused(lambda: b.rescue_roc(which=_lib.QM_RROC_NORM))
        assert code == QM_E_STATE and "QM_NORM_COLUMNS" in msg
        b.normalize(run.want_gids, columns=True)
        b.atomize()
        code, msg = refused(b.rescue_roc)
        assert code == QM_E_STATE and "qm_batch_atomize(QM_ATOM_COLUMNS)" in msg
        rn, ra, base = b.rescue_roc(which=_lib.QM_RROC_NORM)    # one producer suffices for its own matching
        assert ra is None and int(rn[:, 0, 0].sum()) > 0
        assert b.device_bytes > before                          # the sweep's arrays are counted
        b.atomize(columns=True)
        for which in (0, 4, 7):
            assert b._L.qm_batch_rescue_roc(b._h, which, None) == QM_E_INVAL
        first = b.rescue_roc()
        b.normalize(run.want_gids, columns=True)                # a new call of a producer forgets its matching's rows
        code, msg = refused(lambda: b.rescue_roc_counts(_lib.QM_RROC_NORM))
        assert code == QM_E_STATE
        np.testing.assert_array_equal(b.rescue_roc_counts(_lib.QM_RROC_ATOM)[1], first[1])
        np.testing.assert_array_equal(b.rescue_roc()[0], first[0])
        code, msg = refused(b.rescue_roc_timings)
        assert code == QM_E_STATE and "timing is off" in msg
        b.run()                                                 # a batch re-run since the producers
        code, msg = refused(b.rescue_roc)
        assert code == QM_E_STATE and "qm_batch_finish first" in msg
        b.finish()
        code, msg = refused(b.rescue_roc)
        assert code == QM_E_STATE and "behind the latest run" in msg
        code, msg = refused(b.rescue_roc_counts)
        assert code == QM_E_STATE
        sb.upload(0, *[x if i < 1 or i > 2 else (x & 3).astype(np.int32) for i, x in enumerate(cols[0])])
        sb.run()
        sb.finish()
        code, msg = refused(sb.rescue_roc)
        assert code == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        assert b._L.qm_batch_get_rescue_roc(None, None, None, None) == QM_E_INVAL
    finally:
        sb.close()
        run.close()
