"""Clusters of records matched by replayed haplotype on the device (qm_batch_haplotypes; qmvt_haplo.hip) against
the restatement of quasimodo_amd.haplo, exactly: both count blocks, the class bytes, the site indices, the entry classes and
qm_truth_sites, on the planted family of haplo_family.py; tied to the batch's masks and scalars, to the truth set's table and
-- through the found entries -- to the variant-type pass, an independent kernel.  Every comparison is exact: these are integers.
One planted family: it leaves the scans, the bitmap rank and the gather loop on their first iteration, its genome is pure ACGT and
no window of it touches an end of the genome -- the step seams, more than 8192 sites, more than 64 entries per site, the genome's
ends, bytes that are no base and every pair of inline lengths are test_gpu_haplo_edges.py's."""
import numpy as np
import pytest

from haplo_family import Family, codes, truth_codes
from quasimodo_amd import haplo as hp
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_NPASS, S_TP_LINES = 0, 1
R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}


def cut(n, tail):
    """the largest size <= n that leaves a span tail of `tail` records (records go four to a lane)"""
    return n - ((n - tail) % 4)


class Setup:
    """Two families (genome, truth set) and seven VCFs:
    0 the first family sorted, 1 the same records shuffled, 2 two thirds of them (another open set on the same truth set),
    3 no kept record, 4 the records of 0 with no genome, 5 the second family, shuffled, 6 no record at all."""

    def __init__(self, engine):
        rng = np.random.default_rng(5)
        self.fam = [Family(20), Family(21, repeats=2)]
        self.truths = [truth_codes(f.truth) for f in self.fam]
        n0 = len(self.fam[0].recs)
        keep0 = list(range(cut(n0, 1)))
        order = sorted(keep0, key=lambda i: self.fam[0].recs[i][0])
        self.perm = list(keep0)
        rng.shuffle(self.perm)
        sub = [i for i in keep0 if i % 3]
        sub = sub[:cut(len(sub), 2)]
        dead = [r[:3] + (False, r[4]) for r in self.fam[0].recs[:cut(n0, 3)]]
        self.cols = [codes([self.fam[0].recs[i] for i in order]), codes([self.fam[0].recs[i] for i in self.perm]),
                     self.fam[0].columns(rng, sub), codes(dead), codes([self.fam[0].recs[i] for i in order]),
                     self.fam[1].columns(rng), codes([])]
        self.order = order
        self.which = [0, 0, 0, 0, 0, 1, 0]
        assert [len(c[0]) % 4 for c in self.cols[:4]] == [1, 1, 2, 3]
        self.engine = engine
        self.gids = [engine.genome_load(f.genome.encode()) for f in self.fam]
        self.tids = [engine.truth_load(*t) for t in self.truths]
        self.genome_of = [self.gids[0]] * 4 + [-1, self.gids[1], self.gids[0]]
        self.b = engine.batch([len(c[0]) for c in self.cols], [self.tids[w] for w in self.which], alleles=True)
        for v, c in enumerate(self.cols):
            self.b.upload(v, *c)
        self.b.run()
        self.b.finish()
        self.masks = []
        for v in range(self.b.n_vcf):
            cls = self.b.cls(v)
            self.masks.append(((cls & 1).astype(bool), (cls & 2).astype(bool)))
        self.want = {}

    def restated(self, gap):
        if gap not in self.want:
            self.want[gap] = [hp.counts(self.fam[w].genome, self.truths[w], c[0], c[1], c[2], c[4], *self.masks[v], gap)
                              for v, (c, w) in enumerate(zip(self.cols, self.which))]
        return self.want[gap]

    def close(self):
        self.b.close()
        for t in self.tids:
            self.engine.truth_release(t)
        for g in self.gids:
            self.engine.genome_release(g)


@pytest.fixture(scope="module")
def setup(engine):
    s = Setup(engine)
    yield s
    s.close()


@pytest.mark.parametrize("gap", [10, 0, 32])
def test_counts_classes_and_sites_against_the_restatement(setup, gap):
    b = setup.b
    rec, tru = b.haplotypes(setup.genome_of, gap=gap, columns=True)
    assert rec.shape == (7, 16) and tru.shape == (7, 8) and rec.dtype == np.uint64
    want = setup.restated(gap)
    scal = b.scalars()
    for v in range(b.n_vcf):
        if setup.genome_of[v] < 0:
            assert not rec[v].any() and not tru[v].any()       # a VCF without a genome keeps zero rows
            with pytest.raises(QmvtError, match="named no genome"):
                b.haplotyped(v)
            continue
        wrec, wtru, wcls, wsite, wecls = want[v]
        cls, site, ecls = b.haplotyped(v)
        np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d, gap %d" % (v, gap))
        np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d, gap %d" % (v, gap))
        np.testing.assert_array_equal(cls, wcls, err_msg="classes of VCF %d, gap %d" % (v, gap))
        np.testing.assert_array_equal(site, wsite, err_msg="sites of VCF %d, gap %d" % (v, gap))
        np.testing.assert_array_equal(ecls, wecls, err_msg="entry classes of VCF %d, gap %d" % (v, gap))
        kept, tp = setup.masks[v]
        assert int(rec[v][R["kept"]]) == int(kept.sum()) == int(scal[v][S_NPASS])
        assert int(rec[v][R["tp"]]) == int((kept & tp).sum()) == int(scal[v][S_TP_LINES])
        assert int(rec[v][R["tp_h"]]) - int(rec[v][R["tp"]]) == int(rec[v][R["rescued"]])
        assert int(tru[v][T["found_h"]]) >= int(tru[v][T["found"]])
        assert int(tru[v][T["entries"]]) == len(setup.engine.truth_entries(setup.tids[setup.which[v]])[0])
    # sorted and shuffled: the same records, the same outcome line by line
    np.testing.assert_array_equal(rec[0], rec[1])
    np.testing.assert_array_equal(tru[0], tru[1])
    back = {i: k for k, i in enumerate(setup.perm)}
    c0, s0, e0 = b.haplotyped(0)
    c1, s1, e1 = b.haplotyped(1)
    np.testing.assert_array_equal(c0, c1[[back[i] for i in setup.order]])
    np.testing.assert_array_equal(s0, s1[[back[i] for i in setup.order]])
    np.testing.assert_array_equal(e0, e1)
    # two VCFs on one truth set with different open sets; one without a kept record
    assert rec[2].tolist() != rec[0].tolist() and tru[2].tolist() != tru[0].tolist() and int(tru[2][T["sites"]]) == int(tru[0][T["sites"]])
    assert int(rec[3][R["kept"]]) == 0 and not rec[3].any() and int(tru[3][T["found"]]) == 0 and int(tru[3][T["tried"]]) == 0
    assert int(tru[3][T["open"]]) + int(tru[3][T["unusable"]]) == int(tru[3][T["entries"]])
    assert not rec[6].any() and int(tru[6][T["entries"]]) == int(tru[0][T["entries"]])
    if gap == 10:                                   # what the family plants arrives on the device
        for c in ("rescued", "lone", "outside", "mismatch", "conflict", "toomany", "toolong", "long", "nokey", "novar", "range", "refmismatch"):
            assert int(rec[0][R[c]]) >= 1, c
        assert int(tru[0][T["matched"]]) >= 50 and int(tru[0][T["tried"]]) - int(tru[0][T["matched"]]) >= 50
    # FOUND is the found count of the variant-type pass
    _, ttru = b.vartype()
    for v in range(b.n_vcf):
        if setup.genome_of[v] >= 0:
            assert int(tru[v][T["found"]]) == int(ttru[v][:, 1].sum())
    for w in range(2):
        got = setup.engine.truth_sites(setup.tids[w], setup.gids[w], gap)
        for x, y in zip(got, hp.truth_sites(setup.fam[w].genome, setup.truths[w], gap)):
            np.testing.assert_array_equal(x, y)
        assert len(got[0]) == int(tru[5 if w else 0][T["sites"]])


def test_the_pass_leaves_the_batch_alone_and_counts_its_bytes(setup):
    b = setup.b
    before = ([b.cls(v).copy() for v in range(b.n_vcf)], b.scalars().copy(), b.roc().copy())
    rec, tru = b.haplotypes(setup.genome_of)
    bytes1 = b.device_bytes
    rec2, tru2 = b.haplotypes(setup.genome_of, columns=True)
    np.testing.assert_array_equal(rec, rec2)
    np.testing.assert_array_equal(tru, tru2)
    assert b.device_bytes >= bytes1 > 0
    for v in range(b.n_vcf):
        np.testing.assert_array_equal(b.cls(v), before[0][v])
    np.testing.assert_array_equal(b.scalars(), before[1])
    np.testing.assert_array_equal(b.roc(), before[2])


def test_more_than_one_workgroup_and_lists_far_past_the_cap(engine):
    """the family some hundred times over in one VCF: more than one workgroup of the record walks, every open line hundreds of
    times (one slot list takes hundreds of claims, eight are stored), shuffled"""
    fam = Family(22, repeats=1)
    truth = truth_codes(fam.truth)
    rng = np.random.default_rng(1)
    recs = fam.recs * (70000 // len(fam.recs) + 1)
    rng.shuffle(recs)
    cols = codes(recs)
    assert len(recs) > 4 * 16 * 1024
    gid, tid = engine.genome_load(fam.genome.encode()), engine.truth_load(*truth)
    b = engine.batch([len(recs)], [tid], alleles=True)
    try:
        b.upload(0, *cols)
        b.run()
        b.finish()
        c = b.cls(0)
        rec, tru = b.haplotypes([gid], columns=True)
        wrec, wtru, wcls, wsite, wecls = hp.counts(fam.genome, truth, cols[0], cols[1], cols[2], cols[4], (c & 1).astype(bool), (c & 2).astype(bool))
        cls, site, ecls = b.haplotyped(0)
        np.testing.assert_array_equal(rec[0], wrec)
        np.testing.assert_array_equal(tru[0], wtru)
        np.testing.assert_array_equal(cls, wcls)
        np.testing.assert_array_equal(site, wsite)
        np.testing.assert_array_equal(ecls, wecls)
        assert int(rec[0][R["toomany"]]) > 800
    finally:
        b.close()
        engine.truth_release(tid)
        engine.genome_release(gid)


def test_no_open_entry_anywhere(engine):
    """No (VCF, site) pair at all: every usable entry of the truth set is found by spelling, or sits in a TOOLONG site.  The
    unmatched lines inside the windows are LONE (or TOOLONG) all the same -- the walk that says so runs without a pair list."""
    genome = "TTGACCTAGGCATCGATTACGGATCCATGCAAGTCTAGCT" * 12          # G[11] = C, G[14] = C; L = 480
    snv = lambda p, k=1: (p, genome[p - 1], "ACGT"[("ACGT".index(genome[p - 1]) + k) % 4])
    chain = [snv(p) for p in range(121, 121 + 260, 20)]                # one site of 13 entries, its window longer than 256 bases
    truth = truth_codes([(11, "C", "G")] + chain)
    line = lambda v, kept=True: v + (kept, hp.F_IDDOT)
    vcfs = [codes([line((11, "C", "G")), line((14, "C", "T")), line(snv(125, 2)), line(snv(470))]),     # found; LONE; TOOLONG; OUTSIDE
            codes([line((11, "C", "G")), line((14, "C", "T"), False)]),                                    # ... the line beside it not kept
            codes([line((11, "C", "G"))])]
    gid, tid = engine.genome_load(genome.encode()), engine.truth_load(*truth)
    b = engine.batch([len(c[0]) for c in vcfs], [tid] * 3, alleles=True)
    try:
        for v, c in enumerate(vcfs):
            b.upload(v, *c)
        b.run()
        b.finish()
        rec, tru = b.haplotypes([gid] * 3, columns=True)
        for v, c in enumerate(vcfs):
            m = b.cls(v)
            wrec, wtru, wcls, wsite, wecls = hp.counts(genome, truth, c[0], c[1], c[2], c[4], (m & 1).astype(bool), (m & 2).astype(bool))
            cls, site, ecls = b.haplotyped(v)
            np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d" % v)
            np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d" % v)
            np.testing.assert_array_equal(cls, wcls, err_msg="classes of VCF %d" % v)
            np.testing.assert_array_equal(site, wsite)
            np.testing.assert_array_equal(ecls, wecls)
            assert int(cls.max()) < len(hp.CLASS_NAMES) and int(tru[v][T["tried"]]) == 0
            assert int(rec[v][R["open"]]) == int(rec[v][R["lone"]]) + int(rec[v][R["toolong"]])
        assert b.haplotyped(0)[0].tolist() == [hp.MATCHED, hp.LONE, hp.TOOLONG, hp.OUTSIDE]
        assert [int(rec[0][R[c]]) for c in ("kept", "open", "lone", "toolong", "outside")] == [4, 2, 1, 1, 1]
        assert b.haplotyped(1)[0].tolist() == [hp.MATCHED, hp.NOTKEPT] and not rec[1][4:].any() and not rec[2][4:].any()
    finally:
        b.close()
        engine.truth_release(tid)
        engine.genome_release(gid)


def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    fam = Family(23, repeats=1)
    truth = truth_codes(fam.truth)
    cols = fam.columns()
    n = len(cols[0])
    gid, gid2 = engine.genome_load(fam.genome.encode()), engine.genome_load(fam.genome.encode())
    tid = engine.truth_load(*truth)
    b = engine.batch([n, n], [tid, tid], alleles=True)
    sb = engine.batch([n], [tid])                                       # a single-base batch
    try:
        for v in range(2):
            b.upload(v, *cols)
        c, msg = refused(lambda: b.haplotypes([gid, gid]))
        assert c == QM_E_STATE and "qm_batch_finish first" in msg       # before finish
        b.run()
        b.finish()
        bytes0 = b.device_bytes
        for getter in (b.haplotype_counts, lambda: b.haplotyped(0), b.haplotype_timings):
            c, msg = refused(getter)                                    # getters before the pass
            assert c == QM_E_STATE and "no qm_batch_haplotypes behind the latest run" in msg
        g2 = np.array([gid, gid], np.int32)
        call = lambda g, gap, what=0: b._L.qm_batch_haplotypes(b._h, g.ctypes.data, gap, what, None)
        assert call(g2, 10, 4) == QM_E_INVAL                            # what
        assert call(g2, -1) == QM_E_INVAL and call(g2, 33) == QM_E_INVAL
        assert call(np.array([gid, 99], np.int32), 10) == QM_E_INVAL    # no such genome
        c, msg = refused(lambda: b.haplotypes([gid, gid2]))             # one truth set, two genomes
        assert c == QM_E_INVAL and "share truth set" in msg
        snv = lambda x: np.where((x >= 0) & (x < 4), x, 0).astype(np.int32)
        sb.upload(0, cols[0], snv(cols[1]), snv(cols[2]), cols[3], cols[4])
        sb.run()
        sb.finish()
        c, msg = refused(lambda: sb.haplotypes([gid]))                  # a single-base batch
        assert c == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        assert b.device_bytes == bytes0                                 # a batch that never ran the pass holds none of its buffers
        rec, tru = b.haplotypes([gid, -1])                              # it does run
        assert b.device_bytes > bytes0 and int(tru[0][T["matched"]]) > 0 and not rec[1].any()
        c, msg = refused(lambda: b.haplotyped(0))                       # that call kept no columns
        assert c == QM_E_STATE and "QM_HAP_COLUMNS" in msg
        b.set_timing(True)
        rec1, tru1 = b.haplotypes([gid, gid], columns=True)
        assert set(b.haplotype_timings()) == {"hap_sites_ms", "hap_records_ms", "hap_truth_ms", "hap_claim_ms", "hap_replay_ms"}
        np.testing.assert_array_equal(rec1[0], rec1[1])
        np.testing.assert_array_equal(rec1[0], rec[0])
        assert b._L.qm_batch_get_haplotyped(b._h, 2, None, None, None) == QM_E_INVAL     # the batch has two VCFs
        b.run()                                                         # a new run forgets the pass
        b.finish()
        c, msg = refused(b.haplotype_counts)
        assert c == QM_E_STATE
        engine.genome_release(gid2)
        c, msg = refused(lambda: b.haplotypes([gid, gid2]))             # a released genome
        assert c == QM_E_STATE and "released genome" in msg
        gid2 = None
        with pytest.raises(QmvtError):
            engine.truth_sites(tid, 99)
        with pytest.raises(ValueError, match="gap"):
            engine.truth_sites(tid, gid, 40)
        rec3, tru3 = b.haplotypes([gid, gid])                           # ... and the pass runs again behind the new run
        np.testing.assert_array_equal(rec3, rec1)
        engine.truth_release(tid)
        c, msg = refused(lambda: b.haplotypes([gid, gid]))              # a released truth set
        assert c == QM_E_STATE and "truth set %d was released" % tid in msg
        tid = None
    finally:
        b.close()
        sb.close()
        if tid is not None:
            engine.truth_release(tid)
        engine.genome_release(gid)
        if gid2 is not None:
            engine.genome_release(gid2)
