"""The subset search on the device (qm_batch_hapsubsets; k_hap_subsets in qmvt_haplo.hip) against the restatement
of quasimodo_amd.haplo, exactly, on the planted family of haplo_subsets.py: the count block, both second class arrays, the list
of PARTIAL sites and their masks; at g = 0, 10 and 32, sorted and shuffled, on span tails of 1, 2 and 3 records; the narrow-hash
mode against the normal one bit for bit; the four identities; the haplotype pass's own answers before and after; the state rules;
one batch whose pair lists run past the cap.  Every comparison is exact: these are integers."""
import numpy as np
import pytest

import haplo_subsets as hs
from haplo_family import Family, codes, truth_codes
from quasimodo_amd import haplo as hp
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
U = {name: k for k, name in enumerate(hp.SUB_COLS)}
R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}


class Setup:
    def __init__(self, engine):
        self.engine = engine
        self.e = e = hs.family()
        self.gid = engine.genome_load(e.genome.encode("latin-1"))
        self.tids = [engine.truth_load(*t) for t in e.tcodes]
        self.b = b = engine.batch([len(c[0]) for c in e.cols], [self.tids[v[1]] for v in e.vcfs], alleles=True)
        for v, c in enumerate(e.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        self.masks = []
        for v in range(b.n_vcf):
            m = b.cls(v)
            self.masks.append(((m & 1).astype(bool), (m & 2).astype(bool)))
        self.genome_of = [self.gid if v[3] else -1 for v in e.vcfs]
        self.want = {}

    def restated(self, v, gap):
        if (v, gap) not in self.want:
            self.want[(v, gap)] = hs.restate(self.e, v, gap, self.masks[v])
        return self.want[(v, gap)]

    def close(self):
        self.b.close()
        for t in self.tids:
            self.engine.truth_release(t)
        self.engine.genome_release(self.gid)


@pytest.fixture(scope="module")
def setup(engine):
    s = Setup(engine)
    yield s
    s.close()


def fetch(b, vs):
    return b.hapsubset_counts().copy(), {v: b.hapsubsetted(v) for v in vs}


@pytest.mark.parametrize("gap", [10, 0, 32])
def test_counts_classes_sites_and_masks_against_the_restatement(setup, gap):
    b, e = setup.b, setup.e
    with_genome = [v for v, vc in enumerate(e.vcfs) if vc[3]]
    bytes0 = b.device_bytes
    rec, tru = b.haplotypes(setup.genome_of, gap=gap, columns=True)
    pass_before = (rec.copy(), tru.copy(), [b.haplotyped(v) for v in with_genome])
    base = ([b.cls(v).copy() for v in range(b.n_vcf)], b.scalars().copy(), b.roc().copy())
    bytes1 = b.device_bytes
    sub = b.hapsubsets(columns=True)
    assert sub.shape == (b.n_vcf, 8) and sub.dtype == np.uint64
    if gap == 10:
        assert bytes1 >= bytes0 and b.device_bytes > bytes1          # the batch grows only with the search
    normal = fetch(b, with_genome)
    for v, vc in enumerate(e.vcfs):
        case = "%s, gap %d" % (vc[0], gap)
        if not vc[3]:
            assert not sub[v].any(), case                               # a VCF without a genome keeps a zero row
            with pytest.raises(QmvtError, match="named no genome"):
                b.hapsubsetted(v)
            continue
        res, (wsub, wcls, wecls, chosen) = setup.restated(v, gap)
        cls_s, ecls_s, site_s, sm, tm = normal[1][v]
        np.testing.assert_array_equal(sub[v], wsub, err_msg="sub of " + case)
        np.testing.assert_array_equal(cls_s, wcls, err_msg="second classes of " + case)
        np.testing.assert_array_equal(ecls_s, wecls, err_msg="second entry classes of " + case)
        assert list(zip(site_s.tolist(), sm.tolist(), tm.tolist())) == [d[:3] for d in chosen], "sites and masks of " + case
        # the identities
        cls, site, ecls = pass_before[2][with_genome.index(v)]
        s = [int(x) for x in sub[v]]
        assert s[U["searched"]] == s[U["partial"]] + s[U["nosubset"]], case
        kept = setup.masks[v][0]
        tried = {int(x) for x in site[kept & ((cls == hp.MISMATCH) | (cls == hp.CONFLICT))]}
        assert s[U["searched"]] == len(tried), case
        partial = np.isin(site, site_s) & np.isin(cls, (hp.MISMATCH, hp.CONFLICT))
        assert s[U["rescued_s"]] + s[U["left_lines"]] == int(partial.sum()), case
        open_ents = int(np.isin(ecls_s, (hp.SUBSET, hp.LEFT)).sum())
        assert s[U["found_s"]] - int(tru[v][T["found_h"]]) + s[U["left_entries"]] == open_ents, case
        assert int((cls_s == hp.SUBSET).sum()) == s[U["rescued_s"]] and int((cls_s == hp.LEFT).sum()) == s[U["left_lines"]], case
        same = ~np.isin(cls_s, (hp.SUBSET, hp.LEFT))
        np.testing.assert_array_equal(cls_s[same], cls[same])            # outside PARTIAL sites: the pass's own bytes
        np.testing.assert_array_equal(ecls_s[~np.isin(ecls_s, (hp.SUBSET, hp.LEFT))], ecls[~np.isin(ecls_s, (hp.SUBSET, hp.LEFT))])
        assert s[U["tp_s"]] >= int(rec[v][R["tp_h"]]) and s[U["found_s"]] >= int(tru[v][T["found_h"]]), case
    # sorted and shuffled: the same counts, the same sites and masks, the same rescued (POS, REF, ALT)
    for t, (v, perm) in e.twin.items():
        np.testing.assert_array_equal(sub[v], sub[t])
        for k in (2, 3, 4):
            np.testing.assert_array_equal(normal[1][v][k], normal[1][t][k])
        np.testing.assert_array_equal(normal[1][v][0][perm], normal[1][t][0])
        np.testing.assert_array_equal(normal[1][v][1], normal[1][t][1])
        spelled = lambda w: sorted(zip(*[x[normal[1][w][0] == hp.SUBSET].tolist() for x in e.cols[w][:3]]))
        assert spelled(v) == spelled(t) and (gap != 10 or len(spelled(v)) >= 30)
    # the narrow hashes: every candidate collides, the answers are the same bit for bit
    sub_n = b.hapsubsets(columns=True, narrow_hash=True)
    narrow = fetch(b, with_genome)
    np.testing.assert_array_equal(sub_n, sub)
    for v in with_genome:
        for x, y in zip(narrow[1][v], normal[1][v]):
            np.testing.assert_array_equal(x, y)
    # the pass's own answers, and the batch, are what they were
    rec2, tru2 = b.haplotype_counts()
    np.testing.assert_array_equal(rec2, pass_before[0])
    np.testing.assert_array_equal(tru2, pass_before[1])
    for k, v in enumerate(with_genome):
        for x, y in zip(b.haplotyped(v), pass_before[2][k]):
            np.testing.assert_array_equal(x, y)
    for v in range(b.n_vcf):
        np.testing.assert_array_equal(b.cls(v), base[0][v])
    np.testing.assert_array_equal(b.scalars(), base[1])
    np.testing.assert_array_equal(b.roc(), base[2])
    if gap == 10:                                                       # what the family plants arrives on the device
        hs.present(e, {(v, 10): setup.restated(v, 10) for v in with_genome})
        main = e.index("main")
        assert int(sub[main][U["partial"]]) == 13 and int(sub[main][U["nosubset"]]) == 3
        assert int(sub[e.index("other")][U["partial"]]) == 1


def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    e = hs.family()
    gid, gid2 = engine.genome_load(e.genome.encode("latin-1")), engine.genome_load(e.genome.encode("latin-1"))
    tid, tid2 = engine.truth_load(*e.tcodes[0]), engine.truth_load(*e.tcodes[0])
    cols = e.cols[e.index("main")]
    n = len(cols[0])
    b = engine.batch([n, n], [tid, tid2], alleles=True)
    try:
        for v in range(2):
            b.upload(v, *cols)
        c, msg = refused(b.hapsubsets)
        assert c == QM_E_STATE and "qm_batch_finish first" in msg
        b.run()
        b.finish()
        c, msg = refused(b.hapsubsets)                                  # no haplotype call
        assert c == QM_E_STATE and "no qm_batch_haplotypes behind the latest run" in msg
        bytes0 = b.device_bytes
        rec, tru = b.haplotypes([gid, gid2])
        bytes1 = b.device_bytes
        for getter in (b.hapsubset_counts, lambda: b.hapsubsetted(0), b.hapsubset_timings):
            c, msg = refused(getter)                                    # getters before the search
            assert c == QM_E_STATE and "no qm_batch_hapsubsets behind the latest qm_batch_haplotypes" in msg
        call = lambda what: b._L.qm_batch_hapsubsets(b._h, what, None)
        assert call(1) == QM_E_INVAL and call(8) == QM_E_INVAL and call(2 | 16) == QM_E_INVAL
        c, msg = refused(lambda: b.hapsubsets(columns=True))            # the haplotype call kept no columns
        assert c == QM_E_STATE and "QM_HAP_COLUMNS" in msg
        assert b.device_bytes == bytes1 > bytes0                        # nothing of the search is allocated before it runs
        sub = b.hapsubsets()
        assert b.device_bytes > bytes1 and int(sub[0][U["partial"]]) == 13
        np.testing.assert_array_equal(sub[0], sub[1])
        c, msg = refused(lambda: b.hapsubsetted(0))                     # that search kept no columns
        assert c == QM_E_STATE and "QM_HAPSUB_COLUMNS" in msg
        _, _, site_s, sm, tm = b.hapsubsetted(0, columns=False)         # the sites and masks come without them
        assert len(site_s) == 13 and sm.min() >= 1 and tm.min() >= 1
        m = np.zeros(1, np.int64)
        few = np.zeros(4, np.int32)
        assert b._L.qm_batch_get_hapsubsetted(b._h, 0, None, None, few.ctypes.data, None, None, 4, m.ctypes.data_as(b._L.qm_batch_get_hapsubsetted.argtypes[8])) == -5
        assert int(m[0]) == 13 and few.tolist() == site_s[:4].tolist()  # QM_E_RANGE: the number, and what fits
        assert b._L.qm_batch_get_hapsubsetted(b._h, 2, None, None, None, None, None, 0, None) == QM_E_INVAL      # the batch has two VCFs
        assert b._L.qm_batch_get_hapsubsetted(b._h, -1, None, None, None, None, None, 0, None) == QM_E_INVAL
        c, msg = refused(b.hapsubset_timings)
        assert c == QM_E_STATE and "timing is off" in msg
        b.set_timing(True)
        b.haplotypes([gid, gid2], columns=True)                         # a second haplotype call forgets the search
        c, msg = refused(b.hapsubset_counts)
        assert c == QM_E_STATE and "no qm_batch_hapsubsets" in msg
        sub2 = b.hapsubsets(columns=True)
        np.testing.assert_array_equal(sub2, sub)
        ms = b.hapsubset_timings()
        assert set(ms) == {"hap_subsets_ms"} and ms["hap_subsets_ms"] >= 0
        assert set(b.haplotype_timings()) == {"hap_sites_ms", "hap_records_ms", "hap_truth_ms", "hap_claim_ms", "hap_replay_ms"}
        b.haplotypes([gid, -1], columns=True)                           # a VCF without a genome
        sub3 = b.hapsubsets(columns=True)
        np.testing.assert_array_equal(sub3[0], sub[0])
        assert not sub3[1].any()
        c, msg = refused(lambda: b.hapsubsetted(1))
        assert c == QM_E_STATE and "named no genome" in msg
        b.haplotypes([gid, gid2], columns=True)
        b.run()                                                         # a run since
        b.finish()
        c, msg = refused(b.hapsubsets)
        assert c == QM_E_STATE and "no qm_batch_haplotypes behind the latest run" in msg
        c, msg = refused(b.hapsubset_counts)
        assert c == QM_E_STATE
        b.haplotypes([gid, gid2], columns=True)
        engine.genome_release(gid2)                                     # a released genome of that call
        gid2 = None
        c, msg = refused(b.hapsubsets)
        assert c == QM_E_STATE and "released genome" in msg
        b.haplotypes([gid, -1], columns=True)
        np.testing.assert_array_equal(b.hapsubsets()[0], sub[0])        # ... the call that does not name it runs
        engine.truth_release(tid2)                                      # a released truth set of the batch
        tid2 = None
        c, msg = refused(b.hapsubsets)
        assert c == QM_E_STATE and "was released" in msg
    finally:
        b.close()
        for t in (tid, tid2):
            if t is not None:
                engine.truth_release(t)
        for g in (gid, gid2):
            if g is not None:
                engine.genome_release(g)


def test_lists_far_past_the_cap_are_not_searched(engine):
    """the family of the haplotype tests some hundred times over in one VCF, shuffled: about 70 000 records, more than one
    workgroup of the record walks, every open line hundreds of times.  Every tried site whose lines are distinct spellings is
    TOOMANY and is not searched; what is searched equals the restatement."""
    fam = Family(22, repeats=1)
    truth = truth_codes(fam.truth)
    rng = np.random.default_rng(1)
    recs = fam.recs * (70000 // len(fam.recs) + 1)
    rng.shuffle(recs)
    cols = codes(recs)
    gid, tid = engine.genome_load(fam.genome.encode()), engine.truth_load(*truth)
    b = engine.batch([len(recs)], [tid], alleles=True)
    try:
        b.upload(0, *cols)
        b.run()
        b.finish()
        c = b.cls(0)
        rec, tru = b.haplotypes([gid], columns=True)
        sub = b.hapsubsets(columns=True)
        cls, site, ecls = b.haplotyped(0)
        cls_s, ecls_s, site_s, sm, tm = b.hapsubsetted(0)
        detail = []
        wsub, wcls, wecls = hp.subset_counts(fam.genome, truth, cols[0], cols[1], cols[2], cols[4], (c & 1).astype(bool), (c & 2).astype(bool),
                                             detail=detail)
        np.testing.assert_array_equal(sub[0], wsub)
        np.testing.assert_array_equal(cls_s, wcls)
        np.testing.assert_array_equal(ecls_s, wecls)
        assert list(zip(site_s.tolist(), sm.tolist(), tm.tolist())) == [d[:3] for d in detail]
        assert int(rec[0][R["toomany"]]) > 800
        toomany = set(site[cls == hp.TOOMANY].tolist())
        assert toomany and not toomany & set(site_s.tolist())
        np.testing.assert_array_equal(cls_s[cls == hp.TOOMANY], cls[cls == hp.TOOMANY])
        assert int(sub[0][U["searched"]]) == int(tru[0][T["tried"]]) - int(tru[0][T["matched"]]) - len(toomany)
        np.testing.assert_array_equal(b.hapsubsets(columns=True, narrow_hash=True), sub)
    finally:
        b.close()
        engine.truth_release(tid)
        engine.genome_release(gid)


def test_a_refused_haplotype_call_leaves_the_previous_one_searchable(engine):
    """qm_batch_haplotypes refuses two VCFs that share a truth set and name two genomes AFTER it has laid out the entry offsets of
    the new call: the offsets are committed with the call, so the search and the getters behind the refusal still read the
    previous call's arrays with the previous call's sizes (one VCF with a genome, then two asked for)"""
    e = hs.family()
    gid, gid2 = engine.genome_load(e.genome.encode("latin-1")), engine.genome_load(e.genome.encode("latin-1"))
    tid = engine.truth_load(*e.tcodes[0])
    cols = e.cols[e.index("main")]
    b = engine.batch([len(cols[0])] * 2, [tid, tid], alleles=True)
    try:
        for v in range(2):
            b.upload(v, *cols)
        b.run()
        b.finish()
        b.haplotypes([-1, gid], columns=True)
        before = b.haplotyped(1)
        b.hapsubsets(columns=True)
        first = fetch(b, [1])
        c, msg = refused(lambda: b.haplotypes([gid, gid2], columns=True))
        assert c == QM_E_INVAL and "share truth set" in msg
        for x, y in zip(b.haplotyped(1), before):
            np.testing.assert_array_equal(x, y)
        b.hapsubsets(columns=True)
        again = fetch(b, [1])
        np.testing.assert_array_equal(again[0], first[0])
        for x, y in zip(again[1][1], first[1][1]):
            np.testing.assert_array_equal(x, y)
        assert int(again[0][1][U["partial"]]) == 13 and not again[0][0].any()
    finally:
        b.close()
        engine.truth_release(tid)
        engine.genome_release(gid)
        engine.genome_release(gid2)
