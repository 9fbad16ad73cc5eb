"""The QUAL ROC under normal-form and atom matching (quasimodo_amd.rescueroc) without a device: hand-derived
literals, an independent double loop over every threshold that counts with normalize.py / atomize.py directly, the conditions
the GPU comparisons rest on, the table writers and the refusals of the flag."""
import gzip
import os

import numpy as np
import pytest

from quasimodo_amd import atomize as at
from quasimodo_amd import normalize as nz
from quasimodo_amd import rescueroc as rr
from quasimodo_amd import tables
import rescueroc_family as fam

ID = 2            # QM_F_IDDOT


def cols_of(recs):
    """recs: [(pos, REF, ALT, QUAL, flags)] as strings"""
    return (np.array([r[0] for r in recs], np.int32), np.array([nz.code(r[1]) for r in recs], np.int32),
            np.array([nz.code(r[2]) for r in recs], np.int32), np.array([r[3] for r in recs], np.float32),
            np.array([r[4] for r in recs], np.uint8))


def truth_of(vs):
    return (np.array([v[0] for v in vs], np.int32), np.array([nz.code(v[1]) for v in vs], np.int32),
            np.array([nz.code(v[2]) for v in vs], np.int32))


def steps(n_bins, *pairs):
    """a non-increasing row: value v for every t <= upto, pairs given with upto ascending"""
    row = np.zeros(n_bins, np.uint64)
    for upto, v in reversed(pairs):
        row[:upto + 1] = v
    return row


# ---- literals ---------------------------------------------------------------------------------------------------------------
def test_a_deletion_in_a_repeat_spelled_three_ways():
    """G[100 .. 103] = CAAA; the deletion of one A is CAAA -> CAA at 100, AA -> A at 102 and CA -> C at 100: one form.  At QUAL
    5, 30 and 200 the three lines are TP_N down to their own thresholds, and the one form is found up to 200."""
    g = ("ACGT" * 25)[:99] + "CAAAT" + "GCGC"
    truth = truth_of([(100, "CA", "C")])
    c = cols_of([(100, "CAAA", "CAA", 5, ID), (102, "AA", "A", 30, ID), (100, "CA", "C", 200, ID)])
    d = {}
    roc, base = rr.sweep_norm(g, truth, *c, n_bins=256, detail=d)
    assert base == 1 and d["best"] == {(100, nz.code("CA"), nz.code("C")): 200}
    np.testing.assert_array_equal(roc[0], steps(256, (5, 3), (30, 2), (200, 1)))
    assert not roc[1].any()
    np.testing.assert_array_equal(roc[2], steps(256, (200, 1)))
    # by atoms none of them is atomisable: the verdict by spelling, which only the third line has
    roc_a, base_a = rr.sweep_atom(truth, *c, n_bins=256)
    assert base_a == 1
    np.testing.assert_array_equal(roc_a[0], steps(256, (200, 1)))
    np.testing.assert_array_equal(roc_a[1], steps(256, (5, 2), (30, 1)))
    np.testing.assert_array_equal(roc_a[2], steps(256, (200, 1)))
    # a line whose ID is not `.` hits and is still an FP line that carries nothing; QM_F_TPLINE makes a TP line of anything
    c2 = cols_of([(102, "AA", "A", 30, 0), (50, "A", "C", 40, 8)])
    roc, _ = rr.sweep_norm(g, truth, *c2, n_bins=256)
    np.testing.assert_array_equal(roc[0], steps(256, (40, 1)))
    np.testing.assert_array_equal(roc[1], steps(256, (30, 1)))
    assert not roc[2].any()
    # no genome: zero rows, zero baseline
    roc, base = rr.sweep_norm(None, truth, *c, n_bins=256)
    assert base == 0 and not roc.any()


def test_an_mnp_beside_two_truth_snvs():
    """G[7 .. 8] = AC, the truth set holds A -> G at 7 and C -> T at 8, a haplotype caller writes AC -> GT at 7: by spelling one
    FP and two FNs at every threshold, by atoms one TP line that finds both entries"""
    truth = truth_of([(7, "A", "G"), (8, "C", "T")])
    c = cols_of([(7, "AC", "GT", 50, ID), (8, "C", "T", 10, ID)])
    d = {}
    roc, base = rr.sweep_atom(truth, *c, n_bins=256, detail=d)
    assert base == 2
    np.testing.assert_array_equal(roc[0], steps(256, (10, 2), (50, 1)))
    assert not roc[1].any()
    np.testing.assert_array_equal(roc[2], steps(256, (50, 2)))          # the SNV at QUAL 10 adds nothing: its atom has 50 already
    assert d["best_atom"] == {at.atom_key(7, "A", "G"): 50, at.atom_key(8, "C", "T"): 50}


def test_the_best_of_an_atomisable_entry_is_the_minimum_over_its_atoms():
    """the truth set spells the MNP, two callers' lines carry one atom each, at QUAL 50 and at QUAL 10: the entry is whole from
    threshold 10 down; with one carrier alone it is never whole"""
    truth = truth_of([(7, "AC", "GT")])
    c = cols_of([(7, "A", "G", 50, ID), (8, "C", "T", 10, ID)])
    d = {}
    roc, base = rr.sweep_atom(truth, *c, n_bins=256, detail=d)
    assert base == 1 and d["best"] == {0: 10}
    np.testing.assert_array_equal(roc[2], steps(256, (10, 1)))
    np.testing.assert_array_equal(roc[0], steps(256, (10, 2), (50, 1)))  # both lines have all their atoms in the set
    roc, _ = rr.sweep_atom(truth, *cols_of([(7, "A", "G", 50, ID)]), n_bins=256, detail=d)
    assert d["best"] == {} and not roc[2].any()
    # a partial record carries the atom it hits: ACG -> GTC at 7 hits two of three atoms and is an FP line itself
    roc, _ = rr.sweep_atom(truth, *cols_of([(7, "ACG", "GTC", 33, ID)]), n_bins=256, detail=d)
    assert d["best"] == {0: 33}
    np.testing.assert_array_equal(roc[1], steps(256, (33, 1)))
    assert not roc[0].any()


def test_qual_bins():
    for q, want in ((np.nan, -1), (-1.0, -1), (-np.inf, -1), (-0.5, -1), (0.0, 0), (19.999, 19), (20.0, 20), (255.9, 255), (256.0, 255), (np.inf, 255)):
        assert rr.qual_bin(q, 256) == want, q
    assert rr.qual_bin(19.999, 20) == 19 and rr.qual_bin(20.0, 20) == 19 and rr.qual_bin(20.0, 21) == 20 and rr.qual_bin(7.0, 1) == 0


# ---- an independent double loop ---------------------------------------------------------------------------------------------
def exact_tp(truth, pos, ref, alt, flags, kept):
    index = set(nz.truth_order(*truth))
    out = np.zeros(len(pos), bool)
    for i in range(len(pos)):
        f = int(flags[i])
        hit = not f & 4 and (int(pos[i]), int(ref[i]), int(alt[i])) in index
        out[i] = kept[i] and bool((hit and f & 2) or f & 8)
    return out


@pytest.mark.parametrize("which, n_truth, n_bins", [(0, 120, 40), (1, 65, 21)], ids=["g600", "g17"])
def test_against_a_filter_at_every_threshold(which, n_truth, n_bins):
    """for every t: keep the records with bin >= t, count TP lines and found units with normalize.counts / atomize.counts"""
    rng = np.random.default_rng(77 + which)
    g = fam.GENOMES[which]
    tvs = fam.truth_set(g, rng, n_truth)
    truth = fam.codes(tvs)
    pos, ref, alt, qual, flags = fam.records(g, rng, 160, tvs, False)
    qual = np.where(np.isfinite(qual) & (qual > 30), qual / 8, qual).astype(np.float32)   # spread over the 40 / 21 bins
    roc_n, roc_a, base = rr.sweep(g, truth, pos, ref, alt, qual, flags, n_bins)
    ok = lambda c: ((c >= 0) & (c < 4)) | (c >= 0x08000000)
    bins = np.array([rr.qual_bin(q, n_bins) for q in qual])
    da = {}
    rr.sweep_atom(truth, pos, ref, alt, qual, flags, n_bins, detail=da)
    for j, atoms in enumerate(da["per"]):      # an atomisable entry spelled like a carrier needs no second route
        if atoms is not None and j in da["best_entry"]:
            assert da["best"][j] >= da["best_entry"][j]
    assert len(set(bins.tolist())) > 10 and int(roc_n[2, 0]) > 3 and int(roc_a[2, 0]) > 3
    for t in range(n_bins):
        kept = ok(ref) & ok(alt) & (bins >= t)
        tp = exact_tp(truth, pos, ref, alt, flags, kept)
        rec, _ = nz.counts(g, truth, pos, ref, alt, flags, kept, tp)[:2]
        assert (int(roc_n[0, t]), int(roc_n[1, t])) == (int(rec[2]), int(rec[0]) - int(rec[2])), t
        carriers = kept & ((flags & 2) != 0)
        tru = nz.counts(g, truth, pos, ref, alt, flags, carriers, tp & carriers)[1]
        assert int(roc_n[2, t]) == int(tru[2]) and int(base[0]) == int(tru[1]), t
        rec = at.counts(truth, pos, ref, alt, flags, kept, tp)[0]
        assert (int(roc_a[0, t]), int(roc_a[1, t])) == (int(rec[2]), int(rec[0]) - int(rec[2])), t
        tru = at.counts(truth, pos, ref, alt, flags, carriers, tp & carriers)[1]
        assert int(roc_a[2, t]) == int(tru[5]) and int(base[1]) == int(tru[0]), t


# ---- what the GPU comparisons rest on ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_the_draws_of_the_gpu_tests_are_not_vacuous(sorted_):
    for kw in (dict(), dict(pass_is_bin=True, all_iddot=True)):
        tvs, truths, cols = fam.family(41, sorted_, **kw)
        tot = [dict(rescued_n=0, rescued_a=0, partial_entries=0, bins_n=0, bins_a=0) for _ in fam.GENOMES]
        for v, (c, w) in enumerate(zip(cols, fam.WHICH)):
            if len(c[0]) > 1100:
                continue                           # (the large VCFs are drawn like the small ones)
            got = fam.conditions(fam.GENOMES[w], truths[w], c, pass_is_bin=bool(kw))
            for k in tot[w]:
                tot[w][k] = max(tot[w][k], got[k]) if k.startswith("bins") else tot[w][k] + got[k]
            if kw:
                assert got["pass_is_bin"] and got["all_iddot"], v
        for k in ("rescued_n", "rescued_a", "partial_entries"):                  # per family
            assert sum(t[k] for t in tot) > 0, (k, tot)
        for w, t in enumerate(tot):                                               # per truth set
            assert t["rescued_n"] > 0 and t["rescued_a"] > 0, (w, t)
            assert t["bins_n"] > 1 and t["bins_a"] > 1, (w, t)
        for w, n in enumerate(fam.TRUTH_N):
            assert len(nz.truth_order(*truths[w])) == n


# ---- files ------------------------------------------------------------------------------------------------------------------
def test_write_rescue_roc_literal(tmp_path):
    roc = np.zeros((3, 4), np.uint64)
    roc[0] = [3, 2, 1, 0]
    roc[1] = [2, 1, 0, 0]
    roc[2] = [2, 2, 1, 0]
    p = str(tmp_path / "normalized_roc.tsv.gz")
    tables.write_rescue_roc(p, roc, 4, "normalized")
    text = gzip.open(p, "rb").read().decode()
    assert text == ("#Version qmvt normal-form ROC (not rtg vcfeval), baseline = distinct normal forms of the truth entries\n"
                    "#total baseline variants: 4\n#score field: QUAL\n"
                    "#score\ttrue_positives_baseline\tfalse_positives\ttrue_positives_call\tfalse_negatives\tprecision\tsensitivity\tf_measure\n"
                    "2\t1\t0\t1\t3\t1.0000\t0.2500\t0.4000\n"
                    "1\t2\t1\t2\t2\t0.6667\t0.5000\t0.5714\n"
                    "0\t2\t2\t3\t2\t0.6000\t0.5000\t0.5455\n")
    q = str(tmp_path / "again.tsv.gz")
    tables.write_rescue_roc(q, roc, 4, "normalized")
    assert open(p, "rb").read() == open(q, "rb").read()
    tables.write_rescue_roc(q, roc, 4, "atomized")
    assert gzip.open(q, "rb").read().decode().splitlines()[0] == "#Version qmvt atom ROC (not rtg vcfeval), baseline = allele-extended truth entries"
    # the spelling file is the batch's own ROC in the layout of write_weighted_roc
    tables.write_rescue_roc(q, roc, 4, "spelling")
    w = str(tmp_path / "weighted.tsv.gz")
    tables.write_weighted_roc(w, roc, 4)
    assert gzip.open(q, "rb").read().decode().splitlines()[1:] == gzip.open(w, "rb").read().decode().splitlines()[1:]
    with pytest.raises(KeyError):
        tables.write_rescue_roc(q, roc, 4, "haplotype")


def test_caller_roc_rescue_table_literal(tmp_path):
    """TP 3, FP 1, U 2 of 4 at t = 20: precision 0.75, recall 0.5, F1 0.6; the largest F1 sits at t = 5 and 6 alike: t = 5"""
    roc = np.zeros((3, 256), np.uint64)
    roc[0] = steps(256, (6, 6), (20, 3), (30, 1))
    roc[1] = steps(256, (4, 9), (6, 2), (20, 1))
    roc[2] = steps(256, (6, 4), (20, 2), (30, 1))
    assert rr.operating_point(roc, 4, 20) == [3, 1, 2, 0.75, 0.5, 0.6]
    t, row = rr.best_f1(roc, 4)
    assert t == 5 and row == [6, 2, 0, 0.75, 1.0, 0.857]
    assert rr.operating_point(roc, 4, 31) == [0, 0, 4, None, None, None]
    empty = np.zeros((3, 256), np.uint64)
    assert rr.best_f1(empty, 4) == (None, [0, 0, 4, None, None, None])
    stats = {"rroc": {m: (roc, 4) for m in rr.MATCHINGS}}
    p = str(tmp_path / "caller_roc_rescue.tsv")
    rr.write_caller_roc_rescue(p, [("lofreq", "mix-1-1", stats), ("lofreq", "mix-1-0", {}), ("lofreq", "mix-2-1", stats)])
    lines = open(p).read().split("\n")
    assert lines[0] == "\t".join(rr.TABLE_HEADER[0] + rr.TABLE_HEADER[1]) and lines[-1] == ""
    assert lines[1] == "LoFreq\tmix-1-1\tspelling\t3\t1\t2\t0.75\t0.5\t0.6\t5\t6\t2\t0\t0.75\t1\t0.857"
    assert [ln.split("\t")[:3] for ln in lines[1:-1]] == (
        [["LoFreq", s, m] for s in ("mix-1-1", "mix-2-1") for m in rr.MATCHINGS] + [["LoFreq", "pooled", m] for m in rr.MATCHINGS])
    assert lines[7] == "LoFreq\tpooled\tspelling\t6\t2\t4\t0.75\t0.5\t0.6\t5\t12\t4\t0\t0.75\t1\t0.857"
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]


# ---- the flag ---------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_file(tmp_path):
    """check_alleles and the shared-call rule: without the allele-extended mode, beside normalize or atomize (the sweep runs
    them itself) or any other pass -- said before an engine is made or a file written"""
    from quasimodo_amd import passes, workflow
    from quasimodo_amd.extract import Job, extract_many
    p = next(x for x in passes.PASSES if x.name == "rescueroc")
    assert p == passes.Pass("rescueroc", ("rescue_roc",), ("rescue_roc",), "--rescue-roc", None, ())
    passes.check_alleles({"rescueroc"}, True)
    with pytest.raises(ValueError, match=r"^normalize \("):                      # (the one rule names the pass that was asked for, not this one)
        passes.check_alleles({"normalize"}, False)
    with pytest.raises(ValueError, match="--alleles"):
        passes.check_alleles({"rescueroc"}, False)
    for other in ("normalize", "atomize", "haplo", "vartype", "motifs"):
        with pytest.raises(passes.SharedCallError) as ei:
            passes.check_shared_call({"rescueroc", other})
        assert "--rescue-roc" in ei.value.for_cli()
    vcf, truth, fa = tmp_path / "TM-1-1.TM.c.vcf", tmp_path / "t.vcf", tmp_path / "g.fa"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t50\tPASS\t.\n")
    truth.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t.\t.\t.\n")
    fa.write_text(">c\nACATG\n")
    job = lambda: [Job(str(vcf), str(truth), "hcmv", "", "c")]
    before = sorted(os.listdir(str(tmp_path)))
    for kw, said in ((dict(rescue_roc=[str(fa)]), "--alleles"), (dict(alleles=False, rescue_roc={"genomes": [str(fa)]}), "--alleles"),
                     (dict(alleles=True, rescue_roc=[str(fa)], normalize=[str(fa)]), "does not combine"),
                     (dict(alleles=True, rescue_roc=[str(fa)], atomize=True), "does not combine"),
                     (dict(alleles=True, rescue_roc=[str(fa), str(fa)]), "2 genomes entries for 1 jobs")):
        with pytest.raises(ValueError, match=said):
            extract_many(job(), **kw)
    j = job()
    j[0].rescue_roc, j[0].atomize = str(fa), True                    # asked for through the Job fields
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(j, alleles=True)
    assert sorted(os.listdir(str(tmp_path))) == before
    for kw, said in ((dict(rescue_roc={"TM": str(fa), "TA": str(fa)}), "--rescue-roc needs --alleles"),
                     (dict(alleles=True, rescue_roc={"TM": str(fa), "TA": str(fa)}, normalize={"TM": str(fa), "TA": str(fa)}), "--rescue-roc cannot be combined with --normalize"),
                     (dict(alleles=True, rescue_roc={"TM": str(fa), "TA": str(fa)}, atomize=True), "--atomize cannot be combined with --rescue-roc")):
        with pytest.raises(workflow.WorkflowError, match=said):
            workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), **kw)
    assert sorted(os.listdir(str(tmp_path))) == before
