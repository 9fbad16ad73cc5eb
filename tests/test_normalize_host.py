"""The normal form of indels and MNPs (quasimodo_amd.normalize) without a device: hand-derived literals, the
property that makes a normal form one -- two variants have equal forms iff they turn the genome into the same sequence --, the
codec between allele codes and strings, the table writers and the refusals of the flag."""
import os

import numpy as np
import pytest

from quasimodo_amd import normalize as nz

BASES = "ACGT"


# ---- literals ---------------------------------------------------------------------------------------------------------------
def test_the_same_deletion_spelled_twice():
    """CAAA -> CAA at 100 and the deletion of one A spelled two bases further right (AA -> A at 102: with G[100 .. 103] = CAAA
    the REF at 102 starts with A) are both CA -> C at 100"""
    g = ("ACGT" * 25)[:99] + "CAAAT" + "GCGC"
    assert g[99:103] == "CAAA"
    assert nz.normalize(g, 100, "CAAA", "CAA") == (nz.RESPELLED, 100, "CA", "C")
    assert nz.normalize(g, 102, "AA", "A") == (nz.RESPELLED, 100, "CA", "C")
    assert nz.normalize(g, 100, "CA", "C") == (nz.UNCHANGED, 100, "CA", "C")


def test_an_mnp_that_is_an_snv():
    g = "GGTTGGACGG"
    assert g[6:8] == "AC"
    assert nz.normalize(g, 7, "AC", "AT") == (nz.RESPELLED, 8, "C", "T")
    assert nz.normalize(g, 8, "C", "T") == (nz.UNCHANGED, 8, "C", "T")
    assert nz.normalize(g, 6, "GAC", "GAT") == (nz.RESPELLED, 8, "C", "T")
    assert nz.normalize(g, 7, "ACG", "ATG") == (nz.RESPELLED, 8, "C", "T")


def test_insertion_in_a_dinucleotide_repeat_goes_to_its_start():
    g = "GGT" + "ACACACAC" + "TTG"
    assert nz.normalize(g, 9, "C", "CAC") == (nz.RESPELLED, 3, "T", "TAC")
    assert nz.normalize(g, 11, "C", "CAC") == (nz.RESPELLED, 3, "T", "TAC")
    assert nz.normalize(g, 6, "AC", "ACAC") == (nz.RESPELLED, 3, "T", "TAC")
    assert nz.normalize(g, 3, "T", "TAC") == (nz.UNCHANGED, 3, "T", "TAC")


def test_a_walk_that_reaches_the_first_base_stops_there():
    g = "AAAACGT"
    assert nz.normalize(g, 1, "AA", "A") == (nz.UNCHANGED, 1, "AA", "A")
    assert nz.normalize(g, 1, "AAA", "AA") == (nz.RESPELLED, 1, "AA", "A")
    assert nz.normalize(g, 3, "AA", "A") == (nz.RESPELLED, 1, "AA", "A")
    assert nz.normalize(g, 4, "AC", "C") == (nz.RESPELLED, 1, "AA", "A")
    assert nz.normalize(g, 1, "A", "AA") == (nz.UNCHANGED, 1, "A", "AA")
    assert nz.normalize(g, 4, "A", "AA") == (nz.RESPELLED, 1, "A", "AA")


def test_reasons():
    assert nz.normalize("GNAAAC", 4, "AA", "A") == (nz.NOBASE, 4, "AA", "A")         # the walk meets the N at 2
    assert nz.normalize("GNAAAC", 3, "AA", "A") == (nz.NOBASE, 3, "AA", "A")
    assert nz.normalize("ACGT", 2, "G", "T") == (nz.REFMISMATCH, 2, "G", "T")
    assert nz.normalize("ANGT", 1, "AC", "A") == (nz.REFMISMATCH, 1, "AC", "A")      # a no-base under the REF
    assert nz.normalize("ACGT", 2, "C", "C") == (nz.NOVAR, 2, "C", "C")
    assert nz.normalize("ACGT", 2, "CG", "CG") == (nz.NOVAR, 2, "CG", "CG")
    assert nz.normalize("ACGT", 4, "TT", "T") == (nz.RANGE, 4, "TT", "T")
    assert nz.normalize("ACGT", 0, "A", "C") == (nz.RANGE, 0, "A", "C")
    assert nz.normalize("ACGT", 5, "A", "C") == (nz.RANGE, 5, "A", "C")
    assert nz.normalize("ACGT", 2, "C", "T", nokey=True) == (nz.NOKEY, 2, "C", "T")
    long14 = "ACGTACGTACGTAC"
    assert nz.normalize(long14 * 2, 1, long14, "A") == (nz.LONG, 1, long14, "A")
    assert nz.normalize(long14 * 2, 1, "A", long14) == (nz.LONG, 1, "A", long14)
    assert nz.normalize(long14 * 2, 1, long14[:13], "A")[0] == nz.UNCHANGED          # 13 bases still have an inline code
    assert nz.normalize("acgt", 2, "C", "T") == (nz.UNCHANGED, 2, "C", "T")           # lower case counts as a base


# ---- the property ---------------------------------------------------------------------------------------------------------
def planted_norm_genome(seed=5, n=600):
    """random bases without N; a 70-base homopolymer (longer than a wave, across packed-word edges) at 101, a 40-base (AC)n at
    251 and a 30-base (ACG)n at 401 (1-based), each between bases that break the repeat"""
    rng = np.random.default_rng(seed)
    g = [BASES[i] for i in rng.integers(0, 4, n)]
    for start, unit, length in ((101, "A", 70), (251, "AC", 40), (401, "ACG", 30)):
        for k in range(length):
            g[start - 1 + k] = unit[k % len(unit)]
        g[start - 2] = "T"
        g[start - 1 + length] = "T"
    return "".join(g)


REPEATS = ((101, 70), (251, 40), (401, 30))


def near_repeat(p, lr):
    return any(p + lr - 1 >= s - 1 and p <= s + n for s, n in REPEATS)


def draw_variants(g, rng, n, in_repeats):
    """variants at p >= 2 whose REF is the genome's, alleles of 1 .. 13 bases: an event (delete d bases, insert up to 6, often
    a copy of what follows: a repeat unit more) padded by genome bases on either side, so that one event comes in many spellings"""
    out = []
    while len(out) < n:
        if in_repeats:
            s, ln = REPEATS[rng.integers(0, 3)]
            q = int(rng.integers(s - 2, s + ln + 2))
        else:
            q = int(rng.integers(2, len(g)))
        d = int(rng.integers(0, 7))
        k = int(rng.integers(0, 7))
        ins = g[q - 1 + d:q - 1 + d + k] if rng.random() < 0.6 else "".join(BASES[i] for i in rng.integers(0, 4, k))
        left, right = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        p = q - left
        if p < 2 or q - 1 + d + right > len(g):
            continue
        ref = g[p - 1:q - 1 + d + right]
        alt = g[p - 1:q - 1] + ins + g[q - 1 + d:q - 1 + d + right]
        if not 1 <= len(ref) <= 13 or not 1 <= len(alt) <= 13 or ref == alt:
            continue
        if in_repeats and not near_repeat(p, len(ref)):
            continue
        out.append((p, ref, alt))
    return out


def test_equal_forms_iff_equal_sequences():
    g = planted_norm_genome()
    assert g[100:170] == "A" * 70 and g[250:290] == "AC" * 20 and g[400:430] == "ACG" * 10 and "N" not in g
    rng = np.random.default_rng(11)
    vs = draw_variants(g, rng, 320, True) + draw_variants(g, rng, 130, False)
    assert sum(near_repeat(p, len(r)) for p, r, _ in vs) >= 300
    assert all(p >= 2 and g[p - 1:p - 1 + len(r)] == r for p, r, _ in vs)
    forms, seqs = [], []
    for p, r, a in vs:
        c, q, r2, a2 = nz.normalize(g, p, r, a)
        assert c in (nz.UNCHANGED, nz.RESPELLED), (p, r, a, c)
        assert len(r2) <= len(r) and len(a2) <= len(a) and g[q - 1:q - 1 + len(r2)] == r2       # never longer; still a REF
        assert nz.normalize(g, q, r2, a2) == (nz.UNCHANGED, q, r2, a2)                           # idempotent
        forms.append((q, r2, a2))
        seqs.append(g[:p - 1] + a + g[p - 1 + len(r):])
    n_equal = 0
    for i in range(len(vs)):
        for j in range(i + 1, len(vs)):
            assert (forms[i] == forms[j]) == (seqs[i] == seqs[j]), (vs[i], vs[j], forms[i], forms[j])
            n_equal += forms[i] == forms[j] and vs[i] != vs[j]
    assert n_equal >= 100                                                                        # the draw does hold respellings
    assert max(p - q for (p, _, _), (q, _, _) in zip(vs, forms)) >= 64                           # a walk longer than a wave


# ---- the codec ------------------------------------------------------------------------------------------------------------
def test_codec_round_trip():
    rng = np.random.default_rng(3)
    assert [nz.code(b) for b in BASES] == [0, 1, 2, 3]
    assert nz.code("CA") == (2 << 26) | 1 and nz.code("AC") == (2 << 26) | (1 << 2)
    for n in range(1, 14):
        for _ in range(20):
            s = "".join(BASES[i] for i in rng.integers(0, 4, n))
            c = nz.code(s)
            assert nz.is_inline(c) and nz.spell(c) == s and 0 <= c < nz.DICT
    for bad in ("", "ACGTACGTACGTAC", "AN", "a"):
        with pytest.raises(ValueError):
            nz.code(bad)
    for c in (-1, 4, 0x07ffffff, nz.DICT, nz.DICT | 5, 14 << 26):
        assert not nz.is_inline(c) and nz.spell(c) is None
    g = "GGTTGGACGG"
    assert nz.form_codes(g, 7, nz.code("AC"), nz.code("AT")) == (nz.RESPELLED, 8, 1, 3)
    assert nz.form_codes(g, 7, nz.DICT | 9, 0) == (nz.LONG, 7, nz.DICT | 9, 0)
    assert nz.form_codes(g, 7, -1, 0) == (nz.LONG, 7, -1, 0)


def test_constants_match_the_header():
    from quasimodo_amd import _lib
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "qmvt.h")).read()
    assert len(nz.R_COLS) == _lib.QM_NORM_R_COLS == 12 and len(nz.T_COLS) == _lib.QM_NORM_T_COLS == 5
    assert "#define QM_NORM_R_COLS 12" in text and "#define QM_NORM_T_COLS 5" in text and "#define QM_NORM_COLUMNS 2u" in text
    for k, name in enumerate(nz.CLASS_NAMES):
        assert "QM_NORM_C_%s = %d" % (name.upper(), k) in text
    for k, name in enumerate(("kept", "tp", "tp_n", "rescued", "respelled", "single", "long", "nokey", "novar", "range", "refmismatch", "nobase")):
        assert "QM_NORM_R_%s = %d" % (name.upper(), k) in text
    assert nz.INLINE_MAX == 13 and "#define QM_ALLELE_INLINE_MAX 13" in text
    assert _lib.QM_ABI_VERSION == 6
    for name in ("qm_batch_normalize", "qm_batch_get_normalize", "qm_batch_get_normalized", "qm_batch_normalize_timings",
                 "qm_truth_normalized", "qm_truth_entries", "qm_extract_files_normalize"):
        assert name in _lib.EXPORTS


def test_counts_restatement_on_a_small_case():
    """the per-VCF tables by hand: one truth deletion spelled untrimmed, found by a trimmed record; one SNV found exactly"""
    g = ("ACGT" * 25)[:99] + "CAAAT" + "GCGC"
    c = nz.code
    truth = ([100, 5], [c("CAAA"), c("A")], [c("CAA"), c("G")])
    pos = [102, 5, 5, 50, 100]
    ref = [c("AA"), c("A"), c("A"), c("C"), c("CAAA")]
    alt = [c("A"), c("G"), c("T"), c("C"), c("CAA")]
    flags = [3, 3, 3, 3, 1]                              # the last one is not kept
    kept = [True, True, True, True, False]
    tp = [False, True, False, False, False]
    rec, tru, cls, npos, nref, nalt, row = nz.counts(g, truth, pos, ref, alt, flags, kept, tp)
    assert dict(zip(nz.R_COLS, rec.tolist())) == {"kept": 4, "tp": 1, "tp_n": 2, "rescued": 1, "respelled": 1, "single_base": 0, "long": 0,
                                                  "nokey": 0, "novar": 1, "range": 0, "refmismatch": 0, "nobase": 0}
    assert dict(zip(nz.T_COLS, tru.tolist())) == {"entries": 2, "forms": 2, "found": 2, "found_by_form_only": 1, "not_normalisable": 0}
    assert cls.tolist() == [nz.RESCUED, nz.UNCHANGED, nz.UNCHANGED, nz.NOVAR, nz.RESPELLED]
    assert (npos.tolist(), nref.tolist(), nalt.tolist()) == ([100, 5, 5, 50, 100], [c("CA"), 0, 0, 1, c("CA")], [1, 2, 3, 1, 1])
    assert row.tolist() == [1, 0, -1, -1, 1]             # the table's order: the key of position 5 first


# ---- writers, paths and refusals ------------------------------------------------------------------------------------------
def test_table_writer_and_rescued_reader(tmp_path):
    from quasimodo_amd.extract import Job, _paths
    rec = np.array([10, 4, 7, 3, 5, 1, 1, 0, 0, 2, 0, 1], np.uint64)
    tru = np.array([9, 8, 6, 2, 1], np.uint64)
    row = nz.performance_row(rec, tru)
    # by spelling: 4 of 10 lines, 6 - 2 = 4 of 8 forms; by normal form: 7 of 10 lines, 6 of 8 forms; R's round(x, 3)
    assert row[:6] == [4, 6, 4, 0.4, 0.5, 0.444] and row[6:12] == [7, 3, 2, 0.7, 0.75, 0.724]
    assert row[12:] == [3, 5, 1, 1, 0, 0, 2, 0, 1, 9, 8, 1]
    assert nz.performance_row(np.zeros(12, np.uint64), tru)[:6] == [0, 0, 4, None, None, None]
    path = tmp_path / "t.tsv"
    nz.write_performance_normalized(str(path), [("lofreq", "TA-1-10", {"norm_rec": rec, "norm_tru": tru}), ("lofreq", "TA-1-0", {"n_pass": 3}),
                                                ("mine", "TM-1-1", {"norm_rec": np.zeros(12, np.uint64), "norm_tru": tru})])
    lines = path.read_text().split("\n")
    assert lines[0].split("\t") == ["caller", "mixture", "TP", "FP", "FN", "Precision", "Recall", "F1", "TP_N", "FP_N", "FN_N", "Precision_N",
                                    "Recall_N", "F1_N", "rescued", "respelled", "single_base", "long", "nokey", "novar", "range", "refmismatch",
                                    "nobase", "truth_entries", "truth_forms", "truth_not_normalisable"]
    assert lines[1] == "LoFreq\tTA-1-10\t4\t6\t4\t0.4\t0.5\t0.444\t7\t3\t2\t0.7\t0.75\t0.724\t3\t5\t1\t1\t0\t0\t2\t0\t1\t9\t8\t1"
    assert lines[2].split("\t")[:8] == ["mine", "TM-1-1", "0", "0", "4", "NA", "NA", "NA"] and lines[3:] == [""]   # the pure-strain job is left out
    nz.write_performance_normalized(str(path), [("a", None, {"norm_rec": rec, "norm_tru": tru})], custom=True)
    assert path.read_text().split("\n")[0].split("\t")[:3] == ["caller", "TP", "FP"] and path.read_text().split("\n")[1].startswith("a\t4\t6")
    j = Job("/x/callers/lofreq/TA-1-10.AD169.lofreq.vcf", "/x/t.vcf", "hcmv")
    _paths(j)
    assert nz.rescued_path(j) == "/x/callers/lofreq/norm/TA-1-10.AD169.lofreq.rescued.tsv"
    res = tmp_path / "r.tsv"
    res.write_text(nz.RESCUED_HEADER + "\n12\t102\tAA\tA\t100\tCA\tC\t100\tCAAA\tCAA\n40\t7\tAC\tAT\t8\tC\tT\t.\t.\t.\n")
    assert nz.read_rescued(str(res)) == [(12, ("102", "AA", "A"), (100, "CA", "C"), (100, "CAAA", "CAA")), (40, ("7", "AC", "AT"), (8, "C", "T"), None)]
    res.write_text("#line\tPOS\n")
    with pytest.raises(ValueError):
        nz.read_rescued(str(res))


def test_refusals_in_front_of_any_file(tmp_path):
    from quasimodo_amd import passes, workflow
    from quasimodo_amd.extract import Job, extract_many
    p = [x for x in passes.PASSES if x.name == "normalize"]
    assert len(p) == 1 and p[0].flag == "--normalize" and p[0].shares == () and p[0].fields == ("normalize",)
    fa, fb = str(tmp_path / "a.fa"), str(tmp_path / "b.fa")
    mk = lambda: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i) for i in range(2)]
    with pytest.raises(ValueError, match="--alleles"):                          # --normalize without --alleles
        extract_many(mk(), normalize=[fa, fa])
    with pytest.raises(ValueError, match="--alleles"):
        extract_many(mk(), alleles=False, normalize={"genomes": [fa, None]})
    with pytest.raises(ValueError, match="a normalised truth set belongs to one genome") as ei:   # two genomes for one truth set
        extract_many(mk(), alleles=True, normalize=[fa, fb])
    assert "s.c0.vcf" in str(ei.value) and "s.c1.vcf" in str(ei.value) and "a.fa" in str(ei.value) and "b.fa" in str(ei.value)
    with pytest.raises(ValueError, match="genomes entries"):
        extract_many(mk(), alleles=True, normalize=[fa])
    for other in (dict(fn=True), dict(strata=[("all", [0], [100])]), dict(boot={}), dict(explain=3), dict(surface=True),
                  dict(context={"genomes": [fa, fa]}), dict(genomes=[fa, fa])):
        with pytest.raises(ValueError, match="does not combine"):
            extract_many(mk(), alleles=True, normalize=[fa, fa], **other)
    with pytest.raises(passes.SharedCallError):
        passes.check_shared_call({"normalize", "motifs"})
    passes.check_alleles({"normalize"}, True)
    with pytest.raises(workflow.WorkflowError, match="--normalize needs --alleles"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), normalize={"TM": fa, "TA": fa})
    with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, normalize={"TM": fa, "TA": fa}, truth_side=True)
    assert not any(x.is_file() for x in tmp_path.rglob("*"))                    # no file was written
