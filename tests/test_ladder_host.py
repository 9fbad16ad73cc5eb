"""The restatement of the ladder (quasimodo_amd.ladder) on the host: hand-written literals on a small genome, the
identities that tie its rows to the four producers on a planted draw, the cumulative table against a direct count over the
per-line tiers, the writers on literal input -- and the conditions of the draw the GPU tests compare the device on, so that
those cannot pass vacuously."""
import numpy as np
import pytest

from haplo_family import codes, host_masks, truth_codes
from ladder_family import LadderFamily, conditions
from quasimodo_amd import haplo as hp
from quasimodo_amd import ladder as ld
from quasimodo_amd import normalize as nz

K, S, N, A, H, B = ld.M_K, ld.M_S, ld.M_N, ld.M_A, ld.M_H, ld.M_B
ID = hp.F_IDDOT


def small():
    """400 bases of TGCA with the blocks written in; (genome, truth variants, records)"""
    g = list("TGCA" * 100)

    def put(p, s):
        g[p - 1:p - 1 + len(s)] = list(s)

    put(20, "GAAAAAAC")                                  # a run of six A behind a G
    put(71, "AC")
    for b in (121, 171, 221):
        put(b, "ACG")
    truth = [(20, "GA", "G"),                            # a deletion, left-aligned
             (71, "A", "G"), (72, "C", "T"),             # two adjacent SNVs
             (121, "A", "T"), (121, "ACG", "A"),         # an SNV plus a deletion
             (171, "A", "T"), (171, "ACG", "A"),         # the same, in a site with a line too many
             (221, "A", "T"), (221, "ACG", "A"),         # the same, behind a line with an ID
             (371, "C", "G")]
    recs = [(23, "AA", "A", True, ID),                   # the deletion respelled inside the repeat
            (71, "AC", "GT", True, ID),                  # AC>GT beside the two truth SNVs
            (121, "ACG", "T", True, ID),                 # ACG>T against SNV plus deletion
            (171, "ACG", "T", True, ID),                 # ... chosen by the subset search
            (176, "A", "C", True, ID),                   # ... and the line it leaves
            (221, "ACG", "T", True, 0),                  # a matched site's line whose ID is not '.'
            (271, "C", "A", True, ID),                   # a plain FP
            (321, "T", "A", False, ID),                  # not kept
            (371, "C", "G", True, ID)]                   # a TP by spelling
    return "".join(g), truth, recs


def restated(genome_n, genome_h, subsets, detail=None):
    g, truth, recs = small()
    cols, tc = codes(recs), truth_codes(truth)
    kept, tp = host_masks(cols, tc)
    out = ld.masks(g if genome_n else None, g if genome_h else None, tc, cols[0], cols[1], cols[2], cols[4], kept, tp, subsets=subsets, detail=detail)
    order = nz.truth_order(*tc)
    by_entry = {(p, nz.spell(r), nz.spell(a)): int(out[3][j]) for j, (p, r, a) in enumerate(order)}
    return out, by_entry


def test_literals_with_every_method():
    detail = {}
    (rec, tru, mask, emask), ent = restated(True, True, True, detail)
    assert mask.tolist() == [K | N | H, K | A | H, K | H, K | B, K, K, K, 0, K | S]
    assert detail["hap"][2][5] == hp.RESCUED and detail["hap"][2][2] == hp.RESCUED       # the line with an ID: its class says RESCUED
    assert detail["sub"][1][3] == hp.SUBSET and detail["sub"][1][4] == hp.LEFT
    assert ent == {(20, "GA", "G"): N | H, (71, "A", "G"): A | H, (72, "C", "T"): A | H, (121, "A", "T"): H, (121, "ACG", "A"): H,
                   (171, "A", "T"): B, (171, "ACG", "A"): B, (221, "A", "T"): H, (221, "ACG", "A"): H, (371, "C", "G"): S | N | A}
    want = np.zeros(18, np.uint64)
    want[[ld.KEPT, ld.TP]] = 8, 1
    for m, c in ((0, 3), (N | H, 1), (A | H, 1), (H, 1), (B, 1)):
        want[ld.CELL0 + m] = c
    np.testing.assert_array_equal(rec, want)
    want[:] = 0
    want[[ld.KEPT, ld.TP]] = 10, 1
    for m, c in ((N | H, 1), (A | H, 2), (H, 4), (B, 2)):
        want[ld.CELL0 + m] = c
    np.testing.assert_array_equal(tru, want)
    # the ladder: spelling, + normal form, + atoms, + haplotype, + subset
    assert ld.cumulative(rec, tru) == [(1, 7, 9), (2, 6, 8), (3, 5, 6), (4, 4, 2), (5, 3, 0)]
    ld.identities(rec, tru, emask, norm=detail["norm"][:2], atom=detail["atom"][:2], hap=detail["hap"][:2], sub=detail["sub"][0])


def test_literals_without_the_subset_search():
    (rec, tru, mask, emask), ent = restated(True, True, False)
    assert mask.tolist() == [K | N | H, K | A | H, K | H, K, K, K, K, 0, K | S]
    assert ent[(171, "A", "T")] == 0 and ent[(171, "ACG", "A")] == 0 and ent[(121, "A", "T")] == H
    assert int(rec[ld.CELL0]) == 4 and ld.cells_with(rec, B) == 0 and ld.cells_with(tru, B) == 0


@pytest.mark.parametrize("genome_n, genome_h", [(False, False), (True, False), (False, True)])
def test_literals_of_a_vcf_without_a_genome(genome_n, genome_h):
    """-1 in the normalisation call: no N; -1 in the haplotype call: no H and no B; the VCF takes part with what is left"""
    (rec, tru, mask, emask), ent = restated(genome_n, genome_h, True)
    n, h, b = (N if genome_n else 0), (H if genome_h else 0), (B if genome_h else 0)
    assert mask.tolist() == [K | n | h, K | A | h, K | h, K | b, K, K, K, 0, K | S]
    assert ent[(20, "GA", "G")] == n | h and ent[(71, "A", "G")] == A | h and ent[(371, "C", "G")] == S | n | A
    assert ent[(171, "A", "T")] == b and ent[(121, "ACG", "A")] == h
    if not genome_n:
        assert ld.cells_with(rec, N) == 0 and ld.cells_with(tru, N) == 0
    if not genome_h:
        assert ld.cells_with(rec, H | B) == 0 and ld.cells_with(tru, H | B) == 0


# ---- the planted draw of the GPU tests ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def draw():
    fam = LadderFamily(7)
    cols = fam.columns()
    detail = {}
    truth = truth_codes(fam.truth)
    kept, tp = host_masks(cols, truth)
    res = ld.masks(fam.genome, fam.genome, truth, cols[0], cols[1], cols[2], cols[4], kept, tp, subsets=True, detail=detail)
    return fam, cols, truth, res, detail


def test_the_conditions_of_the_draw():
    """what the GPU comparison rests on: every bit on at least 5 kept lines and 5 entries, the pairs N|H and A|H, every bit alone"""
    for seed in (7, 8):
        fam = LadderFamily(seed)
        for rng in (None, np.random.default_rng(seed)):
            got, _ = conditions(fam, fam.columns(rng))
            for c in ld.LETTERS:
                assert got["lines_" + c] >= 5 and got["entries_" + c] >= 5, (c, got)
                assert got["set_" + c] >= 1, (c, got)
            assert got["set_N+H"] >= 1 and got["set_A+H"] >= 1 and got["set_N+B"] >= 1 and got["set_none"] >= 5, got


def test_identities_on_the_draw(draw):
    fam, cols, truth, (rec, tru, mask, emask), d = draw
    forms_of = [nz.form_codes(fam.genome, *e)[1:] for e in nz.truth_order(*truth)]
    ld.identities(rec, tru, emask, norm=d["norm"][:2], atom=d["atom"][:2], hap=d["hap"][:2], sub=d["sub"][0], forms_of=forms_of)
    open_ = (mask & K) != 0
    assert not (mask[(mask & S) != 0] & 15).any()                  # N, A, H and B are never set with S
    assert not (((mask & H) != 0) & ((mask & B) != 0)).any()       # H and B never together
    assert not mask[~open_].any()                                  # a record that is not kept: byte 0
    np.testing.assert_array_equal(rec, ld.count_records(mask))
    np.testing.assert_array_equal(tru, ld.count_entries(emask))


def test_cumulative_table_against_the_tiers(draw):
    _, _, _, (rec, tru, mask, emask), _ = draw
    lines = [ld.tier(b) for b in mask if b & K and not b & S]
    ents = [ld.tier(b) for b in emask if not b & S]
    tp0, kept, n_ent = int(((mask & S) != 0).sum()), int(((mask & K) != 0).sum()), len(emask)
    want = []
    for k in range(5):
        tp_k = tp0 + sum(1 for t in lines if t is not None and t < k)
        found_k = int(((emask & S) != 0).sum()) + sum(1 for t in ents if t is not None and t < k)
        want.append((tp_k, kept - tp_k, n_ent - found_k))
    assert ld.cumulative(rec, tru) == want
    assert want[4][1] == int(rec[ld.CELL0]) and want[4][2] == int(tru[ld.CELL0])        # cell 0: the final FP and FN
    assert want[0][0] < want[1][0] < want[2][0] < want[3][0] < want[4][0]                # every tier adds something here


def test_tier_and_set_name():
    assert [ld.tier(b) for b in (0, N, A, H, B, N | H, A | H, A | B, K | S)] == [None, 0, 1, 2, 3, 0, 1, 1, None]
    assert [ld.set_name(m) for m in (0, 1, 6, 15)] == ["none", "N", "A+H", "N+A+H+B"]
    assert len(ld.TABLE_HEADER[1]) == 30 + 30 and ld.TABLE_HEADER[1][6:12] == ("TP_N", "FP_N", "FN_N", "Precision_N", "Recall_N", "F1_N")


# ---- the writers -------------------------------------------------------------------------------------------------------------------
def test_writers_on_literal_input(tmp_path):
    (rec, tru, mask, emask), _ = restated(True, True, True)
    rows = [("gatk", "TA-1-10", {"ladder_rec": rec, "ladder_tru": tru}), ("gatk", "TA-1-0", {}),
            ("gatk", "TA-1-50", {"ladder_rec": rec, "ladder_tru": tru})]
    path = tmp_path / "caller_performance_ladder.tsv"
    ld.write_performance_ladder(str(path), rows)
    text = path.read_text().split("\n")
    assert text[0].split("\t") == list(ld.TABLE_HEADER[0] + ld.TABLE_HEADER[1]) and text[-1] == "" and len(text) == 5
    one = text[1].split("\t")
    assert one[:2] == ["GATK", "TA-1-10"]
    # TP FP FN Precision Recall F1 by spelling, then after every tier: round(x, 3) as R prints it
    assert one[2:8] == ["1", "7", "9", "0.125", "0.1", "0.111"]
    assert one[8:14] == ["2", "6", "8", "0.25", "0.2", "0.222"]
    assert one[26:32] == ["5", "3", "0", "0.625", "1", "0.769"]
    sets = dict(zip(ld.TABLE_HEADER[1][30:], one[32:]))
    assert sets["lines_N+H"] == "1" and sets["lines_B"] == "1" and sets["entries_H"] == "4" and sets["entries_A+H"] == "2" and sets["lines_N"] == "0"
    assert text[2].split("\t")[:2] == ["GATK", "TA-1-50"] and text[2].split("\t")[2:] == one[2:]
    pooled = text[3].split("\t")
    assert pooled[:2] == ["GATK", "pooled"] and pooled[2:8] == ["2", "14", "18", "0.125", "0.1", "0.111"]
    # the per-sample file
    g, truth, recs = small()
    order = nz.truth_order(*truth_codes(truth))
    rows = ld.job_rows(mask, emask, [10 + i for i in range(len(recs))], [r[:3] for r in recs], [(p, nz.spell(r), nz.spell(a)) for p, r, a in order])
    out = tmp_path / "ladder" / "x.ladder.tsv"
    ld.write_job_ladder(str(out), rows)
    text = out.read_text().split("\n")
    assert text[0] == ld.LADDER_HEADER
    assert text[1:8] == ["line\t10\t23\tAA\tA\tN+H\tnormalized", "line\t11\t71\tAC\tGT\tA+H\tatomized", "line\t12\t121\tACG\tT\tH\thaplotype",
                         "line\t13\t171\tACG\tT\tB\tsubset", "line\t14\t176\tA\tC\tnone\tnone", "line\t15\t221\tACG\tT\tnone\tnone",
                         "line\t16\t271\tC\tA\tnone\tnone"]
    assert text[8] == "entry\t.\t20\tGA\tG\tN+H\tnormalized" and len(text) == 1 + 7 + 9 + 1
    assert ld.read_job_ladder(str(out)) == [(r[0], None if r[1] == "." else r[1]) + r[2:] for r in rows]


# ---- the flag ---------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_file(tmp_path):
    """the Pass row, check_alleles and the shared-call rule: without the allele-extended mode, beside any of the four passes the
    ladder runs itself or any other pass -- said before an engine is made or a file written"""
    import os
    from quasimodo_amd import passes, workflow
    from quasimodo_amd.extract import Job, extract_many
    names = [x.name for x in passes.PASSES]
    p = passes.PASSES[names.index("ladder")]
    assert p == passes.Pass("ladder", ("ladder",), ("ladder",), "--match-ladder", "ladder: the jobs of one call share one gap", ())
    assert names.index("ladder") == names.index("rescueroc") + 1 and names[-2:] == ["context", "surface"]
    assert p.needs_alleles == "a single-base batch has no rescue passes to combine"
    passes.check_alleles({"ladder"}, True)
    with pytest.raises(ValueError, match=r"^ladder \(--match-ladder\) needs the allele-extended mode"):
        passes.check_alleles({"ladder"}, False)
    for other in ("normalize", "atomize", "haplo", "hapsub", "rescueroc", "vartype", "motifs"):
        with pytest.raises(passes.SharedCallError) as ei:
            passes.check_shared_call({"ladder", other})
        assert "--match-ladder" in ei.value.for_cli()
    vcf, truth, fa = tmp_path / "TM-1-1.TM.c.vcf", tmp_path / "t.vcf", tmp_path / "g.fa"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t50\tPASS\t.\n")
    truth.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t.\t.\t.\n")
    fa.write_text(">c\nACATG\n")
    job = lambda: [Job(str(vcf), str(truth), "hcmv", "", "c")]
    before = sorted(os.listdir(str(tmp_path)))
    for kw, said in ((dict(ladder=[str(fa)]), "--alleles"), (dict(alleles=False, ladder={"genomes": [str(fa)]}), "--alleles"),
                     (dict(alleles=True, ladder=[str(fa)], normalize=[str(fa)]), "does not combine"),
                     (dict(alleles=True, ladder=[str(fa)], atomize=True), "does not combine"),
                     (dict(alleles=True, ladder=[str(fa)], haplo={"gap": 3, "genomes": [str(fa)]}), "does not combine"),
                     (dict(alleles=True, ladder=[str(fa)], rescue_roc=[str(fa)]), "does not combine"),
                     (dict(alleles=True, ladder={"genomes": [str(fa)], "gap": 33}), "gap"),
                     (dict(alleles=True, ladder=[str(fa), str(fa)]), "2 genomes entries for 1 jobs")):
        with pytest.raises(ValueError, match=said):
            extract_many(job(), **kw)
    j = job()
    j[0].ladder, j[0].ladder_genome, j[0].atomize = 10, str(fa), True     # asked for through the Job fields
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(j, alleles=True)
    j = job()
    j[0].ladder = 10                                                       # the gap without the genome
    with pytest.raises(ValueError, match="Job.ladder without Job.ladder_genome"):
        extract_many(j, alleles=True)
    assert sorted(os.listdir(str(tmp_path))) == before
    fas = {"TM": str(fa), "TA": str(fa)}
    for kw, said in ((dict(match_ladder=fas), "--match-ladder needs --alleles"),
                     (dict(alleles=True, match_ladder=fas, normalize=fas), "--match-ladder cannot be combined with --normalize"),
                     (dict(alleles=True, match_ladder=fas, haplotypes=fas), "--match-ladder cannot be combined with --haplotypes"),
                     (dict(alleles=True, match_ladder=fas, rescue_roc=fas), "--match-ladder cannot be combined with --rescue-roc"),
                     (dict(alleles=True, match_ladder=fas, atomize=True), "--atomize cannot be combined with --match-ladder"),
                     (dict(alleles=True, match_ladder=fas, hap_gap=33), "--hap-gap")):
        with pytest.raises(workflow.WorkflowError, match=said):
            workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), **kw)
    assert sorted(os.listdir(str(tmp_path))) == before
