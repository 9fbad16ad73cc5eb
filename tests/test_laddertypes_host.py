"""The restatement of the match ladder per variant type and size (quasimodo_amd.laddertypes) on the host: hand-written
literals over the ladder's 400-base genome, every identity that ties its blocks to the ladder and to the type pass on the planted
draw, the cumulative per-row table against a direct count over per-line tiers, the writers on literal input, the Pass row and the
refusals that come before any file or device is touched -- and the conditions of the draw the GPU tests compare the device on."""
import os

import numpy as np
import pytest

from haplo_family import codes, host_masks, truth_codes
from ladder_family import LadderFamily, conditions
from quasimodo_amd import ladder as ld
from quasimodo_amd import laddertypes as lt
from quasimodo_amd import normalize as nz
from quasimodo_amd import vartype as vt
from test_ladder_host import restated, small

K, S, N, A, H, B = ld.M_K, ld.M_S, ld.M_N, ld.M_A, ld.M_H, ld.M_B
EDGES = vt.DEFAULT_EDGES
NAMES = vt.row_names(EDGES)
NR = vt.n_rows(EDGES)
# the method sets the ladder reaches on the planted family: H and B are never set together (include/qmvt.h), and no planted case
# is rescued by normal form AND by atoms -- 8 of the 16 cells, every method bit among them alone and in a pair
REACHED = (0, N, A, H, B, N | H, A | H, N | B)


def block(cells):
    """{(row name, column): count} -> [NR][18], KEPT / ENTRIES formed as the sum"""
    out = np.zeros((NR, 18), np.uint64)
    for (name, col), c in cells.items():
        out[NAMES.index(name), col] = c
    out[:, ld.KEPT] = out[:, ld.TP:].sum(axis=1)
    return out


def literal(subsets=True):
    (rec, tru, mask, emask), _ = restated(True, True, subsets)
    g, truth, recs = small()
    cols, tc = codes(recs), truth_codes(truth)
    kept, tp = host_masks(cols, tc)
    trec, ttru, rows = vt.counts(tc, cols[0], cols[1], cols[2], cols[4], kept, tp, EDGES)
    return (rec, tru, mask, emask), (trec, ttru, rows), lt.entry_rows(tc, EDGES)


# ---- literals ---------------------------------------------------------------------------------------------------------------------
def test_literals_on_the_small_genome():
    """a deletion respelled in a repeat lands in the DEL row of its spelling with N|H; AC>GT beside two truth SNVs: the line in
    MNP:2, both entries in SNV:1, A|H; ACG>T against SNV plus deletion: the line in CPX:3, the entries in SNV:1 and DEL:2; the
    partial site by subset; a plain FP; a record that is not kept; a TP by spelling"""
    (lrec, ltru, mask, emask), (trec, ttru, rows), erows = literal()
    assert [NAMES[r] for r in rows] == ["DEL:1", "MNP:2", "CPX:3", "CPX:3", "SNV:1", "CPX:3", "SNV:1", "SNV:1", "SNV:1"]
    assert mask.tolist() == [K | N | H, K | A | H, K | H, K | B, K, K, K, 0, K | S]
    rec, tru = lt.counts(mask, emask, rows, erows, NR)
    c0 = ld.CELL0
    np.testing.assert_array_equal(rec, block({("DEL:1", c0 + (N | H)): 1, ("MNP:2", c0 + (A | H)): 1, ("CPX:3", c0 + H): 1, ("CPX:3", c0 + B): 1,
                                              ("CPX:3", c0): 1, ("SNV:1", c0): 2, ("SNV:1", ld.TP): 1}))
    np.testing.assert_array_equal(tru, block({("DEL:1", c0 + (N | H)): 1, ("SNV:1", c0 + (A | H)): 2, ("SNV:1", c0 + H): 2, ("DEL:2", c0 + H): 2,
                                              ("SNV:1", c0 + B): 1, ("DEL:2", c0 + B): 1, ("SNV:1", ld.TP): 1}))
    assert int(rec[NAMES.index("SNV:1"), ld.KEPT]) == 3 and int(tru[NAMES.index("SNV:1"), ld.KEPT]) == 6   # the record that is not kept: nowhere
    lt.identities(rec, tru, ladder=(lrec, ltru), types=(trec, ttru), edges=EDGES)
    # per row: by spelling, then after normal form, atoms, haplotype, subset
    assert ld.cumulative(rec[NAMES.index("DEL:1")], tru[NAMES.index("DEL:1")]) == [(0, 1, 1), (1, 0, 0), (1, 0, 0), (1, 0, 0), (1, 0, 0)]
    assert ld.cumulative(rec[NAMES.index("CPX:3")], tru[NAMES.index("CPX:3")]) == [(0, 3, 0), (0, 3, 0), (0, 3, 0), (1, 2, 0), (2, 1, 0)]
    assert ld.cumulative(rec[NAMES.index("SNV:1")], tru[NAMES.index("SNV:1")]) == [(1, 2, 5), (1, 2, 5), (1, 2, 3), (1, 2, 1), (1, 2, 0)]


def test_literals_without_the_subset_search():
    (lrec, ltru, mask, emask), (trec, ttru, rows), erows = literal(subsets=False)
    rec, tru = lt.counts(mask, emask, rows, erows, NR)
    assert int(rec[NAMES.index("CPX:3"), ld.CELL0]) == 2 and not rec[:, ld.CELL0 + B].any() and not tru[:, ld.CELL0 + B].any()
    lt.identities(rec, tru, ladder=(lrec, ltru), types=(trec, ttru), edges=EDGES)


def test_a_long_allele_through_a_shape_row():
    """a deletion of 19 bases whose REF is a dictionary id: with its shape row it counts in DEL:16-50, without one in NOSHAPE;
    two long alleles in LONGPAIR, equal codes in NOVAR, a record without a key in NOKEY -- plain counts under their bytes"""
    long_ = "ACGTTGCAACGTTGCAACGT"
    shapes = vt.shapes_of([long_])
    ref = np.array([nz.DICT | 0, nz.DICT | 0, nz.code("AC"), nz.code("A"), nz.DICT | 0], np.int64)
    alt = np.array([nz.code("A"), nz.DICT | 0 | 1 << 20, nz.code("AC"), nz.code("C"), nz.code("A")], np.int64)
    nokey = [False, False, False, True, False]
    mask = np.array([K | N, K, K, K, 0], np.uint8)
    for sh, first in ((shapes, "DEL:16-50"), (None, "NOSHAPE")):
        rows = [vt.row_codes(r, a, EDGES, sh, nk) for r, a, nk in zip(ref, alt, nokey)]
        assert [NAMES[r] for r in rows] == [first, "LONGPAIR", "NOVAR", "NOKEY", first]
        erows = [vt.row_codes(nz.DICT | 0, nz.code("A"), EDGES, sh)]
        rec, tru = lt.counts(mask, np.array([N], np.uint8), rows, erows, NR)
        np.testing.assert_array_equal(rec, block({(first, ld.CELL0 + N): 1, ("LONGPAIR", ld.CELL0): 1, ("NOVAR", ld.CELL0): 1, ("NOKEY", ld.CELL0): 1}))
        np.testing.assert_array_equal(tru, block({(first, ld.CELL0 + N): 1}))
        lt.identities(rec, tru, edges=EDGES)


def test_counts_refuses_what_does_not_fit():
    with pytest.raises(ValueError, match="2 mask bytes for 1 rows"):
        lt.counts([K, K], [], [0], [], NR)
    with pytest.raises(ValueError, match="row 44 of 44"):
        lt.counts([K], [], [NR], [], NR)
    rec, tru = lt.counts([], [], [], [], 9)
    assert rec.shape == tru.shape == (9, 18) and not rec.any() and not tru.any()


# ---- the planted draw of the GPU tests ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def draw():
    fam = LadderFamily(7)
    cols = fam.columns()
    truth = truth_codes(fam.truth)
    kept, tp = host_masks(cols, truth)
    got, (lrec, ltru, mask, emask) = conditions(fam, cols, masks=(kept, tp))
    trec, ttru, rows = vt.counts(truth, cols[0], cols[1], cols[2], cols[4], kept, tp, EDGES)
    erows = lt.entry_rows(truth, EDGES)
    return (lrec, ltru, mask, emask), (trec, ttru, rows), erows, lt.counts(mask, emask, rows, erows, NR)


def test_the_conditions_of_the_draw(draw):
    """what the GPU comparison on the family rests on: every cell the ladder reaches there is non-empty in at least one row, on
    the records' side; several rows hold open lines; a long allele has no row without a shape table"""
    _, _, _, (rec, tru) = draw
    for m in REACHED:
        assert rec[:, ld.CELL0 + m].any(), ld.set_name(m)
    for m in range(16):
        if m not in REACHED:
            assert not rec[:, ld.CELL0 + m].any() and (not tru[:, ld.CELL0 + m].any() or m == (A | B)), ld.set_name(m)
    assert sum(1 for r in rec if int(r[ld.KEPT]) > int(r[ld.TP])) >= 5
    assert int(rec[NAMES.index("NOSHAPE"), ld.KEPT]) >= 1 and int(tru[NAMES.index("NOSHAPE"), ld.KEPT]) >= 1
    assert int(rec[NAMES.index("NOKEY"), ld.KEPT]) >= 1


def test_identities_on_the_draw(draw):
    (lrec, ltru, mask, emask), (trec, ttru, rows), erows, (rec, tru) = draw
    lt.identities(rec, tru, ladder=(lrec, ltru), types=(trec, ttru), edges=EDGES)
    np.testing.assert_array_equal(rec.sum(axis=0), ld.count_records(mask))
    np.testing.assert_array_equal(tru.sum(axis=0), ld.count_entries(emask))
    with pytest.raises(AssertionError, match="sum to the ladder's rec"):
        lt.identities(rec, tru, ladder=(lrec + np.uint64(1), ltru))
    bad = tru.copy()
    bad[NAMES.index("NOKEY"), [ld.KEPT, ld.CELL0]] = 1
    with pytest.raises(AssertionError, match="never land in NOKEY"):
        lt.identities(rec, bad)


def test_cumulative_rows_against_the_tiers(draw):
    """ladder.cumulative on every row against a direct count over the tiers of the row's lines and entries"""
    (_, _, mask, emask), (_, _, rows), erows, (rec, tru) = draw
    busy = 0
    for row in range(NR):
        mine, theirs = mask[np.asarray(rows) == row], emask[np.asarray(erows) == row]
        lines = [ld.tier(b) for b in mine if b & K and not b & S]
        ents = [ld.tier(b) for b in theirs if not b & S]
        tp0, kept, found0 = int(((mine & S) != 0).sum()), int(((mine & K) != 0).sum()), int(((theirs & S) != 0).sum())
        want = []
        for k in range(5):
            tp_k = tp0 + sum(1 for t in lines if t is not None and t < k)
            want.append((tp_k, kept - tp_k, len(theirs) - found0 - sum(1 for t in ents if t is not None and t < k)))
        assert ld.cumulative(rec[row], tru[row]) == want, NAMES[row]
        busy += want[0] != want[4]
    assert busy >= 4                                                     # the tiers move something in several rows


# ---- the writers -------------------------------------------------------------------------------------------------------------------
def test_table_rows_and_the_writer_on_literal_input(tmp_path):
    (_, _, mask, emask), (_, _, rows), erows = literal()
    rec, tru = lt.counts(mask, emask, rows, erows, NR)
    table = lt.table_rows(rec, tru, EDGES)
    nb = len(EDGES)
    assert len(table) == 5 * (nb + 1) + 4 and all(len(r) == 2 + 30 for r in table)
    assert len(lt.TABLE_HEADER) == 4 + 30 and lt.TABLE_HEADER[4:10] == ("TP", "FP", "FN", "Precision", "Recall", "F1")
    assert lt.TABLE_HEADER[10:16] == ("TP_N", "FP_N", "FN_N", "Precision_N", "Recall_N", "F1_N") and lt.TABLE_HEADER[-1] == "F1_B"
    by = {(r[0], r[1]): r[2:] for r in table}
    # SNV:1 -- 3 kept lines, 1 TP; 6 entries, 1 found, 2 more by atoms, 2 by haplotype, 1 by subset
    assert by[("SNV", "1")][:6] == [1, 2, 5, 0.333, 0.167, 0.222]
    assert by[("SNV", "1")][24:] == [1, 2, 0, 0.333, 1.0, 0.5]
    assert by[("SNV", "all")] == by[("SNV", "1")]
    # DEL:1 -- the respelled deletion: FP and FN by spelling, TP and found from the first tier on
    d1 = by[("DEL", "1")]
    assert d1[:5] == [0, 1, 1, 0.0, 0.0] and np.isnan(d1[5]) and d1[6:12] == [1, 0, 0, 1.0, 1.0, 1.0]   # (0 / 0 as R has it: NaN)
    # DEL:2 -- nothing kept in the row: NA, the entries still counted down
    assert by[("DEL", "2")][:6] == [0, 0, 3, None, None, None] and by[("DEL", "2")][18:21] == [0, 0, 1] and by[("DEL", "2")][24:27] == [0, 0, 0]
    assert by[("DEL", "all")][:3] == [0, 1, 4] and by[("DEL", "all")][6:9] == [1, 0, 3]
    assert by[("INS", "all")] == [0, 0, 0, None, None, None] * 5
    assert by[("NOKEY", "NA")] == [0, 0, 0, None, None, None] * 5          # behind the grid: plain counts
    rows_in = [("gatk", "TA-1-10", {"ladder_types_rec": rec, "ladder_types_tru": tru}), ("gatk", "TA-1-0", {}),
               ("gatk", "TA-1-50", {"ladder_types_rec": rec, "ladder_types_tru": tru})]
    path = tmp_path / "caller_performance_ladder_types.tsv"
    lt.write_performance_ladder_types(str(path), rows_in, EDGES)
    text = path.read_text().split("\n")
    per = len(table)
    assert text[0].split("\t") == list(lt.TABLE_HEADER) and text[-1] == "" and len(text) == 1 + 3 * per + 1
    one = text[1].split("\t")
    assert one[:4] == ["GATK", "TA-1-10", "SNV", "1"] and one[4:10] == ["1", "2", "5", "0.333", "0.167", "0.222"]
    assert text[1 + per].split("\t")[:4] == ["GATK", "TA-1-50", "SNV", "1"]
    pooled = text[1 + 2 * per].split("\t")
    assert pooled[:4] == ["GATK", "pooled", "SNV", "1"] and pooled[4:10] == ["2", "4", "10", "0.333", "0.167", "0.222"]
    dele = [ln.split("\t") for ln in text if ln.startswith("GATK\tTA-1-10\tDEL\t1\t")][0]
    assert dele[4:10] == ["0", "1", "1", "0", "0", "NaN"] and dele[10:16] == ["1", "0", "0", "1", "1", "1"]
    with pytest.raises(ValueError, match="count blocks of shape"):
        lt.write_performance_ladder_types(str(path), rows_in, (1, 2))
    assert sorted(os.listdir(str(tmp_path))) == ["caller_performance_ladder_types.tsv"]


# ---- the flag ---------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_file(tmp_path):
    """the Pass row and its place, check_alleles, the shared-call rule against every other pass, and what extract_many and the
    workflow refuse before an engine is made or a file written"""
    from quasimodo_amd import passes, workflow
    from quasimodo_amd.extract import Job, extract_many
    names = [x.name for x in passes.PASSES]
    p = passes.PASSES[names.index("laddertypes")]
    assert p == passes.Pass("laddertypes", ("ladder_types",), ("ladder_types",), "--ladder-by-type",
                            "ladder_types: the jobs of one call share one gap and one list of size edges", ())
    assert names.index("laddertypes") == names.index("ladder") + 1 and names[-2:] == ["context", "surface"]
    assert p.needs_alleles == "a single-base batch has neither types nor rescue passes to cross"
    passes.check_alleles({"laddertypes"}, True)
    with pytest.raises(ValueError, match=r"^laddertypes \(--ladder-by-type\) needs the allele-extended mode"):
        passes.check_alleles({"laddertypes"}, False)
    for other in names:
        if other != "laddertypes":
            with pytest.raises(passes.SharedCallError) as ei:
                passes.check_shared_call({"laddertypes", other})
            assert "--ladder-by-type" in ei.value.for_cli()
    vcf, truth, fa = tmp_path / "TM-1-1.TM.c.vcf", tmp_path / "t.vcf", tmp_path / "g.fa"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t50\tPASS\t.\n")
    truth.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t.\t.\t.\n")
    fa.write_text(">c\nACATG\n")
    job = lambda: [Job(str(vcf), str(truth), "hcmv", "", "c")]
    before = sorted(os.listdir(str(tmp_path)))
    f = str(fa)
    for kw, said in ((dict(ladder_types=[f]), "--alleles"), (dict(alleles=False, ladder_types={"genomes": [f]}), "--alleles"),
                     (dict(alleles=True, ladder_types=[f], ladder=[f]), "does not combine"),
                     (dict(alleles=True, ladder_types=[f], vartype=True), "does not combine"),
                     (dict(alleles=True, ladder_types=[f], normalize=[f]), "does not combine"),
                     (dict(alleles=True, ladder_types=[f], atomize=True), "does not combine"),
                     (dict(alleles=True, ladder_types=[f], haplo={"gap": 3, "genomes": [f]}), "does not combine"),
                     (dict(alleles=True, ladder_types=[f], rescue_roc=[f]), "does not combine"),
                     (dict(alleles=True, ladder_types={"genomes": [f], "gap": 33}), "gap"),
                     (dict(alleles=True, ladder_types={"genomes": [f], "edges": (1, 1)}), "size edges ascend"),
                     (dict(alleles=True, ladder_types=[f, f]), "2 genomes entries for 1 jobs")):
        with pytest.raises(ValueError, match=said):
            extract_many(job(), **kw)
    j = job()
    j[0].ladder_types, j[0].ladder_types_genome, j[0].vartype = (10, EDGES), f, EDGES   # asked for through the Job fields
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(j, alleles=True)
    j = job()
    j[0].ladder_types = (10, EDGES)                                        # the parameters without the genome
    with pytest.raises(ValueError, match="Job.ladder_types without Job.ladder_types_genome"):
        extract_many(j, alleles=True)
    j = job() + job()
    j[0].ladder_types, j[0].ladder_types_genome = (10, EDGES), f
    j[1].ladder_types, j[1].ladder_types_genome = (10, (1, 2)), f
    with pytest.raises(ValueError, match="share one gap and one list of size edges"):
        extract_many(j, alleles=True)
    assert sorted(os.listdir(str(tmp_path))) == before
    fas = {"TM": f, "TA": f}
    for kw, said in ((dict(ladder_by_type=fas), "--ladder-by-type needs --alleles"),
                     (dict(alleles=True, ladder_by_type=fas, match_ladder=fas), "--ladder-by-type cannot be combined with --match-ladder"),
                     (dict(alleles=True, ladder_by_type=fas, by_type=True), "--by-type cannot be combined with --ladder-by-type"),
                     (dict(alleles=True, ladder_by_type=fas, normalize=fas), "--ladder-by-type cannot be combined with --normalize"),
                     (dict(alleles=True, ladder_by_type=fas, haplotypes=fas), "--ladder-by-type cannot be combined with --haplotypes"),
                     (dict(alleles=True, ladder_by_type=fas, rescue_roc=fas), "--ladder-by-type cannot be combined with --rescue-roc"),
                     (dict(alleles=True, ladder_by_type=fas, atomize=True), "--atomize cannot be combined with --ladder-by-type"),
                     (dict(alleles=True, ladder_by_type=fas, truth_side=True), "--ladder-by-type cannot be combined with --truth-side"),
                     (dict(alleles=True, ladder_by_type=fas, hap_gap=33), "--hap-gap"),
                     (dict(alleles=True, ladder_by_type=fas, ladder_type_bins="1,1"), "--type-bins"),
                     (dict(alleles=True, ladder_type_bins="1,2"), "ladder_type_bins needs ladder_by_type")):
        with pytest.raises(workflow.WorkflowError, match=said):
            workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), **kw)
    assert sorted(os.listdir(str(tmp_path))) == before
