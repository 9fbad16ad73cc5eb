"""Clusters of records matched by replayed haplotype, on the host: quasimodo_amd.haplo on hand-derived
literals, against an independent statement on whole genomes (plain slicing, no windows), tied to the normal form of 4.17, on the
planted family the GPU tests share; the pass table, the refusals, the exports, the constants, the table writer and the reader of the sites files."""
import os

import numpy as np
import pytest

from haplo_family import Family, codes, host_masks, truth_codes
from quasimodo_amd import haplo as hp
from quasimodo_amd.normalize import normalize as normal_form

#            1234567890123456789012345678901234567890
GENOME = "TTGACCTAGGCATCGATTACGGATCCATGCAAGTCTAGCT" * 3    # L = 120; G[11 .. 13] = CAT, G[61 .. 63] = GAT
R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}


def run(genome, truth, recs, gap=None, detail=None):
    """truth: [(p, REF, ALT)]; recs: [(p, REF, ALT)] -- all kept, ID '.'"""
    cols = codes([r + (True, hp.F_IDDOT) for r in recs])
    tr = truth_codes(truth)
    kept, tp = host_masks(cols, tr)
    return hp.counts(genome, tr, cols[0], cols[1], cols[2], cols[4], kept, tp, gap, detail)


def test_trim_and_footprint_literals():
    assert hp.trim(100, "ACG", "A") == (101, "CG", "")
    assert hp.trim(100, "ACG", "T") == (100, "ACG", "T")
    assert hp.trim(100, "A", "ACC") == (101, "", "CC")
    assert hp.trim(7, "GAT", "GCT") == (8, "A", "C")
    assert hp.trim(7, "AA", "A") == (8, "A", "")               # the prefix goes first
    assert hp.footprint(101, "CG") == (101, 102) and hp.footprint(101, "") == (101, 101)
    assert hp.unusable(GENOME, 11, "CAT", "C") is None
    assert hp.unusable(GENOME, 11, "CAT", None) == hp.LONG
    assert hp.unusable(GENOME, 11, "CAT", "C", nokey=True) == hp.NOKEY
    assert hp.unusable(GENOME, 11, "C", "C") == hp.NOVAR
    assert hp.unusable(GENOME, 0, "C", "A") == hp.RANGE and hp.unusable(GENOME, 119, "CTA", "C") == hp.RANGE
    assert hp.unusable(GENOME, 11, "GAT", "G") == hp.REFMISMATCH
    assert hp.unusable(GENOME.lower(), 11, "CAT", "C") == hp.REFMISMATCH     # (symbols() is what folds the case)
    assert hp.unusable(hp.symbols(GENOME.lower().encode()), 11, "CAT", "C") is None
    assert hp.symbols("acgtNRx-") == "ACGTNNNN"


def test_the_snv_beside_the_deletion_both_directions():
    # G[11 .. 13] = CAT.  Truth: SNV C>G at 11 beside the deletion CAT>C anchored at 11; the caller: CAT>G at 11.
    split, joined = [(11, "C", "G"), (11, "CAT", "C")], [(11, "CAT", "G")]
    detail = []
    rec, tru, cls, site, ecls = run(GENOME, split, joined, detail=detail)
    assert cls.tolist() == [hp.RESCUED] and site.tolist() == [0] and sorted(ecls.tolist()) == [hp.RESCUED] * 2
    assert [int(rec[R[c]]) for c in ("kept", "tp", "tp_h", "rescued", "open")] == [1, 0, 1, 1, 1] and int(rec[5:].sum()) == 0
    assert tru.tolist() == [2, 0, 2, 2, 0, 1, 1, 1]
    # window [1, 23]: the replay is G[1 .. 10] + G + G[14 .. 23]
    assert detail[0][1:4] == (1, 23, hp.MATCH) and detail[0][6] == detail[0][7] == GENOME[:10] + "G" + GENOME[13:23]
    rec, tru, cls, site, ecls = run(GENOME, joined, split)
    assert cls.tolist() == [hp.RESCUED] * 2 and ecls.tolist() == [hp.RESCUED]
    assert [int(rec[R[c]]) for c in ("kept", "tp", "tp_h", "rescued", "open")] == [2, 0, 2, 2, 2]
    assert tru.tolist() == [1, 0, 1, 1, 0, 1, 1, 1]
    # the SNV with its base changed
    rec, tru, cls, site, ecls = run(GENOME, split, [(11, "CAT", "A")])
    assert cls.tolist() == [hp.MISMATCH] and sorted(ecls.tolist()) == [hp.MISMATCH] * 2
    assert int(rec[R["mismatch"]]) == 1 and int(rec[R["tp_h"]]) == 0 and tru.tolist() == [2, 0, 0, 2, 0, 1, 1, 0]
    # a line without ID '.' is rescued, but no TP_H line
    cols = codes([(11, "CAT", "G", True, 0)])
    tr = truth_codes(split)
    rec, tru, cls, _, _ = hp.counts(GENOME, tr, cols[0], cols[1], cols[2], cols[4], *host_masks(cols, tr))
    assert cls.tolist() == [hp.RESCUED] and int(rec[R["tp_h"]]) == 0 and int(rec[R["rescued"]]) == 0 and int(tru[T["found_h"]]) == 2


def test_conflict_lone_outside_and_the_edges():
    # two insertions at one point
    rec, tru, cls, _, ecls = run(GENOME, [(11, "C", "CAC")], [(11, "C", "CA"), (11, "C", "CC")])
    assert cls.tolist() == [hp.CONFLICT] * 2 and ecls.tolist() == [hp.CONFLICT] and int(rec[R["conflict"]]) == 2 and int(tru[T["tried"]]) == 1
    # an insertion in front of a substitution of the same base is no conflict: C>CA at 11 (q = 12, r = '') beside A>G at 12
    rec, tru, cls, _, _ = run(GENOME, [(11, "CA", "CAG")], [(11, "C", "CA"), (12, "A", "G")])
    assert cls.tolist() == [hp.RESCUED] * 2
    # the site's entry is found: the line beside it is LONE; a line far away is OUTSIDE; one that ends behind the window too
    rec, tru, cls, site, ecls = run(GENOME, [(11, "C", "G")], [(11, "C", "G"), (14, "C", "T"), (60, "C", "A"), (19, "ACGG", "A")])
    assert cls.tolist() == [hp.MATCHED, hp.LONE, hp.OUTSIDE, hp.OUTSIDE] and site.tolist() == [0, 0, -1, -1] and ecls.tolist() == [hp.MATCHED]
    assert int(rec[R["lone"]]) == 1 and int(rec[R["outside"]]) == 2 and int(rec[R["open"]]) == 1 and tru.tolist() == [1, 1, 1, 0, 0, 1, 0, 0]
    # a site at p = 1: the window starts at 1.  TT>T at 1 against T>'' spelled at 2 (TG>G)
    detail = []
    rec, tru, cls, _, _ = run(GENOME, [(1, "TT", "T")], [(2, "TG", "G")], detail=detail)
    assert cls.tolist() == [hp.RESCUED] and detail[0][1:3] == (1, 12) and detail[0][6] == GENOME[:1] + GENOME[2:12]
    # an insertion at L + 1, spelled on the last base and on the last two
    L = len(GENOME)
    detail = []
    rec, tru, cls, site, _ = run(GENOME, [(L, "T", "TAC")], [(L - 1, "CT", "CTAC")], detail=detail)
    assert cls.tolist() == [hp.RESCUED] and detail[0][1:3] == (L + 1 - 10, L + 1) and detail[0][6] == GENOME[L - 10:] + "AC"
    # g = 0: the window is the footprint; neighbours one base apart are two sites
    assert hp.sites(hp.symbols(GENOME), [(11, "C", "G"), (12, "A", "G"), (14, "C", "G")], 0)[1] == [(0, 11, 11), (1, 12, 12), (2, 14, 14)]
    assert hp.sites(hp.symbols(GENOME), [(11, "C", "G"), (12, "A", "G"), (14, "C", "G")], 1)[1] == [(0, 10, 15)]
    detail = []
    rec, tru, cls, _, _ = run(GENOME, [(11, "CA", "GG")], [(11, "C", "G"), (12, "A", "G")], gap=0, detail=detail)
    assert cls.tolist() == [hp.RESCUED] * 2 and detail[0][1:3] == (11, 12) and detail[0][6] == "GG"
    rec, tru, cls, _, _ = run(GENOME, [(11, "CA", "GG")], [(11, "C", "G"), (13, "T", "G")], gap=0)
    assert cls.tolist() == [hp.MISMATCH, hp.OUTSIDE]
    for bad in (-1, 33, 1.5, True, "3"):
        with pytest.raises(ValueError, match="gap"):
            hp.check_gap(bad)
    assert hp.check_gap(None) == 10 and hp.check_gap(np.int32(32)) == 32


def test_toomany_and_toolong_literals():
    g = "ACGT" * 100
    snv = lambda p, k=1: (p, g[p - 1], "ACGT"[("ACGT".index(g[p - 1]) + k) % 4])
    truth = [snv(p) for p in range(41, 50)]                    # nine entries side by side
    rec, tru, cls, _, ecls = run(g, truth, [snv(41, 2)])
    assert cls.tolist() == [hp.TOOMANY] and ecls.tolist() == [hp.TOOMANY] * 9 and int(rec[R["toomany"]]) == 1
    rec, tru, cls, _, ecls = run(g, truth[:8], [snv(41, 2)])
    assert cls.tolist() == [hp.MISMATCH]
    rec, tru, cls, _, _ = run(g, [snv(41)], [snv(p, 2) for p in range(41, 50)])
    assert cls.tolist() == [hp.TOOMANY] * 9 and int(rec[R["toomany"]]) == 9
    chain = lambda last: [snv(p) for p in list(range(41, last, 20)) + [last]]
    assert hp.sites(g, chain(41 + 235), 10)[1] == [(0, 31, 286)]                      # 256 bases
    rec, tru, cls, _, _ = run(g, chain(41 + 235), [snv(45, 2)] + chain(41 + 235)[2:])      # (all but two entries are found)
    assert cls.tolist() == [hp.MISMATCH] + [hp.MATCHED] * 11
    rec, tru, cls, _, ecls = run(g, chain(41 + 236), [snv(45, 2)] + chain(41 + 236)[2:])
    assert cls.tolist() == [hp.TOOLONG] + [hp.MATCHED] * 11 and set(ecls.tolist()) == {hp.TOOLONG, hp.MATCHED}
    assert int(rec[R["toolong"]]) == 1 and int(rec[R["open"]]) == 1 and int(tru[T["tried"]]) == 0 and int(tru[T["sites"]]) == 1


FAMILY = Family(20)
FAMILY_COLS = FAMILY.columns()
FAMILY_TRUTH = truth_codes(FAMILY.truth)


@pytest.fixture(scope="module")
def family_result():
    detail = []
    kept, tp = host_masks(FAMILY_COLS, FAMILY_TRUTH)
    out = hp.counts(FAMILY.genome, FAMILY_TRUTH, FAMILY_COLS[0], FAMILY_COLS[1], FAMILY_COLS[2], FAMILY_COLS[4], kept, tp, None, detail)
    return out, detail, kept, tp


def test_the_family_plants_every_class(family_result):
    (rec, tru, cls, site, ecls), detail, kept, tp = family_result
    outcomes = [d[3] for d in detail]
    assert outcomes.count(hp.MATCH) >= 50 and outcomes.count(hp.MISMATCH) >= 50
    assert outcomes.count(hp.CONFLICT) >= 1 and outcomes.count(hp.TOOMANY) >= 2
    for c in ("toolong", "lone", "outside", "long", "nokey", "novar", "range", "refmismatch", "conflict", "toomany", "mismatch"):
        assert int(rec[R[c]]) >= 1, c
    assert any(len(d[4]) == 8 and d[3] == hp.MATCH for d in detail) and any(len(d[5]) == 8 and d[3] == hp.MATCH for d in detail)
    assert any(len(d[4]) == 9 for d in detail) and any(len(d[5]) == 9 for d in detail)
    assert any(d[2] - d[1] + 1 == 256 for d in detail)
    assert any(len(d[4]) > len(set((int(FAMILY_COLS[0][i]), int(FAMILY_COLS[1][i]), int(FAMILY_COLS[2][i])) for i in d[4])) for d in detail)
    # the ties of the tables among themselves
    assert int(rec[R["kept"]]) == int(kept.sum()) and int(rec[R["tp"]]) == int(tp.sum())
    assert int(rec[R["tp_h"]]) - int(rec[R["tp"]]) == int(rec[R["rescued"]]) > 0
    assert int(tru[T["found_h"]]) > int(tru[T["found"]]) and int(tru[T["matched"]]) == outcomes.count(hp.MATCH) and int(tru[T["tried"]]) == len(detail)
    assert int(rec[R["open"]]) == sum(int(rec[R[c]]) for c in ("lone", "mismatch", "conflict", "toomany", "toolong")) + int(((cls == hp.RESCUED) & kept).sum())
    assert int(kept.sum()) == int(((cls == hp.MATCHED) & kept).sum()) + int(rec[R["open"]]) + int(rec[R["outside"]]) + int(rec[R["long"]:].sum())
    assert (cls[~kept] != hp.RESCUED).all() and hp.NOTKEPT in cls[~kept]


def test_match_iff_the_whole_genomes_are_equal(family_result):
    """The independent statement: plain slicing on the whole genome, no windows.  Every decidable tried site: the anchors of two
    spellings may overlap where their trimmed forms do not, so each variant is applied as its trimmed form."""
    _, detail, _, _ = family_result
    G = hp.symbols(FAMILY.genome)
    ent = hp.truth_order(*FAMILY_TRUTH)
    checked = 0
    for s, ws, we, what, recs, ents, x, y in detail:
        if what not in (hp.MATCH, hp.MISMATCH):
            continue
        sides = []
        for side in ([(int(FAMILY_COLS[0][i]), hp.spell(FAMILY_COLS[1][i]), hp.spell(FAMILY_COLS[2][i])) for i in recs],
                     [(ent[j][0], hp.spell(ent[j][1]), hp.spell(ent[j][2])) for j in ents]):
            forms = [hp.trim(*v) for v in set(side)]
            sides.append(whole(G, forms))
        assert (sides[0] == sides[1]) == (what == hp.MATCH), (s, ws, we)
        checked += 1
    assert checked >= 100


def whole(G, forms):
    """the whole genome with trimmed forms (q, r, a) applied from the right; insertions at one point behind a replaced base
    keep the order (q, |r|) of the definition"""
    s = G
    for q, r, a in sorted(forms, key=lambda t: (t[0], len(t[1])), reverse=True):
        assert s[q - 1:q - 1 + len(r)] == r
        s = s[:q - 1] + a + s[q - 1 + len(r):]
    return s


def test_one_variant_per_side_is_a_match_iff_the_normal_forms_agree(family_result):
    _, detail, _, _ = family_result
    ent = hp.truth_order(*FAMILY_TRUTH)
    seen = set()
    for s, ws, we, what, recs, ents, x, y in detail:
        if len(recs) != 1 or len(ents) != 1 or what not in (hp.MATCH, hp.MISMATCH):
            continue
        i, j = recs[0], ents[0]
        a = normal_form(FAMILY.genome, int(FAMILY_COLS[0][i]), hp.spell(FAMILY_COLS[1][i]), hp.spell(FAMILY_COLS[2][i]))
        b = normal_form(FAMILY.genome, ent[j][0], hp.spell(ent[j][1]), hp.spell(ent[j][2]))
        assert (a[1:] == b[1:]) == (what == hp.MATCH)
        seen.add(what)
    assert seen == {hp.MATCH, hp.MISMATCH}
    # and on the literal genome: a deletion in the run CC at 5 .. 6, spelled on either base
    rec, tru, cls, _, _ = run(GENOME, [(4, "AC", "A")], [(5, "CC", "C")])
    assert cls.tolist() == [hp.RESCUED] and normal_form(GENOME, 5, "CC", "C")[1:] == normal_form(GENOME, 4, "AC", "A")[1:]


def test_sites_and_order_independence(family_result):
    (rec, tru, cls, site, ecls), _, kept, tp = family_result
    first, lo, hi = hp.truth_sites(FAMILY.genome, FAMILY_TRUTH)
    assert len(first) == int(tru[T["sites"]]) and (np.diff(first) > 0).all() and (np.diff(hi) >= 0).all() and (lo[1:] > hi[:-1]).all()
    rng = np.random.default_rng(3)
    cols = FAMILY.columns(rng)
    k2, t2 = host_masks(cols, FAMILY_TRUTH)
    r2, u2, c2, s2, e2 = hp.counts(FAMILY.genome, FAMILY_TRUTH, cols[0], cols[1], cols[2], cols[4], k2, t2)
    np.testing.assert_array_equal(r2, rec)
    np.testing.assert_array_equal(u2, tru)
    np.testing.assert_array_equal(e2, ecls)
    assert sorted(c2.tolist()) == sorted(cls.tolist())
    for g in (0, 32):                               # other gaps: other sites, the same ties
        r3, u3, _, _, _ = hp.counts(FAMILY.genome, FAMILY_TRUTH, FAMILY_COLS[0], FAMILY_COLS[1], FAMILY_COLS[2], FAMILY_COLS[4], kept, tp, g)
        assert int(r3[R["tp_h"]]) - int(r3[R["tp"]]) == int(r3[R["rescued"]]) and int(u3[T["found_h"]]) >= int(u3[T["found"]]) == int(tru[T["found"]])
    assert int(u3[T["sites"]]) < int(tru[T["sites"]])


def test_the_pass_table():
    from quasimodo_amd import passes
    p = [x for x in passes.PASSES if x.name == "haplo"]
    assert len(p) == 1 and p[0] == passes.Pass("haplo", ("haplo",), ("haplo",), "--haplotypes", "haplo: the jobs of one call share one gap", ())
    for other in (x.name for x in passes.PASSES):
        if other != "haplo":
            with pytest.raises(passes.SharedCallError):
                passes.check_shared_call({"haplo", other})
    passes.check_shared_call({"haplo"})
    passes.check_alleles({"haplo"}, True)
    with pytest.raises(ValueError, match=r"^normalize \("):                      # (the one rule names the pass that was asked for, not this one)
        passes.check_alleles({"normalize"}, False)
    with pytest.raises(ValueError, match="--alleles"):
        passes.check_alleles({"haplo"}, False)


def test_refusals_in_front_of_any_file(tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    from quasimodo_amd import passes, workflow
    from quasimodo_amd.extract import Job, extract_many
    fa = str(tmp_path / "a.fa")
    mk = lambda **kw: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i, haplo_genome=fa, **kw) for i in range(2)]
    assert passes.requested_by(mk(haplo=10)) == {"haplo"} and passes.requested_by(mk()) == set()
    with pytest.raises(ValueError, match="--alleles"):
        extract_many(mk(), haplo=10)
    with pytest.raises(ValueError, match="--alleles"):
        extract_many(mk(haplo=10), alleles=False)
    with pytest.raises(ValueError, match="gap"):
        extract_many(mk(), alleles=True, haplo=33)
    jobs = mk()
    jobs[0].haplo, jobs[1].haplo = 10, 5
    with pytest.raises(ValueError, match="share one gap"):
        extract_many(jobs, alleles=True)
    jobs = mk(haplo=10)
    jobs[1].haplo_genome = str(tmp_path / "b.fa")
    with pytest.raises(ValueError, match="the sites of a truth set belong to one genome"):
        extract_many(jobs, alleles=True)
    with pytest.raises(ValueError, match="genome"):
        extract_many([Job(str(tmp_path / "s.c.vcf"), str(tmp_path / "t.vcf"), "hcmv", "", "c")], alleles=True, haplo=10)
    for other in (dict(fn=True), dict(strata=[("all", [0], [100])]), dict(boot={}), dict(explain=3), dict(surface=True),
                  dict(context={"genomes": [fa, fa]}), dict(genomes=[fa, fa]), dict(normalize=[fa, fa]), dict(atomize=True), dict(vartype=True)):
        with pytest.raises(ValueError, match="does not combine"):
            extract_many(mk(), alleles=True, haplo=10, **other)
    with pytest.raises(workflow.WorkflowError, match="--haplotypes needs --alleles"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), haplotypes={"TM": fa, "TA": fa})
    with pytest.raises(workflow.WorkflowError, match="--hap-gap"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, haplotypes={"TM": fa, "TA": fa}, hap_gap=33)
    with pytest.raises(workflow.WorkflowError, match="--hap-gap needs --haplotypes"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, hap_gap=3)
    with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, haplotypes={"TM": fa, "TA": fa}, atomize=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", str(tmp_path / "a.vcf"), "--snps", str(tmp_path / "a.snps"),
                        "-l", "a", "-o", str(tmp_path / "v"), "--haplotypes"], capture_output=True, text=True)
    assert r.returncode != 0 and "allele-extended" in r.stderr + r.stdout and "--haplotypes" in r.stderr + r.stdout
    assert not any(x.is_file() for x in tmp_path.rglob("*")) and not (tmp_path / "v").exists()   # no file was written


def test_the_sites_file_reader(tmp_path):
    p = tmp_path / "x.sites.tsv"
    p.write_text(hp.SITES_HEADER + "\n3\t90\t112\t7:100:ACG:T;9:100:ACG:T\t100:A:T;100:ACG:A\tAAT\tAAT\n")
    assert hp.read_sites(str(p)) == [(3, 90, 112, [(7, "100", "ACG", "T"), (9, "100", "ACG", "T")], [(100, "A", "T"), (100, "ACG", "A")], "AAT", "AAT")]
    p.write_text("#other\n")
    with pytest.raises(ValueError, match="not a sites file"):
        hp.read_sites(str(p))


def test_exports_ids_and_constants():
    from conftest import ROOT
    from quasimodo_amd import _lib
    text = open(os.path.join(ROOT, "include", "qmvt.h")).read()
    for name in ("qm_batch_haplotypes", "qm_batch_get_haplotypes", "qm_batch_get_haplotyped", "qm_batch_haplotype_timings", "qm_truth_sites",
                 "qm_extract_files_haplotypes"):
        assert name in _lib.EXPORTS and name + "(" in text
        assert hasattr(_lib.lib(), name)
    assert _lib.QM_ABI_VERSION == 6 and _lib.source_kernels_id() == "db744d8883a55744"
    assert "qmvt_haplo.hip" in _lib._ASRC and "qmvt_haplo.h" in _lib._ASRC and "qmvt_haplo.hip" not in _lib._KSRC
    mk = open(os.path.join(ROOT, "quasimodo_amd", "csrc", "Makefile")).read()
    ksrc = next(ln for ln in mk.split("\n") if ln.startswith("KSRC ="))
    assert "qmvt_haplo" not in ksrc and "qmvt_haplo.o" in mk
    for name, value in (("R_COLS", len(hp.R_COLS)), ("T_COLS", len(hp.T_COLS)), ("MAX_GAP", hp.MAX_GAP), ("DEFAULT_GAP", hp.DEFAULT_GAP),
                        ("MAX_WINDOW", hp.MAX_WINDOW), ("MAX_ITEMS", hp.MAX_ITEMS)):
        assert getattr(_lib, "QM_HAP_" + name) == value and "#define QM_HAP_%s %d" % (name, value) in text
    assert len(hp.R_COLS) == 16 and len(hp.T_COLS) == 8 and len(hp.CLASS_NAMES) == 14
    for k, name in enumerate(hp.R_COLS):
        assert "QM_HAP_R_%s = %d" % (name.upper(), k) in text
    for k, name in enumerate(hp.CLASS_NAMES):
        assert "QM_HAP_C_%s = %d" % (name.upper(), k) in text


def test_the_table_writer_on_fixed_rows(tmp_path):
    rec = [10, 4, 7, 3, 5, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    tru = [8, 4, 7, 4, 0, 3, 3, 2]
    assert hp.performance_row(rec, tru) == [4, 6, 4, 0.4, 0.5, 0.444, 7, 3, 1, 0.7, 0.875, 0.778] + rec[3:] + [8, 4, 0, 3, 3, 2]
    assert hp.performance_row([0] * 16, tru)[:12] == [0, 0, 4, None, None, None, 0, 0, 1, None, None, None]
    path = str(tmp_path / "caller_performance_haplotype.tsv")
    hp.write_performance_haplotype(path, [("lofreq", "TA", {"hap_rec": rec, "hap_tru": tru}), ("bcftools", "TA", {}),
                                          ("clc", "TM", {"hap_rec": [0] * 16, "hap_tru": tru})])
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 4
    head = lines[0].split("\t")
    assert head[:8] == ["caller", "mixture", "TP", "FP", "FN", "Precision", "Recall", "F1"] and head[8:14] == ["TP_H", "FP_H", "FN_H", "Precision_H", "Recall_H", "F1_H"]
    assert head[14:] == list(hp.R_COLS[3:]) + ["truth_entries", "truth_open", "truth_unusable", "sites", "sites_tried", "sites_matched"]
    row = lines[1].split("\t")
    assert row[1:14] == ["TA", "4", "6", "4", "0.4", "0.5", "0.444", "7", "3", "1", "0.7", "0.875", "0.778"] and len(row) == len(head)
    assert lines[2].split("\t")[2:8] == ["0", "0", "4", "NA", "NA", "NA"]
    assert not [f for f in os.listdir(str(tmp_path)) if ".tmp." in f]
