"""The restatement of the subset search (quasimodo_amd.haplo: forms, search, subset_counts) judged on the host:
the literals of the planted blocks, derived by hand; an independent double loop over all pairs of subsets that substitutes each
side into the WHOLE genome by plain slicing; the two tests of admissibility against each other; a MATCH site handed to `search`;
the table writer.  CPU only.  (The device is held to this restatement by tests/test_gpu_haplo_subsets.py.)"""
import functools

import numpy as np
import pytest

import haplo_subsets as hs
from haplo_subset_edges import all_pairs_ok, brute, plain_forms, whole   # noqa: F401  (the independent judge: it moved to the edge families)
from quasimodo_amd import haplo as hp


@functools.lru_cache(maxsize=None)
def fam():
    return hs.family()


@functools.lru_cache(maxsize=None)
def restated():
    e = fam()
    return {(v, gap): hs.restate(e, v, gap) for v, vc in enumerate(e.vcfs) if vc[3] for gap in e.gaps}


def test_what_the_family_plants_arrives():
    hs.present(fam(), restated())


def test_the_literals_of_the_first_blocks():
    """(a) to (g) as masks and as line sets, each derived by hand from the planted spellings"""
    e = fam()
    v = e.index("main")
    res, (sub, cls_s, ecls_s, chosen) = restated()[(v, 10)]
    c = e.cols[v]
    spelled = lambda idx: sorted((int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in idx)
    by_block = {}
    for name in "abcdefg":
        at = e.planted[name]["at"]
        (s,) = [d[0] for d in res[5] if d[1] <= at <= d[2]]
        by_block[name] = [d for d in chosen if d[0] == s]
    g = e.genome
    assert [(d[1], d[2]) for d in by_block["a"]] == [(1, 3)]
    assert spelled(by_block["a"][0][3]) == [(120, "ACG", "T")] and [x[0] for x in spelled(by_block["a"][0][4])] == [125]
    assert by_block["a"][0][7] == g[109:119] + "T" + g[122:132]                                              # the window is 110 .. 132
    assert [(d[1], d[2]) for d in by_block["b"]] == [(1, 3)]
    assert by_block["b"][0][4] == [] and len(by_block["b"][0][5]) == 2 and len(by_block["b"][0][6]) == 1      # one entry is left
    assert [(d[1], d[2]) for d in by_block["c"]] == [(1, 1)]
    assert spelled(by_block["c"][0][3]) == [(319, g[318] + "ACG", g[318] + "A")] and spelled(by_block["c"][0][4]) == [(322, "G", "T")]
    assert [(d[1], d[2]) for d in by_block["d"]] == [(1, 1)]                                                 # the tie: S mask 1, not 2
    assert spelled(by_block["d"][0][3]) == [(421, "A", "AA")] and spelled(by_block["d"][0][4]) == [(422, "A", "AA")]
    assert [(d[1], d[2]) for d in by_block["e"]] == [(1, 1)]
    assert spelled(by_block["e"][0][3]) == [(519, g[518] + "ACG", g[518] + "A"), (520, "ACGT", "AT")] and by_block["e"][0][4] == []
    assert by_block["f"] == [] and by_block["g"] == []
    # the counts of the whole VCF follow from the planted blocks: 16 searched sites, 3 of them without a subset
    assert [int(x) for x in sub[:3]] == [16, 13, 3]
    assert int(sub[4]) + int(sub[6]) == sum(len(d[3]) + len(d[4]) for d in chosen)
    assert int(sub[3]) - int(res[0][2]) == int(sub[4])              # every planted line is kept with ID '.', none is a TP line
    assert int(sub[5]) - int(res[1][2]) + int(sub[7]) == sum(len(d[5]) + len(d[6]) for d in chosen)


def test_an_independent_double_loop_confirms_every_optimum_and_every_nosubset():
    e = fam()
    G = hp.symbols(e.genome)
    searched = partial = 0
    for (v, gap), (res, (sub, cls_s, ecls_s, chosen)) in restated().items():
        c = e.cols[v]
        ent_s = [(p, hp.spell(r), hp.spell(a)) for p, r, a in e.order[e.vcfs[v][1]]]
        masks = {d[0]: (d[1], d[2]) for d in chosen}
        n = 0
        for s, ws, we, what, recs, ents, _, _ in res[5]:
            if what not in (hp.MISMATCH, hp.CONFLICT):
                assert s not in masks
                continue
            n += 1
            got = brute(G, tuple((int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in recs), tuple(ent_s[j] for j in ents))
            assert got == masks.get(s), "VCF %d, gap %d, site %d" % (v, gap, s)
            partial += got is not None
        assert n == int(sub[0]) == int(sub[1]) + int(sub[2])
        assert n == int(res[1][6]) - int(res[1][7]) - sum(d[3] == hp.TOOMANY for d in res[5])      # tried, not MATCH, not TOOMANY
        searched += n
    assert searched >= 33 and partial >= 27


def test_the_neighbour_test_and_the_all_pairs_test_of_conflicts_agree():
    e = fam()
    sides = set()
    for (v, gap), (res, _) in restated().items():
        c = e.cols[v]
        ent_s = [(p, hp.spell(r), hp.spell(a)) for p, r, a in e.order[e.vcfs[v][1]]]
        for s, ws, we, what, recs, ents, _, _ in res[5]:
            if what != hp.TOOMANY:
                sides.add(tuple(hp.forms([(int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in recs])))
                sides.add(tuple(hp.forms([ent_s[j] for j in ents])))
    n = bad = 0
    for fs in sides:
        for m in range(1, 1 << len(fs)):
            pick = hp.subset(list(fs), m)
            assert hp.admissible(list(fs), m) == all_pairs_ok(pick)
            n += 1
            bad += not all_pairs_ok(pick)
    assert n > 1500 and bad >= 64


def test_the_order_of_forms_is_total_and_free_of_the_record_order():
    side = [(10, "A", "AC"), (10, "A", "AG"), (9, "TA", "TAC"), (10, "AC", "A"), (10, "A", "T"), (10, "A", "ACC"), (12, "G", "T")]
    want = [(10, "A", "T"), (11, "", "C"), (11, "", "G"), (11, "", "CC"), (11, "C", ""), (12, "G", "T")]
    assert want == sorted(want, key=hp.form_key)
    rng = np.random.default_rng(3)
    for _ in range(20):
        rng.shuffle(side)
        assert hp.forms(side) == want


def test_a_match_site_handed_to_search_gives_the_full_masks():
    e = fam()
    v = e.index("main")
    G = hp.symbols(e.genome)
    c = e.cols[v]
    # block (a) without the unrelated SNV: the haplotype pass calls it MATCH, the search takes everything
    recs, ents = [(120, "ACG", "T")], [(120, "A", "T"), (120, "ACG", "A")]
    assert hp.decide(G, 110, 132, recs, ents)[0] == hp.MATCH
    ms, mt, fa, fb, x = hp.search(G, 110, 132, recs, ents)
    assert (ms, mt) == (1, 3) and x == hp.decide(G, 110, 132, recs, ents)[1]
    # ... and every MATCH site of the family's restatement
    res = restated()[(v, 10)][0]
    ent_s = [(p, hp.spell(r), hp.spell(a)) for p, r, a in e.order[0]]
    for s, ws, we, what, ri, ei, x, y in res[5]:
        if what == hp.MATCH:
            got = hp.search(G, ws, we, [(int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in ri], [ent_s[j] for j in ei])
            assert got[0] == (1 << len(got[2])) - 1 and got[1] == (1 << len(got[3])) - 1 and got[4] == x == y
    with pytest.raises(ValueError, match="at most 8"):
        hp.search(G, 1, 50, [(k, G[k - 1], "ACGT"["ACGT".index(G[k - 1]) ^ 1]) for k in range(10, 19)], ents)


def test_the_table_rows_against_hand_derived_ones(tmp_path):
    rec = [10, 4, 6, 2, 5] + [0] * 11                # kept 10, TP 4, TP_H 6
    tru = [8, 3, 5, 5, 0, 4, 3, 1]                   # entries 8, found 3, FOUND_H 5
    sub = [2, 1, 1, 7, 2, 6, 1, 1]                   # TP_S 7, FOUND_S 6
    row = hp.performance_row_subsets(rec, tru, sub)
    assert row[:6] == [4, 6, 5, 0.4, 0.375, 0.387]
    assert row[6:12] == [6, 4, 3, 0.6, 0.625, 0.612]
    assert row[12:18] == [7, 3, 2, 0.7, 0.75, 0.724]
    assert row[18:] == [2, 1, 1, 2, 1, 1]
    empty = hp.performance_row_subsets([0] * 16, tru, [0, 0, 0, 0, 0, 5, 0, 0])
    assert empty[12:18] == [0, 0, 3, None, None, None]
    path = str(tmp_path / "caller_performance_hapsubsets.tsv")
    hp.write_performance_hapsubsets(path, [("lofreq", "TA-1-10", {"hap_rec": rec, "hap_tru": tru, "hap_sub": sub}),
                                           ("varscan", "TA-1-10", {"hap_rec": rec, "hap_tru": tru})])
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and len(lines) == 3
    head = lines[0].split("\t")
    assert head[:2] == ["caller", "mixture"] and head[14:20] == ["TP_S", "FP_S", "FN_S", "Precision_S", "Recall_S", "F1_S"]
    assert head[20:] == ["sites_searched", "sites_partial", "sites_nosubset", "rescued_S", "left_lines", "left_entries"]
    cells = lines[1].split("\t")
    assert cells[1] == "TA-1-10" and cells[14:] == ["7", "3", "2", "0.7", "0.75", "0.724", "2", "1", "1", "2", "1", "1"]
    hp.write_performance_hapsubsets(path, [("x", "s", {"hap_rec": [0] * 16, "hap_tru": tru, "hap_sub": [0, 0, 0, 0, 0, 5, 0, 0]})], custom=True)
    assert open(path).read().split("\n")[1].split("\t")[13:19] == ["0", "0", "3", "NA", "NA", "NA"]


def test_check_hapsub_and_the_pass_table():
    """the pass `hapsub` is the haplotype pass and the search behind it from one call: asked for in place of `haplo`, it needs the
    allele-extended mode, its jobs share one gap, and it shares its call with no other pass -- `haplo` included"""
    from quasimodo_amd.passes import PASSES, Pass, SharedCallError, check_alleles, check_shared_call
    with pytest.raises(ValueError, match=r"^haplo \("):              # not asked for: the one rule names haplo, which was
        check_alleles({"haplo"}, False)
    check_alleles({"hapsub"}, True)
    with pytest.raises(ValueError, match="--alleles"):
        check_alleles({"hapsub"}, False)
    (p,) = [x for x in PASSES if x.name == "hapsub"]
    assert p == Pass("hapsub", ("hapsub",), ("hapsub",), "--hap-subsets", "hapsub: the jobs of one call share one gap", ())
    check_shared_call({"hapsub"})
    for other in (x.name for x in PASSES):
        if other != "hapsub":
            with pytest.raises(SharedCallError):
                check_shared_call({"hapsub", other})


def test_the_subsets_file_is_read_back_as_written(tmp_path):
    path = tmp_path / "x.subsets.tsv"
    path.write_text(hp.SUBSETS_HEADER + "\n3\t110\t132\t7:120:ACG:T\t8:125:C:T;9:126:G:A\t120:ACG:A;120:A:T\t.\tAAT\tAAT\n")
    assert hp.read_subsets(str(path)) == [(3, 110, 132, [(7, "120", "ACG", "T")], [(8, "125", "C", "T"), (9, "126", "G", "A")],
                                           [(120, "ACG", "A"), (120, "A", "T")], [], "AAT", "AAT")]
    path.write_text("#site\n")
    with pytest.raises(ValueError, match="not a subsets file"):
        hp.read_subsets(str(path))

    class J:
        fp_out = "/o/callers/c/fp/s1.c.both.fp.vcf"
    assert hp.subsets_path(J) == "/o/callers/c/hap/s1.c.both.subsets.tsv" and hp.sites_path(J) == "/o/callers/c/hap/s1.c.both.sites.tsv"
