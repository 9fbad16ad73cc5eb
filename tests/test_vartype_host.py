"""The host side of TP, FP and FN by variant type and size: the definition on strings (vartype.shape) against
hand-checked literals, the kernels' integer arithmetic (vartype.shape_codes) against it on random pairs at every inline length and
on long / short pairs through a shape table, qm_dict_shapes against Python slicing, the size bins, the pass-table entry, the
exports and the table writer.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from quasimodo_amd import vartype as vt

T = {name: k for k, name in enumerate(vt.TYPE_NAMES)}

# R -> A, type, size: checked by hand against the definition (prefix first and greedy, then the suffix of what is left)
LITERALS = [
    ("A", "G", "SNV", 1), ("AC", "AT", "SNV", 1), ("ATA", "ACA", "SNV", 1), ("AC", "GT", "MNP", 2), ("ACG", "TCA", "MNP", 3),
    ("A", "AT", "INS", 1), ("A", "AA", "INS", 1), ("AT", "ACGT", "INS", 2), ("AT", "A", "DEL", 1), ("AA", "A", "DEL", 1),
    ("ATA", "A", "DEL", 2), ("CAC", "C", "DEL", 2), ("ACGT", "AT", "DEL", 2), ("AC", "G", "CPX", 2), ("ACG", "TT", "CPX", 3),
    ("ACGTACGTACGTA", "A", "DEL", 12), ("A", "ACGTACGTACGTAC", "INS", 13), ("G", "ACGTACGTACGTAC", "CPX", 14),
    ("ACGTACGTACGTACG", "AG", "DEL", 13), ("ACGTACGTACGTACG", "ATG", "CPX", 13), ("TC", "TCATCATCATCATCATC", "INS", 15),
]


def test_the_literal_table():
    for ref, alt, kind, size in LITERALS:
        assert vt.shape(ref, alt) == (T[kind], size), (ref, alt)
    with pytest.raises(ValueError, match="no variant"):
        vt.shape("ACG", "ACG")


class Codes:
    """allele strings as codes: inline up to 13 bases, ids of this test's own dictionary beyond"""

    def __init__(self):
        self.strings = []

    def __call__(self, s):
        if len(s) <= vt.INLINE_MAX:
            return vt.code(s)
        if s not in self.strings:
            self.strings.append(s)
        return vt.DICT | self.strings.index(s)


def test_the_literal_table_on_codes():
    code = Codes()
    pairs = [(code(r), code(a)) for r, a, _, _ in LITERALS]
    shapes = vt.shapes_of(code.strings)
    for (r, a), (ref, alt, kind, size) in zip(pairs, LITERALS):
        assert vt.shape_codes(r, a, shapes) == (T[kind], size), (ref, alt)


def test_shape_codes_equals_shape_at_every_inline_length():
    """both orientations, every pair of lengths 1 .. 13; an alphabet of two bases makes long common prefixes and suffixes likely"""
    rng = np.random.default_rng(5)
    n, seen = 0, set()
    for lr in range(1, 14):
        for la in range(1, 14):
            for rep in range(150):
                alpha = "ACGT" if rep % 3 == 0 else "AC"
                ref = "".join(alpha[i] for i in rng.integers(0, len(alpha), lr))
                alt = "".join(alpha[i] for i in rng.integers(0, len(alpha), la))
                if rep % 5 == 0 and lr != la:                      # a pure indel by construction: the short allele cut out of the long one
                    lo, sh = (ref, la) if lr > la else (alt, lr)
                    k = int(rng.integers(0, sh + 1))
                    cut = lo[:k] + lo[len(lo) - (sh - k):] if sh > k else lo[:k]
                    ref, alt = (lo, cut) if lr > la else (cut, lo)
                if ref == alt:
                    assert vt.shape_codes(vt.code(ref), vt.code(alt)) == (None, vt.NOVAR)
                    continue
                want = vt.shape(ref, alt)
                assert vt.shape_codes(vt.code(ref), vt.code(alt)) == want, (ref, alt)
                seen.add(want[0])
                n += 1
    assert n > 20000 and seen == set(range(5))


def test_head_and_tail_decide_every_long_short_pair():
    """The head / tail equivalence: 10^5 pairs of a long allele (14 .. 60 bases; 14 .. 26: head and tail overlap) and a short one
    (1 .. 13), half of them pure indels by construction (the short allele is a prefix and a suffix of the long one put together),
    in both orientations, through a shape table built from the strings -- against the full-string rule."""
    rng = np.random.default_rng(6)
    strings, pairs = [], []
    for i in range(50_000):
        n_long = int(rng.integers(14, 27 if i % 2 else 61))
        n_short = int(rng.integers(1, 14))
        alpha = "ACGT" if i % 3 else "AC"
        long_ = "".join(alpha[k] for k in rng.integers(0, len(alpha), n_long))
        if i % 2 == 0:
            k = int(rng.integers(0, n_short + 1))
            short = long_[:k] + (long_[n_long - (n_short - k):] if n_short > k else "")
        else:
            short = "".join(alpha[k] for k in rng.integers(0, len(alpha), n_short))
        strings.append(long_)
        pairs.append((i, short))
    shapes = vt.shapes_of(strings)
    kinds = np.zeros(5, np.int64)
    for i, short in pairs:
        want = vt.shape(strings[i], short)
        assert vt.shape_codes(vt.DICT | i, vt.code(short), shapes) == want, (strings[i], short)
        back = vt.shape(short, strings[i])
        assert vt.shape_codes(vt.code(short), vt.DICT | i, shapes) == back, (short, strings[i])
        kinds[want[0]] += 1
        kinds[back[0]] += 1
        if i % 2 == 0:
            assert want == (vt.DEL, len(strings[i]) - len(short)) and back == (vt.INS, len(strings[i]) - len(short))
    assert kinds.sum() == 100_000 and kinds[vt.INS] >= 25_000 and kinds[vt.DEL] >= 25_000 and kinds[vt.CPX] > 10_000
    assert kinds[vt.SNV] == kinds[vt.MNP] == 0           # the lengths differ


def test_rows_behind_the_grid_and_their_order():
    shapes = vt.shapes_of(["ACGTACGTACGTAC", "ACGTACGTACGTACGT"])
    a, long0, long1, past = vt.code("A"), vt.DICT | 0, vt.DICT | 1, vt.DICT | 2
    assert vt.shape_codes(a, long0, shapes) == (vt.INS, 13)
    assert vt.shape_codes(long0, long0, shapes, nokey=True) == (None, vt.NOKEY)     # NOKEY in front of NOVAR
    assert vt.shape_codes(-1, a, shapes) == (None, vt.NOKEY) and vt.shape_codes(a, 5, shapes) == (None, vt.NOKEY)
    assert vt.shape_codes(past, past, shapes) == (None, vt.NOVAR)                   # NOVAR in front of LONGPAIR and NOSHAPE
    assert vt.shape_codes(long0, long1, shapes) == (None, vt.LONGPAIR)
    assert vt.shape_codes(long0, past, shapes) == (None, vt.LONGPAIR)               # LONGPAIR in front of NOSHAPE
    assert vt.shape_codes(a, past, shapes) == (None, vt.NOSHAPE) and vt.shape_codes(past, a, shapes) == (None, vt.NOSHAPE)
    assert vt.shape_codes(a, long0, None) == (None, vt.NOSHAPE)                     # no table
    assert vt.shape_codes(a, 14 << 26, shapes) == (None, vt.NOSHAPE)                # valid, no inline code, no id
    edges = (1, 2, 6)
    assert vt.row_codes(a, long0, edges, shapes) == vt.INS * 3 + 2 and vt.row_codes(a, long0, edges) == 15 + vt.NOSHAPE
    assert vt.row_codes(a, a, edges) == 15 + vt.NOVAR and vt.row_codes(a, vt.code("C"), edges, nokey=True) == 15 + vt.NOKEY


def test_dict_shapes_against_slicing():
    from quasimodo_amd import _lib
    from quasimodo_amd.vcfio import AlleleDict
    rng = np.random.default_rng(7)
    strings = ["ACGTACGTACGTAC", "ACGTTGCATTGACCAGTTACGATAC", "T" * 27, "ACGTACGTACGTACGTACGTACGTACG"]      # 14, 25, 27 and 27 bases
    strings += ["".join("ACGT"[k] for k in rng.integers(0, 4, int(n))) for n in rng.integers(14, 200, 40)]
    d = AlleleDict()
    try:
        assert [a.shape for a in d.shapes()] == [(0,)] * 3                         # an empty dictionary
        assert d.code(b"ACGTACGTACGTA") == vt.code("ACGTACGTACGTA")                 # thirteen bases: inline, not interned
        ids = [d.code(s.encode()) for s in strings]
        assert ids == [vt.DICT | i for i in range(len(strings))] and d.code(strings[1].encode()) == ids[1]
        ln, head, tail = d.shapes()
        assert ln.dtype == np.int32 and head.dtype == tail.dtype == np.uint32 and len(ln) == len(d) == len(strings)
        for i, s in enumerate(strings):
            assert (int(ln[i]), int(head[i]), int(tail[i])) == (len(s), vt.pack(s[:13]), vt.pack(s[-13:])), s
        want = vt.shapes_of(strings)
        for got, w in zip((ln, head, tail), want):
            np.testing.assert_array_equal(got, w)
        # a window of rows, and one past the end
        L = _lib.lib()
        l3, h3, t3 = np.zeros(3, np.int32), np.zeros(3, np.uint32), np.zeros(3, np.uint32)
        p = lambda x: x.ctypes.data_as(C.c_void_p)
        assert L.qm_dict_shapes(d._h, 2, 3, p(l3), p(h3), p(t3)) == 3 and l3.tolist() == ln[2:5].tolist() and t3.tolist() == tail[2:5].tolist()
        assert L.qm_dict_shapes(d._h, len(strings) - 1, 3, p(l3), p(h3), p(t3)) == 1 and l3[0] == ln[-1]
        assert L.qm_dict_shapes(d._h, len(strings), 3, p(l3), p(h3), p(t3)) == 0
        assert L.qm_dict_shapes(None, 0, 3, p(l3), p(h3), p(t3)) == 0
    finally:
        d.close()


def test_edges_bins_and_row_names():
    assert vt.check_edges() == vt.DEFAULT_EDGES == (1, 2, 3, 4, 5, 6, 16, 51)
    assert vt.check_edges([1]) == (1,) and vt.check_edges(range(1, 17)) == tuple(range(1, 17))
    assert vt.parse_edges("1,2,6") == (1, 2, 6)
    for bad, said in (([], "size bins"), (list(range(1, 18)), "size bins"), ([2, 3], "first size edge"), ([0, 1], "first size edge"),
                      ([1, 3, 3], "ascend"), ([1, 5, 4], "ascend"), ([1, 2.5], "integers"), ([1, 1 << 31], "31 bits")):
        with pytest.raises(ValueError, match=said):
            vt.check_edges(bad)
    with pytest.raises(ValueError, match="comma-separated"):
        vt.parse_edges("1,x")
    e = vt.DEFAULT_EDGES
    assert [vt.bin_of(s, e) for s in (1, 2, 5, 6, 15, 16, 50, 51, 10 ** 6)] == [0, 1, 4, 5, 5, 6, 6, 7, 7]
    assert [vt.bin_of(s, (1,)) for s in (1, 99)] == [0, 0]
    assert vt.size_labels(e) == ["1", "2", "3", "4", "5", "6-15", "16-50", "51+"] and vt.size_labels((1,)) == ["1+"]
    names = vt.row_names(e)
    assert len(names) == vt.n_rows(e) == 44 and names[0] == "SNV:1" and names[8] == "MNP:1" and names[2 * 8 + 5] == "INS:6-15"
    assert names[39] == "CPX:51+" and names[40:] == ["NOKEY", "NOVAR", "LONGPAIR", "NOSHAPE"]
    assert vt.n_rows(tuple(range(1, 17))) == 84 and vt.row_of(vt.DEL, 7, e) == 3 * 8 + 5


def test_the_pass_table():
    from quasimodo_amd import passes
    names = [p.name for p in passes.PASSES]
    i = names.index("vartype")
    assert names[i - 1] == "atomize" and names[i + 1] == "context" and names[-2:] == ["context", "surface"]
    p = passes.PASSES[i]
    assert p.flag == "--by-type" and p.fields == ("vartype",) and p.keywords == ("vartype",) and p.shares == ()
    assert p.agree == "vartype: the typed jobs of one call share one list of size edges"
    for other in names:
        if other != "vartype":
            with pytest.raises(passes.SharedCallError):
                passes.check_shared_call({"vartype", other})
    passes.check_shared_call({"vartype"})
    passes.check_alleles({"vartype"}, True)
    with pytest.raises(ValueError, match=r"^atomize \("):                        # (the one rule names the pass that was asked for, not this one)
        passes.check_alleles({"atomize"}, False)
    with pytest.raises(ValueError, match="--alleles"):
        passes.check_alleles({"vartype"}, False)


def test_refusals_in_front_of_any_file(tmp_path):
    from conftest import ROOT
    from quasimodo_amd import workflow
    from quasimodo_amd.extract import Job, extract_many
    fa = str(tmp_path / "a.fa")
    mk = lambda **kw: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i, **kw) for i in range(2)]
    with pytest.raises(ValueError, match="--alleles"):
        extract_many(mk(), vartype=True)
    with pytest.raises(ValueError, match="--alleles"):
        extract_many(mk(), alleles=False, vartype=[1, 2, 6])
    with pytest.raises(ValueError, match="first size edge"):
        extract_many(mk(), alleles=True, vartype=[2, 6])
    jobs = mk()
    jobs[0].vartype, jobs[1].vartype = (1, 2), (1, 3)
    with pytest.raises(ValueError, match="share one list of size edges"):
        extract_many(jobs, alleles=True)
    for other in (dict(fn=True), dict(strata=[("all", [0], [100])]), dict(boot={}), dict(explain=3), dict(surface=True),
                  dict(context={"genomes": [fa, fa]}), dict(genomes=[fa, fa]), dict(normalize=[fa, fa]), dict(atomize=True)):
        with pytest.raises(ValueError, match="does not combine"):
            extract_many(mk(), alleles=True, vartype=True, **other)
    with pytest.raises(workflow.WorkflowError, match="--by-type needs --alleles"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), by_type=True)
    with pytest.raises(workflow.WorkflowError, match="--type-bins"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, by_type="1,1")
    with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, by_type=True, atomize=True)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", str(tmp_path / "a.vcf"), "--snps", str(tmp_path / "a.snps"),
                        "-l", "a", "-o", str(tmp_path / "v"), "--by-type"], capture_output=True, text=True)
    assert r.returncode != 0 and "allele-extended" in r.stderr + r.stdout and "--by-type" in r.stderr + r.stdout
    assert not any(x.is_file() for x in tmp_path.rglob("*")) and not (tmp_path / "v").exists()   # no file was written


def test_exports_ids_and_constants():
    from conftest import ROOT
    from quasimodo_amd import _lib
    text = open(os.path.join(ROOT, "include", "qmvt.h")).read()
    for name in ("qm_dict_shapes", "qm_batch_types", "qm_batch_get_types", "qm_batch_get_typed", "qm_batch_types_timings", "qm_extract_files_types"):
        assert name in _lib.EXPORTS and name in text
        assert hasattr(_lib.lib(), name)
    assert _lib.QM_ABI_VERSION == 6 and "#define QM_ABI_VERSION 6" in text and _lib.lib().qm_abi_version() == 6
    assert _lib.source_kernels_id() == "db744d8883a55744"
    assert "qmvt_types.hip" in _lib._ASRC and "qmvt_types.h" in _lib._ASRC
    assert "qmvt_types.hip" not in _lib._KSRC and "qmvt_types.h" not in _lib._KSRC
    mk = open(os.path.join(ROOT, "quasimodo_amd", "csrc", "Makefile")).read()
    ksrc = next(ln for ln in mk.split("\n") if ln.startswith("KSRC ="))
    asrc = next(ln for ln in mk.split("\n") if ln.startswith("ASRC ="))
    assert "qmvt_types" not in ksrc and "qmvt_types.hip qmvt_types.h" in asrc and "qmvt_types.o" in mk
    assert _lib.QM_TYPE_MAX_BINS == vt.MAX_BINS == 16 and "#define QM_TYPE_MAX_BINS 16" in text
    assert _lib.QM_TYPE_MAX_ROWS == 5 * 16 + 4 and "#define QM_TYPE_MAX_ROWS 84" in text and "#define QM_TYPE_COLUMNS 2u" in text
    for k, name in enumerate(vt.TYPE_NAMES):
        assert "QM_TYPE_%s = %d" % (name, k) in text and getattr(_lib, "QM_TYPE_" + name) == k
    for k, name in enumerate(vt.OFFGRID_NAMES):
        assert "QM_TYPE_X_%s = %d" % (name, k) in text and getattr(_lib, "QM_TYPE_X_" + name) == k
    assert vt.INLINE_MAX == 13 and "#define QM_ALLELE_INLINE_MAX 13" in text


def hand_case():
    """truth: an SNV, an MNP, a 1-base insertion, a 2-base deletion, a 20-base insertion (id 0); records below"""
    c = vt.code
    long_ = "A" + "CGTACGTACGTACGTACGTA"                                # A -> A + 20 bases: INS 20
    shapes = vt.shapes_of([long_, "G" * 14, "T" * 15])
    truth = ([100, 200, 300, 400, 500], [c("A"), c("AC"), c("A"), c("CAC"), c("A")], [c("G"), c("GT"), c("AT"), c("C"), vt.DICT | 0])
    rows = [                                                              # (pos, ref, alt, flags, kept, tp)
        (100, c("A"), c("G"), 3, True, True),                             # SNV, TP, finds its entry
        (100, c("A"), c("G"), 1, True, False),                            # the same with an ID: kept, FP, SNV
        (200, c("AC"), c("GT"), 3, True, True),                           # MNP 2
        (300, c("A"), c("AA"), 3, True, False),                           # INS 1, not the truth's spelling
        (400, c("CAC"), c("C"), 3, False, False),                         # DEL 2, not kept: its entry stays missed
        (500, c("A"), vt.DICT | 0, 3, True, True),                        # INS 20 through the table
        (600, vt.DICT | 1, vt.DICT | 2, 3, True, False),                  # LONGPAIR
        (700, c("A"), vt.DICT | 9, 3, True, False),                       # NOSHAPE
        (800, c("AC"), c("AC"), 3, True, False),                          # NOVAR
        (0, c("A"), c("C"), 7, True, False),                              # NOKEY
        (900, c("AC"), c("G"), 3, True, False),                           # CPX 2
    ]
    return truth, rows, shapes


def test_counts_on_a_hand_written_vcf_and_truth_set():
    truth, rows, shapes = hand_case()
    cols = [np.array([r[k] for r in rows]) for k in range(6)]
    e = (1, 2, 6)
    rec, tru, row = vt.counts(truth, cols[0], cols[1], cols[2], cols[3], cols[4].astype(bool), cols[5].astype(bool), e, shapes)
    names = vt.row_names(e)
    assert [names[k] for k in row] == ["SNV:1", "SNV:1", "MNP:2-5", "INS:1", "DEL:2-5", "INS:6+", "LONGPAIR", "NOSHAPE", "NOVAR", "NOKEY", "CPX:2-5"]
    got = {names[k]: (rec[k].tolist(), tru[k].tolist()) for k in range(len(names)) if rec[k].any() or tru[k].any()}
    assert got == {"SNV:1": ([2, 1], [1, 1]), "MNP:2-5": ([1, 1], [1, 1]), "INS:1": ([1, 0], [1, 0]), "DEL:2-5": ([0, 0], [1, 0]),
                   "INS:6+": ([1, 1], [1, 1]), "CPX:2-5": ([1, 0], [0, 0]), "NOKEY": ([1, 0], [0, 0]), "NOVAR": ([1, 0], [0, 0]),
                   "LONGPAIR": ([1, 0], [0, 0]), "NOSHAPE": ([1, 0], [0, 0])}
    # without the table the long records and the long entry land in NOSHAPE; LONGPAIR comes first
    rec0, tru0, row0 = vt.counts(truth, cols[0], cols[1], cols[2], cols[3], cols[4].astype(bool), cols[5].astype(bool), e, None)
    assert names[row0[5]] == "NOSHAPE" and names[row0[6]] == "LONGPAIR" and rec0[15 + vt.NOSHAPE].tolist() == [2, 1] and tru0[15 + vt.NOSHAPE].tolist() == [1, 1]
    assert int(rec0[:, 0].sum()) == int(rec[:, 0].sum()) == 10 and int(tru0[:, 0].sum()) == int(tru[:, 0].sum()) == 5


def test_table_writer_on_a_hand_written_block(tmp_path):
    e = (1, 2, 6)
    nr = vt.n_rows(e)
    rec, tru = np.zeros((nr, 2), np.uint64), np.zeros((nr, 2), np.uint64)
    rec[0], tru[0] = (10, 8), (12, 6)                   # SNV:1    TP 8, FP 2, FN 6, P 0.8, R 0.5, F1 0.615
    rec[7], tru[7] = (3, 1), (4, 1)                     # INS:2-5  TP 1, FP 2, FN 3, P 0.333, R 0.25, F1 0.286
    rec[8], tru[8] = (1, 1), (2, 2)                     # INS:6+   TP 1, FP 0, FN 0, P 1, R 1, F1 1
    tru[9] = (5, 0)                                     # DEL:1    no kept record: 0, 0, 5, NA
    rec[15 + vt.NOVAR] = (2, 0)
    rec[15 + vt.LONGPAIR], tru[15 + vt.LONGPAIR] = (1, 1), (3, 1)
    path = tmp_path / "t.tsv"
    st = {"type_rec": rec, "type_tru": tru}
    vt.write_performance_types(str(path), [("lofreq", "TM-1-1", st), ("lofreq", "TM-1-0", {}), ("lofreq", "TM-1-10", st), ("x", "TM-1-1", st)], e)
    lines = path.read_text().split("\n")
    assert lines[0].split("\t") == list(vt.TABLE_HEADER) and lines[-1] == ""
    body = [ln.split("\t") for ln in lines[1:-1]]
    per = 5 * 4 + 4                                     # three bins and `all` per type, the four rows behind the grid
    assert len(body) == per * 5                         # three jobs, two pooled blocks
    assert [r[:2] for r in body[::per]] == [["LoFreq", "TM-1-1"], ["LoFreq", "TM-1-10"], ["x", "TM-1-1"], ["LoFreq", "pooled"], ["x", "pooled"]]
    first = {(r[2], r[3]): r[4:] for r in body[:per]}
    assert first[("SNV", "1")] == ["8", "2", "6", "0.8", "0.5", "0.615"] and first[("SNV", "all")] == first[("SNV", "1")]
    assert first[("INS", "2-5")] == ["1", "2", "3", "0.333", "0.25", "0.286"] and first[("INS", "6+")] == ["1", "0", "0", "1", "1", "1"]
    assert first[("INS", "all")] == ["2", "2", "3", "0.5", "0.5", "0.5"]
    assert first[("DEL", "1")] == ["0", "0", "5", "NA", "NA", "NA"] and first[("MNP", "all")] == ["0", "0", "0", "NA", "NA", "NA"]
    assert first[("NOVAR", "NA")] == ["0", "2", "0", "NA", "NA", "NA"] and first[("LONGPAIR", "NA")] == ["1", "0", "2", "NA", "NA", "NA"]
    assert [r[2:4] for r in body[:4]] == [["SNV", "1"], ["SNV", "2-5"], ["SNV", "6+"], ["SNV", "all"]]
    assert [r[2] for r in body[per - 4:per]] == list(vt.OFFGRID_NAMES)
    pooled = {(r[2], r[3]): r[4:] for r in body[3 * per:4 * per]}
    assert pooled[("SNV", "1")] == ["16", "4", "12", "0.8", "0.5", "0.615"] and pooled[("LONGPAIR", "NA")] == ["2", "0", "4", "NA", "NA", "NA"]
    with pytest.raises(ValueError, match="count blocks of shape"):
        vt.write_performance_types(str(path), [("c", "s", st)], (1, 2))
