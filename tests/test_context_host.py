"""Sequence-context profiles, the parts that need no device: the numpy restatement of the position -> cell
table against cells written out by hand and against a per-position loop, the pass table's entry, the exports, the table writer
and the command line."""
import numpy as np
import pytest

from quasimodo_amd import _lib, passes
from quasimodo_amd import context as cx


# ---- a genome with every feature planted (shared with the device tests) ---------------------------------------------------
def planted_genome(seed, L=60000, tile=4096):
    """bytes [L]: a seeded random genome with runs of every length 1 .. 20 and one of 40 (flanked by other bases, so the lengths
    are exact), runs across the edges of the 8-base packed words and of the build kernel's tiles, an AT-only and a GC-only
    stretch of 300 bases, an N block longer than 2 * 1024 + 1, and lower case"""
    rng = np.random.default_rng(seed)
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].copy()

    def run(at, n, base):
        other = b"C" if base != b"C" else b"G"
        g[at - 1] = other[0]
        g[at:at + n] = base[0]
        g[at + n] = other[0]
    at = 100
    for n in list(range(1, 21)) + [40]:
        run(at, n, b"ACGT"[n % 4:n % 4 + 1])
        at += n + 37
    run(8 * 700 - 3, 7, b"G")                      # across a word edge
    run(8 * 701 + 7, 2, b"T")                      # the last base of a word and the first of the next
    run(tile - 5, 11, b"A")                        # across the first tile edge
    run(2 * tile - 1, 2, b"C")                     # one base on either side of the second
    run(3 * tile - 16, 16, b"T")                   # ends with a tile
    run(3 * tile + 16, 17, b"G")                   # the second lane of a tile
    g[20000:20300] = np.frombuffer(b"AT", np.uint8)[rng.integers(0, 2, 300)]
    g[21000:21300] = np.frombuffer(b"GC", np.uint8)[rng.integers(0, 2, 300)]
    g[30000:30000 + 2 * 1024 + 150] = ord("N")
    g[30500] = ord("R")                            # another byte that is no base, inside the block
    g[40000:40400] |= 32                           # lower case
    run(40100, 9, b"a")
    return g.tobytes()


def brute_cells(seq, w, ng):
    """the contract, position by position"""
    code = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}
    c = [code.get(b, 15) for b in seq]
    L = len(c)

    def run(i):                                    # 1-based
        if i < 1 or i > L or c[i - 1] > 3:
            return 0
        a = b = i
        while a > 1 and c[a - 2] == c[i - 1]:
            a -= 1
        while b < L and c[b] == c[i - 1]:
            b += 1
        return b - a + 1
    out = []
    for p in range(1, L + 1):
        hp = min(15, max(run(p - 1), run(p), run(p + 1)))
        win = c[max(1, p - w) - 1:min(L, p + w)]
        nb = sum(1 for x in win if x < 4)
        gc = sum(1 for x in win if x in (1, 2))
        out.append(255 if nb == 0 else hp * ng + min(ng - 1, gc * ng // nb))
    return np.array(out, np.uint8)


# ---- the table -----------------------------------------------------------------------------------------------------------
#          1234567 8901 2345678 901234 5 6..41
HAND = b"ACGGGTA" b"cccc" b"TAANAAC" b"NNNNNN" b"G" + b"T" * 16
# w = 2, ng = 4, cell = hp * 4 + gb, derived by hand:
#   runs: 1 1 (3 3 3) 1 1 (4 4 4 4) 1 (2 2) 0 (2 2) 1 (0 x 6) 1 (16 x 16); the N at 15 splits AANAA into two runs of 2
#   hp:   p1 1 (its right neighbour is a single C); p2 .. p5 3, p6 3 (the T just behind GGG); p7 .. p12 4 (p7 and p12 touch cccc);
#         p13 .. p18 2 (p15, the N, and p18, the C behind AA); p19 1 (behind the C); p20 .. p23 0; p24 1 (before the G);
#         p25 15 (the G before sixteen Ts); p26 .. p41 15
#   gb:   the windows p - 2 .. p + 2 cut at 1 and 41; p21 and p22 see only N: no cell
HAND_CELLS = [6, 15, 15, 15, 14, 14, 18, 18, 19, 19, 18, 17, 9, 8, 8, 9, 9, 9, 6, 3, 255, 255, 3, 6, 61, 61, 60] + [60] * 14


def test_cells_hand_case():
    assert len(HAND) == 41 == len(HAND_CELLS)
    got = cx.cells(HAND, 2, 4)
    assert got.dtype == np.uint8 and got.tolist() == HAND_CELLS
    np.testing.assert_array_equal(got, brute_cells(HAND, 2, 4))
    gen = cx.positions(got, 4)
    assert gen.shape == (65,) and gen.sum() == 41 and gen[64] == 2 and gen[60] == 15 and gen[61] == 2
    # p = 1 and p = L: the windows are cut at the genome's ends
    assert cx.cells(b"G", 0, 1).tolist() == [1] and cx.cells(b"G", 1024, 15).tolist() == [1 * 15 + 14]
    assert cx.cells(b"N", 5, 3).tolist() == [255] and cx.cells(b"", 5, 3).shape == (0,)
    assert cx.cells(b"NA", 0, 2).tolist() == [255, 2] and cx.cells(b"NA", 1, 2).tolist() == [2, 2]   # next to a base: row 1


@pytest.mark.parametrize("w,ng", [(0, 1), (1, 15), (50, 10), (1024, 7)])
def test_cells_equal_the_per_position_loop(w, ng):
    g = planted_genome(3, 60000)
    seq = g[80:900] + g[29900:30120] + g[32100:32300] + g[40050:40810]      # runs of 1 .. 20, an N block's edges, lower case
    assert len(seq) == 2000
    np.testing.assert_array_equal(cx.cells(seq, w, ng), brute_cells(seq, w, ng))


def test_the_planted_genome_fills_the_grid():
    """what the device comparison relies on: at (50, 10) every homopolymer row 1 .. 15, at least 8 GC bins and NONE are populated"""
    tab = cx.cells(planted_genome(1), 50, 10)
    gen = cx.positions(tab, 10)
    assert gen.sum() == 60000 and gen[160] > 0
    grid = gen[:160].reshape(16, 10)
    assert (grid.sum(axis=1)[1:] > 0).all() and (grid.sum(axis=0) > 0).sum() >= 8
    assert grid[0].sum() > 0                       # inside the N block, within 50 of its edges


def test_rows_of_and_names():
    tab = cx.cells(HAND, 2, 4)
    assert cx.rows_of(tab, [-3, 0, 1, 21, 41, 42, 1 << 30], 4).tolist() == [64, 64, 6, 64, 60, 64, 64]
    names = cx.cell_names(4)
    assert len(names) == 66 and names[0] == ("0", "0") and names[63] == ("15+", "3") and names[64] == ("none", "none") and names[65] == ("nokey", "nokey")
    assert cx.gc_bounds(3, 10) == (0.3, 0.4) and cx.gc_bounds(2, 15) == (0.133, 0.2)
    assert cx.n_cells(10) == 161


def test_parameter_limits():
    for w, ng in ((-1, 10), (1025, 10), (50, 0), (50, 16)):
        with pytest.raises(ValueError):
            cx.check_params(w, ng)
        with pytest.raises(ValueError):
            cx.cells(b"ACGT", w, ng)
    assert cx.check_params(0, 1) == (0, 1) and cx.check_params(1024, 15) == (1024, 15)
    assert (cx.MAX_HALF_WINDOW, cx.MAX_GC_BINS, cx.NONE_BYTE) == (_lib.QM_CX_MAX_HALF_WINDOW, _lib.QM_CX_MAX_GC_BINS, _lib.QM_CX_NONE)


# ---- the pass table, the exports -----------------------------------------------------------------------------------------
def test_pass_table_entry():
    names = [p.name for p in passes.PASSES]
    assert "context" in names and names[-1] == "surface" and names.index("context") == len(names) - 2
    p = passes.PASSES[names.index("context")]
    assert p.fields == ("context",) and p.keywords == ("context",) and p.shares == () and p.flag == "--seq-context"
    assert p.agree == "context: the profiled jobs of one call share one half window and one GC bin count"
    for other in names:
        if other != "context":
            with pytest.raises(passes.SharedCallError):
                passes.check_shared_call({"context", other})
    passes.check_shared_call({"context"})


def test_exports_abi_and_kernels_id():
    for name in ("qm_genome_context", "qm_batch_context", "qm_batch_get_context", "qm_batch_context_timings", "qm_extract_files_context"):
        assert name in _lib.EXPORTS
    assert _lib.QM_ABI_VERSION == 6
    assert _lib.source_kernels_id() == "db744d8883a55744"      # the classification kernels are untouched
    assert "qmvt_context.hip" in _lib._ASRC and "qmvt_context.h" in _lib._ASRC and "qmvt_context.hip" not in _lib._KSRC


# ---- the table writer -------------------------------------------------------------------------------------------------------
def _literal(ng=2):
    nc = cx.n_cells(ng)
    rec, tru, gen = np.zeros((nc + 1, 3), np.uint64), np.zeros((nc, 2), np.uint64), np.zeros(nc, np.uint64)
    gen[1 * ng + 0], gen[1 * ng + 1], gen[15 * ng + 1], gen[nc - 1] = 3000, 7, 40, 5
    rec[1 * ng + 0] = [9, 6, 3]
    rec[15 * ng + 1] = [7, 1, 6]
    rec[3 * ng + 0] = [1, 0, 1]                    # a count in a cell without positions (a record of another genome's coordinates)
    rec[nc - 1] = [2, 0, 2]
    rec[nc] = [4, 1, 3]
    tru[1 * ng + 0] = [8, 6]
    tru[15 * ng + 1] = [3, 1]
    tru[nc - 1] = [1, 0]
    return rec, tru, gen


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]


def test_table_writer(tmp_path):
    rec, tru, gen = _literal()
    st = {"context_rec": rec, "context_tru": tru, "context_gen": gen, "pure_strain": False}
    pure = {"context_rec": rec, "context_tru": np.zeros_like(tru), "context_gen": gen, "pure_strain": True}
    p = str(tmp_path / "t.tsv")
    cx.write_performance_context(p, [("lofreq", "TA-1-10", st), ("clc", "TA-0-1", pure)], 2)
    head, rows = _table(p)
    assert head == ("caller mixture homopolymer gc_bin gc_from gc_to positions calleridentify TP_lines FP_lines genomediff TP FN "
                    "Precision Recall F1 FP_per_kb").split()
    per = 4 + 16 + 2 + 2                           # the cells in use, the two marginal families, none, nokey
    assert len(rows) == 2 * per
    mine = rows[:per]
    assert all(r["caller"] == "LoFreq" and r["mixture"] == "TA-1-10" for r in mine) and rows[per]["caller"] == "CLC"
    assert [(r["homopolymer"], r["gc_bin"]) for r in mine[:5]] == [("1", "0"), ("1", "1"), ("3", "0"), ("15+", "1"), ("0", "all")]
    c10 = mine[0]
    assert (c10["gc_from"], c10["gc_to"], c10["positions"]) == ("0", "0.5", "3000")
    assert (c10["calleridentify"], c10["TP_lines"], c10["FP_lines"], c10["genomediff"], c10["TP"], c10["FN"]) == ("9", "6", "3", "8", "6", "2")
    assert (c10["Precision"], c10["Recall"], c10["F1"], c10["FP_per_kb"]) == ("0.667", "0.75", "0.706", "1")
    assert mine[1]["calleridentify"] == "0" and mine[1]["Precision"] == "NA" and mine[1]["Recall"] == "NA" and mine[1]["FP_per_kb"] == "0"
    assert mine[2]["positions"] == "0" and mine[2]["FP_per_kb"] == "NA" and mine[2]["Precision"] == "0" and mine[2]["F1"] == "NA"
    long_ = mine[3]
    assert (long_["homopolymer"], long_["gc_from"], long_["gc_to"], long_["FP_per_kb"], long_["Recall"]) == ("15+", "0.5", "1", "150", "0.333")
    hp_rows, gc_rows, none, nokey = mine[4:20], mine[20:22], mine[22], mine[23]
    assert [r["homopolymer"] for r in hp_rows] == [str(h) for h in range(15)] + ["15+"] and all(r["gc_bin"] == "all" and r["gc_from"] == "NA" for r in hp_rows)
    assert [(r["homopolymer"], r["gc_bin"]) for r in gc_rows] == [("all", "0"), ("all", "1")]
    assert (none["homopolymer"], none["gc_bin"], none["positions"], none["FP_lines"], none["genomediff"], none["FN"], none["FP_per_kb"]) == ("none", "none", "5", "2", "1", "1", "400")
    assert (nokey["homopolymer"], nokey["positions"], nokey["calleridentify"], nokey["genomediff"], nokey["TP"], nokey["Precision"], nokey["FP_per_kb"]) == ("nokey", "NA", "4", "NA", "NA", "NA", "NA")
    num = lambda x: 0 if x == "NA" else int(x)
    for fam in (hp_rows, gc_rows):                 # each marginal family plus none and nokey is the whole genome
        for col, want in (("calleridentify", 23), ("TP_lines", 8), ("FP_lines", 15), ("genomediff", 12), ("TP", 7), ("positions", 3052)):
            assert sum(num(r[col]) for r in fam + [none, nokey]) == want, col
    # a pure-strain sample: TP 0, Precision 0, the other truth-side columns NA; nokey as ever
    pr = rows[per]
    assert (pr["genomediff"], pr["TP"], pr["FN"], pr["Precision"], pr["Recall"], pr["F1"], pr["FP_per_kb"]) == ("NA", "0", "NA", "0", "NA", "NA", "1")
    # genomediff from the truth file's rows replaces the distinct keys; the custom spelling has no mixture column
    gd = np.zeros(cx.n_cells(2), np.int64)
    gd[2] = 10
    cx.write_performance_context(p, [("c0", None, dict(st, context_genomediff=gd, pure_strain=True))], 2, custom=True)
    head, rows = _table(p)
    assert head[:2] == ["caller", "homopolymer"] and head[-4:] == ["precision", "recall", "f1", "FP_per_kb"]
    assert (rows[0]["caller"], rows[0]["genomediff"], rows[0]["TP"], rows[0]["FN"], rows[0]["recall"]) == ("c0", "10", "6", "4", "0.6")
    # no truth side at all (an allele-extended call)
    cx.write_performance_context(p, [("lofreq", "s", dict(st, context_tru=None))], 2)
    assert _table(p)[1][0]["genomediff"] == "NA" and _table(p)[1][0]["FP_lines"] == "3"


def test_truth_rows_places_the_counted_rows(tmp_path):
    tab = cx.cells(HAND, 2, 4)
    f = tmp_path / "t.vcf"
    f.write_text("#h\nx\t2\t.\tC\tT\nx\t2\t.\tC\tT\nx\t21\t.\tA\tG\nx\t99\t.\tA\tG\nx\t5\t.\tAC\tG\nx\tzz\t.\tA\tG\n")
    got = cx.truth_rows(str(f), "hcmv", tab, 4)
    assert got.sum() == 5 and got[15] == 2 and got[64] == 3


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_dryrun_lists_the_table(tmp_path):
    import subprocess, sys, os
    from test_tables_workflow import _build_bundle
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGTACGTAC\n")
    cmd = [sys.executable, os.path.join(root, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data), "-o", str(tmp_path / "o"), "--dryrun"]
    ref = ["--merlin-ref", str(fa), "--ad169-ref", str(fa)]
    off = subprocess.run(cmd, capture_output=True, text=True)
    on = subprocess.run(cmd + ["--seq-context"] + ref, capture_output=True, text=True)
    assert off.returncode == 0 and on.returncode == 0, on.stderr
    assert "caller_performance_context.tsv" in on.stdout and "caller_performance_context.tsv" not in off.stdout
