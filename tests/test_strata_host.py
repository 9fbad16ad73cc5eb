"""BED strata on the host (quasimodo_amd.strata): the readers on literal texts, the segment table against a
brute-force mask per position, the table writer against hand-computed rows.  No device."""
import numpy as np
import pytest

from quasimodo_amd import strata as st
from quasimodo_amd.tables import r_round3

I32MAX = (1 << 31) - 1


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode())
    return str(p)


# ---- readers --------------------------------------------------------------------------------------------------------------
def test_read_bed_skips_and_splits(tmp_path):
    p = _write(tmp_path, "repeats.hcmv.bed",
               "# a comment\n"
               "track name=x description=\"y\"\n"
               "browser position chr1:1-100\n"
               "\n"
               "chr1\t10\t20\n"
               "chrX   30    45   extra  columns\r\n"          # blanks against tabs, CRLF
               "   \n"
               "other \t 5\t6\tname\r\n")
    name, s, e = st.read_bed(p)
    assert name == "repeats.hcmv"                              # the file's stem; the chrom column is ignored
    assert s.tolist() == [10, 30, 5] and e.tolist() == [20, 45, 6]


def test_read_bed_by_name_order_of_first_appearance(tmp_path):
    p = _write(tmp_path, "genes.bed", "c\t0\t10\tUL74\nc\t20\t30\tUL73\n#x\nc 40 50 UL74 0 +\n")
    got = st.read_bed_by_name(p)
    assert [g[0] for g in got] == ["UL74", "UL73"]
    assert got[0][1].tolist() == [0, 40] and got[0][2].tolist() == [10, 50]
    assert got[1][1].tolist() == [20] and got[1][2].tolist() == [30]


@pytest.mark.parametrize("text,line,what", [
    ("c\t1\t2\nc\t5\n", 2, "column"),                          # fewer than 3 columns
    ("c\t1\t2\n\nc\t7\t7\n", 3, "end"),                        # end <= start
    ("c\t9\t3\n", 1, "end"),
    ("#h\nc\t-1\t3\n", 2, "negative"),
    ("c\t1\tx\n", 1, "integer"),
    ("c\t1.5\t3\n", 1, "integer"),
    ("c\t1\t%d\n" % (I32MAX + 1), 1, "2^31"),
])
def test_read_bed_refuses_with_file_and_line(tmp_path, text, line, what):
    p = _write(tmp_path, "bad.bed", text)
    with pytest.raises(ValueError) as ei:
        st.read_bed(p)
    assert p in str(ei.value) and "line %d" % line in str(ei.value) and what in str(ei.value)


def test_read_bed_by_name_refuses(tmp_path):
    p = _write(tmp_path, "three.bed", "c\t1\t2\tn\nc\t1\t2\n")
    with pytest.raises(ValueError, match="line 2"):
        st.read_bed_by_name(p)
    p = _write(tmp_path, "many.bed", "".join("c\t%d\t%d\tn%d\n" % (k, k + 1, k) for k in range(33)))
    with pytest.raises(ValueError) as ei:
        st.read_bed_by_name(p)
    assert p in str(ei.value) and "line 33" in str(ei.value)
    p32 = _write(tmp_path, "ok.bed", "".join("c\t%d\t%d\tn%d\n" % (k, k + 1, k) for k in range(32)))
    assert len(st.read_bed_by_name(p32)) == 32


def test_strata_set_limits():
    with pytest.raises(ValueError, match="empty"):
        st.flatten([])
    with pytest.raises(ValueError, match="33"):
        st.flatten([("s%d" % k, [k], [k + 1]) for k in range(33)])
    for s, e in (([-1], [4]), ([4], [4]), ([5], [4]), ([0], [I32MAX + 1])):
        with pytest.raises(ValueError):
            st.flatten([("a", s, e)])


# ---- the segment table ----------------------------------------------------------------------------------------------------
def brute_masks(strata, lo, hi):
    """mask of every position lo .. hi - 1, interval by interval: start < p <= end"""
    p = np.arange(lo, hi, dtype=np.int64)
    m = np.zeros(p.shape[0], np.uint32)
    for k, (_, s, e) in enumerate(strata):
        inside = np.zeros(p.shape[0], bool)
        for a, b in zip(s, e):
            inside |= (p > a) & (p <= b)
        m |= inside.astype(np.uint32) << np.uint32(k)
    return m


def random_strata(rng, n_strata, genome=2000, per=6):
    out = []
    for k in range(n_strata):
        s = rng.integers(0, genome - 1, per)
        e = np.minimum(s + rng.integers(1, 200, per), genome)
        if k % 3 == 0:                                          # touching: the next interval starts where this one ends
            s = np.append(s, e[0]); e = np.append(e, min(int(e[0]) + 17, genome))
        if k % 3 == 1:                                          # nested
            s = np.append(s, s[1] + 1) if e[1] - s[1] > 2 else s
            e = np.append(e, e[1] - 1) if len(s) > len(e) else e
        out.append(("s%d" % k, s.astype(np.int64), e.astype(np.int64)))
    return out


def check_table(strata, lo=-50, hi=2100):
    b, m = st.flatten(strata)
    assert b.dtype == np.int32 and m.dtype == np.uint32 and b.shape == m.shape
    assert b[0] == -(1 << 31) and m[0] == 0 and (np.diff(b.astype(np.int64)) > 0).all()
    assert (m[1:] != m[:-1]).all(), "equal neighbours are merged"
    np.testing.assert_array_equal(st.mask_of((b, m), np.arange(lo, hi)), brute_masks(strata, lo, hi))
    return b, m


@pytest.mark.parametrize("seed,n_strata", [(1, 1), (2, 3), (3, 8), (4, 32)])
def test_flatten_against_brute_force(seed, n_strata):
    check_table(random_strata(np.random.default_rng(seed), n_strata))


def test_flatten_literal_cases():
    # touching intervals of one stratum are one run; the BED off-by-one: (10, 20) holds 11 .. 20
    b, m = check_table([("a", [10, 20], [20, 30])])
    assert b.tolist() == [-(1 << 31), 11, 31] and m.tolist() == [0, 1, 0]
    # nested and overlapping
    b, m = check_table([("a", [10, 12, 15], [40, 14, 50])])
    assert b.tolist() == [-(1 << 31), 11, 51] and m.tolist() == [0, 1, 0]
    # two strata that change at the same position: (0, 5) ends where (5, 9) begins -- one breakpoint, no empty segment
    b, m = check_table([("a", [0], [5]), ("b", [5], [9])])
    assert b.tolist() == [-(1 << 31), 1, 6, 10] and m.tolist() == [0, 1, 2, 0]
    # equal neighbours merge across strata: b covers what a leaves and both are one mask only where they overlap
    b, m = check_table([("a", [0, 7], [4, 9]), ("a2", [4], [7])])
    assert m.tolist() == [0, 1, 2, 1, 0]
    # an interval ending at 2^31 - 1 never closes; pos < 1 and every negative int32 get mask 0
    b, m = st.flatten([("a", [100], [I32MAX]), ("b", [0], [I32MAX])])
    assert b.tolist() == [-(1 << 31), 1, 101] and m.tolist() == [0, 2, 3]
    probe = np.array([-(1 << 31), -1, 0, 1, 100, 101, I32MAX], np.int32)
    assert st.mask_of((b, m), probe).tolist() == [0, 0, 0, 2, 2, 3, 3]


# ---- the table writer -----------------------------------------------------------------------------------------------------
def test_write_performance_strata_hand_table(tmp_path):
    names = ["repeat", "UL74"]
    mixed = {"strata_rec": np.array([[4, 3, 1], [2000, 1, 1999], [5, 0, 5], [2, 1, 1]], np.uint64),
             "strata_tru": np.array([[6, 3], [0, 0], [4, 0]], np.uint64), "pure_strain": False}
    empty = {"strata_rec": np.zeros((4, 3), np.uint64), "strata_tru": np.array([[2, 0], [0, 0], [0, 0]], np.uint64)}
    pure = {"strata_rec": np.array([[3, 0, 3], [0, 0, 0], [1, 0, 1], [0, 0, 0]], np.uint64),
            "strata_tru": np.zeros((3, 2), np.uint64), "pure_strain": True}
    path = str(tmp_path / "t.tsv")
    st.write_performance_strata(path, [("lofreq", "TA-1-1", names, mixed), ("clc", "TA-1-10", names, empty), ("gatk", "TM-1-0", names, pure)])
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == ["caller", "mixture", "stratum", "genomediff", "calleridentify", "TP_lines", "FP_lines", "TP", "FN",
                                    "Precision", "Recall", "F1"]
    # P = 3/4, R = 3/6, F1 = 2 * .75 * .5 / 1.25 = 0.6
    assert lines[1] == "LoFreq\tTA-1-1\trepeat\t6\t4\t3\t1\t3\t3\t0.75\t0.5\t0.6"
    # genomediff 0: Recall NA (a zero denominator), and with it F1; the truth-side TP need not equal the TP lines
    assert lines[2] == "LoFreq\tTA-1-1\tUL74\t0\t2000\t1\t1999\t0\t0\t0\tNA\tNA"
    # P = 0 and R = 0: F1 has a zero denominator
    assert lines[3] == "LoFreq\tTA-1-1\toutside\t4\t5\t0\t5\t0\t4\t0\t0\tNA"
    assert lines[4] == "LoFreq\tTA-1-1\tnokey\tNA\t2\t1\t1\tNA\tNA\tNA\tNA\tNA"
    # nothing kept: Precision NA
    assert lines[5] == "CLC\tTA-1-10\trepeat\t2\t0\t0\t0\t0\t2\tNA\t0\tNA"
    # the pure-strain rows (caller_performance_compare.R:121-128): TP 0, Precision 0, the rest of the truth side NA
    assert lines[9] == "GATK\tTM-1-0\trepeat\tNA\t3\t0\t3\t0\tNA\t0\tNA\tNA"
    assert lines[12] == "GATK\tTM-1-0\tnokey\tNA\t0\t0\t0\tNA\tNA\tNA\tNA\tNA"
    assert lines[13] == "" and len(lines) == 14


def test_write_performance_strata_rounds_as_r(tmp_path):
    # 1 / 2000 = 0.0005, a tie at the third digit: the existing helper decides (R's long-double round), not Python's round()
    st_ = {"strata_rec": np.array([[2000, 1, 1999], [0, 0, 0], [0, 0, 0]], np.uint64), "strata_tru": np.array([[2000, 1], [0, 0]], np.uint64)}
    path = str(tmp_path / "t.tsv")
    st.write_performance_strata(path, [("x", "m", ["all"], st_)])
    row = open(path).read().split("\n")[1].split("\t")
    want = r_round3(1 / 2000)
    assert row[9] == row[10] == ("%.15g" % want)
    p = r_round3(1 / 2000)
    assert row[11] == "%.15g" % r_round3(2 * (p * p) / (p + p))
    # 9 / 16 = 0.5625 exactly: a true tie in binary, rounded half to even by nearbyint -> 0.562
    st_ = {"strata_rec": np.array([[16, 9, 7], [0, 0, 0], [0, 0, 0]], np.uint64), "strata_tru": np.array([[16, 9], [0, 0]], np.uint64)}
    st.write_performance_strata(path, [("x", "m", ["all"], st_)])
    assert open(path).read().split("\n")[1].split("\t")[9] == "0.562"


def test_write_custom_header(tmp_path):
    st_ = {"strata_rec": np.array([[4, 2, 2], [0, 0, 0], [0, 0, 0]], np.uint64), "strata_tru": np.array([[4, 2], [0, 0]], np.uint64),
           "pure_strain": True}   # the custom script has no pure-strain branch
    path = str(tmp_path / "t.txt")
    st.write_performance_strata(path, [("mycaller", None, ["all"], st_)], custom=True)
    lines = open(path).read().split("\n")
    assert lines[0].split("\t") == ["caller", "stratum", "genomediff", "calleridentify", "TP_lines", "FP_lines", "TP", "FN", "precision",
                                    "recall", "f1"]
    assert lines[1] == "mycaller\tall\t4\t4\t2\t2\t2\t2\t0.5\t0.5\t0.5"


# ---- the truth file's rows as R counts them --------------------------------------------------------------------------------
def test_truth_rows_counts_what_r_counts(tmp_path):
    strata = [("lo", [0], [100]), ("mid", [50], [200])]
    hcmv = _write(tmp_path, "t.vcf",
                  "##header\n#CHROM\tPOS\tID\tREF\tALT\n"
                  "c\t10\t.\tA\tC\n"        # lo
                  "c\t10\t.\tA\tC\n"        # the same key on a second row: R counts rows
                  "c\t60\t.\tG\tT\n"        # lo and mid
                  "c\t150\t.\tN\tA\n"       # not a single base: no part of genomediff in hcmv mode
                  "c\t150\t.\tAC\tA\n"
                  "c\t201\t.\tT\tA\n"       # outside
                  "c\t0150\t.\tT\tA\n"      # a POS the device holds no key for still has a place: mid
                  "c\tx7\t.\tT\tA\n")       # no number: outside
    assert st.truth_rows(hcmv, "hcmv", strata).tolist() == [3, 2, 2]
    custom = _write(tmp_path, "t.snps",
                    "10\tA\tC\t11\n"
                    "60\tN\tA\t61\n"        # R's filter is ref != "." and alt != ".": counted, although no device key
                    "70\ta\tg\t71\n"
                    "80\t.\tG\t81\n"        # an insertion: not counted
                    "90\tG\t.\t91\n"
                    "\n"
                    "300\tC\tT\t301\n")
    assert st.truth_rows(custom, "custom", strata).tolist() == [3, 2, 1]


def test_table_takes_genomediff_from_the_truth_rows(tmp_path):
    st_ = {"strata_rec": np.array([[4, 2, 2], [1, 1, 0], [0, 0, 0]], np.uint64), "strata_tru": np.array([[4, 2], [1, 1]], np.uint64),
           "strata_genomediff": np.array([5, 1])}      # one row of the stratum has no device key: it is a missed variant
    path = str(tmp_path / "t.tsv")
    st.write_performance_strata(path, [("x", "m", ["all"], st_)])
    lines = open(path).read().split("\n")
    assert lines[1] == "x\tm\tall\t5\t4\t2\t2\t2\t3\t0.5\t0.4\t0.444"
    assert lines[2] == "x\tm\toutside\t1\t1\t1\t0\t1\t0\t1\t1\t1"
