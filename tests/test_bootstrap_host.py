"""The host side of the paired block bootstrap (quasimodo_amd.bootstrap): the hash of the draws against pinned
literals and a plain-Python-int restatement, the percentile interval at hand-derived indices, the windowed truth rows against
strata.truth_rows, and the table writers on a three-window case worked out by hand."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from quasimodo_amd import bootstrap as bs
from quasimodo_amd import strata as st

M64 = (1 << 64) - 1
I32MAX = (1 << 31) - 1


def mix_int(x):
    z = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws_int(seed, n_win, n_rep):
    """the hash of include/qmvt.h with Python integers"""
    return [[((mix_int((seed + 0x9E3779B97F4A7C15 * (b * n_win + j + 1)) & M64) >> 32) * n_win) >> 32 for j in range(n_win)] for b in range(n_rep)]


def test_pinned_hash_and_draws():
    assert mix_int(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert int(bs.mix64(np.uint64(0x9E3779B97F4A7C15))) == 0xE220A8397B1DCDAF
    d = bs.draws(0, 8, 2)
    assert d.tolist() == [[7, 3, 0, 7, 0, 2, 1, 6], [1, 7, 3, 6, 4, 4, 5, 4]] == draws_int(0, 8, 2)
    assert bs.multiplicities(0, 8, 2).tolist() == [[2, 1, 1, 1, 0, 0, 1, 2], [0, 1, 0, 1, 3, 1, 1, 1]]
    d = bs.draws(2024, 236, 3)
    assert d[0, :8].tolist() == [146, 22, 70, 27, 196, 130, 32, 140]
    assert d[1, :8].tolist() == [148, 182, 125, 231, 57, 161, 54, 106]
    assert d[2, :4].tolist() == [168, 207, 136, 125]
    assert d.tolist() == draws_int(2024, 236, 3)


@pytest.mark.parametrize("seed", [0, 1, 2024, M64, 1 << 63])
def test_draws_equal_the_integer_restatement(seed):
    for n_win, n_rep in ((1, 3), (2, 5), (8, 4), (236, 3), (4096, 2)):
        d = bs.draws(seed, n_win, n_rep)
        assert d.shape == (n_rep, n_win) and d.min() >= 0 and d.max() < n_win
        assert d.tolist() == draws_int(seed, n_win, n_rep), (seed, n_win)


@pytest.mark.parametrize("n_win", [1, 2, 8, 236, 4096])
def test_every_multiplicity_row_sums_to_n_win(n_win):
    m = bs.multiplicities(7, n_win, 5)
    assert m.shape == (5, n_win) and (m.sum(axis=1) == n_win).all() and m.min() >= 0
    assert bs.multiplicities(7, n_win, 0).shape == (0, n_win)


def test_draws_refuse_bad_shapes():
    for n_win, n_rep in ((0, 1), (4097, 1), (8, -1), (8, 16385)):
        with pytest.raises(ValueError):
            bs.draws(0, n_win, n_rep)


def test_interval_indices():
    """k = (n * 50) // 2000: n = 0, 1, 2, 39 -> 0; 40 -> 1; 1000 -> 25"""
    assert bs.interval([]) == (None, None)
    assert bs.interval([0.25]) == (0.25, 0.25)
    assert bs.interval([0.5, 0.25]) == (0.25, 0.5)
    v39 = [float(i) for i in range(39)]
    assert bs.interval(v39[::-1]) == (0.0, 38.0)
    v40 = [float(i) for i in range(40)]
    assert bs.interval(v40[::-1]) == (1.0, 38.0)
    v1000 = [float((i * 617) % 1000) for i in range(1000)]     # a permutation of 0 .. 999
    assert sorted(v1000) == [float(i) for i in range(1000)]
    assert bs.interval(v1000) == (25.0, 974.0)
    assert bs.interval(v1000, level_pm=900) == (50.0, 949.0)
    assert bs.interval(v1000, level_pm=1000) == (0.0, 999.0)


def test_interval_ties_and_none():
    assert bs.interval([0.5] * 100) == (0.5, 0.5)
    assert bs.interval([1.0] * 30 + [0.0] * 10) == (0.0, 1.0)          # n = 40, k = 1: v[1] = 0, v[38] = 1
    assert bs.interval([1.0] * 39 + [0.0]) == (1.0, 1.0)               # the single 0 is cut at k = 1
    assert bs.interval([None, 0.5, float("nan"), None, 0.25]) == (0.25, 0.5)
    assert bs.interval([None, float("nan")]) == (None, None)
    vals = [None] * 5 + [float(i) for i in range(40)]                   # the dropped entries do not count towards n
    assert bs.interval(vals) == (1.0, 38.0)


HCMV_TRUTHS = [os.path.join(GOLDEN, "hcmv", "input", "nucmer", "%s.maskrepeat.variants.vcf" % m) for m in ("TM", "TA")]
CUSTOM_TRUTH = os.path.join(GOLDEN, "custom", "input", "nucmer", "Merlin.BAC_TB40E.GFP.maskrepeat.snps")
ALL = [("all", [0], [I32MAX])]


@pytest.mark.parametrize("window,n_win", [(1024, 256), (1024, 100), (7, 2), (1, 1), (100000, 4096)])
def test_truth_row_windows_against_truth_rows(window, n_win):
    for path, mode in [(p, "hcmv") for p in HCMV_TRUTHS] + [(CUSTOM_TRUTH, "custom")]:
        rows = bs.truth_row_windows(path, mode, window, n_win)
        assert rows.shape == (n_win + 1,) and rows.dtype == np.int64
        assert int(rows.sum()) == int(st.truth_rows(path, mode, ALL).sum())
        pos, unplaced = st.truth_row_positions(path, mode)
        want = np.zeros(n_win + 1, np.int64)
        for p in pos:                                             # the definition, position by position
            w = (p - 1) // window
            want[w if p >= 1 and w < n_win else n_win] += 1
        want[n_win] += unplaced
        assert rows.tolist() == want.tolist()
        # a partitioning strata set over the same windows gives the same rows
        if 1 < n_win <= 32 - 1:
            part = [("w%d" % w, [w * window], [(w + 1) * window]) for w in range(n_win)]
            assert st.truth_rows(path, mode, part).tolist() == rows.tolist()


def test_custom_truth_has_302_rows_against_300_keys():
    from quasimodo_amd.vcfio import scan_truth
    rows = bs.truth_row_windows(CUSTOM_TRUTH, "custom", 1024, 256)
    assert int(rows.sum()) == 302
    t = scan_truth(open(CUSTOM_TRUTH, "rb").read(), custom=True)
    assert t.genomediff == 302
    p, r, a = (np.asarray(x, np.int64) for x in (t.pos, t.ref, t.alt))
    ok = (r >= 0) & (r < 4) & (a >= 0) & (a < 4)
    assert np.unique((p[ok] << 4) | (r[ok] << 2) | a[ok]).shape[0] == 300
    assert bs.truth_max_pos(CUSTOM_TRUTH, "custom") == max(st.truth_row_positions(CUSTOM_TRUTH, "custom")[0])


def test_windows_for():
    assert bs.windows_for(0, 1024) == 256
    assert bs.windows_for(236000, 1024) == 256
    assert bs.windows_for(262144, 1024) == 256 and bs.windows_for(262145, 1024) == 257
    assert bs.windows_for(4096 * 1024, 1024) == 4096
    with pytest.raises(ValueError, match="larger window"):
        bs.windows_for(4096 * 1024 + 1, 1024)


# ---- the writers: three windows, n_rep = 4, worked out by hand -------------------------------------------------------------
# seed 0, n_win 3: the multiplicities are computed by the integer restatement and then used as plain numbers below
def _hand():
    mult = np.array([[d.count(w) for w in range(3)] for d in draws_int(0, 3, 4)], np.int64)
    assert (mult.sum(axis=1) == 3).all()
    # caller A: kept lines only in window 0, so a replicate that never draws window 0 has calleridentify 0
    cnt_a = np.array([[4, 3, 5, 3], [0, 0, 2, 0], [0, 0, 3, 0], [0, 0, 1, 0], [0, 0, 0, 0]], np.uint64)   # windows, outside, nokey
    cnt_b = np.array([[2, 1, 5, 1], [3, 2, 2, 2], [1, 1, 3, 1], [1, 0, 1, 0], [2, 0, 0, 0]], np.uint64)
    extra = np.array([1, 0, 0, 1], np.int64)                           # rows minus keys: windows, outside
    def rep(cnt):
        return (mult @ cnt[:3].astype(np.int64) + cnt[3].astype(np.int64) + cnt[4].astype(np.int64)).astype(np.uint64)
    prm = {"window": 10, "n_win": 3, "n_rep": 4, "seed": 0}
    sa = {"boot_cnt": cnt_a, "boot_rep": rep(cnt_a), "boot_extra": extra, "boot_params": prm, "pure_strain": False}
    sb = {"boot_cnt": cnt_b, "boot_rep": rep(cnt_b), "boot_extra": extra, "boot_params": prm, "pure_strain": False}
    pure = {"boot_cnt": np.array([[2, 0, 0, 0], [1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], [1, 0, 0, 0]], np.uint64),
            "boot_params": prm, "pure_strain": True}
    pure["boot_rep"] = rep(pure["boot_cnt"])
    return mult, sa, sb, pure, extra


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]


def _f(x):
    from quasimodo_amd.tables import r_round3, r_str
    return r_str(r_round3(x))


def test_writers_on_a_hand_case(tmp_path):
    mult, sa, sb, pure, extra = _hand()
    zero = [b for b in range(4) if mult[b, 0] == 0]
    assert len(zero) >= 1, "the case needs a replicate that never draws window 0 (seed 0, n_win 3 has one)"
    path = tmp_path / "ci.tsv"
    bs.write_performance_ci(str(path), [("lofreq", "TM-1-10", sa), ("varscan", "TM-1-10", sb), ("lofreq", "TM-1-0", pure)])
    head, rows = _table(str(path))
    assert head == ["caller", "mixture", "genomediff", "calleridentify", "TP", "Precision", "Precision_lo", "Precision_hi", "Recall", "Recall_lo",
                    "Recall_hi", "F1", "F1_lo", "F1_hi", "n_rep", "n_valid", "window", "n_win", "seed"]
    a, b, p = rows
    # caller A by hand: calleridentify 4, TP 3 (hit keys), genomediff 11 keys + 2 extra rows = 13
    assert (a["caller"], a["mixture"], a["genomediff"], a["calleridentify"], a["TP"]) == ("LoFreq", "TM-1-10", "13", "4", "3")
    assert a["Precision"] == "0.75" and a["Recall"] == _f(3 / 13) == "0.231"
    assert a["F1"] == _f(2 * 0.75 * 0.231 / (0.75 + 0.231))           # F1 of the rounded two, as strata_rows writes it
    # per replicate: n = 4 m0, TP = 3 m0, genomediff = 5 m0 + 2 m1 + 3 m2 + 1 (outside) + m0 (extra of window 0) + 1 (extra outside)
    n = 4 * mult[:, 0]
    tp = 3 * mult[:, 0]
    gd = 6 * mult[:, 0] + 2 * mult[:, 1] + 3 * mult[:, 2] + 2
    valid = [i for i in range(4) if n[i] > 0]
    assert a["n_rep"] == "4" and a["n_valid"] == str(len(valid)) == str(4 - len(zero))
    assert a["Precision_lo"] == a["Precision_hi"] == "0.75"            # 3 m0 / 4 m0 in every valid replicate
    rec = sorted(tp[i] / gd[i] for i in range(4))                      # Recall is valid everywhere (0 where window 0 is not drawn)
    assert (a["Recall_lo"], a["Recall_hi"]) == (_f(rec[0]), _f(rec[3])) and a["Recall_lo"] == "0"
    f1 = sorted(2 * (0.75 * (tp[i] / gd[i])) / (0.75 + tp[i] / gd[i]) for i in valid)
    assert (a["F1_lo"], a["F1_hi"]) == (_f(f1[0]), _f(f1[-1]))
    assert (a["window"], a["n_win"], a["seed"]) == ("10", "3", "0")
    # caller B: nokey and outside enter every replicate once
    nb = 2 * mult[:, 0] + 3 * mult[:, 1] + 1 * mult[:, 2] + 1 + 2
    tb = 1 * mult[:, 0] + 2 * mult[:, 1] + 1 * mult[:, 2]
    assert (b["calleridentify"], b["TP"], b["genomediff"], b["n_valid"]) == ("9", "4", "13", "4")
    pb = sorted(tb[i] / nb[i] for i in range(4))
    assert (b["Precision_lo"], b["Precision_hi"]) == (_f(pb[0]), _f(pb[3]))
    # the pure-strain row (caller_performance_compare.R:121-128)
    assert [p[k] for k in head[2:14]] == ["0", "4", "0", "0", "NA", "NA", "NA", "NA", "NA", "NA", "NA", "NA"] and p["n_valid"] == "0"

    pairs = tmp_path / "pairs.tsv"
    bs.write_performance_ci_pairs(str(pairs), [("lofreq", "TM-1-10", sa), ("varscan", "TM-1-10", sb), ("lofreq", "TM-1-0", pure)])
    head, rows = _table(str(pairs))
    assert head == ["mixture", "caller_a", "caller_b", "dF1", "dF1_lo", "dF1_hi", "n_rep", "n_valid"]
    assert len(rows) == 1 and (rows[0]["mixture"], rows[0]["caller_a"], rows[0]["caller_b"]) == ("TM-1-10", "LoFreq", "VarScan2")
    def f1_of(t, n_, g):
        p_, r_ = t / n_, t / g
        return 2 * (p_ * r_) / (p_ + r_)
    assert rows[0]["dF1"] == _f(f1_of(3, 4, 13) - f1_of(4, 9, 13))     # the unrounded point F1s
    d = sorted(f1_of(tp[i], n[i], gd[i]) - f1_of(tb[i], nb[i], gd[i]) for i in valid)
    assert (rows[0]["dF1_lo"], rows[0]["dF1_hi"], rows[0]["n_valid"]) == (_f(d[0]), _f(d[-1]), str(len(valid)))

    custom = tmp_path / "ci.txt"
    bs.write_performance_ci(str(custom), [("lab", None, sa)], custom=True)
    head, rows = _table(str(custom))
    assert head[:6] == ["caller", "genomediff", "calleridentify", "TP", "precision", "precision_lo"] and "mixture" not in head
    assert rows[0]["caller"] == "lab" and rows[0]["f1_hi"] == a["F1_hi"]
