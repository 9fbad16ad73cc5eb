"""Paired block-bootstrap confidence intervals for caller performance.

The genome is cut into `n_win` windows of `window` positions; a replicate draws `n_win` windows with replacement and sums the
windows' counts with the multiplicities of the draw.  The draws come from a counter-based hash of (seed, replicate, n_win)
alone, so every VCF -- on every batch, rank and device -- is resampled with the same windows and the difference between two
callers on one sample has an interval of its own.

`draws` / `multiplicities` restate the hash of include/qmvt.h (qm_boot_draws) in numpy uint64; `interval` is the percentile
interval; the writers need no device."""
import os

import numpy as np

from .tables import CALLER_MAP, r_round3, r_str

MAX_WINDOWS = 4096                # include/qmvt.h QM_BOOT_MAX_WINDOWS
MAX_REP = 16384                   # QM_BOOT_MAX_REP
DEFAULTS = {"window": 1024, "n_win": 256, "n_rep": 1000, "seed": 0}
KEPT, TP_LINES, TRUTH_KEYS, HIT_KEYS = 0, 1, 2, 3   # the columns of boot_cnt / boot_rep
_M64 = (1 << 64) - 1


def mix64(x):
    """the splitmix64 finaliser on uint64 arrays (wrapping arithmetic)"""
    x = np.asarray(x, np.uint64)
    with np.errstate(over="ignore"):
        z = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draws(seed, n_win, n_rep):
    """int64 [n_rep][n_win]: idx(b, j), the window that draw j of replicate b takes"""
    n_win, n_rep = int(n_win), int(n_rep)
    if not 1 <= n_win <= MAX_WINDOWS or not 0 <= n_rep <= MAX_REP:
        raise ValueError("n_win %d (1 to %d), n_rep %d (0 to %d)" % (n_win, MAX_WINDOWS, n_rep, MAX_REP))
    ctr = (np.arange(n_rep, dtype=np.uint64)[:, None] * np.uint64(n_win) + np.arange(n_win, dtype=np.uint64)[None, :] + np.uint64(1))
    with np.errstate(over="ignore"):
        x = np.uint64(int(seed) & _M64) + np.uint64(0x9E3779B97F4A7C15) * ctr
        z = mix64(x)
        return (((z >> np.uint64(32)) * np.uint64(n_win)) >> np.uint64(32)).astype(np.int64)


def multiplicities(seed, n_win, n_rep):
    """int64 [n_rep][n_win]: mult[b][w] = how often replicate b draws window w; every row sums to n_win"""
    d = draws(seed, n_win, n_rep)
    out = np.zeros((int(n_rep), int(n_win)), np.int64)
    for b in range(d.shape[0]):
        out[b] = np.bincount(d[b], minlength=int(n_win))
    return out


def windows_for(max_pos, window, n_win=DEFAULTS["n_win"]):
    """n_win raised to cover position max_pos, up to MAX_WINDOWS; ValueError (asking for a larger window) beyond"""
    need = max(int(n_win), (max(int(max_pos), 1) - 1) // int(window) + 1)
    if need > MAX_WINDOWS:
        raise ValueError("position %d needs %d windows of %d positions (at most %d): choose a larger window (--bootstrap-window), "
                         "at least %d" % (max_pos, need, window, MAX_WINDOWS, (max(int(max_pos), 1) - 1) // MAX_WINDOWS + 1))
    return need


def truth_row_windows(path, mode, window, n_win):
    """int64 [n_win + 1]: the rows of a truth file that R counts as `genomediff` (strata.truth_rows), per window and then
    `outside`, by the row's POS: position p >= 1 with (p - 1) // window < n_win lies in window (p - 1) // window."""
    from .strata import truth_row_positions
    pos, unplaced = truth_row_positions(path, mode)
    out = np.zeros(int(n_win) + 1, np.int64)
    out[n_win] = unplaced
    p = np.array(pos, np.int64)
    w = (p - 1) // int(window)
    inside = (p >= 1) & (w < int(n_win))
    out[:n_win] += np.bincount(w[inside], minlength=int(n_win))
    out[n_win] += int((~inside).sum())
    return out


def truth_max_pos(path, mode):
    """the largest POS among the rows truth_row_windows places (0 when there is none)"""
    from .strata import truth_row_positions
    pos, _ = truth_row_positions(path, mode)
    return max(pos) if pos else 0


def interval(values, level_pm=950):
    """The percentile interval of the valid replicates: None and NaN entries are dropped, the n others sorted ascending;
    k = (n * (1000 - level_pm)) // 2000; the bounds are v[k] and v[n - 1 - k].  (None, None) when n = 0."""
    v = sorted(float(x) for x in values if x is not None and x == x)
    n = len(v)
    if n == 0:
        return None, None
    k = (n * (1000 - int(level_pm))) // 2000
    return v[k], v[n - 1 - k]


def _ratios(tp, n, gd):
    """unrounded (p, r, f1) of integer arrays, NaN where the denominator is zero (for F1 also where p + r = 0)"""
    tp, n, gd = (np.asarray(x, np.float64) for x in (tp, n, gd))
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(n > 0, tp / n, np.nan)
        r = np.where(gd > 0, tp / gd, np.nan)
        f = np.where((p + r) > 0, 2 * (p * r) / (p + r), np.nan)
    return p, r, f


def replicates(stats, mult):
    """One VCF's replicates: (calleridentify, TP, genomediff) int64 [n_rep] each.  stats holds boot_rep [n_rep][4] and,
    optionally, boot_extra [n_win + 1] (the truth file's rows minus the device's distinct keys per window, then outside): the
    replicate's genomediff is rep[b][2] + sum_w mult[b][w] * extra[w] + extra[outside]."""
    rep = np.asarray(stats["boot_rep"]).astype(np.int64).reshape(-1, 4)
    gd = rep[:, TRUTH_KEYS].copy()
    extra = stats.get("boot_extra")
    if extra is not None:
        extra = np.asarray(extra, np.int64)
        gd += np.asarray(mult, np.int64)[:rep.shape[0]] @ extra[:-1] + extra[-1]
    return rep[:, KEPT], rep[:, HIT_KEYS], gd


def point(stats):
    """One VCF's point counts (calleridentify, TP, genomediff): the sums of boot_cnt over the windows, outside and nokey, plus
    the truth file's extra rows -- a replicate with every multiplicity 1."""
    cnt = np.asarray(stats["boot_cnt"]).astype(np.int64)
    extra = stats.get("boot_extra")
    return int(cnt[:, KEPT].sum()), int(cnt[:, HIT_KEYS].sum()), int(cnt[:, TRUTH_KEYS].sum()) + (0 if extra is None else int(np.asarray(extra, np.int64).sum()))


def _point_ratios(n, tp, gd):
    """Precision, Recall, F1 as strata.strata_rows writes them (rounded ratios, F1 of the rounded two); None = NA"""
    p = None if n == 0 else r_round3(float(tp) / float(n))
    r = None if gd == 0 else r_round3(float(tp) / float(gd))
    f1 = None if p is None or r is None or p + r == 0 else r_round3(2 * (p * r) / (p + r))
    return p, r, f1


def ci_row(stats, mult, pure=False, level_pm=950):
    """(genomediff, calleridentify, TP, P, P_lo, P_hi, R, R_lo, R_hi, F1, F1_lo, F1_hi, n_valid) of one VCF; None = NA.
    The point columns follow strata.strata_rows; the bounds are `interval` over the unrounded replicate ratios, rounded on
    output.  n_valid counts the replicates with a valid F1 (calleridentify > 0, genomediff > 0, Precision + Recall > 0).
    A pure-strain sample (caller_performance_compare.R:121-128): genomediff 0, TP 0, Precision 0, the rest NA.
    Without a truth side (the allele-extended mode, boot_truth false): everything but calleridentify NA."""
    n, tp, gd = point(stats)
    if pure:
        return (0, n, 0, 0.0, None, None, None, None, None, None, None, None, 0)
    if not stats.get("boot_truth", True):
        return (None, n, None) + (None,) * 9 + (0,)
    rn, rtp, rgd = replicates(stats, mult)
    p, r, f = _ratios(rtp, rn, rgd)
    out = [gd, n, tp]
    for pt, vals in zip(_point_ratios(n, tp, gd), (p, r, f)):
        lo, hi = interval(vals, level_pm)
        out += [pt, r_round3(lo), r_round3(hi)]
    return tuple(out) + (int(np.count_nonzero(f == f)),)


def pair_row(stats_a, stats_b, mult, level_pm=950):
    """(dF1, dF1_lo, dF1_hi, n_valid) of two VCFs of one sample: the difference of the unrounded point F1s, and `interval` over
    the replicate-by-replicate differences of the replicates in which both F1s are valid."""
    (na, ta, ga), (nb, tb, gb) = point(stats_a), point(stats_b)
    fa, fb = _ratios([ta], [na], [ga])[2][0], _ratios([tb], [nb], [gb])[2][0]
    d = None if fa != fa or fb != fb else r_round3(float(fa - fb))
    (na, ta, ga), (nb, tb, gb) = replicates(stats_a, mult), replicates(stats_b, mult)
    diff = _ratios(ta, na, ga)[2] - _ratios(tb, nb, gb)[2]   # NaN where either is
    lo, hi = interval(diff, level_pm)
    return d, r_round3(lo), r_round3(hi), int(np.count_nonzero(diff == diff))


def _params(rows):
    for _, _, stats in rows:
        if "boot_params" in stats:
            return stats["boot_params"]
    return dict(DEFAULTS)


def write_performance_ci(path, rows, custom=False, level_pm=950):
    """rows: iterable of (caller_lower, sample, stats) -- stats holds boot_cnt, boot_rep, boot_params (window, n_win, n_rep,
    seed), pure_strain and, optionally, boot_extra and boot_truth.  final_tables/caller_performance_ci.tsv; custom=True:
    snpcall_benchmark_ci.txt (no mixture column, the custom table's header spelling, no pure-strain branch)."""
    rows = list(rows)
    prm = _params(rows)
    mult = multiplicities(prm["seed"], prm["n_win"], prm["n_rep"])
    names = ("precision", "recall", "f1") if custom else ("Precision", "Recall", "F1")
    head = (["caller"] if custom else ["caller", "mixture"]) + ["genomediff", "calleridentify", "TP"]
    for nm in names:
        head += [nm, nm + "_lo", nm + "_hi"]
    head += ["n_rep", "n_valid", "window", "n_win", "seed"]
    with open(path, "w") as fh:
        fh.write("\t".join(head) + "\n")
        for caller, sample, stats in rows:
            lead = [caller] if custom else [CALLER_MAP.get(caller, caller), sample]
            vals = ci_row(stats, mult, bool(stats.get("pure_strain")) and not custom, level_pm)
            tail = [int(prm["n_rep"]), vals[-1], int(prm["window"]), int(prm["n_win"]), int(prm["seed"])]
            fh.write("\t".join(lead + [r_str(v) for v in vals[:-1]] + [r_str(v) for v in tail]) + "\n")


def write_performance_ci_pairs(path, rows, level_pm=950):
    """final_tables/caller_performance_ci_pairs.tsv: per mixed sample and unordered pair of its callers (in the rows' order)
    dF1 = F1(caller_a) - F1(caller_b) with its interval over the shared draws."""
    rows = [r for r in rows if not r[2].get("pure_strain") and r[2].get("boot_truth", True)]
    prm = _params(rows)
    mult = multiplicities(prm["seed"], prm["n_win"], prm["n_rep"])
    by = {}
    for caller, sample, stats in rows:
        by.setdefault(sample, []).append((caller, stats))
    with open(path, "w") as fh:
        fh.write("\t".join(["mixture", "caller_a", "caller_b", "dF1", "dF1_lo", "dF1_hi", "n_rep", "n_valid"]) + "\n")
        for sample, members in by.items():
            for i in range(len(members)):
                for k in range(i + 1, len(members)):
                    d, lo, hi, nv = pair_row(members[i][1], members[k][1], mult, level_pm)
                    fh.write("\t".join([sample, CALLER_MAP.get(members[i][0], members[i][0]), CALLER_MAP.get(members[k][0], members[k][0])]
                                       + [r_str(x) for x in (d, lo, hi, int(prm["n_rep"]), nv)]) + "\n")
