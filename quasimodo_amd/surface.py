"""The filter surface: TP, FP and FN of a caller under every filter QUAL >= q AND AF >= a of a threshold grid, the
cell of the largest F1 and the writers of the per-sample surface table and final_tables/caller_best_filter.tsv.  The counts come
from the engine (qm_batch_surface); nothing here counts a record."""
import os

from .tables import CALLER_MAP

DEFAULTS = {"q_step": 4, "nq": 64, "na": 50}     # QUAL 0 .. 252 in steps of 4 (20 is a grid line), AF in steps of 0.02
DEFAULT_QUAL = 20                                # the reference's hard-wired filter: QUAL >= 20, any AF
TP, FP, U = 0, 1, 2                              # include/qmvt.h QM_SF_*: the first axis of S
COUNTED, NO_AF, NO_BIN, TRUTH = 0, 1, 2, 3       # ... and the entries of extra
HEADER = ("qual_min", "af_min", "true_positives_baseline", "false_positives", "true_positives_call", "false_negatives",
          "precision", "sensitivity", "f_measure")
BEST_HEADER = ("caller", "mixture", "best_qual_min", "best_af_min") + tuple("best_" + h for h in HEADER[2:]) + \
              tuple("default_" + h for h in HEADER[2:]) + ("records_without_af",)


def params(q_step=None, nq=None, na=None):
    """(q_step, nq, na) as ints, the defaults for None; ValueError names the argument outside its limits"""
    from .engine import surface_params
    return surface_params(*(DEFAULTS[k] if v is None else v for k, v in (("q_step", q_step), ("nq", nq), ("na", na))))


def workflow_params(q_step=None, nq=None, na=None):
    """params() for the workflows: the default filter QUAL >= 20 must be a grid line inside the grid"""
    q, n, a = params(q_step, nq, na)
    if DEFAULT_QUAL % q or n * q <= DEFAULT_QUAL:
        raise ValueError("surface: QUAL %d must be a grid line (q_step %d must divide it, nq * q_step = %d must exceed it)" % (DEFAULT_QUAL, q, n * q))
    return q, n, a


def surface_path(job):
    """a job's surface table beside fp/ and tp/: surface/<x>.surface.tsv"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "surface", base[:-len(".fp.vcf")] + ".surface.tsv")


def cell_numbers(S, truth_unique, i, k):
    """the six numbers of cell (i, k) as tables.write_weighted_roc computes them: (TP_baseline, FP, TP_call, FN, precision,
    sensitivity, F1); a cell with no call is all zeros"""
    tp_call, fp, tp_base = int(S[TP][i][k]), int(S[FP][i][k]), int(S[U][i][k])
    if tp_call + fp == 0:
        return 0, 0, 0, 0, 0.0, 0.0, 0.0
    t = int(truth_unique)
    prec = tp_call / (tp_call + fp)
    sens = tp_base / t if t else 0.0
    f1 = 2 * prec * sens / (prec + sens) if prec + sens > 0 else 0.0
    return tp_base, fp, tp_call, t - tp_base, prec, sens, f1


def _fmt(nums):
    return "%d\t%d\t%d\t%d\t%.4f\t%.4f\t%.4f" % tuple(nums)


def surface_rows(S, truth_unique, q_step):
    """the table's lines: the header, then one row per cell, QUAL ascending then AF ascending (af_min = k / na); cells with no
    call are written with zeros, so the grid stays rectangular"""
    nq, na = len(S[TP]), len(S[TP][0])
    lines = ["\t".join(HEADER)]
    for i in range(nq):
        for k in range(na):
            lines.append("%d\t%.4f\t%s" % (i * q_step, k / na, _fmt(cell_numbers(S, truth_unique, i, k))))
    return lines


def write_surface(path, S, truth_unique, q_step):
    """one job's surface table, written atomically"""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(surface_rows(S, truth_unique, q_step)) + "\n")
    os.replace(tmp, path)


def best_cell(S, truth_unique):
    """(i, k) of the cell of largest F1, or None when no cell holds a call.  F1 = 2 TPc U / (TPc T' + U (TPc + FP)) is compared
    as a fraction of Python integers (no rounding decides); cells with TPc + FP == 0 are skipped; ties go to the smaller
    qual_min, then the smaller af_min."""
    t = int(truth_unique)
    best, bn, bd = None, 0, 1
    for i in range(len(S[TP])):
        for k in range(len(S[TP][0])):
            tpc, fp, u = int(S[TP][i][k]), int(S[FP][i][k]), int(S[U][i][k])
            if tpc + fp == 0:
                continue
            num, den = 2 * tpc * u, tpc * t + u * (tpc + fp)
            if den == 0:
                num, den = 0, 1
            if best is None or num * bd > bn * den:   # strictly larger only: the first cell in (qual, af) order keeps a tie
                best, bn, bd = (i, k), num, den
    return best


def pooled(surfaces):
    """the cell-wise sums of several (S, T') pairs of one grid shape: (S, T') of the pooled sample"""
    surfaces = list(surfaces)
    S0 = surfaces[0][0]
    out = [[[sum(int(S[c][i][k]) for S, _ in surfaces) for k in range(len(S0[c][0]))] for i in range(len(S0[c]))] for c in range(3)]
    return out, sum(int(t) for _, t in surfaces)


def best_filter_rows(entries, q_step):
    """the rows of caller_best_filter.tsv.  entries: (caller_lower, sample, S, extra) in the order of caller_performance.tsv;
    behind the rows of every caller comes its `pooled` row, the same rule on the cell-wise sums over its samples."""
    rows, callers = [], []
    for c, *_ in entries:
        if c not in callers:
            callers.append(c)

    def row(caller, sample, S, t, no_af):
        na = len(S[TP][0])
        b = best_cell(S, t)
        bi, bk = b if b is not None else (0, 0)
        return "%s\t%s\t%d\t%.4f\t%s\t%s\t%d" % (CALLER_MAP.get(caller, caller), sample, bi * q_step, bk / na, _fmt(cell_numbers(S, t, bi, bk)),
                                                 _fmt(cell_numbers(S, t, DEFAULT_QUAL // q_step, 0)), no_af)
    for c in callers:
        mine = [(s, S, ex) for cc, s, S, ex in entries if cc == c]
        for s, S, ex in mine:
            rows.append(row(c, s, S, int(ex[TRUTH]), int(ex[NO_AF])))
        pS, pT = pooled((S, int(ex[TRUTH])) for _, S, ex in mine)
        rows.append(row(c, "pooled", pS, pT, sum(int(ex[NO_AF]) for _, _, ex in mine)))
    return rows


def write_caller_best_filter(path, entries, q_step):
    """final_tables/caller_best_filter.tsv: per caller x mixed sample and per caller pooled, the cell of largest F1 with its six
    numbers, the same numbers at (QUAL >= 20, AF >= 0) and the counted records without AF.  Written atomically."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(["\t".join(BEST_HEADER)] + best_filter_rows(entries, q_step)) + "\n")
    os.replace(tmp, path)
