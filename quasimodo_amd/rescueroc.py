"""The QUAL ROC under normal-form and atom matching: the 256-threshold sweep of the batch's own ROC (DESIGN.md
2), with the hit of the normalisation pass (hitN, 4.17) or of the atomisation pass (hitA, 4.18) in place of the hit by spelling.

`sweep` is the restatement of what k_rroc_records / k_rroc_units compute (csrc/qmvt_rroc.hip), built on the definitions of
quasimodo_amd.normalize (forms, the truth order) and quasimodo_amd.atomize (atoms, the atom set); everything is integers, the
device is compared with it exactly.  `operating_point`, `best_f1` and `write_caller_roc_rescue` make final_tables/
caller_roc_rescue.tsv; the three ROC files per job go through tables.write_rescue_roc.
"""
import math
import os

import numpy as np

from . import atomize as A
from . import normalize as N

F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8
NORM, ATOM = 1, 2                 # include/qmvt.h QM_RROC_NORM, QM_RROC_ATOM
MATCHINGS = ("spelling", "normalized", "atomized")
FIXED_T = 20                      # the filter the passes themselves report at: QUAL >= 20


def qual_bin(q, n_bins):
    """the QUAL bin of the batch's own ROC on a float32: floor(q) clamped to n_bins - 1; NaN and q < 0 give -1"""
    q = float(np.float32(q))
    if q != q or q < 0:
        return -1
    if q >= n_bins:
        return n_bins - 1
    return int(math.floor(q))


def _valid(c):
    c = int(c)
    return 0 <= c < 4 or c >= 0x08000000


def _suffix(hist):
    return np.cumsum(hist[:, ::-1], axis=1, dtype=np.uint64)[:, ::-1].copy()


def sweep_norm(genome, truth, pos, ref, alt, qual, flags, n_bins=256, detail=None):
    """(roc_n uint64 [3][n_bins] -- suffix sums TP(t), FP(t), U(t) --, base: the distinct forms) of one VCF.  genome None: the VCF
    names none, zero rows and a zero baseline.  detail: a dict that receives best {form: bin}"""
    hist = np.zeros((3, n_bins), np.uint64)
    if genome is None:
        return hist, 0
    forms, _ = N.truth_forms(genome, *truth)
    best, memo = {}, {}
    for i in range(len(pos)):
        b = qual_bin(qual[i], n_bins)
        if b < 0 or not (_valid(ref[i]) and _valid(alt[i])):
            continue
        f = int(flags[i])
        key = (int(pos[i]), int(ref[i]), int(alt[i]), bool(f & F_NOKEY))
        if key not in memo:                        # (callers repeat each other: one normalisation per distinct line)
            memo[key] = N.form_codes(genome, *key)[1:]
        form = memo[key]
        hit = not f & F_NOKEY and form in forms
        if (hit and f & F_IDDOT) or f & F_TPLINE:
            hist[0, b] += 1
        else:
            hist[1, b] += 1
        if hit and f & F_IDDOT:
            best[form] = max(best.get(form, -1), b)
    for b in best.values():
        hist[2, b] += 1
    if detail is not None:
        detail["best"] = best
        detail["rows"] = {form: v[0] for form, v in forms.items()}
    return _suffix(hist), len(forms)


def sweep_atom(truth, pos, ref, alt, qual, flags, n_bins=256, detail=None):
    """(roc_a uint64 [3][n_bins], base: the allele-extended entries) of one VCF.  detail: a dict that receives best_atom {atom:
    bin}, best_entry {entry index: bin} -- raised by EVERY carrier spelled like the entry, atomisable or not -- and best {entry
    index: bin}, what the sweep counts"""
    hist = np.zeros((3, n_bins), np.uint64)
    ent, per, aset = A.truth_atoms(*truth)
    index = {e: j for j, e in enumerate(ent)}
    best_atom, best_entry, memo = {}, {}, {}
    for i in range(len(pos)):
        b = qual_bin(qual[i], n_bins)
        if b < 0 or not (_valid(ref[i]) and _valid(alt[i])):
            continue
        f = int(flags[i])
        nokey = bool(f & F_NOKEY)
        key = (int(pos[i]), int(ref[i]), int(alt[i]), nokey)
        if key not in memo:
            memo[key] = A.atoms_codes(*key)
        why, at = memo[key]
        e = None if nokey else index.get((int(pos[i]), int(ref[i]), int(alt[i])))
        if why is None:
            hits = [key for _, key in at if key in aset]
            hit = len(hits) == len(at)
        else:
            hits, hit = [], e is not None
        if (hit and f & F_IDDOT) or f & F_TPLINE:
            hist[0, b] += 1
        else:
            hist[1, b] += 1
        if f & F_IDDOT and not nokey:      # a carrier
            for key in hits:
                best_atom[key] = max(best_atom.get(key, -1), b)
            if e is not None:
                best_entry[e] = max(best_entry.get(e, -1), b)
    best = {}
    for j, atoms in enumerate(per):
        if atoms is None:
            if j in best_entry:
                best[j] = best_entry[j]
        elif all(key in best_atom for key in atoms):
            best[j] = min(best_atom[key] for key in atoms)
    for b in best.values():
        hist[2, b] += 1
    if detail is not None:
        detail.update(best_atom=best_atom, best_entry=best_entry, best=best, per=per)
    return _suffix(hist), len(ent)


def sweep(genome, truth, pos, ref, alt, qual, flags, n_bins=256):
    """(roc_n, roc_a, base [2]) of one VCF: what Batch.rescue_roc returns for it"""
    rn, bn = sweep_norm(genome, truth, pos, ref, alt, qual, flags, n_bins)
    ra, ba = sweep_atom(truth, pos, ref, alt, qual, flags, n_bins)
    return rn, ra, np.array([bn, ba], np.uint64)


# ---- final_tables/caller_roc_rescue.tsv -------------------------------------------------------------------------------
TABLE_HEADER = (("caller", "mixture", "matching"),
                ("TP", "FP", "FN", "Precision", "Recall", "F1", "best_t", "TP_best", "FP_best", "FN_best", "Precision_best", "Recall_best",
                 "F1_best"))


def operating_point(roc, base, t):
    """[TP, FP, FN, Precision, Recall, F1] at threshold t: the call side counts lines (TP(t) out of TP(t) + FP(t)), the truth
    side counts units (U(t) out of the baseline); R's round(x, 3) as in the other tables; None = NA (no line at the threshold)."""
    from .tables import r_div, r_round3
    n_bins = roc.shape[1]
    tp, fp, u = (int(roc[k, t]) if t < n_bins else 0 for k in range(3))
    base = int(base)
    if tp + fp == 0:
        return [0, 0, base - u, None, None, None]
    p, r = r_round3(r_div(tp, tp + fp)), r_round3(r_div(u, base))
    return [tp, fp, base - u, p, r, r_round3(r_div(2 * (p * r), p + r))]


def best_f1(roc, base):
    """(t, operating point) of the largest F1 over all thresholds; ties go to the smallest t; (None, NA row) where no threshold
    has a finite F1"""
    best_t, best_row = None, None
    for t in range(roc.shape[1]):
        row = operating_point(roc, base, t)
        f1 = row[5]
        if f1 is None or math.isnan(f1) or math.isinf(f1):
            continue
        if best_row is None or f1 > best_row[5]:
            best_t, best_row = t, row
    if best_row is None:
        return None, [0, 0, int(base) - 0, None, None, None]
    return best_t, best_row


def table_row(roc, base):
    t, row = best_f1(roc, base)
    return operating_point(roc, base, FIXED_T) + [t] + row


def write_caller_roc_rescue(path, rows):
    """final_tables/caller_roc_rescue.tsv.  rows: iterable of (caller_lower, sample, stats) with stats["rroc"] = {matching: (roc
    [3][n_bins], base)} over MATCHINGS; jobs without it (pure-strain samples) are left out.  One row per caller, mixture and
    matching, then a pooled block per caller (mixture "pooled": the rows and the baselines of its mixtures added up).  Written
    atomically."""
    from .tables import CALLER_MAP, r_str
    lines = ["\t".join(TABLE_HEADER[0] + TABLE_HEADER[1])]
    pooled, order = {}, []
    for caller, sample, stats in rows:
        if "rroc" not in stats:
            continue
        for m in MATCHINGS:
            roc, base = stats["rroc"][m]
            roc = np.asarray(roc, np.uint64)
            lines.append("\t".join([CALLER_MAP.get(caller, caller), sample, m] + [r_str(v) for v in table_row(roc, base)]))
            if (caller, m) not in pooled:
                pooled[(caller, m)] = [np.zeros_like(roc), 0]
                if caller not in order:
                    order.append(caller)
            pooled[(caller, m)][0] += roc
            pooled[(caller, m)][1] += int(base)
    for caller in order:
        for m in MATCHINGS:
            roc, base = pooled[(caller, m)]
            lines.append("\t".join([CALLER_MAP.get(caller, caller), "pooled", m] + [r_str(v) for v in table_row(roc, base)]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
