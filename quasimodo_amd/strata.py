"""BED strata: TP, FP and FN counts per genome region.

A stratum is (name, starts, ends): BED intervals, 0-based and half-open -- (start, end) holds the 1-based POS values p with
start < p <= end.  Intervals of one stratum may overlap or touch (the stratum is their union); strata may overlap each other,
so a position carries a membership mask of up to 32 bits.  The chrom column is read and ignored: the engine has no contig
column anywhere, only POS decides membership.

`flatten` is the pure-numpy restatement of the segment table qm_strata_load builds; the readers and the table writer need no
device."""
import os

import numpy as np

from .tables import CALLER_MAP, r_round3, r_str

MAX_STRATA = 32                   # include/qmvt.h QM_STRATA_MAX
MAX_SEGMENTS = 1 << 22            # QM_STRATA_MAX_SEGMENTS
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
OUTSIDE, NOKEY = "outside", "nokey"


def _check_interval(start, end, where):
    if start < 0:
        raise ValueError("%s: start %d is negative" % (where, start))
    if end <= start:
        raise ValueError("%s: end %d is not beyond start %d" % (where, end, start))
    if end > INT32_MAX:
        raise ValueError("%s: end %d is beyond 2^31 - 1" % (where, end))


def _bed_rows(path, min_cols):
    """(line number, columns) of every data line; both tabs and runs of blanks split columns"""
    with open(path, "rb") as fh:
        text = fh.read().decode("utf-8", "replace")
    for no, line in enumerate(text.split("\n"), 1):
        cols = line.split()
        if not cols or cols[0].startswith("#") or cols[0] in ("track", "browser"):
            continue
        if len(cols) < min_cols:
            raise ValueError("%s line %d: %d column(s), need %d" % (path, no, len(cols), min_cols))
        try:
            start, end = int(cols[1]), int(cols[2])
        except ValueError:
            raise ValueError("%s line %d: start / end %r %r are not integers" % (path, no, cols[1], cols[2])) from None
        _check_interval(start, end, "%s line %d" % (path, no))
        yield no, cols, start, end


def read_bed(path):
    """One stratum, named by the file's stem: (name, starts, ends)."""
    iv = [(s, e) for _, _, s, e in _bed_rows(path, 3)]
    name = os.path.basename(str(path))
    name = name[:name.rindex(".")] if "." in name[1:] else name
    return (name, np.array([s for s, _ in iv], np.int64), np.array([e for _, e in iv], np.int64))


def read_bed_by_name(path):
    """One stratum per distinct value of column 4, in order of first appearance: [(name, starts, ends), ...]."""
    by = {}
    for no, cols, s, e in _bed_rows(path, 4):
        if cols[3] not in by:
            if len(by) == MAX_STRATA:
                raise ValueError("%s line %d: %r is name %d (at most %d strata)" % (path, no, cols[3], MAX_STRATA + 1, MAX_STRATA))
            by[cols[3]] = []
        by[cols[3]].append((s, e))
    return [(n, np.array([s for s, _ in iv], np.int64), np.array([e for _, e in iv], np.int64)) for n, iv in by.items()]


def check(strata):
    """[(name, starts int64, ends int64)] of a valid strata set; ValueError otherwise."""
    strata = [(str(n), np.asarray(s, np.int64).reshape(-1), np.asarray(e, np.int64).reshape(-1)) for n, s, e in strata]
    if not strata:
        raise ValueError("an empty strata set")
    if len(strata) > MAX_STRATA:
        raise ValueError("%d strata (at most %d)" % (len(strata), MAX_STRATA))
    for n, s, e in strata:
        if s.shape != e.shape:
            raise ValueError("stratum %r: %d starts and %d ends" % (n, s.shape[0], e.shape[0]))
        for k in np.flatnonzero((s < 0) | (e <= s) | (e > INT32_MAX))[:1]:
            _check_interval(int(s[k]), int(e[k]), "stratum %r, interval %d" % (n, int(k)))
    return strata


def freeze(strata):
    """a checked strata set as nested tuples: what a Job carries (hashable, travels to the ranks of a multi-GPU run)"""
    return tuple((n, tuple(int(x) for x in s), tuple(int(x) for x in e)) for n, s, e in check(strata))


def flatten(strata):
    """The segment table: (breakpoints int32 [m], masks uint32 [m]) with b[0] = INT32_MIN < b[1] < ... < b[m - 1], masks[i] valid
    on [b[i], b[i + 1]), the last segment running to INT32_MAX, equal neighbours merged:
    mask(p) = masks[searchsorted(b, p, "right") - 1] for every int32 p."""
    strata = check(strata)
    # the positions where a membership can change: the first position of an interval, the one behind its last
    cand = np.unique(np.concatenate([np.concatenate([s + 1, e + 1]) for _, s, e in strata]))
    cand = cand[cand <= INT32_MAX]
    masks = np.zeros(cand.shape[0], np.uint32)
    for k, (_, s, e) in enumerate(strata):
        # intervals of the stratum that have begun at p minus those that have ended before it: p is covered when any is left
        open_ = np.searchsorted(np.sort(s + 1), cand, "right") - np.searchsorted(np.sort(e + 1), cand, "right")
        masks |= (open_ > 0).astype(np.uint32) << np.uint32(k)
    b = np.concatenate([[INT32_MIN], cand]).astype(np.int64)
    m = np.concatenate([[0], masks]).astype(np.uint32)
    keep = np.concatenate([[True], m[1:] != m[:-1]])
    b, m = b[keep], m[keep]
    if b.shape[0] > MAX_SEGMENTS:
        raise ValueError("%d segments (at most %d)" % (b.shape[0], MAX_SEGMENTS))
    return b.astype(np.int32), m


def mask_of(table, pos):
    """the membership masks of int32 positions under a flattened table"""
    b, m = table
    return m[np.searchsorted(b, np.asarray(pos, np.int32), "right") - 1]


def row_names(strata):
    """the rows of the record side: the strata, outside, nokey (the truth side has no nokey row)"""
    return [str(s[0]) for s in strata] + [OUTSIDE, NOKEY]


def truth_row_positions(path, mode):
    """(POS of every row of a truth file that R counts as `genomediff` and whose POS is a plain decimal number of at most
    2^31 - 1, how many counted rows have no such POS).  What truth_rows and bootstrap.truth_row_windows place."""
    ix, iy, iz = (1, 3, 4) if mode == "hcmv" else (0, 1, 2)
    pos, unplaced = [], 0
    with open(path, "rb") as fh:
        for ln in fh.read().split(b"\n"):
            if not ln or ln[:1] == b"#":
                continue
            f = ln.split(b"\t")
            y, z = (f[iy] if len(f) > iy else b""), (f[iz] if len(f) > iz else b"")
            if mode == "hcmv":
                if y not in (b"A", b"C", b"G", b"T") or z not in (b"A", b"C", b"G", b"T"):
                    continue
            elif y == b"." or z == b".":
                continue
            p = f[ix] if len(f) > ix else b""
            if p.isdigit() and len(p) <= 10 and int(p) <= INT32_MAX:
                pos.append(int(p))
            else:
                unplaced += 1
    return pos, unplaced


def truth_rows(path, mode, strata):
    """int64 [S + 1]: the rows of a truth file that R counts as `genomediff`, per stratum and then `outside`, by the row's POS.
    hcmv: rows whose REF and ALT are each one of A, C, G, T (caller_performance_compare.R:29-55); custom: rows of the show-snps
    table with neither allele '.' (custom_snp_benchmark.R:23-27).  R counts ROWS, as text: a key on two rows counts twice, and
    a row the device can hold no key for (`N`, a lower-case base, a POS that is no canonical decimal below 2^28) counts too.
    Those are the rows by which this differs from the distinct keys of the bitmaps (strata_tru column 0); none of them can be
    hit, so they are missed variants.  A POS that is no plain decimal number of at most 2^31 - 1 lies in no stratum: `outside`."""
    table = flatten(strata)
    S = len(strata)
    out = np.zeros(S + 1, np.int64)
    pos, unplaced = truth_row_positions(path, mode)
    out[S] += unplaced
    m = mask_of(table, np.array(pos, np.int32))
    for s in range(S):
        out[s] += int((((m >> np.uint32(s)) & 1) != 0).sum())
    out[S] += int((m == 0).sum())
    return out


def _ratio(a, b):
    return None if b == 0 else r_round3(float(a) / float(b))


def strata_rows(names, rec, tru, pure=False, genomediff=None):
    """One VCF's rows: (stratum, genomediff, calleridentify, TP_lines, FP_lines, TP, FN, Precision, Recall, F1); None = NA.
    rec [S + 2][3] (kept, TP, FP lines), tru [S + 1][2] (truth keys, hit ones) or None.  calleridentify = the kept lines,
    Precision = TP / calleridentify, Recall = TP / genomediff (caller_performance_compare.R:97-99; a zero denominator gives NA).
    A pure-strain sample (:121-128): TP 0, Precision 0, the other truth-side columns NA.  The nokey row has no truth side.
    genomediff [S + 1] (truth_rows): the truth file's rows as R counts them, in place of the distinct keys of tru's column 0, so
    that the rows of a partitioning set sum to the whole-genome table's genomediff; FN = genomediff - TP."""
    out = []
    S = len(names)
    for k, name in enumerate(list(names) + [OUTSIDE, NOKEY]):
        n, tpl, fpl = (int(x) for x in rec[k])
        if k == S + 1:
            out.append((name, None, n, tpl, fpl, None, None, None, None, None))
        elif pure:
            out.append((name, None, n, tpl, fpl, 0, None, 0.0, None, None))
        elif tru is None:
            out.append((name, None, n, tpl, fpl, None, None, None, None, None))
        else:
            gd, tp = int(tru[k][0] if genomediff is None else genomediff[k]), int(tru[k][1])
            p, r = _ratio(tp, n), _ratio(tp, gd)
            f1 = None if p is None or r is None or p + r == 0 else r_round3(2 * (p * r) / (p + r))
            out.append((name, gd, n, tpl, fpl, tp, gd - tp, p, r, f1))
    return out


def write_performance_strata(path, rows, custom=False):
    """rows: iterable of (caller_lower, sample, names, stats) -- stats holds strata_rec, strata_tru (or None), pure_strain and,
    optionally, strata_genomediff (truth_rows: what the genomediff column then shows).
    final_tables/caller_performance_strata.tsv; custom=True: snpcall_benchmark_strata.txt (no mixture column, the custom
    table's header spelling, no pure-strain branch).  FP is counted in LINES (the distinct non-truth keys behind the whole-genome
    table's FP need the join's dedupe), and the columns say so."""
    tail = ["stratum", "genomediff", "calleridentify", "TP_lines", "FP_lines", "TP", "FN"]
    head = ["caller"] + tail + ["precision", "recall", "f1"] if custom else ["caller", "mixture"] + tail + ["Precision", "Recall", "F1"]
    with open(path, "w") as fh:
        fh.write("\t".join(head) + "\n")
        for caller, sample, names, stats in rows:
            lead = [caller] if custom else [CALLER_MAP.get(caller, caller), sample]
            for vals in strata_rows(names, stats["strata_rec"], stats.get("strata_tru"), bool(stats.get("pure_strain")) and not custom,
                                    stats.get("strata_genomediff")):
                fh.write("\t".join(lead + [r_str(v) for v in vals]) + "\n")
