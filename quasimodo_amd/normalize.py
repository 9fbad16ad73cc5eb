"""Normal form of indels and MNPs: trim and left-align one variant against its genome, as `bcftools norm` and
`vt normalize` do (Tan et al. 2015), so that two spellings of one event compare equal.

`normalize` is the string restatement of what k_norm_truth / k_norm_records compute on allele codes; `code` / `spell` are the
codec between the inline allele codes of include/qmvt.h and strings; `counts` restates the pass's tables for one VCF; the
readers and writers of the pass's files follow.

Genome: one contig, G[p] 1-based; ACGTacgt are bases (lower case counts as its upper case), every other byte is no base.
"""
import os

import numpy as np

INLINE_MAX = 13                   # include/qmvt.h QM_ALLELE_INLINE_MAX
DICT = 0x40000000                 # QM_ALLELE_DICT
# class bytes (QM_NORM_C_*): what became of a record, or why it has no normal form
UNCHANGED, RESPELLED, RESCUED, LONG, NOKEY, NOVAR, RANGE, REFMISMATCH, NOBASE = range(9)
CLASS_NAMES = ("unchanged", "respelled", "rescued", "long", "nokey", "novar", "range", "refmismatch", "nobase")
REASONS = (LONG, NOKEY, NOVAR, RANGE, REFMISMATCH, NOBASE)
# columns of the per-VCF tables (QM_NORM_R_* / QM_NORM_T_*)
R_COLS = ("kept", "tp", "tp_n", "rescued", "respelled", "single_base") + tuple(CLASS_NAMES[r] for r in REASONS)
T_COLS = ("entries", "forms", "found", "found_by_form_only", "not_normalisable")
F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8

_BASES = "ACGT"


def base_at(genome, p):
    """G[p] as one of ACGT, or None where the genome holds no base (p outside it included)"""
    if p < 1 or p > len(genome):
        return None
    c = genome[p - 1:p].upper()
    c = c.decode("ascii", "replace") if isinstance(c, bytes) else c
    return c if c in _BASES and c else None


def normalize(genome, p, ref, alt, nokey=False):
    """(p, R, A) -> (class, p', R', A'): class UNCHANGED or RESPELLED with the normal form, or a reason with the input unchanged.
    ref / alt: strings over ACGT (any length; longer than INLINE_MAX: LONG)"""
    same = (p, ref, alt)
    if not ref or not alt or len(ref) > INLINE_MAX or len(alt) > INLINE_MAX or set(ref + alt) - set(_BASES):
        return (LONG,) + same
    if nokey:
        return (NOKEY,) + same
    if ref == alt:
        return (NOVAR,) + same
    if p < 1 or p + len(ref) - 1 > len(genome):
        return (RANGE,) + same
    if any(base_at(genome, p + k) != ref[k] for k in range(len(ref))):
        return (REFMISMATCH,) + same
    q, r, a = p, ref, alt
    changed = True
    while changed:
        changed = False
        if r and a and r[-1] == a[-1] and ((len(r) >= 2 and len(a) >= 2) or q > 1):
            r, a = r[:-1], a[:-1]
            changed = True
        if not r or not a:
            g = base_at(genome, q - 1)
            if g is None:
                return (NOBASE,) + same
            r, a, q = g + r, g + a, q - 1
            changed = True
    while len(r) >= 2 and len(a) >= 2 and r[0] == a[0]:
        r, a, q = r[1:], a[1:], q + 1
    return (UNCHANGED if (q, r, a) == same else RESPELLED, q, r, a)


def form(genome, p, ref, alt, nokey=False):
    """the form of a variant: its normal form, or its spelling where it has none"""
    return normalize(genome, p, ref, alt, nokey)[1:]


# ---- codec -------------------------------------------------------------------------------------------------------------
def code(s):
    """inline allele code of a string of 1 .. INLINE_MAX bases ACGT (include/qmvt.h); ValueError otherwise"""
    if not 1 <= len(s) <= INLINE_MAX or set(s) - set(_BASES):
        raise ValueError("no inline allele code for %r" % (s,))
    bits = 0
    for k, ch in enumerate(s):
        bits |= _BASES.index(ch) << (2 * k)
    return bits if len(s) == 1 else (len(s) << 26) | bits


def is_inline(c):
    c = int(c)
    return 0 <= c < 4 or (2 << 26) <= c < (14 << 26)


def spell(c):
    """the string of an inline allele code; None for any other code (dictionary ids, no allele)"""
    c = int(c)
    if not is_inline(c):
        return None
    n = 1 if c < 4 else c >> 26
    return "".join(_BASES[(c >> (2 * k)) & 3] for k in range(n))


def allele_nib(r, a):
    """csrc/qmvt_dev.h allele_nib: the low nibble of an allele-extended key"""
    r, a = int(r) & 0xffffffff, int(a) & 0xffffffff
    return ((r << 2) ^ a ^ ((r ^ a) >> 4)) & 15


def truth_order(pos, ref, alt):
    """the distinct valid entries of a truth set in the order of its allele-extended table: by (pos << 4 | nib, ref, alt)"""
    ok = lambda c: 0 <= c < 4 or c >= 0x08000000
    ent = {(int(p), int(r), int(a)) for p, r, a in zip(pos, ref, alt) if 0 <= int(p) < (1 << 28) and ok(int(r)) and ok(int(a))}
    return sorted(ent, key=lambda e: ((e[0] << 4) | allele_nib(e[1], e[2]), e[1], e[2]))


def form_codes(genome, p, r, a, nokey=False):
    """(class, p', r', a') on allele codes: what the device computes for one record or truth entry"""
    p, r, a = int(p), int(r), int(a)
    rs, as_ = spell(r), spell(a)
    if rs is None or as_ is None:
        return LONG, p, r, a
    c, q, r2, a2 = normalize(genome, p, rs, as_, nokey)
    return c, q, code(r2), code(a2)


def truth_forms(genome, pos, ref, alt):
    """(forms, n_not_normalisable): {form: (smallest entry index, any member respelled, member spellings)} of a truth set"""
    forms, bad = {}, 0
    for j, (p, r, a) in enumerate(truth_order(pos, ref, alt)):
        c, q, r2, a2 = form_codes(genome, p, r, a)
        bad += c in REASONS
        f = forms.setdefault((q, r2, a2), [j, False, set()])
        f[1] = f[1] or c == RESPELLED
        f[2].add((p, r, a))
    return forms, bad


def counts(genome, truth, pos, ref, alt, flags, kept, tp):
    """The pass for one VCF, restated.  truth: (pos, ref, alt) code arrays of its truth set; kept / tp: the batch's masks as bool
    arrays.  Returns (rec [len(R_COLS)], tru [len(T_COLS)], cls uint8 [n], npos, nref, nalt int32 [n], row int32 [n]): row = the
    smallest truth entry index of the record's form, -1 where the form is not in the truth set."""
    forms, bad = truth_forms(genome, *truth)
    spellings = set().union(*[f[2] for f in forms.values()]) if forms else set()
    n = len(pos)
    rec, tru = np.zeros(len(R_COLS), np.uint64), np.zeros(len(T_COLS), np.uint64)
    cls, row = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    out = [np.array(x, np.int32).copy() for x in (pos, ref, alt)]
    found, found_eq = set(), set()
    for i in range(n):
        f = int(flags[i])
        c, q, r2, a2 = form_codes(genome, pos[i], ref[i], alt[i], bool(f & F_NOKEY))
        valid = all(0 <= int(x) < 4 or int(x) >= 0x08000000 for x in (ref[i], alt[i]))
        hit = valid and not f & F_NOKEY and (q, r2, a2) in forms
        tp_n = bool(kept[i]) and (bool(hit and f & F_IDDOT) or bool(f & F_TPLINE))
        if hit:
            row[i] = forms[(q, r2, a2)][0]
        cls[i] = RESCUED if tp_n and not tp[i] else c
        out[0][i], out[1][i], out[2][i] = q, r2, a2
        if not kept[i]:
            continue
        rec[0] += 1
        rec[1] += bool(tp[i])
        rec[2] += tp_n
        rec[3] += tp_n and not tp[i]
        rec[4] += c == RESPELLED
        rec[5] += c == RESPELLED and r2 < 4 and a2 < 4
        if c in REASONS:
            rec[6 + REASONS.index(c)] += 1
        if hit:
            found.add((q, r2, a2))
            if (int(pos[i]), int(ref[i]), int(alt[i])) in spellings:
                found_eq.add((q, r2, a2))
    tru[:] = (sum(len(f[2]) for f in forms.values()), len(forms), len(found), len(found - found_eq), bad)
    return rec, tru, cls, out[0], out[1], out[2], row


# ---- files and tables --------------------------------------------------------------------------------------------------
RESCUED_HEADER = "#line\tPOS\tREF\tALT\tNORM_POS\tNORM_REF\tNORM_ALT\tTRUTH_POS\tTRUTH_REF\tTRUTH_ALT"
TABLE_HEADER = (("caller", "mixture"), (("TP", "FP", "FN", "Precision", "Recall", "F1", "TP_N", "FP_N", "FN_N", "Precision_N", "Recall_N", "F1_N")
                + R_COLS[3:] + ("truth_entries", "truth_forms", "truth_not_normalisable")))


def rescued_path(job):
    """the rescued lines of a job beside fp/ and tp/: norm/<x>.rescued.tsv"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "norm", base[:-len(".fp.vcf")] + ".rescued.tsv")


def read_rescued(path):
    """[(line number in the input VCF, (POS, REF, ALT) as the line spells them, (pos, ref, alt) of the normal form, the truth
    entry (pos, ref, alt) of the smallest index with that form or None)]"""
    with open(path, newline="\n") as fh:
        lines = fh.read().split("\n")
    if lines[0] != RESCUED_HEADER or lines[-1] != "":
        raise ValueError("%s: not a rescued-lines file (header %r)" % (path, lines[0]))
    out = []
    for k, ln in enumerate(lines[1:-1]):
        r = ln.split("\t")
        if len(r) != 10:
            raise ValueError("%s row %d: %r" % (path, k + 1, ln))
        out.append((int(r[0]), (r[1], r[2], r[3]), (int(r[4]), r[5], r[6]), None if r[7] == "." else (int(r[7]), r[8], r[9])))
    return out


def performance_row(rec, tru):
    """One VCF's rows of the pass -> TP, FP, FN, Precision, Recall, F1 by spelling, the same six by normal form, then the
    rescued, respelled, single-base and reason counts and the truth set's sizes.  The call side counts lines (TP lines of the
    batch / TP_N lines, out of the kept lines), the truth side counts forms (found by an equally spelled kept record / found at
    all, out of the distinct forms); the ratios with the rounding of tables.py; None = NA."""
    from .tables import r_div, r_round3
    rec, tru = [int(x) for x in rec], [int(x) for x in tru]
    kept, forms = rec[0], tru[1]
    out = []
    for tp, hit in ((rec[1], tru[2] - tru[3]), (rec[2], tru[2])):
        if kept == 0:
            out += [0, 0, forms - hit, None, None, None]
            continue
        p, r = r_round3(r_div(tp, kept)), r_round3(r_div(hit, forms))
        out += [tp, kept - tp, forms - hit, p, r, r_round3(r_div(2 * (p * r), p + r))]
    return out + rec[3:] + [tru[0], tru[1], tru[4]]


def write_performance_normalized(path, rows, custom=False):
    """final_tables/caller_performance_normalized.tsv (custom: snpcall_benchmark_normalized.txt, without the mixture column).
    rows: iterable of (caller_lower or label, sample, stats) with stats["norm_rec"] / stats["norm_tru"]; jobs without them
    (pure-strain samples) are left out.  Written atomically."""
    from .tables import CALLER_MAP, r_str
    head = (TABLE_HEADER[0][:1] if custom else TABLE_HEADER[0]) + TABLE_HEADER[1]
    lines = ["\t".join(head)]
    for caller, sample, stats in rows:
        if "norm_rec" not in stats:
            continue
        name = [caller] if custom else [CALLER_MAP.get(caller, caller), sample]
        lines.append("\t".join(name + [r_str(v) for v in performance_row(stats["norm_rec"], stats["norm_tru"])]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
