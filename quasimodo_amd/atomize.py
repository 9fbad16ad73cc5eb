"""MNPs matched against adjacent SNVs: every equal-length substitution is split into its single-base atoms, as
`bcftools norm --atomize` and `vt decompose_blocksub` do, on the record side and on the truth side, and matched atom by atom.

`atoms` is the string restatement of what k_atom_truth / k_atom_records compute on allele codes; `counts` restates the pass's
tables for one VCF; the readers and writers of the pass's files follow.  The codec (`code`, `spell`, `is_inline`), the order of
a truth set's allele-extended table (`truth_order`) and DICT are those of quasimodo_amd.normalize.  No genome takes part.
"""
import os

import numpy as np

from .normalize import DICT, code, is_inline, spell, truth_order   # noqa: F401  (DICT, code: for the callers of this module)

INLINE_MAX = 13                   # include/qmvt.h QM_ALLELE_INLINE_MAX
POS_LIMIT = 1 << 28               # an atom is (pos << 4) | (ref << 2) | alt in 32 bits
# class bytes (QM_ATOM_C_*): how many atoms of an atomisable record the truth set holds, or why a record is not atomisable
FULL, PARTIAL, NONE, RESCUED, LONG, NOKEY, NOVAR, UNEQUAL, RANGE = range(9)
CLASS_NAMES = ("full", "partial", "none", "rescued", "long", "nokey", "novar", "unequal", "range")
REASONS = (LONG, NOKEY, NOVAR, UNEQUAL, RANGE)
# columns of the per-VCF tables (QM_ATOM_R_* / QM_ATOM_T_*)
R_COLS = ("kept", "tp", "tp_a", "rescued", "multi", "partial", "atoms", "atoms_hit") + tuple(CLASS_NAMES[r] for r in REASONS)
T_COLS = ("entries", "atomisable", "atoms", "atoms_found", "found", "found_a")
F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8

_BASES = "ACGT"


def reason(p, ref, alt, nokey=False):
    """None for an atomisable variant (p, R, A), else the first reason that applies.  ref / alt: strings over ACGT of 1 ..
    INLINE_MAX bases, or None for an allele without an inline code"""
    if ref is None or alt is None:
        return LONG
    if nokey:
        return NOKEY
    if ref == alt:
        return NOVAR
    if len(ref) != len(alt):
        return UNEQUAL
    if p < 0 or p + len(ref) - 1 >= POS_LIMIT:
        return RANGE
    return None


def atoms(p, ref, alt):
    """the atoms of an atomisable variant: [(offset k, (p + k, R[k], A[k]))] for every k with R[k] != A[k]"""
    return [(k, (p + k, ref[k], alt[k])) for k in range(len(ref)) if ref[k] != alt[k]]


def atom_key(q, r, a):
    """the 32-bit word of the atom (q, r, a), r and a single bases"""
    return (q << 4) | (_BASES.index(r) << 2) | _BASES.index(a)


def mismatch_mask(r, a):
    """what the kernels take from two inline codes of one length without a loop: bit 2 k is set where base k differs"""
    r, a = int(r), int(a)
    n = 1 if r < 4 else r >> 26
    d = (r ^ a) & 0x03ffffff
    return (d | d >> 1) & 0x1555555 & ((1 << (2 * n)) - 1)


def atoms_codes(p, r, a, nokey=False):
    """(reason or None, [(offset, 32-bit atom)]) on allele codes: what the device computes for one record or truth entry"""
    p, r, a = int(p), int(r), int(a)
    rs, as_ = spell(r), spell(a)
    why = reason(p, rs, as_, nokey)
    if why is not None:
        return why, []
    return None, [(k, atom_key(*t)) for k, t in atoms(p, rs, as_)]


def truth_atoms(pos, ref, alt):
    """(entries in table order, [atom keys or None per entry], the atom set) of a truth set"""
    ent = truth_order(pos, ref, alt)
    per = []
    for p, r, a in ent:
        why, at = atoms_codes(p, r, a)
        per.append(None if why is not None else [k for _, k in at])
    return ent, per, set().union(*[set(x) for x in per if x is not None]) if ent else set()


def counts(truth, pos, ref, alt, flags, kept, tp):
    """The pass for one VCF, restated.  truth: (pos, ref, alt) code arrays of its truth set; kept / tp: the batch's masks as bool
    arrays.  Returns (rec [len(R_COLS)], tru [len(T_COLS)], cls uint8 [n], n_atoms uint8 [n], hit_mask uint16 [n])."""
    ent, per, aset = truth_atoms(*truth)
    index = {e: j for j, e in enumerate(ent)}
    n = len(pos)
    rec, tru = np.zeros(len(R_COLS), np.uint64), np.zeros(len(T_COLS), np.uint64)
    cls, na, hm = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint16)
    atoms_found, entries_found = set(), set()
    valid = lambda c: 0 <= int(c) < 4 or int(c) >= 0x08000000
    for i in range(n):
        f = int(flags[i])
        why, at = atoms_codes(pos[i], ref[i], alt[i], bool(f & F_NOKEY))
        k, t = bool(kept[i]), bool(tp[i])
        if why is None:
            hits = [(o, key) for o, key in at if key in aset]
            na[i], hm[i] = len(at), sum(1 << o for o, _ in hits)
            tp_a = k and bool((len(hits) == len(at) and f & F_IDDOT) or f & F_TPLINE)
            cls[i] = FULL if len(hits) == len(at) else PARTIAL if hits else NONE
        else:
            hits, tp_a = [], t               # the exact verdict of the batch
            cls[i] = why
        if tp_a and not t:
            cls[i] = RESCUED
        if not k:
            continue
        rec[0] += 1
        rec[1] += t
        rec[2] += tp_a
        rec[3] += tp_a and not t
        if why is None:
            rec[4] += len(at) >= 2
            rec[5] += 0 < len(hits) < len(at)
            rec[6] += len(at)
            rec[7] += len(hits)
            atoms_found.update(key for _, key in hits)
        else:
            rec[8 + REASONS.index(why)] += 1
        e = (int(pos[i]), int(ref[i]), int(alt[i]))
        if not f & F_NOKEY and valid(e[1]) and valid(e[2]) and e in index:
            entries_found.add(index[e])
    found_a = sum((j in entries_found) if a is None else all(key in atoms_found for key in a) for j, a in enumerate(per))
    tru[:] = (len(ent), sum(a is not None for a in per), len(aset), len(atoms_found), len(entries_found), found_a)
    return rec, tru, cls, na, hm


# ---- files and tables --------------------------------------------------------------------------------------------------
ATOMS_HEADER = "#line\tPOS\tREF\tALT\tN_ATOMS\tN_HIT\tHIT_MASK\tCLASS"
TABLE_HEADER = (("caller", "mixture"), (("TP", "FP", "FN", "Precision", "Recall", "F1", "TP_A", "FP_A", "FN_A", "Precision_A", "Recall_A", "F1_A")
                + R_COLS[3:] + ("truth_entries", "truth_atomisable", "truth_atoms")))


def atoms_path(job):
    """the multi-atom lines of a job beside fp/ and tp/: atoms/<x>.atoms.tsv"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "atoms", base[:-len(".fp.vcf")] + ".atoms.tsv")


def read_atoms(path):
    """[(line number in the input VCF, (POS, REF, ALT) as the line spells them, n_atoms, n_hit, hit_mask, class name)]"""
    with open(path, newline="\n") as fh:
        lines = fh.read().split("\n")
    if lines[0] != ATOMS_HEADER or lines[-1] != "":
        raise ValueError("%s: not an atoms file (header %r)" % (path, lines[0]))
    out = []
    for k, ln in enumerate(lines[1:-1]):
        r = ln.split("\t")
        if len(r) != 8 or r[7] not in CLASS_NAMES:
            raise ValueError("%s row %d: %r" % (path, k + 1, ln))
        out.append((int(r[0]), (r[1], r[2], r[3]), int(r[4]), int(r[5]), int(r[6], 16), r[7]))
    return out


def performance_row(rec, tru):
    """One VCF's rows of the pass -> TP, FP, FN, Precision, Recall, F1 by spelling, the same six by atoms, then the rescued,
    multi, partial, atoms, atoms_hit and reason counts and the truth set's sizes.  The call side counts lines (TP lines of the
    batch / TP_A lines, out of the kept lines), the truth side counts entries (found by an equally spelled kept record / with
    every atom found, out of the allele-extended entries); the ratios with the rounding of tables.py; None = NA."""
    from .tables import r_div, r_round3
    rec, tru = [int(x) for x in rec], [int(x) for x in tru]
    kept, entries = rec[0], tru[0]
    out = []
    for tp, hit in ((rec[1], tru[4]), (rec[2], tru[5])):
        if kept == 0:
            out += [0, 0, entries - hit, None, None, None]
            continue
        p, r = r_round3(r_div(tp, kept)), r_round3(r_div(hit, entries))
        out += [tp, kept - tp, entries - hit, p, r, r_round3(r_div(2 * (p * r), p + r))]
    return out + rec[3:] + [tru[0], tru[1], tru[2]]


def write_performance_atomized(path, rows):
    """final_tables/caller_performance_atomized.tsv.  rows: iterable of (caller_lower, sample, stats) with stats["atom_rec"] /
    stats["atom_tru"]; jobs without them (pure-strain samples) are left out.  Written atomically."""
    from .tables import CALLER_MAP, r_str
    lines = ["\t".join(TABLE_HEADER[0] + TABLE_HEADER[1])]
    for caller, sample, stats in rows:
        if "atom_rec" not in stats:
            continue
        lines.append("\t".join([CALLER_MAP.get(caller, caller), sample] + [r_str(v) for v in performance_row(stats["atom_rec"], stats["atom_tru"])]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
