"""TP, FP and FN by variant type and size: every kept record and every truth entry of an allele-extended batch is
typed SNV, MNP, INS, DEL or CPX from its two alleles and binned by size, as hap.py, `rtg vcfeval` and truvari report them.

`shape` is the definition on strings; `shape_codes` is what k_type_records / k_type_truth compute on allele codes -- integer work
on the 2-bit fields, with a table of (length, first 13 bases, last 13 bases) for the alleles that are dictionary ids --; `counts`
restates the pass's tables for one VCF; the writer of caller_performance_types.tsv follows.  The codec (`code`, `spell`), the order
of a truth set's allele-extended table (`truth_order`) and DICT are those of quasimodo_amd.normalize.  No genome takes part.
"""
import os

import numpy as np

from .normalize import DICT, code, is_inline, spell, truth_order   # noqa: F401  (code, spell: for the callers of this module)

INLINE_MAX = 13                   # include/qmvt.h QM_ALLELE_INLINE_MAX: an inline code, and either end of a shape row
MAX_BINS = 16                     # QM_TYPE_MAX_BINS
DEFAULT_EDGES = (1, 2, 3, 4, 5, 6, 16, 51)
SNV, MNP, INS, DEL, CPX = range(5)                  # QM_TYPE_*
TYPE_NAMES = ("SNV", "MNP", "INS", "DEL", "CPX")
NOKEY, NOVAR, LONGPAIR, NOSHAPE = range(4)          # QM_TYPE_X_*: the rows behind the grid, the first that applies wins
OFFGRID_NAMES = ("NOKEY", "NOVAR", "LONGPAIR", "NOSHAPE")
F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8
POS_LIMIT = 1 << 28

_BASES = "ACGT"
_FIELDS = 0x1555555               # bit 2 k for k = 0 .. 12


# ---- the definition, on strings ------------------------------------------------------------------------------------------
def shape(ref, alt):
    """(type, size) of the variant (ref, alt), two different strings over ACGT: the longest common prefix is trimmed, then the
    longest common suffix of what is left; what remains of either allele names the type and the size"""
    if ref == alt:
        raise ValueError("no variant: REF and ALT are both %r" % (ref,))
    m = min(len(ref), len(alt))
    cp = 0
    while cp < m and ref[cp] == alt[cp]:
        cp += 1
    cs = 0
    while cs < m - cp and ref[len(ref) - 1 - cs] == alt[len(alt) - 1 - cs]:
        cs += 1
    tr, ta = len(ref) - cp - cs, len(alt) - cp - cs
    if tr == 0:
        return INS, ta
    if ta == 0:
        return DEL, tr
    if tr == ta:
        return (SNV, 1) if tr == 1 else (MNP, tr)
    return CPX, max(tr, ta)


# ---- size bins and rows --------------------------------------------------------------------------------------------------
def check_edges(edges=None):
    """the ascending lower edges of the size bins as a tuple (None: DEFAULT_EDGES); ValueError unless there are 1 .. MAX_BINS of
    them, the first is 1 and they ascend"""
    e = DEFAULT_EDGES if edges is None else tuple(edges)
    if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in e):
        raise ValueError("vartype: the size edges are integers, not %r" % (e,))
    e = tuple(int(x) for x in e)
    if not 1 <= len(e) <= MAX_BINS:
        raise ValueError("vartype: %d size bins (1 to %d)" % (len(e), MAX_BINS))
    if e[0] != 1:
        raise ValueError("vartype: the first size edge is %d (it must be 1: every variant has a size of at least 1)" % e[0])
    if any(b <= a for a, b in zip(e, e[1:])):
        raise ValueError("vartype: the size edges ascend, %r do not" % (e,))
    if e[-1] >= 1 << 31:
        raise ValueError("vartype: size edge %d does not fit 31 bits" % e[-1])
    return e


def parse_edges(text):
    """`1,2,3,4,5,6,16,51` (the CLI's --type-bins) -> checked edges"""
    try:
        e = [int(x) for x in str(text).split(",")]
    except ValueError:
        raise ValueError("vartype: size edges are comma-separated integers, not %r" % (text,))
    return check_edges(e)


def bin_of(size, edges):
    """the bin of a size >= 1: edges[b] <= size < edges[b + 1], the last bin is open"""
    return sum(1 for e in edges[1:] if size >= e)


def n_rows(edges):
    return 5 * len(edges) + 4


def size_labels(edges):
    """`1`, `6-15`, `51+`"""
    out = []
    for b, lo in enumerate(edges):
        if b + 1 == len(edges):
            out.append("%d+" % lo)
        else:
            hi = edges[b + 1] - 1
            out.append("%d" % lo if hi == lo else "%d-%d" % (lo, hi))
    return out


def row_names(edges):
    """the name of every row: `SNV:1` ... `CPX:51+`, then the four rows behind the grid"""
    lab = size_labels(edges)
    return ["%s:%s" % (t, s) for t in TYPE_NAMES for s in lab] + list(OFFGRID_NAMES)


def row_of(kind, size, edges):
    return kind * len(edges) + bin_of(size, edges)


# ---- what the device computes, on codes ------------------------------------------------------------------------------------
def pack(s):
    """up to 13 bases, 2 bits per base, base k at bits 2 k: the layout of an inline code and of a shape row's head and tail"""
    bits = 0
    for k, ch in enumerate(s):
        bits |= _BASES.index(ch) << (2 * k)
    return bits


def shapes_of(strings):
    """the shape table (len int32, head uint32, tail uint32) of interned alleles, row i for dictionary id i: what
    qm_dict_shapes returns"""
    n = len(strings)
    ln, head, tail = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, s in enumerate(strings):
        ln[i], head[i], tail[i] = len(s), pack(s[:INLINE_MAX]), pack(s[-INLINE_MAX:])
    return ln, head, tail


def _valid(c):
    return 0 <= c < 4 or 0x08000000 <= c < 0x80000000


def _allele(c, shapes):
    """(len, head word, tail word, bases in the tail word) of a valid code, or None for a long allele without a shape row"""
    if is_inline(c):
        n = 1 if c < 4 else c >> 26
        return n, c & 0x03ffffff, c & 0x03ffffff, n
    i = c & 0x3fffffff if c >= DICT else -1     # (a valid code under DICT is no inline code and no id: it has no row either)
    if shapes is None or not 0 <= i < len(shapes[0]):
        return None
    return int(shapes[0][i]), int(shapes[1][i]) & 0x03ffffff, int(shapes[2][i]) & 0x03ffffff, INLINE_MAX


def _diff(x, y):
    d = x ^ y
    return (d | d >> 1) & _FIELDS


def shape_codes(r, a, shapes=None, nokey=False):
    """(type, size) of the variant with allele codes (r, a), or (None, reason) with the first of NOKEY, NOVAR, LONGPAIR,
    NOSHAPE that applies.  shapes: (len, head, tail) arrays with one row per dictionary id, or None.  The arithmetic is the
    kernels': XOR of the 2-bit fields, equal fields counted from the bottom (prefix) and from the top (suffix)."""
    r, a = int(r), int(a)
    if nokey or not _valid(r) or not _valid(a):
        return None, NOKEY
    if r == a:
        return None, NOVAR
    if not is_inline(r) and not is_inline(a):
        return None, LONGPAIR
    R, A = _allele(r, shapes), _allele(a, shapes)
    if R is None or A is None:
        return None, NOSHAPE
    m = min(R[0], A[0])
    fields = (1 << (2 * m)) - 1
    x = (_diff(R[1], A[1]) & fields) | (1 << (2 * m))
    cp = ((x & -x).bit_length() - 1) >> 1
    ds = _diff(R[2] >> (2 * (R[3] - m)), A[2] >> (2 * (A[3] - m))) & fields
    cs = min(m - 1 - ((ds.bit_length() - 1) >> 1) if ds else m, m - cp)
    tr, ta = R[0] - cp - cs, A[0] - cp - cs
    kind = INS if tr == 0 else DEL if ta == 0 else CPX if tr != ta else SNV if tr == 1 else MNP
    return kind, max(tr, ta)


def row_codes(r, a, edges, shapes=None, nokey=False):
    kind, x = shape_codes(r, a, shapes, nokey)
    return 5 * len(edges) + x if kind is None else row_of(kind, x, edges)


def counts(truth, pos, ref, alt, flags, kept, tp, edges=None, shapes=None):
    """The pass for one VCF, restated.  truth: (pos, ref, alt) code arrays of its truth set; kept / tp: the batch's masks as bool
    arrays.  Returns (rec [n_rows][2]: kept records and the TP lines among them, tru [n_rows][2]: truth entries and the found
    ones, row uint8 [n]: the row of every record, kept or not)."""
    edges = check_edges(edges)
    ent = truth_order(*truth)
    index = {e: j for j, e in enumerate(ent)}
    n, nr = len(pos), n_rows(edges)
    rec, tru, rows = np.zeros((nr, 2), np.uint64), np.zeros((nr, 2), np.uint64), np.zeros(n, np.uint8)
    found, memo = set(), {}
    for i in range(n):
        f, r, a = int(flags[i]), int(ref[i]), int(alt[i])
        k = (r, a, bool(f & F_NOKEY))
        if k not in memo:
            memo[k] = row_codes(r, a, edges, shapes, k[2])
        rows[i] = row = memo[k]
        if not kept[i]:
            continue
        rec[row, 0] += 1
        rec[row, 1] += bool(tp[i])
        e = (int(pos[i]), r, a)
        if not f & F_NOKEY and _valid(r) and _valid(a) and 0 <= e[0] < POS_LIMIT and e in index:
            found.add(index[e])
    for j, (_, r, a) in enumerate(ent):
        row = row_codes(r, a, edges, shapes)
        tru[row, 0] += 1
        tru[row, 1] += j in found
    return rec, tru, rows


# ---- the table ---------------------------------------------------------------------------------------------------------
TABLE_HEADER = ("caller", "mixture", "type", "size", "TP", "FP", "FN", "Precision", "Recall", "F1")


def _performance(kept, tp, entries, found):
    """TP, FP, FN, Precision (TP / kept), Recall (found / entries), F1 with the rounding of tables.py; None = NA"""
    from .tables import r_div, r_round3
    if kept == 0:
        return [0, 0, entries - found, None, None, None]
    p, r = r_round3(r_div(tp, kept)), r_round3(r_div(found, entries))
    return [tp, kept - tp, entries - found, p, r, r_round3(r_div(2 * (p * r), p + r))]


def table_rows(rec, tru, edges):
    """One VCF's (or a pool's) count blocks -> [(type, size, TP, FP, FN, Precision, Recall, F1)]: every type's bins and its
    `all` marginal, then the rows behind the grid as plain counts (their ratios NA)"""
    rec, tru = np.asarray(rec).astype(np.int64), np.asarray(tru).astype(np.int64)
    nb, lab, out = len(edges), size_labels(edges), []
    for t, name in enumerate(TYPE_NAMES):
        blk = slice(t * nb, (t + 1) * nb)
        for b in range(nb):
            r, u = rec[t * nb + b], tru[t * nb + b]
            out.append([name, lab[b]] + _performance(int(r[0]), int(r[1]), int(u[0]), int(u[1])))
        r, u = rec[blk].sum(axis=0), tru[blk].sum(axis=0)
        out.append([name, "all"] + _performance(int(r[0]), int(r[1]), int(u[0]), int(u[1])))
    for x, name in enumerate(OFFGRID_NAMES):
        r, u = rec[5 * nb + x], tru[5 * nb + x]
        out.append([name, "NA", int(r[1]), int(r[0] - r[1]), int(u[0] - u[1]), None, None, None])
    return out


def write_performance_types(path, rows, edges=None):
    """final_tables/caller_performance_types.tsv.  rows: iterable of (caller_lower, sample, stats) with stats["type_rec"] /
    stats["type_tru"] ([n_rows][2] each); jobs without them (pure-strain samples) are left out.  Per job the rows of table_rows;
    behind them one pooled block per caller, the sums over its mixtures (mixture `pooled`).  Written atomically."""
    from .tables import CALLER_MAP, r_str
    edges = check_edges(edges)
    lines = ["\t".join(TABLE_HEADER)]
    pools = {}
    for caller, sample, stats in rows:
        if "type_rec" not in stats:
            continue
        rec, tru = np.asarray(stats["type_rec"]).astype(np.int64), np.asarray(stats["type_tru"]).astype(np.int64)
        if rec.shape != (n_rows(edges), 2) or tru.shape != rec.shape:
            raise ValueError("vartype: %s %s has count blocks of shape %r for %d size bins" % (caller, sample, rec.shape, len(edges)))
        name = CALLER_MAP.get(caller, caller)
        for r in table_rows(rec, tru, edges):
            lines.append("\t".join([name, sample] + [r_str(v) for v in r]))
        if name not in pools:
            pools[name] = [np.zeros_like(rec), np.zeros_like(tru)]
        pools[name][0] += rec
        pools[name][1] += tru
    for name, (rec, tru) in pools.items():
        for r in table_rows(rec, tru, edges):
            lines.append("\t".join([name, "pooled"] + [r_str(v) for v in r]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
