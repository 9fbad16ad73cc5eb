"""The four rescues combined: final TP, FP and FN when everything the engine knows is applied, and the Venn of
methods.  A kept line that is no TP by spelling can be "really a TP" by normal form (4.17), by atoms (4.18), by replayed haplotype
(4.20) or by a subset of a mismatched site (4.21); a truth entry no kept record spells can be found in the same four ways.  Every
record and every (VCF, truth entry) gets one mask byte of method bits, and the lines and entries without S are counted in the 16
cells of the four bits.

`masks` is the restatement of what k_ladder_records / k_ladder_truth compute (csrc/qmvt_ladder.hip), built on `counts` of
quasimodo_amd.normalize, .atomize and .haplo and on haplo.subset_counts: it combines their class bytes and found sets and decides
nothing itself.  Everything is integers; the device is compared with it exactly.  The ladder -- a line's tier is its lowest set
bit in the order normal form, atoms, haplotype, subset -- is a convention of this module: the device hands out the full Venn, so
another order needs no new kernel.
"""
import os

import numpy as np

from . import atomize as A
from . import haplo as H
from . import normalize as N

F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8
SUBSETS, COLUMNS = 1, 2           # include/qmvt.h QM_LADDER_SUBSETS, QM_LADDER_COLUMNS
M_N, M_A, M_H, M_B, M_K, M_S = 1, 2, 4, 8, 64, 128   # QM_LADDER_M_*
METHODS = ("normalized", "atomized", "haplotype", "subset")   # bit k of a cell index
LETTERS = "NAHB"
N_COLS = 18                       # QM_LADDER_COLS
KEPT, TP, CELL0 = 0, 1, 2         # QM_LADDER_KEPT, _TP, _CELL0; truth side: the entries, those with S, the cells
COLS = ("kept", "tp") + tuple("cell_%d" % m for m in range(16))
T_COLS = ("entries", "found") + COLS[2:]


def _valid(c):
    c = int(c)
    return 0 <= c < 4 or c >= 0x08000000


def masks(genome_n, genome_h, truth, pos, ref, alt, flags, kept, tp, gap=None, subsets=False, detail=None):
    """The pass for one VCF, restated.  genome_n / genome_h: the genome the VCF named in the normalisation / haplotype call, None
    for -1 (the bits N, or H and B, stay zero); truth: (pos, ref, alt) code arrays of its truth set; kept / tp: the batch's masks
    as bool arrays.  Returns (rec [18], tru [18] uint64, mask uint8 [n], entry_mask uint8 [entries]).  detail: a dict that
    receives what the producers' restatements returned ("norm", "atom", "hap", "sub")."""
    n = len(pos)
    kept, tp = np.asarray(kept, bool).reshape(n), np.asarray(tp, bool).reshape(n)
    flags = np.asarray(flags, np.uint8).reshape(n)
    ent = N.truth_order(*truth)
    index = {e: j for j, e in enumerate(ent)}
    iddot = (flags & F_IDDOT) != 0
    mask, emask = np.zeros(n, np.uint8), np.zeros(len(ent), np.uint8)
    mask[kept] |= M_K
    mask[kept & tp] |= M_S
    # S of the entries: spelled like a kept record with valid codes and no NOKEY (the passes' ebits)
    for i in np.flatnonzero(kept):
        e = (int(pos[i]), int(ref[i]), int(alt[i]))
        if not int(flags[i]) & F_NOKEY and _valid(e[1]) and _valid(e[2]) and e in index:
            emask[index[e]] |= M_S
    got = {}
    # by atoms
    got["atom"] = a_res = A.counts(truth, pos, ref, alt, flags, kept, tp)
    mask[kept & (a_res[2] == A.RESCUED)] |= M_A
    carried = set()
    for i in np.flatnonzero(kept):
        why, at = A.atoms_codes(pos[i], ref[i], alt[i], bool(int(flags[i]) & F_NOKEY))
        if why is None:
            carried.update(key for o, key in at if int(a_res[4][i]) >> o & 1)
    _, per, _ = A.truth_atoms(*truth)
    for j, atoms in enumerate(per):
        if atoms is not None and atoms and all(key in carried for key in atoms):
            emask[j] |= M_A
    # by normal form
    if genome_n is not None:
        got["norm"] = n_res = N.counts(genome_n, truth, pos, ref, alt, flags, kept, tp)
        mask[kept & (n_res[2] == N.RESCUED)] |= M_N
        found = {int(r) for r in n_res[6][kept] if r >= 0}        # forms by the smallest entry index of their members
        forms, _ = N.truth_forms(genome_n, *truth)
        for j, (p, r, a) in enumerate(ent):
            if forms[N.form_codes(genome_n, p, r, a)[1:]][0] in found:
                emask[j] |= M_N
    # by replayed haplotype, and by a subset of a mismatched site
    if genome_h is not None:
        tried = []
        got["hap"] = h_res = H.counts(genome_h, truth, pos, ref, alt, flags, kept, tp, gap, tried)
        open_ = kept & ~tp & iddot                                # a matched site's line with an ID other than '.' is no TP
        mask[open_ & (h_res[2] == H.RESCUED)] |= M_H
        emask[h_res[4] == H.RESCUED] |= M_H
        if subsets:
            got["sub"] = s_res = H.subset_counts(genome_h, truth, pos, ref, alt, flags, kept, tp, gap, counted=(h_res, tried))
            mask[open_ & (s_res[1] == H.SUBSET)] |= M_B
            emask[s_res[2] == H.SUBSET] |= M_B
    if detail is not None:
        detail.update(got)
    return count_records(mask), count_entries(emask), mask, emask


def count_records(mask):
    """rec [18] from the mask bytes of one VCF"""
    mask = np.asarray(mask, np.uint8)
    rec = np.zeros(N_COLS, np.uint64)
    rec[KEPT] = int(((mask & M_K) != 0).sum())
    rec[TP] = int(((mask & M_S) != 0).sum())
    open_ = ((mask & M_K) != 0) & ((mask & M_S) == 0)
    rec[CELL0:] = np.bincount(mask[open_] & 15, minlength=16)
    return rec


def count_entries(emask):
    """tru [18] from the entry bytes of one VCF"""
    emask = np.asarray(emask, np.uint8)
    tru = np.zeros(N_COLS, np.uint64)
    tru[KEPT] = len(emask)
    tru[TP] = int(((emask & M_S) != 0).sum())
    tru[CELL0:] = np.bincount(emask[(emask & M_S) == 0] & 15, minlength=16)
    return tru


def cells_with(row, bits):
    """the sum of the cells of one row whose index has any of `bits`"""
    return sum(int(row[CELL0 + m]) for m in range(16) if m & bits)


def tier(byte):
    """the tier of a mask byte without S: the lowest set method bit (0 .. 3, the index into METHODS), None for none"""
    m = int(byte) & 15
    return None if m == 0 else (m & -m).bit_length() - 1


def set_name(m):
    """the method set of a cell index or a mask byte: 'N+H', 'A', ...; 'none' for the empty one"""
    return "+".join(LETTERS[k] for k in range(4) if int(m) >> k & 1) or "none"


def cumulative(rec, tru):
    """[(TP_k, FP_k, FN_k)] for k = 0 .. 4: by spelling, then after every tier in the order of METHODS, cumulative -- from the cells"""
    rec, tru = [int(x) for x in rec], [int(x) for x in tru]
    out = []
    for k in range(5):
        low = (1 << k) - 1
        tp_k = rec[TP] + cells_with(rec, low)
        out.append((tp_k, rec[KEPT] - tp_k, tru[KEPT] - tru[TP] - cells_with(tru, low)))
    return out


def identities(rec, tru, emask=None, norm=None, atom=None, hap=None, sub=None, forms_of=None):
    """Asserts what ties one VCF's rows to the rows of its producers (each (rec, tru) of the pass, or None where the pass gave
    nothing for this VCF; sub: the search's block).  emask and forms_of ([entries]: any id of every entry's form) check the
    number of distinct forms among the entries with S or N against QM_NORM_T_FOUND."""
    rec, tru = [int(x) for x in rec], [int(x) for x in tru]
    assert rec[KEPT] - rec[TP] == sum(rec[CELL0:]), "KEPT - TP = the 16 cells"
    assert tru[KEPT] - tru[TP] == sum(tru[CELL0:]), "ENTRIES - FOUND = the 16 cells"
    for m in range(16):
        if m & M_H and m & M_B:
            assert rec[CELL0 + m] == 0, "H and B are never set together (cell %d)" % m
    if norm is not None:
        assert cells_with(rec, M_N) == int(norm[0][3]), "cells with N = QM_NORM_R_RESCUED"
        if emask is not None and forms_of is not None:
            got = {f for f, b in zip(forms_of, emask) if int(b) & (M_S | M_N)}
            assert len(got) == int(norm[1][2]), "forms among the entries with S or N = QM_NORM_T_FOUND"
    else:
        assert cells_with(rec, M_N) == 0 and cells_with(tru, M_N) == 0
    if atom is not None:
        assert cells_with(rec, M_A) == int(atom[0][3]), "cells with A = QM_ATOM_R_RESCUED"
        assert tru[TP] == int(atom[1][4]), "FOUND = QM_ATOM_T_FOUND"
        assert tru[TP] + cells_with(tru, M_A) == int(atom[1][5]), "FOUND + cells with A = QM_ATOM_T_FOUND_A"
    if hap is not None:
        assert cells_with(rec, M_H) == int(hap[0][3]), "cells with H = QM_HAP_R_RESCUED"
        assert tru[TP] + cells_with(tru, M_H) == int(hap[1][2]), "FOUND + cells with H = QM_HAP_T_FOUND_H"
        if sub is not None:
            assert rec[TP] + cells_with(rec, M_H | M_B) == int(sub[3]), "TP + cells with H or B = QM_HAPSUB_TP_S"
            assert tru[TP] + cells_with(tru, M_H | M_B) == int(sub[5]), "FOUND + cells with H or B = QM_HAPSUB_FOUND_S"
    else:
        assert cells_with(rec, M_H | M_B) == 0 and cells_with(tru, M_H | M_B) == 0


# ---- files and tables --------------------------------------------------------------------------------------------------
SUFFIXES = ("",) + tuple("_" + c for c in LETTERS)
TABLE_HEADER = (("caller", "mixture"),
                tuple(x + s for s in SUFFIXES for x in ("TP", "FP", "FN", "Precision", "Recall", "F1"))
                + tuple("lines_" + set_name(m) for m in range(1, 16)) + tuple("entries_" + set_name(m) for m in range(1, 16)))
LADDER_HEADER = "#kind\tline\tPOS\tREF\tALT\tMETHODS\tTIER"
POOLED = "pooled"


def ladder_path(job):
    """the ladder file of a job beside fp/ and tp/: ladder/<x>.ladder.tsv"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "ladder", base[:-len(".fp.vcf")] + ".ladder.tsv")


def performance_row(rec, tru):
    """One VCF's rows -> TP, FP, FN, Precision, Recall, F1 by spelling and after each of the four tiers, cumulative, then the 15
    non-empty method sets as plain counts of lines and of entries.  The call side counts lines out of the kept lines, the truth
    side entries out of the allele-extended entries; the ratios with the rounding of tables.py; None = NA."""
    from .tables import r_div, r_round3
    kept, entries = int(rec[KEPT]), int(tru[KEPT])
    out = []
    for tp_k, fp_k, fn_k in cumulative(rec, tru):
        if kept == 0:
            out += [0, 0, fn_k, None, None, None]
            continue
        p, r = r_round3(r_div(tp_k, kept)), r_round3(r_div(entries - fn_k, entries))
        out += [tp_k, fp_k, fn_k, p, r, r_round3(r_div(2 * (p * r), p + r))]
    return out + [int(rec[CELL0 + m]) for m in range(1, 16)] + [int(tru[CELL0 + m]) for m in range(1, 16)]


def write_performance_ladder(path, rows):
    """final_tables/caller_performance_ladder.tsv.  rows: iterable of (caller_lower, sample, stats) with stats["ladder_rec"] /
    stats["ladder_tru"]; jobs without them (pure-strain samples) are left out.  Per caller and mixture in the order given, then
    one pooled row per caller (the sums of its rows), callers in the order of their first row.  Written atomically."""
    from .tables import CALLER_MAP, r_str
    lines = ["\t".join(TABLE_HEADER[0] + TABLE_HEADER[1])]
    pooled = {}
    for caller, sample, stats in rows:
        if "ladder_rec" not in stats:
            continue
        rec, tru = np.asarray(stats["ladder_rec"], np.uint64), np.asarray(stats["ladder_tru"], np.uint64)
        lines.append("\t".join([CALLER_MAP.get(caller, caller), sample] + [r_str(v) for v in performance_row(rec, tru)]))
        acc = pooled.setdefault(caller, [np.zeros(N_COLS, np.uint64), np.zeros(N_COLS, np.uint64)])
        acc[0] += rec
        acc[1] += tru
    for caller, (rec, tru) in pooled.items():
        lines.append("\t".join([CALLER_MAP.get(caller, caller), POOLED] + [r_str(v) for v in performance_row(rec, tru)]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)


def job_rows(mask, emask, line_no, spelled, entries):
    """the rows of one sample's ladder file: every kept line that is no TP by spelling -- ("line", its line number in the input
    VCF, POS, REF, ALT as the line spells them, its method set, its tier or "none") -- in input order, then every truth entry
    without S -- ("entry", ".", pos, ref, alt, set, tier) -- in table order.  spelled: [(POS, REF, ALT)] per record; entries:
    [(pos, ref, alt)] per entry, alleles as strings ("." for an allele longer than 13 bases); the three columns go out as given"""
    out = []
    for kind, bytes_, names, what in (("line", mask, line_no, spelled), ("entry", emask, None, entries)):
        for i, b in enumerate(bytes_):
            b = int(b)
            if b & M_S or (kind == "line" and not b & M_K):
                continue
            t = tier(b)
            out.append((kind, "." if names is None else int(names[i]), what[i][0], what[i][1], what[i][2], set_name(b & 15),
                        "none" if t is None else METHODS[t]))
    return out


def write_job_ladder(path, rows):
    """callers/{caller}/ladder/<x>.ladder.tsv from job_rows.  Written atomically."""
    lines = [LADDER_HEADER] + ["\t".join(str(x) for x in r) for r in rows]
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)


def read_job_ladder(path):
    """[(kind, line number or None, POS, REF, ALT, method set, tier)] of a ladder file"""
    with open(path, newline="\n") as fh:
        lines = fh.read().split("\n")
    if lines[0] != LADDER_HEADER or lines[-1] != "":
        raise ValueError("%s: not a ladder file (header %r)" % (path, lines[0]))
    out = []
    for k, ln in enumerate(lines[1:-1]):
        r = ln.split("\t")
        if len(r) != 7 or r[0] not in ("line", "entry") or r[6] not in METHODS + ("none",):
            raise ValueError("%s row %d: %r" % (path, k + 1, ln))
        out.append((r[0], None if r[1] == "." else int(r[1]), int(r[2]) if r[2].isdigit() else r[2], r[3], r[4], r[5], r[6]))
    return out
