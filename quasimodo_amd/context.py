"""Sequence-context profiles: TP, FP and FN counts per homopolymer x GC cell.

A position p (1-based POS) of a one-contig genome of length L lies in cell hp(p) * n_gc + gb(p):

  run(i)  0 when i < 1, i > L or G[i] is no base (not ACGTacgt); else the length of the maximal block of consecutive positions
          around i whose bases equal G[i]'s, case-insensitively
  hp(p)   min(15, max(run(p - 1), run(p), run(p + 1))): a call next to a run counts as in its context
  gb(p)   min(n_gc - 1, gc * n_gc // nb) over the window [max(1, p - w), min(L, p + w)]: nb its positions that hold a base,
          gc those of them that are C or G; a window without a base (nb = 0) gives the position no cell: NONE

`cells` is the pure-numpy restatement of the table qm_genome_context builds (run lengths from a run-length encoding, windows
from cumulative sums: not the device's tiles); the names, the marginals and the table writer need no device."""
import numpy as np

from .strata import truth_row_positions
from .tables import CALLER_MAP, r_round3, r_str

MAX_HALF_WINDOW = 1024            # include/qmvt.h QM_CX_MAX_HALF_WINDOW
MAX_GC_BINS = 15                  # QM_CX_MAX_GC_BINS
HP_ROWS = 16                      # homopolymer rows 0 .. 15; the last one holds 15 and longer
NONE_BYTE = 255                   # QM_CX_NONE: the table's byte of a position without a cell
DEFAULT_HALF_WINDOW, DEFAULT_GC_BINS = 50, 10
ALL, NONE, NOKEY = "all", "none", "nokey"

_CODE = np.full(256, 15, np.uint8)
for _k, _b in enumerate(b"ACGT"):
    _CODE[_b] = _CODE[_b + 32] = _k


def check_params(half_window, n_gc):
    """(half_window, n_gc) as ints; ValueError outside the library's limits"""
    w, ng = int(half_window), int(n_gc)
    if not 0 <= w <= MAX_HALF_WINDOW:
        raise ValueError("context: half window %d (0 to %d)" % (w, MAX_HALF_WINDOW))
    if not 1 <= ng <= MAX_GC_BINS:
        raise ValueError("context: %d GC bins (1 to %d)" % (ng, MAX_GC_BINS))
    return w, ng


def n_cells(n_gc):
    """the grid and NONE: the rows of the truth side and of `gen`; the record side has one more, nokey"""
    return HP_ROWS * int(n_gc) + 1


def cells(genome_bytes, half_window=DEFAULT_HALF_WINDOW, n_gc=DEFAULT_GC_BINS):
    """uint8 [L]: the cell of every position (entry p - 1 for POS p), NONE_BYTE where it has none"""
    w, ng = check_params(half_window, n_gc)
    code = _CODE[np.frombuffer(bytes(genome_bytes), np.uint8)]
    L = code.shape[0]
    if L == 0:
        return np.zeros(0, np.uint8)
    base = code < 4
    # run lengths: the blocks of equal codes, every position of a block gets the block's length, blocks of no base 0
    first = np.concatenate([[0], np.flatnonzero(code[1:] != code[:-1]) + 1])
    length = np.diff(np.concatenate([first, [L]]))
    run = np.where(base, np.repeat(length, length), 0)
    around = np.concatenate([[0], run, [0]])
    hp = np.minimum(15, np.maximum(np.maximum(around[:-2], around[1:-1]), around[2:]))
    # windows: differences of cumulative sums
    cb = np.concatenate([[0], np.cumsum(base, dtype=np.int64)])
    cg = np.concatenate([[0], np.cumsum((code == 1) | (code == 2), dtype=np.int64)])
    i = np.arange(L, dtype=np.int64)
    lo, hi = np.maximum(0, i - w), np.minimum(L, i + w + 1)
    nb, gc = cb[hi] - cb[lo], cg[hi] - cg[lo]
    gb = np.minimum(ng - 1, gc * ng // np.maximum(nb, 1))
    return np.where(nb > 0, hp * ng + gb, NONE_BYTE).astype(np.uint8)


def rows_of(table, pos, n_gc):
    """the output row of int positions under a table of `cells`: the cell, row 16 n_gc (NONE) outside 1 .. L and where the
    table has no cell"""
    pos = np.asarray(pos, np.int64)
    none = HP_ROWS * int(n_gc)
    inside = (pos >= 1) & (pos <= table.shape[0])
    c = table[np.where(inside, pos - 1, 0)].astype(np.int64) if table.shape[0] else np.zeros(pos.shape, np.int64)
    return np.where(inside & (c != NONE_BYTE), c, none)


def positions(table, n_gc):
    """int64 [n_cells]: the positions of the genome per cell (`gen`): sum L"""
    return np.bincount(rows_of(table, np.arange(1, table.shape[0] + 1), n_gc), minlength=n_cells(n_gc)).astype(np.int64)


def hp_name(h):
    return "15+" if int(h) == 15 else str(int(h))


def gc_bounds(g, n_gc):
    """(gc_from, gc_to) of GC bin g as fractions rounded like the table's ratios: gc / nb in [g / n_gc, (g + 1) / n_gc)"""
    return r_round3(g / float(n_gc)), r_round3((g + 1) / float(n_gc))


def cell_names(n_gc):
    """[(homopolymer, gc_bin)] of every record-side row: the grid, then (none, none) and (nokey, nokey)"""
    ng = int(n_gc)
    return [(hp_name(h), str(g)) for h in range(HP_ROWS) for g in range(ng)] + [(NONE, NONE), (NOKEY, NOKEY)]


def truth_rows(path, mode, table, n_gc):
    """int64 [n_cells]: the rows of a truth file that R counts as `genomediff` (strata.truth_rows' row rule), per cell by the
    row's POS; a POS that is no plain decimal number of at most 2^31 - 1, or outside the genome, lies in NONE."""
    pos, unplaced = truth_row_positions(path, mode)
    out = np.bincount(rows_of(table, np.array(pos, np.int64), n_gc), minlength=n_cells(n_gc)).astype(np.int64)
    out[HP_ROWS * int(n_gc)] += unplaced
    return out


def _ratio(a, b):
    return None if b == 0 else r_round3(float(a) / float(b))


def _row(hp, gb, lo, hi, positions_, rec, tru, gd, pure, truth_side=True):
    n, tpl, fpl = (int(x) for x in rec)
    per_kb = None if positions_ is None else _ratio(1000 * fpl, int(positions_))
    head = (hp, gb, lo, hi, None if positions_ is None else int(positions_), n, tpl, fpl)
    if not truth_side:
        return head + (None, None, None, None, None, None, per_kb)
    if pure:
        return head + (None, 0, None, 0.0, None, None, per_kb)
    if tru is None:
        return head + (None, None, None, None, None, None, per_kb)
    gd, tp = int(tru[0] if gd is None else gd), int(tru[1])
    p, r = _ratio(tp, n), _ratio(tp, gd)
    f1 = None if p is None or r is None or p + r == 0 else r_round3(2 * (p * r) / (p + r))
    return head + (gd, tp, gd - tp, p, r, f1, per_kb)


def context_rows(n_gc, rec, tru, gen, pure=False, genomediff=None):
    """One VCF's rows: (homopolymer, gc_bin, gc_from, gc_to, positions, calleridentify, TP_lines, FP_lines, genomediff, TP, FN,
    Precision, Recall, F1, FP_per_kb); None = NA.  rec [n_cells + 1][3] (kept, TP, FP lines), tru [n_cells][2] (truth keys, hit
    ones) or None, gen [n_cells] positions per cell.  First every cell with a position or a count, then the marginals `gc_bin =
    all` per homopolymer row and `homopolymer = all` per GC bin, then none, then nokey.  The number rules are strata_rows':
    Precision = TP / calleridentify, Recall = TP / genomediff, R's round(x, 3), NA on a zero denominator, a pure-strain sample
    TP 0 and Precision 0 with the other truth-side columns NA, nokey without a truth side; genomediff [n_cells] (truth_rows)
    replaces the distinct keys of tru's column 0 and FN = genomediff - TP.  FP_per_kb = 1000 * FP_lines / positions.  Each
    marginal family plus none and nokey sums to the whole-genome table."""
    ng = int(n_gc)
    nc = n_cells(ng)
    rec = np.asarray(rec).astype(np.int64).reshape(nc + 1, 3)
    gen = np.asarray(gen).astype(np.int64).reshape(nc)
    tru = None if tru is None else np.asarray(tru).astype(np.int64).reshape(nc, 2)
    gd = None if genomediff is None else np.asarray(genomediff).astype(np.int64).reshape(nc)
    grid = lambda a: a[:HP_ROWS * ng].reshape((HP_ROWS, ng) + a.shape[1:])
    R, G = grid(rec), grid(gen)
    T = None if tru is None else grid(tru)
    D = None if gd is None else grid(gd)
    pick = lambda a, *ix: None if a is None else a[ix]
    out = []
    for h in range(HP_ROWS):
        for g in range(ng):
            if G[h, g] > 0 or R[h, g].any() or (T is not None and T[h, g].any()) or (D is not None and D[h, g] > 0):
                lo, hi = gc_bounds(g, ng)
                out.append(_row(hp_name(h), str(g), lo, hi, G[h, g], R[h, g], pick(T, h, g), pick(D, h, g), pure))
    for h in range(HP_ROWS):
        out.append(_row(hp_name(h), ALL, None, None, G[h].sum(), R[h].sum(0), None if T is None else T[h].sum(0),
                        None if D is None else D[h].sum(), pure))
    for g in range(ng):
        lo, hi = gc_bounds(g, ng)
        out.append(_row(ALL, str(g), lo, hi, G[:, g].sum(), R[:, g].sum(0), None if T is None else T[:, g].sum(0),
                        None if D is None else D[:, g].sum(), pure))
    k = HP_ROWS * ng
    out.append(_row(NONE, NONE, None, None, gen[k], rec[k], pick(tru, k), pick(gd, k), pure))
    out.append(_row(NOKEY, NOKEY, None, None, None, rec[k + 1], None, None, pure, truth_side=False))
    return out


HEAD_TAIL = ["homopolymer", "gc_bin", "gc_from", "gc_to", "positions", "calleridentify", "TP_lines", "FP_lines", "genomediff", "TP", "FN"]


def write_performance_context(path, rows, n_gc, custom=False):
    """rows: iterable of (caller_lower, sample, stats) -- stats holds context_rec, context_tru (or None), context_gen, pure_strain
    and, optionally, context_genomediff (truth_rows: what the genomediff column then shows).
    final_tables/caller_performance_context.tsv; custom=True: snpcall_benchmark_context.txt (no mixture column, the custom
    table's header spelling, no pure-strain branch)."""
    head = (["caller"] + HEAD_TAIL + ["precision", "recall", "f1"] if custom else ["caller", "mixture"] + HEAD_TAIL + ["Precision", "Recall", "F1"])
    with open(path, "w") as fh:
        fh.write("\t".join(head + ["FP_per_kb"]) + "\n")
        for caller, sample, stats in rows:
            lead = [caller] if custom else [CALLER_MAP.get(caller, caller), sample]
            for vals in context_rows(n_gc, stats["context_rec"], stats.get("context_tru"), stats["context_gen"],
                                     bool(stats.get("pure_strain")) and not custom, stats.get("context_genomediff")):
                fh.write("\t".join(lead + [r_str(v) for v in vals]) + "\n")
