"""The match ladder per variant type and size: the rows of the type pass (4.19) crossed with the 18 columns of the
ladder (4.23).  "How good is this caller on deletions of 6-15 bases once respellings stop counting against it" is one row of it.

Records are typed AS SPELLED: a record's row is the row byte of the type pass, so a deletion a caller spelled at the other end of a
repeat counts in the DEL row of its own spelling, under whatever method bits the ladder gave it.  A truth entry's row is the row of
its two allele codes (never NOKEY).  `counts` is the restatement of what k_ltype_records / k_ltype_truth compute
(csrc/qmvt_ltypes.hip): a bincount over (row, column) of the bytes its two producers left.  It decides nothing itself; everything
is integers and the device is compared with it exactly.  The tier order and the cumulative TP, FP and FN stay ladder.cumulative,
applied per row.
"""
import os

import numpy as np

from . import ladder as L
from . import vartype as V

N_COLS = L.N_COLS
KEPT, TP, CELL0 = L.KEPT, L.TP, L.CELL0


def _cross(bytes_, rows, n_rows, every):
    """[n_rows][18] from one byte and one row per item; every: all items count (entries), else those with a byte other than 0"""
    bytes_, rows = np.asarray(bytes_, np.uint8).reshape(-1), np.asarray(rows, np.int64).reshape(-1)
    if bytes_.shape != rows.shape:
        raise ValueError("laddertypes: %d mask bytes for %d rows" % (bytes_.shape[0], rows.shape[0]))
    take = np.ones(len(bytes_), bool) if every else bytes_ != 0
    b, r = bytes_[take].astype(np.int64), rows[take]
    if len(r) and (r.min() < 0 or r.max() >= n_rows):
        raise ValueError("laddertypes: row %d of %d" % (int(r.max() if r.max() >= n_rows else r.min()), n_rows))
    col = np.where((b & L.M_S) != 0, TP, CELL0 + (b & 15))
    out = np.bincount(r * N_COLS + col, minlength=n_rows * N_COLS).reshape(n_rows, N_COLS).astype(np.uint64)
    out[:, KEPT] = out[:, TP:].sum(axis=1)
    return out


def counts(mask, emask, rows, erows, n_rows):
    """The pass for one VCF, restated.  mask uint8 [n]: the ladder's mask byte of every record (0: not kept); emask uint8
    [entries]: that of every entry of its truth set; rows [n] / erows [entries]: the row of every record (the type pass's row
    byte) and of every entry (entry_rows).  Returns (rec, tru) uint64 [n_rows][18], columns ladder.COLS / ladder.T_COLS."""
    return _cross(mask, rows, n_rows, False), _cross(emask, erows, n_rows, True)


def entry_rows(truth, edges=None, shapes=None):
    """the row of every entry of a truth set, (pos, ref, alt) code arrays, in the order of its allele-extended table: what
    k_type_truth and k_ltype_truth compute"""
    edges = V.check_edges(edges)
    return np.array([V.row_codes(r, a, edges, shapes) for _, r, a in V.truth_order(*truth)], np.int64)


def identities(rec, tru, ladder=None, types=None, edges=None):
    """Asserts what ties one VCF's blocks ([n_rows][18] each) to its producers' rows: ladder = (rec [18], tru [18]) of the ladder,
    types = (rec [n_rows][2], tru [n_rows][2]) of the type pass; edges: for the NOKEY row of the truth side"""
    rec, tru = np.asarray(rec).astype(np.int64), np.asarray(tru).astype(np.int64)
    assert rec.shape == tru.shape and rec.shape[1] == N_COLS
    assert (rec[:, KEPT] - rec[:, TP] == rec[:, CELL0:].sum(axis=1)).all(), "per row: KEPT - TP = the 16 cells"
    assert (tru[:, KEPT] - tru[:, TP] == tru[:, CELL0:].sum(axis=1)).all(), "per row: ENTRIES - FOUND = the 16 cells"
    if ladder is not None:
        assert (rec.sum(axis=0) == np.asarray(ladder[0]).astype(np.int64)).all(), "the rows of rec sum to the ladder's rec"
        assert (tru.sum(axis=0) == np.asarray(ladder[1]).astype(np.int64)).all(), "the rows of tru sum to the ladder's tru"
    if types is not None:
        assert (rec[:, :2] == np.asarray(types[0]).astype(np.int64)).all(), "KEPT, TP per row = the type pass's kept, TP"
        assert (tru[:, :2] == np.asarray(types[1]).astype(np.int64)).all(), "ENTRIES, FOUND per row = the type pass's entries, found"
    nb = (rec.shape[0] - 4) // 5 if edges is None else len(edges)
    assert not tru[5 * nb + V.NOKEY].any(), "truth entries never land in NOKEY"


# ---- the table ---------------------------------------------------------------------------------------------------------
TABLE_HEADER = ("caller", "mixture", "type", "size") + tuple(x + s for s in L.SUFFIXES for x in ("TP", "FP", "FN", "Precision", "Recall", "F1"))
POOLED = L.POOLED


def table_rows(rec, tru, edges):
    """One VCF's (or a pool's) blocks -> [[type, size] + 5 x (TP, FP, FN, Precision, Recall, F1)]: by spelling and after each
    tier, cumulative (ladder.cumulative on the row) -- every type's bins and its `all` marginal, then the four rows behind the
    grid as plain counts (their ratios NA).  NA too where a row kept nothing."""
    from .tables import r_div, r_round3
    rec, tru = np.asarray(rec).astype(np.int64), np.asarray(tru).astype(np.int64)
    nb, lab = len(edges), V.size_labels(edges)
    if rec.shape != (V.n_rows(edges), N_COLS) or tru.shape != rec.shape:
        raise ValueError("laddertypes: count blocks of shape %r for %d size bins" % (rec.shape, nb))

    def perf(r, u, ratios=True):
        kept, entries, out = int(r[KEPT]), int(u[KEPT]), []
        for tp_k, fp_k, fn_k in L.cumulative(r, u):
            if not ratios:
                out += [tp_k, fp_k, fn_k, None, None, None]
            elif kept == 0:
                out += [0, 0, fn_k, None, None, None]
            else:
                p, q = r_round3(r_div(tp_k, kept)), r_round3(r_div(entries - fn_k, entries))
                out += [tp_k, fp_k, fn_k, p, q, r_round3(r_div(2 * (p * q), p + q))]
        return out

    out = []
    for t, name in enumerate(V.TYPE_NAMES):
        for b in range(nb):
            out.append([name, lab[b]] + perf(rec[t * nb + b], tru[t * nb + b]))
        blk = slice(t * nb, (t + 1) * nb)
        out.append([name, "all"] + perf(rec[blk].sum(axis=0), tru[blk].sum(axis=0)))
    for x, name in enumerate(V.OFFGRID_NAMES):
        out.append([name, "NA"] + perf(rec[5 * nb + x], tru[5 * nb + x], ratios=False))
    return out


def write_performance_ladder_types(path, rows, edges=None):
    """final_tables/caller_performance_ladder_types.tsv.  rows: iterable of (caller_lower, sample, stats) with
    stats["ladder_types_rec"] / stats["ladder_types_tru"] ([n_rows][18] each); jobs without them (pure-strain samples) are left
    out.  Per job the rows of table_rows; behind them one pooled block per caller, the sums over its mixtures.  Written
    atomically."""
    from .tables import CALLER_MAP, r_str
    edges = V.check_edges(edges)
    lines = ["\t".join(TABLE_HEADER)]
    pools = {}
    for caller, sample, stats in rows:
        if "ladder_types_rec" not in stats:
            continue
        rec, tru = np.asarray(stats["ladder_types_rec"]).astype(np.int64), np.asarray(stats["ladder_types_tru"]).astype(np.int64)
        if rec.shape != (V.n_rows(edges), N_COLS) or tru.shape != rec.shape:
            raise ValueError("laddertypes: %s %s has count blocks of shape %r for %d size bins" % (caller, sample, rec.shape, len(edges)))
        name = CALLER_MAP.get(caller, caller)
        for r in table_rows(rec, tru, edges):
            lines.append("\t".join([name, sample] + [r_str(v) for v in r]))
        if name not in pools:
            pools[name] = [np.zeros_like(rec), np.zeros_like(tru)]
        pools[name][0] += rec
        pools[name][1] += tru
    for name, (rec, tru) in pools.items():
        for r in table_rows(rec, tru, edges):
            lines.append("\t".join([name, POOLED] + [r_str(v) for v in r]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
