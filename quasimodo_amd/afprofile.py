"""Allele-frequency profiles: the host side of the first output of the reference's rule mutationcontext
(rules/mutationcontext.smk: {mix}.{caller}.snp.profile.pdf; scripts/mutation_context_profile.R:19-46, filterVCF + varPlot).  The
counts come from the engine (qm_batch_af_profile); this module names the bins and writes the tables.  The plot
itself is out of scope; the points it would show are written by the library (Job.points_out)."""
import os

import numpy as np

TYPES = ("TP", "FP")                       # the class rows of the engine's grids, varPlot's `type`
EXTRA_NAMES = ("no_af", "outside", "in_grid")   # include/qmvt.h QM_AFP_NO_AF, QM_AFP_OUTSIDE, QM_AFP_N_GRID
DEFAULTS = dict(window=1024, n_pos_bins=256, n_af_bins=20)   # 262 kb: HCMV is 236 kb


def _atomic(path, text):
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write(text)
    os.replace(tmp, path)


def _rows(rows):
    out = []
    for row in rows:
        sample, grid, extra = row[0], np.asarray(row[1]), np.asarray(row[2])
        types = tuple(row[3]) if len(row) > 3 else TYPES
        if grid.ndim != 3 or grid.shape[0] != 2 or extra.shape != (2, len(EXTRA_NAMES)):
            raise ValueError("sample %r: grid %s / extra %s, need [2][n_af_bins][n_pos_bins] and [2][3]" % (sample, grid.shape, extra.shape))
        out.append((sample, grid, extra, types))
    return out


def write_profile_grid(path, rows, window=DEFAULTS["window"]):
    """final_tables/{mix}.{caller}.snp.profile.tsv: long format, header `sample type af_lo af_hi pos_lo pos_hi count`, one line
    per non-zero cell (cell [a][p]: af_lo = a / n_af_bins <= AF < af_hi, the last bin closed at 1; positions pos_lo ..
    pos_hi = p * window + 1 .. (p + 1) * window), samples in the given order, TP before FP, cells in [a][p] order; then one
    `# sample type no_af outside in_grid` line per sample and type.  rows: (sample, grid [2][A][P], extra [2][3][, types]);
    types: the class rows to write (default TP and FP; ("FP",) for an unmixed sample).  Written atomically."""
    rows = _rows(rows)
    window = int(window)
    lines = ["sample\ttype\taf_lo\taf_hi\tpos_lo\tpos_hi\tcount"]
    for sample, grid, extra, types in rows:
        nA = grid.shape[1]
        for t, name in enumerate(TYPES):
            if name not in types:
                continue
            for a, p in zip(*np.nonzero(grid[t])):
                lines.append("%s\t%s\t%.6g\t%.6g\t%d\t%d\t%d" % (sample, name, a / nA, (a + 1) / nA, p * window + 1, (p + 1) * window, int(grid[t, a, p])))
    lines.append("# sample\ttype\t" + "\t".join(EXTRA_NAMES))
    for sample, grid, extra, types in rows:
        for t, name in enumerate(TYPES):
            if name in types:
                lines.append("# %s\t%s\t%s" % (sample, name, "\t".join(str(int(x)) for x in extra[t])))
    _atomic(path, "\n".join(lines) + "\n")


def af_sweep(grid):
    """[2][n_af_bins] int64: TP(af >= a / n_af_bins), FP(...) -- suffix sums of the grid's AF marginal"""
    m = np.asarray(grid).astype(np.int64).sum(axis=2)
    return np.cumsum(m[:, ::-1], axis=1)[:, ::-1]


def write_af_sweep(path, rows):
    """final_tables/{mix}.{caller}.snp.profile.afsweep.tsv: header `sample af_min TP FP`, one line per sample and AF bin edge
    t = a / n_af_bins: the SNVs of the grid with AF >= t.  rows: as write_profile_grid's (a type left out reads 0)."""
    lines = ["sample\taf_min\tTP\tFP"]
    for sample, grid, extra, types in _rows(rows):
        sw = af_sweep(grid)
        nA = grid.shape[1]
        for a in range(nA):
            lines.append("%s\t%.6g\t%d\t%d" % (sample, a / nA, sw[0, a] if "TP" in types else 0, sw[1, a] if "FP" in types else 0))
    _atomic(path, "\n".join(lines) + "\n")


def sample_rows(sample_stats):
    """The rows of one mix's tables as the rule picks its samples: sorted, `-1-0` left out, `-0-1` as FP only (varPlot(sample, vcf)).
    sample_stats: {sample: stats with af_grid / af_extra}."""
    rows = []
    for s in sorted(sample_stats):
        if s.endswith("-1-0"):
            continue
        st = sample_stats[s]
        rows.append((s, st["af_grid"], st["af_extra"], ("FP",) if s.endswith("-0-1") else TYPES))
    return rows
