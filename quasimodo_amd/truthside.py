"""The truth-side view: the host side of the caller Venn diagram of scripts/caller_performance_compare.R:110-119,510-549
(`Genome` against the distinct single-base `pos-ref-alt` keys of the compared callers, per mixed sample) and of the
missed-variant lists.  The counts come from the engine (qm_batch_truth_hits / qm_batch_truth_regions for the regions inside
`Genome`, Engine.fp_overlap over the keys of the kept records outside the in-truth record mask for the others);
this module names the regions, writes final_tables/caller_snp_venn.tsv and states which rows of a truth file belong into a
missed-variant (FN) list.  Drawing the diagram is out of scope."""
import os

from .tables import CALLER_MAP

GENOME = "Genome"
MAX_GROUP = 5                                  # include/qmvt.h QM_TRUTH_GROUP_MAX
VENN_CALLERS = ("lofreq", "varscan", "clc")    # rules/vis_eval_vcf.smk:2 venn_snpcallers
_BASES = (b"A", b"C", b"G", b"T")


def venn_callers(callers):
    """the Venn callers of a run: venn_snpcallers restricted to the callers it has, in venn_snpcallers' order"""
    have = set(callers)
    return [c for c in VENN_CALLERS if c in have]


def check_group(callers):
    """a group of the truth-side pass holds 1 to MAX_GROUP callers"""
    callers = list(callers)
    if not 1 <= len(callers) <= MAX_GROUP:
        raise ValueError("a truth-side group holds 1 to %d callers, not %d (%s)" % (MAX_GROUP, len(callers), ", ".join(callers)))
    if len(set(callers)) != len(callers):
        raise ValueError("a truth-side group names a caller twice (%s)" % ", ".join(callers))
    return callers


def set_names(callers):
    """[Genome, <caller names as caller_performance_compare.R:24-27 spells them>]: bit i of a region's mask is set i"""
    return [GENOME] + [CALLER_MAP.get(c, c) for c in check_group(callers)]


def region_name(mask, names):
    """'Genome&LoFreq&CLC' for mask 0b1011 over [Genome, LoFreq, VarScan2, CLC]"""
    if not 0 < mask < 1 << len(names):
        raise ValueError("region mask %d outside 1 .. %d" % (mask, (1 << len(names)) - 1))
    return "&".join(n for i, n in enumerate(names) if mask >> i & 1)


def venn_counts(truth_regions, fp_regions, n):
    """The 2^(n+1) - 1 non-empty regions of Genome + n callers, in mask order (bit 0 = Genome, bit i + 1 = caller i).
    truth_regions: qm_batch_truth_regions' slots of the group ([m] = truth keys hit by exactly the callers of m; slot 0 = missed
    by all = `Genome` only).  fp_regions: Engine.fp_overlap's slots over the callers' keys outside the truth set."""
    if len(truth_regions) < 1 << n or len(fp_regions) < 1 << n:
        raise ValueError("need %d region slots per side" % (1 << n))
    return [(m, int(truth_regions[m >> 1]) if m & 1 else int(fp_regions[m >> 1])) for m in range(1, 1 << (n + 1))]


def reorder_regions(regions, have, want):
    """Region slots counted over the sets `have` (bit i = have[i]) as slots over the same sets in the order `want`."""
    n = len(have)
    if sorted(have) != sorted(want) or len(set(have)) != n:
        raise ValueError("reorder_regions: %r and %r are not the same sets" % (list(have), list(want)))
    to = [list(want).index(c) for c in have]
    out = [0] * (1 << n)
    for m in range(1 << n):
        out[sum(1 << to[i] for i in range(n) if m >> i & 1)] = int(regions[m])
    return out


def write_caller_snp_venn(path, per_sample, callers):
    """final_tables/caller_snp_venn.tsv: `sample region count`, one row per mixed sample (sorted) and non-empty region, in mask
    order.  per_sample: {sample: (truth_regions, fp_regions)} (venn_counts).  Written atomically."""
    names = set_names(callers)
    n = len(names) - 1
    lines = ["sample\tregion\tcount"]
    for sample in sorted(per_sample):
        tr, fr = per_sample[sample]
        for m, c in venn_counts(tr, fr, n):
            lines.append("%s\t%s\t%d" % (sample, region_name(m, names), c))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)


def snp_key(line):
    """The key make_snp_vector (caller_performance_compare.R:29-55) gives one well-formed data row: the TEXT of POS, REF, ALT when
    REF and ALT are each exactly one of A, C, G, T (upper case); None for every other row ('#' rows, rows with fewer than five
    columns).  A trailing '\r' is not part of the row.
    This is a PER-ROW rule and UNPINNED (no R here).  R's read.table acts on the whole file: with its eight colClasses one row
    of another field count makes the read fail and tryCatch return an EMPTY set; it strips quotes and cuts a line at a '#'
    anywhere in it (tables.r_hostile_rows counts such rows; the strict table writers refuse such files).  On the files
    mummer2vcf.py writes -- eight columns, no quotes, '#' only in the header -- the two agree."""
    line = line.rstrip(b"\r")
    if line.startswith(b"#"):
        return None
    f = line.split(b"\t")
    if len(f) < 5 or f[3] not in _BASES or f[4] not in _BASES:
        return None
    return (f[1], f[3], f[4])


def snp_keys(text):
    """the keys of a VCF's rows by the per-row rule of snp_key (what make_snp_vector builds from a file it reads whole)"""
    return {k for k in (snp_key(ln) for ln in text.split(b"\n")) if k is not None}


def fn_text(truth_text, kept_keys):
    """A missed-variant list: the truth file's header lines, then, in file order, every data row whose key the reference puts
    into `Genome` (snp_key) and that is not among kept_keys (the kept single-base keys of one VCF, or of several for
    `missed_by_all`).  A key on several rows is written on each of them; lines keep their bytes and end in a newline."""
    lines = truth_text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    head = [ln for ln in lines if ln.startswith(b"#")]
    rows = []
    for ln in lines:
        k = snp_key(ln)
        if k is not None and k not in kept_keys:
            rows.append(ln)
    return b"".join(ln + b"\n" for ln in head + rows)
