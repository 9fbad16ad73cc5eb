"""Why a line is a false positive and a truth key a false negative: the class names of the near-miss pass, the
readers of its two why-files and the writer of final_tables/caller_error_classes.tsv.  The classes themselves come from the
engine (qm_batch_nearmiss); nothing here decides one."""
import os

from .tables import CALLER_MAP, r_div, r_round3, r_str

MAX_RADIUS = 64            # include/qmvt.h QM_NM_MAX_RADIUS
DEFAULT_RADIUS = 10        # --explain-radius
# in the order of include/qmvt.h QM_NM_R_* / QM_NM_T_*: the columns of Batch.nearmiss' two arrays
RECORD_CLASSES = ("idcol", "allele", "refbase", "near", "isolated", "nokey")
TRUTH_CLASSES = ("filtered", "allele", "position", "near", "uncalled")
NONE = 255                 # a record that is no FP line, a truth key that was hit
UNHELD = "."               # the class of a truth row the device cannot hold
FP_WHY_HEADER = "#line\tPOS\tREF\tALT\tQUAL\tclass"
FN_WHY_HEADER = "#POS\tREF\tALT\tclass"


def check_radius(radius):
    r = int(radius)
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("explain: radius %d (0 to %d)" % (r, MAX_RADIUS))
    return r


def fp_why_path(job):
    """the explanation of a job's FP lines beside fp/ and tp/: why/<x>.fp.why.tsv"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "why", base[:-len(".fp.vcf")] + ".fp.why.tsv")


def fn_why_path(job):
    """the explanation of a job's missed truth rows: why/<x>.fn.why.tsv"""
    return fp_why_path(job)[:-len(".fp.why.tsv")] + ".fn.why.tsv"


def _rows(path, header, classes):
    with open(path, newline="\n") as fh:   # (a field is the line's own text: a '\r' inside one stays)
        lines = fh.read().split("\n")
    if lines[0] != header or lines[-1] != "":
        raise ValueError("%s: not a why-file (header %r)" % (path, lines[0]))
    rows = [ln.split("\t") for ln in lines[1:-1]]
    width = header.count("\t") + 1
    for k, r in enumerate(rows):
        if len(r) != width or r[-1] not in classes:
            raise ValueError("%s row %d: %r" % (path, k + 1, "\t".join(r)))
    return rows


def read_fp_why(path):
    """[(line number in the input VCF, POS, REF, ALT, QUAL, class)], the four columns as the line spells them"""
    return [(int(r[0]), r[1], r[2], r[3], r[4], r[5]) for r in _rows(path, FP_WHY_HEADER, RECORD_CLASSES)]


def read_fn_why(path):
    """[(POS, REF, ALT, class)] as the truth file spells them; class `.`: a row the device cannot hold"""
    return [tuple(r) for r in _rows(path, FN_WHY_HEADER, TRUTH_CLASSES + (UNHELD,))]


def class_rows(caller, sample, rec, tru):
    """the table's rows of one caller x sample: every class of both sides, zero rows included; share = count over the side's
    total, R's round(x, 3), NA for an empty side"""
    out = []
    for side, names, counts in (("FP", RECORD_CLASSES, rec), ("FN", TRUTH_CLASSES, tru)):
        counts = [int(x) for x in counts]
        if len(counts) != len(names):
            raise ValueError("%s/%s: %d %s counts for %d classes" % (caller, sample, len(counts), side, len(names)))
        total = sum(counts)
        for name, n in zip(names, counts):
            out.append((CALLER_MAP.get(caller, caller), sample, side, name, n, r_round3(r_div(n, total)) if total else None))
    return out


def write_caller_error_classes(path, rows):
    """final_tables/caller_error_classes.tsv: `caller mixture side class count share`.  rows: iterable of (caller_lower, sample,
    rec [6], tru [5]) in the order of caller_performance.tsv.  Written atomically."""
    lines = ["\t".join(["caller", "mixture", "side", "class", "count", "share"])]
    for caller, sample, rec, tru in rows:
        lines += ["\t".join(r_str(v) for v in row) for row in class_rows(caller, sample, rec, tru)]
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
