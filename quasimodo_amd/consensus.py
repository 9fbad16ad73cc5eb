"""k-of-n caller consensus: the host side of the vote pass (qm_batch_votes).  The vote histograms come from the
engine; this module does the level arithmetic (TP, FP, FN, Precision, Recall, F1 of "at least k of the n callers agree"),
states as text which lines a consensus VCF holds, and writes final_tables/caller_consensus.tsv and caller_private.tsv.
The reference has no counterpart; the caller Venn diagrams it draws (scripts/caller_performance_compare.R:110-119) are the
motivation.  A 2^n-slot region table cannot grow to 32 members; a vote histogram can."""
import os
import re

from .tables import CALLER_MAP, performance_row, r_str

MAX_GROUP = 32                                 # include/qmvt.h QM_VOTE_GROUP_MAX
_BASE_CODE = {b"A": 0, b"C": 1, b"G": 2, b"T": 3}
_POS = re.compile(rb"(0|[1-9][0-9]*)\Z")
POS_LIMIT = 1 << 28


def check_group(members):
    """a vote group holds 1 to MAX_GROUP members, each once"""
    members = list(members)
    if not 1 <= len(members) <= MAX_GROUP:
        raise ValueError("a vote group holds 1 to %d members, not %d" % (MAX_GROUP, len(members)))
    if len(set(members)) != len(members):
        raise ValueError("a vote group names a member twice (%s)" % ", ".join(str(m) for m in members))
    return members


def level_counts(tp_votes, fp_votes, n):
    """[(k, TP_k, FP_k, FN_k)] for k = 1 .. n: TP_k = sum of tp_votes[c] over c >= k, FP_k the same over fp_votes, FN_k = T' - TP_k
    with T' = the sum of the whole tp_votes row (slot 0 = truth keys nobody calls)."""
    if not 1 <= n <= MAX_GROUP:
        raise ValueError("n = %d outside 1 .. %d" % (n, MAX_GROUP))
    if len(tp_votes) < n + 1 or len(fp_votes) < n + 1:
        raise ValueError("need %d vote slots per side" % (n + 1))
    tp_votes = [int(x) for x in tp_votes]
    fp_votes = [int(x) for x in fp_votes]
    if any(tp_votes[n + 1:]) or any(fp_votes[n + 1:]) or fp_votes[0]:
        raise ValueError("votes outside 0 .. n = %d (or a key outside the truth set with no vote)" % n)
    t = sum(tp_votes)
    out = []
    for k in range(1, n + 1):
        tp, fp = sum(tp_votes[k:]), sum(fp_votes[k:])
        out.append((k, tp, fp, t - tp))
    return out


def level_row(tp, fp, fn):
    """(TP, FP, FN, Precision, Recall, F1) of one consensus level, the ratios as tables.performance_row computes them for
    caller_performance.tsv: the level's distinct keys TP + FP stand for the kept lines, T' = TP + FN for genomediff; no key at the
    level: three NA (None); R's x / 0 and 0 / 0; round(x, 3)."""
    st = {"n_pass": tp + fp, "genomediff": tp + fn, "TP_R": tp, "FP_R": fp}
    _, _, _, _, p, r, f1 = performance_row(st)
    return tp, fp, fn, p, r, f1


def device_key(line):
    """pos << 4 | ref << 2 | alt of one data line as the device keys it, or None: '#' lines, fewer than five columns, REF or ALT
    not exactly one of A, C, G, T, a POS that is not a canonical decimal below 2^28 (such a kept line is QM_F_NOKEY: it takes
    no part in the votes).  A trailing '\\r' is not part of the line."""
    line = line.rstrip(b"\r")
    if line.startswith(b"#"):
        return None
    f = line.split(b"\t")
    if len(f) < 5 or f[3] not in _BASE_CODE or f[4] not in _BASE_CODE or not _POS.match(f[1]):
        return None
    pos = int(f[1])
    if pos >= POS_LIMIT:
        return None
    return pos << 4 | _BASE_CODE[f[3]] << 2 | _BASE_CODE[f[4]]


def _lines(text):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def member_keys(filtered_text):
    """{key: first line carrying it} over the kept lines of one member (the text of its <x>.filtered.vcf)"""
    first = {}
    for ln in _lines(filtered_text):
        k = device_key(ln)
        if k is not None and k not in first:
            first[k] = ln
    return first


def vote_masks(filtered_texts):
    """{key: mask} over the members' kept lines: bit i set iff member i calls the key (a key on several lines counts once)"""
    check_group(range(len(filtered_texts)))
    masks = {}
    for i, t in enumerate(filtered_texts):
        for k in member_keys(t):
            masks[k] = masks.get(k, 0) | 1 << i
    return masks


def consensus_text(filtered_texts, k):
    """The consensus VCF of a group at level k, from the members' kept lines (the texts of their <x>.filtered.vcf, in member
    order): the '#' lines of the first member, then one line per key that at least k members call, in ascending key order
    (pos << 4 | ref << 2 | alt; truth and non-truth keys interleaved).  The line of a key is the first kept line carrying it in
    the lowest-numbered member that calls it, byte for byte; every line ends in a newline."""
    n = len(filtered_texts)
    check_group(range(n))
    if not 1 <= k <= n:
        raise ValueError("consensus level k = %d outside 1 .. n = %d" % (k, n))
    per = [member_keys(t) for t in filtered_texts]
    votes = {}
    for m in per:
        for key in m:
            votes[key] = votes.get(key, 0) + 1
    head = [ln for ln in _lines(filtered_texts[0]) if ln.startswith(b"#")]
    rows = []
    for key in sorted(votes):
        if votes[key] >= k:
            rows.append(next(m[key] for m in per if key in m))
    return b"".join(ln + b"\n" for ln in head + rows)


def _write_atomic(path, lines):
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)


def write_caller_consensus(path, per_sample):
    """final_tables/caller_consensus.tsv: `sample k n TP FP FN Precision Recall F1`, one row per sample (sorted) and level
    k = 1 .. n.  per_sample: {sample: (n, tp_votes, fp_votes)}.  Written atomically."""
    lines = ["\t".join(["sample", "k", "n", "TP", "FP", "FN", "Precision", "Recall", "F1"])]
    for sample in sorted(per_sample):
        n, tpv, fpv = per_sample[sample]
        for k, tp, fp, fn in level_counts(tpv, fpv, n):
            lines.append("\t".join([sample, str(k), str(n)] + [r_str(v) for v in level_row(tp, fp, fn)]))
    _write_atomic(path, lines)


def write_caller_private(path, per_sample):
    """final_tables/caller_private.tsv: `sample caller private_TP private_FP`, one row per sample (sorted) and member, in member
    order.  per_sample: {sample: (callers, private_tp, private_fp)}; caller names as caller_performance.tsv spells them."""
    lines = ["\t".join(["sample", "caller", "private_TP", "private_FP"])]
    for sample in sorted(per_sample):
        callers, ptp, pfp = per_sample[sample]
        for i, c in enumerate(check_group(callers)):
            lines.append("%s\t%s\t%d\t%d" % (sample, CALLER_MAP.get(c, c), int(ptp[i]), int(pfp[i])))
    _write_atomic(path, lines)
