"""Clusters of records matched by replayed haplotype: the unmatched records of a small region and the unmatched
truth entries of the same region are each replayed onto the genome; where the two sequences are equal, both sides are rescued.
The bounded core of what `rtg vcfeval` and hap.py's `xcmp` do: all or nothing per region.  Behind it, opt-in, a subset search
inside the regions that did not match (k_hap_subsets): `forms`, `search`, `subset_counts` below.

Everything here is the definition on strings, which k_hap_sites / k_hap_truth / k_hap_records / k_hap_claim / k_hap_replay
(csrc/qmvt_haplo.hip) restate on allele codes and the 4-bit packed genome; `counts` restates the pass's tables for one VCF; the
writer of caller_performance_haplotype.tsv follows.  The codec (`code`, `spell`) and the order of a truth set's allele-extended
table (`truth_order`) are those of quasimodo_amd.normalize.

Genome: one contig, G[p] 1-based, length L; ACGTacgt are bases (lower case counts as its upper case), every other byte is the one
symbol `N`, which equals itself only.
"""
import os
from bisect import bisect_left

import numpy as np

from .normalize import F_IDDOT, F_NOKEY, F_PASS, F_TPLINE, INLINE_MAX, code, spell, truth_order   # noqa: F401  (the flags and the codec: for the callers of this module)

MAX_GAP = 32                      # include/qmvt.h QM_HAP_MAX_GAP
DEFAULT_GAP = 10                  # QM_HAP_DEFAULT_GAP
MAX_WINDOW = 256                  # QM_HAP_MAX_WINDOW
MAX_ITEMS = 8                     # QM_HAP_MAX_ITEMS
POS_LIMIT = 1 << 28
# class bytes (QM_HAP_C_*): what became of a record or of a truth entry
(MATCHED, RESCUED, OUTSIDE, LONE, MISMATCH, CONFLICT, TOOMANY, TOOLONG, LONG, NOKEY, NOVAR, RANGE, REFMISMATCH,
 NOTKEPT) = range(14)
CLASS_NAMES = ("matched_spelling", "rescued", "outside", "lone", "mismatch", "conflict", "toomany", "toolong", "long", "nokey",
               "novar", "range", "refmismatch", "notkept")
REASONS = (LONG, NOKEY, NOVAR, RANGE, REFMISMATCH)
MATCH = RESCUED                   # the outcome of a site whose two replays are equal
# columns of the per-VCF tables (QM_HAP_R_* / QM_HAP_T_*)
R_COLS = ("kept", "tp", "tp_h", "rescued", "open") + CLASS_NAMES[OUTSIDE:NOTKEPT]
T_COLS = ("entries", "found", "found_h", "open", "unusable", "sites", "tried", "matched")

_BASES = "ACGT"


def check_gap(gap=None):
    """the gap g as an int (None: DEFAULT_GAP); ValueError unless 0 <= g <= MAX_GAP"""
    g = DEFAULT_GAP if gap is None else gap
    if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) <= MAX_GAP:
        raise ValueError("haplo: the gap is an integer from 0 to %d, not %r" % (MAX_GAP, gap))
    return int(g)


def symbols(genome):
    """the genome as a str over ACGTN"""
    s = genome.decode("latin-1") if isinstance(genome, (bytes, bytearray)) else str(genome)
    return "".join(c if c in _BASES else "N" for c in s.upper())


# ---- one variant ---------------------------------------------------------------------------------------------------------
def unusable(G, p, ref, alt, nokey=False):
    """None for a usable variant, else the first reason that applies.  G: symbols(genome); ref / alt: strings over ACGT of 1 ..
    INLINE_MAX bases, or None for an allele without an inline code"""
    if ref is None or alt is None:
        return LONG
    if nokey:
        return NOKEY
    if ref == alt:
        return NOVAR
    if p < 1 or p + len(ref) - 1 > len(G):
        return RANGE
    if G[p - 1:p - 1 + len(ref)] != ref:
        return REFMISMATCH
    return None


def trim(p, ref, alt):
    """the trimmed form (q, r, a): the longest common prefix goes first, then the longest common suffix of what is left"""
    m = min(len(ref), len(alt))
    cp = 0
    while cp < m and ref[cp] == alt[cp]:
        cp += 1
    cs = 0
    while cs < m - cp and ref[len(ref) - 1 - cs] == alt[len(alt) - 1 - cs]:
        cs += 1
    return p + cp, ref[cp:len(ref) - cs], alt[cp:len(alt) - cs]


def footprint(q, r):
    return q, max(q, q + len(r) - 1)


# ---- the sites of a (truth set, genome, gap) -------------------------------------------------------------------------------
def sites(G, entries, gap):
    """entries: [(p, ref, alt)] in the table's order, alleles as strings or None.  Returns (site_of [n] -- the site of every
    usable entry, -1 for the others --, [(first_entry, window_lo, window_hi)] per site).  A site's entries are the usable ones
    among first_entry .. the next site's first_entry - 1."""
    site_of, out, spans = [], [], []
    top = None
    for j, (p, ref, alt) in enumerate(entries):
        if unusable(G, p, ref, alt) is not None:
            site_of.append(-1)
            continue
        lo, hi = footprint(*trim(p, ref, alt)[:2])
        if top is None or lo > top + 2 * gap:
            out.append(j)
            spans.append([lo, hi])
        else:
            spans[-1][0] = min(spans[-1][0], lo)
            spans[-1][1] = max(spans[-1][1], hi)
        top = hi if top is None else max(top, hi)
        site_of.append(len(out) - 1)
    L = len(G)
    return site_of, [(f, max(1, lo - gap), min(L + 1, hi + gap)) for f, (lo, hi) in zip(out, spans)]


def site_at(table, lo, hi, ends=None):
    """the site whose window holds the footprint [lo, hi], or -1: the first site whose window ends at or behind hi, if it starts
    at or before lo (window ends never descend; windows of different sites are disjoint but where a common prefix moved an
    entry's footprint behind the next entry's -- then the first such site is the record's)"""
    k = bisect_left([s[2] for s in table] if ends is None else ends, hi)
    return k if k < len(table) and table[k][1] <= lo else -1


# ---- one site --------------------------------------------------------------------------------------------------------------
def ordered(side):
    """the variants of a side -- spellings (p, ref, alt) -- as trimmed forms: identical spellings collapse, sorted by (q, |r|)"""
    return sorted((trim(*v) for v in set(side)), key=lambda t: (t[0], len(t[1])))


def conflicts(forms):
    return any(b[0] < a[0] + len(a[1]) or (b[0] == a[0] and not b[1]) for a, b in zip(forms, forms[1:]))


def replay(G, ws, we, forms):
    """the window [ws, we] of G with the ordered, conflict-free trimmed forms substituted"""
    out, cur = [], ws
    for q, r, a in forms:
        out.append(G[cur - 1:q - 1])
        out.append(a)
        cur = q + len(r)
    out.append(G[cur - 1:min(we, len(G))])
    return "".join(out)


def decide(G, ws, we, recs, ents):
    """(outcome, record replay, entry replay) of a tried site: recs / ents are the spellings of its open lines and open entries
    (duplicates and all).  The replays are None unless the outcome is MATCH or MISMATCH."""
    if len(recs) > MAX_ITEMS or len(ents) > MAX_ITEMS:
        return TOOMANY, None, None
    a, b = ordered(recs), ordered(ents)
    if conflicts(a) or conflicts(b):
        return CONFLICT, None, None
    x, y = replay(G, ws, we, a), replay(G, ws, we, b)
    return (MATCH if x == y else MISMATCH), x, y


# ---- the pass for one VCF ----------------------------------------------------------------------------------------------------
def counts(genome, truth, pos, ref, alt, flags, kept, tp, gap=None, detail=None):
    """The pass for one VCF, restated.  truth: (pos, ref, alt) code arrays of its truth set; kept / tp: the batch's masks as bool
    arrays.  Returns (rec [len(R_COLS)], tru [len(T_COLS)] uint64, cls uint8 [n], site int32 [n], entry_cls uint8 [entries]).
    detail: a list that receives (site, window_lo, window_hi, outcome, record indices, entry indices, record replay, entry
    replay) of every tried site."""
    g = check_gap(gap)
    G = symbols(genome)
    ent = truth_order(*truth)
    ent_s = [(p, spell(r), spell(a)) for p, r, a in ent]
    index = {e: j for j, e in enumerate(ent)}
    site_of, table = sites(G, ent_s, g)
    toolong = [hi - lo + 1 > MAX_WINDOW for _, lo, hi in table]
    ends = [s[2] for s in table]
    n = len(pos)
    rec, tru = np.zeros(len(R_COLS), np.uint64), np.zeros(len(T_COLS), np.uint64)
    cls, site = np.zeros(n, np.uint8), np.full(n, -1, np.int32)
    found = set()
    open_recs = {}
    col = {name: k for k, name in enumerate(R_COLS)}
    for i in range(n):
        f, p, r, a = int(flags[i]), int(pos[i]), int(ref[i]), int(alt[i])
        valid = all(0 <= x < 4 or x >= 0x08000000 for x in (r, a))
        hit = valid and not f & F_NOKEY and 0 <= p < POS_LIMIT and (p, r, a) in index
        rs, as_ = spell(r), spell(a)
        why = unusable(G, p, rs, as_, bool(f & F_NOKEY))
        if why is None:
            site[i] = site_at(table, *footprint(*trim(p, rs, as_)[:2]), ends)
        if hit:
            cls[i] = MATCHED
        elif why is not None:
            cls[i] = why
        elif not kept[i]:
            cls[i] = NOTKEPT
        elif site[i] < 0:
            cls[i] = OUTSIDE
        elif toolong[site[i]]:
            cls[i] = TOOLONG
        else:
            cls[i] = LONE                           # until its site says otherwise
            open_recs.setdefault(int(site[i]), []).append(i)
        if not kept[i]:
            continue
        rec[0] += 1
        rec[1] += bool(tp[i])
        rec[2] += bool(tp[i])
        if hit:
            found.add(index[(p, r, a)])
        elif why is not None:
            rec[col[CLASS_NAMES[why]]] += 1
        else:
            rec[col["outside" if site[i] < 0 else "open"]] += 1
    ecls = np.zeros(len(ent), np.uint8)
    open_ents = {}
    for j, e in enumerate(ent_s):
        why = unusable(G, *e)
        tru[4] += why is not None
        if j in found:
            ecls[j] = MATCHED
        elif why is not None:
            ecls[j] = why
        else:
            tru[3] += 1
            ecls[j] = TOOLONG if toolong[site_of[j]] else LONE
            if not toolong[site_of[j]]:
                open_ents.setdefault(site_of[j], []).append(j)
    tru[0], tru[1], tru[2], tru[5] = len(ent), len(found), len(found), len(table)
    for s, recs in sorted(open_recs.items()):
        ents = open_ents.get(s)
        if not ents:
            continue
        tru[6] += 1
        _, ws, we = table[s]
        what, x, y = decide(G, ws, we, [(int(pos[i]), spell(ref[i]), spell(alt[i])) for i in recs], [ent_s[j] for j in ents])
        cls[recs] = what
        ecls[ents] = what
        if what == MATCH:
            tru[7] += 1
            tru[2] += len(ents)
            for i in recs:
                if int(flags[i]) & F_IDDOT and not tp[i]:
                    rec[2] += 1
                    rec[3] += 1
        if detail is not None:
            detail.append((s, ws, we, what, list(recs), list(ents), x, y))
    for c in (LONE, MISMATCH, CONFLICT, TOOMANY, TOOLONG):
        rec[col[CLASS_NAMES[c]]] = int(((cls == c) & np.asarray(kept, bool)).sum())
    return rec, tru, cls, site, ecls


# ---- a subset search inside a mismatched site ---------------------------------------------------------------
# class bytes of the second arrays (QM_HAP_C_SUBSET / QM_HAP_C_LEFT): inside a PARTIAL site only
SUBSET, LEFT = 14, 15
SUB_CLASS_NAMES = CLASS_NAMES + ("subset", "left")
SUB_COLS = ("searched", "partial", "nosubset", "tp_s", "rescued_s", "found_s", "left_lines", "left_entries")   # QM_HAPSUB_*
SEARCHED_OUTCOMES = (MISMATCH, CONFLICT)


def form_key(f):
    """the total order of distinct trimmed forms: (q, |r|, |a|, a as a string over A<C<G<T)"""
    return f[0], len(f[1]), len(f[2]), f[2]


def forms(side):
    """the distinct trimmed forms of a side -- spellings (p, ref, alt) --: spellings that trim to one form collapse; in the total
    order of form_key.  Bit k of a side's mask is forms(side)[k]."""
    return sorted({trim(*v) for v in side}, key=form_key)


def conflict(a, b):
    """two forms, a before b in the order: b starts inside a's REF, or b is an insertion at a's start"""
    return b[0] < a[0] + len(a[1]) or (b[0] == a[0] and not b[1])


def subset(fs, mask):
    return [f for k, f in enumerate(fs) if mask >> k & 1]


def admissible(fs, mask):
    """no two forms of the subset conflict (the neighbour test: `conflicts` on the subset in order)"""
    return mask != 0 and not conflicts(subset(fs, mask))


def _bits(m):
    return bin(m).count("1")


def search(G, ws, we, recs, ents):
    """The optimum of a site: recs / ents are the spellings of its open lines and open entries (at most MAX_ITEMS each).  A
    candidate is a non-empty admissible subset S of the line forms and one T of the entry forms whose replays over [ws, we] are
    equal; the optimum has the largest |S| + |T|, then the larger |T|, then the smallest S mask, then the smallest T mask.
    Returns (S mask, T mask, line forms, entry forms, the replay) or None."""
    if len(recs) > MAX_ITEMS or len(ents) > MAX_ITEMS:
        raise ValueError("haplo.search: %d lines and %d entries (at most %d each)" % (len(recs), len(ents), MAX_ITEMS))
    fa, fb = forms(recs), forms(ents)
    by_replay = {}
    for mt in range(1, 1 << len(fb)):
        if admissible(fb, mt):
            by_replay.setdefault(replay(G, ws, we, subset(fb, mt)), []).append(mt)
    best = None
    for ms in range(1, 1 << len(fa)):
        if not admissible(fa, ms):
            continue
        x = replay(G, ws, we, subset(fa, ms))
        for mt in by_replay.get(x, ()):
            key = (-(_bits(ms) + _bits(mt)), -_bits(mt), ms, mt)
            if best is None or key < best[0]:
                best = (key, x)
    return None if best is None else (best[0][2], best[0][3], fa, fb, best[1])


def subset_counts(genome, truth, pos, ref, alt, flags, kept, tp, gap=None, detail=None, counted=None):
    """The search behind the pass for one VCF, restated.  counted: (what `counts` returned, the list its detail= filled) for
    the same arguments, or None: `counts` runs here.  Returns (sub [len(SUB_COLS)] uint64, cls_s uint8 [n], ecls_s uint8
    [entries]): the count block and the second class bytes -- the pass's own but inside PARTIAL sites, where they are SUBSET
    or LEFT.  detail: a list that receives (site, S mask, T mask, rescued record indices, left record indices, found entry
    indices, left entry indices, the replay) of every PARTIAL site, sites ascending."""
    if counted is None:
        tried = []
        res = counts(genome, truth, pos, ref, alt, flags, kept, tp, gap, tried)
    else:
        res, tried = counted
    rec, tru, cls, _, ecls = res
    G = symbols(genome)
    ent_s = [(p, spell(r), spell(a)) for p, r, a in truth_order(*truth)]
    sub = np.zeros(len(SUB_COLS), np.uint64)
    cls_s, ecls_s = cls.copy(), ecls.copy()
    sub[3], sub[5] = rec[2], tru[2]
    for s, ws, we, what, recs, ents, _, _ in tried:
        if what not in SEARCHED_OUTCOMES:
            continue
        sub[0] += 1
        spelled = [(int(pos[i]), spell(ref[i]), spell(alt[i])) for i in recs]
        got = search(G, ws, we, spelled, [ent_s[j] for j in ents])
        if got is None:
            sub[2] += 1
            continue
        ms, mt, fa, fb, x = got
        sub[1] += 1
        chosen_a, chosen_b = set(subset(fa, ms)), set(subset(fb, mt))
        inr = [i for i, v in zip(recs, spelled) if trim(*v) in chosen_a]
        outr = [i for i in recs if i not in inr]
        ine = [j for j in ents if trim(*ent_s[j]) in chosen_b]
        oute = [j for j in ents if j not in ine]
        cls_s[inr], cls_s[outr], ecls_s[ine], ecls_s[oute] = SUBSET, LEFT, SUBSET, LEFT
        sub[3] += sum(1 for i in inr if int(flags[i]) & F_IDDOT and not tp[i])
        sub[4] += len(inr)
        sub[5] += len(ine)
        sub[6] += len(outr)
        sub[7] += len(oute)
        if detail is not None:
            detail.append((s, ms, mt, inr, outr, ine, oute, x))
    return sub, cls_s, ecls_s


def truth_sites(genome, truth, gap=None):
    """(first_entry, lo, hi) int32 arrays: the sites of a truth set, what qm_truth_sites returns"""
    ent_s = [(p, spell(r), spell(a)) for p, r, a in truth_order(*truth)]
    table = sites(symbols(genome), ent_s, check_gap(gap))[1]
    return tuple(np.array([t[k] for t in table], np.int32).reshape(len(table)) for k in range(3))


# ---- files and tables ----------------------------------------------------------------------------------------------------------
SITES_HEADER = "#site\tWIN_LO\tWIN_HI\tLINES\tENTRIES\tREPLAY_LINES\tREPLAY_TRUTH"


def sites_path(job):
    """the MATCH sites of a job beside fp/ and tp/: hap/<x>.sites.tsv"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "hap", base[:-len(".fp.vcf")] + ".sites.tsv")


SUBSETS_HEADER = "#site\tWIN_LO\tWIN_HI\tRESCUED\tLEFT_LINES\tFOUND\tLEFT_ENTRIES\tREPLAY_LINES\tREPLAY_TRUTH"


def subsets_path(job):
    """the PARTIAL sites of a job beside its sites file: hap/<x>.subsets.tsv"""
    return sites_path(job)[:-len(".sites.tsv")] + ".subsets.tsv"


def read_subsets(path):
    """[(site, window_lo, window_hi, the lines rescued by subset and the lines left as [(line number in the input VCF, POS, REF,
    ALT as the line spells them)], the entries found by subset and the entries left as [(pos, ref, alt)], the replay of the
    chosen lines, the replay of the chosen entries)]; an empty list is written as `.`"""
    with open(path, newline="\n") as fh:
        lines = fh.read().split("\n")
    if lines[0] != SUBSETS_HEADER or lines[-1] != "":
        raise ValueError("%s: not a subsets file (header %r)" % (path, lines[0]))
    cells = lambda c: [] if c == "." else [y.split(":") for y in c.split(";")]
    out = []
    for k, ln in enumerate(lines[1:-1]):
        r = ln.split("\t")
        if len(r) != 9:
            raise ValueError("%s row %d: %r" % (path, k + 1, ln))
        recs = [[(int(x[0]), x[1], x[2], x[3]) for x in cells(c)] for c in r[3:5]]
        ents = [[(int(x[0]), x[1], x[2]) for x in cells(c)] for c in r[5:7]]
        out.append((int(r[0]), int(r[1]), int(r[2]), recs[0], recs[1], ents[0], ents[1], r[7], r[8]))
    return out


def read_sites(path):
    """[(site, window_lo, window_hi, [(line number in the input VCF, POS, REF, ALT as the line spells them)], [(pos, ref, alt) of
    the entries found by haplotype], the replay of the lines, the replay of the entries)]"""
    with open(path, newline="\n") as fh:
        lines = fh.read().split("\n")
    if lines[0] != SITES_HEADER or lines[-1] != "":
        raise ValueError("%s: not a sites file (header %r)" % (path, lines[0]))
    out = []
    for k, ln in enumerate(lines[1:-1]):
        r = ln.split("\t")
        if len(r) != 7:
            raise ValueError("%s row %d: %r" % (path, k + 1, ln))
        recs = [(int(x[0]), x[1], x[2], x[3]) for x in (y.split(":") for y in r[3].split(";"))]
        ents = [(int(x[0]), x[1], x[2]) for x in (y.split(":") for y in r[4].split(";"))]
        out.append((int(r[0]), int(r[1]), int(r[2]), recs, ents, r[5], r[6]))
    return out


TABLE_HEADER = (("caller", "mixture"), (("TP", "FP", "FN", "Precision", "Recall", "F1", "TP_H", "FP_H", "FN_H", "Precision_H", "Recall_H", "F1_H")
                + R_COLS[3:] + ("truth_entries", "truth_open", "truth_unusable", "sites", "sites_tried", "sites_matched")))


def performance_row(rec, tru):
    """One VCF's rows of the pass -> TP, FP, FN, Precision, Recall, F1 by spelling, the same six by haplotype, then the class
    counts and the truth set's sizes.  The call side counts lines (TP / TP_H lines out of the kept lines), the truth side counts
    entries (found / found by spelling or haplotype, out of the entries); the ratios with the rounding of tables.py; None = NA."""
    from .tables import r_div, r_round3
    rec, tru = [int(x) for x in rec], [int(x) for x in tru]
    kept, entries = rec[0], tru[0]
    out = []
    for tp, hit in ((rec[1], tru[1]), (rec[2], tru[2])):
        if kept == 0:
            out += [0, 0, entries - hit, None, None, None]
            continue
        p, r = r_round3(r_div(tp, kept)), r_round3(r_div(hit, entries))
        out += [tp, kept - tp, entries - hit, p, r, r_round3(r_div(2 * (p * r), p + r))]
    return out + rec[3:] + [tru[0], tru[3], tru[4], tru[5], tru[6], tru[7]]


SUBSETS_TABLE_HEADER = (("caller", "mixture"), (TABLE_HEADER[1][:12] + ("TP_S", "FP_S", "FN_S", "Precision_S", "Recall_S", "F1_S")
                        + ("sites_searched", "sites_partial", "sites_nosubset", "rescued_S", "left_lines", "left_entries")))


def performance_row_subsets(rec, tru, sub):
    """One VCF's rows of the pass and of the search -> TP, FP, FN, Precision, Recall, F1 by spelling, by haplotype (_H) and by
    subset (_S: TP_S lines out of the kept lines, FOUND_S entries out of the entries), then the six counts of the search;
    ratios and NA as performance_row"""
    from .tables import r_div, r_round3
    sub = [int(x) for x in sub]
    kept, entries = int(rec[0]), int(tru[0])
    out = performance_row(rec, tru)[:12]
    if kept == 0:
        out += [0, 0, entries - sub[5], None, None, None]
    else:
        p, r = r_round3(r_div(sub[3], kept)), r_round3(r_div(sub[5], entries))
        out += [sub[3], kept - sub[3], entries - sub[5], p, r, r_round3(r_div(2 * (p * r), p + r))]
    return out + [sub[0], sub[1], sub[2], sub[4], sub[6], sub[7]]


def write_performance_hapsubsets(path, rows, custom=False):
    """final_tables/caller_performance_hapsubsets.tsv (custom: without the mixture column).  rows: iterable of (caller_lower or
    label, sample, stats) with stats["hap_rec"] / stats["hap_tru"] / stats["hap_sub"]; jobs without them are left out.  Written
    atomically."""
    from .tables import CALLER_MAP, r_str
    head = (SUBSETS_TABLE_HEADER[0][:1] if custom else SUBSETS_TABLE_HEADER[0]) + SUBSETS_TABLE_HEADER[1]
    lines = ["\t".join(head)]
    for caller, sample, stats in rows:
        if "hap_sub" not in stats:
            continue
        name = [caller] if custom else [CALLER_MAP.get(caller, caller), sample]
        lines.append("\t".join(name + [r_str(v) for v in performance_row_subsets(stats["hap_rec"], stats["hap_tru"], stats["hap_sub"])]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)


def write_performance_haplotype(path, rows, custom=False):
    """final_tables/caller_performance_haplotype.tsv (custom: without the mixture column).  rows: iterable of (caller_lower or
    label, sample, stats) with stats["hap_rec"] / stats["hap_tru"]; jobs without them (pure-strain samples) are left out.
    Written atomically."""
    from .tables import CALLER_MAP, r_str
    head = (TABLE_HEADER[0][:1] if custom else TABLE_HEADER[0]) + TABLE_HEADER[1]
    lines = ["\t".join(head)]
    for caller, sample, stats in rows:
        if "hap_rec" not in stats:
            continue
        name = [caller] if custom else [CALLER_MAP.get(caller, caller), sample]
        lines.append("\t".join(name + [r_str(v) for v in performance_row(stats["hap_rec"], stats["hap_tru"])]))
    tmp = "%s.tmp.%d" % (path, os.getpid())
    with open(tmp, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    os.replace(tmp, path)
