"""Edge families of the haplotype tests, beside the planted family of haplo_family.py: inputs built so that the
mechanisms of qmvt_haplo.hip leave their first iteration -- the step seams of k_hap_sites, the words, steps and VCFs of
k_hap_rank, a second block of k_hap_pairs, a second and third gather round of k_hap_replay, both ends of the genome, bytes that
are no base, every pair of inline allele lengths, overlapping windows.  Plain Python over strings; `codes`, `truth_codes` and
`host_masks` are those of haplo_family.py.  Every family comes with a `present` check: what it plants is asserted on the
restatement's output (and on the truth set's sorted order), so that a generator that drifts fails instead of passing vacuously.
The checks are shared by the host test and the device test."""
import functools

import numpy as np

from haplo_family import BASES, allele, codes, host_masks, truth_codes
from quasimodo_amd import haplo as hp

R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}
TRIED = (hp.MATCH, hp.MISMATCH, hp.CONFLICT, hp.TOOMANY)


def strip(ref, alt):
    """(cp, cs) by a loop over characters: the common prefix goes first, then the common suffix of what is left"""
    cp = 0
    while cp < len(ref) and cp < len(alt) and ref[cp] == alt[cp]:
        cp += 1
    r, a = ref[cp:], alt[cp:]
    cs = 0
    while cs < len(r) and cs < len(a) and r[len(r) - 1 - cs] == a[len(a) - 1 - cs]:
        cs += 1
    return cp, cs


def line(p, r, a, kept=True, extra=hp.F_IDDOT):
    return (p, r, a, kept, extra)


def rand_genome(rng, n):
    return [BASES[i] for i in rng.integers(0, 4, n)]


def at(g, p, n=1):
    return "".join(g[p - 1:p - 1 + n]).upper()


def snv(g, p, k=1):
    """the k-th of the three SNVs at p"""
    ref = at(g, p)
    return (p, ref, BASES[(BASES.index(ref) + k) % 4])


def prefixed(g, v):
    """the same variant spelled with one more shared base in front"""
    p, r, a = v
    c = at(g, p - 1)
    assert p >= 2 and c in BASES and max(len(r), len(a)) < hp.INLINE_MAX
    return (p - 1, c + r, c + a)


class Edge:
    """name; genome: str; truths: [[(p, REF, ALT)]]; vcfs: [(tag, index of its truth set, [(p, REF, ALT, kept, flags beyond
    PASS)], has a genome)]; gaps: the gaps it is built for; planted: what `present` looks for.  shuffle: the tags that get a
    twin with the same records in a shuffled order (twin: {its index: (the index of the sorted one, the permutation)})."""

    def __init__(self, name, genome, truths, vcfs, gaps, planted=None, shuffle=()):
        self.name, self.genome, self.truths, self.gaps, self.planted = name, "".join(genome), truths, tuple(gaps), planted or {}
        self.vcfs, self.twin = list(vcfs), {}
        rng = np.random.default_rng(len(name) + 7)
        for tag in shuffle:
            v = self.index(tag)
            perm = list(range(len(self.vcfs[v][2])))
            rng.shuffle(perm)
            self.twin[len(self.vcfs)] = (v, perm)
            self.vcfs.append((tag + "_shuffled", self.vcfs[v][1], [self.vcfs[v][2][i] for i in perm], True))
        self.tcodes = [truth_codes(t) for t in truths]
        self.cols = [codes(v[2]) for v in self.vcfs]
        self.order = [hp.truth_order(*t) for t in self.tcodes]      # the table order of every truth set, on codes

    def index(self, tag):
        return [v[0] for v in self.vcfs].index(tag)

    def entry_index(self, w, p, ref, alt):
        """where the entry sits in the sorted table of truth set w"""
        return self.order[w].index((p, allele(ref), allele(alt)))

    def restate(self, v, gap, masks=None):
        """hp.counts of VCF v at `gap` (masks: the batch's kept and TP masks; None: host_masks) + the detail of its tried sites"""
        c, w = self.cols[v], self.vcfs[v][1]
        kept, tp = host_masks(c, self.tcodes[w]) if masks is None else masks
        detail = []
        return hp.counts(self.genome, self.tcodes[w], c[0], c[1], c[2], c[4], kept, tp, gap, detail) + (detail,)


# ---- (a) every pair of inline lengths ------------------------------------------------------------------------------------------
def trim_targets(lr, la):
    """the (cp, cs) to plant for |REF| = lr, |ALT| = la: both extremes of either, one interior value, the single differing base"""
    m = min(lr, la)
    out = set()
    for cp in (0, m - 1, m, m // 2):
        for cs in (0, m - cp, (m - cp) // 2, m - cp - 1):
            if 0 <= cp <= m and 0 <= cs <= m - cp and not (lr == la and cp + cs >= m):
                out.add((cp, cs))
    return sorted(out)


def spell_pair(rng, lr, la, cp, cs):
    """(REF, ALT) of these lengths whose common prefix and suffix are exactly cp and cs, or None where there is none"""
    pick = lambda n: "".join(BASES[i] for i in rng.integers(0, 4, n))
    for _ in range(400):
        pre, suf = pick(cp), pick(cs)
        ref, alt = pre + pick(lr - cp - cs) + suf, pre + pick(la - cp - cs) + suf
        if ref != alt and strip(ref, alt) == (cp, cs):
            return ref, alt
    return None


def trim_family():
    """Every (|REF|, |ALT|) in 1 .. 13 x 1 .. 13, each with the extreme and one interior (cp, cs), as isolated truth entries in
    slots of 40 bases (a site of its own at g = 0 and at g = 10); one record per entry that respells it with a shorter or a
    longer shared prefix (or a shorter shared suffix), every seventh with one ALT base changed; lengths 14 and 15: LONG."""
    rng = np.random.default_rng(41)
    slot = 40
    plan = [(lr, la, cp, cs) for lr in range(1, 14) for la in range(1, 14) for cp, cs in trim_targets(lr, la)]
    g = rand_genome(rng, slot * (len(plan) + 8))
    truth, recs, planted = [], [], []
    for k, (lr, la, cp, cs) in enumerate(plan):
        pair = spell_pair(rng, lr, la, cp, cs)
        if pair is None:
            continue
        ref, alt = pair
        p = slot * (k + 1) + 14
        g[p - 1:p - 1 + lr] = ref
        truth.append((p, ref, alt))
        planted.append((p, ref, alt, cp, cs))
    for k, (p, ref, alt, cp, cs) in enumerate(planted):
        lr, la = len(ref), len(alt)
        m = min(lr, la)
        if k % 7 == 3 and la - cp - cs > 0:                     # one ALT base changed (never into REF's base there)
            bad = [c for c in BASES if c != alt[cp] and (cp >= lr or c != ref[cp])][k % 2]
            alt = alt[:cp] + bad + alt[cp + 1:]
        d = min(cp, m - 1)
        if d >= 1 and k % 2 == 0:
            d = 1 if k % 4 == 0 else d
            recs.append(line(p + d, ref[d:], alt[d:]))          # a shorter shared prefix
        elif max(lr, la) < hp.INLINE_MAX:
            recs.append(line(*prefixed(g, (p, ref, alt))))      # a longer one
        elif d >= 1:
            recs.append(line(p + d, ref[d:], alt[d:]))
        elif cs >= 1 and m > 1:
            recs.append(line(p, ref[:-1], alt[:-1]))            # a shorter shared suffix
        else:
            recs.append(line(p, ref, alt))
    longs = []
    for k, (lr, la) in enumerate(((14, 1), (1, 15), (15, 14), (14, 14))):
        p = slot * (len(plan) + 2 + k) + 14
        ref = at(g, p, lr)
        alt = (ref[0] + "ACGTTGCAACGTTGCA")[:la] if la > 1 else BASES[(BASES.index(ref[0]) + 1) % 4]
        truth.append((p, ref, alt))
        longs.append((p, ref, alt))
        recs.append(line(p + 1, at(g, p + 1, lr), alt))
    return Edge("trim", g, [truth], [("respelled", 0, recs, True)], (0, 10), {"forms": planted, "longs": longs}, shuffle=("respelled",))


def present_trim(e, res):
    forms = e.planted["forms"]
    seen = {}
    for p, ref, alt, cp, cs in forms:
        assert strip(ref, alt) == (cp, cs) and at(e.genome, p, len(ref)) == ref
        seen.setdefault((len(ref), len(alt)), set()).add((cp, cs))
    for lr in range(1, 14):
        for la in range(1, 14):
            m, got = min(lr, la), seen.get((lr, la), set())
            assert any(cp == 0 and cs == 0 for cp, cs in got), (lr, la)
            assert any(cp == (m if lr != la else m - 1) for cp, cs in got), (lr, la)
            assert any(cs == m - cp - (lr == la) for cp, cs in got), (lr, la)
            if lr == la and lr >= 3:                            # the single differing base first, last and in the middle
                assert {(0, m - 1), (m - 1, 0), (m // 2, m - m // 2 - 1)} <= got, (lr, la)
    for gap in e.gaps:
        rec, tru, cls, site, ecls, detail = res[(0, gap)]
        assert int(tru[T["sites"]]) == len(forms) and int(tru[T["unusable"]]) == len(e.planted["longs"])   # every entry a site of its own
        assert int(tru[T["matched"]]) >= 500 and int(tru[T["tried"]]) - int(tru[T["matched"]]) >= 50
        assert int(rec[R["long"]]) >= 3 and all(len(d[4]) == 1 and len(d[5]) == 1 for d in detail)


def check_normal_form_tie(e, v, gap, hap, first, ncls, nrow):
    """The tie of the trim family to the normal-form pass (4.17) -- see normal_form_tie in test_gpu_haplo_edges.py for the
    derivation.  hap: (class bytes, site indices, entry classes) of VCF v at `gap`; first: the first entry of every site; ncls,
    nrow: the class bytes and truth rows of the normal-form pass for the same records."""
    from quasimodo_amd import normalize as nm
    cls, site, ecls = hap
    flags = e.cols[v][4]
    assert set(e.genome) <= set(BASES) and min(e.cols[v][0]) > 1
    assert ((flags & hp.F_PASS) != 0).all() and ((flags & hp.F_IDDOT) != 0).all() and ((flags & hp.F_TPLINE) == 0).all()
    ends = np.append(first[1:], len(ecls))
    lines_of = np.bincount(site[np.isin(cls, TRIED)], minlength=len(first))
    tried_entries = np.isin(ecls, TRIED).astype(np.int64)
    entries_of = np.add.reduceat(tried_entries, first)
    n_match = n_mismatch = 0
    for i in np.flatnonzero(np.isin(cls, (hp.MATCH, hp.MISMATCH))):
        s = int(site[i])
        if lines_of[s] != 1 or entries_of[s] != 1:
            continue
        j = int(first[s] + np.flatnonzero(tried_entries[first[s]:ends[s]])[0])
        rescued = ncls[i] == nm.RESCUED
        if rescued and nrow[i] != j:
            continue                                            # its form is an entry of another site
        case = "line %d of VCF %d, gap %d" % (i, v, gap)
        if cls[i] == hp.MATCH:
            assert rescued and nrow[i] == j, case
            n_match += 1
        else:
            assert not rescued, case
            n_mismatch += 1
    assert n_match >= 500 and n_mismatch >= 50, (v, gap, n_match, n_mismatch)
    for i in np.flatnonzero((ncls == nm.RESCUED) & np.isin(cls, TRIED)):    # rescued by normal form and tried here with its own entry: MATCH
        s = int(site[i])
        if lines_of[s] == 1 and entries_of[s] == 1 and first[s] <= nrow[i] < ends[s]:
            assert cls[i] == hp.MATCH, "line %d of VCF %d, gap %d" % (i, v, gap)


# ---- (b) the seams of k_hap_sites ------------------------------------------------------------------------------------------------
SEAM_GAP = 2
DEL_OFFS = (1, 6, 11, 16)


class Table:
    """a truth table built in ascending positions, one entry per position: the index of an entry is its place in the list"""

    def __init__(self, g, at_pos=30):
        self.g, self.p, self.ent = g, at_pos, []

    def fill(self, upto):                                      # isolated SNVs (more than 2 g apart) until the table holds `upto` entries
        while len(self.ent) < upto:
            self.ent.append(snv(self.g, self.p))
            self.p += 12

    def add(self, v, step):
        self.ent.append(v)
        self.p = v[0] + step

    def bad_ref(self, step=3):                                 # REFMISMATCH: the REF is not the genome's base
        c = at(self.g, self.p)
        self.add((self.p, BASES[(BASES.index(c) + 1) % 4], c), step)

    def long(self, step=3):                                    # LONG: a REF of 14 bases
        self.add((self.p, at(self.g, self.p, 14), at(self.g, self.p)), step)


def seam_records(g, table, special=()):
    """by the index of the entry: spelled alike, another ALT at its position, respelled with one more base in front, nothing"""
    recs = []
    for i, v in enumerate(table):
        if i in special or len(v[1]) != 1 or len(v[2]) != 1 or at(g, v[0]) != v[1]:
            continue
        if i % 4 == 0:
            recs.append(line(*v))
        elif i % 4 == 1:
            recs.append(line(*snv(g, v[0], 2)))
        elif i % 4 == 2:
            recs.append(line(*prefixed(g, v)))
    return recs


def seam_family():
    rng = np.random.default_rng(43)
    g = rand_genome(rng, 14000)
    # table 0: 4 * 256 + 1 entries; sites across 255|256 and 511|512; a deletion at 766 whose footprint carries cmax over the seam
    t = Table(g)
    t.fill(253)
    x = t.p
    for k in range(6):                                         # 253 .. 258: six adjacent SNVs, one site
        t.add(snv(g, x + k), 1)
    t.p += 12
    t.fill(509)
    y = t.p
    for k in range(6):                                         # 509 .. 514: SNVs three bases apart, one site
        t.add(snv(g, y + 3 * k), 3)
    t.p += 12
    t.fill(766)
    d = t.p
    t.add((d, at(g, d, 13), at(g, d)), 1)                      # 766: q = d + 1, |r| = 12, hi = d + 12
    for off in DEL_OFFS:                                       # 767 .. 770: each more than 2 g behind the one before, inside hi + 2 g
        t.add(snv(g, d + off), 0)
    t.p = d + 16 + 12
    t.fill(1025)
    t0 = t.ent
    special = set(range(253, 259)) | set(range(766, 771))
    r0 = seam_records(g, t0, special)
    r0.append(line(x, at(g, x, 6), "".join(snv(g, x + k)[2] for k in range(6))))        # the six SNVs as one MNP: MATCH
    r0 += [line(*t0[766]), line(*t0[767]), line(*prefixed(g, t0[768])), line(*t0[769]), line(*snv(g, d + 16, 2))]
    r0.sort(key=lambda r: r[0])
    # table 1: 4 * 256 entries; REFMISMATCH at 255 and LONG at 256 inside one site (254 and 257 usable), again alone at 511 | 512
    t = Table(g)
    t.fill(254)
    t.add(snv(g, t.p), 1)
    t.bad_ref(1)
    t.long(1)
    t.add(snv(g, t.p), 12)
    t.fill(511)
    t.bad_ref(12)
    t.long(12)
    t.fill(1024)
    t1 = t.ent
    r1 = seam_records(g, t1)
    # table 2: no usable entry in its first 256 rows
    t = Table(g)
    for k in range(256):
        (t.bad_ref if k % 2 else t.long)()
    z = t.p
    for k in range(4):
        t.add(snv(g, z + k), 1)
    t.p += 12
    t.fill(300)
    t2 = t.ent
    r2 = seam_records(g, t2, set(range(256, 260))) + [line(z, at(g, z, 4), "".join(snv(g, z + k)[2] for k in range(4)))]
    r2.sort(key=lambda r: r[0])
    # table 3: no usable entry at all
    t = Table(g)
    for k in range(6):
        (t.bad_ref if k % 2 else t.long)(12)
    t3 = t.ent
    r3 = [line(*snv(g, 40 + 9 * k)) for k in range(9)] + [line(200, at(g, 200, 14), "A"), line(210, BASES[(BASES.index(at(g, 210)) + 2) % 4], at(g, 210))]
    planted = {"straddle": (x, y), "deletion": d, "first_usable": z}
    return Edge("seams", g, [t0, t1, t2, t3], [("n1025", 0, r0, True), ("n1024", 1, r1, True), ("late", 2, r2, True), ("none", 3, r3, True)],
                (SEAM_GAP,), planted, shuffle=("n1025",))


def present_seams(e, res):
    g, gap = e.genome, SEAM_GAP
    G = hp.symbols(g)
    spelled = [[(p, hp.spell(r), hp.spell(a)) for p, r, a in o] for o in e.order]
    site_of = [hp.sites(G, s, gap)[0] for s in spelled]
    x, y = e.planted["straddle"]
    d = e.planted["deletion"]
    assert [len(o) for o in e.order] == [1025, 1024, 300, 6]                   # a multiple of 256 plus one; a multiple
    # table 0, read from the sorted order
    ix = [e.entry_index(0, *snv(g, x + k)) for k in range(6)]
    assert ix == list(range(253, 259)) and len({site_of[0][i] for i in ix}) == 1   # one site over 255 | 256
    iy = [e.entry_index(0, *snv(g, y + 3 * k)) for k in range(6)]
    assert iy == list(range(509, 515)) and len({site_of[0][i] for i in iy}) == 1   # ... and over 511 | 512
    i_del = e.entry_index(0, d, at(g, d, 13), at(g, d))
    behind = [e.entry_index(0, *snv(g, d + off)) for off in DEL_OFFS]
    assert i_del == 766 and behind == [767, 768, 769, 770] and len({site_of[0][i] for i in [i_del] + behind}) == 1
    for a, b in zip(DEL_OFFS, DEL_OFFS[1:]):                    # 768 .. 770: more than 2 g behind the end of the entry before each,
        assert d + b > d + a + 2 * gap and d + b <= d + 12 + 2 * gap   # inside the deletion's end + 2 g: only the carried maximum keeps them
    assert site_of[0][771] == site_of[0][770] + 1
    # table 1: unusable at 255 and 256 inside a site, and alone at 511 and 512
    why = lambda w, i: hp.unusable(G, *spelled[w][i])
    assert [why(1, i) for i in (254, 255, 256, 257)] == [None, hp.REFMISMATCH, hp.LONG, None]
    assert site_of[1][254] == site_of[1][257] >= 0 and site_of[1][255] == site_of[1][256] == -1
    assert [why(1, i) for i in (511, 512)] == [hp.REFMISMATCH, hp.LONG]
    # table 2: the first usable entry is row 256; table 3: none
    assert all(why(2, i) is not None for i in range(256)) and why(2, 256) is None and site_of[2][256] == 0
    assert all(why(3, i) is not None for i in range(6))
    out = {tag: res[(e.index(tag), gap)] for tag in ("n1025", "n1024", "late", "none")}
    rec, tru, cls, site, ecls, detail = out["n1025"]
    s = site_of[0][255]
    assert any(dt[0] == s and dt[3] == hp.MATCH and len(dt[5]) == 6 for dt in detail)            # tried across the seam: MATCH
    assert any(dt[0] == site_of[0][766] and dt[5] == [768, 770] for dt in detail) and any(dt[0] == site_of[0][511] for dt in detail)
    assert int(tru[T["matched"]]) >= 200 and int(tru[T["tried"]]) - int(tru[T["matched"]]) >= 200
    rec, tru, cls, site, ecls, detail = out["n1024"]
    assert ecls[255] == hp.REFMISMATCH and ecls[256] == hp.LONG and int(tru[T["unusable"]]) == 4
    rec, tru, cls, site, ecls, detail = out["late"]
    assert int(tru[T["unusable"]]) == 256 and detail[0][0] == 0 and detail[0][3] == hp.MATCH and detail[0][5] == [256, 257, 258, 259]
    rec, tru, cls, site, ecls, detail = out["none"]
    assert int(tru[T["sites"]]) == 0 and int(tru[T["tried"]]) == 0 and not detail and int(tru[T["unusable"]]) == 6
    assert int(rec[R["outside"]]) == 9 and int(rec[R["long"]]) == 1 and int(rec[R["refmismatch"]]) == 1 and (site == -1).all()


# ---- (c) rank and pairs across words, steps and VCFs -----------------------------------------------------------------------------
RANK_SITES = 8192 + 45


def rank_family():
    """8237 single-entry sites (g = 1, eight bases apart): 258 words of the site bitmap -- two steps of k_hap_rank, two blocks of
    k_hap_pairs.  Five VCFs: three on this truth set with different open sets, one on a small second truth set between them, one
    without a genome."""
    n = RANK_SITES
    rng = np.random.default_rng(47)
    g = rand_genome(rng, 10 + 8 * n + 30)
    big = [snv(g, 10 + 8 * j) for j in range(n)]
    small = [snv(g, 14 + 8 * j) for j in range(40)]

    def vcf(truth, found, opened):                              # opened(j): 0 nothing, 1 respelled (MATCH), 2 another ALT (MISMATCH)
        recs = []
        for j, v in enumerate(truth):
            if found(j):
                recs.append(line(*v))
            elif opened(j) == 1:
                recs.append(line(*prefixed(g, v)))
            elif opened(j) == 2:
                recs.append(line(*snv(g, v[0], 2)))
        return recs

    sparse_open = [0, 31, 32, 63, 64, 254 * 32 + 31, 255 * 32, 255 * 32 + 31, 256 * 32, 256 * 32 + 31, 257 * 32, n - 1]
    sparse = vcf(big, lambda j: j not in sparse_open, lambda j: 1 + sparse_open.index(j) % 2)
    dense = vcf(big, lambda j: j % 3 == 0, lambda j: (2 - j % 2) if j % 3 == 1 else 0)
    tail = vcf(big, lambda j: j < 8100 and j % 2 == 1 and j != 31, lambda j: 1 + j % 2 if j >= 8100 else {0: 2, 31: 1, 32: 1}.get(j, 0))
    little = vcf(small, lambda j: j % 2 == 0, lambda j: 1 + (j % 4 == 1))
    return Edge("rank", g, [big, small], [("sparse", 0, sparse, True), ("small", 1, little, True), ("dense", 0, dense, True),
                                          ("nogenome", 0, sparse[:101], False), ("tail", 0, tail, True)],
                (1,), {"sparse_open": sparse_open}, shuffle=("dense",))


def present_rank(e, res):
    n = RANK_SITES
    assert len(e.order[0]) == n > 8192 + 32 and (n + 31) // 32 == 258 and n % 32 == 13        # a last, partial word
    assert [v[0] for v in e.vcfs[:5]] == ["sparse", "small", "dense", "nogenome", "tail"]       # the small truth set sits between
    assert max(len(v[2]) for v in e.vcfs) <= 40000 and len(e.genome) < 100000
    rec, tru, cls, site, ecls, detail = res[(0, 1)]
    assert int(tru[T["sites"]]) == n and int(tru[T["open"]]) == 12
    assert [d[0] for d in detail] == e.planted["sparse_open"]                                   # bits 0, 31, 32; words 255, 256; the last word
    assert {d[0] // 32 for d in detail} >= {0, 1, 254, 255, 256, 257} and {d[0] % 32 for d in detail} >= {0, 31, 12}
    assert [d[3] for d in detail] == [hp.MATCH, hp.MISMATCH] * 6
    rec, tru, cls, site, ecls, detail = res[(2, 1)]
    assert int(tru[T["open"]]) > 5000 and int(tru[T["tried"]]) > 2500 and int(tru[T["matched"]]) > 1000
    assert int(tru[T["open"]]) - int(tru[T["tried"]]) > 2500                                    # open sites without an open line: pairs never tried
    assert detail[-1][0] >= 256 * 32
    rec, tru, cls, site, ecls, detail = res[(4, 1)]
    assert sum(d[0] >= 8192 for d in detail) == n - 8192 and {0, 31, 32} <= {d[0] for d in detail}
    assert {d[3] for d in detail} == {hp.MATCH, hp.MISMATCH}
    rec, tru, cls, site, ecls, detail = res[(1, 1)]
    assert int(tru[T["sites"]]) == 40 and int(tru[T["tried"]]) == 20 and int(tru[T["matched"]]) == 10


# ---- (d) sites with more than 64 entries -------------------------------------------------------------------------------------------
def dense_site(g, b, n):
    """n SNV entries from b on: one at b, then three at each position, what is left at the last one"""
    out, p = [snv(g, b)], b + 1
    while len(out) < n:
        out += [snv(g, p, k) for k in (1, 2, 3)][:n - len(out)]
        p += 1
    return out


def dense_family():
    rng = np.random.default_rng(53)
    g = rand_genome(rng, 1000)
    starts = {65: 100, 128: 400, 129: 700}
    truth = [v for n, b in starts.items() for v in dense_site(g, b, n)]
    tc = truth_codes(truth)
    order = [(p, hp.spell(r), hp.spell(a)) for p, r, a in hp.truth_order(*tc)]
    first = {n: min(i for i, v in enumerate(order) if v[0] >= b) for n, b in starts.items()}

    def vcf(plan):
        """plan: {n: (the in-site offsets that stay open, their lines)}; a line is ('same', offset) -- the entry respelled --,
        ('wrong', offset) -- respelled with another ALT --, ('mnp', offset, offset + 1, ...) -- adjacent entries as one MNP"""
        recs = []
        for n, (opened, lines) in plan.items():
            ent = order[first[n]:first[n] + n]
            recs += [line(*v) for o, v in enumerate(ent) if o not in opened]
            for ln in lines:
                if ln[0] == "same":
                    recs.append(line(*prefixed(g, ent[ln[1]])))
                elif ln[0] == "wrong":
                    p, r, a = ent[ln[1]]
                    recs.append(line(*prefixed(g, (p, r, [c for c in BASES if c not in (r, a)][0]))))
                else:
                    vs = [ent[o] for o in ln[1:]]
                    assert [v[0] for v in vs] == list(range(vs[0][0], vs[0][0] + len(vs)))
                    recs.append(line(vs[0][0], "".join(v[1] for v in vs), "".join(v[2] for v in vs)))
        recs.sort(key=lambda r: r[0])
        return recs

    eight = (0, 20, 63, 64, 90, 110, 125, 128)                 # rounds 0 .. 63, 64 .. 127, 128: three, four and one open entries
    same = lambda offs: tuple(("same", o) for o in offs)
    vcfs = [("match", 0, vcf({129: (eight, same((0, 20, 90, 110, 125, 128)) + (("mnp", 63, 64),)),
                              65: ((0, 63, 64), same((0,)) + (("mnp", 63, 64),)),
                              128: ((0, 63, 64, 127), same((0, 63, 64, 127)))}), True),
            ("toomany", 0, vcf({129: (eight + (40,), same((0,))),
                                65: ((0, 63, 64), same((0, 63)) + (("wrong", 64),)),
                                128: ((127,), (("wrong", 127),))}), True),
            ("mismatch", 0, vcf({129: ((0, 63, 64, 128), same((0, 63, 128)) + (("wrong", 64),)),
                                 65: ((64,), same((64,))),
                                 128: ((0, 64), same((0, 64)))}), True),
            ("conflict", 0, vcf({129: ((62, 63), same((62,))), 65: ((), ()), 128: ((63,), ())}), True)]
    return Edge("dense", g, [truth], vcfs, (10, 0), {"first": first, "eight": eight}, shuffle=("match", "mismatch"))


def present_dense(e, res):
    first = e.planted["first"]
    site_of, table = hp.sites(hp.symbols(e.genome), [(p, hp.spell(r), hp.spell(a)) for p, r, a in e.order[0]], 10)
    assert len(table) == 3 and sorted(first.values()) == [t[0] for t in table] and all(t[2] - t[1] + 1 <= 256 for t in table)
    sizes = sorted(site_of.count(s) for s in range(3))
    assert sizes == [65, 128, 129]
    s = {n: site_of[first[n]] for n in first}
    by = lambda tag: {d[0]: d for d in res[(e.index(tag), 10)][5]}
    m = by("match")
    assert m[s[129]][3] == hp.MATCH and [j - first[129] for j in m[s[129]][5]] == list(e.planted["eight"]) and len(m[s[129]][4]) == 7
    assert m[s[65]][3] == hp.MATCH and [j - first[65] for j in m[s[65]][5]] == [0, 63, 64]
    assert m[s[128]][3] == hp.MATCH and [j - first[128] for j in m[s[128]][5]] == [0, 63, 64, 127]
    t = by("toomany")
    assert t[s[129]][3] == hp.TOOMANY and len(t[s[129]][5]) == 9 and len(t[s[129]][4]) == 1
    assert t[s[65]][3] == hp.MISMATCH and t[s[128]][3] == hp.MISMATCH and [j - first[128] for j in t[s[128]][5]] == [127]
    x = by("mismatch")
    assert x[s[129]][3] == hp.MISMATCH and [j - first[129] for j in x[s[129]][5]] == [0, 63, 64, 128]
    assert x[s[65]][3] == hp.MATCH and [j - first[65] for j in x[s[65]][5]] == [64]
    assert x[s[128]][3] == hp.MATCH and [j - first[128] for j in x[s[128]][5]] == [0, 64]
    c = by("conflict")
    assert c[s[129]][3] == hp.CONFLICT and s[128] not in c and s[65] not in c
    assert int(res[(e.index("match"), 0)][1][T["sites"]]) > 100                                  # g = 0: neighbours are sites of their own


# ---- (e) both ends of the genome -------------------------------------------------------------------------------------------------
def ends_family(L):
    assert L % 8 in (0, 1, 7)
    rng = np.random.default_rng(59 + L)
    g = rand_genome(rng, L)
    g[:6] = "ACGTAC"
    g[L - 6:] = "ACGTCA"
    t0 = [(1, "A", "G"), (2, "CGT", "C"), (L - 2, "TCA", "T")]                 # an SNV at 1, a deletion anchored at 2, the last two bases deleted
    t1 = [(1, "A", "G"), (L, "A", "AAC")]                                      # ... and an insertion behind the last base: q = L + 1
    far = [line(0, "A", "C"), line(L - 1, "CAG", "C"), line(L, "AT", "A"), line(hp.POS_LIMIT - 1, "A", "C")]   # RANGE: one base past L; the
    wrap = lambda recs: [far[0]] + recs + far[1:]                              # smallest and the largest position a batch accepts
    vcfs = [("match", 0, wrap([line(1, "ACGT", "GC"), line(L - 3, "GTCA", "GT")]), True),
            ("mismatch", 0, wrap([line(1, "ACGT", "TC"), line(L - 1, "CA", "G")]), True),
            ("ins_match", 1, wrap([line(1, "AC", "GC"), line(L - 1, "CA", "CAAC")]), True),
            ("ins_mismatch", 1, wrap([line(1, "AC", "TC"), line(L - 1, "CA", "CAAG")]), True)]
    return Edge("ends%d" % (L % 8), g, [t0, t1], vcfs, (10, 0, 1), {"L": L}, shuffle=("match",))


def present_ends(e, res):
    L = e.planted["L"]
    assert len(e.genome) == L
    for gap in e.gaps:
        lo_end = {10: L - 11, 1: L - 2, 0: L - 1}[gap]
        d = res[(e.index("match"), gap)][5]
        if gap:
            assert [(x[1], x[2], x[3]) for x in d] == [(1, 4 + gap, hp.MATCH), (lo_end, L + 1, hp.MATCH)], (gap, d)   # clipped at 1 and at L + 1
        else:                                                   # g = 0: the record's footprint [1, 4] lies in neither [1, 1] nor [3, 4]
            assert [(x[1], x[2], x[3]) for x in d] == [(L - 1, L, hp.MATCH)]
        d = res[(e.index("mismatch"), gap)][5]
        assert [x[3] for x in d] == ([hp.MISMATCH] * 2 if gap else [hp.MISMATCH]) and d[-1][2] == (L + 1 if gap else L)
        d = res[(e.index("ins_match"), gap)][5]
        assert [(x[1], x[2], x[3]) for x in d] == [(1, 1 + gap, hp.MATCH), (L + 1 - gap, L + 1, hp.MATCH)]        # the window [L + 1, L + 1] at g = 0
        assert d[1][6] == d[1][7] == e.genome[L - gap:] + "AC"
        d = res[(e.index("ins_mismatch"), gap)][5]
        assert [x[3] for x in d] == [hp.MISMATCH] * 2
        for tag in ("match", "ins_mismatch"):
            assert int(res[(e.index(tag), gap)][0][R["range"]]) == 4


# ---- (f) bytes that are no base ----------------------------------------------------------------------------------------------------
NOBASE = ("N", "R", "-", "n", "y")


def nobase_family():
    """Per byte Z that is no base, four blocks in slots of 60 bases (each a site of its own at g = 10), the last two in lower case:
    ACCG Z TTA -- a C deleted in front of Z and a T inserted behind it, spelled on either base of the runs: the two sides read Z
                  behind pieces of different offsets and realign behind it: MATCH;
    AT Z TC    -- the T in front of Z deleted against the T behind it: A Z T C against A T Z C, a base against Z twice: MISMATCH
                  (equal where Z counts as T);
    AG Z C     -- an entry and a record whose REF spells T over Z: REFMISMATCH on both sides;
    acgt       -- lower case under an upper-case REF: usable.
    Z again six bases in front of every block: inside the window's flank."""
    rng = np.random.default_rng(61)
    g = rand_genome(rng, 60 * (4 * len(NOBASE) + 2))
    truth, recs, planted = [], [], []
    b = 80
    for k, z in enumerate(NOBASE):
        low = (lambda s: s.lower()) if k >= 3 else (lambda s: s)
        g[b - 1:b + 7] = low("ACCG") + z + low("TTA")
        g[b - 7] = z
        truth += [(b, "AC", "A"), (b + 5, "T", "TT")]
        recs += [line(b + 1, "CC", "C"), line(b + 6, "T", "TT")]
        planted.append(("match", b))
        b += 60
        g[b - 1:b + 4] = low("AT") + z + low("TC")
        g[b - 7] = z
        truth.append((b, "AT", "A"))
        recs.append(line(b + 3, "TC", "C"))
        planted.append(("mismatch", b))
        b += 60
        g[b - 1:b + 3] = low("AG") + z + low("C")
        truth.append((b + 1, "GTC", "G"))
        recs.append(line(b + 1, "GTC", "A"))
        planted.append(("refmismatch", b))
        b += 60
        g[b - 1:b + 3] = "acgt"
        g[b - 7] = z
        truth.append((b, "A", "G"))
        recs.append(line(b, "AC", "GC"))
        planted.append(("lower", b))
        b += 60
    return Edge("nobase", g, [truth], [("lines", 0, recs, True)], (10, 3), {"blocks": planted}, shuffle=("lines",))


def present_nobase(e, res):
    G = hp.symbols(e.genome)
    assert set(e.genome) - set("ACGTacgt") == set(NOBASE) and G.count("N") >= 6 * len(NOBASE)
    for gap in e.gaps:
        rec, tru, cls, site, ecls, detail = res[(0, gap)]
        at_lo = {}
        for d in detail:
            at_lo[d[1] + gap] = d
        for what, b in e.planted["blocks"]:
            if what == "match":
                d = at_lo[b + 1]
                assert d[3] == hp.MATCH and "N" in d[6] and len(d[4]) == 2 and len(d[5]) == 2, (what, b, gap)
                assert d[6].index("N", gap) == gap + 2           # the byte behind the deleted C, in both replays
            elif what == "mismatch":
                d = at_lo[b + 1]
                assert d[3] == hp.MISMATCH and len(d[6]) == len(d[7]), (what, b, gap)
                diff = [(x, y) for x, y in zip(d[6], d[7]) if x != y]
                assert sorted(diff) == [("N", "T"), ("T", "N")]  # nothing but a base against the byte that is none
            elif what == "lower":
                assert at_lo[b][3] == hp.MATCH
        n = len(NOBASE)
        assert int(rec[R["refmismatch"]]) == n and int(tru[T["unusable"]]) == n
        assert int(tru[T["tried"]]) == 3 * n and int(tru[T["matched"]]) == 2 * n


# ---- (g) overlapping windows ---------------------------------------------------------------------------------------------------------
def overlap_family():
    """The configuration of the Sites paragraph: X, an SNV at 99; D, spelled at 100 with twelve shared bases in front, so its
    footprint is 112; E, an SNV at 101, behind D in table order.  D opens a site (112 > 99 + 2 g for g <= 5), E joins it, and the
    window of D's site starts at 101 - g: at or before 99 + g, the end of X's window, for g >= 1."""
    rng = np.random.default_rng(67)
    g = rand_genome(rng, 240)
    x, e1 = snv(g, 99), snv(g, 101)
    d = (100, at(g, 100, 13), at(g, 100, 12) + snv(g, 112)[2])
    truth = [x, d, e1]
    a = [line(*snv(g, 98)), line(*snv(g, 100)), line(*e1), line(*snv(g, 112))]                 # E is found: D alone is open, spelled as the SNV it is
    b = [line(*snv(g, 96)), line(*snv(g, 99, 2)), line(*snv(g, 100, 2)), line(100, at(g, 100, 2), at(g, 100) + e1[2]),
         line(100, at(g, 100, 6), "".join(snv(g, 100 + k, 3)[2] for k in range(6))), line(*snv(g, 102)), line(*snv(g, 105)), line(*snv(g, 112, 2)), line(*snv(g, 114))]
    return Edge("overlap", g, [truth], [("a", 0, a, True), ("b", 0, b, True)], (2, 1, 5), {"d": d}, shuffle=("a", "b"))


def present_overlap(e, res):
    G = hp.symbols(e.genome)
    ent = [(p, hp.spell(r), hp.spell(a)) for p, r, a in e.order[0]]
    assert [v[0] for v in ent] == [99, 100, 101] and strip(ent[1][1], ent[1][2]) == (12, 0)
    for gap in e.gaps:
        site_of, table = hp.sites(G, ent, gap)
        assert site_of == [0, 1, 1] and table == [(0, 99 - gap, 99 + gap), (1, 101 - gap, 112 + gap)]
        assert table[1][1] <= table[0][2]                       # two sites, overlapping windows
        for v in (0, 1):
            rec, tru, cls, site, ecls, detail = res[(v, gap)]
            pos = e.cols[v][0].tolist()
            assert {0, 1} <= set(site.tolist()), (v, gap)       # records on both sides of the overlap
            inside = [s for p, r, s in zip(pos, e.cols[v][1].tolist(), site.tolist()) if r < 4 and table[1][1] <= p <= table[0][2]]
            assert inside and set(inside) == {0}                # a footprint inside both windows belongs to the first site
        assert res[(0, gap)][3].tolist()[3] == 1 and res[(0, gap)][2].tolist()[3] == hp.MATCH    # D spelled as the SNV it is
        assert res[(1, gap)][3].tolist()[4] == 1                # the MNP 100 .. 105 ends behind the first window


@functools.lru_cache(maxsize=None)
def family(name):
    return {"trim": trim_family, "seams": seam_family, "rank": rank_family, "dense": dense_family, "ends0": lambda: ends_family(200),
            "ends1": lambda: ends_family(201), "ends7": lambda: ends_family(207), "nobase": nobase_family, "overlap": overlap_family}[name]()


PRESENT = {"trim": present_trim, "seams": present_seams, "rank": present_rank, "dense": present_dense, "ends0": present_ends,
           "ends1": present_ends, "ends7": present_ends, "nobase": present_nobase, "overlap": present_overlap}
NAMES = tuple(PRESENT)
