"""The planted family of the subset-search tests: one genome of 1900 bases, one truth set, and VCFs whose open
lines and open entries make MISMATCH and CONFLICT sites with and without a partial match.  Blocks of SLOT bases, so that at the
default gap every block is a site of its own; the bases a block needs are written into the random genome.  Plain Python over
strings, with the tools of haplo_family.py and haplo_edges.py.  Every block carries a `present` entry -- the outcome of the
haplotype pass and the optimum, derived by hand -- that `present` asserts on the restatement's output, so that a generator that
drifts fails instead of passing vacuously.  Not collected as a test.

block  plants                                                                              comes out (S and T in forms)
(a)    ACG>T against A>T + ACG>A, one unrelated SNV line 5 bases on                        PARTIAL 1 + 2, the SNV is left
(b)    the reverse: an extra truth SNV nobody called                                       PARTIAL 1 + 2, that entry is left
(c)    two overlapping lines, one of which alone spells the truth                          CONFLICT becomes PARTIAL 1 + 1
(d)    two lines that insert one A at two points of one run, one truth entry               a tie: S mask 1 wins
(e)    two spellings of one form on the line side                                          both lines are rescued
(f)    a 2 x 2 site without a subset                                                       NOSUBSET
(g)    a 1 x 1 MISMATCH site                                                               NOSUBSET
(h1)   8 forms on both sides, one wrong on each                                            7 + 7
(h2)   8 entries; 7 respelled lines and an MNP over the last two, in conflict with one     CONFLICT becomes 7 + 8
(i1)   8 lines each inserting one A into a run of 12 A, 8 entries doing the same with      8 + 7: every admissible T with the
       other spellings, one of them inserting two                                          double replays alike, the smallest wins
(i2)   the same 8 lines against 8 entries that insert one C each                           NOSUBSET after 255 x 255 pairs
(j)    insertions of one base at one point, T against G, beside a respelled SNV            equal deltas, other symbols: 1 + 1
(kL)   a partial site in a window clipped at position 1                                    1 + 1
(kR)   ... and one clipped at L + 1, with an insertion behind the last base                1 + 1, the insertion is left
(kN)   a window that holds an N                                                            1 + 1
(l)    a site of 65 entries, 62 found by spelling, 3 open (a second gather round)          CONFLICT becomes 1 + 1
(m)    VCF `other`: block (a) with other lines; VCF `nogenome`: the lines of `main`        another optimum; zero rows

The VCFs end on span tails of 1 (main and its shuffled twin), 2 (other) and 3 (nogenome) records."""
import numpy as np

from haplo_edges import Edge, at, line, prefixed, rand_genome, snv
from quasimodo_amd import haplo as hp

SLOT = 100
GAPS = (10, 0, 32)
PARTIAL, NOSUBSET = "partial", "nosubset"


def pad(recs, tail, filler):
    """recs plus lines that are not kept, until len % 4 == tail"""
    out = list(recs)
    while len(out) % 4 != tail:
        out.append(filler)
    return out


def family():
    rng = np.random.default_rng(77)
    g = rand_genome(rng, 19 * SLOT)
    L = len(g)
    truth, main, other, planted = [], [], [], {}

    def put(p, s):
        g[p - 1:p - 1 + len(s)] = list(s)

    def plant(name, b, was, outcome, s=0, t=0, rescued=None, vcf="main"):
        planted[name] = {"at": b, "was": was, "outcome": outcome, "s": s, "t": t, "rescued": rescued, "vcf": vcf}

    b = 120                                                     # (a)
    put(b, "ACG")
    truth += [(b, "A", "T"), (b, "ACG", "A")]
    main += [line(b, "ACG", "T"), line(*snv(g, b + 5))]
    plant("a", b, hp.MISMATCH, PARTIAL, 1, 3, rescued=[(b, "ACG", "T")])
    other += [line(*prefixed(g, (b, "A", "T"))), line(*snv(g, b + 5, 2))]          # (m): A>T alone, the deletion is left
    plant("m", b, hp.MISMATCH, PARTIAL, 1, 1, vcf="other")
    b = 220                                                     # (b)
    put(b, "ACG")
    truth += [(b, "A", "T"), (b, "ACG", "A"), snv(g, b + 5)]
    main += [line(b, "ACG", "T")]
    plant("b", b, hp.MISMATCH, PARTIAL, 1, 3)
    b = 320                                                     # (c)
    put(b, "ACG")
    truth += [(b, "ACG", "A")]
    main += [line(*prefixed(g, (b, "ACG", "A"))), line(b + 2, "G", "T")]
    plant("c", b, hp.CONFLICT, PARTIAL, 1, 1, rescued=[prefixed(g, (b, "ACG", "A"))])
    b = 420                                                     # (d)
    put(b, "CAAAAG")
    truth += [(b, "C", "CA")]
    main += [line(b + 1, "A", "AA"), line(b + 2, "A", "AA")]
    plant("d", b, hp.MISMATCH, PARTIAL, 1, 1, rescued=[(b + 1, "A", "AA")])
    b = 520                                                     # (e)
    put(b, "ACGT")
    truth += [(b, "ACG", "A")]
    main += [line(*prefixed(g, (b, "ACG", "A"))), line(b, "ACGT", "AT")]
    plant("e", b, hp.CONFLICT, PARTIAL, 1, 1, rescued=[prefixed(g, (b, "ACG", "A")), (b, "ACGT", "AT")])
    b = 620                                                     # (f)
    truth += [snv(g, b, 1), (b + 6, at(g, b + 6, 3), at(g, b + 6))]
    main += [line(*snv(g, b, 2)), line(*snv(g, b + 3, 1))]
    plant("f", b, hp.MISMATCH, NOSUBSET)
    b = 720                                                     # (g)
    truth += [snv(g, b, 1)]
    main += [line(*snv(g, b, 2))]
    plant("g", b, hp.MISMATCH, NOSUBSET)
    b = 820                                                     # (h1)
    truth += [snv(g, b + 3 * i) for i in range(7)] + [snv(g, b + 21, 1)]
    main += [line(*prefixed(g, snv(g, b + 3 * i))) for i in range(7)] + [line(*snv(g, b + 21, 2))]
    plant("h1", b, hp.MISMATCH, PARTIAL, 0x7f, 0x7f)
    b = 920                                                     # (h2)
    spots = [b + 3 * i for i in range(6)] + [b + 18, b + 19]
    truth += [snv(g, p) for p in spots]
    main += [line(*prefixed(g, snv(g, p))) for p in spots[:7]]
    main += [line(b + 18, at(g, b + 18, 2), snv(g, b + 18)[2] + snv(g, b + 19)[2])]
    plant("h2", b, hp.CONFLICT, PARTIAL, 0xbf, 0xff)
    for name, b in (("i1", 1020), ("i2", 1120)):                # (i)
        put(b, "C" + "A" * 12 + "G")
        main += [line(b + k, "A", "AA") for k in range(1, 9)]                       # forms (b + 2 .. b + 9, "", "A")
    b = 1020
    truth += [(b, "C", "CA"), (b + 1, "AA", "AAA"), (b + 2, "AA", "AAA"), (b + 4, "A", "AAA")]      # q = b + 1, b + 3, b + 4, b + 5 (the double)
    truth += [(b + k, "A", "AA") for k in range(9, 13)]                                             # q = b + 10 .. b + 13
    plant("i1", b, hp.MISMATCH, PARTIAL, 0xff, 0x7f)
    b = 1120
    truth += [(b + k, "A", "AC") for k in range(1, 9)]
    plant("i2", b, hp.MISMATCH, NOSUBSET)
    b = 1220                                                    # (j)
    put(b, "CA")
    truth += [(b, "C", "CG"), snv(g, b + 5, 1)]
    main += [line(b, "C", "CT"), line(*prefixed(g, snv(g, b + 5, 1)))]
    plant("j", b, hp.MISMATCH, PARTIAL, 2, 2)
    b = 1320                                                    # (kN)
    put(b + 3, "N")
    truth += [snv(g, b), snv(g, b + 6, 1)]
    main += [line(*prefixed(g, snv(g, b))), line(*snv(g, b + 6, 2))]
    plant("kN", b, hp.MISMATCH, PARTIAL, 1, 1)
    truth += [snv(g, 3, 1), snv(g, 6, 1)]                       # (kL)
    main += [line(*prefixed(g, snv(g, 3, 1))), line(*snv(g, 6, 2))]
    plant("kL", 3, hp.MISMATCH, PARTIAL, 1, 1)
    truth += [snv(g, L - 2, 1), (L, at(g, L), at(g, L) + "A")]  # (kR)
    main += [line(*prefixed(g, snv(g, L - 2, 1)))]
    plant("kR", L - 2, hp.MISMATCH, PARTIAL, 1, 1)
    b = 1420                                                    # (l)
    chain = [snv(g, b + 10 * i, k) for i in range(21) for k in (1, 2, 3)] + [snv(g, b + 210, 1), snv(g, b + 210, 2)]
    assert len(chain) == 65
    truth += chain
    chain.sort(key=lambda v: (v[0], hp.code(v[2])))             # the table's order inside one position and REF: by the ALT's code
    opened = chain[62:]
    main += [line(*v) for v in chain[:62]] + [line(*prefixed(g, opened[2]))]
    t_forms = hp.forms(opened)
    plant("l", b + 210, hp.CONFLICT, PARTIAL, 1, 1 << t_forms.index(hp.trim(*opened[2])))
    filler = line(*snv(g, 1780), kept=False)
    vcfs = [("main", 0, pad(main, 1, filler), True), ("other", 0, pad(other, 2, filler), True),
            ("nogenome", 0, pad(main, 3, filler), False)]
    e = Edge("subsets", g, [truth], vcfs, GAPS, planted, shuffle=("main",))
    assert [len(c[0]) % 4 for c in e.cols] == [1, 2, 3, 1]
    return e


def restate(e, v, gap, masks=None):
    """(what e.restate gives, its detail) and (sub, cls_s, ecls_s, the detail of the PARTIAL sites) of VCF v at `gap`"""
    res = e.restate(v, gap, masks)
    c, w = e.cols[v], e.vcfs[v][1]
    kept, tp = res_masks(e, v, masks)
    detail = []
    sub, cls_s, ecls_s = hp.subset_counts(e.genome, e.tcodes[w], c[0], c[1], c[2], c[4], kept, tp, gap, detail, counted=(res[:5], res[5]))
    return res, (sub, cls_s, ecls_s, detail)


def res_masks(e, v, masks):
    from haplo_family import host_masks
    return host_masks(e.cols[v], e.tcodes[e.vcfs[v][1]]) if masks is None else masks


def present(e, restated):
    """restated: {(v, gap): what `restate` returns}.  At the default gap every block is where it was planted and comes out as
    derived by hand; the family reaches PARTIAL, NOSUBSET, a site that was CONFLICT and an optimum decided by a tie-break."""
    seen = set()
    for name, want in e.planted.items():
        v = e.index(want["vcf"])
        res, (sub, cls_s, ecls_s, chosen) = restated[(v, 10)]
        tried = [d for d in res[5] if d[1] <= want["at"] <= d[2]]
        assert len(tried) == 1, "block %s: %d tried sites hold %d" % (name, len(tried), want["at"])
        s, ws, we, what, recs, ents, _, _ = tried[0]
        assert what == want["was"], "block %s: the pass calls it %s" % (name, hp.CLASS_NAMES[what])
        hit = [d for d in chosen if d[0] == s]
        if want["outcome"] == NOSUBSET:
            assert not hit, "block %s: a subset %r" % (name, hit)
            assert all(cls_s[i] == what for i in recs) and all(ecls_s[j] == what for j in ents), name
            seen.add(NOSUBSET)
            continue
        assert len(hit) == 1, "block %s: no subset" % name
        _, ms, mt, inr, outr, ine, oute, x = hit[0]
        assert (ms, mt) == (want["s"], want["t"]), "block %s: masks %#x, %#x" % (name, ms, mt)
        assert all(cls_s[i] == hp.SUBSET for i in inr) and all(cls_s[i] == hp.LEFT for i in outr), name
        assert all(ecls_s[j] == hp.SUBSET for j in ine) and all(ecls_s[j] == hp.LEFT for j in oute), name
        if want["rescued"] is not None:
            c = e.cols[v]
            got = sorted((int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in inr)
            assert got == sorted(want["rescued"]), "block %s: rescued %r" % (name, got)
        seen.add(PARTIAL)
        if what == hp.CONFLICT:
            seen.add("was conflict")
        if name in ("d", "i1"):
            seen.add("tie-break")
    assert seen == {PARTIAL, NOSUBSET, "was conflict", "tie-break"}, seen
    if (e.index("main"), 32) in restated:                         # gap 32: the window of (l) is too long, the site is not searched
        res, (sub, cls_s, _, _) = restated[(e.index("main"), 32)]
        assert (res[2] == hp.TOOLONG).any() and not ((cls_s >= hp.SUBSET) & (res[2] == hp.TOOLONG)).any()
