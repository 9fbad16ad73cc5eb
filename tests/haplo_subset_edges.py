"""Edge families of the subset-search tests, beside the planted family of haplo_subsets.py: inputs built so that
the machinery of k_hap_subsets leaves its first iteration -- the power table and the scan behind the prefix hashes, subset hashes
composed across every seam of those tables, a verification that has to look behind its first stride, the order of forms inside
one q, one, two and four rounds of the mask loops, every level of the order key decided alone, items against forms, windows of
253 .. 257 bases and windows clipped at either end.  Plain Python over strings, with the tools of haplo_edges.py.  Every family
comes with a `present` check: what it plants is asserted on the restatement's output, so that a generator that drifts fails instead
of passing vacuously.  The checks are shared by the host test and the device test.  Not collected as a test.

The independent judge of the search lives here too (`whole`, `plain_forms`, `all_pairs_ok`, `brute`; `candidates` lists every
candidate, not the optimum alone): a double loop over all pairs of subsets that substitutes into the WHOLE genome by plain slicing.

Windows: at gap g the window of a site is [first entry - g, last entry + g].  Truth SNVs that the VCF calls by spelling (`found`)
are not open; they stretch a window without entering any replay, also where they lie inside a tandem run: the run stays intact in
both replays.  `stretch(ws, W)` plants them so that the window is exactly [ws, ws + W - 1] at gap 10."""
import functools

import numpy as np

import haplo_subsets as hs
from haplo_edges import Edge, at, dense_site, line, prefixed, rand_genome, snv, strip
from haplo_family import BASES
from quasimodo_amd import haplo as hp

GAP = 10


# ---- the independent judge -----------------------------------------------------------------------------------------------------
def whole(G, fs):
    """the genome with the forms substituted, right to left, by plain slicing"""
    for q, r, a in sorted(fs, key=lambda f: (f[0], len(f[1])), reverse=True):
        assert G[q - 1:q - 1 + len(r)] == r
        G = G[:q - 1] + a + G[q - 1 + len(r):]
    return G


def plain_forms(side):
    out = set()
    for p, ref, alt in side:
        cp, cs = strip(ref, alt)
        out.add((p + cp, ref[cp:len(ref) - cs], alt[cp:len(alt) - cs]))
    return sorted(out, key=lambda f: (f[0], len(f[1]), len(f[2]), f[2]))


def all_pairs_ok(fs):
    return not any(b[0] < a[0] + len(a[1]) or (b[0] == a[0] and not b[1]) for i, a in enumerate(fs) for b in fs[i + 1:])


@functools.lru_cache(maxsize=None)
def brute(G, recs, ents):
    """the optimum by a double loop over all pairs of subsets, or None"""
    sides = []
    for side in (recs, ents):
        fs = plain_forms(side)
        subs = []
        for m in range(1, 1 << len(fs)):
            pick = [f for k, f in enumerate(fs) if m >> k & 1]
            if all_pairs_ok(pick):
                subs.append((m, bin(m).count("1"), whole(G, pick)))
        sides.append(subs)
    best = None
    for ms, ns, x in sides[0]:
        for mt, nt, y in sides[1]:
            if x == y and (best is None or (-(ns + nt), -nt, ms, mt) < best):
                best = (-(ns + nt), -nt, ms, mt)
    return None if best is None else best[2:]


@functools.lru_cache(maxsize=None)
def candidates(G, recs, ents):
    """every candidate of a site as (|S| + |T|, |T|, S mask, T mask), the optimum first: the same double loop, nothing dropped"""
    sides = []
    for side in (recs, ents):
        fs = plain_forms(side)
        subs = []
        for m in range(1, 1 << len(fs)):
            pick = [f for k, f in enumerate(fs) if m >> k & 1]
            if all_pairs_ok(pick):
                subs.append((m, bin(m).count("1"), whole(G, pick)))
        sides.append(subs)
    out = [(-(ns + nt), -nt, ms, mt) for ms, ns, x in sides[0] for mt, nt, y in sides[1] if x == y]
    return [(-k[0], -k[1], k[2], k[3]) for k in sorted(out)]


def narrow_hash(s):
    """the narrow hash of a replay: the polynomial mod 2^32 in base 0x9E3779B1 over the symbols code + 1 (A, C,
    G, T = 0 .. 3), of which the top 4 bits are kept"""
    h = 0
    for c in s:
        h = (h * 0x9E3779B1 + BASES.index(c) + 1) & 0xffffffff
    return h >> 28


# ---- tools -----------------------------------------------------------------------------------------------------------------------
def other(c, k=1):
    return BASES[(BASES.index(c) + k) % 4]


class Build:
    def __init__(self, seed, n):
        self.rng = np.random.default_rng(seed)
        self.g = rand_genome(self.rng, n)
        self.truth, self.recs, self.planted = [], [], []

    def put(self, p, s):
        self.g[p - 1:p - 1 + len(s)] = list(s)

    def pick(self, n):
        return "".join(BASES[i] for i in self.rng.integers(0, 4, n))

    def found(self, p):
        """a truth SNV that the VCF calls by spelling"""
        v = snv(self.g, p)
        self.truth.append(v)
        self.recs.append(line(*v))

    def stretch(self, ws, W, last=True):
        """found SNVs 20 bases apart from ws + 10 on (and at ws + W - 11): the window is [ws, ws + W - 1] at gap 10"""
        ps = list(range(ws + GAP, ws + W - GAP - 1, 2 * GAP)) + ([ws + W - GAP - 1] if last else [])
        for p in ps:
            self.found(p)
        return ps

    def pair(self, p, k=1):
        """an entry SNV and the line that respells it with one more base in front"""
        v = snv(self.g, p, k)
        self.truth.append(v)
        self.recs.append(line(*prefixed(self.g, v)))
        return v

    def edge(self, name, gaps=(GAP,), vcfs=None, truths=None, planted=None, shuffle=("main",)):
        vcfs = vcfs or [("main", 0, sorted(self.recs, key=lambda r: r[0]), True)]
        return Edge(name, self.g, truths or [self.truth], vcfs, gaps, self.planted if planted is None else planted, shuffle=shuffle)


def spelled(e, v, idx):
    c = e.cols[v]
    return sorted((int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in idx)


def site_with(res, p):
    """the tried site of a restatement whose window holds p"""
    hit = [d for d in res[5] if d[1] <= p <= d[2]]
    assert len(hit) == 1, "%d tried sites hold %d" % (len(hit), p)
    return hit[0]


def outcome_at(restated, v, gap, p):
    """(the tried site that holds p, its row of the search's detail or None)"""
    res, (sub, cls_s, ecls_s, chosen) = restated[(v, gap)]
    d = site_with(res, p)
    hit = [c for c in chosen if c[0] == d[0]]
    return d, (hit[0] if hit else None)


def bits(m):
    return bin(m).count("1")


# ---- (1) hash: S != T as forms, equal as strings, over every seam of the prefix tables ---------------------------------------------
def tandem_site(B, ws, kind, u, o1, n, W=None, swapped=False, change=False, n_at=None, fp=True, end=False, lower=False):
    """A tandem run of n bases with a unit of u at window offsets o1 .. o1 + n - 1 of the window that starts at ws.  One variant
    inserts (deletes) one unit at the run's LEFT end, spelled with the anchor base in front; one does the same at its RIGHT end.
    The left one is the open line and the right one the open entry, or the reverse (swapped: an entry's form lies at least a gap
    inside its window, a line's form anywhere in it).  A run that is no multiple of its unit makes the right insertion a rotation of
    the left one.  change: one base of the run between the two forms is another, so the two replays differ.  n_at: an N at this
    window offset.  fp: one unrelated FP SNV line in the window.  end: the run ends on the genome's last base.  Returns the plant."""
    g = B.g
    rs = ws + o1
    re = rs + n - 1
    while True:
        unit = B.pick(u)
        if u == 1 or all(unit != unit[:d] * (u // d) for d in range(1, u) if u % d == 0):
            break
    pat = unit * (n // u + 3)
    B.put(rs, pat[:n])
    if at(g, rs - 1) == pat[u - 1]:                            # the run is no longer than planted on either side
        g[rs - 2] = other(pat[u - 1])
    if not end and at(g, re + 1) == pat[n]:
        g[re] = other(pat[n])
    if change:
        c = rs + n // 2 if kind == "ins" else rs + u + (n - 2 * u) // 2
        assert rs <= c <= re and (kind == "ins" or rs + u <= c <= re - u)
        g[c - 1] = other(at(g, c), 2)
    if n_at is not None:
        g[ws + n_at - 1] = "N"
    if kind == "ins":
        left = (rs - 1, at(g, rs - 1), at(g, rs - 1) + unit)
        right = (re, at(g, re), at(g, re) + pat[n:n + u])
        q2 = re + 1
    else:
        assert n > u
        left = (rs - 1, at(g, rs - 1, u + 1), at(g, rs - 1))
        right = (re - u, at(g, re - u, u + 1), at(g, re - u))
        q2 = re - u + 1
    o2 = q2 - ws
    if W is None:
        W = max(o2 + (u if kind == "del" else 0) + 16, 36)
    ln, en = (right, left) if swapped else (left, right)
    stretched = B.stretch(ws, W)
    B.truth.append(en)
    B.recs.append(line(*ln))
    fpl = None
    if fp:
        free = [p for p in (q2 + u + 3, rs - 4, rs - 6, q2 + u + 5) if ws <= p <= ws + W - 1 - end and p not in stretched
                and not rs - 2 <= p <= re + 2 and at(g, p) in BASES]
        fpl = snv(g, free[0], 2)
        B.recs.append(line(*fpl))
    if lower:
        g[ws - 1:ws + W - 1] = [c.lower() for c in g[ws - 1:ws + W - 1]]
    plant = {"ws": ws, "W": W, "o1": o1, "o2": o2, "n": n, "u": u, "kind": kind, "swapped": swapped, "twin": change, "n_at": n_at,
             "line": ln, "entry": en, "fp": fpl, "at": ws + GAP, "end": end}
    B.planted.append(plant)
    return plant


def hash_plan():
    plan = []
    for i in range(4):                                          # every pair of residues mod 4
        for j in range(4):
            if (i + j) % 2:
                n = (j - i) % 4 + 1
                plan.append(("del", 1, 12 + i, n if n >= 3 else n + 4))
            else:
                n = {0: 4, 1: 5, 2: 6, 3: 3}[(j - i) % 4]
                plan.append(("ins", {4: 2, 5: 1, 6: 3, 3: 3}[n], 12 + i, n))
    plan += [("ins", 1, 0, 12), ("ins", 1, 13, 4), ("del", 2, 30, 6),                          # o1 < 4 d <= o2 for d = 1, 2; 4; 8
             ("ins", 1, 60, 3), ("ins", 2, 60, 4), ("ins", 1, 60, 5),                          # o2 = 63, 64, 65 (d = 16)
             ("del", 1, 124, 4), ("ins", 1, 124, 4), ("ins", 1, 124, 5),                       # o2 = 127, 128, 129 (d = 32)
             ("ins", 1, 14, 1),                                                                 # a run of one base: a plain respelling
             ("ins", 3, 12, 63), ("ins", 2, 13, 64), ("ins", 1, 14, 65),
             ("ins", 1, 0, 204), ("del", 2, 20, 200), ("ins", 3, 21, 201),
             ("ins", 12, 15, 29), ("ins", 12, 16, 41), ("del", 12, 14, 36)]                    # 12-base units: ALTs (REFs) of 13 bases
    return plan


def hash_family():
    """See the issue's family `hash`.  The three sites with o2 = 251, 252, 253 have the sides exchanged (the line at the right
    end): at gap 10 an entry's form lies at offsets 10 .. W - 11 unless the window is clipped.  o2 = W - 1 is an entry that deletes
    the genome's last base, in a window clipped at L + 1; that site has no twin (the genome has one end).  The longest insertion an
    inline code spells with its anchor has 12 bases: those are the `13-base` sites, rotated where the run is no multiple of 12."""
    B = Build(81, 30000)
    ws = 40
    for kind, u, o1, n in hash_plan():
        for change in (False, True):
            p = tandem_site(B, ws, kind, u, o1, n, change=change)
            ws += p["W"] + 60
    for u, n in ((2, 8), (3, 9), (1, 10)):                      # o2 = 251, 252, 253
        for change in (False, True):
            tandem_site(B, ws, "ins", u, 243, n, W=256, swapped=True, change=change)
            ws += 256 + 60
    W = 30                                                      # the genome's end: L = ws + W - 1
    tandem_site(B, ws, "del", 1, W - 6, 6, W=W + 1, end=True)
    del B.g[ws + W - 1:]
    return B.edge("hash")


def check_tandem(e, restated, plants, v=0, gap=GAP):
    """every plant of the tandem kind is where it was planted and comes out as it must: PARTIAL with the open line and the open
    entry and nothing else, NOSUBSET for a twin.  Returns the plants that are PARTIAL."""
    L = len(e.genome)
    good = []
    for pl in plants:
        d, hit = outcome_at(restated, v, gap, pl["at"])
        assert (d[1], d[2]) == (pl["ws"], min(pl["ws"] + pl["W"] - 1, L + 1)), (pl, d[:3])
        assert d[3] == hp.MISMATCH, pl
        forms = (hp.trim(*pl["line"]), hp.trim(*pl["entry"]))
        lo, hi = sorted(f[0] - pl["ws"] for f in forms)
        assert (lo, hi) == (pl["o1"], pl["o2"]) and forms[0] != forms[1], pl
        if pl["twin"] or (pl["n_at"] is not None and pl["o1"] <= pl["n_at"] < pl["o1"] + pl["n"]):
            assert hit is None, ("a subset in a twin", pl, hit)
            continue
        assert hit is not None, ("no subset", pl)
        assert bits(hit[1]) == 1 and bits(hit[2]) == 1, pl
        assert spelled(e, v, hit[3]) == [pl["line"]] and (pl["fp"] is None or spelled(e, v, hit[4]) == [pl["fp"]]), pl
        assert [e.order[e.vcfs[v][1]][j][0] for j in hit[5]] == [pl["entry"][0]] and hit[6] == [], pl
        good.append(pl)
    return good


def present_hash(e, restated):
    good = check_tandem(e, restated, e.planted)
    twins = [pl for pl in e.planted if pl["twin"]]
    assert len(good) == len(twins) + 1 and good[-1]["end"]
    assert {(pl["o1"] % 4, pl["o2"] % 4) for pl in good} == {(i, j) for i in range(4) for j in range(4)}
    for d in (1, 2, 4, 8, 16, 32):
        assert any(pl["o1"] < 4 * d <= pl["o2"] for pl in good), d
    assert any(pl["o1"] == 0 for pl in good)
    o2 = {pl["o2"] for pl in good if not pl["end"]}
    assert {63, 64, 65, 127, 128, 129, 251, 252, 253} <= o2
    end = good[-1]
    assert end["o2"] == len(e.genome) - end["ws"] and hp.trim(*end["entry"])[0] == len(e.genome)    # W - 1 of the W bases the window holds
    runs = {pl["n"] for pl in good}
    assert {1, 3, 4, 5, 63, 64, 65} <= runs and max(runs) >= 200
    assert {pl["u"] for pl in good} >= {1, 2, 3, 12}
    long13 = [pl for pl in good if pl["u"] == 12]
    assert sum(pl["kind"] == "ins" and pl["line"][2][1:] != pl["entry"][2][1:] and len(pl["entry"][2]) == 13 for pl in long13) == 2
    assert sum(pl["kind"] == "del" and len(pl["entry"][1]) == 13 for pl in long13) == 1
    for a, b in zip(e.planted[0:-1:2], e.planted[1:-1:2]):      # a twin: the same plan one slot on, one base of the run apart
        assert not a["twin"] and b["twin"] and all(a[k] == b[k] for k in ("W", "o1", "o2", "n", "u", "kind", "swapped"))


# ---- (2) verify: colliding candidates that only the symbol loop can refute -------------------------------------------------------
STRIDES = ((10, 64), (64, 128), (128, 192), (192, 246))


def big_site(B, ws, wrong):
    """W = 256 and eight 12-base insertions on each side: entry k inserts I behind the base X at p (I ends in X), line k inserts
    X + I[:-1] behind the base in front of it -- another form, the same string.  wrong = 'base': the last line's insertion ends in
    another base (searched until the narrow hashes of the two full replays collide; their first difference lies behind offset 256);
    wrong = 'form': the last pair is an FP SNV line and an entry nobody called."""
    g = B.g
    B.stretch(ws, 256)
    ps = [ws + 20 + 20 * k for k in range(7)] + [ws + 229]
    win = lambda: "".join(g[ws - 1:ws + 255])
    ents, lns = [], []
    for p in ps[:7] if wrong == "form" else ps:
        ins = B.pick(11) + at(g, p)
        ents.append((p, at(g, p), at(g, p) + ins))
        lns.append((p - 1, at(g, p - 1), at(g, p - 1) + at(g, p) + ins[:-1]))
    plant = {"ws": ws, "at": ws + GAP, "wrong": wrong}
    if wrong == "form":
        ents.append(snv(g, ws + 200))
        lns.append(snv(g, ws + 180, 2))
        plant["tot"] = 256 + 7 * 12
    else:
        p, found = ps[7], None
        for _ in range(400):
            ins = B.pick(11) + at(g, p)
            ents[7] = (p, at(g, p), at(g, p) + ins)
            y = whole(win(), [(hp.trim(*v)[0] - ws + 1,) + hp.trim(*v)[1:] for v in ents])
            for j, k in ((j, k) for j in range(11) for k in (1, 2, 3)):
                bad = at(g, p) + ins[:j] + other(ins[j], k) + ins[j + 1:-1]
                lns[7] = (p - 1, at(g, p - 1), at(g, p - 1) + bad)
                x = whole(win(), [(hp.trim(*v)[0] - ws + 1,) + hp.trim(*v)[1:] for v in lns])
                if narrow_hash(x) == narrow_hash(y):
                    found = (x, y)
                    break
            if found:
                break
        assert found
        plant["replays"] = found
        plant["tot"] = len(found[0])
    B.truth += ents
    B.recs += [line(*v) for v in lns]
    plant["lines"], plant["entries"] = lns, ents
    return plant


def verify_family():
    B = Build(83, 3200)
    ws = 40
    strides = []
    for lo, hi in STRIDES:                                      # 1 x 1: a line SNV X > Y against an entry SNV X > Z at one position
        got = None
        for o, t in ((o, t) for o in range(lo, hi) for t in range(1, 2 * GAP)):    # t: a found SNV behind it sets the window's end
            win = "".join(B.g[ws - 1:ws + o + t + GAP])
            for ky, kz in ((1, 2), (1, 3), (2, 3)):
                x, y = (win[:o] + other(win[o], k) + win[o + 1:] for k in (ky, kz))
                if narrow_hash(x) == narrow_hash(y) and o % 20 != 10 and o + t <= 245:
                    got = (o, t, ky, kz, x, y)
                    break
            if got:
                break
        o, t, ky, kz, x, y = got
        B.stretch(ws, o + GAP + 1, last=False)
        B.truth.append(snv(B.g, ws + o, kz))
        B.recs.append(line(*snv(B.g, ws + o, ky)))
        B.found(ws + o + t)
        strides.append({"ws": ws, "o": o, "W": o + t + GAP + 1, "at": ws + o, "replays": (x, y)})
        ws += o + t + GAP + 60
    big = [big_site(B, ws, "base"), big_site(B, ws + 320, "form")]
    return B.edge("verify", planted={"strides": strides, "big": big})


def present_verify(e, restated):
    collisions = 0
    for k, pl in enumerate(e.planted["strides"]):
        d, hit = outcome_at(restated, 0, GAP, pl["at"])
        x, y = pl["replays"]
        assert (d[1], d[2], d[3]) == (pl["ws"], pl["ws"] + pl["W"] - 1, hp.MISMATCH) and (d[6], d[7]) == (x, y), pl
        assert hit is None and len(d[4]) == 1 and len(d[5]) == 1, pl
        first = [i for i in range(len(x)) if x[i] != y[i]]
        assert first == [pl["o"]] and STRIDES[k][0] <= pl["o"] < STRIDES[k][1] and pl["o"] // 64 == k, pl
        collisions += narrow_hash(x) == narrow_hash(y) and len(x) == len(y)
    base, form = e.planted["big"]
    d, hit = outcome_at(restated, 0, GAP, base["at"])
    x, y = base["replays"]
    assert d[2] - d[1] + 1 == 256 and d[3] == hp.MISMATCH and (d[6], d[7]) == (x, y) and len(d[4]) == len(d[5]) == 8
    assert len(x) == len(y) == 256 + 96 and min(i for i in range(len(x)) if x[i] != y[i]) >= 256
    collisions += narrow_hash(x) == narrow_hash(y)
    assert hit is not None and (hit[1], hit[2]) == (0x7f, 0x7f)           # the full pair is refuted; without the last pair: 7 + 7
    d, hit = outcome_at(restated, 0, GAP, form["at"])
    assert d[2] - d[1] + 1 == 256 and d[3] == hp.MISMATCH and len(d[4]) == len(d[5]) == 8
    assert hit is not None and bits(hit[1]) == bits(hit[2]) == 7 and len(hit[7]) == form["tot"] >= 340
    assert collisions == 5, collisions


# ---- (3) order: the rank of a form -------------------------------------------------------------------------------------------------
def ordered_alts(B, n, ks, ends="ACGT"):
    """eight ALTs of n bases: for every k of ks a pair that first differs at base k, A against C, and that differs at its last
    base the other way, T against C (k = n - 1: at that base alone); what is left is drawn.  ends: the bases a first and a last
    base may be."""
    while True:
        out = []
        for k in ks:
            head = B.pick(k)
            if k == n - 1:
                out += [head + "A", head + "C"]
            else:
                out += [head + "A" + B.pick(n - k - 2) + "T", head + "C" + B.pick(n - k - 2) + "C"]
        while len(out) < min(8, 4 ** n):
            out.append(B.pick(n))
        if len(set(out)) == len(out) and all(a[0] in ends and a[-1] in ends for a in out):
            return out


def packed(a):
    return sum(BASES.index(c) << (2 * i) for i, c in enumerate(a))


MIXED = ((0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1))


def order_family():
    B = Build(85, 2600)
    g = B.g
    b = 60
    sites = []
    plan = [(13, (0, 1, 2, 3)), (13, (4, 5, 6, 7)), (1, ()), (13, (8, 9, 10, 11)), (13, (12, 0, 6, 11)), (8, (0, 1, 2, 3)),
            (8, (4, 5, 6, 7)), (2, (0, 1))]
    for k, (n, ks) in enumerate(plan):
        rank = k % (4 if n == 1 else 8)
        if n == 13:                                             # eight entries (b, G, 13 bases); the lines spell one as an SNV and an insertion
            B.put(b, "G")
            alts = ordered_alts(B, n, ks, "ACT")
            B.truth += [(b, "G", a) for a in alts]
            a = sorted(alts)[rank]
            B.recs += [line(b, "G", a[0]), line(b, "G", "G" + a[1:])]
            side = "T"
        else:                                                   # eight lines that insert at b; the entry respells one
            alts = ordered_alts(B, n, ks)
            x = at(g, b - 1)
            B.recs += [line(b - 1, x, x + a) for a in alts]
            a = sorted(alts)[rank]
            B.truth.append(prefixed(g, (b - 1, x, x + a)))
            side = "S"
        sites.append({"at": b, "n": n, "alts": alts, "rank": rank, "side": side})
        b += 80
    mixed = []
    for rank in range(7):                                       # seven entry forms at one q, ordered by |r| first; the line respells one
        B.put(b - 1, "TCAG")
        w, x, v = at(g, b - 1), at(g, b), at(g, b + 1)
        y = [c for c in BASES if c not in (x, v)]
        ents = [(b - 1, w, w + x), (b - 1, w, w + x + y[0]), (b - 1, w + x, w), (b, x, y[0]), (b, x, y[1] + y[0]),
                (b - 1, w + x + v, w), (b, x + v, y[1])]
        B.truth += ents
        B.recs.append(line(*prefixed(g, ents[rank])))
        mixed.append({"at": b, "entries": ents, "rank": rank})
        b += 80
    return B.edge("order", planted={"sites": sites, "mixed": mixed})


def present_order(e, restated):
    ranks, seen = set(), {}
    for pl in e.planted["sites"]:
        d, hit = outcome_at(restated, 0, GAP, pl["at"])
        alts, n = pl["alts"], pl["n"]
        assert d[3] == hp.CONFLICT and hit is not None, pl
        mask = hit[2] if pl["side"] == "T" else hit[1]
        assert mask == 1 << pl["rank"] and (hit[1] if pl["side"] == "T" else hit[2]) == (3 if pl["side"] == "T" else 1), (pl, hit[:3])
        assert len(hit[6 if pl["side"] == "T" else 4]) == len(alts) - 1
        ranks.add((n, pl["rank"]))
        for a in alts:
            for c in alts:
                if a < c:
                    k = min(i for i in range(n) if a[i] != c[i])
                    seen.setdefault(n, {}).setdefault(k, set()).add(packed(a) < packed(c))
    for n in (13, 8, 2):                                        # at every base a pair that the packed number orders the other way
        assert all(False in seen[n][k] for k in range(n - 1)) and n - 1 in seen[n], (n, seen[n])
    assert sorted(r for n, r in ranks) == list(range(8)) and {n for n, r in ranks} == {13, 8, 2, 1}
    got = set()
    for pl in e.planted["mixed"]:
        d, hit = outcome_at(restated, 0, GAP, pl["at"])
        fs = hp.forms(pl["entries"])
        assert [(len(f[1]), len(f[2])) for f in fs] == list(MIXED) and len({f[0] for f in fs}) == 1, pl
        assert d[3] == hp.CONFLICT and hit is not None and (hit[1], hit[2]) == (1, 1 << pl["rank"]), (pl, hit[:3])
        got.add(hit[2])
    assert len(got) == 7


# ---- (4) rounds: every (n_S, n_T) in 1 .. 8 x 1 .. 8 -------------------------------------------------------------------------------
def rounds_family():
    """Site (n_S, n_T): SNV forms two bases apart between two found SNVs; min(n_S, n_T) respelled pairs (one less on the diagonal),
    the surplus as FP SNV lines and as entries nobody called.  Where the surplus goes -- in front, behind, or in front of the last
    pair -- changes with the site, so that the optimum's masks reach all four quarters of 1 .. 255 on either side."""
    B = Build(87, 6600)
    g = B.g
    b = 50
    for ns in range(1, 9):
        for nt in range(1, 9):
            m = min(ns, nt) - (ns == nt)
            seq = ["P"] * m
            for side, n, var in (("S", ns, (ns + nt) % 3), ("T", nt, (ns + 2 * nt) % 3)):
                if var == 2 and m:
                    where = max(i for i, s in enumerate(seq) if s == "P")
                elif var == 1:
                    where = len(seq)
                else:
                    where = 0
                seq[where:where] = [side] * (n - m)
            B.found(b)
            for i, s in enumerate(seq):
                p = b + 2 * (i + 1)
                if s == "P":
                    B.pair(p)
                elif s == "S":
                    B.recs.append(line(*snv(g, p, 2)))
                else:
                    B.truth.append(snv(g, p))
            B.found(b + 2 * (len(seq) + 1))
            B.planted.append({"at": b, "ns": ns, "nt": nt, "m": m})
            b += 100
    return B.edge("rounds", gaps=(GAP, 0))


def present_rounds(e, restated):
    quarters = {"S": set(), "T": set()}
    seen = set()
    for pl in e.planted:
        d, hit = outcome_at(restated, 0, GAP, pl["at"])
        assert (len(d[4]), len(d[5])) == (pl["ns"], pl["nt"]) and d[3] == hp.MISMATCH, (pl, d[:6])
        seen.add((len(d[4]), len(d[5])))
        if pl["m"] == 0:
            assert hit is None and (pl["ns"], pl["nt"]) == (1, 1)
            continue
        assert hit is not None and bits(hit[1]) == bits(hit[2]) == pl["m"], (pl, hit[:3])
        quarters["S"].add(hit[1] >> 6)
        quarters["T"].add(hit[2] >> 6)
    assert seen == {(i, j) for i in range(1, 9) for j in range(1, 9)}
    assert quarters == {"S": {0, 1, 2, 3}, "T": {0, 1, 2, 3}}, quarters
    res, (sub, _, _, _) = restated[(0, 0)]                      # gap 0: the sites fall apart, every count is another
    assert int(sub[0]) != int(restated[(0, GAP)][1][0][0]) and int(res[1][hp.T_COLS.index("sites")]) > 300


# ---- (5) ties: the four levels of the key, each decided alone ------------------------------------------------------------------------
def ties_family():
    B = Build(89, 900)
    g = B.g
    sites = []
    b = 60                                                      # level 0, the larger |S| + |T|: five forms a side, one wrong on each
    for i in range(4):
        B.pair(b + 3 * i)
    B.truth.append(snv(g, b + 12))
    B.recs.append(line(*snv(g, b + 12, 2)))
    sites.append({"at": b, "level": 0, "want": (0xf, 0xf)})
    b = 200                                                     # level 1, the larger |T|: see the issue
    B.put(b - 1, "C" + "A" * 12 + "G")
    x, y = b, b + 8
    B.recs += [line(x - 1, "CAAA", "C"), line(x - 1, "CA", "C"), line(x, "AA", "A")]
    B.truth += [(y - 1, "AAA", "A"), (y + 1, "AA", "A")]
    sites.append({"at": y, "level": 1, "want": (2, 3)})         # (x, AAA, ) is the second of three line forms
    b = 340                                                     # level 2, the smallest S mask, both >= 64: six FP SNV lines in front of two
    for i in range(6):                                          # lines that insert one A at two points of a run; the entry at a third
        B.recs.append(line(*snv(g, b + 2 * i, 2)))
    B.found(b + 4)
    B.put(b + 13, "C" + "A" * 6 + "G")
    B.recs += [line(b + 14, "A", "AA"), line(b + 15, "A", "AA")]
    B.truth.append((b + 13, "C", "CA"))
    sites.append({"at": b + 13, "level": 2, "want": (0x40, 1)})
    b = 480                                                     # level 3, the smallest T mask at one S: two entries nobody called in
    B.truth += [snv(g, b), snv(g, b + 3)]                       # front of two that insert one A at two points of a run
    B.put(b + 8, "C" + "A" * 6 + "G")
    B.truth += [(b + 9, "A", "AA"), (b + 10, "A", "AA")]
    B.recs.append(line(b + 8, "C", "CA"))
    sites.append({"at": b + 8, "level": 3, "want": (1, 4)})
    return B.edge("ties", planted=sites)


def site_sides(e, v, d):
    """the spellings of a tried site's open lines and open entries, as `brute` takes them"""
    c, ent = e.cols[v], e.order[e.vcfs[v][1]]
    return (tuple((int(c[0][i]), hp.spell(c[1][i]), hp.spell(c[2][i])) for i in d[4]),
            tuple((ent[j][0], hp.spell(ent[j][1]), hp.spell(ent[j][2])) for j in d[5]))


def present_ties(e, restated):
    G = hp.symbols(e.genome)
    for pl in e.planted:
        d, hit = outcome_at(restated, 0, GAP, pl["at"])
        assert hit is not None and (hit[1], hit[2]) == pl["want"], (pl, hit)
        cands = candidates(G, *site_sides(e, 0, d))
        best, lv = cands[0], pl["level"]
        assert best[2:] == pl["want"]
        rivals = [c for c in cands[1:] if c[:lv] == best[:lv] and c[lv] != best[lv]]
        assert rivals, pl                                       # the runner-up under this level of the key: tied above it, another here
        if lv == 1:
            assert sorted(c[:2] for c in cands) == [(2, 1), (2, 1), (3, 1), (3, 2)] and d[3] == hp.CONFLICT
        if lv == 2:
            assert rivals[0][2] == 0x80 and best[2] >= 64


# ---- (6) items: counts of items against counts of forms --------------------------------------------------------------------------------
def items_family():
    B = Build(91, 2400)
    g = B.g
    t0, t1, a, c_, b_ = [], [], [], [], []                      # truth sets 0 and 1; VCFs a and c on 0, b on 1
    planted = {}
    p = 60                                                      # eight open lines that trim to three forms, two of them in S
    B.put(p, "ACGT")
    t0.append((p, "ACG", "A"))
    f1 = [line(p, "ACGT", "AT"), line(*prefixed(g, (p, "ACG", "A")), extra=0), line(*prefixed(g, (p, "ACGT", "AT")))]
    s = snv(g, p + 8)
    t0.append((p + 6, at(g, p + 6, 2) + s[1], at(g, p + 6, 2) + s[2]))
    f2 = [line(*s), line(*prefixed(g, s), extra=0), line(p + 8, s[1] + at(g, p + 9), s[2] + at(g, p + 9))]
    w = snv(g, p + 12, 2)
    f3 = [line(*w), line(*prefixed(g, w))]
    a += f1 + f2 + f3
    planted["eight"] = {"at": p, "rescued": 6, "iddot": 4}
    p = 160                                                     # two open entries of one form
    B.put(p, "ACGT")
    t0 += [(p, "ACG", "A"), (p, "ACGT", "AT")]
    a += [line(*prefixed(g, (p, "ACG", "A"))), line(*snv(g, p + 6, 2))]
    planted["twice"] = {"at": p}
    p = 260                                                     # a PARTIAL site of truth set 0 that VCF c calls another way
    t0 += [snv(g, p), snv(g, p + 3)]
    a += [line(*prefixed(g, snv(g, p))), line(*snv(g, p + 3, 2))]
    c_ += [line(*snv(g, p, 2)), line(*prefixed(g, snv(g, p + 3)), extra=0)]
    planted["shared"] = {"at": p}
    p = 400                                                     # truth set 1: a site of 130 entries, three SNVs per position
    site = dense_site(g, p, 130)
    t1 += site
    order = sorted(site, key=lambda v: (v[0], hp.code(v[2])))
    six = (0, 63, 64, 127, 128, 129)
    b_ += [line(*v) for o, v in enumerate(order) if o not in six]
    b_ += [line(*prefixed(g, order[o])) for o in (0, 64, 128)]
    nine = six + (20, 40, 100)
    d_ = [line(*v) for o, v in enumerate(order) if o not in nine] + [line(*prefixed(g, order[0]))]
    planted["dense"] = {"at": p, "six": six}
    p = 600                                                     # a PARTIAL site of truth set 1
    t1 += [snv(g, p), snv(g, p + 3)]
    b_ += [line(*prefixed(g, snv(g, p))), line(*snv(g, p + 3, 2))]
    d_ += [line(*prefixed(g, snv(g, p))), line(*snv(g, p + 3, 2))]
    planted["second"] = {"at": p}
    vcfs = [("a", 0, a, True), ("b", 1, b_, True), ("nogenome", 0, list(a), False), ("c", 0, c_, True), ("nine", 1, d_, True)]
    return Edge("items", g, [t0, t1], vcfs, (GAP,), planted, shuffle=("a", "b"))


def present_items(e, restated):
    pl = e.planted
    va, vb, vc, vn = (e.index(t) for t in ("a", "b", "c", "nine"))
    assert [v[1] for v in e.vcfs[:5]] == [0, 1, 0, 0, 1] and not e.vcfs[2][3] and len(e.order[1]) >= 100
    res, (sub, cls_s, ecls_s, chosen) = restated[(va, GAP)]
    d, hit = outcome_at(restated, va, GAP, pl["eight"]["at"])
    assert len(d[4]) == 8 and len(hp.forms(site_sides(e, va, d)[0])) == 3 and hit is not None and bits(hit[1]) == 2
    assert len(hit[3]) == 6 and len(hit[4]) == 2 and len(hit[5]) == 2
    flags = e.cols[va][4]
    assert sum(bool(flags[i] & hp.F_IDDOT) for i in hit[3]) == 4                              # rescued lines with and without IDDOT
    d, hit = outcome_at(restated, va, GAP, pl["twice"]["at"])
    assert d[3] == hp.CONFLICT and len(d[5]) == 2 and hit is not None and (hit[1], hit[2]) == (1, 1) and len(hit[5]) == 2
    iddot = sum(bool(flags[i] & hp.F_IDDOT) for c in chosen for i in c[3])
    assert int(sub[3]) - int(res[0][2]) == iddot < int(sub[4])                               # TP_S - TP_H: the rescued lines with IDDOT
    for v, name in ((va, "shared"), (vc, "shared"), (vb, "second"), (vn, "second")):
        d, hit = outcome_at(restated, v, GAP, pl[name]["at"])
        assert hit is not None and bits(hit[1]) == bits(hit[2]) == 1, (v, name)
    assert outcome_at(restated, va, GAP, pl["shared"]["at"])[1][2] != outcome_at(restated, vc, GAP, pl["shared"]["at"])[1][2]
    d, hit = outcome_at(restated, vb, GAP, pl["dense"]["at"])
    first = min(d[5])
    assert d[3] == hp.CONFLICT and [j - first for j in d[5]] == list(pl["dense"]["six"]), d[5]
    assert hit is not None and [j - first for j in hit[5]] == [0, 64, 128] and [j - first for j in hit[6]] == [63, 127, 129]
    d, hit = outcome_at(restated, vn, GAP, pl["dense"]["at"])
    assert d[3] == hp.TOOMANY and len(d[5]) == 9 and hit is None


# ---- (7) edges: windows ------------------------------------------------------------------------------------------------------------------
def edges_family():
    B = Build(93, 4200)
    g = B.g
    ws = 40
    for W in (253, 254, 255, 256, 257):                         # W = 257: TOOLONG, not searched
        tandem_site(B, ws, "ins", 1, W - 32, 5, W=W)
        ws += W + 60
    wide = B.planted[:]
    B.planted = []
    for n_at, o1 in ((3, 1), (4, 1), (63, 58), (64, 58), (3, 6), (4, 6), (63, 66), (64, 52)):    # an N inside the run (four) and outside it
        tandem_site(B, ws, "ins", 1, o1, 9, n_at=n_at, W=100)
        ws += 160
    tandem_site(B, ws, "del", 2, 14, 8, lower=True)             # a lower-case stretch
    tandem_site(B, ws + 120, "ins", 3, 15, 9, change=True, lower=True)
    first = snv(g, 1)                                           # a window clipped at 1: a line form at q = 1, spelled (1, XY, ZY)
    B.truth += [first, snv(g, 6)]
    B.recs += [line(1, first[1] + at(g, 2), first[2] + at(g, 2)), line(*snv(g, 6, 2))]
    return B.edge("edges", planted={"wide": wide, "tandem": B.planted, "first": first})


def present_edges(e, restated):
    res, (sub, cls_s, ecls_s, chosen) = restated[(0, GAP)]
    wide = e.planted["wide"]
    assert [pl["W"] for pl in wide] == [253, 254, 255, 256, 257]
    assert len(check_tandem(e, restated, wide[:4])) == 4
    ws = wide[4]["ws"]
    assert not [d for d in res[5] if d[1] <= ws + GAP <= d[2]]                                  # 257: never tried
    i_long = [i for i, p in enumerate(e.cols[0][0].tolist()) if ws <= p < ws + 257]
    assert len(i_long) >= 10 and set(res[2][i_long].tolist()) == {hp.MATCHED, hp.TOOLONG} and (cls_s[i_long] == res[2][i_long]).all()
    good = check_tandem(e, restated, e.planted["tandem"])
    assert sorted((pl["n_at"], pl["o1"] <= pl["n_at"] < pl["o1"] + pl["n"]) for pl in e.planted["tandem"] if pl["n_at"] is not None) \
        == [(3, False), (3, True), (4, False), (4, True), (63, False), (63, True), (64, False), (64, True)]
    assert len(good) == 5 and sum(pl["n_at"] is None for pl in good) == 1
    assert any(c.islower() for c in e.genome) and "N" in e.genome
    d, hit = outcome_at(restated, 0, GAP, 1)
    assert d[1] == 1 and hit is not None and (hit[1], hit[2]) == (1, 1) and spelled(e, 0, hit[3])[0][0] == 1
    assert hp.trim(*spelled(e, 0, hit[3])[0]) == e.planted["first"]


def right_family(L):
    """A window of 256 positions clipped at L + 1 (it holds the genome's last 255 bases): the entry inserts at L + 1, at the right
    end of a run -- its form offset is the number of bases the window holds --, the line at the run's left end."""
    B = Build(95 + L, L)
    ws = L - 254
    tandem_site(B, ws, "ins", 1, 248, 7, W=257, end=True)
    assert ws + 248 + 7 - 1 == L
    B.pair(ws + 31)
    return B.edge("right%d" % L)


def present_right(e, restated):
    L = len(e.genome)
    (pl,) = e.planted
    assert L % 8 in (4, 7, 0) and pl["o2"] == 255 == L - pl["ws"] + 1 and hp.trim(*pl["entry"])[0] == L + 1
    d, hit = outcome_at(restated, 0, GAP, pl["at"])
    assert (d[1], d[2], d[3]) == (L - 254, L + 1, hp.MISMATCH) and hit is not None and bits(hit[1]) == bits(hit[2]) == 2
    assert pl["line"] in spelled(e, 0, hit[3]) and spelled(e, 0, hit[4]) == [pl["fp"]] and hit[6] == []
    assert len(hit[7]) == 256


@functools.lru_cache(maxsize=None)
def family(name):
    return {"hash": hash_family, "verify": verify_family, "order": order_family, "rounds": rounds_family, "ties": ties_family,
            "items": items_family, "edges": edges_family, "right260": lambda: right_family(260), "right263": lambda: right_family(263),
            "right264": lambda: right_family(264)}[name]()


PRESENT = {"hash": present_hash, "verify": present_verify, "order": present_order, "rounds": present_rounds, "ties": present_ties,
           "items": present_items, "edges": present_edges, "right260": present_right, "right263": present_right,
           "right264": present_right}
NAMES = tuple(PRESENT)


def restate_all(e, masks=None):
    """{(v, gap): hs.restate} of every VCF with a genome at every gap of the family (masks: {v: (kept, tp)} of a batch, or None)"""
    return {(v, gap): hs.restate(e, v, gap, None if masks is None else masks[v]) for v, vc in enumerate(e.vcfs) if vc[3] for gap in e.gaps}


def judge(e, restated):
    """`brute` on every searched site of a restatement: the same masks, or None for NOSUBSET.  Returns (searched, partial)."""
    G = hp.symbols(e.genome)
    searched = partial = 0
    for (v, gap), (res, (sub, cls_s, ecls_s, chosen)) in restated.items():
        masks = {d[0]: (d[1], d[2]) for d in chosen}
        n = 0
        for d in res[5]:
            if d[3] not in (hp.MISMATCH, hp.CONFLICT):
                assert d[0] not in masks
                continue
            n += 1
            got = brute(G, *site_sides(e, v, d))
            assert got == masks.get(d[0]), "%s, VCF %d, gap %d, site %d: %r against %r" % (e.name, v, gap, d[0], got, masks.get(d[0]))
            partial += got is not None
        assert n == int(sub[0]) == int(sub[1]) + int(sub[2])
        searched += n
    return searched, partial
