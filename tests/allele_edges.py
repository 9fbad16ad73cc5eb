"""Edge families of the three allele passes -- normal form (qmvt_norm.hip), atomisation (qmvt_atom.hip, 4.18), type
and size (qmvt_types.hip, 4.19) --, in the layout of haplo_edges.py: inputs built so that the mechanisms of the kernels leave the
cases a random draw reaches -- every pair of inline allele lengths with every extreme of the common prefix and suffix, one long
allele against every inline length, both hash tables half full, wrapped and contended, the span walk on its seams, both ends of the
genome, bytes that are no base.  Plain Python over strings (and numpy columns for the large VCFs).  Every family is one finished
allele-extended batch for all three passes and comes with a `present` check: what it plants is asserted on the restatements'
output, so that a generator that drifts fails instead of passing vacuously.  `nm_hash`, `at_hash` and the slot rule are restated
here for choosing plants only: nothing that is compared with the device goes through them.  No assert here reads a device."""
import functools

import numpy as np

import haplo_edges as he
from haplo_edges import BASES, at as bases_at, rand_genome, strip
from quasimodo_amd import atomize as at
from quasimodo_amd import normalize as nz
from quasimodo_amd import vartype as vt
from test_normalize_host import planted_norm_genome

NR = {name: k for k, name in enumerate(nz.R_COLS)}
NT = {name: k for k, name in enumerate(nz.T_COLS)}
AR = {name: k for k, name in enumerate(at.R_COLS)}
AT = {name: k for k, name in enumerate(at.T_COLS)}
EDGES16 = (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 14, 16, 21, 51, 52, 100)
HAS_FORM = (nz.UNCHANGED, nz.RESPELLED, nz.RESCUED)
PLAIN = nz.F_IDDOT


def line(p, r, a, kept=True, extra=PLAIN):
    return (p, r, a, kept, extra)


def snv(g, p, k=1):
    """the k-th of the three SNVs at p (g: a string or a list; lower case reads as upper case)"""
    ref = bases_at(g, p)
    return (p, ref, BASES[(BASES.index(ref) + k) % 4])


class Coder:
    """allele strings as codes: inline up to 13 bases, ids of the family's own dictionary beyond; an int is a code already"""

    def __init__(self):
        self.ids = {}

    def __call__(self, s):
        if isinstance(s, (int, np.integer)):
            return int(s)
        return nz.code(s) if len(s) <= nz.INLINE_MAX else nz.DICT | self.ids.setdefault(s, len(self.ids))

    def shapes(self):
        return vt.shapes_of(sorted(self.ids, key=self.ids.get)) if self.ids else None


class Family:
    """name; genomes: [str]; truths: [(index of its genome, [(p, REF, ALT)])] -- REF and ALT strings or codes --; vcfs: [(tag, index
    of its truth set, records, has a genome)], records [(p, REF, ALT, kept, flags beyond PASS)] or the five finished columns;
    edges: the size edges the type pass runs with; planted: what `present` looks for; reasons: {tag: how many of its records have
    no normal form}, None where every record of the family has one.  shuffle: the tags that get a twin with the same records in a
    shuffled order (twin: {its index: (the index of the sorted one, the permutation)})."""

    def __init__(self, name, genomes, truths, vcfs, edges=(None,), planted=None, reasons=None, shuffle=(), coder=None):
        self.name, self.genomes, self.edges, self.planted, self.reasons = name, ["".join(g) for g in genomes], tuple(edges), planted or {}, reasons
        self.coder = coder or Coder()
        self.tgen = [t[0] for t in truths]
        self.tcodes = [self.truth_columns(t[1]) for t in truths]
        self.order = [nz.truth_order(*t) for t in self.tcodes]
        self.vcfs, self.cols, self.twin = [], [], {}
        for tag, w, recs, has in vcfs:
            self.vcfs.append((tag, w, recs, has))
            self.cols.append(recs if isinstance(recs[0], np.ndarray) else self.columns(recs))
        rng = np.random.default_rng(len(name) + 11)
        for tag in shuffle:
            v = self.index(tag)
            perm = rng.permutation(len(self.cols[v][0]))
            self.twin[len(self.vcfs)] = (v, perm)
            self.vcfs.append((tag + "_shuffled", self.vcfs[v][1], None, self.vcfs[v][3]))
            self.cols.append([x[perm].copy() for x in self.cols[v]])
        self.shapes = self.coder.shapes()
        if self.reasons is not None:
            for t, (v, _) in self.twin.items():
                self.reasons[self.vcfs[t][0]] = self.reasons[self.vcfs[v][0]]

    def index(self, tag):
        return [v[0] for v in self.vcfs].index(tag)

    def truth_columns(self, truth):
        n = len(truth)
        return tuple(np.array(x, np.int32).reshape(n) for x in ([t[0] for t in truth], [self.coder(t[1]) for t in truth], [self.coder(t[2]) for t in truth]))

    def columns(self, recs):
        n = len(recs)
        pos = np.array([r[0] for r in recs], np.int32).reshape(n)
        ref = np.array([self.coder(r[1]) for r in recs], np.int32).reshape(n)
        alt = np.array([self.coder(r[2]) for r in recs], np.int32).reshape(n)
        kept = np.array([bool(r[3]) for r in recs], bool).reshape(n)
        flags = (kept.astype(np.uint8) | np.array([r[4] for r in recs], np.uint8).reshape(n)).astype(np.uint8)
        return [pos, ref, alt, np.where(kept, 50, 5).astype(np.float32), flags]

    def genome_of(self, v):
        return self.genomes[self.tgen[self.vcfs[v][1]]]

    def host_masks(self, v):
        """kept and TP masks as the batch makes them for these records (no header rules take part): kept = PASS; a TP line is kept
        and (spelled like a valid truth entry, with a key and ID '.', or TPLINE)"""
        pos, ref, alt, _, flags = self.cols[v]
        ent = set(self.order[self.vcfs[v][1]])
        kept = (flags & nz.F_PASS).astype(bool)
        hit = np.array([e in ent for e in zip(pos.tolist(), ref.tolist(), alt.tolist())], bool).reshape(len(pos))
        return kept, kept & ((hit & ((flags & nz.F_NOKEY) == 0) & ((flags & nz.F_IDDOT) != 0)) | ((flags & nz.F_TPLINE) != 0))

    def restate(self, v, masks=None):
        """(nz.counts or None without a genome, at.counts, {edges: vt.counts}) of VCF v (masks: the batch's kept and TP masks;
        None: host_masks)"""
        c, (_, w, _, has) = self.cols[v], self.vcfs[v]
        kept, tp = self.host_masks(v) if masks is None else masks
        t = self.tcodes[w]
        return (nz.counts(self.genome_of(v), t, c[0], c[1], c[2], c[4], kept, tp) if has else None,
                at.counts(t, c[0], c[1], c[2], c[4], kept, tp),
                {e: vt.counts(t, c[0], c[1], c[2], c[4], kept, tp, e, self.shapes) for e in self.edges})

    def strings(self, v):
        """[(p, REF, ALT)] of VCF v with the alleles spelled out (None: a code that is no allele the family can spell)"""
        back = {nz.DICT | i: s for s, i in self.coder.ids.items()}
        sp = lambda c: nz.spell(c) if nz.is_inline(c) else back.get(int(c))
        pos, ref, alt = self.cols[v][:3]
        return [(p, sp(r), sp(a)) for p, r, a in zip(pos.tolist(), ref.tolist(), alt.tolist())]


def free_suffix(ref, alt):
    """the common suffix of the two alleles counted without regard to the prefix: what clz sees before the clamp"""
    n = 0
    while n < min(len(ref), len(alt)) and ref[-1 - n] == alt[-1 - n]:
        n += 1
    return n


def hamming(x, y):
    return sum(a != b for a, b in zip(x, y))


# ---- (1) every pair of inline lengths -----------------------------------------------------------------------------------------------
def pairs_family():
    """The entries and records of haplo_edges' trim family without its long ones: every (|REF|, |ALT|) in 1 .. 13 x 1 .. 13 at the
    extreme and one interior (cp, cs), every REF the genome's, p >= 2, one record per entry that respells it, every seventh with
    one ALT base changed.  Behind them a 13-base MNP with 13 atoms: spelled alike, its last 12 bases, with one atom wrong, its last
    11 bases."""
    t = he.family("trim")
    forms = t.planted["forms"]
    g = t.genome
    truth = [(p, r, a) for p, r, a, _, _ in forms]
    recs = list(t.vcfs[0][2][:len(forms)])
    p = len(g) - 66
    ref = bases_at(g, p, 13)
    alt = "".join(BASES[(BASES.index(c) + 1) % 4] for c in ref)
    truth.append((p, ref, alt))
    wrong = alt[:6] + BASES[(BASES.index(ref[6]) + 2) % 4] + alt[7:]
    recs += [line(p, ref, alt), line(p + 1, ref[1:], alt[1:]), line(p, ref, wrong), line(p + 2, ref[2:], alt[2:])]
    return Family("pairs", [g], [(0, truth)], [("respelled", 0, recs, True)], planted={"forms": forms, "mnp13": len(forms)}, shuffle=("respelled",))


def present_pairs(f, res):
    forms = f.planted["forms"]
    g = f.genomes[0]
    assert set(g) <= set(BASES)
    seen = {}
    for p, ref, alt, cp, cs in forms:
        assert strip(ref, alt) == (cp, cs) and bases_at(g, p, len(ref)) == ref and p >= 2
        seen.setdefault((len(ref), len(alt)), set()).add((cp, cs))
    for lr in range(1, 14):
        for la in range(1, 14):
            m, got = min(lr, la), seen.get((lr, la), set())
            assert any(cp == 0 and cs == 0 for cp, cs in got), (lr, la)
            assert any(cp == (m if lr != la else m - 1) for cp, cs in got), (lr, la)
            assert any(cs == m - cp - (lr == la) for cp, cs in got), (lr, la)
            if lr == la and lr >= 3:
                assert {(0, m - 1), (m - 1, 0), (m // 2, m - m // 2 - 1)} <= got, (lr, la)
    recs = f.strings(0)
    assert all(p >= 2 and bases_at(g, p, len(r)) == r for p, r, a in recs)             # every REF is the genome's
    both = [(r, a) for _, r, a in recs] + [(r, a) for _, r, a, _, _ in forms]
    overlap = [(r, a) for r, a in both if free_suffix(r, a) > min(len(r), len(a)) - strip(r, a)[0]]
    assert len(overlap) >= 100 and {min(len(r), len(a)) for r, a in overlap} >= set(range(1, 13))   # the clamp decides at every m
    assert sum(len(r) == 13 or len(a) == 13 for r, a in both) >= 300
    for v in (0, 1):
        n, a, ty = res[v]
        rec, tru, cls = n[0], n[1], n[2]
        assert np.isin(cls, HAS_FORM).all() and not rec[NR["long"]:].any()                # no record is left out
        assert int(rec[NR["rescued"]]) >= 1000 and int(rec[NR["kept"]]) - int(rec[NR["tp_n"]]) >= 150
        assert int(rec[NR["respelled"]]) >= 1000 and int(rec[NR["single_base"]]) >= 20
        acls, na, hm = a[2], a[3], a[4]
        k = f.planted["mnp13"]
        at_k = (lambda x: x[np.argsort(f.twin[1][1])][k:k + 4]) if v == 1 else (lambda x: x[k:k + 4])
        assert at_k(na).tolist() == [13, 12, 13, 11] and at_k(hm).tolist() == [0x1fff, 0xfff, 0x1fff & ~(1 << 6), 0x7ff]
        assert at_k(acls).tolist() == [at.FULL, at.RESCUED, at.PARTIAL, at.RESCUED]
        assert set(na[acls <= at.RESCUED].tolist()) >= set(range(1, 14))                    # every atom count
        rows = ty[None][2]
        kinds = set((rows // len(vt.DEFAULT_EDGES)).tolist())
        assert kinds == {vt.SNV, vt.MNP, vt.INS, vt.DEL, vt.CPX} and rows.max() < 5 * len(vt.DEFAULT_EDGES)


# ---- (2) one long allele against one inline allele ----------------------------------------------------------------------------------
LONG_LENGTHS = (14, 15, 25, 26, 27, 60)


def long_short_targets(m):
    out = set()
    for cp in (0, m // 2, m - 1, m):
        for cs in (0, (m - cp) // 2, m - cp - 1, m - cp):
            if 0 <= cp <= m and 0 <= cs <= m - cp:
                out.add((cp, cs))
    return sorted(out)


def spell_long_short(rng, n, m, cp, cs):
    """(long, short) of n and m bases whose common prefix is exactly cp and whose common suffix, of what is left, exactly cs"""
    pick = lambda k: "".join(BASES[i] for i in rng.integers(0, 4, k))
    for _ in range(400):
        short = pick(m)
        long_ = short[:cp] + pick(n - cp - cs) + short[m - cs:]
        if len(long_) == n and strip(long_, short) == (cp, cs):
            return long_, short
    raise AssertionError((n, m, cp, cs))


def longshort_family():
    """Long lengths 14, 15, 25, 26, 27 and 60 (head and tail words overlapping by 12 bases, by one, touching, apart) against every
    inline length, both orientations, cp in {0, m / 2, m - 1, m} x cs in {0, half of what is left, m - cp - 1, m - cp}; every
    third as a truth entry as well.  Behind the grid: sizes 99 and 100; the last id of the shape table and the first past it; valid
    codes under DICT that are no inline codes (length fields 14 and 15); two long alleles; NOVAR on a long id."""
    rng = np.random.default_rng(71)
    code = Coder()
    vs, plan = [], []
    for n in LONG_LENGTHS:
        for m in range(1, 14):
            for cp, cs in long_short_targets(m):
                for flip in (False, True):
                    long_, short = spell_long_short(rng, n, m, cp, cs)
                    vs.append((short, long_) if flip else (long_, short))
                    plan.append((n, m, cp, cs, flip))
    for n in (100, 101):                                        # sizes 99 and 100 behind a one-base anchor
        long_, short = spell_long_short(rng, n, 1, 1, 0)
        vs += [(long_, short), (short, long_)]
    last = spell_long_short(rng, 30, 5, 2, 1)
    vs.append(last)
    for r, a in vs:
        code(r), code(a)
    past = nz.DICT | len(code.ids)
    offgrid = [("A", past), (past, "ACG"), ((14 << 26) | 5, "A"), ("CC", (15 << 26) | 77), (vs[0][0], vs[2][0]), (nz.DICT | 3, nz.DICT | 3)]
    want = [vt.NOSHAPE, vt.NOSHAPE, vt.NOSHAPE, vt.NOSHAPE, vt.LONGPAIR, vt.NOVAR]
    g = rand_genome(rng, 3 * (len(vs) + len(offgrid)) + 80)
    recs, truth = [], []
    for k, (r, a) in enumerate(vs + offgrid):
        p = 10 + 3 * k
        recs.append(line(p, r, a, kept=k % 11 != 5))
        if k % 3 == 0 or k >= len(vs):
            truth.append((p, r, a))
    planted = {"plan": plan, "n_grid": len(vs), "last": last, "offgrid": want}
    return Family("longshort", [g], [(0, truth)], [("grid", 0, recs, True)], edges=(None, (1,), EDGES16), planted=planted,
                  reasons={"grid": len(recs)}, shuffle=("grid",), coder=code)


def present_longshort(f, res):
    plan, n_grid = f.planted["plan"], f.planted["n_grid"]
    recs = f.strings(0)
    seen = {}
    for (n, m, cp, cs, flip), (_, r, a) in zip(plan, recs):
        long_, short = (a, r) if flip else (r, a)
        assert (len(long_), len(short)) == (n, m) and strip(r, a) == (cp, cs)
        seen.setdefault((n, m, flip), set()).add((cp, cs))
    for n in LONG_LENGTHS:
        for m in range(1, 14):
            for flip in (False, True):
                assert seen[(n, m, flip)] == set(long_short_targets(m)), (n, m, flip)
    assert any(free_suffix(r, a) > min(len(r), len(a)) - strip(r, a)[0] for _, r, a in recs[:n_grid])
    sizes = {vt.shape(r, a)[1] for _, r, a in recs[:n_grid]}
    for edges in (vt.DEFAULT_EDGES, EDGES16):
        assert all(e in sizes and e - 1 in sizes for e in edges[1:]), (edges, sorted(sizes))       # both sides of every edge
    ln = f.shapes[0]
    assert int(f.cols[0][1][n_grid - 1]) == nz.DICT | (len(ln) - 1) and int(f.cols[0][2][n_grid]) == nz.DICT | len(ln)   # the last id, the first past it
    assert set(ln.tolist()) == set(LONG_LENGTHS) | {30, 100, 101}
    for v in (0, 1):
        n, a, ty = res[v]
        back = np.argsort(f.twin[1][1]) if v == 1 else np.arange(len(recs))
        assert (n[2] == nz.LONG).all() and (a[2] == at.LONG).all() and not a[3].any()              # LONG to both other passes
        kept = int((f.cols[v][4] & 1).sum())
        assert int(n[0][NR["long"]]) == int(a[0][AR["long"]]) == kept and 0 < kept < len(recs)
        for edges, (rec, tru, rows) in ty.items():
            nb = len(vt.check_edges(edges))
            assert (rows[back][:n_grid] < 5 * nb).all()
            assert (rows[back][n_grid:] - 5 * nb).tolist() == f.planted["offgrid"]
            assert int(tru[5 * nb + vt.NOSHAPE, 0]) == 4 and int(tru[5 * nb + vt.LONGPAIR, 0]) == 1 and int(tru[5 * nb + vt.NOVAR, 0]) == 1
            assert int(tru[:, 1].sum()) >= 300                                                     # entries found by their spelling
            if nb == 16:
                assert np.count_nonzero(rec[:5 * nb, 0]) >= 40 and (rec[2 * nb:4 * nb, 0] > 0).all()   # every bin of INS and DEL


# ---- (3) the hash tables on their edges -----------------------------------------------------------------------------------------------
M32 = 0xffffffff
MIN_SLOTS = 64


def nm_hash(p, r, a):
    x = ((p * 0x9e3779b1) ^ (r * 0x85ebca77) ^ (a * 0xc2b2ae3d)) & M32
    x ^= x >> 15
    x = (x * 0x2c1b3c6d) & M32
    x ^= x >> 12
    x = (x * 0x297a2d39) & M32
    return x ^ (x >> 15)


def at_hash(x):
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def slots_of(n):
    """the power of two at or above 2 n, 64 at the least"""
    s = MIN_SLOTS
    while s < 2 * n:
        s <<= 1
    return s


def fill(keys, slots, home):
    """{slot: key} of a linear-probing table that holds the distinct keys: which slots are taken does not depend on the order"""
    table = {}
    for k in keys:
        h = home(k) & (slots - 1)
        while h in table and table[h] != k:
            h = (h + 1) & (slots - 1)
        table[h] = k
    return table


def probe(table, slots, home, key):
    """(the slot of the key or -1, the slots looked at): the probe of nm_probe / at_probe"""
    h, path = home(key) & (slots - 1), []
    for _ in range(slots):
        path.append(h)
        if h not in table:
            return -1, path
        if table[h] == key:
            return h, path
        h = (h + 1) & (slots - 1)
    return -1, path


FORM_HOME = lambda k: nm_hash(*k)
ATOM_HOME = at_hash


def tables_of(f, w):
    """((slots, {slot: form}), (slots, {slot: atom})) of truth set w: the two tables as the kernels size and fill them"""
    forms, _ = nz.truth_forms(f.genomes[f.tgen[w]], *f.tcodes[w])
    _, per, aset = at.truth_atoms(*f.tcodes[w])
    fs, as_ = slots_of(len(f.order[w])), slots_of(sum(len(x) for x in per if x is not None))
    return (fs, fill(sorted(forms), fs, FORM_HOME)), (as_, fill(sorted(aset), as_, ATOM_HOME))


def snv_keys(v):
    p, r, a = v
    return (p, BASES.index(r), BASES.index(a)), at.atom_key(p, r, a)


def wrap_truth(g, rng, slots, n, used):
    """n SNVs whose forms and atoms fill tables of `slots` slots, six forms and six atoms with their home in the last two slots;
    returns (the truth set, the absent SNVs whose form probe / atom probe starts in the last two slots)"""
    cand = [snv(g, p, k) for p in range(500, 5990) for k in (1, 2, 3) if p not in used]
    last = (slots - 2, slots - 1)
    fh = [v for v in cand if FORM_HOME(snv_keys(v)[0]) & (slots - 1) in last]
    ah = [v for v in cand if ATOM_HOME(snv_keys(v)[1]) & (slots - 1) in last and v not in fh]
    both = lambda vs, pick, home: [v for v in vs if home(snv_keys(v)[pick]) & (slots - 1) == slots - 2][:3] + [v for v in vs if home(snv_keys(v)[pick]) & (slots - 1) == slots - 1][:3]
    fin, ain = both(fh, 0, FORM_HOME), both(ah, 1, ATOM_HOME)   # three keys at home in either slot: the chain takes slots - 2 .. 3 at the least
    fh, ah = fin + [v for v in fh if v not in fin], ain + [v for v in ah if v not in ain]
    truth = fh[:6] + ah[:6]
    rest = [v for v in cand if v not in fh and v not in ah]
    truth += [rest[i] for i in rng.choice(len(rest), n - len(truth), replace=False)]
    used.update(v[0] for v in truth)
    return truth, fh[6:10], ah[6:10]


def delete_one_a_spellings(g):
    """every spelling of 2 .. 13 bases of `one A less` inside the 70-base run at 101 .. 170 of planted_norm_genome and the T on
    either side of it"""
    out = []
    for p in range(100, 171):
        for lr in range(2, 14):
            if p + lr - 1 > 171:
                continue
            ref = g[p - 1:p - 1 + lr]
            k = ref.index("A")
            alt = ref[:k] + ref[k + 1:]
            assert g[:p - 1] + alt + g[p - 1 + lr:] == g[:100] + g[101:]
            out.append((p, ref, alt))
    return out


SNV_AT = 3000


def tables_family():
    g = planted_norm_genome(n=6000)
    rng = np.random.default_rng(73)
    used = set()
    truths, vcfs, planted = [], [], {}

    def add(tag, truth, recs):
        truths.append((0, truth))
        vcfs.append((tag, len(truths) - 1, recs, True))
        vcfs.append((tag + "_nogenome", len(truths) - 1, recs[:40], False))      # one VCF per table names no genome

    def around(truth, absent=()):                               # every entry as it is spelled, with another ALT, nine bases on; the absent ones
        recs = [line(*v) for v in truth] + [line(*snv(g, v[0], 2 if v[2] != snv(g, v[0], 2)[2] else 3)) for v in truth]
        recs += [line(*snv(g, v[0] + 9)) for v in truth] + [line(*v) for v in absent]
        return recs

    for n in (1, 32, 33):                                       # 64 slots with one key, exactly half full, then 128 slots
        truth = [snv(g, 600 + 17 * n + 7 * k, 1 + k % 3) for k in range(n)]
        add("size%d" % n, truth, around(truth))
    for slots, n in ((64, 20), (1024, 300)):
        truth, fabs, aabs = wrap_truth(g, rng, slots, n, used)
        add("wrap%d" % slots, truth, around(truth, fabs + aabs))
        planted["wrap%d" % slots] = (len(truths) - 1, slots, truth[:6], truth[6:12], fabs, aabs)
    spell = delete_one_a_spellings(g)
    held = spell[5::190]
    x = snv(g, SNV_AT, 1)
    mnps = []
    for k in range(13):                                         # thirteen MNPs over the SNV at SNV_AT, each with a second atom of its own
        s, ref = SNV_AT - k, bases_at(g, SNV_AT - k, 13)
        alt = list(ref)
        alt[k] = x[2]
        j = 12 - k if k != 6 else 7                            # (at a position of its own: x - k + j differs from MNP to MNP)
        alt[j] = BASES[(BASES.index(ref[j]) + 2) % 4]
        mnps.append((s, ref, "".join(alt)))
    ac = [(261, "AC", "ACAC"), (272, "CA", "CACA")]              # one insertion of a unit into the (AC)n at 251, twice
    bad = (450, BASES[(BASES.index(g[449]) + 1) % 4], g[449])    # REFMISMATCH: the one entry without a normal form
    truth = [v for v in spell if v not in held] + mnps + ac + [bad]
    recs = [line(*v) for v in held] + [line(*v) for v in spell[::16] if v not in held] + [line(*x), line(SNV_AT - 1, bases_at(g, SNV_AT - 1, 2), g[SNV_AT - 2] + x[2])]
    recs += [line(*mnps[0]), line(*mnps[12], extra=0), line(266, "C", "CAC"), line(281, "ACAC", "ACACAC"), line(120, "AAA", "A"), line(*bad)]
    add("contended", truth, recs)
    add("contended_reversed", truth[::-1], recs)
    planted.update(spell=spell, held=held, n_recs=len(recs))
    return Family("tables", [g], truths, vcfs, planted=planted, reasons={v[0]: (1 if v[0].startswith("contended") and v[3] else 0) for v in vcfs},
                  shuffle=("wrap1024", "contended"))


def present_tables(f, res):
    g = f.genomes[0]
    for n, slots in ((1, 64), (32, 64), (33, 128)):             # sizing: both tables on 2 n == slots and one past it
        w = f.vcfs[f.index("size%d" % n)][1]
        (fs, ft), (as_, atab) = tables_of(f, w)
        assert (fs, len(ft), as_, len(atab)) == (slots, n, slots, n), (n, fs, len(ft), as_, len(atab))
    for slots in (64, 1024):                                    # wrap: the chain from the last two slots runs over slot 0
        w, s, fh, ah, fabs, aabs = f.planted["wrap%d" % slots]
        (fs, ft), (as_, atab) = tables_of(f, w)
        assert fs == as_ == s == slots and len(ft) == len(atab) == len(f.order[w]) <= slots // 2
        for table, home, present, absent, pick in ((ft, FORM_HOME, fh, fabs, 0), (atab, ATOM_HOME, ah, aabs, 1)):
            chain = [slots - 2]
            while (chain[-1] + 1) % slots in table:
                chain.append((chain[-1] + 1) % slots)
            assert all(c in table for c in (slots - 2, slots - 1, 0, 1, 2, 3)) and len(chain) < slots // 2, (slots, pick)
            assert {home(snv_keys(v)[pick]) & (slots - 1) for v in present} == {slots - 2, slots - 1}
            at_slot = sorted(probe(table, slots, home, snv_keys(v)[pick])[0] for v in present)
            assert len(at_slot) == 6 and all(x >= 0 for x in at_slot)                   # six keys for two home slots: four or more sit behind the wrap
            assert len(absent) == 4
            for v in absent:                                    # absent: from the last two slots through slot 0 to an empty one
                slot, path = probe(table, slots, home, snv_keys(v)[pick])
                assert slot == -1 and path[0] >= slots - 2 and 0 in path and path[-1] not in table and path[-1] < slots // 2, (slots, pick, v)
        keys = {snv_keys((p, r, a)) for p, r, a in f.strings(f.index("wrap%d" % slots))}
        assert sum(k[0] in set(ft.values()) for k in keys) == len(f.order[w]) and sum(k[1] in set(atab.values()) for k in keys) == len(f.order[w])
    spell, held = f.planted["spell"], f.planted["held"]
    assert len(spell) == 786 and len(held) == 5 and len(spell) - len(held) > 2 * 256      # more entries of one form than two workgroups hold
    assert all(nz.normalize(g, *v)[1:] == (100, "TA", "T") for v in spell)
    key = (100, nz.code("TA"), nz.code("T"))
    for tag in ("contended", "contended_reversed", "contended_shuffled"):
        v = f.index(tag)
        w = f.vcfs[v][1]
        n, a, ty = res[v]
        rec, tru, cls, npos, nref, nalt, row = n
        back = np.argsort(f.twin[v][1]) if v in f.twin else np.arange(len(cls))
        first = min(j for j, e in enumerate(f.order[w]) if (e[0], nz.spell(e[1]), nz.spell(e[2])) in set(spell))
        assert (row[back][:len(held)] == first).all() and (cls[back][:len(held)] == nz.RESCUED).all()
        assert list(zip(npos[back][:5].tolist(), nref[back][:5].tolist(), nalt[back][:5].tolist())) == [key] * 5
        n_forms = 1 + 13 + 1 + 1                                # the deletion, the MNPs, the insertion, the entry without a form
        assert tru.tolist() == [len(spell) - len(held) + 16, n_forms, 5, 1, 1], tru.tolist()   # found: the deletion, two MNPs, the insertion (by form only), the bad entry
        assert int(rec[NR["refmismatch"]]) == 1 and int(rec[NR["rescued"]]) == len(held) + 2
        arec, atru, acls, na, hm = a
        k = f.planted["n_recs"] - 8
        assert acls[back][k:k + 2].tolist() == [at.RESCUED, at.RESCUED] and na[back][k:k + 2].tolist() == [1, 1]   # the SNV every MNP carries
        assert int(atru[AT["atomisable"]]) == 14 and int(atru[AT["atoms"]]) == 1 + 13 + 1      # the shared atom once, 13 second atoms, the bad entry's
    a, b = res[f.index("contended")], res[f.index("contended_reversed")]
    for x, y in zip(a[0], b[0]):
        np.testing.assert_array_equal(x, y)                     # loaded forwards and reversed: the same rows, the same counts
    for v, vc in enumerate(f.vcfs):
        assert (res[v][0] is None) == (not vc[3])


# ---- (4) the span walk ------------------------------------------------------------------------------------------------------------------
WALK_SIZES = (16384, 16385, 1, 65536, 65537, 0, 1023, 1025, 2, 3)
INDEL, MNP2, NOKEY, LONG = range(4)
WALK_L = 20000


def seam_plan(n):
    """{index: kind} of a VCF of n records: the four kinds over the four indices around every multiple of 1024 (16 384 and 65 536
    among them; two on either side, which kind sits where moves with the seam), and over the first and the last four indices"""
    plan = {}

    def put(i, kind):
        if 0 <= i < n:
            plan.setdefault(i, kind % 4)
    for s in range(0, n + 1, 1024):
        for d in (-2, -1, 0, 1):
            put(s + d, s // 1024 + d + 2)
    for d in range(4):
        put(d, d + n)
        put(n - 1 - d, d + n + 1)
    return plan


def walk_family():
    rng = np.random.default_rng(79)
    g = "".join(rand_genome(rng, WALK_L))
    gc = np.array([BASES.index(c) for c in g], np.int32)
    code = Coder()
    long_id = code("ACGTTGCAACGTTG")
    base = []
    for w in (0, 1):                                            # 400 SNV entries per truth set
        p = rng.choice(np.arange(2, WALK_L - 20), 400, replace=False)
        base.append((p, gc[p - 1], (gc[p - 1] + rng.integers(1, 4, 400)) % 4))
    extra, vcfs, plans = [set(), set()], [], []
    for v, n in enumerate(WALK_SIZES):
        w = v % 2
        pos = rng.integers(2, WALK_L - 20, n).astype(np.int32)
        from_truth = rng.random(n) < 0.4                        # four in ten are entries of the truth set, at their place in the order
        j = rng.integers(0, 400, n)
        pos = np.where(from_truth, base[w][0][j], pos).astype(np.int32)
        o = np.argsort(pos, kind="stable")
        pos, j, from_truth = pos[o], j[o], from_truth[o]
        ref = gc[pos - 1].astype(np.int32)
        alt = np.where(from_truth, base[w][2][j], (ref + 1 + pos % 3) % 4).astype(np.int32)
        kept = rng.random(n) < 0.9
        flags = (kept.astype(np.uint8) | np.uint8(PLAIN)).astype(np.uint8)
        plan = seam_plan(n)
        for i, kind in plan.items():
            p = int(pos[i])
            kept[i], flags[i] = True, nz.F_PASS | PLAIN
            if kind == INDEL:                                   # the deletion of the base behind p, spelled with a shared suffix
                extra[w].add((p, g[p - 1:p + 1], g[p - 1]))
                ref[i], alt[i] = nz.code(g[p - 1:p + 2]), nz.code(g[p - 1] + g[p + 1])
            elif kind == MNP2:                                  # two SNV entries as one record
                a, b = snv(g, p, 2), snv(g, p + 1, 3)
                extra[w].update((a, b))
                ref[i], alt[i] = nz.code(g[p - 1:p + 1]), nz.code(a[2] + b[2])
            elif kind == NOKEY:
                flags[i] |= nz.F_NOKEY
            else:
                ref[i], alt[i] = long_id, gc[p - 1]
        vcfs.append(("n%d" % n, w, [pos, ref, alt, np.where(kept, 50, 5).astype(np.float32), flags], True))
        plans.append(plan)
    truths = []
    for w in (0, 1):
        p, r, a = base[w]
        truths.append((0, [(int(x), int(y), int(z)) for x, y, z in zip(p, r, a)] + sorted(extra[w])))
    reasons = {"n%d" % n: sum(k in (NOKEY, LONG) for k in plan.values()) for n, plan in zip(WALK_SIZES, plans)}
    return Family("walk", [g], truths, vcfs, planted={"plans": plans}, reasons=reasons, shuffle=("n16385", "n1025", "n3"), coder=code)


def present_walk(f, res):
    assert [len(c[0]) for c in f.cols[:len(WALK_SIZES)]] == list(WALK_SIZES) and [v[1] for v in f.vcfs[:10]] == [0, 1] * 5
    for v, (n, plan) in enumerate(zip(WALK_SIZES, f.planted["plans"])):
        must = {0, n - 1} | {s + d for s in range(1024, n + 1, 1024) for d in (-1, 0)}
        assert {i for i in must if 0 <= i < n} <= set(plan), n
        for s in (16384, 65536):                                # a kind of its own at every index around either seam
            if n > s:
                assert len({plan[s + d] for d in (-2, -1, 0, 1) if s + d < n}) == min(4, n - s + 2)
        if n == 0:
            assert not res[v][0][0].any() and not res[v][1][0].any()
            continue
        nzc, atc, ty = res[v]
        rows, nb = ty[None][2], len(vt.DEFAULT_EDGES)
        for i, kind in plan.items():
            case = (n, i, kind)
            if kind == INDEL:
                assert nzc[2][i] == nz.RESCUED and nzc[6][i] >= 0 and atc[2][i] == at.UNEQUAL and rows[i] == vt.row_of(vt.DEL, 1, vt.DEFAULT_EDGES), case
            elif kind == MNP2:
                assert atc[2][i] == at.RESCUED and atc[3][i] == 2 and atc[4][i] == 3 and nzc[2][i] == nz.UNCHANGED and rows[i] // nb == vt.MNP, case
            elif kind == NOKEY:
                assert nzc[2][i] == nz.NOKEY and atc[2][i] == at.NOKEY and rows[i] == 5 * nb + vt.NOKEY, case
            else:
                assert nzc[2][i] == nz.LONG and atc[2][i] == at.LONG and rows[i] < 5 * nb, case
        assert int(nzc[0][NR["nokey"]]) + int(nzc[0][NR["long"]]) == f.reasons["n%d" % n]
        if n >= 1023:
            assert int(nzc[0][NR["tp"]]) > n // 4 and int(nzc[0][NR["kept"]]) < n


# ---- (5) both ends of the genome, bytes that are no base ------------------------------------------------------------------------------
def ends_family(L):
    """Genome 0 begins with a homopolymer (AAAAAAAAAAAAAAC), genome 1 with (AC)n (ACACACACACACACT); both end with ACGTCA at L.  Per
    genome: an entry whose walk stops at q = 1, respelled by records of 1-, 2- and 13-base REFs; records and entries that end at L
    and one base past it; the smallest and the largest position."""
    assert L % 8 in (0, 1, 7)
    rng = np.random.default_rng(83 + L)
    heads = ("AAAAAAAAAAAAAAC", "ACACACACACACACT")
    genomes = []
    for h in heads:
        g = rand_genome(rng, L)
        g[:15] = h
        g[15] = "G"
        g[L - 7:] = "TACGTCA"
        genomes.append("".join(g))
    a, c = genomes
    t0 = [(3, "AA", "A"), (2, "A", "AA"), (L - 2, "TCA", "T"), (L, "A", "AAC"), (L, "AT", "A"), (40, a[39], BASES[(BASES.index(a[39]) + 1) % 4])]
    r0 = [line(0, "A", "C"), line(5, "A", "AA"), line(6, "AA", "A"), line(1, a[:13], a[1:13]), line(1, "A", "AA"), line(1, "AA", "A"),
          line(2, a[1:13], a[1:2] + a[1:13]), line(L - 3, "GTCA", "GT"), line(L - 1, "CA", "CAAC"), line(L, "A", "G"), line(L - 1, "CA", "C"),
          line(L, "AT", "A"), line(L - 1, "CAG", "C"), line(L + 1, "A", "C"), line(at.POS_LIMIT - 1, "A", "C")]
    t1 = [(3, "ACA", "A"), (1, "A", "ACA"), (L - 1, "CA", "C")]
    r1 = [line(7, "ACA", "A"), line(8, "CAC", "C"), line(1, c[:13], c[:11]), line(5, "A", "ACA"), line(2, "C", "CAC"), line(1, c[:11], c[:13]),
          line(L - 4, "CGTCA", "CGTC"), line(L - 4, c[L - 5:] + "A", "C")]
    reasons = {"homopolymer": 5, "dinucleotide": 1}             # RANGE: position 0, three that end past L, the largest position; one on genome 1
    return Family("ends%d" % (L % 8), genomes, [(0, t0), (1, t1)], [("homopolymer", 0, r0, True), ("dinucleotide", 1, r1, True)],
                  planted={"L": L}, reasons=reasons, shuffle=("homopolymer", "dinucleotide"))


def present_ends(f, res):
    L = f.planted["L"]
    assert [len(g) for g in f.genomes] == [L, L]
    A, AA, C = nz.code("A"), nz.code("AA"), nz.code("C")
    rec, tru, cls, npos, nref, nalt, row = res[0][0]
    forms = list(zip(npos.tolist(), nref.tolist(), nalt.tolist()))
    assert forms[1:7] == [(1, A, AA), (1, AA, A), (1, AA, A), (1, A, AA), (1, AA, A), (1, A, AA)]      # every walk stops at q = 1
    assert cls[1:7].tolist() == [nz.RESCUED] * 6 and set(row[1:7].tolist()) == {0, 1}
    assert forms[7] == (L - 2, nz.code("TCA"), nz.code("T")) and cls[7] == nz.RESCUED                  # ends at L
    assert forms[8] == (L, A, nz.code("AAC")) and cls[8] == nz.RESCUED and cls[9] == nz.UNCHANGED and cls[10] == nz.UNCHANGED
    assert cls[[0, 11, 12, 13, 14]].tolist() == [nz.RANGE] * 5 and int(rec[NR["range"]]) == 5          # one base past L
    assert int(tru[NT["not_normalisable"]]) == 1 and int(tru[NT["forms"]]) == 6 and int(tru[NT["found"]]) == 5
    rec, tru, cls, npos, nref, nalt, row = res[1][0]
    forms = list(zip(npos.tolist(), nref.tolist(), nalt.tolist()))
    assert forms[:3] == [(1, nz.code("ACA"), A)] * 3 and forms[3:6] == [(1, A, nz.code("ACA"))] * 3 and cls[:6].tolist() == [nz.RESCUED] * 6
    assert forms[6] == (L - 1, nz.code("CA"), C) and cls[6] == nz.RESCUED and cls[7] == nz.RANGE
    assert tru.tolist() == [3, 3, 3, 3, 0]


NOBASE = ("N", "R", "-", "n", "y")
LOWER = ("a", "c", "g", "t")
RUN = 2049


def nobase_family():
    """Genome 0: per byte Z a block Z XXXXXX W (X = G, or A behind g): a deletion in the run walks down to Z -- NOBASE for the five
    bytes that are no base, a form in upper-case codes behind the four lower-case bases; the truth set spells the same deletion two
    bases further left.  Behind the blocks `acgtac` under upper-case REFs.  Genome 1: a homopolymer of 2049 bases with a deletion of
    twelve spelled in 13 bases at its far end: 256 packed words of walk."""
    rng = np.random.default_rng(89)
    g = rand_genome(rng, 40 * (len(NOBASE) + len(LOWER)) + 80)
    truth, recs, blocks = [], [], []
    for k, z in enumerate(NOBASE + LOWER):
        b = 40 + 40 * k
        x = "A" if z == "g" else "G"
        g[b - 1:b + 7] = z + x * 6 + ("T" if k % 2 else "C")
        truth.append((b + 2, x + x, x))
        recs += [line(b + 4, x + x, x), line(b + 2, x + x, x), line(b + 5, x, x + x), line(b + 1, x, BASES[(BASES.index(x) + 1) % 4])]
        blocks.append((z, b, x))
    b = 40 * (len(NOBASE) + len(LOWER)) + 50
    g[b - 1:b + 5] = "acgtac"
    truth.append((b + 1, "CG", "C"))
    recs += [line(b, "ACGT", "ACT"), line(b + 2, "G", "A"), line(b, "AC", "CA")]
    run = rand_genome(rng, 10) + ["C"] + ["A"] * RUN + ["T"] + rand_genome(rng, 20)
    far = 11 + RUN - 12                                         # the last 13 bases of the run
    t1 = [(11, "C" + "A" * 12, "C"), (20, "A", "AA")]
    r1 = [line(far, "A" * 13, "A"), line(far + 12, "A", "AA"), line(far + 6, "A" * 7 + "T", "A" * 6 + "T")]
    return Family("nobase", [g, run], [(0, truth), (1, t1)], [("blocks", 0, recs, True), ("run", 1, r1, True)], planted={"blocks": blocks},
                  reasons={"blocks": 3 * len(NOBASE), "run": 0}, shuffle=("blocks",))


def present_nobase(f, res):
    g = f.genomes[0]
    assert set(g) - set("ACGTacgt") == set(NOBASE) and set(LOWER) <= set(g)
    rec, tru, cls, npos, nref, nalt, row = res[0][0]
    forms = list(zip(npos.tolist(), nref.tolist(), nalt.tolist()))
    for k, (z, b, x) in enumerate(f.planted["blocks"]):
        got, c = forms[4 * k:4 * k + 4], cls[4 * k:4 * k + 4].tolist()
        if z in NOBASE:                                         # the walk meets the byte: no form; the entry stays in under its spelling
            assert c == [nz.NOBASE, nz.NOBASE, nz.NOBASE, nz.UNCHANGED] and got[0] == (b + 4, nz.code(x + x), nz.code(x)) and row[4 * k + 1] >= 0, (z, c)
        else:                                                   # a base: the form is spelled in upper-case codes from the lower-case byte
            want = (b, nz.code(z.upper() + x), nz.code(z.upper()))
            assert got[0] == got[1] == want and c[:2] == [nz.RESCUED, nz.RESPELLED] and got[2] == (b, nz.code(z.upper()), nz.code(z.upper() + x)), (z, c, got)
    k = 4 * len(f.planted["blocks"])
    assert cls[k:k + 3].tolist() == [nz.RESCUED, nz.UNCHANGED, nz.UNCHANGED]                          # lower case under an upper-case REF
    assert int(rec[NR["nobase"]]) == 3 * len(NOBASE) and int(tru[NT["not_normalisable"]]) == len(NOBASE) and not int(rec[NR["refmismatch"]])
    rec, tru, cls, npos, nref, nalt, row = res[1][0]
    assert len(f.genomes[1]) // 8 >= 256 and cls.tolist() == [nz.RESCUED, nz.RESCUED, nz.RESPELLED] and row.tolist() == [0, 1, -1]
    assert npos.tolist() == [11, 11, 11] and int(f.cols[1][0][0]) - 11 >= 2036                        # 2036 steps of the walk


@functools.lru_cache(maxsize=None)
def family(name):
    return {"pairs": pairs_family, "longshort": longshort_family, "tables": tables_family, "walk": walk_family, "ends0": lambda: ends_family(200),
            "ends1": lambda: ends_family(201), "ends7": lambda: ends_family(207), "nobase": nobase_family}[name]()


PRESENT = {"pairs": present_pairs, "longshort": present_longshort, "tables": present_tables, "walk": present_walk, "ends0": present_ends,
           "ends1": present_ends, "ends7": present_ends, "nobase": present_nobase}
NAMES = tuple(PRESENT)


# ---- the judges that are no restatement: shared by the host test (on the restatements) and the device test (on the device's output) ----
def check_ties(f, v, forms, ncls, na, rows):
    """The ties between the three passes for VCF v.  forms: (npos, nref, nalt) and ncls of the normal-form pass; na: the atom
    counts; rows: the type rows at the family's first edges.  Type and size are invariant under normalisation: shifting happens to
    pure indels only and keeps their size, and trimming the prefix first or the suffix first leaves equal lengths; so vt.shape of
    the spelled form gives the row of the original record.  For equal-length records the atoms are the Hamming distance of the
    form.  And the records without a normal form are as many as the family planted.  Returns how many records were judged."""
    edges = vt.check_edges(f.edges[0])
    assert not (f.cols[v][4] & nz.F_TPLINE).any()               # (RESCUED then means: its form is an entry's)
    has = np.isin(ncls, HAS_FORM)
    for i in np.flatnonzero(has):
        r, a = nz.spell(forms[1][i]), nz.spell(forms[2][i])
        kind, size = vt.shape(r, a)
        assert rows[i] == vt.row_of(kind, size, edges), (f.name, v, i, r, a)
        if len(r) == len(a):
            assert na[i] == hamming(r, a), (f.name, v, i, r, a)
    left_out = int((~has).sum())
    assert left_out == (0 if f.reasons is None else f.reasons[f.vcfs[v][0]]), (f.name, f.vcfs[v][0], left_out)
    return int(has.sum())


def check_partition(f, v, forms, ncls, row):
    """Forms partition sequences, by plain slicing of the genome: two records with a normal form share their form iff substituting
    them gives one string; and a record's truth row is the first entry (in table order) that gives the record's string, -1 where
    no entry does.  (An entry takes part where its REF is the genome's: in these families no record with a normal form makes the
    string of an entry without one.)  Returns how many records have such an entry."""
    g = f.genome_of(v).upper()
    first = {}
    for j, (p, r, a) in enumerate(f.order[f.vcfs[v][1]]):
        r, a = nz.spell(r), nz.spell(a)
        if r is not None and a is not None and r != a and p >= 1 and g[p - 1:p - 1 + len(r)] == r:
            first.setdefault(g[:p - 1] + a + g[p - 1 + len(r):], j)
    by_form, by_seq, n = {}, {}, 0
    for i, (p, r, a) in enumerate(f.strings(v)):
        if ncls[i] not in HAS_FORM:
            continue
        form, seq = (int(forms[0][i]), int(forms[1][i]), int(forms[2][i])), g[:p - 1] + a + g[p - 1 + len(r):]
        assert by_form.setdefault(form, seq) == seq and by_seq.setdefault(seq, form) == form, (f.name, v, i, p, r, a)
        assert row[i] == first.get(seq, -1), (f.name, v, i, p, r, a)
        n += row[i] >= 0
    return n
