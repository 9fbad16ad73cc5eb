"""The planted family of the haplotype tests: a random genome with planted repeats, a truth set and the
records of one VCF, laid out in slots of SLOT bases so that -- at the default gap -- every planted case is a site of its own.
The cases are planted, not drawn: a random family would be all LONE and OUTSIDE and prove nothing.  Strings throughout; `codes`
turns them into the columns the device takes.

What this family does NOT reach (Family(20), the largest one the per-VCF comparisons use: 430 truth entries, 184 sites): a second
step of k_hap_rank or a second block of k_hap_pairs (six words of the site bitmap), a second gather round of k_hap_replay (no
site holds more than some 16 entries), anything particular on the 255|256 seam of k_hap_sites, a byte that is no base (the genome
is pure ACGT), a window clipped at 1 or at L + 1 (the first planted base is at 80, the last slot is empty), alleles of 8 to 13
bases.  Those are planted by haplo_edges.py."""
import numpy as np

from quasimodo_amd import haplo as hp
from quasimodo_amd.normalize import DICT

BASES = "ACGT"
SLOT = 60
CASES = ("snv_del", "del_snv", "snv_del_wrong", "shift", "shift_wrong", "mnp_snvs", "snvs_mnp", "two_ins", "lone", "outside",
         "straddle", "dup", "eight_lines", "nine_lines", "eight_entries", "nine_entries", "w256", "w257", "toolong", "matched",
         "unusable")
SLOTS = {"w256": 6, "w257": 6, "toolong": 7}


def other(rng, *not_these):
    return str(rng.choice([c for c in BASES if c not in not_these]))


class Family:
    """genome: str; truth: [(p, REF, ALT)]; recs: [(p, REF, ALT, kept, flags beyond PASS)]; planted: [(case, first base)]"""

    def __init__(self, seed, repeats=6, gap=hp.DEFAULT_GAP):
        rng = np.random.default_rng(seed)
        plan = [c for c in CASES for _ in range(repeats if c not in SLOTS else 1)]
        plan += ["snv_del", "del_snv", "shift", "mnp_snvs", "snvs_mnp"] * 7 + ["snv_del_wrong", "shift_wrong"] * 25
        rng.shuffle(plan)
        n_slots = 2 + sum(SLOTS.get(c, 1) for c in plan)
        g = [BASES[i] for i in rng.integers(0, 4, n_slots * SLOT)]
        self.truth, self.recs, self.planted = [], [], []
        at = SLOT
        for case in plan:
            b = at + 20                             # 1-based, well inside the slot
            getattr(self, "_" + case)(rng, g, b)
            self.planted.append((case, b))
            at += SLOTS.get(case, 1) * SLOT
        self.genome = "".join(g)
        self.gap = gap

    # G[p] while the genome is still a list
    @staticmethod
    def _at(g, p, n=1):
        return "".join(g[p - 1:p - 1 + n])

    def _rec(self, p, r, a, kept=True, extra=hp.F_IDDOT):
        self.recs.append((p, r, a, kept, extra))

    def _snv_del(self, rng, g, b):                  # truth: SNV beside a deletion anchored on it; the caller: one complex row
        x = other(rng, g[b - 1], g[b + 1])
        self.truth += [(b, g[b - 1], x), (b, self._at(g, b, 3), g[b - 1])]
        self._rec(b, self._at(g, b, 3), x)

    def _del_snv(self, rng, g, b):                  # the reverse
        x = other(rng, g[b - 1], g[b + 1])
        self.truth.append((b, self._at(g, b, 3), x))
        self._rec(b, g[b - 1], x)
        self._rec(b, self._at(g, b, 3), g[b - 1], extra=hp.F_IDDOT if rng.random() < 0.8 else 0)

    def _snv_del_wrong(self, rng, g, b):            # ... with the SNV's base changed
        x = other(rng, g[b - 1], g[b + 1])
        self.truth += [(b, g[b - 1], x), (b, self._at(g, b, 3), g[b - 1])]
        self._rec(b, self._at(g, b, 3), other(rng, g[b - 1], g[b + 1], x))

    def _run(self, rng, g, b, n=6):                 # a homopolymer run b .. b + n - 1 with other bases on both sides
        c = other(rng, g[b - 2], g[b + n - 1])
        g[b - 1:b - 1 + n] = c * n
        return c

    def _shift(self, rng, g, b):                    # one deletion in a repeat, left-aligned in the truth set, shifted by the caller
        c = self._run(rng, g, b)
        self.truth.append((b - 1, g[b - 2] + c, g[b - 2]))
        self._rec(b + 2, c + c, c)

    def _shift_wrong(self, rng, g, b):              # ... of another length
        c = self._run(rng, g, b)
        self.truth.append((b - 1, g[b - 2] + c, g[b - 2]))
        self._rec(b + 2, c + c + c, c)

    def _mnp_snvs(self, rng, g, b):                 # truth: an MNP; the caller: its SNVs
        x, y = other(rng, g[b - 1]), other(rng, g[b])
        self.truth.append((b, self._at(g, b, 2), x + y))
        self._rec(b, g[b - 1], x)
        self._rec(b + 1, g[b], y)

    def _snvs_mnp(self, rng, g, b):
        x, y = other(rng, g[b - 1]), other(rng, g[b])
        self.truth += [(b, g[b - 1], x), (b + 1, g[b], y)]
        self._rec(b, self._at(g, b, 2), x + y)

    def _two_ins(self, rng, g, b):                  # two insertions at one point
        self.truth.append((b, g[b - 1], g[b - 1] + "AC"))
        self._rec(b, g[b - 1], g[b - 1] + "A")
        self._rec(b, g[b - 1], g[b - 1] + "C")

    def _lone(self, rng, g, b):                     # the site's only entry is found; an unmatched line beside it
        x = other(rng, g[b - 1])
        self.truth.append((b, g[b - 1], x))
        self._rec(b, g[b - 1], x)
        self._rec(b + 3, g[b + 2], other(rng, g[b + 2]))

    def _outside(self, rng, g, b):
        self._rec(b, g[b - 1], other(rng, g[b - 1]))

    def _straddle(self, rng, g, b):                 # a deletion that starts inside the window and ends behind it
        self.truth.append((b, g[b - 1], other(rng, g[b - 1])))
        self._rec(b + 7, self._at(g, b + 7, 7), g[b + 6])

    def _dup(self, rng, g, b):                      # the complex row twice
        self._snv_del(rng, g, b)
        self.recs.append(self.recs[-1])

    def _pairs(self, rng, g, b, n):                 # n MNPs of two bases, side by side; their SNVs
        mnps, snvs = [], []
        for k in range(n):
            p = b + 2 * k
            x, y = other(rng, g[p - 1]), other(rng, g[p])
            mnps.append((p, self._at(g, p, 2), x + y))
            snvs += [(p, g[p - 1], x), (p + 1, g[p], y)]
        return mnps, snvs

    def _eight_lines(self, rng, g, b):              # exactly eight open lines against four open entries: MATCH
        mnps, snvs = self._pairs(rng, g, b, 4)
        self.truth += mnps
        for s in snvs:
            self._rec(*s)

    def _nine_lines(self, rng, g, b):
        self._eight_lines(rng, g, b)
        self._rec(b + 9, g[b + 8], other(rng, g[b + 8]))

    def _eight_entries(self, rng, g, b):
        mnps, snvs = self._pairs(rng, g, b, 4)
        self.truth += snvs
        for m in mnps:
            self._rec(*m)

    def _nine_entries(self, rng, g, b):
        self._eight_entries(rng, g, b)
        self.truth.append((b + 9, g[b + 8], other(rng, g[b + 8])))

    def _chain(self, rng, g, b, last, step=20):     # SNV entries b, b + step, ..., last: one site at the default gap
        for k, p in enumerate(list(range(b, last, step)) + [last]):
            self.truth.append((p, g[p - 1], other(rng, g[p - 1])))
            if k >= 2:                              # all but two entries are found
                self._rec(*self.truth[-1])
        self._rec(b + 5, g[b + 4], other(rng, g[b + 4]))

    def _w256(self, rng, g, b):                     # a window of exactly 256 bases at the default gap: 236 + 2 * 10
        self._chain(rng, g, b, b + 235)

    def _w257(self, rng, g, b):
        self._chain(rng, g, b, b + 236)

    def _toolong(self, rng, g, b):
        self._chain(rng, g, b, b + 300)

    def _matched(self, rng, g, b):                  # spelled alike: an SNV, an insertion, one line that is not kept
        x = other(rng, g[b - 1])
        self.truth += [(b, g[b - 1], x), (b + 2, g[b + 1], g[b + 1] + "GT")]
        self._rec(b, g[b - 1], x, extra=hp.F_IDDOT | (hp.F_TPLINE if rng.random() < 0.3 else 0))
        self._rec(b + 2, g[b + 1], g[b + 1] + "GT", kept=rng.random() < 0.7)

    def _unusable(self, rng, g, b):                 # every reason, on both sides where a truth set can hold it
        self.truth += [(b, other(rng, g[b - 1]), g[b - 1]), (b + 1, "A" * 14, "C")]          # REFMISMATCH, LONG
        self._rec(b + 2, other(rng, g[b + 1]), g[b + 1])                                     # REFMISMATCH
        self._rec(b + 3, "ACGTACGTACGTACG", "A")                                             # LONG
        self._rec(b + 4, g[b + 3], other(rng, g[b + 3]), extra=hp.F_IDDOT | hp.F_NOKEY)      # NOKEY
        self._rec(b + 5, g[b + 4], g[b + 4])                                                 # NOVAR
        self._rec(len(g) - 1, "ACGT", "A")                                                   # RANGE (the genome ends first)
        self._rec(b + 6, g[b + 5], other(rng, g[b + 5]), kept=False)                         # NOTKEPT

    def columns(self, rng=None, keep=None):
        """(pos, ref, alt int32, qual float32, flags uint8) of the records (keep: indices, in that order; rng: shuffled)"""
        idx = list(range(len(self.recs))) if keep is None else list(keep)
        if rng is not None:
            rng.shuffle(idx)
        else:
            idx.sort(key=lambda i: self.recs[i][0])
        return codes([self.recs[i] for i in idx])


def allele(s):
    return hp.code(s) if len(s) <= hp.INLINE_MAX else DICT | (len(s) * 7 + BASES.index(s[0]))   # (any id: the pass reads no dictionary)


def codes(recs):
    n = len(recs)
    pos = np.array([r[0] for r in recs], np.int32).reshape(n)
    ref = np.array([allele(r[1]) for r in recs], np.int32).reshape(n)
    alt = np.array([allele(r[2]) for r in recs], np.int32).reshape(n)
    kept = np.array([bool(r[3]) for r in recs], bool).reshape(n)
    qual = np.where(kept, 50, 5).astype(np.float32)
    flags = (kept.astype(np.uint8) | np.array([r[4] for r in recs], np.uint8).reshape(n)).astype(np.uint8)
    return [pos, ref, alt, qual, flags]


def truth_codes(truth):
    n = len(truth)
    return tuple(np.array(x, np.int32).reshape(n) for x in ([t[0] for t in truth], [allele(t[1]) for t in truth], [allele(t[2]) for t in truth]))


def host_masks(cols, truth):
    """kept and TP masks as the batch makes them for these planted records (no header rules take part): kept = PASS; a TP line
    is kept and (spelled like a truth entry with valid codes, no NOKEY and ID '.', or TPLINE)"""
    ent = set(zip(*[x.tolist() for x in truth]))
    pos, ref, alt, _, flags = cols
    kept = (flags & hp.F_PASS).astype(bool)
    hit = np.array([(int(p), int(r), int(a)) in ent for p, r, a in zip(pos, ref, alt)], bool).reshape(len(pos))
    tp = kept & ((hit & ((flags & hp.F_NOKEY) == 0) & ((flags & hp.F_IDDOT) != 0)) | ((flags & hp.F_TPLINE) != 0))
    return kept, tp
