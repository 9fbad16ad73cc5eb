"""Draws for the rescue-ROC sweep, shared by the host test and the GPU tests: truth sets that hold indels with
many spellings (the planted repeats of test_normalize_host) beside runs of adjacent SNVs, and records that respell the indels,
join the SNVs into MNPs (whole and partial), repeat entries as they are spelled, miss, and have no form or no atoms at all --
at every QUAL the bins treat differently and under every flag.  `conditions` checks what the GPU comparisons rest on."""
import numpy as np

from quasimodo_amd import atomize as at
from quasimodo_amd import normalize as nz
from quasimodo_amd import rescueroc as rr
from test_gpu_normalize import G17, G600, codes, draw, respell, truth_variants
from test_normalize_host import BASES

QUALS = [np.nan, -1.0, -np.inf, 0.0, 19.999, 20.0, 255.9, 256.0, np.inf]   # no bin; bins 0, 19, 20, 255; clamped twice


def other_base(rng, ch):
    return BASES[(BASES.index(ch) + int(rng.integers(1, 4))) % 4]


def snv_runs(g, rng, n):
    """n SNVs against the genome's REF in runs of two or three adjacent positions: what a caller joins into one MNP"""
    out, seen = [], set()
    while len(out) < n:
        p = int(rng.integers(1, len(g) - 2))
        for k in range(int(rng.integers(2, 4))):
            if len(out) < n and p + k not in seen and g[p + k - 1] in BASES:
                seen.add(p + k)
                out.append((p + k, g[p + k - 1], other_base(rng, g[p + k - 1])))
        if len(seen) >= len(g) - 4:
            break
    return out


def truth_set(g, rng, n):
    """string variants with exactly n distinct entries where the genome has room for them (n = 1: one indel)"""
    if n == 1:
        return draw(g, rng, 1, len(g) >= 600)
    vs, want_snv = [], min(n // 2, len(g) // 2)
    vs += snv_runs(g, rng, want_snv)
    for _ in range(max(n // 10, 2)):                # MNPs the truth set spells itself: entries with two or three atoms
        ln = int(rng.integers(2, 4))
        p = int(rng.integers(1, len(g) - ln + 1))
        r = "".join(ch if ch in BASES else "A" for ch in g[p - 1:p - 1 + ln])
        vs.append((p, r, "".join(other_base(rng, ch) for ch in r)))
    for _ in range(50):
        have = len(nz.truth_order(*codes(vs)))
        if have >= n:
            break
        vs += truth_variants(g, rng, max(n - have, 8))[:n - have]
    while len(nz.truth_order(*codes(vs))) > n:
        vs.pop()
    return vs


def records(g, rng, n, tvs, sorted_, pass_is_bin=False, all_iddot=False):
    """(pos, ref, alt, qual, flags) of one VCF.  pass_is_bin: PASS <=> valid codes and QUAL bin >= 20 (the filter the passes
    report at); else PASS is drawn, so that hits sit among records that are not kept too."""
    pos, ref, alt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    snvs = [v for v in tvs if len(v[1]) == 1 and len(v[2]) == 1]
    by_pos = {v[0]: v for v in snvs}
    mnps = [v for v in tvs if len(v[1]) == len(v[2]) >= 2 and all(x != y for x, y in zip(v[1], v[2]))]
    indels = [v for v in tvs if v not in snvs] or tvs
    others = draw(g, rng, max(min(n // 4, 200), 4), len(g) >= 600) if n else []
    for i in range(n):
        u = rng.random()
        v = indels[int(rng.integers(0, len(indels)))]
        if u < 0.25:
            v = respell(g, rng, *v) or v
        elif u < 0.35:
            pass                                    # spelled as the truth spells it
        elif u < 0.55 and snvs:                     # an MNP over a truth SNV and its neighbours: whole, partial or padded
            p0 = snvs[int(rng.integers(0, len(snvs)))][0]
            ln = int(rng.integers(1, 4))
            p0 = max(1, min(p0 - int(rng.integers(0, ln)), len(g) - ln + 1))
            r = "".join(g[q - 1] if g[q - 1] in BASES else "A" for q in range(p0, p0 + ln))
            a = "".join(by_pos[q][2] if q in by_pos and rng.random() < 0.85 else (r[q - p0] if rng.random() < 0.5 else other_base(rng, r[q - p0]))
                        for q in range(p0, p0 + ln))
            v = (p0, r, a)                          # (r == a now and then: NOVAR)
        elif u < 0.60 and snvs:
            v = snvs[int(rng.integers(0, len(snvs)))]
        elif u < 0.65 and mnps:                     # one atom of an MNP the truth set spells: the entry is carried in part
            m = mnps[int(rng.integers(0, len(mnps)))]
            k = int(rng.integers(0, len(m[1])))
            v = (m[0] + k, m[1][k], m[2][k])
        elif u < 0.85:
            v = others[int(rng.integers(0, len(others)))]
        elif u < 0.88:
            v = (int(rng.choice([0, len(g), len(g) + 1, len(g) + 40])), "AC", "A")   # RANGE by normal form
        pos[i], ref[i], alt[i] = v[0], nz.code(v[1]), nz.code(v[2])
        if 0.88 <= u < 0.94:                        # a dictionary id (valid, no inline code), or a code that is no allele
            ref[i] = int(rng.choice([nz.DICT | 3, nz.DICT | 4, -1, 5]))
        elif u >= 0.94:
            alt[i] = nz.DICT | int(rng.integers(0, 3))
    qual = (rng.random(n) * 300).astype(np.float32)
    special = rng.random(n) < 0.35
    qual = np.where(special, np.array(QUALS, np.float32)[rng.integers(0, len(QUALS), n)], qual).astype(np.float32)
    ok = lambda c: ((c >= 0) & (c < 4)) | (c >= 0x08000000)
    valid = ok(ref) & ok(alt)
    if pass_is_bin:
        passed = valid & (np.array([rr.qual_bin(q, 256) for q in qual], np.int64) >= 20)
    else:
        passed = valid & (rng.random(n) < 0.6)
    iddot = np.ones(n, bool) if all_iddot else rng.random(n) > 0.15
    nokey = rng.random(n) < 0.04
    tpline = rng.random(n) < 0.03
    flags = (passed.astype(np.uint8) | (iddot.astype(np.uint8) << 1) | (nokey.astype(np.uint8) << 2) | (tpline.astype(np.uint8) << 3))
    if sorted_ and n:
        o = np.argsort(pos, kind="stable")
        pos, ref, alt, qual, flags = pos[o], ref[o], alt[o], qual[o], flags[o]
    return (np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(ref, np.int32), np.ascontiguousarray(alt, np.int32),
            np.ascontiguousarray(qual, np.float32), np.ascontiguousarray(flags, np.uint8))


# the batch of the main GPU comparison: sizes around the steps of a span (1024 records) and of a workgroup (16 384), several VCFs
# per truth set, two truth sets, one VCF without a genome
SIZES = [0, 1, 2, 1023, 1024, 1025, 16384, 16385, 300]
WHICH = [0, 0, 1, 0, 1, 0, 0, 1, 0]
NO_GENOME = 8
GENOMES = [G600, G17]
TRUTH_N = [2000, 65]


def family(seed, sorted_, sizes=SIZES, which=WHICH, truth_n=TRUTH_N, **kw):
    """(truth variants per truth set, their code arrays, the columns of every VCF)"""
    rng = np.random.default_rng(seed)
    tvs = [truth_set(g, rng, n) for g, n in zip(GENOMES, truth_n)]
    truths = [codes(v) for v in tvs]
    cols = [records(GENOMES[w], rng, n, tvs[w], sorted_, **kw) for n, w in zip(sizes, which)]
    return tvs, truths, cols


def conditions(genome, truth, cols, pass_is_bin=False):
    """What a comparison on this VCF rests on, as a dict of counts (the host test asserts them for the draws the GPU tests use):
    rescued records by either matching, partially carried entries, the distinct best bins of either side"""
    pos, ref, alt, qual, flags = cols
    dn, da = {}, {}
    rr.sweep_norm(genome, truth, pos, ref, alt, qual, flags, 256, detail=dn)
    rr.sweep_atom(truth, pos, ref, alt, qual, flags, 256, detail=da)
    ent = nz.truth_order(*truth)
    index = set(ent)
    forms, _ = nz.truth_forms(genome, *truth)
    rescued_n = rescued_a = 0
    for i in range(len(pos)):
        f = int(flags[i])
        if f & 4 or rr.qual_bin(qual[i], 256) < 0:
            continue
        key = (int(pos[i]), int(ref[i]), int(alt[i]))
        if key in index:
            continue
        if nz.form_codes(genome, *key)[1:] in forms and nz.is_inline(key[1]) and nz.is_inline(key[2]):
            rescued_n += 1
        why, atoms = at.atoms_codes(*key)
        if why is None and all(k in _aset(da) for _, k in atoms):
            rescued_a += 1
    partial = sum(1 for j, atoms in enumerate(da["per"]) if atoms is not None and j not in da["best"]
                  and any(k in da["best_atom"] for k in atoms))
    out = dict(rescued_n=rescued_n, rescued_a=rescued_a, partial_entries=partial, bins_n=len(set(dn["best"].values())),
               bins_a=len(set(da["best"].values())))
    if pass_is_bin:
        bins = np.array([rr.qual_bin(q, 256) for q in qual], np.int64)
        ok = lambda c: ((c >= 0) & (c < 4)) | (c >= 0x08000000)
        out["pass_is_bin"] = bool(np.array_equal((flags & 1) != 0, ok(ref) & ok(alt) & (bins >= 20)))
        out["all_iddot"] = bool(((flags & 2) != 0).all())
    return out


def _aset(detail):
    if "aset" not in detail:
        detail["aset"] = set().union(*[set(x) for x in detail["per"] if x is not None]) if detail["per"] else set()
    return detail["aset"]
