"""Indels and MNPs matched by normal form on the device (qm_batch_normalize, qm_truth_normalized; k_norm_truth / k_norm_insert /
k_norm_fill / k_norm_records / k_norm_found) against the string restatement of quasimodo_amd.normalize, tied
to the batch's columns and class masks.  Every comparison is exact: these are integers."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_columns, random_truth
from quasimodo_amd import normalize as nz
from quasimodo_amd._lib import QmvtError
from test_normalize_host import BASES, draw_variants, planted_norm_genome

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_TP_R = 3
G600 = planted_norm_genome()
G600N = G600[:49] + "N" + "G" * 8 + G600[58:]      # a walk down the G run at 51 .. 58 meets the N at 50
G17 = "AAAAAACACACACGGGG"                           # 17 bases: every walk ends at an edge


def codes(variants):
    """(pos, ref, alt) int32 arrays of string variants"""
    p = np.array([v[0] for v in variants], np.int32)
    r = np.array([nz.code(v[1]) for v in variants], np.int32)
    a = np.array([nz.code(v[2]) for v in variants], np.int32)
    return p, r, a


def respell(g, rng, p, r, a):
    """another spelling of the same event: any window of the genome that covers what differs between the genome and the sequence
    the variant makes of it -- inside a repeat that window moves freely -- or None when none fits 13 bases"""
    m = g[:p - 1] + a + g[p - 1 + len(r):]
    delta = len(m) - len(g)
    cp = cs = 0
    while cp < min(len(g), len(m)) and g[cp] == m[cp]:
        cp += 1
    while cs < min(len(g), len(m)) and g[-1 - cs] == m[-1 - cs]:
        cs += 1
    if cp < 1:
        return None
    for _ in range(20):
        s = int(rng.integers(max(1, cp - 6), cp + 1))           # 0-based start, at least 1: p >= 2
        e = int(rng.integers(len(g) - cs, min(len(g), len(g) - cs + 6) + 1))
        if not (1 <= e - s <= 13 and 1 <= e + delta - s <= 13):
            continue
        ref, alt = g[s:e], m[s:e + delta]
        if ref != alt and not set(ref + alt) - set(BASES) and g[:s] + alt + g[e:] == m:
            return s + 1, ref, alt
    return None


def draw(g, rng, n, in_repeats):
    """draw_variants, without the ones that touch a position without a base"""
    out = []
    while len(out) < n:
        out += [v for v in draw_variants(g, rng, n - len(out), in_repeats) if not set(v[1] + v[2]) - set(BASES)]
    return out


def truth_variants(g, rng, n):
    """n draws, most of them in the planted repeats where one event has many spellings, some spelled twice on purpose"""
    vs = draw(g, rng, n - n // 3, len(g) >= 600) + draw(g, rng, n // 3, False)
    for k in range(0, len(vs), 7):
        other = respell(g, rng, *vs[k])
        if other:
            vs[(k + 3) % len(vs)] = other
    return vs


def want_forms(g, truth):
    forms, _ = nz.truth_forms(g, *truth)
    return sorted(forms)


# ---- the truth side ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
@pytest.mark.parametrize("genome", [G600, G17, G600N], ids=["g600", "g17", "g600n"])
def test_truth_normalized(engine, genome, n):
    rng = np.random.default_rng(1000 + n)
    truth = codes(truth_variants(genome, rng, n))
    if n >= 63:                                     # entries without a normal form stay in under their spelling
        p, r, a = (x.copy() for x in truth)
        r[0], a[1] = nz.DICT | 7, nz.DICT | 8       # LONG
        a[2] = r[2]                                 # NOVAR
        p[3] = len(genome) + 5                      # RANGE
        r[4] = nz.code("ACGTTGCA" if genome[int(p[4]) - 1] != "A" else "CCGTTGCA")   # REFMISMATCH
        truth = (p, r, a)
    tid = engine.truth_load(*truth)
    gid = engine.genome_load(genome.encode())
    try:
        got = engine.truth_normalized(tid, gid)
        ent = engine.truth_entries(tid)
    finally:
        engine.genome_release(gid)
        engine.truth_release(tid)
    assert list(zip(*(x.tolist() for x in ent))) == nz.truth_order(*truth)
    want = want_forms(genome, truth)
    assert list(zip(*(x.tolist() for x in got))) == want
    if n == 2000 and len(genome) == 600:
        assert len(want) < len(ent[0]) - 50          # equivalent spellings did merge


# ---- the record side --------------------------------------------------------------------------------------------------------
def record_columns(g, rng, n, truth_vs, sorted_, extra=()):
    """records as respellings of truth entries, as other variants, as SNVs, and as every reason a record has no normal form"""
    pos, ref, alt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    others = draw(g, rng, max(n // 4, 4), len(g) >= 600)
    for i in range(n):
        u = rng.random()
        v = truth_vs[int(rng.integers(0, len(truth_vs)))]
        if u < 0.30:
            v = respell(g, rng, *v) or v
        elif u < 0.40:
            pass                                    # spelled as the truth spells it
        elif u < 0.60:
            v = others[int(rng.integers(0, len(others)))]
        elif u < 0.80:                              # an SNV; one in four against another REF base
            p = int(rng.integers(1, len(g) + 1))
            r = g[p - 1] if g[p - 1] in BASES and rng.random() < 0.75 else BASES[int(rng.integers(0, 4))]
            v = (p, r, BASES[(BASES.index(r) + int(rng.integers(1, 4))) % 4])
        elif u < 0.84:                              # NOVAR
            v = (v[0], v[1], v[1])
        elif u < 0.88:                              # RANGE
            v = (int(rng.choice([0, len(g), len(g) + 1, len(g) + 40])), "AC", "A")
        elif u < 0.92:                              # NOBASE where the genome has an N in front of a run; REFMISMATCH elsewhere
            v = (int(rng.integers(51, 58)), "GG", "G")
        pos[i], ref[i], alt[i] = v[0], nz.code(v[1]), nz.code(v[2])
        if 0.92 <= u < 0.96:                        # LONG: a dictionary id, or a code that is no allele
            ref[i] = int(rng.choice([nz.DICT | 3, nz.DICT | 4, -1, 5]))
        elif u >= 0.96:
            alt[i] = nz.DICT | int(rng.integers(0, 3))
    for i, (p, r, a) in enumerate(extra):         # records given as codes
        pos[i], ref[i], alt[i] = p, r, a
    qual = rng.integers(0, 300, n).astype(np.float32)
    ok = lambda c: ((c >= 0) & (c < 4)) | (c >= 0x08000000)
    passed = ok(ref) & ok(alt) & (qual >= 20)
    iddot = rng.random(n) > 0.1                     # some IDs are not `.`
    nokey = rng.random(n) < 0.03
    tpline = rng.random(n) < 0.02
    flags = (passed.astype(np.uint8) | (iddot.astype(np.uint8) << 1) | (nokey.astype(np.uint8) << 2) | (tpline.astype(np.uint8) << 3))
    if sorted_:
        o = np.argsort(pos, kind="stable")
        pos, ref, alt, qual, flags = pos[o], ref[o], alt[o], qual[o], flags[o]
    return pos, ref, alt, qual, flags.astype(np.uint8)


SIZES = [3000, 1, 255, 256, 257, 300]              # 256: the alignment of a VCF; 3000: more than one step of a span
WHICH = [0, 0, 1, 0, 1, 0]                         # truth set and genome of every VCF ...
NO_GENOME = 5                                      # ... but the last one names no genome: zero rows


def make_batch(engine, seed, sorted_, reverse_truth=False):
    rng = np.random.default_rng(seed)
    genomes = [G600N, G17]
    tvs = [truth_variants(G600N, rng, 400), truth_variants(G17, rng, 40)]
    truths = [codes(v) for v in tvs]
    for k in (0, 1):                               # a dictionary-coded entry that an equally spelled record still hits
        p, r, a = truths[k]
        truths[k] = (np.append(p, 20).astype(np.int32), np.append(r, nz.DICT | 3).astype(np.int32), np.append(a, 1).astype(np.int32))
    cols = [record_columns(genomes[w], rng, n, tvs[w], sorted_, extra=[(20, nz.DICT | 3, 1)] * min(n - 1, 3)) for n, w in zip(SIZES, WHICH)]
    load = (lambda t: tuple(x[::-1].copy() for x in t)) if reverse_truth else (lambda t: t)
    tids = [engine.truth_load(*load(t)) for t in truths]
    gids = [engine.genome_load(g.encode()) for g in genomes]
    b = engine.batch(SIZES, [tids[w] for w in WHICH], alleles=True)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    want_gids = [gids[w] for w in WHICH]
    want_gids[NO_GENOME] = -1
    return b, cols, truths, genomes, tids, gids, want_gids


def release(engine, b, tids, gids):
    b.close()
    for t in tids:
        engine.truth_release(t)
    for g in gids:
        engine.genome_release(g)


def fetch(b, gids):
    rec, tru = b.normalize(gids, columns=True)
    per = [b.normalized(v) if gids[v] >= 0 else None for v in range(b.n_vcf)]
    return rec, tru, per


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_records_against_the_restatement(engine, sorted_):
    b, cols, truths, genomes, tids, gids, want_gids = make_batch(engine, 21, sorted_)
    try:
        rec, tru, per = fetch(b, want_gids)
        classes = np.zeros(9, np.int64)
        for v, (c, w) in enumerate(zip(cols, WHICH)):
            cls = b.cls(v)
            kept, tp = (cls & 1).astype(bool), (cls & 2).astype(bool)
            if v == NO_GENOME:
                assert not rec[v].any() and not tru[v].any()
                with pytest.raises(QmvtError) as ei:
                    b.normalized(v)
                assert ei.value.code == QM_E_STATE and "named no genome" in str(ei.value)
                continue
            wrec, wtru, wcls, wp, wr, wa, wrow = nz.counts(genomes[w], truths[w], c[0], c[1], c[2], c[4], kept, tp)
            np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d" % v)
            np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d" % v)
            gp, gr, ga, gcls, grow = per[v]
            np.testing.assert_array_equal(gcls, wcls)
            np.testing.assert_array_equal(gp, wp)
            np.testing.assert_array_equal(gr, wr)
            np.testing.assert_array_equal(ga, wa)
            np.testing.assert_array_equal(grow, wrow)
            np.testing.assert_array_equal(b.normalized(v, columns=False)[0], wcls)
            tp_n = kept & (((grow >= 0) & ((c[4] & 2) != 0)) | ((c[4] & 8) != 0))
            assert not (tp & ~tp_n).any()                        # an exact TP line is always a TP_N line
            assert int(rec[v][2]) == int(tp_n.sum()) and int(rec[v][3]) == int((tp_n & ~tp).sum())
            assert int(rec[v][0]) == int(kept.sum()) and int(rec[v][1]) == int(tp.sum())
            classes += np.bincount(gcls, minlength=9)
        assert int(rec[0][3]) > 0 and int(rec[:, 3].sum()) > 20  # rescued lines
        assert (classes > 0).all(), classes                      # every class byte occurred
        assert int(rec[0][4]) > 0 and int(rec[0][5]) > 0         # respelled; some into single bases
        assert (rec[0][6:] > 0).all()                            # every reason among the kept records of the large VCF
        assert int(tru[0][3]) > 0 and int(tru[0][4]) > 0
        assert tru[0][0] == tru[1][0] == tru[3][0] and tru[0][1] == tru[3][1]
        b.set_timing(True)
        b.normalize(want_gids)
        ms = b.normalize_timings()
        assert set(ms) == {"norm_truth_ms", "norm_records_ms", "norm_found_ms"} and all(x >= 0 for x in ms.values())
        with pytest.raises(QmvtError) as ei:                     # that call kept no columns
            b.normalized(0)
        assert ei.value.code == QM_E_STATE and "QM_NORM_COLUMNS" in str(ei.value)
    finally:
        release(engine, b, tids, gids)


def test_single_base_batch_of_snvs(engine):
    """SNVs are their own normal form: TP_N lines are the TP mask, the forms found are the batch's TP_R"""
    rng = np.random.default_rng(5)
    L = len(G600)
    gcode = np.array([BASES.index(ch) for ch in G600], np.int32)
    tpos = rng.integers(1, L + 1, 300).astype(np.int32)
    tref = gcode[tpos - 1]
    talt = ((tref + rng.integers(1, 4, 300)) % 4).astype(np.int32)
    tid = engine.truth_load(tpos, tref, talt)
    gid = engine.genome_load(G600.encode())
    sizes = [2000, 257]
    cols = []
    for n in sizes:
        pos, ref, alt, qual, flags = random_columns(rng, n, L, (tpos, tref, talt), frac_truth=0.5, weird=False)
        ref = gcode[pos - 1]                                     # every REF is the genome's
        alt = np.where(alt == ref, (ref + 1) % 4, alt).astype(np.int32)
        cols.append((pos, ref, alt, qual, (flags & ~np.uint8(4)).astype(np.uint8)))
    b = engine.batch(sizes, [tid, tid], alleles=True)
    try:
        for v, c in enumerate(cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        rec, tru = b.normalize([gid, gid], columns=True)
        scal = b.scalars()
        for v in range(2):
            cls = b.cls(v)
            assert int(rec[v][2]) == int(rec[v][1]) == int(((cls & 2) != 0).sum()) > 0
            assert int(rec[v][3]) == 0 and not rec[v][4:].any()
            assert int(tru[v][2]) == int(scal[v][S_TP_R]) > 0 and int(tru[v][3]) == 0
            assert int(tru[v][0]) == int(tru[v][1]) == engine.truth_size(tid, alleles=True)
            gp, gr, ga, gcls, grow = b.normalized(v)
            assert not gcls.any() and np.array_equal(gp, cols[v][0]) and np.array_equal(gr, cols[v][1]) and np.array_equal(ga, cols[v][2])
    finally:
        release(engine, b, [tid], [gid])


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_same_answer_twice_and_with_the_truth_loaded_backwards(engine):
    b, cols, truths, genomes, tids, gids, want_gids = make_batch(engine, 33, False)
    try:
        first = fetch(b, want_gids)
        again = fetch(b, want_gids)
    finally:
        release(engine, b, tids, gids)
    b, _, _, _, tids, gids, want_gids = make_batch(engine, 33, False, reverse_truth=True)
    try:
        back = fetch(b, want_gids)
    finally:
        release(engine, b, tids, gids)
    for other in (again, back):
        np.testing.assert_array_equal(first[0], other[0])
        np.testing.assert_array_equal(first[1], other[1])
        for x, y in zip(first[2], other[2]):
            assert (x is None) == (y is None)
            for p, q in zip(x or (), y or ()):
                np.testing.assert_array_equal(p, q)              # the truth row of every rescued line included
    assert int(first[0][:, 3].sum()) > 0


# ---- state and argument errors ------------------------------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_refusals(engine):
    rng = np.random.default_rng(9)
    tvs = truth_variants(G600, rng, 50)
    truth = codes(tvs)
    tid, tid2 = engine.truth_load(*truth), engine.truth_load(*truth)
    gid, gid2 = engine.genome_load(G600.encode()), engine.genome_load(G17.encode())
    cols = [record_columns(G600, rng, 40, tvs, True) for _ in range(2)]
    b = engine.batch([40, 40], [tid, tid], alleles=True)
    sb = engine.batch([40], [tid])                              # a single-base batch
    try:
        for v in range(2):
            b.upload(v, *cols[v])
        c, msg = refused(lambda: b.normalize([gid, gid]))
        assert c == QM_E_STATE and "qm_batch_finish first" in msg          # before finish
        b.run()
        c, msg = refused(lambda: b.normalize([gid, gid]))
        assert c == QM_E_STATE
        b.finish()
        c, msg = refused(b.normalize_counts)                                # getters before the pass
        assert c == QM_E_STATE and "no qm_batch_normalize behind the latest run" in msg
        c, msg = refused(lambda: b.normalized(0))
        assert c == QM_E_STATE and "no qm_batch_normalize behind the latest run" in msg
        c, msg = refused(b.normalize_timings)
        assert c == QM_E_STATE
        c, msg = refused(lambda: b.normalize([gid, gid2]))                  # two genomes for one truth set
        assert c == QM_E_INVAL and "VCF 0 and VCF 1" in msg and "genomes %d and %d" % (gid, gid2) in msg
        c, msg = refused(lambda: b.normalize([gid, 99]))
        assert c == QM_E_INVAL and "names genome 99" in msg
        with pytest.raises(ValueError):
            b.normalize([gid])
        g = np.array([gid, gid], np.int32)
        assert b._L.qm_batch_normalize(b._h, g.ctypes.data_as(C.c_void_p), 4, None) == QM_E_INVAL
        sb.upload(0, *[x if i < 1 or i > 2 else (x & 3).astype(np.int32) for i, x in enumerate(cols[0])])
        sb.run()
        sb.finish()
        c, msg = refused(lambda: sb.normalize([gid]))                       # a single-base batch
        assert c == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        rec, _ = b.normalize([gid, -1])                                     # it does run
        assert int(rec[0][0]) > 0 and not rec[1].any()
        b.run()                                                             # a new run forgets the pass
        b.finish()
        c, msg = refused(b.normalize_counts)
        assert c == QM_E_STATE
        engine.genome_release(gid2)
        c, msg = refused(lambda: b.normalize([gid2, gid2]))                 # a released genome
        assert c == QM_E_STATE and "released genome %d" % gid2 in msg
        c, msg = refused(lambda: engine.truth_normalized(tid, gid2))
        assert c == QM_E_INVAL and "no live genome" in msg
        engine.truth_release(tid2)
        n_out = C.c_int64()
        assert engine._L.qm_truth_normalized(engine._h, tid2, gid, None, None, None, 0, C.byref(n_out)) == QM_E_INVAL
        assert engine._L.qm_truth_entries(engine._h, tid2, None, None, None, 0, C.byref(n_out)) == QM_E_INVAL
        engine.truth_release(tid)
        c, msg = refused(lambda: b.normalize([gid, gid]))                   # a released truth set
        assert c == QM_E_STATE and "truth set %d was released" % tid in msg
    finally:
        b.close()
        sb.close()
        engine.genome_release(gid)
