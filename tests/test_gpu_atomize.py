"""MNPs matched against adjacent SNVs on the device (qm_batch_atomize, qm_truth_atoms; k_atom_truth / k_atom_records /
k_atom_found) against the string restatement of quasimodo_amd.atomize, tied to the batch's columns, class masks
and scalars.  Every comparison is exact: these are integers."""
import ctypes as C

import numpy as np
import pytest

from quasimodo_amd import atomize as at
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_NPASS, S_TP_LINES, S_TP_R = 0, 1, 3
BASES = "ACGT"
TOP = (1 << 28) - 1                                 # the last position a batch and an atom hold
L = 6000


def genome(seed=2):
    rng = np.random.default_rng(seed)
    return "".join(BASES[i] for i in rng.integers(0, 4, L + 40))


G = genome()


def other(rng, ch):
    return BASES[(BASES.index(ch) + int(rng.integers(1, 4))) % 4]


def ref_at(p, n):
    return G[p - 1:p - 1 + n]


def mutate(rng, ref, must=None):
    """an ALT of the length of ref that differs in a random non-empty set of bases (and at offset `must`)"""
    alt = [other(rng, ch) if rng.random() < 0.4 else ch for ch in ref]
    k = int(rng.integers(0, len(ref))) if must is None else must
    if alt[k] == ref[k]:
        alt[k] = other(rng, ref[k])
    return "".join(alt)


def truth_variants(rng, n):
    """n string variants: SNVs (some in adjacent pairs), MNPs of 2 .. 13 bases -- a third of them laid over an SNV of the set
    with that SNV's ALT, so that atoms repeat --, and indels"""
    vs = []
    while len(vs) < max(n // 2, 1):
        p = int(rng.integers(1, L))
        vs.append((p, ref_at(p, 1), other(rng, ref_at(p, 1))))
        if rng.random() < 0.4:                      # the neighbour as well: what a caller writes as one MNP
            vs.append((p + 1, ref_at(p + 1, 1), other(rng, ref_at(p + 1, 1))))
    snvs = list(vs)
    while len(vs) < n - n // 6:
        m = int(rng.integers(2, 14))
        if rng.random() < 0.34:
            p0, _, a0 = snvs[int(rng.integers(0, len(snvs)))]
            k = int(rng.integers(0, m))
            if p0 - k < 1:
                continue
            alt = mutate(rng, ref_at(p0 - k, m), must=k)
            vs.append((p0 - k, ref_at(p0 - k, m), alt[:k] + a0 + alt[k + 1:]))
        else:
            p = int(rng.integers(1, L))
            vs.append((p, ref_at(p, m), mutate(rng, ref_at(p, m))))
    while len(vs) < n:
        p = int(rng.integers(1, L))
        m = int(rng.integers(2, 8))
        vs.append((p, ref_at(p, m), ref_at(p, 1)) if rng.random() < 0.5 else (p, ref_at(p, 1), ref_at(p, 1) + "ACGTACG"[:m]))
    return vs[:n]


def codes(variants):
    """(pos, ref, alt) int32 arrays of string variants"""
    p = np.array([v[0] for v in variants], np.int32)
    r = np.array([at.code(v[1]) for v in variants], np.int32)
    a = np.array([at.code(v[2]) for v in variants], np.int32)
    return p, r, a


def plant(truth):
    """entries that are not atomisable stay in under their spelling; two entries at the last positions"""
    p, r, a = (x.copy() for x in truth)
    r[0], a[1] = at.DICT | 7, at.DICT | 8           # LONG
    a[2] = r[2]                                     # NOVAR
    p[3], r[3], a[3] = TOP, at.code("AC"), at.code("GT")          # RANGE: its second base would lie at 2^28
    p[4], r[4], a[4] = TOP - 1, at.code("AC"), at.code("GT")      # the last MNP that is in range
    return p, r, a


# ---- the truth side ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 2000])
def test_truth_atoms(engine, n):
    rng = np.random.default_rng(1000 + n)
    truth = codes(truth_variants(rng, n))
    if n >= 63:
        truth = plant(truth)
    tid = engine.truth_load(*truth)
    try:
        got = engine.truth_atoms(tid)
        again = engine.truth_atoms(tid)
        ent = engine.truth_entries(tid)
    finally:
        engine.truth_release(tid)
    order, per, aset = at.truth_atoms(*truth)
    assert list(zip(*(x.tolist() for x in ent))) == order
    assert got.dtype == np.uint32 and got.tolist() == sorted(aset) and again.tolist() == got.tolist()
    if n >= 63:
        total = sum(len(x) for x in per if x is not None)
        assert len(aset) < total                     # atoms of overlapping entries did merge
        assert sum(x is None for x in per) >= 4      # the planted entries and the indels take no part
        assert (TOP << 4 | 7) in aset and (TOP - 1) << 4 | 2 in aset and got[-1] == (TOP << 4 | 7)


# ---- the record side --------------------------------------------------------------------------------------------------------
def record_columns(rng, n, tvs, sorted_, kept_nokey):
    """records as recombinations of adjacent truth SNVs into MNPs, MNPs with one wrong atom, truth MNPs split into SNVs, truth
    entries as they are spelled, unrelated variants, indels, and every reason a record is not atomisable"""
    nxt = {}
    for p, r, a in tvs:
        if len(r) == len(a) == 1:
            nxt.setdefault(p, (r, a))
    pairs = [(p, r, a) for p, (r, a) in sorted(nxt.items()) if p + 1 in nxt]
    mnps = [v for v in tvs if len(v[1]) == len(v[2]) >= 2]
    pos, ref, alt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i in range(n):
        u = rng.random()
        v = tvs[int(rng.integers(0, len(tvs)))]
        if u < 0.22 and pairs:                      # two (or three) adjacent truth SNVs as one MNP
            p, r, a = pairs[int(rng.integers(0, len(pairs)))]
            r2, a2 = nxt[p + 1]
            v = (p, r + r2, a + a2)
            if p + 2 in nxt and rng.random() < 0.5:
                v = (p, v[1] + nxt[p + 2][0], v[2] + nxt[p + 2][1])
            elif rng.random() < 0.3:                # ... padded with a base that does not differ
                v = (p, v[1] + ref_at(p + 2, 1), v[2] + ref_at(p + 2, 1))
            if u < 0.08:                            # one atom wrong
                k = int(rng.integers(0, 2))
                wrong = next(ch for ch in BASES if ch not in (v[1][k], v[2][k]))
                v = (p, v[1], v[2][:k] + wrong + v[2][k + 1:])
        elif u < 0.40 and mnps:                     # one SNV of a truth MNP
            p, r, a = mnps[int(rng.integers(0, len(mnps)))]
            ks = [k for k in range(len(r)) if r[k] != a[k]]
            k = ks[int(rng.integers(0, len(ks)))]
            v = (p + k, r[k], a[k])
        elif u < 0.52:
            pass                                    # spelled as the truth spells it (indels among them)
        elif u < 0.68:                              # unrelated: an SNV or an MNP anywhere
            m = int(rng.integers(1, 14))
            p = int(rng.integers(1, L))
            v = (p, ref_at(p, m), mutate(rng, ref_at(p, m)))
        elif u < 0.78:                              # an indel
            p = int(rng.integers(1, L))
            v = (p, ref_at(p, 3), ref_at(p, 1))
        elif u < 0.82:                              # NOVAR
            v = (v[0], v[1], v[1])
        elif u < 0.86:                              # RANGE, and the last MNP in range
            v = (TOP if rng.random() < 0.7 else TOP - 1, "AC", "GT")
        pos[i], ref[i], alt[i] = v[0], at.code(v[1]), at.code(v[2])
        if 0.86 <= u < 0.91:                        # LONG: a dictionary id, or a code that is no allele
            ref[i] = int(rng.choice([at.DICT | 3, at.DICT | 7, -1, 5]))
        elif 0.91 <= u < 0.94:
            alt[i] = at.DICT | int(rng.integers(0, 9))
    qual = rng.integers(0, 300, n).astype(np.float32)
    ok = lambda c: ((c >= 0) & (c < 4)) | (c >= 0x08000000)
    nokey = rng.random(n) < 0.04
    passed = ok(ref) & ok(alt) & (qual >= 20)
    if not kept_nokey:                              # FOUND == TP_R holds where no kept record lacks its key
        qual[nokey] = 5
        passed &= ~nokey
    iddot = rng.random(n) > 0.1                     # some IDs are not `.`
    tpline = rng.random(n) < 0.02
    flags = (passed.astype(np.uint8) | (iddot.astype(np.uint8) << 1) | (nokey.astype(np.uint8) << 2) | (tpline.astype(np.uint8) << 3))
    if sorted_:
        o = np.argsort(pos, kind="stable")
        pos, ref, alt, qual, flags = pos[o], ref[o], alt[o], qual[o], flags[o]
    return pos, ref, alt, qual, flags.astype(np.uint8)


SIZES = [0, 1, 255, 256, 257, 70000]                # 256: the alignment of a VCF; 70 000: more than one span, more than one workgroup
WHICH = [1, 0, 0, 1, 0, 1]                          # the truth set of every VCF: each is shared by three
KEPT_NOKEY = 4                                      # the one VCF with kept records that have no key


def make_batch(engine, seed, sorted_, reverse_truth=False):
    rng = np.random.default_rng(seed)
    tvs = [truth_variants(rng, 500), truth_variants(rng, 1200)]
    truths = [plant(codes(v)) for v in tvs]
    for k in (0, 1):                                # (the entries plant() wrote over are no longer in the truth sets)
        tvs[k] = tvs[k][5:]
    cols = [record_columns(rng, n, tvs[w], sorted_, v == KEPT_NOKEY) for v, (n, w) in enumerate(zip(SIZES, WHICH))]
    for c, w in list(zip(cols, WHICH))[2:]:         # kept LONG records spelled like the planted LONG entry: found by spelling
        c[0][:2], c[1][:2], c[2][:2] = truths[w][0][0], truths[w][1][0], truths[w][2][0]
        c[3][:2], c[4][:2] = 50, 3
        if sorted_:
            o = np.argsort(c[0], kind="stable")
            for x in c:
                x[:] = x[o]
    load = (lambda t: tuple(x[::-1].copy() for x in t)) if reverse_truth else (lambda t: t)
    tids = [engine.truth_load(*load(t)) for t in truths]
    b = engine.batch(SIZES, [tids[w] for w in WHICH], alleles=True)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b, cols, truths, tids


def release(engine, b, tids):
    b.close()
    for t in tids:
        engine.truth_release(t)


def fetch(b):
    rec, tru = b.atomize(columns=True)
    return rec, tru, [b.atomized(v) for v in range(b.n_vcf)]


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_records_against_the_restatement(engine, sorted_):
    b, cols, truths, tids = make_batch(engine, 21, sorted_)
    try:
        before = ([b.cls(v).copy() for v in range(b.n_vcf)], b.scalars().copy(), b.roc().copy())
        bytes0 = b.device_bytes
        rec, tru, per = fetch(b)
        assert b.device_bytes > bytes0            # the pass's buffers are the batch's, allocated by its first call
        scal = b.scalars()
        classes = np.zeros(9, np.int64)
        for v, (c, w) in enumerate(zip(cols, WHICH)):
            cls = b.cls(v)
            kept, tp = (cls & 1).astype(bool), (cls & 2).astype(bool)
            wrec, wtru, wcls, wna, whm = at.counts(truths[w], c[0], c[1], c[2], c[4], kept, tp)
            np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d" % v)
            np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d" % v)
            gcls, gna, ghm = per[v]
            np.testing.assert_array_equal(gcls, wcls)
            np.testing.assert_array_equal(gna, wna)
            np.testing.assert_array_equal(ghm, whm)
            nh = np.array([bin(int(x)).count("1") for x in ghm], np.int64)
            atomisable = gna > 0
            tp_a = np.where(atomisable, kept & (((nh == gna) & ((c[4] & 2) != 0)) | ((c[4] & 8) != 0)), tp)
            assert not (tp & ~tp_a).any()                        # an exact TP line is always a TP_A line
            assert int(rec[v][2]) == int(tp_a.sum()) and int(rec[v][3]) == int((tp_a & ~tp).sum())
            assert int(rec[v][0]) == int(kept.sum()) == int(scal[v][S_NPASS]) and int(rec[v][1]) == int(tp.sum()) == int(scal[v][S_TP_LINES])
            assert int(tru[v][4]) <= int(tru[v][5])
            if v != KEPT_NOKEY:
                assert int(tru[v][4]) == int(scal[v][S_TP_R])
            classes += np.bincount(gcls, minlength=9)
        big = len(SIZES) - 1
        assert int(rec[big][3]) > 100 and int(rec[big][5]) > 100  # rescued and partial lines: on the restatement as well (rec == wrec)
        assert int(rec[2][3]) > 0 and int(rec[2][5]) > 0
        assert (classes > 0).all(), classes                      # every class byte occurred
        assert (rec[big][[8, 10, 11, 12]] > 0).all() and int(rec[big][9]) == 0 and int(rec[KEPT_NOKEY][9]) > 0   # every reason among kept records
        assert int(rec[big][4]) > 0 and int(rec[big][7]) < int(rec[big][6])
        assert int(tru[big][3]) > 0 and int(tru[big][5]) > int(tru[big][4]) > 0
        assert not rec[0].any() and int(tru[0][0]) == int(tru[3][0]) == int(tru[5][0]) and not tru[0][3:].any()   # the empty VCF
        assert tru[1][0] == tru[2][0] == tru[4][0] and tru[1][2] == tru[4][2] and tru[0][2] == tru[5][2]
        # neutrality: the batch's masks, scalars and ROC are what they were
        for v in range(b.n_vcf):
            np.testing.assert_array_equal(b.cls(v), before[0][v])
        np.testing.assert_array_equal(b.scalars(), before[1])
        np.testing.assert_array_equal(b.roc(), before[2])
        b.set_timing(True)
        rec2, tru2 = b.atomize()
        np.testing.assert_array_equal(rec2, rec)
        np.testing.assert_array_equal(tru2, tru)
        ms = b.atomize_timings()
        assert set(ms) == {"atom_truth_ms", "atom_records_ms", "atom_found_ms"} and all(x >= 0 for x in ms.values())
        with pytest.raises(QmvtError) as ei:                     # that call kept no columns
            b.atomized(0)
        assert ei.value.code == QM_E_STATE and "QM_ATOM_COLUMNS" in str(ei.value)
    finally:
        release(engine, b, tids)


def test_an_empty_truth_set(engine):
    """tru stays zero and everything kept is FP"""
    rng = np.random.default_rng(4)
    tvs = truth_variants(rng, 50)
    none = (np.zeros(0, np.int32),) * 3
    tid = engine.truth_load(*none)
    cols = record_columns(rng, 300, tvs, True, False)
    cols = cols[:4] + ((cols[4] & ~np.uint8(8)).astype(np.uint8),)
    b = engine.batch([300], [tid], alleles=True)
    try:
        b.upload(0, *cols)
        b.run()
        b.finish()
        rec, tru = b.atomize(columns=True)
        assert engine.truth_atoms(tid).shape == (0,)
        cls = b.cls(0)
        wrec, wtru, wcls, wna, whm = at.counts(none, cols[0], cols[1], cols[2], cols[4], (cls & 1).astype(bool), (cls & 2).astype(bool))
        np.testing.assert_array_equal(rec[0], wrec)
        assert not tru.any() and not wtru.any() and int(rec[0][0]) > 0 and int(rec[0][1]) == int(rec[0][2]) == int(rec[0][7]) == 0
        gcls, gna, ghm = b.atomized(0)
        np.testing.assert_array_equal(gcls, wcls)
        np.testing.assert_array_equal(gna, wna)
        assert not ghm.any()
    finally:
        release(engine, b, [tid])


# ---- determinism ------------------------------------------------------------------------------------------------------------
def test_same_answer_twice_and_with_the_truth_loaded_backwards(engine):
    b, cols, truths, tids = make_batch(engine, 33, False)
    try:
        first = fetch(b)
        again = fetch(b)
    finally:
        release(engine, b, tids)
    b, _, _, tids = make_batch(engine, 33, False, reverse_truth=True)
    try:
        back = fetch(b)
    finally:
        release(engine, b, tids)
    for o in (again, back):
        np.testing.assert_array_equal(first[0], o[0])
        np.testing.assert_array_equal(first[1], o[1])
        for x, y in zip(first[2], o[2]):
            for p, q in zip(x, y):
                np.testing.assert_array_equal(p, q)
    assert int(first[0][:, 3].sum()) > 0


# ---- state and argument errors ------------------------------------------------------------------------------------------------
def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    rng = np.random.default_rng(9)
    tvs = truth_variants(rng, 50)
    truth = codes(tvs)
    tid = engine.truth_load(*truth)
    cols = [record_columns(rng, 40, tvs, True, False) for _ in range(2)]
    b = engine.batch([40, 40], [tid, tid], alleles=True)
    sb = engine.batch([40], [tid])                              # a single-base batch
    try:
        for v in range(2):
            b.upload(v, *cols[v])
        c, msg = refused(b.atomize)
        assert c == QM_E_STATE and "qm_batch_finish first" in msg          # before finish
        b.run()
        c, msg = refused(b.atomize)
        assert c == QM_E_STATE
        b.finish()
        bytes0 = b.device_bytes
        c, msg = refused(b.atomize_counts)                                  # getters before the pass
        assert c == QM_E_STATE and "no qm_batch_atomize behind the latest run" in msg
        c, msg = refused(lambda: b.atomized(0))
        assert c == QM_E_STATE and "no qm_batch_atomize behind the latest run" in msg
        c, msg = refused(b.atomize_timings)
        assert c == QM_E_STATE
        assert b._L.qm_batch_atomize(b._h, 4, None) == QM_E_INVAL
        snv = lambda x: np.where((x >= 0) & (x < 4), x, 0).astype(np.int32)
        sb.upload(0, cols[0][0].clip(0, 5000), snv(cols[0][1]), snv(cols[0][2]), cols[0][3], cols[0][4])
        sb.run()
        sb.finish()
        c, msg = refused(sb.atomize)                                        # a single-base batch
        assert c == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        assert b.device_bytes == bytes0                                   # a batch that never ran the pass holds none of its buffers
        rec, tru = b.atomize()                                              # it does run
        assert b.device_bytes > bytes0
        assert int(rec[0][0]) > 0 and int(tru[0][0]) == len(at.truth_order(*truth))
        assert b._L.qm_batch_get_atomized(b._h, 2, None, None, None) == QM_E_INVAL        # the batch has two VCFs
        b.run()                                                             # a new run forgets the pass
        b.finish()
        c, msg = refused(b.atomize_counts)
        assert c == QM_E_STATE
        c, msg = refused(lambda: b.atomized(0))
        assert c == QM_E_STATE
        rec3, tru3 = b.atomize(columns=True)                                # ... and the pass runs again behind it
        np.testing.assert_array_equal(rec3, rec)
        np.testing.assert_array_equal(tru3, tru)
        assert b.atomized(1)[0].shape == (40,)
        n_out = C.c_int64()
        assert engine._L.qm_truth_atoms(engine._h, 999, None, 0, C.byref(n_out)) == QM_E_INVAL
        engine.truth_release(tid)
        c, msg = refused(b.atomize)                                         # a released truth set
        assert c == QM_E_STATE and "truth set %d was released" % tid in msg
        tid = None
    finally:
        b.close()
        sb.close()
        if tid is not None:
            engine.truth_release(tid)
