"""TP, FP and FN by variant type and size on the device (qm_batch_types; k_type_records / k_type_truth) against
the restatement of quasimodo_amd.vartype, tied to the batch's masks and scalars, to the truth set's table and -- through the
found entries and the atom counts -- to the atomisation pass, an independent kernel.  The batch has the shape of
test_gpu_atomize's.  Every comparison is exact: these are integers."""
import numpy as np
import pytest

from quasimodo_amd import vartype as vt
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_NPASS, S_TP_LINES = 0, 1
BASES = "ACGT"
L = 6000
SIZES = [0, 1, 255, 256, 257, 70000]                # 256: the alignment of a VCF; 70 000: more than one span, more than one workgroup
WHICH = [1, 0, 0, 1, 0, 1]                          # the truth set of every VCF: each is shared by three
KEPT_NOKEY = 5                                      # the one VCF with kept records that have no key: the large one
# sizes on both sides of every default edge (5|6, 15|16, 50|51) and of the inline / long boundary (13|14 bases)
AROUND = [1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 14, 15, 16, 17, 49, 50, 51, 52, 60]
REPEATS = [("A", "AA"), ("AA", "A"), ("CAC", "C"), ("C", "CAC"), ("ATA", "ACA"), ("ACGT", "AT"), ("TCTC", "TC")]
EDGES16 = (1, 2, 3, 4, 5, 6, 7, 8, 10, 13, 14, 16, 21, 51, 52, 100)


def bases(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def other(rng, ch):
    return BASES[(BASES.index(ch) + int(rng.integers(1, 4))) % 4]


def variant(rng):
    """(pos, REF, ALT) as strings: every grid type, sizes from AROUND where the type allows them (an MNP of more than 13 bases
    would be two long alleles)"""
    u, p = rng.random(), int(rng.integers(1, L))
    s = AROUND[int(rng.integers(0, len(AROUND)))]
    if u < 0.30:
        r = bases(rng, 1)
        return p, r, other(rng, r)
    if u < 0.45:                                    # an MNP whose ends differ: the trimmed span is its length
        m = min(max(s, 2), 13)
        r = bases(rng, m)
        return p, r, other(rng, r[0]) + bases(rng, m - 2) + other(rng, r[-1])
    if u < 0.60:                                    # pure insertions and deletions behind a one-base anchor; long from 13 bases on
        b = bases(rng, 1)
        return p, b, b + bases(rng, s)
    if u < 0.75:
        b = bases(rng, 1)
        return p, b + bases(rng, s), b
    if u < 0.92:                                    # complex: first and last bases differ, the lengths too; at most one allele is long
        big = max(s, 2)
        small = int(rng.integers(1, min(big, 14)))
        x = bases(rng, big)
        y = other(rng, x[0]) + (bases(rng, small - 2) + other(rng, x[-1]) if small >= 2 else "")
        if small == 1 and y[0] == x[-1]:
            y = next(ch for ch in BASES if ch not in (x[0], x[-1]))
        return (p, x, y) if rng.random() < 0.5 else (p, y, x)
    r, a = REPEATS[int(rng.integers(0, len(REPEATS)))]
    return p, r, a


class Codes:
    """allele strings as codes: inline up to 13 bases, ids of the test's own dictionary beyond"""

    def __init__(self):
        self.ids = {}

    def __call__(self, s):
        return vt.code(s) if len(s) <= vt.INLINE_MAX else vt.DICT | self.ids.setdefault(s, len(self.ids))

    def shapes(self):
        return vt.shapes_of(sorted(self.ids, key=self.ids.get))


def truth_variants(rng, n):
    vs = [variant(rng) for _ in range(n - 4)]
    vs.append((int(rng.integers(1, L)), bases(rng, 14), bases(rng, 20)))            # LONGPAIR
    vs.append((int(rng.integers(1, L)), bases(rng, 30), bases(rng, 30)))
    vs += [(int(rng.integers(1, L)), "A", "AA"), (int(rng.integers(1, L)), "CAC", "C")]
    return vs


def record_variants(rng, n, tvs):
    """(pos, REF, ALT, what) per record: truth entries as they are spelled, unrelated variants, NOVAR, LONGPAIR, and `past`:
    the ALT is to become an id the shape table does not hold"""
    out = []
    for _ in range(n):
        u = rng.random()
        if u < 0.45:
            out.append(tvs[int(rng.integers(0, len(tvs)))] + ("",))
        elif u < 0.90:
            out.append(variant(rng) + ("",))
        elif u < 0.94:
            v = variant(rng)
            out.append((v[0], v[1], v[1], ""))                                      # NOVAR, long ones among them
        elif u < 0.97:
            out.append((int(rng.integers(1, L)), bases(rng, 15), bases(rng, 14), ""))
        else:
            out.append(variant(rng)[:2] + ("", "past"))
    return out


def columns(rng, recs, code, sorted_, kept_nokey):
    n = len(recs)
    pos = np.array([r[0] for r in recs], np.int32).reshape(n)
    ref = np.array([code(r[1]) for r in recs], np.int32).reshape(n)
    alt = np.array([0 if r[3] else code(r[2]) for r in recs], np.int32).reshape(n)
    qual = rng.integers(0, 300, n).astype(np.float32)
    bad = rng.random(n) < 0.02                      # codes that are no alleles
    ref[bad] = rng.choice([-1, 5, 0x07ffffff], int(bad.sum()))
    nokey = rng.random(n) < 0.04
    passed = ~bad & (qual >= 20)
    if not kept_nokey:
        qual[nokey] = 5
        passed &= ~nokey
    iddot = rng.random(n) > 0.1
    tpline = rng.random(n) < 0.02
    flags = (passed.astype(np.uint8) | (iddot.astype(np.uint8) << 1) | (nokey.astype(np.uint8) << 2) | (tpline.astype(np.uint8) << 3)).astype(np.uint8)
    order = np.argsort(pos, kind="stable") if sorted_ else np.arange(n)
    return [pos[order], ref[order], alt[order], qual[order], flags[order]], [recs[i] for i in order]


def make_batch(engine, seed, sorted_, truth_sizes=(500, 1200)):
    rng = np.random.default_rng(seed)
    code = Codes()
    tvs = [truth_variants(rng, n) if n else [] for n in truth_sizes]
    recs = [record_variants(rng, n, tvs[w] or [variant(rng)]) for n, w in zip(SIZES, WHICH)]
    truths = [tuple(np.array(x, np.int32).reshape(len(v)) for x in ([t[0] for t in v], [code(t[1]) for t in v], [code(t[2]) for t in v])) for v in tvs]
    made = [columns(rng, r, code, sorted_, v == KEPT_NOKEY) for v, r in enumerate(recs)]
    cols, recs = [m[0] for m in made], [m[1] for m in made]
    shapes = code.shapes()
    past = vt.DICT | (len(shapes[0]) + 3)           # an id past the table: NOSHAPE
    for c, r in zip(cols, recs):
        c[2][np.array([bool(x[3]) for x in r], bool).reshape(len(r))] = past
    for k in range(len(truths)):
        if len(truths[k][0]):
            truths[k][1][0], truths[k][2][0] = vt.code("A"), past      # ... among the truth entries as well
    tids = [engine.truth_load(*t) for t in truths]
    b = engine.batch(SIZES, [tids[w] for w in WHICH], alleles=True)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b, cols, recs, truths, tids, shapes


def release(engine, b, tids):
    b.close()
    for t in tids:
        engine.truth_release(t)


def masks(b, v):
    cls = b.cls(v)
    return (cls & 1).astype(bool), (cls & 2).astype(bool)


def restated(b, cols, truths, edges, shapes):
    return [vt.counts(truths[w], c[0], c[1], c[2], c[4], *masks(b, v), edges, shapes) for v, (c, w) in enumerate(zip(cols, WHICH))]


@pytest.mark.parametrize("sorted_", [True, False], ids=["sorted", "shuffled"])
def test_counts_and_rows_against_the_restatement(engine, sorted_):
    b, cols, recs, truths, tids, shapes = make_batch(engine, 21, sorted_)
    try:
        before = ([b.cls(v).copy() for v in range(b.n_vcf)], b.scalars().copy(), b.roc().copy())
        bytes0 = b.device_bytes
        e = vt.DEFAULT_EDGES
        nb, nr = len(e), vt.n_rows(e)
        rec, tru = b.vartype(shapes=shapes, columns=True)
        assert b.device_bytes > bytes0                                 # the pass's buffers are the batch's, allocated by its first call
        assert rec.shape == tru.shape == (len(SIZES), nr, 2) and rec.dtype == np.uint64
        rows = [b.vartyped(v) for v in range(b.n_vcf)]
        want = restated(b, cols, truths, e, shapes)
        scal = b.scalars()
        at_rec, at_tru = b.atomize(columns=True)                       # the independent kernel, on the same finished batch
        for v, (c, w) in enumerate(zip(cols, WHICH)):
            wrec, wtru, wrow = want[v]
            np.testing.assert_array_equal(rec[v], wrec, err_msg="rec of VCF %d" % v)
            np.testing.assert_array_equal(tru[v], wtru, err_msg="tru of VCF %d" % v)
            np.testing.assert_array_equal(rows[v], wrow, err_msg="rows of VCF %d" % v)
            kept, tp = masks(b, v)
            assert int(rec[v][:, 0].sum()) == int(kept.sum()) == int(scal[v][S_NPASS])
            assert int(rec[v][:, 1].sum()) == int((kept & tp).sum()) == int(scal[v][S_TP_LINES])
            assert (rec[v][:, 1] <= rec[v][:, 0]).all() and (tru[v][:, 1] <= tru[v][:, 0]).all()
            assert int(tru[v][:, 0].sum()) == len(engine.truth_entries(tids[w])[0])
            assert int(tru[v][:, 1].sum()) == int(at_tru[v][4])        # QM_ATOM_T_FOUND
            assert not tru[v][5 * nb + vt.NOKEY].any()                 # truth entries never land in NOKEY
            # SNV iff one atom, MNP iff two or more, for the records the atomisation pass calls atomisable
            gcls, gna, _ = b.atomized(v)
            kind = np.where(rows[v] < 5 * nb, rows[v] // nb, 255)
            atomisable = gna > 0
            np.testing.assert_array_equal(kind[atomisable] == vt.SNV, gna[atomisable] == 1)
            np.testing.assert_array_equal(kind[atomisable] == vt.MNP, gna[atomisable] >= 2)
            assert not np.isin(kind[~atomisable & ((c[4] & 4) == 0)], (vt.SNV, vt.MNP)).any()
            # a pure insertion or deletion has the size | |R| - |A| |
            for i in np.flatnonzero(kept & np.isin(kind, (vt.INS, vt.DEL))):
                r = recs[v][i]
                assert rows[v][i] == vt.row_of(int(kind[i]), abs(len(r[1]) - len(r[2])), e), r
        big = len(SIZES) - 1
        per_type = rec[big][:5 * nb, 0].reshape(5, nb)
        assert (per_type.sum(axis=1) > 0).all() and (rec[big][5 * nb:, 0] > 0).all(), rec[big][:, 0]     # every row class among kept records
        assert (per_type[[vt.INS, vt.DEL], :] > 0).all()               # on both sides of every default edge and of 13|14 bases
        assert (per_type[vt.CPX, 1:] > 0).all() and per_type[vt.CPX, 0] == 0          # (a complex record has a size of at least 2)
        assert (per_type[vt.MNP, 1:6] > 0).all() and not per_type[vt.MNP, [0, 6, 7]].any()   # 2 .. 13 bases: longer ones are LONGPAIR
        assert per_type[vt.SNV, 0] > 0 and not per_type[vt.SNV, 1:].any()
        assert int(rec[big][:, 1].sum()) > 1000 and int(tru[big][:, 1].sum()) > 500
        assert int(tru[big][5 * nb + vt.LONGPAIR, 0]) == 2 and int(tru[big][5 * nb + vt.NOSHAPE, 0]) == 1
        assert not rec[0].any() and not tru[0][:, 1].any() and int(tru[0][:, 0].sum()) > 0               # the empty VCF
        np.testing.assert_array_equal(tru[0][:, 0], tru[3][:, 0])      # one truth set, typed alike
        assert all(int(rec[v][5 * nb + vt.NOKEY, 0]) == 0 for v in range(len(SIZES)) if v != KEPT_NOKEY)
        # neutrality: the batch's masks, scalars and ROC are what they were
        for v in range(b.n_vcf):
            np.testing.assert_array_equal(b.cls(v), before[0][v])
        np.testing.assert_array_equal(b.scalars(), before[1])
        np.testing.assert_array_equal(b.roc(), before[2])
        # a second call gives the same answer; it keeps no row bytes
        b.set_timing(True)
        rec2, tru2 = b.vartype(shapes=shapes)
        np.testing.assert_array_equal(rec2, rec)
        np.testing.assert_array_equal(tru2, tru)
        ms = b.vartype_timings()
        assert set(ms) == {"type_records_ms", "type_truth_ms"} and all(x >= 0 for x in ms.values())
        with pytest.raises(QmvtError) as ei:
            b.vartyped(0)
        assert ei.value.code == QM_E_STATE and "QM_TYPE_COLUMNS" in str(ei.value)
    finally:
        release(engine, b, tids)


def test_one_bin_sixteen_bins_and_no_table(engine):
    b, cols, recs, truths, tids, shapes = make_batch(engine, 33, False)
    try:
        for edges, sh in (((1,), shapes), (EDGES16, shapes), (vt.DEFAULT_EDGES, None)):
            rec, tru = b.vartype(edges, sh, columns=True)
            nb = len(edges)
            assert rec.shape == (len(SIZES), 5 * nb + 4, 2)
            for v, (wrec, wtru, wrow) in enumerate(restated(b, cols, truths, edges, sh)):
                np.testing.assert_array_equal(rec[v], wrec, err_msg="%d bins, rec of VCF %d" % (nb, v))
                np.testing.assert_array_equal(tru[v], wtru, err_msg="%d bins, tru of VCF %d" % (nb, v))
                np.testing.assert_array_equal(b.vartyped(v), wrow, err_msg="%d bins, rows of VCF %d" % (nb, v))
            if sh is None:                                             # without a table every long record lands in NOSHAPE (or LONGPAIR)
                for v, c in enumerate(cols):
                    row = b.vartyped(v)
                    long_ = ((c[1] >= vt.DICT) | (c[2] >= vt.DICT)) & (c[1] != c[2]) & ((c[4] & 4) == 0) & (c[1] >= 0) & ((c[1] < 4) | (c[1] >= 0x08000000))
                    both = (c[1] >= vt.DICT) & (c[2] >= vt.DICT)
                    assert (row[long_ & ~both] == 5 * nb + vt.NOSHAPE).all() and (row[long_ & both] == 5 * nb + vt.LONGPAIR).all()
                    assert (row[~long_] != 5 * nb + vt.NOSHAPE).all()
                assert int(rec[-1][5 * nb + vt.NOSHAPE, 0]) > 1000
            elif nb == 16:
                assert np.count_nonzero(rec[-1][:, 0]) > 40            # the long alleles spread over the upper bins
    finally:
        release(engine, b, tids)


def test_an_empty_truth_set(engine):
    """tru stays zero and everything kept is FP"""
    rng = np.random.default_rng(4)
    code = Codes()
    recs = [r for r in record_variants(rng, 400, [variant(rng) for _ in range(50)]) if not r[3]][:300]
    cols, recs = columns(rng, recs, code, True, False)
    cols[4] = (cols[4] & ~np.uint8(8)).astype(np.uint8)                # no TP line by the text side either
    none = (np.zeros(0, np.int32),) * 3
    tid = engine.truth_load(*none)
    b = engine.batch([300], [tid], alleles=True)
    try:
        b.upload(0, *cols)
        b.run()
        b.finish()
        rec, tru = b.vartype(shapes=code.shapes(), columns=True)
        wrec, wtru, wrow = vt.counts(none, cols[0], cols[1], cols[2], cols[4], *masks(b, 0), None, code.shapes())
        np.testing.assert_array_equal(rec[0], wrec)
        np.testing.assert_array_equal(b.vartyped(0), wrow)
        assert not tru.any() and not wtru.any() and int(rec[0][:, 0].sum()) > 100 and not rec[0][:, 1].any()
    finally:
        release(engine, b, [tid])


def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code, str(ei.value)


def test_state_rules(engine):
    rng = np.random.default_rng(9)
    code = Codes()
    tvs = truth_variants(rng, 50)
    truth = tuple(np.array(x, np.int32) for x in ([t[0] for t in tvs], [code(t[1]) for t in tvs], [code(t[2]) for t in tvs]))
    made = [columns(rng, record_variants(rng, 40, tvs), code, True, False) for _ in range(2)]
    cols = [m[0] for m in made]
    shapes = code.shapes()
    tid = engine.truth_load(*truth)
    b = engine.batch([40, 40], [tid, tid], alleles=True)
    sb = engine.batch([40], [tid])                                      # a single-base batch
    try:
        for v in range(2):
            b.upload(v, *cols[v])
        c, msg = refused(lambda: b.vartype(shapes=shapes))
        assert c == QM_E_STATE and "qm_batch_finish first" in msg       # before finish
        b.run()
        c, msg = refused(lambda: b.vartype(shapes=shapes))
        assert c == QM_E_STATE
        b.finish()
        bytes0 = b.device_bytes
        c, msg = refused(b.vartype_counts)                              # getters before the pass
        assert c == QM_E_STATE and "no qm_batch_types behind the latest run" in msg
        c, msg = refused(lambda: b.vartyped(0))
        assert c == QM_E_STATE and "no qm_batch_types behind the latest run" in msg
        c, msg = refused(b.vartype_timings)
        assert c == QM_E_STATE
        e8 = np.array(vt.DEFAULT_EDGES, np.int32)
        p = lambda x: x.ctypes.data
        call = lambda edges, nb, what=0, sh=shapes: b._L.qm_batch_types(b._h, p(edges), nb, p(sh[0]), p(sh[1]), p(sh[2]), len(sh[0]), what, None)
        assert call(e8, 8, 4) == QM_E_INVAL                             # what
        assert call(e8, 0) == QM_E_INVAL and call(np.arange(1, 18, dtype=np.int32), 17) == QM_E_INVAL      # n_bins outside 1 .. 16
        assert call(np.array([2, 3], np.int32), 2) == QM_E_INVAL       # edges[0] != 1
        assert call(np.array([1, 3, 3], np.int32), 3) == QM_E_INVAL and call(np.array([1, 5, 4], np.int32), 3) == QM_E_INVAL   # not ascending
        short = (np.array([14, 13], np.int32), np.zeros(2, np.uint32), np.zeros(2, np.uint32))
        assert call(e8, 8, 0, short) == QM_E_INVAL and "len 13" in engine._L.qm_last_error(engine._h).decode()
        snv = lambda x: np.where((x >= 0) & (x < 4), x, 0).astype(np.int32)
        sb.upload(0, cols[0][0].clip(0, 5000), snv(cols[0][1]), snv(cols[0][2]), cols[0][3], cols[0][4])
        sb.run()
        sb.finish()
        c, msg = refused(sb.vartype)                                    # a single-base batch
        assert c == QM_E_STATE and "single-base batch" in msg and "QM_BATCH_ALLELES" in msg
        assert b.device_bytes == bytes0                                 # a batch that never ran the pass holds none of its buffers
        rec, tru = b.vartype(shapes=shapes)                             # it does run
        assert b.device_bytes > bytes0
        assert int(rec[0][:, 0].sum()) > 0 and int(tru[0][:, 0].sum()) == len(vt.truth_order(*truth))
        c, msg = refused(lambda: b.vartyped(0))                         # that call kept no row bytes
        assert c == QM_E_STATE and "QM_TYPE_COLUMNS" in msg
        assert b._L.qm_batch_get_typed(b._h, 2, None) == QM_E_INVAL     # the batch has two VCFs
        b.run()                                                         # a new run forgets the pass
        b.finish()
        c, msg = refused(b.vartype_counts)
        assert c == QM_E_STATE
        rec3, tru3 = b.vartype(shapes=shapes, columns=True)             # ... and the pass runs again behind it
        np.testing.assert_array_equal(rec3, rec)
        np.testing.assert_array_equal(tru3, tru)
        assert b.vartyped(1).shape == (40,)
        engine.truth_release(tid)
        c, msg = refused(lambda: b.vartype(shapes=shapes))              # a released truth set
        assert c == QM_E_STATE and "truth set %d was released" % tid in msg
        tid = None
    finally:
        b.close()
        sb.close()
        if tid is not None:
            engine.truth_release(tid)
