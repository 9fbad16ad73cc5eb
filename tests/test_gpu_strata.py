"""Counts per genome region (qm_strata_load, qm_batch_strata, k_strata_records / k_strata_planes / k_strata_truth; DESIGN.md
4.10) against a numpy restatement tied to the batch's columns, class masks and hit bitmaps, and against a hand-written case.
Every comparison is exact: these are integers."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_columns, random_truth
from quasimodo_amd import _lib
from quasimodo_amd import strata as st
from quasimodo_amd._lib import QmvtError
from test_strata_host import random_strata

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE, QM_E_RANGE = -1, -6, -5
F_PASS, F_IDDOT, F_NOKEY = 1, 2, 4
I32MAX = (1 << 31) - 1
S_NPASS, S_TP_LINES, S_FP_LINES, S_TP_R, S_TRUTH = 0, 1, 2, 3, 7


def code(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code


def truth_keys(truth):
    """the sorted distinct single-base keys of a truth set: pos << 4 | ref << 2 | alt"""
    p, r, a = (np.asarray(x, np.int64) for x in truth)
    ok = (r >= 0) & (r < 4) & (a >= 0) & (a < 4)
    return np.unique((p[ok] << 4) | (r[ok] << 2) | a[ok])


def restate_rec(table, S, cols, cls):
    """[S + 2][3] of one VCF from its columns and class bytes (bit 0 kept, bit 1 TP)"""
    pos, flags = cols[0], cols[4]
    kept, tp = (cls & 1) != 0, (cls & 2) != 0
    nokey = (flags & F_NOKEY) != 0
    m = st.mask_of(table, pos)
    out = np.zeros((S + 2, 3), np.uint64)
    rows = [kept & ~nokey & (((m >> np.uint32(s)) & 1) != 0) for s in range(S)] + [kept & ~nokey & (m == 0), kept & nokey]
    for k, sel in enumerate(rows):
        out[k] = [sel.sum(), (sel & tp).sum(), (sel & ~tp).sum()]
    return out


def restate_tru(table, S, keys, hits):
    """[S + 1][2] of one VCF from its truth set's keys and its hit bits"""
    m = st.mask_of(table, (keys >> 4).astype(np.int32))
    out = np.zeros((S + 1, 2), np.uint64)
    for s in range(S + 1):
        sel = ((m >> np.uint32(s)) & 1) != 0 if s < S else m == 0
        out[s] = [sel.sum(), (sel & hits).sum()]
    return out


def make_batch(engine, cols, tids, alleles=False):
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b


def strata_from_segments(bounds, masks, S):
    """a strata set whose flattened table is INT32_MIN, bounds... with the given masks: one interval per segment and set bit (the
    touching intervals of a stratum are its union); the last segment runs to 2^31 - 1"""
    iv = [([], []) for _ in range(S)]
    for i, (b, m) in enumerate(zip(bounds, masks)):
        end = bounds[i + 1] - 1 if i + 1 < len(bounds) else I32MAX
        for s in range(S):
            if (m >> s) & 1:
                iv[s][0].append(b - 1)
                iv[s][1].append(end)
    return [("s%d" % s, np.array(iv[s][0], np.int64), np.array(iv[s][1], np.int64)) for s in range(S)]


def overlapping_set(n_seg):
    """S = 32, n_seg segments in all (INT32_MIN included): neighbours differ, every stratum appears, the last segment is empty"""
    bounds = [1 + 5 * i for i in range(n_seg - 1)]
    masks = [((i * 2654435761) & 0xffffffff) | (1 << (i % 32)) for i in range(1, n_seg - 1)] + [0]
    for i in range(1, len(masks) - 1):
        if masks[i] == masks[i - 1]:
            masks[i] ^= 1 << ((i + 7) % 32)
    assert all(a != b for a, b in zip(masks, masks[1:])) and masks[0] != 0
    return strata_from_segments(bounds, masks, 32)


def partition_set(n_seg, S=5):
    """S strata that partition the positions >= 1 into n_seg - 1 segments (the global table when n_seg > 4096)"""
    bounds = [1 + 4 * i for i in range(n_seg - 1)]
    return strata_from_segments(bounds, [1 << (i % S) for i in range(n_seg - 1)], S)


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,n_strata", [(1, 1), (2, 3), (3, 8), (4, 32)])
def test_segments_equal_flatten(engine, seed, n_strata):
    strata = random_strata(np.random.default_rng(seed), n_strata)
    sid = engine.strata_load(strata)
    try:
        b, m = engine.strata_segments(sid)
        wb, wm = st.flatten(strata)
        assert engine.strata_info(sid) == (n_strata, wb.shape[0])
        np.testing.assert_array_equal(b, wb)
        np.testing.assert_array_equal(m, wm)
    finally:
        engine.strata_release(sid)


def test_load_refuses(engine):
    L, h = engine._L, engine._h
    sid = C.c_int(-1)
    def load(n, offs, s, e):
        offs, s, e = np.array(offs, np.int64), np.array(s, np.int32), np.array(e, np.int32)
        return L.qm_strata_load(h, n, offs.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), C.byref(sid))
    assert load(0, [0], [0], [1]) == QM_E_INVAL                               # an empty strata set
    assert load(33, list(range(34)), list(range(33)), list(range(1, 34))) == QM_E_INVAL
    assert load(1, [0, 1], [-1], [5]) == QM_E_INVAL
    assert load(1, [0, 1], [5], [5]) == QM_E_INVAL
    assert load(1, [0, 1], [6], [5]) == QM_E_INVAL
    with pytest.raises(ValueError):
        engine.strata_load([("a", [0], [I32MAX + 1])])
    with pytest.raises(ValueError):
        engine.strata_load([])
    sid2 = engine.strata_load([("a", [0], [I32MAX])])                          # the largest end there is
    assert engine.strata_segments(sid2)[0].tolist() == [-(1 << 31), 1]
    engine.strata_release(sid2)
    assert code(lambda: engine.strata_release(sid2)) == QM_E_INVAL
    assert code(lambda: engine.strata_info(sid2)) == QM_E_INVAL


# ---- hand cases -----------------------------------------------------------------------------------------------------------
A_, C_, G_, T_ = 0, 1, 2, 3
K = F_PASS | F_IDDOT
HAND_STRATA = [("A", [10], [20]), ("B", [15], [30]), ("C", [100, 200], [200, 250])]   # A 11..20, B 16..30, C 101..250
HAND_TRUTH = [(11, A_, C_), (18, A_, G_), (30, C_, T_), (31, C_, A_), (150, T_, A_), (400, G_, C_)]
HAND = [                                     # pos, ref, alt, flags
    (0, A_, C_, K),                          # pos 0: mask 0, outside
    (10, A_, C_, K),                         # pos = start of A: not in it (BED is 0-based, half-open)
    (11, A_, C_, K),                         # start + 1: in A; a TP line, hits key 0
    (18, A_, G_, F_PASS),                    # a non-'.' ID on a truth key: an FP line in A and B that still sets hit bit 1
    (20, T_, C_, K),                         # pos = end of A: in A (and B)
    (21, T_, C_, K),                         # end + 1: B only
    (25, G_, A_, F_IDDOT),                   # fails the filter inside B: counted nowhere
    (30, C_, T_, K),                         # the last position of B; a TP line, hits key 2
    (31, C_, A_, K),                         # a TP line outside every stratum, hits key 3
    (150, G_, C_, K | F_NOKEY),              # kept, no comparable key: the nokey row only, although pos lies in C
    (250, A_, T_, K),                        # the end of the second, touching interval of C
    (251, A_, T_, K),                        # one beyond
]
HAND_REC = [[3, 1, 2], [4, 1, 3], [1, 0, 1], [4, 1, 3], [1, 0, 1]]          # A, B, C, outside, nokey: kept, TP, FP lines
HAND_TRU = [[2, 2], [2, 2], [1, 0], [2, 1]]                                 # A, B, C, outside: truth keys, hit ones


def test_hand_cases(engine):
    assert len(HAND) == 12
    tid = engine.truth_load(*(np.array([t[k] for t in HAND_TRUTH], np.int32) for k in range(3)))
    sid = engine.strata_load(HAND_STRATA)
    cols = tuple(np.array([h[k] for h in HAND], np.int32) for k in range(3)) + (np.full(len(HAND), 50, np.float32),
                                                                                np.array([h[3] for h in HAND], np.uint8))
    b = make_batch(engine, [cols], [tid])
    b.truth_hits()
    b.strata(sid, truth=True)
    rec, tru = b.strata_counts()
    assert rec.shape == (1, 5, 3) and tru.shape == (1, 4, 2)
    assert rec[0].tolist() == HAND_REC
    assert tru[0].tolist() == HAND_TRU
    assert b.truth_hit_bits(0).tolist() == [True, True, True, True, False, False]
    b.close()
    engine.strata_release(sid)


def test_negative_position_never_reaches_the_pass(engine):
    """mask(p) is defined for every int32 p, but a batch that holds a position outside [0, 2^28) does not finish (QM_E_RANGE), so
    the pass never meets one: negative positions are pinned at the table (test_strata_host) and here at the lookup of the library's
    own table."""
    tid = engine.truth_load(np.array([5], np.int32), np.array([0], np.int32), np.array([1], np.int32))
    b = engine.batch([2], [tid])
    b.upload(0, np.array([-7, 3], np.int32), np.zeros(2, np.int32), np.ones(2, np.int32), np.full(2, 50, np.float32), np.full(2, K, np.uint8))
    def run_and_finish():
        b.run()
        b.finish()
    assert code(run_and_finish) == QM_E_RANGE
    b.close()
    sid = engine.strata_load(HAND_STRATA)
    table = engine.strata_segments(sid)
    assert st.mask_of(table, np.array([-(1 << 31), -7, 0], np.int32)).tolist() == [0, 0, 0]
    engine.strata_release(sid)


# ---- shapes ---------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 3, 255, 256, 257, 1025, 3000, 16385, 70000]
GENOME = 20000


@pytest.fixture(scope="module")
def shape_sets(engine):
    """(name, strata, id, table, partitions) of the three sets, loaded once"""
    sets = [("all", [("all", [0], [I32MAX])], True), ("lds4096", overlapping_set(4096), False), ("global", partition_set(5001), True)]
    out = []
    for name, strata, part in sets:
        sid = engine.strata_load(strata)
        out.append((name, strata, sid, st.flatten(strata), part))
    assert out[0][3][0].shape[0] == 2
    assert engine.strata_info(out[1][2]) == (32, 4096) and out[1][3][0].shape[0] == 4096      # the largest table LDS takes
    assert engine.strata_info(out[2][2])[1] == 5001 > _lib.QM_STRATA_LDS_SEGMENTS                # the global table
    yield out
    for o in out:
        engine.strata_release(o[2])


@pytest.fixture(scope="module", params=[True, False], ids=["sorted", "shuffled"])
def shape_batch(engine, request):
    rng = np.random.default_rng(11 if request.param else 12)
    truths = [random_truth(rng, 700, GENOME), random_truth(rng, 40, GENOME)]
    tids = [engine.truth_load(*t) for t in truths]
    which = [v % 2 for v in range(len(SIZES))]
    cols = [random_columns(rng, n, GENOME, truths[w], sorted_=request.param) for n, w in zip(SIZES, which)]
    b = make_batch(engine, cols, [tids[w] for w in which])
    b.truth_hits()
    ref = {"cols": [b.columns(v) for v in range(len(SIZES))], "cls": [b.cls(v) for v in range(len(SIZES))],
           "hits": [b.truth_hit_bits(v) for v in range(len(SIZES))], "keys": [truth_keys(truths[w]) for w in which], "scal": b.scalars()}
    yield b, ref
    b.close()


@pytest.mark.parametrize("k", [0, 1, 2], ids=["all", "lds4096", "global"])
def test_shapes(engine, shape_batch, shape_sets, k):
    b, ref = shape_batch
    name, strata, sid, table, part = shape_sets[k]
    S = len(strata)
    b.strata(sid, truth=True)
    rec, tru = b.strata_counts()
    assert rec.shape == (len(SIZES), S + 2, 3) and tru.shape == (len(SIZES), S + 1, 2)
    for v in range(len(SIZES)):
        np.testing.assert_array_equal(rec[v], restate_rec(table, S, ref["cols"][v], ref["cls"][v]), err_msg="%s VCF %d rec" % (name, v))
        np.testing.assert_array_equal(tru[v], restate_tru(table, S, ref["keys"][v], ref["hits"][v]), err_msg="%s VCF %d tru" % (name, v))
        assert (rec[v, :, 0] == rec[v, :, 1] + rec[v, :, 2]).all()
        if part:
            sc = ref["scal"][v]
            assert rec[v].sum(axis=0).tolist() == [sc[S_NPASS], sc[S_TP_LINES], sc[S_FP_LINES]]
            assert tru[v].sum(axis=0).tolist() == [sc[S_TRUTH], int(ref["hits"][v].sum())]
            assert int(ref["hits"][v].sum()) == sc[S_TP_R]
    assert rec[:, S + 1, 0].sum() > 0 and rec[:, :S, 1].sum() > 0 and tru[:, :S, 1].sum() > 0      # the case is not empty


# ---- allele-extended batches ----------------------------------------------------------------------------------------------
def test_allele_extended_records_only(engine):
    from test_gpu_alleles import ext_columns, ext_truth
    rng = np.random.default_rng(5)
    truth = ext_truth(rng, 300, GENOME)
    tid = engine.truth_load(*truth)
    cols = [ext_columns(rng, n, GENOME, truth) for n in (257, 3000)]
    b = make_batch(engine, cols, [tid, tid], alleles=True)
    strata = partition_set(700)
    sid = engine.strata_load(strata)
    table = st.flatten(strata)
    assert code(lambda: b.strata(sid, truth=True)) == QM_E_STATE
    b.strata(sid)
    rec, tru = b.strata_counts()
    assert tru is None
    sc = b.scalars()
    indels = 0
    for v in range(2):
        c, cls = b.columns(v), b.cls(v)
        np.testing.assert_array_equal(rec[v], restate_rec(table, 5, c, cls))
        indels += int((((cls & 1) != 0) & ((c[1] >= 4) | (c[2] >= 4))).sum())
        assert rec[v].sum(axis=0).tolist() == [sc[v, S_NPASS], sc[v, S_TP_LINES], sc[v, S_FP_LINES]]   # the set partitions the positions
    assert indels > 0, "kept indels are counted, by their POS"
    b.close()
    engine.strata_release(sid)


# ---- state rules ----------------------------------------------------------------------------------------------------------
def test_state_rules(engine):
    rng = np.random.default_rng(9)
    truth = random_truth(rng, 100, 3000)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, 3000, truth) for n in (500, 1300)]
    s1 = [("lo", [0], [1500]), ("hi", [1500], [I32MAX])]
    s2 = [("x", [100], [900])]
    sid1, sid2 = engine.strata_load(s1), engine.strata_load(s2)
    b = engine.batch([len(c[0]) for c in cols], [tid, tid])
    for v, c in enumerate(cols):
        b.upload(v, *c)
    assert code(lambda: b.strata(sid1)) == QM_E_STATE                          # nothing ran
    assert code(b.strata_counts) == QM_E_STATE
    b.run()
    assert code(lambda: b.strata(sid1)) == QM_E_STATE                          # before finish
    b.finish()
    db0 = b.device_bytes
    assert code(lambda: b.strata(sid1, truth=True)) == QM_E_STATE              # TRUTH without truth hits
    assert code(lambda: b.strata(99)) == QM_E_INVAL
    assert b.device_bytes == db0                                               # nothing allocated until the first pass
    b.strata(sid1)
    nv, S = 2, 2
    db1 = b.device_bytes
    assert db1 == db0 + nv * (S + 2) * 2 * 8
    rec, tru = b.strata_counts()
    assert tru is None
    b._strata = (S, True)                                                      # ask for the half that was not made
    assert code(b.strata_counts) == QM_E_STATE
    t1, t2 = st.flatten(s1), st.flatten(s2)
    cls = [b.cls(v) for v in range(2)]
    for v in range(2):
        np.testing.assert_array_equal(rec[v], restate_rec(t1, 2, cols[v], cls[v]))
    b.truth_hits()
    db2 = b.device_bytes
    b.strata(sid1, truth=True)
    words = (len(truth_keys(truth)) + 31) // 32
    assert b.device_bytes == db2 + (S + 1) * words * 4 + nv * 24 + nv * (S + 1) * 2 * 8
    rec, tru = b.strata_counts()
    keys = truth_keys(truth)
    for v in range(2):
        np.testing.assert_array_equal(tru[v], restate_tru(t1, 2, keys, b.truth_hit_bits(v)))
    # another strata set: that set's counts
    b.strata(sid2, truth=True)
    rec, tru = b.strata_counts()
    assert rec.shape == (2, 3, 3) and tru.shape == (2, 2, 2)
    for v in range(2):
        np.testing.assert_array_equal(rec[v], restate_rec(t2, 1, cols[v], cls[v]))
        np.testing.assert_array_equal(tru[v], restate_tru(t2, 1, keys, b.truth_hit_bits(v)))
    # a released id
    engine.strata_release(sid2)
    assert code(lambda: b.strata(sid2)) == QM_E_INVAL
    # after a re-run the counts are gone until the pass is repeated
    b.run()
    assert code(b.strata_counts) == QM_E_STATE
    b.finish()
    assert code(b.strata_counts) == QM_E_STATE
    assert code(lambda: b.strata(sid1, truth=True)) == QM_E_STATE              # the truth hits are gone too
    b.strata(sid1)
    np.testing.assert_array_equal(b.strata_counts()[0][0], restate_rec(t1, 2, cols[0], cls[0]))
    b.close()
    engine.strata_release(sid1)


# ---- files in, files out ------------------------------------------------------------------------------------------------
BED = "# two strata that partition the positions >= 1\ntrack name=halves\nx\t0\t60000\tlo\nx 100000 2147483647 hi\r\nx\t50000\t100000\tlo\n"


def _bed(tmp_path):
    p = tmp_path / "halves.bed"
    p.write_text(BED)
    strata = st.read_bed_by_name(str(p))
    assert [s[0] for s in strata] == ["lo", "hi"]
    return strata


def _data_rows(path):
    if not path:
        return []
    with open(path, "rb") as fh:
        return [ln.split(b"\t") for ln in fh.read().split(b"\n") if ln and ln[:1] != b"#"]


def _row_of(pos):
    """the golden families hold no line without a comparable key: a kept line sits in lo, hi or (pos < 1) outside"""
    return 0 if 1 <= pos <= 100000 else 1 if pos > 100000 else 2


def text_counts(filtered, tp, fp, truth_keys_text, kept_keys_text):
    """(rec [4][3], tru [3][2]) from the TEXT of the written files and the truth file"""
    rec = np.zeros((4, 3), np.uint64)
    for col, path in enumerate((filtered, tp, fp)):
        for f in _data_rows(path):
            rec[_row_of(int(f[1])), col] += 1
    tru = np.zeros((3, 2), np.uint64)
    for k in truth_keys_text:
        r = _row_of(int(k[0]))
        tru[r, 0] += 1
        tru[r, 1] += k in kept_keys_text
    return rec, tru


def test_extract_many_strata_matches_the_written_files(engine, tmp_path):
    import os
    from quasimodo_amd import truthside as ts
    from quasimodo_amd.extract import extract_many, is_pure_strain
    from test_gpu_afprofile import _golden_jobs
    strata = _bed(tmp_path)
    plain = _golden_jobs(str(tmp_path / "a"))
    extract_many(plain, engine=engine)
    jobs = _golden_jobs(str(tmp_path / "b"))
    extract_many(jobs, engine=engine, strata=strata)
    seen_pure = seen_hit = False
    for p, j in zip(plain, jobs):
        for x, y in ((p.filtered_out, j.filtered_out), (p.fp_out, j.fp_out)) + (((p.tp_out, j.tp_out),) if p.tp_out else ()):
            assert open(x, "rb").read() == open(y, "rb").read()
        rec, tru = j.stats.pop("strata_rec"), j.stats.pop("strata_tru")
        for k in p.stats:
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        pure = is_pure_strain(j.vcf_file)
        kept = ts.snp_keys(open(j.filtered_out, "rb").read())
        genome = set() if pure else ts.snp_keys(open(j.snp_file, "rb").read())
        wrec, wtru = text_counts(j.filtered_out, j.tp_out or None, j.fp_out, genome, kept)
        np.testing.assert_array_equal(rec, wrec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(tru, wtru, err_msg=j.vcf_file)
        assert rec.sum(axis=0).tolist() == [j.stats["n_pass"], j.stats["tp_lines"], j.stats["fp_lines"]]
        if pure:
            seen_pure = True
            assert not tru.any() and not rec[:, 1].any() and rec[:, 2].sum() > 0
        else:
            assert tru.sum(axis=0).tolist() == [j.stats["truth_unique"], j.stats["TP_R"]]
            seen_hit = seen_hit or (tru[0, 1] > 0 and tru[1, 1] > 0)
    assert seen_pure and seen_hit
    with pytest.raises(ValueError):
        extract_many(_golden_jobs(str(tmp_path / "c")), engine=engine, strata=strata, fn=True)
    with pytest.raises(ValueError):
        extract_many(_golden_jobs(str(tmp_path / "c")), engine=engine, strata=strata, profile=dict(want=[1] * len(jobs)))
    with pytest.raises(ValueError):
        extract_many(_golden_jobs(str(tmp_path / "c")), engine=engine, strata=strata, groups=[[0]])
    with pytest.raises(ValueError):
        extract_many(_golden_jobs(str(tmp_path / "c")), engine=engine, strata=strata, genomes=[None] * len(jobs))


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]


def _num(x):
    return 0 if x == "NA" else int(x)


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_strata_table_and_flag_off_tree(engine, tmp_path, gpus):
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    strata = _bed(tmp_path)
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), strata=strata, **kw)
    on = _tree(str(out))
    name = "results/final_tables/caller_performance_strata.tsv"
    assert name in on
    if gpus == 1:                                                   # without the flag: the same tree minus the new table
        off_dir = tmp_path / "off"
        workflow.run_hcmv_variantcall(str(data), str(off_dir), engine=engine)
        assert _tree(str(off_dir)) == {k: v for k, v in on.items() if k != name}
    head, rows = _table(str(out / name))
    assert head == ["caller", "mixture", "stratum", "genomediff", "calleridentify", "TP_lines", "FP_lines", "TP", "FN", "Precision", "Recall", "F1"]
    _, whole = _table(str(out / "results" / "final_tables" / "caller_performance.tsv"))
    assert len(rows) == 4 * len(whole) == 4 * len(jobs)
    for i, w in enumerate(whole):
        mine = rows[4 * i:4 * i + 4]
        assert [r["stratum"] for r in mine] == ["lo", "hi", "outside", "nokey"]
        assert all(r["caller"] == w["caller"] and r["mixture"] == w["mixture"] for r in mine)
        assert mine[3]["genomediff"] == mine[3]["TP"] == mine[3]["FN"] == mine[3]["Precision"] == mine[3]["Recall"] == mine[3]["F1"] == "NA"
        for col in ("calleridentify", "TP", "genomediff"):          # the strata partition the positions: they sum to the whole-genome row
            assert sum(_num(r[col]) for r in mine) == _num(w[col]), (w["caller"], w["mixture"], col)
        assert sum(int(r["TP_lines"]) + int(r["FP_lines"]) for r in mine) == _num(w["calleridentify"])
    # the rows against the text of the written files
    for j, i in zip(jobs, range(len(jobs))):
        pure = bool(j.stats.get("pure_strain"))
        kept = ts.snp_keys(open(j.filtered_out, "rb").read())
        genome = set() if pure else ts.snp_keys(open(j.snp_file, "rb").read())
        wrec, wtru = text_counts(j.filtered_out, j.tp_out or None, j.fp_out, genome, kept)
        for k, r in enumerate(rows[4 * i:4 * i + 4]):
            assert [int(r["calleridentify"]), int(r["TP_lines"]), int(r["FP_lines"])] == wrec[k].tolist()
            if k < 3 and not pure:
                assert [int(r["genomediff"]), int(r["TP"]), int(r["FN"])] == [wtru[k, 0], wtru[k, 1], wtru[k, 0] - wtru[k, 1]]
            if k < 3 and pure:
                assert (r["genomediff"], r["TP"], r["FN"], r["Precision"], r["Recall"], r["F1"]) == ("NA", "0", "NA", "0", "NA", "NA")
    snaps = test_workflow_strata_table_and_flag_off_tree.snaps
    snaps[gpus] = on[name]
    if len(snaps) == 2:                                             # a VCF's rows do not depend on the rank
        assert snaps[1] == snaps[2]


test_workflow_strata_table_and_flag_off_tree.snaps = {}


def test_vareval_strata(engine, tmp_path):
    import os
    from conftest import GOLDEN, golden_cases
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_gpu_afprofile import _tree
    from test_gpu_truthside import _custom_keys
    strata = _bed(tmp_path)
    cases = [e for e in golden_cases() if e["family"] == "custom"]
    fam = os.path.join(GOLDEN, "custom")
    vcfs = [os.path.join(fam, e["vcf"]) for e in cases]
    snps = os.path.join(fam, cases[0]["truth"])
    labels = ["c%d" % k for k in range(len(vcfs))]
    jobs = workflow.run_vareval(vcfs, snps, str(tmp_path / "on"), labels=labels, engine=engine, strata=strata)
    workflow.run_vareval(vcfs, snps, str(tmp_path / "off"), labels=labels, engine=engine)
    on, off = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off"))
    name = "results/final_tables/snpcall_benchmark_strata.txt"
    assert off == {k: v for k, v in on.items() if k != name} and name in on
    head, rows = _table(str(tmp_path / "on" / name))
    assert head == ["caller", "stratum", "genomediff", "calleridentify", "TP_lines", "FP_lines", "TP", "FN", "precision", "recall", "f1"]
    _, whole = _table(str(tmp_path / "on" / "results" / "final_tables" / "snpcall_benchmark.txt"))
    genome = _custom_keys(open(snps, "rb").read())
    assert len(rows) == 4 * len(jobs)
    for i, (j, w) in enumerate(zip(jobs, whole)):
        mine = rows[4 * i:4 * i + 4]
        assert [r["stratum"] for r in mine] == ["lo", "hi", "outside", "nokey"] and all(r["caller"] == labels[i] for r in mine)
        for col in ("calleridentify", "TP", "genomediff"):
            assert sum(_num(r[col]) for r in mine) == _num(w[col]), (labels[i], col)
        kept = ts.snp_keys(open(j.filtered_out, "rb").read())
        wrec, wtru = text_counts(j.filtered_out, j.tp_out or None, j.fp_out, genome, kept)
        for k, r in enumerate(mine):
            assert [int(r["calleridentify"]), int(r["TP_lines"]), int(r["FP_lines"])] == wrec[k].tolist()
            if k < 3:
                assert [int(r["genomediff"]), int(r["TP"]), int(r["FN"])] == [wtru[k, 0], wtru[k, 1], wtru[k, 0] - wtru[k, 1]]
