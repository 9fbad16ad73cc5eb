"""Sequence-context profiles on the device (qm_genome_context, qm_batch_context; k_context_build / k_context_records /
k_context_truth) against the numpy restatement of quasimodo_amd.context, tied to the batch's columns, class
masks and hit bitmaps, and to the merged stratification pass.  Every comparison is exact: these are integers."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_columns, random_truth
from quasimodo_amd import context as cx
from quasimodo_amd import strata as st
from quasimodo_amd._lib import QmvtError, check
from test_context_host import planted_genome

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
F_NOKEY = 4
S_NPASS, S_TP_LINES, S_FP_LINES, S_TP_R, S_TRUTH = 0, 1, 2, 3, 7
TILE = 4096                                        # positions per workgroup of k_context_build (qmvt_context.h CX_TILE)


def code(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code


def raw_genome_context(engine, gid, w, ng):
    """past the wrapper's own check of the parameters: the library's answer and message"""
    with pytest.raises(QmvtError) as ei:
        check(engine._L.qm_genome_context(engine._h, gid, w, ng, None, None), engine._h)
    return ei.value.code, str(ei.value)


def raw_batch_context(b, gids, w, ng):
    g = np.ascontiguousarray(gids, np.int32)
    with pytest.raises(QmvtError) as ei:
        b._ck(b._L.qm_batch_context(b._h, g.ctypes.data_as(C.c_void_p), w, ng, 1, None))
    return ei.value.code, str(ei.value)


def check_table(engine, seq, w, ng):
    gid = engine.genome_load(seq)
    try:
        got, gen = engine.genome_context(gid, w, ng)
    finally:
        engine.genome_release(gid)
    want = cx.cells(seq, w, ng)
    np.testing.assert_array_equal(got, want, err_msg="L = %d, w = %d, ng = %d" % (len(seq), w, ng))
    np.testing.assert_array_equal(gen.astype(np.int64), cx.positions(want, ng))
    assert int(gen.sum()) == len(seq)


# ---- the table ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 7, 8, 9, 15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_table_lengths(engine, L):
    """8 bases per packed word, 16 positions per lane, TILE per workgroup: the genome ends on, before and behind each edge"""
    g = planted_genome(4)
    for start, (w, ng) in ((95, (50, 10)), (29990, (1, 15)), (2 * TILE - L // 2, (1024, 3))):   # planted runs; into the N block; a tile edge inside
        check_table(engine, g[start:start + L], w, ng)


@pytest.fixture(scope="module")
def planted(engine):
    seq = planted_genome(1)
    gid = engine.genome_load(seq)
    yield seq, gid
    engine.genome_release(gid)


@pytest.mark.parametrize("w,ng", [(0, 1), (1, 15), (50, 10), (1024, 10)])
def test_table_planted(engine, planted, w, ng):
    """one genome id through four parameter pairs: each call rebuilds the cached table"""
    seq, gid = planted
    want = cx.cells(seq, w, ng)
    for _ in range(2):                             # built, then served from the cache
        got, gen = engine.genome_context(gid, w, ng)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(gen.astype(np.int64), cx.positions(want, ng))
    assert int(gen.sum()) == len(seq) == 60000


def test_table_refuses(engine, planted):
    _, gid = planted
    for w, ng, named in ((1025, 10, "half window"), (-1, 10, "half window"), (50, 0, "GC bins"), (50, 16, "GC bins")):
        c, msg = raw_genome_context(engine, gid, w, ng)
        assert c == QM_E_INVAL and named in msg
    assert raw_genome_context(engine, 999, 50, 10)[0] == QM_E_INVAL
    with pytest.raises(ValueError):
        engine.genome_context(gid, 1025, 10)


# ---- records and truth --------------------------------------------------------------------------------------------------
SIZES = [70000, 0, 1, 255, 256, 257, 3, 1023, 1024, 1025, 16384, 16385]   # 70 000: more than the 65 536 records one workgroup may see; 1023 .. 1025: a step of the span walk; 16 384: a span
WHICH_TRUTH = [0, 1, 0, 1, 0, 0, 1, 0, 1, 0, 1, 0]   # VCFs 0 and 4 share a truth set and name different genomes
WHICH_GENOME = [0, 0, 1, -1, 1, 0, 1, 0, -1, 1, 0, 1]
LEN_B = 37003


def truth_keys(truth):
    p, r, a = (np.asarray(x, np.int64) for x in truth)
    ok = (r >= 0) & (r < 4) & (a >= 0) & (a < 4)
    return np.unique((p[ok] << 4) | (r[ok] << 2) | a[ok])


def biased_truth(rng, t, L):
    """a third of the keys on the planted runs, a few in the N block"""
    pos, ref, alt = random_truth(rng, t, L)
    u = rng.random(t)
    pos = np.where(u < 0.33, rng.integers(95, 1500, t), np.where(u < 0.38, rng.integers(29990, 32200, t), pos)).astype(np.int32)
    return pos, ref, alt


def biased_columns(rng, n, L, truth, sorted_):
    """random_columns with a fifth of the positions moved onto the planted runs and the N block; positions up to L + 300"""
    pos, ref, alt, qual, flags = random_columns(rng, n, L + 300, truth, sorted_=False)
    u = rng.random(n)
    pos = np.where(u < 0.15, rng.integers(95, 1500, n), np.where(u < 0.2, rng.integers(29990, 32200, n), pos)).astype(np.int32)
    if sorted_:
        o = np.argsort(pos, kind="stable")
        pos, ref, alt, qual, flags = pos[o], ref[o], alt[o], qual[o], flags[o]
    return tuple(np.ascontiguousarray(x) for x in (pos, ref, alt, qual, flags))


def make_batch(engine, cols, tids, alleles=False):
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b


def restate_rec(tab, ng, cols, cls):
    """[n_cells + 1][3] of one VCF from its columns and class bytes (bit 0 kept, bit 1 TP); tab None: no genome, zero rows"""
    nc = cx.n_cells(ng)
    out = np.zeros((nc + 1, 3), np.uint64)
    if tab is None:
        return out
    pos, flags = cols[0], cols[4]
    kept, tp = (cls & 1) != 0, (cls & 2) != 0
    row = np.where((flags & F_NOKEY) != 0, nc, cx.rows_of(tab, pos, ng))
    out[:, 0] = np.bincount(row[kept], minlength=nc + 1)
    out[:, 1] = np.bincount(row[kept & tp], minlength=nc + 1)
    out[:, 2] = np.bincount(row[kept & ~tp], minlength=nc + 1)
    return out


def restate_tru(tab, ng, keys, hits):
    nc = cx.n_cells(ng)
    out = np.zeros((nc, 2), np.uint64)
    if tab is None:
        return out
    row = cx.rows_of(tab, keys >> 4, ng)
    out[:, 0] = np.bincount(row, minlength=nc)
    out[:, 1] = np.bincount(row[hits], minlength=nc)
    return out


@pytest.fixture(scope="module")
def genomes(engine, planted):
    seq_a, gid_a = planted
    seq_b = planted_genome(2)[:LEN_B]
    gid_b = engine.genome_load(seq_b)
    yield [(seq_a, gid_a), (seq_b, gid_b)]
    engine.genome_release(gid_b)


@pytest.fixture(scope="module")
def tables(genomes):
    """the restated tables, once: {(genome, w, ng): cells}"""
    return {(k, w, ng): cx.cells(genomes[k][0], w, ng) for k in (0, 1) for w, ng in ((50, 10), (3, 15))}


@pytest.fixture(scope="module", params=[True, False], ids=["sorted", "shuffled"])
def shape_batch(engine, request, genomes):
    rng = np.random.default_rng(21 if request.param else 22)
    truths = [biased_truth(rng, 700, 60000), biased_truth(rng, 40, 60000)]
    tids = [engine.truth_load(*t) for t in truths]
    cols = [biased_columns(rng, n, 60000, truths[w], request.param) for n, w in zip(SIZES, WHICH_TRUTH)]
    b = make_batch(engine, cols, [tids[w] for w in WHICH_TRUTH])
    b.truth_hits()
    nv = len(SIZES)
    ref = {"cols": [b.columns(v) for v in range(nv)], "cls": [b.cls(v) for v in range(nv)], "hits": [b.truth_hit_bits(v) for v in range(nv)],
           "keys": [truth_keys(truths[w]) for w in WHICH_TRUTH], "scal": b.scalars(),
           "gids": [genomes[k][1] if k >= 0 else -1 for k in WHICH_GENOME]}
    yield b, ref
    b.close()


@pytest.mark.parametrize("w,ng", [(50, 10), (3, 15), (50, 10)], ids=["50x10", "3x15", "50x10-again"])
def test_shapes(engine, shape_batch, tables, w, ng):
    """the second and third case ask the same batch and genomes for other parameters: the cached tables are rebuilt"""
    b, ref = shape_batch
    rec, tru, gen = b.context(ref["gids"], w, ng, truth=True)
    nc, nv = cx.n_cells(ng), len(SIZES)
    assert rec.shape == (nv, nc + 1, 3) and tru.shape == (nv, nc, 2) and gen.shape == (nv, nc)
    for v in range(nv):
        k = WHICH_GENOME[v]
        tab = tables[(k, w, ng)] if k >= 0 else None
        np.testing.assert_array_equal(rec[v], restate_rec(tab, ng, ref["cols"][v], ref["cls"][v]), err_msg="VCF %d rec" % v)
        np.testing.assert_array_equal(tru[v], restate_tru(tab, ng, ref["keys"][v], ref["hits"][v]), err_msg="VCF %d tru" % v)
        assert (rec[v, :, 0] == rec[v, :, 1] + rec[v, :, 2]).all()
        sc = ref["scal"][v]
        if k < 0:
            assert not rec[v].any() and not tru[v].any() and not gen[v].any()
            continue
        np.testing.assert_array_equal(gen[v].astype(np.int64), cx.positions(tab, ng))
        assert rec[v].sum(axis=0).tolist() == [sc[S_NPASS], sc[S_TP_LINES], sc[S_FP_LINES]]
        assert tru[v].sum(axis=0).tolist() == [sc[S_TRUTH], sc[S_TP_R]]
    # the case is not empty: nokey and NONE rows, TP lines and hit keys on long runs, VCFs 0 and 4 placed by different genomes
    assert rec[:, nc, 0].sum() > 0 and rec[:, nc - 1, 0].sum() > 0 and rec[0, 8 * ng:16 * ng, 1].sum() > 0 and tru[0, 8 * ng:16 * ng, 1].sum() > 0
    assert (tru[0, :, 0] != tru[4, :, 0]).any() and tru[0, :, 0].sum() == tru[4, :, 0].sum()


def test_row_marginals_equal_the_strata_pass(engine, shape_batch, tables):
    """strata built from the restated cells, one per homopolymer row: the merged pass counts what the rows of this one sum to"""
    b, ref = shape_batch
    ng = 10
    tab = tables[(0, 50, ng)]
    strata = []
    for h in range(16):
        m = np.concatenate([[False], (tab != cx.NONE_BYTE) & (tab // ng == h), [False]])
        edge = np.flatnonzero(m[1:] != m[:-1])     # position p = i + 1 of table entry i lies in the BED interval (i, i + 1]
        strata.append(("hp%d" % h, edge[0::2].astype(np.int64), edge[1::2].astype(np.int64)))
    sid = engine.strata_load(strata)
    try:
        b.strata(sid, truth=True)
        srec, stru = b.strata_counts()
    finally:
        engine.strata_release(sid)
    rec, tru, _ = b.context(ref["gids"], 50, ng, truth=True)
    seen = 0
    for v in range(len(SIZES)):
        if WHICH_GENOME[v] != 0:
            continue
        rows = np.concatenate([rec[v, :16 * ng].reshape(16, ng, 3).sum(axis=1), rec[v, 16 * ng:]])          # the rows, NONE, nokey
        np.testing.assert_array_equal(srec[v], rows)
        np.testing.assert_array_equal(stru[v], np.concatenate([tru[v, :16 * ng].reshape(16, ng, 2).sum(axis=1), tru[v, 16 * ng:]]))
        seen += int(srec[v].sum())
    assert seen > 0


def test_allele_extended_records_only(engine, genomes, tables):
    from test_gpu_alleles import ext_columns, ext_truth
    rng = np.random.default_rng(5)
    truth = ext_truth(rng, 300, 37000)
    tid = engine.truth_load(*truth)
    cols = [ext_columns(rng, n, 37000, truth) for n in (257, 3000)]
    b = make_batch(engine, cols, [tid, tid], alleles=True)
    gids = [genomes[1][1], genomes[0][1]]
    assert code(lambda: b.context(gids, 50, 10, truth=True)) == QM_E_STATE
    rec, tru, gen = b.context(gids, 50, 10)
    assert tru is None
    sc = b.scalars()
    indels = 0
    for v in range(2):
        c, cls = b.columns(v), b.cls(v)
        np.testing.assert_array_equal(rec[v], restate_rec(tables[(1 - v, 50, 10)], 10, c, cls))
        indels += int((((cls & 1) != 0) & ((c[1] >= 4) | (c[2] >= 4))).sum())
        assert rec[v].sum(axis=0).tolist() == [sc[v, S_NPASS], sc[v, S_TP_LINES], sc[v, S_FP_LINES]]
    assert indels > 0, "kept indels are counted, by their POS"
    b.close()


def test_state_rules(engine, genomes, tables):
    rng = np.random.default_rng(9)
    truth = biased_truth(rng, 100, 3000)
    tid = engine.truth_load(*truth)
    cols = [biased_columns(rng, n, 3000, truth, True) for n in (500, 1300)]
    gids = [genomes[0][1], genomes[1][1]]
    extra = engine.genome_load(b"ACGTTTTTGGA" * 30)
    b = engine.batch([len(c[0]) for c in cols], [tid, tid])
    for v, c in enumerate(cols):
        b.upload(v, *c)
    assert code(lambda: b.context(gids)) == QM_E_STATE                         # nothing ran
    assert code(b.context_counts) == QM_E_STATE
    b.run()
    assert code(lambda: b.context(gids)) == QM_E_STATE                         # before finish
    b.finish()
    db0 = b.device_bytes
    assert code(lambda: b.context(gids, truth=True)) == QM_E_STATE             # TRUTH without truth hits
    for w, ng, named in ((1025, 10, "half window"), (50, 0, "GC bins"), (50, 16, "GC bins")):
        c, msg = raw_batch_context(b, gids, w, ng)
        assert c == QM_E_INVAL and named in msg
    assert code(lambda: b.context([gids[0], 999])) == QM_E_INVAL
    with pytest.raises(ValueError):
        b.context(gids, 50, 16)
    with pytest.raises(ValueError):
        b.context(gids[:1])
    assert b.device_bytes == db0                                               # a batch that never got an answer allocated nothing
    b.set_timing(True)
    rec, tru, gen = b.context(gids, 50, 10)
    nv, nc = 2, 161
    assert tru is None and b.device_bytes == db0 + nv * nc * 8 + nv * 16 + nv * (nc + 1) * 2 * 8
    b._context = (10, True)                                                    # ask for the half that was not made
    assert code(b.context_counts) == QM_E_STATE
    cls = [b.cls(v) for v in range(2)]
    for v in range(2):
        np.testing.assert_array_equal(rec[v], restate_rec(tables[(v, 50, 10)], 10, cols[v], cls[v]))
    b.context(gids, 50, 10)
    t = b.context_timings()
    assert t["context_build_ms"] == 0.0 and t["context_records_ms"] > 0.0      # both tables were cached by the call before
    b.truth_hits()
    rec, tru, gen = b.context(gids, 3, 15, truth=True)                         # other parameters: the other tables' counts
    keys = truth_keys(truth)
    for v in range(2):
        np.testing.assert_array_equal(rec[v], restate_rec(tables[(v, 3, 15)], 15, cols[v], cls[v]))
        np.testing.assert_array_equal(tru[v], restate_tru(tables[(v, 3, 15)], 15, keys, b.truth_hit_bits(v)))
    assert b.context_timings()["context_build_ms"] > 0.0
    # a released genome
    assert not b.context([extra, -1], 50, 10)[0][1].any()
    engine.genome_release(extra)
    assert code(lambda: b.context([extra, -1], 50, 10)) == QM_E_STATE
    # after a re-run the counts are gone until the pass is repeated
    b.run()
    assert code(b.context_counts) == QM_E_STATE
    b.finish()
    assert code(b.context_counts) == QM_E_STATE
    assert code(lambda: b.context(gids, truth=True)) == QM_E_STATE             # the truth hits are gone too
    np.testing.assert_array_equal(b.context(gids, 50, 10)[0][0], restate_rec(tables[(0, 50, 10)], 10, cols[0], cls[0]))
    b.close()
