"""The paired block-bootstrap pass (qm_batch_boot, k_boot_records / k_boot_truth / k_boot_resample) against a
numpy restatement tied to the batch's columns, class masks and hit bitmaps, against the stratification pass on a one-stratum
set, and end to end against the text of the written files.  Every comparison is exact: these are integers."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_cases, random_columns, random_truth
from quasimodo_amd import _lib
from quasimodo_amd import bootstrap as bs
from quasimodo_amd._lib import QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
F_PASS, F_IDDOT, F_NOKEY = 1, 2, 4
I32MAX = (1 << 31) - 1
S_NPASS, S_TP_LINES, S_TP_R, S_TRUTH = 0, 1, 3, 7
SHAPES = [(1, 1), (7, 2), (1024, 236), (3, 4096)]
SIZES = [0, 1, 3, 63, 64, 65, 257, 1023, 1024, 1025, 5000, 16384, 16385, 300]   # 1023 .. 1025: a step of the span walk; 16 384: a span; the last one holds no kept record
TOP = 250000                                            # beyond 1024 * 236 = 241 664


def code(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    return ei.value.code


def truth_keys(truth):
    p, r, a = (np.asarray(x, np.int64) for x in truth)
    ok = (r >= 0) & (r < 4) & (a >= 0) & (a < 4)
    return np.unique((p[ok] << 4) | (r[ok] << 2) | a[ok])


def rows_of(pos, window, n_win):
    pos = np.asarray(pos, np.int64)
    w = (pos - 1) // window
    return np.where((pos >= 1) & (w < n_win), w, n_win)


def restate_cnt(window, n_win, cols, cls, keys, hits):
    """[n_win + 2][4] of one VCF from its columns, class bytes (bit 0 kept, bit 1 TP), truth keys and hit bits"""
    out = np.zeros((n_win + 2, 4), np.uint64)
    kept, tp = (cls & 1) != 0, (cls & 2) != 0
    row = np.where((cols[4] & F_NOKEY) != 0, n_win + 1, rows_of(cols[0], window, n_win))
    out[:, 0] = np.bincount(row[kept], minlength=n_win + 2)
    out[:, 1] = np.bincount(row[kept & tp], minlength=n_win + 2)
    if keys is not None:
        krow = rows_of(keys >> 4, window, n_win)
        out[:, 2] = np.bincount(krow, minlength=n_win + 2)
        out[:, 3] = np.bincount(krow[hits], minlength=n_win + 2)
    return out


def lib_mult(seed, n_win, n_rep):
    m = np.zeros((max(n_rep, 1), n_win), np.uint16)
    assert _lib.lib().qm_boot_draws(C.c_uint64(seed), n_win, n_rep, m.ctypes.data_as(C.c_void_p)) == 0
    return m[:n_rep].astype(np.uint64)


def restate_rep(cnt, mult):
    n_win = mult.shape[1]
    return mult @ cnt[:n_win] + cnt[n_win] + cnt[n_win + 1]


def edge_positions(rng, n):
    """positions on the window edges q * window + {0, 1} of every shape, at 0, beyond the last window, and in between"""
    edges = [0, 1, 2, TOP, TOP - 1, 241664, 241665, 12288, 12289, 14, 15, 7, 8]
    for window, n_win in SHAPES:
        for q in rng.integers(0, n_win + 1, size=12):
            edges += [int(q) * window, int(q) * window + 1]
    pick = rng.random(n)
    pos = np.where(pick < 0.35, rng.integers(0, 21, size=n), np.where(pick < 0.6, rng.integers(0, 13000, size=n), rng.integers(1, TOP + 1, size=n)))
    e = rng.random(n) < 0.3
    return np.where(e, np.array(edges)[rng.integers(0, len(edges), size=n)], pos).astype(np.int32)


def edge_truth(rng, t):
    pos = edge_positions(rng, t)
    return pos, rng.integers(0, 4, size=t).astype(np.int32), rng.integers(0, 4, size=t).astype(np.int32)


def edge_columns(rng, n, truth, sorted_, kept=True):
    pos, ref, alt, qual, flags = random_columns(rng, n, TOP, truth, sorted_=False)
    fresh = rng.random(n) < 0.5                                     # half keep their truth keys, half move to the edges
    pos = np.where(fresh, edge_positions(rng, n), pos).astype(np.int32)
    if not kept:
        flags = (flags & ~np.uint8(F_PASS | 8)).astype(np.uint8)   # fails the filter, and no host decision
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


@pytest.fixture(scope="module", params=[True, False], ids=["sorted", "shuffled"])
def shape_batch(engine, request):
    rng = np.random.default_rng(21 if request.param else 22)
    truths = [edge_truth(rng, 900), edge_truth(rng, 45)]
    tids = [engine.truth_load(*t) for t in truths]
    which = [v % 2 for v in range(len(SIZES))]
    cols = [edge_columns(rng, n, truths[w], request.param, kept=(v != len(SIZES) - 1)) for v, (n, w) in enumerate(zip(SIZES, which))]
    b = make_batch(engine, cols, [tids[w] for w in which])
    b.truth_hits()
    nv = len(SIZES)
    ref = {"cols": [b.columns(v) for v in range(nv)], "cls": [b.cls(v) for v in range(nv)], "hits": [b.truth_hit_bits(v) for v in range(nv)],
           "keys": [truth_keys(truths[w]) for w in which], "scal": b.scalars(), "tids": [tids[w] for w in which], "raw": cols}
    assert not (ref["cls"][nv - 1] & 1).any() and all((ref["cls"][v] & 1).any() for v in range(4, nv - 1))
    yield b, ref
    b.close()


# ---- counts and replicates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,n_win", SHAPES)
def test_counts_against_numpy(engine, shape_batch, window, n_win):
    b, ref = shape_batch
    nv = len(SIZES)
    b.boot(window, n_win, 0, truth=True)
    cnt, rep = b.boot_counts()
    assert cnt.shape == (nv, n_win + 2, 4) and cnt.dtype == np.uint64 and rep.shape == (nv, 0, 4)
    for v in range(nv):
        want = restate_cnt(window, n_win, ref["cols"][v], ref["cls"][v], ref["keys"][v], ref["hits"][v])
        np.testing.assert_array_equal(cnt[v], want, err_msg="VCF %d" % v)
        sc = ref["scal"][v]
        assert cnt[v].sum(axis=0).tolist() == [sc[S_NPASS], sc[S_TP_LINES], sc[S_TRUTH], sc[S_TP_R]]
        assert not cnt[v, n_win + 1, 2:].any()
    assert cnt[:, n_win + 1, 0].sum() > 0 and cnt[:, n_win, 0].sum() > 0 and cnt[:, n_win, 2].sum() > 0      # the case is not empty
    assert window * n_win < 100 or cnt[:, :n_win, 3].sum() > 0
    assert not cnt[nv - 1, :, :2].any()
    # the record side alone: the truth columns are zero
    b.boot(window, n_win, 0)
    rec_only = b.boot_counts()[0]
    np.testing.assert_array_equal(rec_only[:, :, :2], cnt[:, :, :2])
    assert not rec_only[:, :, 2:].any()


def test_counts_equal_the_one_stratum_set(engine, shape_batch):
    b, ref = shape_batch
    sid = engine.strata_load([("all", [0], [I32MAX])])
    b.strata(sid, truth=True)
    rec, tru = b.strata_counts()
    engine.strata_release(sid)
    for window, n_win in SHAPES:
        b.boot(window, n_win, 0, truth=True)
        cnt = b.boot_counts()[0]
        placed = cnt[:, :n_win + 1].sum(axis=1)                                 # windows + outside
        np.testing.assert_array_equal(placed[:, :2], rec[:, 0, :2] + rec[:, 1, :2])   # the stratum and its `outside` (pos 0)
        np.testing.assert_array_equal(cnt[:, n_win + 1, :2], rec[:, 2, :2])           # nokey
        np.testing.assert_array_equal(placed[:, 2:], tru[:, 0] + tru[:, 1])


@pytest.mark.parametrize("window,n_win", SHAPES)
@pytest.mark.parametrize("n_rep", [1, 3, 1000])
def test_replicates_against_numpy(engine, shape_batch, window, n_win, n_rep):
    b, ref = shape_batch
    b.boot(window, n_win, n_rep, seed=2024, truth=True)
    cnt, rep = b.boot_counts()
    mult = lib_mult(2024, n_win, n_rep)
    np.testing.assert_array_equal(mult.astype(np.int64), bs.multiplicities(2024, n_win, n_rep))
    assert rep.shape == (len(SIZES), n_rep, 4)
    for v in range(len(SIZES)):
        np.testing.assert_array_equal(rep[v], restate_rep(cnt[v], mult), err_msg="VCF %d" % v)
        if n_win == 1:
            assert (rep[v] == cnt[v].sum(axis=0)).all()
    if n_rep == 3:
        b.boot(window, n_win, n_rep, seed=2024, truth=True)                     # the same call twice: identical bytes
        cnt2, rep2 = b.boot_counts()
        assert cnt2.tobytes() == cnt.tobytes() and rep2.tobytes() == rep.tobytes()
        b.boot(window, n_win, n_rep, seed=2025, truth=True)
        cnt3, rep3 = b.boot_counts()
        assert cnt3.tobytes() == cnt.tobytes()
        mult3 = lib_mult(2025, n_win, n_rep)                                    # another seed: that seed's draws
        for v in range(len(SIZES)):
            np.testing.assert_array_equal(rep3[v], restate_rep(cnt[v], mult3))
        if n_win >= 236:                                                        # (three draws of two windows can coincide by chance, and do)
            assert (mult3 != mult).any() and rep3.tobytes() != rep.tobytes()


def test_pinned_multiplicities_one_record_per_window(engine):
    tid = engine.truth_load(np.array([5], np.int32), np.array([0], np.int32), np.array([1], np.int32))
    pos = np.arange(8, dtype=np.int32) * 10 + 3                                  # window w of 10 positions holds position 10 w + 3
    def cols(p):
        n = len(p)
        return (np.ascontiguousarray(p, np.int32), np.zeros(n, np.int32), np.ones(n, np.int32), np.full(n, 50, np.float32), np.full(n, F_PASS | F_IDDOT, np.uint8))
    # VCF w holds one kept record, in window w; VCF 8 holds one in every window
    b = make_batch(engine, [cols(pos[w:w + 1]) for w in range(8)] + [cols(pos)], [tid] * 9)
    b.boot(10, 8, 2, seed=0)
    cnt, rep = b.boot_counts()
    want = [[2, 1, 1, 1, 0, 0, 1, 2], [0, 1, 0, 1, 3, 1, 1, 1]]
    assert lib_mult(0, 8, 2).tolist() == want
    assert cnt[8, :, 0].tolist() == [1] * 8 + [0, 0] and rep[8, :, 0].tolist() == [8, 8]
    for w in range(8):                                                          # the replicate counts how often window w was drawn
        assert cnt[w, :, 0].tolist() == [int(k == w) for k in range(10)]
        assert rep[w, :, 0].tolist() == [want[0][w], want[1][w]]
    b.close()


def test_one_contended_window_and_vcf_order(engine):
    """all 5000 records of a VCF in one window (every wave on one counter); VCFs of more than 65 536 records, sorted and shuffled,
    whose workgroups meet in the VCF's rows (at 236 windows and at the full LDS table of 4096); and the batch's VCF order does not
    change a VCF's replicates"""
    rng = np.random.default_rng(33)
    truth = random_truth(rng, 200, 1000)
    tid = engine.truth_load(*truth)
    crowd = random_columns(rng, 5000, 1000, truth)                               # positions 1 .. 1000: window 0 of 1024
    other = random_columns(rng, 700, 200000, truth, sorted_=False)
    big = random_columns(rng, 70000, 200000, truth)                              # five spans: one VCF over two workgroups
    big_sh = random_columns(rng, 70000, 13000, truth, sorted_=False)             # the same, shuffled, inside 3 x 4096 and beyond
    b = make_batch(engine, [crowd, other, big, big_sh], [tid] * 4)
    b.truth_hits()
    keys = truth_keys(truth)
    ref = [(b.columns(v), b.cls(v), b.truth_hit_bits(v)) for v in range(4)]
    for window, n_win in ((3, 4096), (1024, 236)):
        b.boot(window, n_win, 50, seed=9, truth=True)
        cnt, rep = b.boot_counts()
        mult = lib_mult(9, n_win, 50)
        for v in range(4):
            np.testing.assert_array_equal(cnt[v], restate_cnt(window, n_win, ref[v][0], ref[v][1], keys, ref[v][2]), err_msg="%d x %d VCF %d" % (window, n_win, v))
            np.testing.assert_array_equal(rep[v], restate_rep(cnt[v], mult))
        assert cnt[3, :n_win, 0].sum() > 30000
    assert cnt[0, 0, 0] > 3000 and not cnt[0, 1:237, 0].any()
    b2 = make_batch(engine, [other, crowd], [tid, tid])
    b2.truth_hits()
    b2.boot(1024, 236, 50, seed=9, truth=True)
    cnt2, rep2 = b2.boot_counts()
    assert cnt2[1].tobytes() == cnt[0].tobytes() and cnt2[0].tobytes() == cnt[1].tobytes()
    assert rep2[1].tobytes() == rep[0].tobytes() and rep2[0].tobytes() == rep[1].tobytes()
    b.close()
    b2.close()


# ---- allele-extended batches, state rules ---------------------------------------------------------------------------------
def test_allele_extended_records_only(engine):
    from test_gpu_alleles import ext_columns, ext_truth
    rng = np.random.default_rng(5)
    truth = ext_truth(rng, 300, 20000)
    tid = engine.truth_load(*truth)
    cols = [ext_columns(rng, n, 20000, truth) for n in (257, 3000)]
    b = make_batch(engine, cols, [tid, tid], alleles=True)
    assert code(lambda: b.boot(100, 236, 3, truth=True)) == QM_E_STATE
    b.boot(100, 236, 3)
    cnt, rep = b.boot_counts()
    sc = b.scalars()
    mult = lib_mult(0, 236, 3)
    for v in range(2):
        np.testing.assert_array_equal(cnt[v], restate_cnt(100, 236, b.columns(v), b.cls(v), None, None))
        np.testing.assert_array_equal(rep[v], restate_rep(cnt[v], mult))
        assert cnt[v].sum(axis=0).tolist() == [sc[v, S_NPASS], sc[v, S_TP_LINES], 0, 0]
    b.close()


def test_state_rules_arguments_and_device_bytes(engine):
    rng = np.random.default_rng(9)
    truth = random_truth(rng, 100, 3000)
    tid = engine.truth_load(*truth)
    cols = [random_columns(rng, n, 3000, truth) for n in (500, 1300)]
    b = engine.batch([len(c[0]) for c in cols], [tid, tid])
    for v, c in enumerate(cols):
        b.upload(v, *c)
    assert code(lambda: b.boot(10, 8, 2)) == QM_E_STATE                         # nothing ran
    assert code(b.boot_counts) == QM_E_STATE
    b.run()
    assert code(lambda: b.boot(10, 8, 2)) == QM_E_STATE                         # before finish
    b.finish()
    db0 = b.device_bytes
    assert code(b.boot_counts) == QM_E_STATE                                    # none was made
    assert code(lambda: b.boot(10, 8, 2, truth=True)) == QM_E_STATE             # TRUTH without truth hits
    for bad in ((0, 8, 2), (-5, 8, 2), (10, 0, 2), (10, 4097, 2), (10, 8, -1), (10, 8, 16385)):
        assert code(lambda: b.boot(*bad)) == QM_E_INVAL, bad
    L = engine._L
    assert L.qm_batch_boot(b._h, 10, 8, 2, C.c_uint64(0), 0, None) == QM_E_INVAL          # no side
    assert L.qm_batch_boot(b._h, 10, 8, 2, C.c_uint64(0), 4, None) == QM_E_INVAL
    assert L.qm_boot_draws(C.c_uint64(0), 0, 1, None) == QM_E_INVAL and L.qm_boot_draws(C.c_uint64(0), 4097, 0, None) == QM_E_INVAL
    assert b.device_bytes == db0                                                # nothing allocated until the first pass
    nv = 2
    b.boot(10, 8, 0)                                                            # n_rep = 0: counts only
    assert b.device_bytes == db0 + nv * 10 * 4 * 8
    cnt, rep = b.boot_counts()
    assert rep.shape == (2, 0, 4)
    cls = [b.cls(v) for v in range(2)]
    for v in range(2):
        np.testing.assert_array_equal(cnt[v], restate_cnt(10, 8, cols[v], cls[v], None, None))
    assert L.qm_batch_get_boot(b._h, None, None) == 0                           # either pointer may be NULL
    b.boot(10, 8, 5)
    assert b.device_bytes == db0 + nv * 10 * 4 * 8 + nv * 5 * 4 * 8
    b.boot(300, 4096, 1, seed=(1 << 64) - 1)                                    # other parameters, the largest table
    cnt, rep = b.boot_counts()
    np.testing.assert_array_equal(cnt[1], restate_cnt(300, 4096, cols[1], cls[1], None, None))
    np.testing.assert_array_equal(rep[1], restate_rep(cnt[1], lib_mult((1 << 64) - 1, 4096, 1)))
    b.boot(I32MAX, 1, 2)                                                        # one window over every position
    cnt, rep = b.boot_counts()
    assert (rep[0] == cnt[0].sum(axis=0)).all() and cnt[0, 1, 0] == 0
    b.run()                                                                     # after a re-run the counts are gone
    assert code(b.boot_counts) == QM_E_STATE
    b.finish()
    assert code(b.boot_counts) == QM_E_STATE
    b.close()
    # a batch that never calls the pass allocates nothing for it
    b1 = make_batch(engine, cols, [tid, tid])
    b2 = make_batch(engine, cols, [tid, tid])
    assert b1.device_bytes == b2.device_bytes == db0
    b2.boot(10, 8, 2)
    assert b1.device_bytes == db0 and b2.device_bytes > db0
    b1.close()
    b2.close()


# ---- files in, files out ------------------------------------------------------------------------------------------------
PAR = dict(window=1024, n_win=256, n_rep=200, seed=7)


def _data_rows(path):
    if not path:
        return []
    with open(path, "rb") as fh:
        return [ln.split(b"\t") for ln in fh.read().split(b"\n") if ln and ln[:1] != b"#"]


def text_cnt(filtered, tp, truth_keys_text, kept_keys_text, window, n_win):
    """[n_win + 2][4] from the TEXT of the written files and the truth file (the golden families hold no line without a key)"""
    out = np.zeros((n_win + 2, 4), np.uint64)
    for col, path in enumerate((filtered, tp)):
        for f in _data_rows(path):
            out[int(rows_of([int(f[1])], window, n_win)[0]), col] += 1
    for k in truth_keys_text:
        r = int(rows_of([int(k[0])], window, n_win)[0])
        out[r, 2] += 1
        out[r, 3] += k in kept_keys_text
    return out


def test_extract_many_boot_matches_the_written_files(engine, tmp_path):
    from quasimodo_amd import truthside as ts
    from quasimodo_amd.extract import extract_many, is_pure_strain
    from test_gpu_afprofile import _golden_jobs
    plain = _golden_jobs(str(tmp_path / "a"))
    extract_many(plain, engine=engine)
    jobs = _golden_jobs(str(tmp_path / "b"))
    extract_many(jobs, engine=engine, boot=PAR)
    mult = bs.multiplicities(PAR["seed"], PAR["n_win"], PAR["n_rep"]).astype(np.uint64)
    seen_pure = seen_hit = False
    for p, j in zip(plain, jobs):
        for x, y in ((p.filtered_out, j.filtered_out), (p.fp_out, j.fp_out)) + (((p.tp_out, j.tp_out),) if p.tp_out else ()):
            assert open(x, "rb").read() == open(y, "rb").read()
        cnt, rep = j.stats.pop("boot_cnt"), j.stats.pop("boot_rep")
        assert j.stats.pop("boot_params") == PAR and j.stats.pop("boot_truth") is True
        for k in p.stats:
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        pure = is_pure_strain(j.vcf_file)
        kept = ts.snp_keys(open(j.filtered_out, "rb").read())
        genome = set() if pure else ts.snp_keys(open(j.snp_file, "rb").read())
        np.testing.assert_array_equal(cnt, text_cnt(j.filtered_out, j.tp_out or None, genome, kept, PAR["window"], PAR["n_win"]), err_msg=j.vcf_file)
        np.testing.assert_array_equal(rep, restate_rep(cnt, mult), err_msg=j.vcf_file)
        assert cnt.sum(axis=0).tolist() == [j.stats["n_pass"], j.stats["tp_lines"], 0 if pure else j.stats["truth_unique"], j.stats["TP_R"]]
        seen_pure = seen_pure or pure
        seen_hit = seen_hit or cnt[:256, 3].sum() > 0
    assert seen_pure and seen_hit
    for kw in (dict(fn=True), dict(profile=dict(want=[1] * len(jobs))), dict(groups=[[0]]), dict(genomes=[None] * len(jobs)),
               dict(strata=[("all", [0], [I32MAX])])):
        with pytest.raises(ValueError):
            extract_many(_golden_jobs(str(tmp_path / "c")), engine=engine, boot=PAR, **kw)


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]


def _s(x):
    from quasimodo_amd.tables import r_round3, r_str
    return r_str(r_round3(x))


def _raw_f1(stats):
    """the point F1 before any rounding; None where a denominator is zero"""
    n, tp, gd = bs.point(stats)
    if n == 0 or gd == 0 or tp == 0:
        return None
    p, r = tp / n, tp / gd
    return 2 * (p * r) / (p + r)


def _check_ci_rows(jobs, rows, names, strata_rows_of):
    """the ci table's rows against the jobs' counts, numpy replicates and the strata table of the one-stratum set"""
    P, R, F = names
    for j, r in zip(jobs, rows):
        st_ = j.stats
        prm = st_["boot_params"]
        mult = bs.multiplicities(prm["seed"], prm["n_win"], prm["n_rep"])
        all_, outside, nokey = strata_rows_of(j)
        assert int(r["calleridentify"]) == sum(int(x["calleridentify"]) for x in (all_, outside, nokey)) == st_["n_pass"]
        if st_.get("pure_strain"):
            assert (r["genomediff"], r["TP"], r[P], r[R], r[F], r[P + "_lo"], r[F + "_hi"], r["n_valid"]) == ("0", "0", "0", "NA", "NA", "NA", "NA", "0")
            assert (all_["TP"], all_[P]) == ("0", "0")
            continue
        # the point columns: the strata table's rows with outside and nokey folded in, the ratios by strata_rows' formulas
        n, tp, gd = int(r["calleridentify"]), int(r["TP"]), int(r["genomediff"])
        assert tp == int(all_["TP"]) + int(outside["TP"]) and gd == int(all_["genomediff"]) + int(outside["genomediff"])
        assert gd == st_["genomediff"] and tp == st_["TP_R"]
        from quasimodo_amd.strata import _ratio
        from quasimodo_amd.tables import r_round3, r_str
        p, rc = _ratio(tp, n), _ratio(tp, gd)
        f1 = None if p is None or rc is None or p + rc == 0 else r_round3(2 * (p * rc) / (p + rc))
        assert (r[P], r[R], r[F]) == (r_str(p), r_str(rc), r_str(f1))
        if not int(outside["calleridentify"]) and not int(nokey["calleridentify"]) and not int(outside["genomediff"]):
            assert (r[P], r[R], r[F]) == tuple(all_[k] for k in (("Precision", "Recall", "F1") if P == "Precision" else ("precision", "recall", "f1")))
        # the interval columns: bootstrap.interval over a numpy restatement of the replicates
        cnt = st_["boot_cnt"].astype(np.int64)
        nw = prm["n_win"]
        extra = bs.truth_row_windows(j.snp_file, j.mode, prm["window"], nw) - cnt[:nw + 1, 2]
        rep = mult @ cnt[:nw] + cnt[nw] + cnt[nw + 1]
        np.testing.assert_array_equal(rep, st_["boot_rep"].astype(np.int64))
        rn, rtp, rgd = rep[:, 0].astype(float), rep[:, 3].astype(float), (rep[:, 2] + mult @ extra[:nw] + extra[nw]).astype(float)
        pv = [t / a if a > 0 else None for t, a in zip(rtp, rn)]
        rv = [t / g if g > 0 else None for t, g in zip(rtp, rgd)]
        fv = [2 * (a * c) / (a + c) if a is not None and c is not None and a + c > 0 else None for a, c in zip(pv, rv)]
        for nm, vals in ((P, pv), (R, rv), (F, fv)):
            lo, hi = bs.interval(vals)
            assert (r[nm + "_lo"], r[nm + "_hi"]) == (_s(lo), _s(hi)), (j.vcf_file, nm)
        assert r["n_valid"] == str(sum(v is not None for v in fv)) and r["n_rep"] == str(prm["n_rep"])
        assert (r["window"], r["n_win"], r["seed"]) == (str(prm["window"]), str(nw), str(prm["seed"]))
        if r[F] != "NA" and r[F + "_lo"] != "NA":
            assert float(r[F + "_lo"]) <= float(r[F + "_hi"])


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_ci_tables_and_flag_off_tree(engine, tmp_path, gpus):
    from quasimodo_amd import workflow
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    boot = dict(n_rep=200, seed=7)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), bootstrap=boot, **kw)
    on = _tree(str(out))
    names = ["results/final_tables/caller_performance_ci.tsv", "results/final_tables/caller_performance_ci_pairs.tsv"]
    assert all(n in on for n in names)
    head, rows = _table(str(out / names[0]))
    assert head == ["caller", "mixture", "genomediff", "calleridentify", "TP", "Precision", "Precision_lo", "Precision_hi", "Recall", "Recall_lo",
                    "Recall_hi", "F1", "F1_lo", "F1_hi", "n_rep", "n_valid", "window", "n_win", "seed"]
    assert len(rows) == len(jobs) == 60
    if gpus == 1:
        off_dir = tmp_path / "off"                                  # without the flag: the same tree minus the new tables
        workflow.run_hcmv_variantcall(str(data), str(off_dir), engine=engine)
        assert _tree(str(off_dir)) == {k: v for k, v in on.items() if k not in names}
        sdir = tmp_path / "strata"                                  # the one-stratum set's table
        workflow.run_hcmv_variantcall(str(data), str(sdir), engine=engine, strata=[("all", [0], [I32MAX])])
        _, srows = _table(str(sdir / "results" / "final_tables" / "caller_performance_strata.tsv"))
        assert len(srows) == 3 * len(jobs)
        by = {id(j): srows[3 * i:3 * i + 3] for i, j in enumerate(jobs)}
        _check_ci_rows(jobs, rows, ("Precision", "Recall", "F1"), lambda j: by[id(j)])
        # the pairs: dF1 is the difference of the unrounded point F1s
        _, pairs = _table(str(out / names[1]))
        stats = {(r["caller"], r["mixture"]): j.stats for r, j in zip(rows, jobs)}
        assert pairs and all(p["mixture"][-4:] not in ("-1-0", "-0-1") for p in pairs)
        per = {}
        for r in rows:
            if not stats[(r["caller"], r["mixture"])].get("pure_strain"):
                per.setdefault(r["mixture"], []).append(r["caller"])
        assert len(pairs) == sum(len(c) * (len(c) - 1) // 2 for c in per.values())
        mult = bs.multiplicities(7, int(rows[0]["n_win"]), 200)
        for p in pairs:
            fa, fb = (_raw_f1(stats[(p[c], p["mixture"])]) for c in ("caller_a", "caller_b"))
            assert p["dF1"] == ("NA" if fa is None or fb is None else _s(fa - fb)), p
            d, lo, hi, nv = bs.pair_row(stats[(p["caller_a"], p["mixture"])], stats[(p["caller_b"], p["mixture"])], mult)
            assert (p["dF1_lo"], p["dF1_hi"], p["n_valid"]) == (_s(lo), _s(hi), str(nv))
    snaps = test_workflow_ci_tables_and_flag_off_tree.snaps
    snaps[gpus] = [on[n] for n in names]
    if len(snaps) == 2:                                             # the tables do not depend on the ranks: the draws are shared
        assert snaps[1] == snaps[2]


test_workflow_ci_tables_and_flag_off_tree.snaps = {}


def test_vareval_custom_family_and_cli(engine, tmp_path):
    """the custom family end to end: the counts against the text of the written files, the ci table against the strata table of
    the one-stratum set and against numpy replicates, and the CLI flag: the same table beside an otherwise unchanged tree"""
    import subprocess
    import sys
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_gpu_afprofile import _tree
    from test_gpu_truthside import _custom_keys
    root = os.path.dirname(os.path.dirname(GOLDEN))
    cases = [e for e in golden_cases() if e["family"] == "custom"]
    fam = os.path.join(GOLDEN, "custom")
    vcfs = [os.path.join(fam, e["vcf"]) for e in cases]
    snps = os.path.join(fam, cases[0]["truth"])
    labels = ["c%d" % k for k in range(len(vcfs))]
    boot = dict(n_rep=100, window=2048, seed=11)
    jobs = workflow.run_vareval(vcfs, snps, str(tmp_path / "wf"), labels=labels, engine=engine, bootstrap=boot)
    name = "results/final_tables/snpcall_benchmark_ci.txt"
    head, rows = _table(str(tmp_path / "wf" / name))
    assert head == ["caller", "genomediff", "calleridentify", "TP", "precision", "precision_lo", "precision_hi", "recall", "recall_lo", "recall_hi",
                    "f1", "f1_lo", "f1_hi", "n_rep", "n_valid", "window", "n_win", "seed"]
    assert [r["caller"] for r in rows] == labels
    _, whole = _table(str(tmp_path / "wf" / "results" / "final_tables" / "snpcall_benchmark.txt"))
    for r, w in zip(rows, whole):
        assert (r["genomediff"], r["calleridentify"], r["TP"]) == (w["genomediff"], w["calleridentify"], w["TP"])
        assert (r["n_rep"], r["window"], r["n_win"], r["seed"]) == ("100", "2048", "256", "11")
    # cnt against the text of the written files and the truth file
    acgt = (b"A", b"C", b"G", b"T")                                  # the rows the device holds a key for (302 rows, 300 such keys)
    genome = {k for k in _custom_keys(open(snps, "rb").read()) if k[1] in acgt and k[2] in acgt}
    assert len(genome) == 300
    mult = bs.multiplicities(11, 256, 100).astype(np.uint64)
    hit = False
    for j in jobs:
        kept = ts.snp_keys(open(j.filtered_out, "rb").read())
        cnt = j.stats["boot_cnt"]
        np.testing.assert_array_equal(cnt, text_cnt(j.filtered_out, j.tp_out or None, genome, kept, 2048, 256), err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["boot_rep"], restate_rep(cnt, mult), err_msg=j.vcf_file)
        assert cnt[:, 2].sum() == 300 and int(j.stats["boot_extra"].sum()) == 2      # 302 rows against 300 keys
        hit = hit or cnt[:256, 3].sum() > 0
    assert hit
    # the point and interval columns, against the strata table of the one-stratum set and numpy replicates
    workflow.run_vareval(vcfs, snps, str(tmp_path / "st"), labels=labels, engine=engine, strata=[("all", [0], [I32MAX])])
    _, srows = _table(str(tmp_path / "st" / "results" / "final_tables" / "snpcall_benchmark_strata.txt"))
    assert len(srows) == 3 * len(jobs) and [r["stratum"] for r in srows[:3]] == ["all", "outside", "nokey"]
    by = {id(j): srows[3 * i:3 * i + 3] for i, j in enumerate(jobs)}
    _check_ci_rows(jobs, rows, ("precision", "recall", "f1"), lambda j: by[id(j)])
    assert any(r["f1_lo"] != r["f1_hi"] for r in rows)
    # the CLI flag: the same table, and without it the same tree minus the table
    cmd = [sys.executable, os.path.join(root, "run_benchmark.py"), "vareval", "-v", ",".join(vcfs), "--snps", snps, "-l", ",".join(labels)]
    r = subprocess.run(cmd + ["-o", str(tmp_path / "on"), "--bootstrap", "100", "--bootstrap-window", "2048", "--bootstrap-seed", "11"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(cmd + ["-o", str(tmp_path / "off")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    on, off, wf = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off")), _tree(str(tmp_path / "wf"))
    assert off == {k: v for k, v in on.items() if k != name} and name in on
    assert on[name] == wf[name] and set(on) == set(wf)
    with pytest.raises(ValueError, match="larger window"):
        workflow.run_vareval(vcfs, snps, str(tmp_path / "small"), labels=labels, bootstrap=dict(n_rep=10, window=1))
