"""k-of-n caller consensus (qm_batch_votes, k_vote_truth / k_vote_keys / k_vote_runs) against a Python-set
restatement of the contract that works on the uploaded columns, never on the engine's outputs: member i calls key
pos << 4 | ref << 2 | alt iff one of its records is kept, has a comparable key and carries it.  Both the counts and the returned
(ukeys, umasks) are compared.  Ties to numbers that are already pinned: truth_regions and Engine.fp_overlap for n <= 5, T',
QM_S_TP_R and QM_S_FP_R for every n."""
import ctypes

import numpy as np
import pytest

from conftest import random_columns, random_truth

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_TP_R, S_FP_R, S_TRUTH = 3, 4, 7
F_PASS, F_IDDOT, F_NOKEY = 1, 2, 4
A, C, G, T = 0, 1, 2, 3
TOP = (1 << 28) - 1


def run_batch(engine, cols, tids, alleles=False):
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b


def truth_keys(truth):
    tp, tr, ta = (np.asarray(x, np.int64) for x in truth)
    ok = (tr >= 0) & (tr < 4) & (ta >= 0) & (ta < 4)
    return np.unique((tp[ok] << 4) | (tr[ok] << 2) | ta[ok])


def called(cols):
    """(the set of keys the VCF calls, its kept QM_F_NOKEY records) from the columns alone"""
    pos, ref, alt, _, fl = (np.asarray(x) for x in cols)
    p, r, a = pos.astype(np.int64), ref.astype(np.int64), alt.astype(np.int64)
    kept = (r >= 0) & (r < 4) & (a >= 0) & (a < 4) & ((fl & F_PASS) != 0)
    nokey = (fl & F_NOKEY) != 0
    key = (p << 4) | ((r & 3) << 2) | (a & 3)
    return set(key[kept & ~nokey].tolist()), int((kept & nokey).sum())


def restate(members, truth):
    """the vote tables of one group and its (ukeys, umasks), as Python sets see them"""
    tk = set(truth_keys(truth).tolist())
    mask, nokey = {}, 0
    for i, c in enumerate(members):
        keys, nk = called(c)
        nokey += nk
        for k in keys:
            mask[k] = mask.get(k, 0) | 1 << i
    tp, fp, ptp, pfp = [0] * 33, [0] * 33, [0] * 32, [0] * 32
    for k in tk:
        tp[bin(mask.get(k, 0)).count("1")] += 1
    for k, m in mask.items():
        c = bin(m).count("1")
        if k not in tk:
            fp[c] += 1
        if c == 1:
            (ptp if k in tk else pfp)[m.bit_length() - 1] += 1
    uk = sorted(k for k in mask if k not in tk)
    return {"tp_votes": tp, "fp_votes": fp, "private_tp": ptp, "private_fp": pfp, "nokey": nokey,
            "ukeys": uk, "umasks": [mask[k] for k in uk]}


def check_votes(b, groups, cols, truths_of_vcf, scalars=True):
    """every group of one qm_batch_votes against the restatement; returns the restated tables"""
    b.votes(groups)
    got = b.vote_counts()
    sc = b.scalars()
    out = []
    for g, ids in enumerate(groups):
        n = len(ids)
        want = restate([cols[v] for v in ids], truths_of_vcf[ids[0]])
        for name in ("tp_votes", "fp_votes", "private_tp", "private_fp"):
            assert got[name][g].tolist() == want[name], "%s of group %d" % (name, g)
        assert int(got["nokey"][g]) == want["nokey"], "nokey of group %d" % g
        uk, um = b.vote_keys(g)
        assert uk.tolist() == want["ukeys"], "ukeys of group %d" % g
        assert um.tolist() == want["umasks"], "umasks of group %d" % g
        tpv, fpv = got["tp_votes"][g].astype(np.int64), got["fp_votes"][g].astype(np.int64)
        cc = np.arange(33)
        if scalars:
            assert int(tpv.sum()) == sc[ids[0], S_TRUTH], "the tp_votes row sums to T'"
            assert int((cc * tpv).sum()) == int(sum(sc[v, S_TP_R] for v in ids)), "sum of c * tp_votes against the members' QM_S_TP_R"
            if want["nokey"] == 0:
                assert int((cc * fpv).sum()) == int(sum(sc[v, S_FP_R] for v in ids)), "sum of c * fp_votes against the members' QM_S_FP_R"
        assert not tpv[n + 1:].any() and not fpv[n + 1:].any() and fpv[0] == 0
        assert not got["private_tp"][g][n:].any() and not got["private_fp"][g][n:].any()
        out.append(want)
    return got, out


def _fp_key_sets(b, ids, cols):
    """the (pos, ref, alt) of the kept records outside the in-truth record mask, per member: what Engine.fp_overlap is given"""
    sets = []
    for v in ids:
        pos, ref, alt, _, fl = cols[v]
        sel = ((b.cls(v) & 1) != 0) & ~b.intruth_mask(v) & ((fl & F_NOKEY) == 0)
        sets.append((pos[sel], ref[sel], alt[sel]))
    return sets


def check_regions_tie(engine, b, ids, cols, got, g):
    """n <= 5: the vote histograms are the region tables of the truth-side view summed by popcount"""
    n = len(ids)
    reg = b.truth_regions([ids])[0]
    fpr = engine.fp_overlap(_fp_key_sets(b, ids, cols))
    for c in range(n + 1):
        slots = [m for m in range(1 << n) if bin(m).count("1") == c]
        assert int(got["tp_votes"][g][c]) == int(sum(reg[m] for m in slots)), "tp_votes[%d] against truth_regions" % c
        assert int(got["fp_votes"][g][c]) == int(sum(fpr[m] for m in slots if m)), "fp_votes[%d] against fp_overlap" % c


def _cols(recs):
    return tuple(np.array([r[k] for r in recs], dt) for k, dt in enumerate((np.int32, np.int32, np.int32, np.float32, np.uint8)))


def _share(cols_list, rng, L, n_shared, p=0.5):
    """the same keys put into several VCFs (appended: the VCF is no longer sorted unless it is sorted again)"""
    sp = rng.integers(1, L + 1, n_shared).astype(np.int32)
    sr = rng.integers(0, 4, n_shared).astype(np.int32)
    sa = rng.integers(0, 4, n_shared).astype(np.int32)
    out = []
    for c in cols_list:
        take = rng.random(n_shared) < p
        k = int(take.sum())
        add = (sp[take], sr[take], sa[take], np.full(k, 99, np.float32), np.full(k, F_PASS | F_IDDOT, np.uint8))
        out.append(tuple(np.concatenate([x, y]) for x, y in zip(c, add)))
    return out


def _sorted(c):
    o = np.argsort(c[0], kind="stable")
    return tuple(np.ascontiguousarray(x[o]) for x in c)


# ---- hand-derived literal case -----------------------------------------------------------------------------------------------
def test_hand_case(engine):
    """three members, keys at position 0 and 2^28 - 1, a key on two lines of one member, a member without a kept record"""
    truth = [(0, A, C), (10, A, C), (20, C, G), (TOP, A, G)]
    tid = engine.truth_load(*[np.array([t[k] for t in truth], np.int32) for k in range(3)])
    ok = F_PASS | F_IDDOT
    m0 = [(0, A, C, 50, ok), (10, A, C, 50, ok), (10, A, C, 60, ok), (15, G, T, 50, ok), (15, G, T, 50, ok), (TOP, T, C, 50, ok),
          (30, A, G, 50, ok | F_NOKEY)]
    m1 = [(10, A, C, 50, ok), (15, G, T, 50, ok), (0, T, G, 50, ok), (TOP, A, G, 50, ok), (20, C, G, 5, F_IDDOT)]
    m2 = [(20, C, G, 5, F_IDDOT), (40, A, T, 5, F_IDDOT)]          # nothing kept
    cols = [_cols(m0), _cols(m1), _cols(m2)]
    try:
        b = run_batch(engine, cols, [tid] * 3)
        b.truth_hits()
        b.votes([[0, 1, 2]])
        got = b.vote_counts()
        # truth keys: (0,A,C) m0; (10,A,C) m0 m1; (20,C,G) nobody; (TOP,A,G) m1
        assert got["tp_votes"][0].tolist() == [1, 2, 1] + [0] * 30
        assert got["private_tp"][0].tolist() == [1, 1] + [0] * 30
        # other keys: (0,T,G) m1; (15,G,T) m0 m1; (TOP,T,C) m0
        assert got["fp_votes"][0].tolist() == [0, 2, 1] + [0] * 30
        assert got["private_fp"][0].tolist() == [1, 1] + [0] * 30
        assert got["nokey"].tolist() == [1]
        uk, um = b.vote_keys(0)
        assert uk.tolist() == [0 << 4 | T << 2 | G, 15 << 4 | G << 2 | T, TOP << 4 | T << 2 | C]
        assert um.tolist() == [0b010, 0b011, 0b001]
        b.close()
    finally:
        engine.truth_release(tid)


# ---- group sizes, sorted / shuffled / mixed members ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(engine):
    """one batch of 33 VCFs of one truth set (weird = False: no kept NOKEY record), sorted, shuffled and in runs; VCF 32 sits in
    no group"""
    rng = np.random.default_rng(1412)
    L = 30_000
    truth = random_truth(rng, 1_500, L)
    tid = engine.truth_load(*truth)
    sizes = [int(x) for x in rng.integers(200, 2_500, 33)]
    sizes[7] = 0                                             # an empty member
    seams = {3: 16_385, 4: 16_384, 9: 1_024, 12: 3, 18: 1_025, 21: 1_023}   # cut to these below: a span of the record walk, a step of it
    for v, n in seams.items():
        sizes[v] = n
    cols = _share([random_columns(rng, n, L, truth, weird=False) for n in sizes], rng, L, 1_200, p=0.4)
    for v in range(33):
        if v % 3 == 0:
            cols[v] = _sorted(cols[v])
        elif v % 3 == 1:
            o = rng.permutation(len(cols[v][0]))
            cols[v] = tuple(np.ascontiguousarray(x[o]) for x in cols[v])
    cols[7] = tuple(np.zeros(0, dt) for dt in (np.int32, np.int32, np.int32, np.float32, np.uint8))
    for v, n in seams.items():                               # (members v % 3 == 0: sorted, and still sorted)
        cols[v] = tuple(np.ascontiguousarray(x[:n]) for x in cols[v])
    b = run_batch(engine, cols, [tid] * 33)
    b.truth_hits()
    yield b, cols, truth
    b.close()
    engine.truth_release(tid)


@pytest.mark.parametrize("n", [1, 2, 5, 6, 31, 32])
def test_group_sizes(engine, wide, n):
    b, cols, truth = wide
    ids = list(range(n))
    got, _ = check_votes(b, [ids], cols, [truth] * 33)
    if n <= 5:
        check_regions_tie(engine, b, ids, cols, got, 0)


def test_two_groups_on_one_truth_set_and_a_vcf_in_no_group(engine, wide):
    b, cols, truth = wide
    groups = [[9, 3, 4, 20, 1], [0, 31, 7], [12]]           # VCFs 2, 5, 6, ... and 32 in no group; member order is not VCF order
    got, _ = check_votes(b, groups, cols, [truth] * 33)
    check_regions_tie(engine, b, groups[0], cols, got, 0)
    check_regions_tie(engine, b, groups[1], cols, got, 1)


def test_reversed_members_give_equal_counts_and_bit_reversed_masks(wide):
    b, cols, truth = wide
    ids = [4, 5, 6, 7, 8, 9, 10]
    n = len(ids)
    b.votes([ids])
    c1, (k1, m1) = b.vote_counts(), b.vote_keys(0)
    b.votes([ids[::-1]])
    c2, (k2, m2) = b.vote_counts(), b.vote_keys(0)
    assert c1["tp_votes"].tolist() == c2["tp_votes"].tolist() and c1["fp_votes"].tolist() == c2["fp_votes"].tolist()
    assert c1["private_tp"][0][:n].tolist() == c2["private_tp"][0][:n][::-1].tolist()
    assert c1["private_fp"][0][:n].tolist() == c2["private_fp"][0][:n][::-1].tolist()
    assert k1.tolist() == k2.tolist()
    rev = [int(format(int(m), "0%db" % n)[::-1], 2) for m in m1]
    assert rev == m2.tolist()
    b.votes([ids])                                           # and the same call again: the same answer
    c3, (k3, m3) = b.vote_counts(), b.vote_keys(0)
    assert all(c1[x].tolist() == c3[x].tolist() for x in c1) and k1.tolist() == k3.tolist() and m1.tolist() == m3.tolist()


# ---- the last word of the hit bitmaps ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tn", [1, 33, 4097])
def test_last_word_masking(engine, tn):
    """T' of 1 / 33 / 4097 truth keys (p, A, C), p = 1 .. T'; three members hold the first and the last key, every other key,
    and nothing of the truth set"""
    pos = np.arange(1, tn + 1, dtype=np.int32)
    truth = (pos, np.zeros(tn, np.int32), np.ones(tn, np.int32))
    tid = engine.truth_load(*truth)
    ok = F_PASS | F_IDDOT
    ends = sorted({1, tn})
    m0 = _cols([(p, A, C, 40, ok) for p in ends])
    m1 = _cols([(int(p), A, C, 40, ok) for p in pos[::2]] + [(tn + 5, G, T, 40, ok)])
    m2 = _cols([(tn + 5, G, T, 40, ok), (tn + 6, G, T, 40, ok)])
    cols = [m0, m1, m2]
    try:
        b = run_batch(engine, cols, [tid] * 3)
        b.truth_hits()
        got, _ = check_votes(b, [[0, 1, 2]], cols, [truth] * 3)
        assert int(got["tp_votes"][0].sum()) == tn
        check_regions_tie(engine, b, [0, 1, 2], cols, got, 0)
        b.close()
    finally:
        engine.truth_release(tid)


# ---- long runs, duplicates, empty sides ----------------------------------------------------------------------------------------
def test_key_on_5000_lines_crosses_sort_tiles_and_workgroups(engine):
    """one non-truth key on 5 000 lines of member 0 and once in three others: its run of 5 003 sorted pairs spans three sort
    tiles of 2 048 and five run tiles of 1 024, with other keys in front of it and behind it"""
    rng = np.random.default_rng(5000)
    L = 4_000
    truth = random_truth(rng, 300, L)
    tid = engine.truth_load(*truth)
    ok = F_PASS | F_IDDOT
    hot = (2_000, G, T)
    assert (2_000 << 4 | G << 2 | T) not in set(truth_keys(truth).tolist())
    base = [random_columns(rng, n, L, truth, weird=False) for n in (900, 700, 500, 800, 600)]
    def add(c, times):
        extra = _cols([hot + (77, ok)] * times)
        m = tuple(np.concatenate([x, y]) for x, y in zip(c, extra))
        o = rng.permutation(len(m[0]))
        return tuple(np.ascontiguousarray(x[o]) for x in m)
    cols = [add(base[0], 5_000), add(base[1], 1), base[2], add(base[3], 1), add(base[4], 1)]
    try:
        b = run_batch(engine, cols, [tid] * 5)
        b.truth_hits()
        got, want = check_votes(b, [[0, 1, 2, 3, 4]], cols, [truth] * 5)
        i = want[0]["ukeys"].index(2_000 << 4 | G << 2 | T)
        assert want[0]["umasks"][i] == 0b11011
        check_regions_tie(engine, b, [0, 1, 2, 3, 4], cols, got, 0)
        b.close()
    finally:
        engine.truth_release(tid)


def test_groups_on_different_truth_sets_nokey_and_no_non_truth_key(engine):
    """group 0 on truth set 1 with weird records (kept NOKEY lines are counted and skipped, duplicates); group 1 on truth set 2
    whose members hold truth keys only: no pair at all"""
    rng = np.random.default_rng(77)
    L = 50_000
    t1, t2 = random_truth(rng, 3_000, L), random_truth(rng, 500, L)
    tid1, tid2 = engine.truth_load(*t1), engine.truth_load(*t2)
    ok = F_PASS | F_IDDOT
    g0 = [random_columns(rng, n, L, t1, sorted_=s, dup_frac=0.3) for n, s in ((3_000, True), (2_500, False), (1_800, True))]
    tk2 = truth_keys(t2)
    def only_truth(sel):
        k = tk2[sel]
        return _cols([(int(x >> 4), int(x >> 2 & 3), int(x & 3), 60, ok) for x in k])
    g1 = [only_truth(slice(0, None, 2)), only_truth(slice(0, None, 3))]
    cols = g0 + g1
    try:
        b = run_batch(engine, cols, [tid1] * 3 + [tid2] * 2)
        b.truth_hits()
        got, want = check_votes(b, [[0, 1, 2], [3, 4]], cols, [t1] * 3 + [t2] * 2)
        assert want[0]["nokey"] > 0 and want[1]["ukeys"] == [] and not got["fp_votes"][1].any()
        assert b.vote_keys(1)[0].shape == (0,)
        b.close()
    finally:
        engine.truth_release(tid1)
        engine.truth_release(tid2)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_by_code_and_the_batch_stays_usable(engine):
    from quasimodo_amd._lib import QmvtError
    rng = np.random.default_rng(9)
    L = 5_000
    t1, t2 = random_truth(rng, 200, L), random_truth(rng, 100, L)
    tid1, tid2 = engine.truth_load(*t1), engine.truth_load(*t2)
    cols = [random_columns(rng, 400, L, t1, weird=False) for _ in range(3)] + [random_columns(rng, 300, L, t2, weird=False)]
    tids = [tid1] * 3 + [tid2]
    def code(fn):
        with pytest.raises(QmvtError) as e:
            fn()
        return e.value.code
    try:
        b = engine.batch([len(c[0]) for c in cols], tids)
        for v, c in enumerate(cols):
            b.upload(v, *c)
        assert code(lambda: b.votes([[0, 1]])) == QM_E_STATE                 # nothing ran
        b.run()
        assert code(lambda: b.votes([[0, 1]])) == QM_E_STATE                 # not finished
        b.finish()
        assert code(lambda: b.votes([[0, 1]])) == QM_E_STATE                 # no truth_hits behind the run
        assert code(b.vote_counts) == QM_E_STATE
        b.truth_hits()
        assert code(lambda: b.votes([[]])) == QM_E_INVAL                     # a group of 0
        assert code(lambda: b.votes([[0] * 33])) == QM_E_INVAL               # more than 32 members
        assert code(lambda: b.votes([[0, 1], [1, 2]])) == QM_E_INVAL         # a VCF in two groups
        assert code(lambda: b.votes([[0, 0]])) == QM_E_INVAL                 # ... or twice in one
        assert code(lambda: b.votes([[0, 3]])) == QM_E_INVAL                 # members of different truth sets
        assert code(lambda: b.votes([[0, 4]])) == QM_E_INVAL                 # a VCF id out of range
        assert code(lambda: b.votes([[-1]])) == QM_E_INVAL
        check_votes(b, [[0, 1, 2], [3]], cols, [t1] * 3 + [t2])              # the batch is still usable
        assert code(lambda: b.vote_keys(2)) == QM_E_INVAL                    # no such group
        big = len(restate(cols[:3], t1)["ukeys"])
        k, m, n = np.zeros(big, np.uint32), np.zeros(big, np.uint32), ctypes.c_int64(0)
        assert b._L.qm_batch_get_vote_keys(b._h, 0, k.ctypes.data, m.ctypes.data, big - 1, ctypes.byref(n)) == QM_E_INVAL   # capacity too small
        assert n.value == big
        b.run()
        b.finish()
        assert code(b.vote_counts) == QM_E_STATE                             # the batch ran since
        assert code(lambda: b.vote_keys(0)) == QM_E_STATE
        b.truth_hits()
        check_votes(b, [[2, 0]], cols, [t1] * 3 + [t2])
        b.close()
        bx = run_batch(engine, cols[:2], tids[:2], alleles=True)             # an allele-extended batch
        assert code(lambda: bx.votes([[0, 1]])) == QM_E_STATE
        bx.close()
    finally:
        engine.truth_release(tid1)
        engine.truth_release(tid2)
