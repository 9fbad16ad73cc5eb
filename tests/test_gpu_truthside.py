"""The truth-side view (qm_batch_truth_hits / qm_batch_truth_regions, k_truth_hits / k_truth_regions) against
hand-derived literal cases and against a numpy restatement of the contract that works on the uploaded columns, not on the
engine's outputs: the hit bitmap is np.isin over the truth set's distinct keys, its popcount is QM_S_TP_R, and the distinct keys
of the kept records outside the record mask are QM_S_FP_R -- two numbers the oracle already pins.

End to end: `--truth-side` over the golden hcmv family (one and two ranks) and the quirks family against a Python-set restatement
of make_snp_vector that works on TEXT (quasimodo_amd.truthside.snp_keys / fn_text), never on the engine's packing."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, golden_cases, random_columns, random_truth

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
S_TP_R, S_FP_R, S_TRUTH = 3, 4, 7
F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8
A, C, G, T = 0, 1, 2, 3


def run_batch(engine, cols, tids, alleles=False):
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    return b


def truth_keys(truth):
    """sorted distinct pos << 4 | ref << 2 | alt of the single-base rows"""
    tp, tr, ta = (np.asarray(x, np.int64) for x in truth)
    ok = (tr >= 0) & (tr < 4) & (ta >= 0) & (ta < 4)
    return np.unique((tp[ok] << 4) | (tr[ok] << 2) | ta[ok])


def restate(cols, truth):
    """(hit bits over the truth keys, record mask, kept, FP_R) from the columns alone"""
    pos, ref, alt, _, fl = (np.asarray(x) for x in cols)
    tk = truth_keys(truth)
    p, r, a = pos.astype(np.int64), ref.astype(np.int64), alt.astype(np.int64)
    snp = (r >= 0) & (r < 4) & (a >= 0) & (a < 4)
    kept = snp & ((fl & F_PASS) != 0)
    nokey = (fl & F_NOKEY) != 0
    key = (p << 4) | ((r & 3) << 2) | (a & 3)
    cand = kept & ~nokey
    intruth = cand & np.isin(key, tk)
    hits = np.isin(tk, key[cand])
    fpk = key | (nokey.astype(np.int64) << 40)        # keyless records are keys of their own (oracle/qm_oracle.c)
    fp_r = len(np.unique(fpk[kept & ~intruth]))
    return hits, intruth, kept, fp_r


def check_batch(b, cols, truths_of_vcf):
    """every VCF of the batch against the restatement; returns the expected hit bits per VCF"""
    b.truth_hits()
    sc = b.scalars()
    want = []
    for v, c in enumerate(cols):
        hits, intruth, kept, fp_r = restate(c, truths_of_vcf[v])
        got_h, got_m = b.truth_hit_bits(v), b.intruth_mask(v)
        np.testing.assert_array_equal(got_h, hits, err_msg="hit bitmap of VCF %d" % v)
        np.testing.assert_array_equal(got_m, intruth, err_msg="record mask of VCF %d" % v)
        np.testing.assert_array_equal((b.cls(v) & 1) != 0, kept)
        assert len(hits) == sc[v, S_TRUTH]
        assert int(got_h.sum()) == sc[v, S_TP_R], "popcount(hits) against QM_S_TP_R, VCF %d" % v
        pos, ref, alt, _, fl = c
        key = (pos.astype(np.int64) << 4) | ((ref.astype(np.int64) & 3) << 2) | (alt.astype(np.int64) & 3) | \
              (((fl & F_NOKEY) != 0).astype(np.int64) << 40)
        sel = kept & ~got_m                              # the new record mask selects the FP keys
        assert len(np.unique(key[sel])) == sc[v, S_FP_R] == fp_r, "distinct kept keys outside the mask against QM_S_FP_R, VCF %d" % v
        want.append(hits)
    return want


def region_counts(bits):
    """[32] truth keys per membership mask over the group's hit vectors"""
    m = np.zeros(len(bits[0]), np.int64)
    for i, h in enumerate(bits):
        m |= h.astype(np.int64) << i
    return np.bincount(m, minlength=32)[:32]


# ---- hand-derived literal cases ------------------------------------------------------------------------------------------
def test_hand_cases(engine):
    top = (1 << 28) - 1
    #        pos  ref alt      sorted distinct keys: index 0 .. 4 in this order
    truth = [(10, A, C), (20, C, G), (30, G, T), (40, T, A), (top, A, G)]
    tid = engine.truth_load(*[np.array([t[k] for t in truth], np.int32) for k in range(3)])
    # pos ref alt qual flags                      in truth?  what it shows
    recs = [(10, A, C, 50, F_PASS),               # 1  key 0 hit only by a record with a non-'.' ID: no TP line, the bit is set
            (10, A, G, 50, F_PASS | F_IDDOT),     # 0  a truth position, another allele
            (20, C, G, 5, F_IDDOT),               # 0  key 1 hit only by a record that failed the filter: the bit is clear
            (30, G, T, 50, F_PASS | F_IDDOT | F_NOKEY),   # 0  key 2: a NOKEY record at a truth position: the bit is clear
            (40, T, A, 50, F_PASS | F_IDDOT),     # 1  key 3, twice
            (40, T, A, 60, F_PASS | F_IDDOT),     # 1
            (top, A, G, 50, F_PASS | F_IDDOT)]    # 1  key 4 at pos = 2^28 - 1
    cols = tuple(np.array([r[k] for r in recs], dt) for k, dt in enumerate((np.int32, np.int32, np.int32, np.float32, np.uint8)))
    try:
        b = run_batch(engine, [cols], [tid])
        b.truth_hits()
        assert b.truth_hit_bits(0).tolist() == [True, False, False, True, True]
        assert b.intruth_mask(0).tolist() == [True, False, False, False, True, True, True]
        sc = b.scalars()[0]
        assert (sc[S_TP_R], sc[S_FP_R], sc[S_TRUTH]) == (3, 2, 5)       # FP_R: (10, A, G) and the keyless record
        assert (b.cls(0) & 2).tolist() == [0, 0, 0, 0, 2, 2, 2]         # the first record is in the truth set and no TP line
        reg, uni = b.truth_regions([[0]], union=True)
        assert reg[0].tolist() == [2, 3] + [0] * 30
        assert uni[0].tolist() == [True, False, False, True, True]
        b.close()
    finally:
        engine.truth_release(tid)


@pytest.mark.parametrize("tn", [31, 32, 33])
def test_word_edge(engine, tn):
    """T' of 31 / 32 / 33: truth keys (p, A, C) for p = 1 .. T', the VCF holds the first and the last"""
    pos = np.arange(1, tn + 1, dtype=np.int32)
    tid = engine.truth_load(pos, np.zeros(tn, np.int32), np.ones(tn, np.int32))
    cols = (np.array([1, tn], np.int32), np.zeros(2, np.int32), np.ones(2, np.int32), np.full(2, 40, np.float32),
            np.full(2, F_PASS | F_IDDOT, np.uint8))
    try:
        b = run_batch(engine, [cols], [tid])
        b.truth_hits()
        assert b.truth_hit_bits(0).tolist() == [True] + [False] * (tn - 2) + [True]     # (raises on a bit at or beyond T')
        assert b.intruth_mask(0).tolist() == [True, True]
        reg = b.truth_regions([[0]])
        assert reg[0].tolist() == [tn - 2, 2] + [0] * 30
        b.close()
    finally:
        engine.truth_release(tid)


def test_empty_vcf_and_empty_truth_set(engine):
    t_pos = np.array([5, 9], np.int32)
    tid = engine.truth_load(t_pos, np.array([A, C], np.int32), np.array([C, T], np.int32))
    empty_tid = engine.truth_load(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    none = tuple(np.zeros(0, dt) for dt in (np.int32, np.int32, np.int32, np.float32, np.uint8))
    one = (np.array([5, 9], np.int32), np.array([A, C], np.int32), np.array([C, T], np.int32), np.full(2, 40, np.float32),
           np.full(2, F_PASS | F_IDDOT, np.uint8))
    try:
        b = run_batch(engine, [none, one, one], [tid, tid, empty_tid])
        b.truth_hits()
        assert b.truth_hit_bits(0).tolist() == [False, False] and b.intruth_mask(0).tolist() == []       # an empty VCF
        assert b.truth_hit_bits(1).tolist() == [True, True] and b.intruth_mask(1).tolist() == [True, True]
        assert b.truth_hit_bits(2).tolist() == [] and b.intruth_mask(2).tolist() == [False, False]       # an empty truth set
        reg = b.truth_regions([[0, 1], [2]])
        assert reg[0].tolist() == [0, 0, 2] + [0] * 29       # both keys hit by member 1 alone
        assert reg[1].tolist() == [0] * 32
        b.close()
    finally:
        engine.truth_release(tid)
        engine.truth_release(empty_tid)


# ---- random batches ------------------------------------------------------------------------------------------------------
def _runs(cols, rng, n_runs):
    """the records as n_runs ascending runs one behind the other (a VCF of several contigs)"""
    n = len(cols[0])
    grp = rng.integers(0, n_runs, n)
    o = np.lexsort((cols[0], grp))
    return tuple(np.ascontiguousarray(c[o]) for c in cols)


def _share(cols_list, rng, L, n_shared):
    """the same non-truth and truth-free keys put into several VCFs, so that every Venn region of the callers is populated"""
    sp = rng.integers(1, L + 1, n_shared).astype(np.int32)
    sr = rng.integers(0, 4, n_shared).astype(np.int32)
    sa = rng.integers(0, 4, n_shared).astype(np.int32)
    out = []
    for i, c in enumerate(cols_list):
        take = rng.random(n_shared) < 0.6
        k = int(take.sum())
        add = (sp[take], sr[take], sa[take], np.full(k, 99, np.float32), np.full(k, F_PASS | F_IDDOT, np.uint8))
        m = tuple(np.concatenate([x, y]) for x, y in zip(c, add))
        o = np.argsort(m[0], kind="stable")
        out.append(tuple(np.ascontiguousarray(x[o]) for x in m))
    return out


def test_random_sorted_shuffled_runs_two_truth_sets(engine):
    rng = np.random.default_rng(4801)
    L = 300_000
    t1, t2 = random_truth(rng, 20_000, L), random_truth(rng, 150_000, L)      # the second beyond the LDS bitmap's 131 072 keys
    tid1, tid2 = engine.truth_load(*t1), engine.truth_load(*t2)
    try:
        base = _share([random_columns(rng, n, L, t1) for n in (70_000, 50_000, 40_000, 30_000, 20_000)], rng, L, 5_000)
        perm = rng.permutation(len(base[1][0]))
        cols = [base[0], tuple(np.ascontiguousarray(c[perm]) for c in base[1]), _runs(base[2], rng, 24), base[3], base[4],
                random_columns(rng, 60_000, L, t2), random_columns(rng, 45_000, L, t2, sorted_=False)]
        cols += [random_columns(rng, n, L, t2) for n in (16_384, 16_385)]         # a VCF that ends with its span, and one record more
        tids = [tid1] * 5 + [tid2] * 4
        b = run_batch(engine, cols, tids)
        want = check_batch(b, cols, [t1] * 5 + [t2] * 4)
        groups = [[0, 1, 2, 3, 4], [3], [5, 6], [4, 0, 2]]
        reg, uni = b.truth_regions(groups, union=True)
        for g, ids in enumerate(groups):
            bits = [want[v] for v in ids]
            np.testing.assert_array_equal(reg[g], region_counts(bits), err_msg="group %r" % ids)
            assert reg[g].sum() == len(bits[0])                                   # the regions sum to T'
            assert reg[g][0] == len(bits[0]) - int(uni[g].sum())                  # missed by all = T' - popcount(union)
            assert not reg[g][1 << len(ids):].any()
            np.testing.assert_array_equal(uni[g], np.logical_or.reduce(bits))
        assert (reg[0][:32] > 0).all(), "five callers: every one of the 32 regions is populated"
        np.testing.assert_array_equal(b.truth_regions(groups), reg)               # without the union, the same counts
        # the callers' side of the Venn: distinct keys outside the truth set, selected with the record mask, through fp_overlap
        sets = []
        for v in range(5):
            p, r, a, _, fl = cols[v]
            sel = ((b.cls(v) & 1) != 0) & ~b.intruth_mask(v) & ((fl & F_NOKEY) == 0)
            sets.append((p[sel], r[sel], a[sel]))
        ov = engine.fp_overlap(sets)
        assert (ov[1:] > 0).all(), "the shared non-truth keys populate every region without the Genome bit"
        b.truth_hits()
        for v in range(len(cols)):
            np.testing.assert_array_equal(b.truth_hit_bits(v), want[v])           # two calls, the same bits
        b.close()
    finally:
        engine.truth_release(tid1)
        engine.truth_release(tid2)


@pytest.mark.parametrize("path", ["", "radix", "two_level", "partitions", "wide"])
def test_unsorted_paths(engine, monkeypatch, path):
    """"" = the library's own routing (a VCF below and one above the bucket path's smallest size), then every path forced"""
    monkeypatch.setenv("QM_UNSORTED_PATH", path)
    rng = np.random.default_rng(4802)
    L = 4_000_000 if path == "two_level" else 400_000
    truth = random_truth(rng, 30_000, L)
    tid = engine.truth_load(*truth)
    try:
        cols = [random_columns(rng, 120_000, L, truth, sorted_=False), random_columns(rng, 20_000, L, truth),
                random_columns(rng, 9_000, L, truth, sorted_=False)]
        b = run_batch(engine, cols, [tid] * 3)
        st = b.path_stats()
        print("path %r: %r" % (path, st))
        assert st["unsorted"] == 2
        check_batch(b, cols, [truth] * 3)
        b.close()
    finally:
        engine.truth_release(tid)


def test_hand_case_host_decided_lines(engine):
    """QM_F_TPLINE and a cleared QM_F_IDDOT (the host path's decisions): the TP-line bit and the truth key are different things"""
    tid = engine.truth_load(np.array([10, 20], np.int32), np.array([A, C], np.int32), np.array([C, G], np.int32))
    # pos ref alt flags                                in truth?
    recs = [(10, A, C, F_PASS),                      # 1  IDDOT cleared by the host path: no TP line, but the key is hit
            (15, A, G, F_PASS | F_IDDOT | F_TPLINE),  # 0  a TP line by the host's decision, its key is NOT in the truth set
            (20, C, G, F_PASS | F_IDDOT | F_TPLINE),  # 1  a TP line either way
            (25, G, T, F_PASS | F_TPLINE)]            # 0  TPLINE without a '.' ID, key not in the truth set
    cols = (np.array([r[0] for r in recs], np.int32), np.array([r[1] for r in recs], np.int32), np.array([r[2] for r in recs], np.int32),
            np.full(4, 50, np.float32), np.array([r[3] for r in recs], np.uint8))
    try:
        b = run_batch(engine, [cols], [tid])
        b.truth_hits()
        assert (b.cls(0) & 2).tolist() == [0, 2, 2, 2]
        assert b.truth_hit_bits(0).tolist() == [True, True]
        assert b.intruth_mask(0).tolist() == [True, False, True, False]
        sc = b.scalars()[0]
        assert (sc[S_TP_R], sc[S_FP_R]) == (2, 2)
        b.close()
    finally:
        engine.truth_release(tid)


# ---- argument and state rules ----------------------------------------------------------------------------------------------
def test_region_arguments(engine):
    from quasimodo_amd._lib import QmvtError
    rng = np.random.default_rng(4804)
    L = 20_000
    t1, t2 = random_truth(rng, 500, L), random_truth(rng, 600, L)
    tid1, tid2 = engine.truth_load(*t1), engine.truth_load(*t2)
    try:
        cols = [random_columns(rng, 1_000, L, t1) for _ in range(7)]
        b = run_batch(engine, cols, [tid1] * 6 + [tid2])
        b.truth_hits()
        for bad in ([[0, 1, 2, 3, 4, 5]], [[0, 6]], [[0, 7]], [[0, -1]], [[1, 2, 1]], [[0], []]):
            with pytest.raises(QmvtError) as e:
                b.truth_regions(bad, union=True)
            assert e.value.code == QM_E_INVAL, bad
        assert b.truth_regions([]).shape == (0, 32)
        b.close()
    finally:
        engine.truth_release(tid1)
        engine.truth_release(tid2)


def test_state_rules(engine):
    from quasimodo_amd._lib import QmvtError
    rng = np.random.default_rng(4805)
    L = 50_000
    truth = random_truth(rng, 3_000, L)
    tid = engine.truth_load(*truth)
    c1 = random_columns(rng, 8_000, L, truth)

    def refused(f, *a):
        with pytest.raises(QmvtError) as e:
            f(*a)
        assert e.value.code == QM_E_STATE

    b = engine.batch([8_000], [tid])
    b.upload(0, *c1)
    b.run()
    refused(b.truth_hits)                       # before finish
    b.finish()
    refused(b.truth_hit_bits, 0)                # nothing asked yet
    refused(b.intruth_mask, 0)
    refused(b.truth_regions, [[0]])
    before = b.device_bytes
    b.truth_hits()
    assert b.device_bytes > before              # qm_batch_device_bytes includes the new buffers once they exist
    check_batch(b, [c1], [truth])
    b.run()
    refused(b.truth_hit_bits, 0)                # the batch ran since
    refused(b.intruth_mask, 0)
    refused(b.truth_regions, [[0]])
    refused(b.truth_hits)
    b.finish()
    check_batch(b, [c1], [truth])
    b.truth_hits()
    reg_before = b.truth_regions([[0]])
    engine.truth_release(tid)
    refused(b.truth_hits)                       # a truth set of the batch was released
    b.close()
    assert reg_before[0].sum() == len(truth_keys(truth))
    # an allele-extended batch: refused with a message
    tid = engine.truth_load(*truth)
    try:
        bx = run_batch(engine, [c1], [tid], alleles=True)
        with pytest.raises(QmvtError) as e:
            bx.truth_hits()
        assert e.value.code == QM_E_STATE and "allele-extended" in str(e.value)
        bx.close()
    finally:
        engine.truth_release(tid)


# ---- end to end: files and tables ------------------------------------------------------------------------------------------
def _rd(path):
    with open(path, "rb") as fh:
        return fh.read()


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = _rd(os.path.join(d, f))
    return out


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_truth_side_against_the_text_restatement(engine, tmp_path, gpus):
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), truth_side=True, **kw)
    assert len(jobs) == 60
    snp = out / "results" / "snp"
    exp = os.path.join(GOLDEN, "hcmv", "expected")
    truth = {mix: _rd(os.path.join(GOLDEN, "hcmv", "input", "nucmer", "%s.maskrepeat.variants.vcf" % mix)) for mix in ("TM", "TA")}
    kept, n_fn = {}, 0
    for j in jobs:
        base = os.path.basename(j.vcf_file)[:-4]
        smp, _, c = base.split(".")[:3]
        fn = snp / "callers" / c / "fn" / (base + ".fn.vcf")
        if smp.endswith(("-1-0", "-0-1")):
            assert not fn.exists(), "pure-strain samples write no FN file"
            continue
        kept[(smp, c)] = ts.snp_keys(_rd(os.path.join(exp, c, base + ".filtered.vcf")))
        assert fn.read_bytes() == ts.fn_text(truth[smp[:2]], kept[(smp, c)]), str(fn)
        n_fn += 1
    assert n_fn == 36
    vc = ts.venn_callers(sorted({c for _, c in kept}))
    assert vc == ["lofreq", "varscan", "clc"]
    names = ts.set_names(vc)
    want = ["sample\tregion\tcount"]
    for smp in sorted({s for s, _ in kept}):
        sets = [ts.snp_keys(truth[smp[:2]])] + [kept[(smp, c)] for c in vc]
        count = {}
        for k in set().union(*sets):
            m = sum(1 << i for i, st in enumerate(sets) if k in st)
            count[m] = count.get(m, 0) + 1
        for m in range(1, 16):
            want.append("%s\t%s\t%d" % (smp, ts.region_name(m, names), count.get(m, 0)))
        missed = snp / "nucmer" / ("%s.missed_by_all.vcf" % smp)
        assert missed.read_bytes() == ts.fn_text(truth[smp[:2]], set().union(*sets[1:])), str(missed)
    table = (out / "results" / "final_tables" / "caller_snp_venn.tsv").read_text()
    assert table.split("\n") == want + [""]
    assert "TM-1-1\tGenome&LoFreq&VarScan2&CLC\t46" in want and "TM-1-1\tGenome\t3" in want
    new = _tree(str(out))
    test_workflow_truth_side_against_the_text_restatement.snaps[gpus] = {k: v for k, v in new.items() if k.endswith((".fn.vcf", ".missed_by_all.vcf", "caller_snp_venn.tsv"))}
    snaps = test_workflow_truth_side_against_the_text_restatement.snaps
    if len(snaps) == 2:
        assert snaps[1] == snaps[2], "two ranks write the same files and table as one"
    if gpus == 1:
        # without the flag (the feature's code present): every file of the output tree has the same bytes, and the flag adds
        # only callers/*/fn/*.fn.vcf, nucmer/*.missed_by_all.vcf and final_tables/caller_snp_venn.tsv
        off = tmp_path / "off"
        workflow.run_hcmv_variantcall(str(data), str(off), engine=engine)
        old = _tree(str(off))
        assert set(new) - set(old) == set(snaps[1]) and not set(old) - set(new)
        assert len(snaps[1]) == 36 + 6 + 1
        differing = [k for k in old if old[k] != new[k]]
        assert not differing, differing
        assert len(old) > 300 and "results/final_tables/caller_performance.tsv" in old


test_workflow_truth_side_against_the_text_restatement.snaps = {}


def _custom_keys(text):
    """custom_snp_benchmark.R:23-27 on text: columns 1-3 of the show-snps table, rows with a '.' allele dropped"""
    out = set()
    for ln in text.split(b"\n"):
        f = ln.rstrip(b"\r").split(b"\t")
        if ln and not ln.startswith(b"#") and len(f) >= 3 and f[1] != b"." and f[2] != b".":
            out.add((f[0], f[1], f[2]))
    return out


@pytest.mark.parametrize("case", [e for e in golden_cases() if e["family"] == "quirks"], ids=lambda e: e["mode"])
def test_quirks_family_matches_or_names_the_line(engine, tmp_path, case):
    """NOKEY lines: the lists either equal the text restatement or the call fails with an error that names the line"""
    import shutil
    from quasimodo_amd import truthside as ts
    from quasimodo_amd._lib import QmvtError
    from quasimodo_amd.extract import Job, extract_many
    fam = os.path.join(GOLDEN, "quirks")
    vcf = tmp_path / os.path.basename(case["vcf"])
    shutil.copyfile(os.path.join(fam, case["vcf"]), vcf)
    truth_path = os.path.join(fam, case["truth"])
    job = Job(str(vcf), truth_path, case["mode"], str(tmp_path / "o"), "q")
    try:
        extract_many([job], engine=engine, fn=True, groups=[[0]])
    except QmvtError as e:
        print("refused: %s" % e)
        m = re.search(r"line (\d+)", str(e))
        assert e.code == -8 and os.path.basename(str(vcf)) in str(e) and m, str(e)
        line = _rd(str(vcf)).split(b"\n")[int(m.group(1)) - 1]
        f = line.split(b"\t")
        assert re.fullmatch(rb"0|[1-9][0-9]*", f[1]) is None or int(f[1]) >= 1 << 28, "the named line has a canonical POS: %r" % line
        assert not os.path.exists(job.fn_out)
        return
    truth = _rd(truth_path)
    filtered = _rd(os.path.join(fam, case["expected"]["filtered"]))
    kept = ts.snp_keys(filtered)
    if case["mode"] == "hcmv":
        assert _rd(job.fn_out) == ts.fn_text(truth, kept)
        genome = ts.snp_keys(truth)
    else:
        genome = _custom_keys(truth)
        rows = [ln for ln in _rd(job.fn_out).split(b"\n") if ln and not ln.startswith(b"#")]
        assert rows == [ln for ln in truth.split(b"\n") if ln and not ln.startswith(b"#") and len(ln.split(b"\t")) >= 3
                        and tuple(ln.rstrip(b"\r").split(b"\t")[:3]) in genome - kept]
    assert job.stats["truth_regions"][:2].tolist() == [len(genome - kept), len(genome & kept)]
    assert job.stats["fp_regions"][1] == len(kept - genome)
