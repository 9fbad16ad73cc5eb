"""Mutation-context spectra (qm_batch_motifs, k_motif) against a numpy restatement of the contract, and against
hand-derived literal cases, so that the checker is not only the kernel written twice."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, golden_cases, random_columns, random_truth

pytestmark = pytest.mark.gpu

COLS = 98
QM_E_STATE = -6
F_PASS, F_IDDOT, F_NOKEY, F_TPLINE = 1, 2, 4, 8
_LUT = np.full(256, 4, np.int64)
for _k, _c in enumerate(b"ACGT"):
    _LUT[_c] = _k
    _LUT[_c + 32] = _k


def spectra(genome, pos, ref, alt, flags, cls):
    """[3][98] counts of one VCF: rows kept / TP / FP, columns as include/qmvt.h states them."""
    out = np.zeros((3, COLS), np.uint64)
    n = len(pos)
    if n == 0:
        return out
    g = _LUT[np.frombuffer(genome, np.uint8)]
    L = len(g)
    ref, alt = np.asarray(ref, np.int64), np.asarray(alt, np.int64)
    p = np.asarray(pos, np.int64)
    kept = (np.asarray(cls) & 1) != 0
    tp = (np.asarray(cls) & 2) != 0
    counted = kept & (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4)
    inside = (p >= 2) & (p + 1 <= L)
    pc = np.where(inside, p, 2)
    l, m, r = g[pc - 2], g[pc - 1], g[pc]
    ok = counted & inside & ((np.asarray(flags) & F_NOKEY) == 0) & (ref != alt) & (l < 4) & (r < 4)
    a, b = ref.copy(), alt.copy()
    fold = a % 2 == 0
    a = np.where(fold, 3 - a, a)
    b = np.where(fold, 3 - b, b)
    l2 = np.where(fold, 3 - r, l)
    r2 = np.where(fold, 3 - l, r)
    k = np.where(a == 1, np.where(b == 0, 0, b - 1), 3 + b)
    col = np.where(ok, 16 * k + 4 * l2 + r2, 96)
    mism = ok & (m != ref)
    for row, sel in ((1, counted & tp), (2, counted & ~tp)):
        out[row] = np.bincount(col[sel], minlength=COLS)[:COLS].astype(np.uint64)
        out[row, 97] = np.uint64(int((mism & sel).sum()))
    out[0] = out[1] + out[2]
    return out


def random_genome(rng, n, lower=0.05, nfrac=0.01):
    g = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].copy()
    low = rng.random(n) < lower
    g[low] += 32
    g[rng.random(n) < nfrac] = ord("N")
    return g.tobytes()


def run_batch(engine, cols, tids, gids, alleles=False):
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run()
    b.finish()
    b.motifs(gids)
    return b


def check_rows(b, cols, genomes, gids):
    got = b.motif_counts()
    sc = b.scalars()
    for v, c in enumerate(cols):
        if gids[v] < 0:
            assert not got[v].any()
            continue
        want = spectra(genomes[gids[v]], c[0], c[1], c[2], c[4], b.cls(v))
        np.testing.assert_array_equal(got[v], want, err_msg="VCF %d" % v)
        assert np.array_equal(got[v, 0], got[v, 1] + got[v, 2])
        if not b.alleles:
            assert int(got[v, 0, :97].sum()) == sc[v, 0]     # QM_S_NPASS
            assert int(got[v, 1, :97].sum()) == sc[v, 1]     # QM_S_TP_LINES
    return got


# ---- hand-derived cases -------------------------------------------------------------------------------------------
#            1234567890123 4
HAND_G = b"AGCTTGCANGTacg"
A, C, G, T = 0, 1, 2, 3
MOT = lambda name: __import__("quasimodo_amd.motifs", fromlist=["MOTIFS"]).MOTIFS.index(name)
# (pos, ref, alt, flags, expected column or None = not counted, TP row?)
HAND = [
    (2, G, T, 3, "CA G.T", False),      # AGC, G>T: reverse complement -> C>A in G.T
    (3, C, T, 3, "CT G.T", False),
    (4, T, C, 3, "TC C.T", False),
    (5, T, G, 3, "TG T.G", False),
    (6, G, A, 3, "CT G.A", True),       # TGC, G>A -> C>T in G.A; in the truth set
    (7, C, G, 3, "CG G.A", False),
    (8, A, C, 3, 96, False),            # right flank N
    (10, G, C, 3, 96, False),           # left flank N
    (11, T, A, 3, "TA G.A", False),     # lower-case right flank
    (12, A, G, 3, "TC G.A", False),     # lower case all round, folded
    (13, C, A, 3, "CA A.G", False),
    (1, A, C, 3, 96, False),            # p = 1: no left flank
    (14, G, A, 3, 96, False),           # p = len: no right flank
    (100, A, C, 3, 96, False),          # beyond the genome
    (3, C, C, 3, 96, False),            # REF == ALT
    (4, A, G, 3, "TC A.G", False),      # REF mismatch (genome T): motif from the VCF's REF, plus column 97
    (3, C, A, 3 | F_NOKEY, 96, False),  # no comparable key
    (5, T, C, 3 | F_TPLINE, "TC T.G", True),   # a TP line decided by the host path
    (3, C, A, F_IDDOT, None, False),    # fails the filter (QUAL / ID): not kept
    (3, 7, A, 3, None, False),          # not a single-base REF
]


def test_hand_cases(engine):
    gid = engine.genome_load(HAND_G)
    try:
        tid = engine.truth_load(np.array([6], np.int32), np.array([G], np.int32), np.array([A], np.int32))
        pos = np.array([h[0] for h in HAND], np.int32)
        ref = np.array([h[1] for h in HAND], np.int32)
        alt = np.array([h[2] for h in HAND], np.int32)
        fl = np.array([h[3] for h in HAND], np.uint8)
        qual = np.full(len(HAND), 50, np.float32)
        b = run_batch(engine, [(pos, ref, alt, qual, fl)], [tid], [gid])
        got = b.motif_counts()[0]
        want = np.zeros((3, COLS), np.uint64)
        for p, r, a, f, col, is_tp in HAND:
            if col is None:
                continue
            c = col if isinstance(col, int) else MOT(col)
            want[1 if is_tp else 2, c] += 1
        want[2, 97] = 1
        want[0] = want[1] + want[2]
        np.testing.assert_array_equal(got, want)
        assert MOT("CA G.T") == 0 * 16 + 2 * 4 + 3 and MOT("TG T.G") == 5 * 16 + 3 * 4 + 2
        np.testing.assert_array_equal(spectra(HAND_G, pos, ref, alt, fl, b.cls(0)), want)
        b.close()
    finally:
        engine.genome_release(gid)


# ---- random batches --------------------------------------------------------------------------------------------------
def _runs(cols, rng, n_runs):
    """the records as n_runs ascending runs one behind the other (a VCF of several contigs)"""
    n = len(cols[0])
    grp = rng.integers(0, n_runs, n)
    o = np.lexsort((cols[0], grp))
    return tuple(np.ascontiguousarray(c[o]) for c in cols)


def test_random_sorted_shuffled_and_runs(engine):
    rng = np.random.default_rng(9101)
    L = 300_000
    genome = random_genome(rng, L - 20)      # positions near the end fall outside
    gid = engine.genome_load(genome)
    truth = random_truth(rng, 20_000, L)
    tid = engine.truth_load(*truth)
    try:
        base = [random_columns(rng, n, L, truth) for n in (70_000, 50_000, 40_000)]
        perm = rng.permutation(len(base[1][0]))
        cols = [base[0], tuple(np.ascontiguousarray(c[perm]) for c in base[1]), _runs(base[2], rng, 24)]
        cols += [random_columns(rng, n, L, truth) for n in (16_384, 16_385)]      # a VCF that ends with its span, and one record more
        b = run_batch(engine, cols, [tid] * 5, [gid] * 5)
        first = check_rows(b, cols, {gid: genome}, [gid] * 5)
        b.motifs([gid] * 5)
        np.testing.assert_array_equal(b.motif_counts(), first)      # two calls, the same counts
        b.close()
    finally:
        engine.genome_release(gid)


@pytest.mark.parametrize("path", ["", "radix", "two_level", "partitions", "wide"])
def test_shuffled_under_every_forced_path(engine, monkeypatch, path):
    monkeypatch.setenv("QM_UNSORTED_PATH", path)
    rng = np.random.default_rng(9202)
    L = 4_000_000 if path == "two_level" else 400_000
    genome = random_genome(rng, L)
    gid = engine.genome_load(genome)
    truth = random_truth(rng, 30_000, L)
    tid = engine.truth_load(*truth)
    try:
        cols = [random_columns(rng, 120_000, L, truth, sorted_=False), random_columns(rng, 20_000, L, truth)]
        b = run_batch(engine, cols, [tid] * 2, [gid] * 2)
        check_rows(b, cols, {gid: genome}, [gid] * 2)
        b.close()
    finally:
        engine.genome_release(gid)


def test_allele_extended_batch_with_indels(engine):
    rng = np.random.default_rng(9303)
    L = 200_000
    genome = random_genome(rng, L)
    gid = engine.genome_load(genome)
    truth = random_truth(rng, 10_000, L)
    tid = engine.truth_load(*truth)
    try:
        cols = []
        for n, s in ((60_000, True), (30_000, False)):
            pos, ref, alt, qual, flags = random_columns(rng, n, L, truth, sorted_=s)
            ind = rng.random(n) < 0.3           # 2..13-base inline alleles (include/qmvt.h)
            ln = rng.integers(2, 8, n)
            code = (ln << 26) | rng.integers(0, 1 << 12, n)
            which = rng.random(n) < 0.5
            ref = np.where(ind & which, code, ref).astype(np.int32)
            alt = np.where(ind & ~which, code, alt).astype(np.int32)
            ok = (((ref >= 0) & (ref < 4)) | (ref >= (1 << 27))) & (((alt >= 0) & (alt < 4)) | (alt >= (1 << 27)))
            flags = ((flags & 0xfe) | (ok & (np.floor(qual) >= 20))).astype(np.uint8)
            cols.append((pos, ref, alt, qual, flags))
        b = run_batch(engine, cols, [tid] * 2, [gid] * 2, alleles=True)
        got = check_rows(b, cols, {gid: genome}, [gid] * 2)
        assert got[:, 0, :97].sum() > 0
        b.close()
    finally:
        engine.genome_release(gid)


def test_several_genomes_none_and_an_empty_vcf(engine):
    rng = np.random.default_rng(9404)
    L = 100_000
    genomes = [random_genome(rng, L), random_genome(rng, L // 2)]
    gids = [engine.genome_load(g) for g in genomes]
    truth = random_truth(rng, 5_000, L)
    tid = engine.truth_load(*truth)
    try:
        cols = [random_columns(rng, n, L, truth, sorted_=s) for n, s in ((30_000, True), (20_000, False), (0, True), (25_000, True), (10_000, True))]
        per = [gids[0], gids[1], gids[0], -1, gids[1]]
        b = run_batch(engine, cols, [tid] * 5, per)
        got = check_rows(b, cols, dict(zip(gids, genomes)), per)
        assert not got[2].any() and not got[3].any()
        b.close()
    finally:
        for g in gids:
            engine.genome_release(g)


def test_state_and_rerun(engine):
    from quasimodo_amd._lib import QmvtError
    rng = np.random.default_rng(9505)
    L = 50_000
    g1, g2 = random_genome(rng, L), random_genome(rng, L)
    gid = engine.genome_load(g1)
    truth = random_truth(rng, 3_000, L)
    tid = engine.truth_load(*truth)
    c1 = random_columns(rng, 8_000, L, truth)
    b = engine.batch([8_000], [tid])
    b.upload(0, *c1)
    b.run()
    with pytest.raises(QmvtError) as e:
        b.motifs([gid])                      # before finish
    assert e.value.code == QM_E_STATE
    b.finish()
    with pytest.raises(QmvtError) as e:
        b.motif_counts()                     # nothing asked yet
    assert e.value.code == QM_E_STATE
    b.motifs([gid])
    np.testing.assert_array_equal(b.motif_counts()[0], spectra(g1, c1[0], c1[1], c1[2], c1[4], b.cls(0)))
    b.run()
    with pytest.raises(QmvtError) as e:
        b.motif_counts()                     # ran since
    assert e.value.code == QM_E_STATE
    b.finish()
    engine.genome_release(gid)
    with pytest.raises(QmvtError) as e:
        b.motifs([gid])                      # released
    assert e.value.code == QM_E_STATE
    gid2 = engine.genome_load(g2)            # (may take the released slot)
    try:
        c2 = random_columns(rng, 8_000, L, truth)
        b.upload(0, *c2)
        b.run()
        b.finish()
        b.motifs([gid2])
        np.testing.assert_array_equal(b.motif_counts()[0], spectra(g2, c2[0], c2[1], c2[2], c2[4], b.cls(0)))
    finally:
        engine.genome_release(gid2)
    b.close()


# ---- files in, files out ---------------------------------------------------------------------------------------------
_CANON = re.compile(rb"^[1-9][0-9]*$")


def file_columns(path):
    """pos / ref / alt / flags of the data lines of a written VCF, as the R rule reads them"""
    pos, ref, alt, fl = [], [], [], []
    code = {b"A": 0, b"C": 1, b"G": 2, b"T": 3}
    last = 0
    with open(path, "rb") as fh:
        for ln in fh.read().split(b"\n"):
            if not ln or ln[:1] == b"#":
                continue
            c = ln.split(b"\t")
            canon = _CANON.match(c[1]) is not None
            p = int(c[1]) if canon else last
            last = p
            pos.append(p)
            ref.append(code.get(c[3], 9))
            alt.append(code.get(c[4], 9))
            fl.append(0 if canon else F_NOKEY)
    return [np.array(x, np.int64) for x in (pos, ref, alt, fl)]


def spectrum_of_files(genome, filtered, tp, fp):
    out = np.zeros((3, COLS), np.uint64)
    for row, path, cls in ((1, tp, 3), (2, fp, 1)):
        if path is None:
            continue
        pos, ref, alt, fl = file_columns(path)
        out[row] = spectra(genome, pos, ref, alt, fl, np.full(len(pos), cls, np.uint8))[row]
    out[0] = out[1] + out[2]
    pos, ref, alt, fl = file_columns(filtered)
    np.testing.assert_array_equal(spectra(genome, pos, ref, alt, fl, np.ones(len(pos), np.uint8))[0], out[0])
    return out


def _golden_jobs(root):
    from quasimodo_amd.extract import Job
    import shutil
    jobs = []
    for e in golden_cases():
        if e["family"] != "hcmv":
            continue
        fam = os.path.join(GOLDEN, "hcmv")
        d = os.path.join(root, os.path.dirname(e["vcf"]))
        os.makedirs(d, exist_ok=True)
        dst = os.path.join(d, os.path.basename(e["vcf"]))
        shutil.copyfile(os.path.join(fam, e["vcf"]), dst)
        jobs.append(Job(dst, os.path.join(fam, e["truth"]), "hcmv"))
    return jobs


def test_extract_many_genomes_match_the_written_files(engine, tmp_path):
    from quasimodo_amd.extract import extract_many, is_pure_strain
    rng = np.random.default_rng(9606)
    genome = random_genome(rng, 240_000, lower=0.1, nfrac=0.002)
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">seeded test genome\n" + b"\n".join(genome[i:i + 70] for i in range(0, len(genome), 70)) + b"\n")
    plain = _golden_jobs(str(tmp_path / "a"))
    extract_many(plain, engine=engine)
    withg = _golden_jobs(str(tmp_path / "b"))
    extract_many(withg, engine=engine, genomes=[str(fa)] * len(withg))
    seen_pure = seen_mixed = False
    for p, j in zip(plain, withg):
        for x, y in ((p.filtered_out, j.filtered_out), (p.fp_out, j.fp_out)) + (((p.tp_out, j.tp_out),) if p.tp_out else ()):
            assert open(x, "rb").read() == open(y, "rb").read()
        m = j.stats.pop("motifs")
        assert "motifs" not in p.stats
        for k in p.stats:
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        want = spectrum_of_files(genome, j.filtered_out, j.tp_out or None, j.fp_out)
        np.testing.assert_array_equal(m, want, err_msg=j.vcf_file)
        if is_pure_strain(j.vcf_file):
            seen_pure = True
            assert not m[1].any() and np.array_equal(m[0], m[2])
        else:
            seen_mixed = seen_mixed or m[1, :96].sum() > 0
    assert seen_pure and seen_mixed


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_tables(engine, tmp_path, gpus):
    from quasimodo_amd import workflow
    from quasimodo_amd.motifs import MOTIFS
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    rng = np.random.default_rng(9707)
    gm, ga = random_genome(rng, 236_000), random_genome(rng, 231_000)
    fm, fa = tmp_path / "merlin.fa", tmp_path / "ad169.fa"
    fm.write_bytes(b">Merlin\n" + gm + b"\n")
    fa.write_bytes(b">AD169\n" + ga + b"\n")
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), mutation_context={"TM": str(fm), "TA": str(fa)}, **kw)
    tables = out / "results" / "final_tables"
    callers = sorted({os.path.basename(j.vcf_file).split(".")[2] for j in jobs})
    for mix, genome in (("TM", gm), ("TA", ga)):
        for c in callers:
            lines = (tables / ("%s.%s.mutationcontext.tsv" % (mix, c))).read_text().splitlines()
            head = lines[0].split("\t")
            assert head[:3] == ["motif", "alteration", "context"] and [ln.split("\t")[0] for ln in lines[1:]] == list(MOTIFS)
            col = {h: [int(ln.split("\t")[k]) for ln in lines[1:]] for k, h in enumerate(head) if k >= 3}
            for j in jobs:
                smp, _, cc = os.path.basename(j.vcf_file).split(".")[:3]
                if cc != c or smp[:2] != mix or smp.endswith("-1-0"):
                    continue
                want = spectrum_of_files(genome, j.filtered_out, j.tp_out or None, j.fp_out)
                if smp.endswith("-0-1"):
                    assert col["unmixed " + smp] == [int(x) for x in want[0, :96]]
                else:
                    assert col[smp] == [int(x) for x in want[0, :96]]
                    assert col[smp + " (TP)"] == [int(x) for x in want[1, :96]]
                    assert col[smp + " (FP)"] == [int(x) for x in want[2, :96]]
    snap = {p.name: p.read_bytes() for p in tables.glob("*.mutationcontext.tsv")}
    assert len(snap) == 2 * len(callers)
    test_workflow_tables.snaps[gpus] = snap
    if len(test_workflow_tables.snaps) == 2:
        assert test_workflow_tables.snaps[1] == test_workflow_tables.snaps[2]


test_workflow_tables.snaps = {}
