"""Allele-frequency profiles (qm_batch_upload_af, qm_batch_af_profile, k_af_profile) against a numpy restatement
of the contract tied to the batch's class masks, and against hand-derived literal cells, so that the checker is not only the
kernel written twice."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, golden_cases, random_columns, random_truth

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
NO_AF, OUTSIDE, N_GRID = 0, 1, 2
F_PASS, F_IDDOT = 1, 2
NAN = np.float32(np.nan)


def restate(pos, ref, alt, af, cls, window, n_pos, n_af):
    """(grid [2][n_af][n_pos], extra [2][3], counted [2]) of one VCF as include/qmvt.h states them; class 0 = TP, 1 = FP"""
    grid = np.zeros((2, n_af, n_pos), np.uint64)
    extra = np.zeros((2, 3), np.uint64)
    pos, ref, alt = (np.asarray(x, np.int64) for x in (pos, ref, alt))
    af = np.asarray(af, np.float32)
    kept, tp = (np.asarray(cls) & 1) != 0, (np.asarray(cls) & 2) != 0
    counted = kept & (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4)
    n = [0, 0]
    for c, sel in ((0, counted & tp), (1, counted & ~tp)):
        f, p = af[sel], pos[sel]
        n[c] = int(sel.sum())
        nan = np.isnan(f)
        pb = (p - 1) // window
        with np.errstate(invalid="ignore"):
            out = ~nan & ((f < 0) | (f > 1) | (p < 1) | (pb >= n_pos))
        ing = ~nan & ~out
        a = np.minimum(n_af - 1, (f[ing] * np.float32(n_af)).astype(np.int64))     # ONE float32 multiply
        np.add.at(grid[c], (a, pb[ing]), 1)
        extra[c] = [nan.sum(), out.sum(), ing.sum()]
    return grid, extra, n


def make_batch(engine, cols, afs, tids, alleles=False):
    """afs[v] None: the VCF's frequencies are not uploaded"""
    b = engine.batch([len(c[0]) for c in cols], tids, alleles=alleles)
    for v, c in enumerate(cols):
        b.upload(v, *c)
        if afs[v] is not None:
            b.upload_af(v, afs[v])
    b.run()
    b.finish()
    return b


def check(b, cols, afs, window, n_pos, n_af):
    b.af_profile(window, n_pos, n_af)
    grid, extra = b.af_profile_counts()
    assert grid.shape == (len(cols), 2, n_af, n_pos) and extra.shape == (len(cols), 2, 3)
    sc = b.scalars()
    for v, c in enumerate(cols):
        if afs[v] is None:
            assert not grid[v].any() and not extra[v].any(), "VCF %d has no frequencies" % v
            continue
        wg, we, n = restate(c[0], c[1], c[2], afs[v], b.cls(v), window, n_pos, n_af)
        np.testing.assert_array_equal(grid[v], wg, err_msg="VCF %d grid" % v)
        np.testing.assert_array_equal(extra[v], we, err_msg="VCF %d extra" % v)
        for k in (0, 1):
            assert int(grid[v, k].sum()) == int(extra[v, k, N_GRID]) and int(extra[v, k].sum()) == n[k]
        if not b.alleles:
            assert int(extra[v, 0].sum()) == sc[v, 1]                                 # QM_S_TP_LINES
            assert int(extra[v].sum()) == sc[v, 0]                                    # QM_S_NPASS
    return grid, extra


def random_af(rng, n):
    """uniform frequencies with the edges and the oddities mixed in"""
    af = rng.random(n).astype(np.float32)
    k = rng.random(n)
    af = np.where(k < 0.10, (rng.integers(0, 21, n) / 20).astype(np.float32), af)      # bin edges k / 20, 1.0 among them
    af = np.where((k >= 0.10) & (k < 0.15), NAN, af)
    af = np.where((k >= 0.15) & (k < 0.18), np.float32(1.5), af)
    af = np.where((k >= 0.18) & (k < 0.20), np.float32(-0.25), af)
    af = np.where((k >= 0.20) & (k < 0.21), np.float32(-0.0), af)
    af = np.where((k >= 0.21) & (k < 0.22), np.nextafter(np.float32(1), np.float32(2)), af)
    af = np.where((k >= 0.22) & (k < 0.23), np.float32(np.inf), af)
    return np.ascontiguousarray(af, np.float32)


# ---- hand-derived cells ---------------------------------------------------------------------------------------------------
A, C, G, T = 0, 1, 2, 3
W, NP, NA = 100, 4, 20
K = F_PASS | F_IDDOT
# (pos, ref, alt, flags, af, where it must land: ("TP" | "FP", a, p), "no_af", "outside" or None = counted nowhere)
HAND = [
    (0, A, C, K, np.float32(0.5), "outside"),                            # pos < 1
    (0, A, C, K, NAN, "no_af"),                                          # NaN comes first
    (1, A, C, K, np.float32(-0.0), ("FP", 0, 0)),                        # -0.0 is not < 0
    (W, A, G, K, np.float32(0.0), ("FP", 0, 0)),                         # pos = window: still bin 0
    (W + 1, C, T, K, np.float32(1.0), ("FP", NA - 1, 1)),                # pos = window + 1: bin 1; af = 1.0: the last bin, closed
    (150, G, A, K, NAN, "no_af"),
    (160, G, A, K, np.float32(7 / 20), ("FP", 7, 1)),                    # float32(0.35) * 20 rounds to 7.0
    (170, G, T, K, np.float32(3 / 20), ("FP", 3, 1)),
    (200, T, A, K, np.float32(0.5), ("TP", 10, 1)),                      # the truth key
    (210, T, A, F_IDDOT, np.float32(0.5), None),                         # fails the filter: not kept
    (220, 7, A, K, np.float32(0.5), None),                               # not a single-base REF
    (230, C, C + 4, K, np.float32(0.5), None),                           # not a single-base ALT
    (NP * W, C, A, K, np.float32(19 / 20), ("FP", 19, NP - 1)),          # the last position of the last bin
    (NP * W, C, G, K, np.nextafter(np.float32(1), np.float32(2)), "outside"),   # af > 1 by one ulp
    (NP * W + 1, C, A, K, np.float32(0.5), "outside"),                   # the first position beyond the grid
    (NP * W + 1, C, G, K, np.float32(-0.25), "outside"),
]


def test_hand_cases(engine):
    tid = engine.truth_load(np.array([200], np.int32), np.array([T], np.int32), np.array([A], np.int32))
    pos = np.array([h[0] for h in HAND], np.int32)
    ref = np.array([h[1] for h in HAND], np.int32)
    alt = np.array([h[2] for h in HAND], np.int32)
    fl = np.array([h[3] for h in HAND], np.uint8)
    af = np.array([h[4] for h in HAND], np.float32)
    qual = np.full(len(HAND), 50, np.float32)
    b = make_batch(engine, [(pos, ref, alt, qual, fl)], [af], [tid])
    b.af_profile(W, NP, NA)
    grid, extra = b.af_profile_counts()
    wg = np.zeros((2, NA, NP), np.uint64)
    we = np.zeros((2, 3), np.uint64)
    for h in HAND:
        where = h[5]
        if where is None:
            continue
        if where == "no_af":
            we[1, NO_AF] += 1
        elif where == "outside":
            we[1, OUTSIDE] += 1
        else:
            c = 0 if where[0] == "TP" else 1
            wg[c, where[1], where[2]] += 1
            we[c, N_GRID] += 1
    np.testing.assert_array_equal(grid[0], wg)
    np.testing.assert_array_equal(extra[0], we)
    assert we.tolist() == [[0, 0, 1], [2, 4, 6]]
    rg, re_, _ = restate(pos, ref, alt, af, b.cls(0), W, NP, NA)                       # the restatement agrees with the literals
    np.testing.assert_array_equal(rg, wg)
    np.testing.assert_array_equal(re_, we)
    b.close()


# ---- shapes: VCFs smaller than a workgroup's share, several per workgroup, one without frequencies ------------------------
SIZES = (0, 1, 3, 255, 256, 257, 1025, 3000, 1023, 1024, 16384, 16385)   # 1023 .. 1025: a step of the span walk; 16 384: a span
BINS = [(1, 1, 1), (1000, 256, 20), (1 << 27, 128, 64)]          # (window, n_pos_bins, n_af_bins); 128 x 64 = the 8 192 limit


def _shape_cols(rng, truth, L, sorted_):
    cols, afs = [], []
    for v, n in enumerate(SIZES):
        c = list(random_columns(rng, n, L, truth, sorted_=sorted_ or v % 2 == 0))
        if n >= 255:   # positions at the far edges of what a column may hold, and at the edges of the 2^27 window
            far = np.array([1, (1 << 27), (1 << 27) + 1, (1 << 28) - 1, 1000, 1001, 256_000, 256_001], np.int32)
            c[0][-len(far):] = far
            if sorted_ or v % 2 == 0:
                o = np.argsort(c[0], kind="stable")
                c = [x[o] for x in c]
        cols.append(tuple(np.ascontiguousarray(x) for x in c))
        afs.append(random_af(rng, n))
    afs[5] = None                                                   # 257 records without frequencies between two VCFs that have them
    return cols, afs


@pytest.mark.parametrize("sorted_", [True, False])
def test_shapes_in_one_batch(engine, sorted_):
    rng = np.random.default_rng(1101 + sorted_)
    L = 300_000
    truth = random_truth(rng, 3_000, L)
    tid = engine.truth_load(*truth)
    cols, afs = _shape_cols(rng, truth, L, sorted_)
    b = make_batch(engine, cols, afs, [tid] * len(cols))
    assert sorted_ or (b.scalars()[:, 5] == 0).any()               # QM_S_SORTED: an unsorted path was taken
    total = 0
    for window, n_pos, n_af in BINS:                                # repeated with other bin counts: the output regrows
        grid, extra = check(b, cols, afs, window, n_pos, n_af)
        total += int(grid.sum())
    assert total > 1000
    b.close()


def test_allele_extended_batch(engine):
    rng = np.random.default_rng(1202)
    L = 200_000
    truth = random_truth(rng, 2_000, L)
    tid = engine.truth_load(*truth)
    cols, afs = [], []
    for n, s in ((2_500, True), (1_300, False)):
        pos, ref, alt, qual, flags = random_columns(rng, n, L, truth, sorted_=s)
        ind = rng.random(n) < 0.3                                  # 2..13-base inline alleles (include/qmvt.h)
        code = (rng.integers(2, 8, n) << 26) | rng.integers(0, 1 << 12, n)
        which = rng.random(n) < 0.5
        ref = np.where(ind & which, code, ref).astype(np.int32)
        alt = np.where(ind & ~which, code, alt).astype(np.int32)
        ok = (((ref >= 0) & (ref < 4)) | (ref >= (1 << 27))) & (((alt >= 0) & (alt < 4)) | (alt >= (1 << 27)))
        flags = ((flags & 0xfe) | (ok & (np.floor(qual) >= 20))).astype(np.uint8)
        cols.append((pos, ref, alt, qual, flags))
        afs.append(random_af(rng, n))
    b = make_batch(engine, cols, afs, [tid] * 2, alleles=True)
    grid, extra = check(b, cols, afs, 1000, 256, 20)
    kept_indels = sum(int((((b.cls(v) & 1) != 0) & ((cols[v][1] >= 4) | (cols[v][2] >= 4))).sum()) for v in range(2))
    assert kept_indels > 0 and grid.sum() > 0                       # kept records with longer alleles exist and are counted nowhere
    b.close()


def test_division_is_exact_at_the_bin_edges(engine):
    """p = (pos - 1) / window for every window: positions one below, at and one above multiples of the window, up to 2^28 - 1"""
    tid = engine.truth_load(np.array([9], np.int32), np.array([T], np.int32), np.array([T], np.int32))     # matches no record
    windows = [1, 2, 3, 7, 1000, 1024, 65_537, (1 << 27) - 1, 1 << 27, (1 << 27) + 1, (1 << 28) - 1]
    n_pos = 8192
    ps = set()
    for w in windows:
        for q in (0, 1, 2, 3, 5, n_pos - 1, n_pos, n_pos + 1, ((1 << 28) - 1) // w):
            for d in (-1, 0, 1, 2):
                ps.add(q * w + d)
    pos = np.array(sorted(p for p in ps if 0 <= p < (1 << 28)), np.int32)
    n = len(pos)
    cols = [(pos, np.zeros(n, np.int32), np.ones(n, np.int32), np.full(n, 50, np.float32), np.full(n, K, np.uint8))]
    afs = [np.full(n, 0.5, np.float32)]
    b = make_batch(engine, cols, afs, [tid])
    for w in windows:
        grid, extra = check(b, cols, afs, w, n_pos, 1)
        assert int(extra[0, 1].sum()) == n and extra[0, 1, N_GRID] > 0
    b.close()


def test_collision_in_one_cell(engine):
    tid = engine.truth_load(np.array([5000], np.int32), np.array([T], np.int32), np.array([G], np.int32))   # another allele: every record is FP
    n = 70_000
    cols = [(np.full(n, 5000, np.int32), np.zeros(n, np.int32), np.ones(n, np.int32), np.full(n, 50, np.float32), np.full(n, K, np.uint8))]
    afs = [np.full(n, 0.25, np.float32)]
    b = make_batch(engine, cols, afs, [tid])
    b.af_profile(1024, 256, 20)
    grid, extra = b.af_profile_counts()
    assert int(grid[0, 1, 5, 4]) == n and int(grid.sum()) == n and extra[0].tolist() == [[0, 0, 0], [0, 0, n]]
    b.close()


def test_bin_limits(engine):
    from quasimodo_amd._lib import QmvtError
    tid = engine.truth_load(np.array([5], np.int32), np.array([A], np.int32), np.array([C], np.int32))
    cols = [(np.array([5], np.int32), np.array([A], np.int32), np.array([C], np.int32), np.array([50], np.float32), np.array([K], np.uint8))]
    b = make_batch(engine, cols, [np.array([0.5], np.float32)], [tid])
    for window, n_pos, n_af in ((1024, 8193, 1), (1024, 1, 8193), (1024, 4097, 2), (0, 4, 4), (1 << 28, 4, 4), (1024, 0, 4), (1024, 4, 0), (1024, -1, -1)):
        with pytest.raises(QmvtError) as e:
            b.af_profile(window, n_pos, n_af)
        assert e.value.code == QM_E_INVAL
    b.af_profile(1024, 4096, 2)                                     # exactly 8 192 cells
    grid, extra = b.af_profile_counts()
    assert int(grid[0, 0, 1, 0]) == 1 and int(grid.sum()) == 1
    b.close()


def test_state_rules_and_device_bytes(engine):
    from quasimodo_amd._lib import QmvtError
    rng = np.random.default_rng(1303)
    L = 50_000
    truth = random_truth(rng, 1_000, L)
    tid = engine.truth_load(*truth)
    c1 = random_columns(rng, 2_000, L, truth)
    a1 = random_af(rng, 2_000)
    plain = engine.batch([2_000], [tid])                             # never uploads frequencies
    plain.upload(0, *c1)
    plain.run()
    plain.finish()
    b = engine.batch([2_000], [tid])
    b.upload(0, *c1)
    b.run()
    with pytest.raises(QmvtError) as e:
        b.af_profile()                                               # before finish
    assert e.value.code == QM_E_STATE
    b.finish()
    assert b.device_bytes == plain.device_bytes
    with pytest.raises(QmvtError) as e:
        b.af_profile_counts()                                        # no profile was made
    assert e.value.code == QM_E_STATE
    b.upload_af(0, a1)
    assert b.device_bytes >= plain.device_bytes + 4 * 2_000          # the column is counted where it grows
    check(b, [c1], [a1], 1024, 256, 20)                              # (the upload of the frequencies leaves the finished run as it is)
    first = b.af_profile_counts()
    check(b, [c1], [a1], 500, 128, 64)                               # other bin counts: the output regrows
    check(b, [c1], [a1], 1024, 256, 20)
    for x, y in zip(first, b.af_profile_counts()):
        np.testing.assert_array_equal(x, y)
    b.run()
    with pytest.raises(QmvtError) as e:
        b.af_profile_counts()                                        # ran since
    assert e.value.code == QM_E_STATE
    b.finish()
    check(b, [c1], [a1], 1024, 256, 20)
    c2 = random_columns(rng, 2_000, L, truth)
    b.upload(0, *c2)                                                 # new columns: the frequencies no longer belong to them
    b.run()
    b.finish()
    check(b, [c2], [None], 1024, 256, 20)
    a2 = random_af(rng, 2_000)
    b.upload_af(0, a2)
    check(b, [c2], [a2], 1024, 256, 20)
    with pytest.raises(ValueError):
        b.upload_af(0, a2[:10])
    before = plain.device_bytes
    plain.run()
    plain.finish()
    assert plain.device_bytes == before
    plain.close()
    b.close()


# ---- files in, files out -----------------------------------------------------------------------------------------------
R_PATTERN = re.compile(rb".*AF=([01]\.[0-9]+);.*$")
PAR = dict(window=1024, n_pos_bins=256, n_af_bins=20)


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


def file_profile(tp, fp, window, n_pos, n_af):
    """grids and extras from the WRITTEN tp / fp files: their scanned columns through the restatement"""
    from quasimodo_amd.vcfio import scan_vcf
    grid = np.zeros((2, n_af, n_pos), np.uint64)
    extra = np.zeros((2, 3), np.uint64)
    for c, path, cls in ((0, tp, 3), (1, fp, 1)):
        if not path:
            continue
        sv = scan_vcf(open(path, "rb").read())
        af, _ = sv.scan_af()
        g, e, _ = restate(sv.pos, sv.ref, sv.alt, af, np.full(sv.n_records, cls, np.uint8), window, n_pos, n_af)
        grid[c], extra[c] = g[c], e[c]
    return grid, extra


def points_text(tp, fp):
    """the data frame R plots, from the text of the written files: rbind(fp_snp, tp_snp)"""
    out = [b"Position\tFrequency\ttype"]
    for path, name in ((fp, b"FP"), (tp, b"TP")):
        if not path:
            continue
        for ln in open(path, "rb").read().split(b"\n"):
            if not ln or ln[:1] == b"#":
                continue
            c = ln.split(b"\t")
            if c[3] not in (b"A", b"C", b"G", b"T") or c[4] not in (b"A", b"C", b"G", b"T"):
                continue
            m = R_PATTERN.match(c[7]) if len(c) >= 8 else None
            out.append(b"\t".join([c[1], m.group(1) if m else b"NA", name]))
    return b"\n".join(out) + b"\n"


def test_extract_many_profile_matches_the_written_files(engine, tmp_path):
    from quasimodo_amd.extract import extract_many, is_pure_strain
    plain = _golden_jobs(str(tmp_path / "a"))
    extract_many(plain, engine=engine)
    prof = _golden_jobs(str(tmp_path / "b"))
    want = [0 if os.path.basename(j.vcf_file).split(".")[0].endswith("-1-0") else 1 for j in prof]
    points = [str(tmp_path / "points" / (os.path.basename(j.vcf_file)[:-4] + ".points.tsv")) if w else None for j, w in zip(prof, want)]
    extract_many(prof, engine=engine, profile=dict(PAR, want=want, points=points))
    seen_pure = seen_tp = False
    assert 0 in want and 1 in want
    for p, j, w, pt in zip(plain, prof, want, points):
        for x, y in ((p.filtered_out, j.filtered_out), (p.fp_out, j.fp_out)) + (((p.tp_out, j.tp_out),) if p.tp_out else ()):
            assert open(x, "rb").read() == open(y, "rb").read()
        if not w:
            assert "af_grid" not in j.stats and "af_extra" not in j.stats
            continue
        grid, extra = j.stats.pop("af_grid"), j.stats.pop("af_extra")
        for k in p.stats:
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        wg, we = file_profile(j.tp_out or None, j.fp_out, PAR["window"], PAR["n_pos_bins"], PAR["n_af_bins"])
        np.testing.assert_array_equal(grid, wg, err_msg=j.vcf_file)
        np.testing.assert_array_equal(extra, we, err_msg=j.vcf_file)
        assert int(extra[0].sum()) == j.stats["tp_lines"] and int(extra[1].sum()) == j.stats["fp_lines"]
        text = open(pt, "rb").read()
        assert text == points_text(j.tp_out or None, j.fp_out), pt
        if is_pure_strain(j.vcf_file):
            seen_pure = True
            assert not grid[0].any() and not extra[0].any() and b"\tTP\n" not in text and extra[1].sum() > 0
        else:
            seen_tp = seen_tp or grid[0].sum() > 0
    assert seen_pure and seen_tp
    assert not [f for f in os.listdir(str(tmp_path / "points")) if ".tmp." in f]


def test_extract_many_genomes_and_profile_in_one_call_match_a_call_each(engine, tmp_path):
    """The one pair of passes that shares a call (qm_extract_files_profile takes the genome ids too): the spectra, the profiles and
    the three VCFs of every job are those of a call with genomes= alone and of a call with profile= alone."""
    from quasimodo_amd.extract import extract_many
    from test_gpu_motifs import random_genome
    genome = random_genome(np.random.default_rng(9606), 240_000, lower=0.1, nfrac=0.002)
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">seeded test genome\n" + b"\n".join(genome[i:i + 70] for i in range(0, len(genome), 70)) + b"\n")
    runs = {}
    for name in ("both", "genomes", "profile"):
        jobs = _golden_jobs(str(tmp_path / name))
        want = [0 if os.path.basename(j.vcf_file).split(".")[0].endswith("-1-0") else 1 for j in jobs]
        kw = {} if name == "profile" else {"genomes": [str(fa)] * len(jobs)}
        if name != "genomes":
            kw["profile"] = dict(PAR, want=want)
        runs[name] = extract_many(jobs, engine=engine, **kw)
    seen_motifs = seen_grid = False
    for b, g, p in zip(runs["both"], runs["genomes"], runs["profile"]):
        np.testing.assert_array_equal(b.stats["motifs"], g.stats["motifs"], err_msg=b.vcf_file)
        seen_motifs = seen_motifs or bool(b.stats["motifs"].any())
        assert ("af_grid" in b.stats) == ("af_grid" in p.stats) and "af_grid" not in g.stats and "motifs" not in p.stats
        if "af_grid" in p.stats:
            np.testing.assert_array_equal(b.stats["af_grid"], p.stats["af_grid"], err_msg=b.vcf_file)
            np.testing.assert_array_equal(b.stats["af_extra"], p.stats["af_extra"], err_msg=b.vcf_file)
            seen_grid = seen_grid or bool(b.stats["af_grid"].any())
        for other in (g, p):
            for x, y in ((b.filtered_out, other.filtered_out), (b.fp_out, other.fp_out)) + (((b.tp_out, other.tp_out),) if b.tp_out else ()):
                assert open(x, "rb").read() == open(y, "rb").read(), (x, y)
    assert seen_motifs and seen_grid


def _tree(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_tables_and_flag_off_tree(engine, tmp_path, gpus):
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), snp_profile=dict(PAR), **kw)
    on = _tree(str(out))
    new = {k for k in on if k.endswith((".snp.profile.tsv", ".snp.profile.afsweep.tsv", ".points.tsv"))}
    callers = sorted({os.path.basename(j.vcf_file).split(".")[2] for j in jobs})
    assert len(new) == 2 * 2 * len(callers) + sum(1 for j in jobs if not os.path.basename(j.vcf_file).split(".")[0].endswith("-1-0"))
    if gpus == 1:                                                   # without the flag: the same tree minus the new files
        off_dir = tmp_path / "off"
        workflow.run_hcmv_variantcall(str(data), str(off_dir), engine=engine)
        off = _tree(str(off_dir))
        assert off == {k: v for k, v in on.items() if k not in new}
    tables = out / "results" / "final_tables"
    for mix in ("TM", "TA"):
        for c in callers:
            lines = (tables / ("%s.%s.snp.profile.tsv" % (mix, c))).read_text().splitlines()
            assert lines[0].split("\t") == ["sample", "type", "af_lo", "af_hi", "pos_lo", "pos_hi", "count"]
            cells, extras = {}, {}
            for ln in lines[1:]:
                f = ln.split("\t")
                if ln.startswith("# sample"):
                    continue
                if ln.startswith("# "):
                    extras[(f[0][2:], f[1])] = [int(x) for x in f[2:]]
                else:
                    cells[(f[0], f[1], int(round(float(f[2]) * PAR["n_af_bins"])), (int(f[4]) - 1) // PAR["window"])] = int(f[6])
            sweep = (tables / ("%s.%s.snp.profile.afsweep.tsv" % (mix, c))).read_text().splitlines()
            for j in jobs:
                smp, _, cc = os.path.basename(j.vcf_file).split(".")[:3]
                if cc != c or smp[:2] != mix:
                    continue
                if smp.endswith("-1-0"):
                    assert not any(k[0] == smp for k in cells) and (smp, "FP") not in extras
                    continue
                wg, we = file_profile(j.tp_out or None, j.fp_out, PAR["window"], PAR["n_pos_bins"], PAR["n_af_bins"])
                for t, name in enumerate(("TP", "FP")):
                    got = {k[2:]: v for k, v in cells.items() if k[0] == smp and k[1] == name}
                    wantc = {(int(a), int(p)): int(wg[t, a, p]) for a, p in zip(*np.nonzero(wg[t]))}
                    if smp.endswith("-0-1") and name == "TP":
                        assert not got and (smp, "TP") not in extras and not wantc      # FP rows only
                        continue
                    assert got == wantc, (smp, c, name)
                    assert extras[(smp, name)] == [int(x) for x in we[t]]
                first = [ln.split("\t") for ln in sweep if ln.split("\t")[0] == smp][0]
                assert first[1] == "0" and int(first[2]) == int(we[0, N_GRID]) and int(first[3]) == int(we[1, N_GRID])
                pt = out / "results" / "snp" / "callers" / c / "profile" / (os.path.basename(j.vcf_file)[:-4] + ".points.tsv")
                assert pt.read_bytes() == points_text(j.tp_out or None, j.fp_out)
    snap = {k: on[k] for k in new}
    test_workflow_tables_and_flag_off_tree.snaps[gpus] = snap
    if len(test_workflow_tables_and_flag_off_tree.snaps) == 2:      # a VCF's rows do not depend on the rank
        assert test_workflow_tables_and_flag_off_tree.snaps[1] == test_workflow_tables_and_flag_off_tree.snaps[2]


test_workflow_tables_and_flag_off_tree.snaps = {}
