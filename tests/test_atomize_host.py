"""MNPs matched against adjacent SNVs, on the host (quasimodo_amd.atomize): hand-derived cases, the mask
bit-trick against the string loop, atoms against substitution into a genome, the restated tables on a hand-written VCF and truth
set, the table writer and the refusals of the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

from quasimodo_amd import atomize as at

BASES = "ACGT"
c = at.code


# ---- hand-derived cases -----------------------------------------------------------------------------------------------------
def test_an_mnp_is_two_atoms():
    assert at.atoms(100, "AC", "GT") == [(0, (100, "A", "G")), (1, (101, "C", "T"))]
    # A = 0, C = 1, G = 2, T = 3: (100 << 4 | 0 << 2 | 2), (101 << 4 | 1 << 2 | 3)
    assert at.atoms_codes(100, c("AC"), c("GT")) == (None, [(0, 1602), (1, 1623)])
    assert at.atoms_codes(100, c("A"), c("G")) == (None, [(0, 1602)])          # an SNV is its own atom


def test_a_padded_snv_is_one_atom_behind_the_pad():
    assert at.atoms(7, "AC", "AT") == [(1, (8, "C", "T"))]
    assert at.atoms_codes(7, c("AC"), c("AT")) == (None, [(1, (8 << 4) | (1 << 2) | 3)])


def test_thirteen_bases():
    r, a = "ACGTACGTACGTA", "CGTACGTACGTAC"                                       # every base differs
    why, got = at.atoms_codes(50, c(r), c(a))
    assert why is None and [k for k, _ in got] == list(range(13))
    assert got[0][1] == (50 << 4) | (0 << 2) | 1 and got[12][1] == (62 << 4) | (0 << 2) | 1
    assert at.mismatch_mask(c(r), c(a)) == 0x1555555
    why, got = at.atoms_codes(50, c(r), c(r[:12] + "T"))                         # only the last base differs
    assert why is None and got == [(12, (62 << 4) | (0 << 2) | 3)]
    assert at.mismatch_mask(c(r), c(r[:12] + "T")) == 1 << 24


def test_reasons_and_their_order():
    L, N, V, U, R = at.LONG, at.NOKEY, at.NOVAR, at.UNEQUAL, at.RANGE
    assert at.atoms_codes(5, at.DICT | 3, c("A"))[0] == L and at.atoms_codes(5, c("A"), -1)[0] == L and at.atoms_codes(5, 5, c("A"))[0] == L
    assert at.atoms_codes(5, c("AC"), c("GT"), nokey=True)[0] == N
    assert at.atoms_codes(5, c("AC"), c("AC"))[0] == V
    assert at.atoms_codes(5, c("AC"), c("A"))[0] == U and at.atoms_codes(5, c("A"), c("ACG"))[0] == U
    assert at.atoms_codes(-1, c("AC"), c("GT"))[0] == R
    # the first reason that applies: LONG before NOKEY before NOVAR before UNEQUAL before RANGE
    assert at.atoms_codes(-1, at.DICT | 3, at.DICT | 3, nokey=True)[0] == L
    assert at.atoms_codes(-1, c("AC"), c("AC"), nokey=True)[0] == N
    assert at.atoms_codes(-1, c("AC"), c("AC"))[0] == V
    assert at.atoms_codes(-1, c("AC"), c("A"))[0] == U
    assert at.REASONS == (L, N, V, U, R) and [at.CLASS_NAMES[x] for x in at.REASONS] == ["long", "nokey", "novar", "unequal", "range"]
    assert at.atoms_codes(5, c("AC"), c("GT"))[0] is None and at.atoms_codes(0, c("A"), c("G"))[0] is None


def test_the_last_position_an_atom_can_hold():
    top = (1 << 28) - 1
    assert at.atoms_codes(top, c("A"), c("G")) == (None, [(0, (top << 4) | 2)])
    assert at.atoms_codes(top - 12, c("ACGTACGTACGTA"), c("ACGTACGTACGTC")) == (None, [(12, (top << 4) | 1)])   # p + len - 1 = 2^28 - 1
    assert at.atoms_codes(top - 11, c("ACGTACGTACGTA"), c("ACGTACGTACGTC"))[0] == at.RANGE                     # ... = 2^28
    assert at.atoms_codes(top - 11, c("CCGTACGTACGTA"), c("ACGTACGTACGTA"))[0] == at.RANGE                     # (whichever base differs)
    assert at.atoms_codes(top + 1, c("A"), c("G"))[0] == at.RANGE
    assert (top << 4 | 15) < (1 << 32)


# ---- the bit trick ------------------------------------------------------------------------------------------------------------
def test_mismatch_mask_against_the_string_loop():
    rng = np.random.default_rng(7)
    for n in range(1, 14):
        for _ in range(200):
            r = "".join(BASES[i] for i in rng.integers(0, 4, n))
            a = list(r)
            for k in np.flatnonzero(rng.random(n) < rng.random()):
                a[k] = BASES[int(rng.integers(0, 4))]
            a = "".join(a)
            want = sum(1 << (2 * k) for k in range(n) if r[k] != a[k])
            assert at.mismatch_mask(c(r), c(a)) == want, (r, a)
            if r != a:
                why, got = at.atoms_codes(9, c(r), c(a))
                assert why is None and len(got) == bin(want).count("1")
                assert got == [(k, at.atom_key(9 + k, r[k], a[k])) for k in range(n) if r[k] != a[k]]


# ---- atoms against substitution ---------------------------------------------------------------------------------------------
def test_substituting_a_record_is_substituting_its_atoms_in_any_order():
    rng = np.random.default_rng(11)
    g = "".join(BASES[i] for i in rng.integers(0, 4, 600))
    n_multi = 0
    for _ in range(400):
        n = int(rng.integers(1, 14))
        p = int(rng.integers(1, 600 - n + 2))
        ref = g[p - 1:p - 1 + n]
        alt = "".join(ch if rng.random() < 0.5 else BASES[int(rng.integers(0, 4))] for ch in ref)
        if alt == ref:
            continue
        whole = g[:p - 1] + alt + g[p - 1 + n:]
        parts = at.atoms(p, ref, alt)
        n_multi += len(parts) >= 2
        for _ in range(3):
            m = list(g)
            for k in rng.permutation(len(parts)):
                _, (q, r1, a1) = parts[k]
                assert m[q - 1] == r1                    # the atoms do not overlap: every one finds its REF
                m[q - 1] = a1
            assert "".join(m) == whole
    assert n_multi > 100


# ---- the restated tables ----------------------------------------------------------------------------------------------------
def test_constants_match_the_header():
    from quasimodo_amd import _lib
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "qmvt.h")).read()
    assert len(at.R_COLS) == _lib.QM_ATOM_R_COLS == 13 and len(at.T_COLS) == _lib.QM_ATOM_T_COLS == 6
    assert "#define QM_ATOM_R_COLS 13" in text and "#define QM_ATOM_T_COLS 6" in text and "#define QM_ATOM_COLUMNS 2u" in text
    for k, name in enumerate(at.CLASS_NAMES):
        assert "QM_ATOM_C_%s = %d" % (name.upper(), k) in text
    for k, name in enumerate(at.R_COLS):
        assert "QM_ATOM_R_%s = %d" % (name.upper(), k) in text
    for k, name in enumerate(at.T_COLS):
        assert "QM_ATOM_T_%s = %d" % (name.upper(), k) in text
    assert at.INLINE_MAX == 13 and "#define QM_ALLELE_INLINE_MAX 13" in text
    assert _lib.QM_ABI_VERSION == 6
    for name in ("qm_batch_atomize", "qm_batch_get_atomize", "qm_batch_get_atomized", "qm_batch_atomize_timings", "qm_truth_atoms",
                 "qm_extract_files_atomize"):
        assert name in _lib.EXPORTS and name in text


def small_case():
    """truth: SNVs at 100, 101, 200, 201, 500, an MNP AC>GT at 300, an MNP CA>TG at 400, a deletion at 600"""
    truth = ([100, 101, 200, 201, 300, 400, 500, 600], [c("A"), c("C"), c("G"), c("G"), c("AC"), c("CA"), c("T"), c("TA")],
             [c("G"), c("T"), c("A"), c("C"), c("GT"), c("TG"), c("A"), c("T")])
    rows = [                                            # (pos, ref, alt, flags, kept, tp)
        (100, "AC", "GT", 3, True, False),              # 0 a full MNP over the two truth SNVs at 100, 101: rescued
        (200, "GG", "AT", 3, True, False),              # 1 a partial one: G>A at 200 is there, G>T at 201 is not
        (300, "A", "G", 3, True, False),                # 2, 3 the truth MNP at 300 found by its two SNVs
        (301, "C", "T", 3, True, False),
        (400, "C", "T", 3, True, False),                # 4 the truth MNP at 400 found by one of its SNVs only
        (100, "ACT", "GTT", 1, True, False),            # 5 a full one with an ID: not a TP_A line
        (700, "AC", "CA", 11, True, True),              # 6 a TP line of the text side: no atom hit, TP_A all the same
        (100, "AC", "GT", 3, True, False),              # 7 a duplicate of line 0
        (500, "T", "A", 3, True, True),                 # 8 an exact SNV
        (600, "TA", "T", 3, True, True),                # 9 an exact deletion: not atomisable, keeps its verdict
        (200, "GG", "AC", 2, False, False),             # 10 a full one that is not kept
    ]
    return truth, rows


def test_counts_on_a_hand_written_vcf_and_truth_set():
    truth, rows = small_case()
    pos, ref, alt = [r[0] for r in rows], [c(r[1]) for r in rows], [c(r[2]) for r in rows]
    flags, kept, tp = [r[3] for r in rows], [r[4] for r in rows], [r[5] for r in rows]
    rec, tru, cls, na, hm = at.counts(truth, pos, ref, alt, flags, kept, tp)
    assert dict(zip(at.R_COLS, rec.tolist())) == {"kept": 10, "tp": 3, "tp_a": 8, "rescued": 5, "multi": 5, "partial": 1, "atoms": 14,
                                                  "atoms_hit": 11, "long": 0, "nokey": 0, "novar": 0, "unequal": 1, "range": 0}
    # atoms: 100 A>G, 101 C>T, 200 G>A, 201 G>C, 300 A>G, 301 C>T, 400 C>T, 401 A>G, 500 T>A -- 9 of 7 atomisable entries;
    # found: all but 201 G>C (its record is not kept) and 401 A>G; entries found by spelling: 500 and the deletion
    assert dict(zip(at.T_COLS, tru.tolist())) == {"entries": 8, "atomisable": 7, "atoms": 9, "atoms_found": 7, "found": 2, "found_a": 6}
    F, P, N, R = at.FULL, at.PARTIAL, at.NONE, at.RESCUED
    assert cls.tolist() == [R, P, R, R, R, F, N, R, F, at.UNEQUAL, F]
    assert na.tolist() == [2, 2, 1, 1, 1, 2, 2, 2, 1, 0, 2]
    assert hm.tolist() == [3, 1, 1, 1, 1, 3, 0, 3, 1, 0, 3]
    assert int(tru[4]) <= int(tru[5])
    # an empty truth set: tru stays zero, everything kept is FP
    none = (np.zeros(0, np.int32),) * 3
    rec0, tru0, cls0, _, hm0 = at.counts(none, pos, ref, alt, [f & ~8 for f in flags], kept, [False] * len(rows))
    assert not tru0.any() and int(rec0[0]) == 10 and int(rec0[1]) == int(rec0[2]) == int(rec0[7]) == 0 and not hm0.any()
    assert set(cls0.tolist()) == {N, at.UNEQUAL}


def test_an_exact_tp_line_is_a_tp_a_line():
    truth, rows = small_case()
    t = at.truth_order(*truth)
    pos, ref, alt = [e[0] for e in t], [e[1] for e in t], [e[2] for e in t]
    n = len(t)
    rec, tru, cls, na, hm = at.counts(truth, pos, ref, alt, [3] * n, [True] * n, [True] * n)
    assert int(rec[1]) == int(rec[2]) == n and int(rec[3]) == 0 and int(tru[4]) == int(tru[5]) == n
    assert set(cls.tolist()) == {at.FULL, at.UNEQUAL}


# ---- writers, paths and refusals ------------------------------------------------------------------------------------------
def test_table_writer_and_atoms_reader(tmp_path):
    from quasimodo_amd.extract import Job, _paths
    rec = np.array([10, 4, 7, 3, 5, 1, 16, 12, 1, 0, 0, 2, 0], np.uint64)
    tru = np.array([8, 7, 11, 9, 4, 6], np.uint64)
    row = at.performance_row(rec, tru)
    # by spelling: 4 of 10 lines, 4 of 8 entries; by atoms: 7 of 10 lines, 6 of 8 entries; R's round(x, 3)
    assert row[:6] == [4, 6, 4, 0.4, 0.5, 0.444] and row[6:12] == [7, 3, 2, 0.7, 0.75, 0.724]
    assert row[12:] == [3, 5, 1, 16, 12, 1, 0, 0, 2, 0, 8, 7, 11]
    assert at.performance_row(np.zeros(13, np.uint64), tru)[:6] == [0, 0, 4, None, None, None]
    path = tmp_path / "t.tsv"
    at.write_performance_atomized(str(path), [("lofreq", "TA-1-10", {"atom_rec": rec, "atom_tru": tru}), ("lofreq", "TA-1-0", {"n_pass": 3}),
                                              ("mine", "TM-1-1", {"atom_rec": np.zeros(13, np.uint64), "atom_tru": tru})])
    assert path.read_bytes() == (
        b"caller\tmixture\tTP\tFP\tFN\tPrecision\tRecall\tF1\tTP_A\tFP_A\tFN_A\tPrecision_A\tRecall_A\tF1_A\trescued\tmulti\tpartial\tatoms\t"
        b"atoms_hit\tlong\tnokey\tnovar\tunequal\trange\ttruth_entries\ttruth_atomisable\ttruth_atoms\n"
        b"LoFreq\tTA-1-10\t4\t6\t4\t0.4\t0.5\t0.444\t7\t3\t2\t0.7\t0.75\t0.724\t3\t5\t1\t16\t12\t1\t0\t0\t2\t0\t8\t7\t11\n"
        b"mine\tTM-1-1\t0\t0\t4\tNA\tNA\tNA\t0\t0\t2\tNA\tNA\tNA\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t8\t7\t11\n")     # the pure-strain job is left out
    assert not [x for x in os.listdir(tmp_path) if x != "t.tsv"]                  # written through a temporary file that is gone
    j = Job("/x/callers/lofreq/TA-1-10.AD169.lofreq.vcf", "/x/t.vcf", "hcmv")
    _paths(j)
    assert at.atoms_path(j) == "/x/callers/lofreq/atoms/TA-1-10.AD169.lofreq.atoms.tsv"
    res = tmp_path / "r.tsv"
    res.write_text(at.ATOMS_HEADER + "\n12\t100\tAC\tGT\t2\t2\t0x0003\trescued\n40\t200\tGG\tAT\t2\t1\t0x0001\tpartial\n")
    assert at.read_atoms(str(res)) == [(12, ("100", "AC", "GT"), 2, 2, 3, "rescued"), (40, ("200", "GG", "AT"), 2, 1, 1, "partial")]
    assert at.ATOMS_HEADER == "#line\tPOS\tREF\tALT\tN_ATOMS\tN_HIT\tHIT_MASK\tCLASS"
    res.write_text("#line\tPOS\n")
    with pytest.raises(ValueError):
        at.read_atoms(str(res))


def test_refusals_in_front_of_any_file(tmp_path):
    from conftest import ROOT
    from quasimodo_amd import passes, workflow
    from quasimodo_amd.extract import Job, extract_many
    p = [x for x in passes.PASSES if x.name == "atomize"]
    assert len(p) == 1 and p[0].flag == "--atomize" and p[0].shares == () and p[0].fields == ("atomize",) and p[0].agree is None
    fa = str(tmp_path / "a.fa")
    mk = lambda: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i) for i in range(2)]
    with pytest.raises(ValueError, match="--alleles"):                          # --atomize without --alleles
        extract_many(mk(), atomize=True)
    with pytest.raises(ValueError, match="--alleles"):
        extract_many(mk(), alleles=False, atomize=[True, False])
    with pytest.raises(ValueError, match="atomize: 1 entries for 2 jobs"):
        extract_many(mk(), alleles=True, atomize=[True])
    for other in (dict(fn=True), dict(strata=[("all", [0], [100])]), dict(boot={}), dict(explain=3), dict(surface=True),
                  dict(context={"genomes": [fa, fa]}), dict(genomes=[fa, fa]), dict(normalize=[fa, fa])):
        with pytest.raises(ValueError, match="does not combine"):
            extract_many(mk(), alleles=True, atomize=True, **other)
    with pytest.raises(passes.SharedCallError):
        passes.check_shared_call({"atomize", "normalize"})
    passes.check_alleles({"atomize"}, True)
    with pytest.raises(ValueError, match="--alleles"):
        passes.check_alleles({"atomize"}, False)
    with pytest.raises(workflow.WorkflowError, match="--atomize needs --alleles"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), atomize=True)
    with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
        workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), alleles=True, atomize=True, truth_side=True)
    # vareval: a show-snps table has no allele-extended reading
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", str(tmp_path / "a.vcf"), "--snps", str(tmp_path / "a.snps"),
                        "-l", "a", "-o", str(tmp_path / "v"), "--atomize"], capture_output=True, text=True)
    assert r.returncode != 0 and "allele-extended" in r.stderr + r.stdout and "--atomize" in r.stderr + r.stdout
    assert not any(x.is_file() for x in tmp_path.rglob("*")) and not (tmp_path / "v").exists()   # no file was written
