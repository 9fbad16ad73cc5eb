"""The host side of the k-of-n caller consensus (quasimodo_amd/consensus.py): level arithmetic from hand-written
vote histograms, the text rule of a consensus VCF on a hand-derived three-member case, and the table writers byte for byte.
No GPU."""
import math

import pytest

from quasimodo_amd import consensus as K


def test_level_counts_by_hand():
    #            c = 0  1  2  3
    tp_votes = [4, 1, 2, 3] + [0] * 29      # T' = 10
    fp_votes = [0, 5, 1, 2] + [0] * 29
    assert K.level_counts(tp_votes, fp_votes, 3) == [(1, 6, 8, 4), (2, 5, 3, 5), (3, 3, 2, 7)]
    assert K.level_counts([7, 0], [0, 0], 1) == [(1, 0, 0, 7)]


def test_level_counts_refuses_votes_outside_the_group():
    with pytest.raises(ValueError):
        K.level_counts([1, 1, 1], [0, 0, 0], 1)          # a vote count above n
    with pytest.raises(ValueError):
        K.level_counts([1, 1], [1, 0], 1)                # a non-truth key nobody calls
    with pytest.raises(ValueError):
        K.level_counts([1], [0], 1)                      # too few slots
    with pytest.raises(ValueError):
        K.level_counts([0] * 40, [0] * 40, 33)


def test_level_row_ratios_and_rounding():
    # 6 / 14 = 0.428571 -> 0.429, 6 / 10 = 0.6, F1 of the ROUNDED ratios: 2 * 0.429 * 0.6 / 1.029 = 0.500291 -> 0.5
    assert K.level_row(6, 8, 4) == (6, 8, 4, 0.429, 0.6, 0.5)
    # no key at the level: the three ratios are NA, as caller_performance.tsv writes a caller that kept nothing
    assert K.level_row(0, 0, 7) == (0, 0, 7, None, None, None)
    # keys at the level, none true: P = 0, R = 0, F1 = 0 / 0 = NaN
    tp, fp, fn, p, r, f1 = K.level_row(0, 3, 7)
    assert (tp, fp, fn, p, r) == (0, 3, 7, 0.0, 0.0) and math.isnan(f1)
    # an empty truth set: R = 0 / 0 = NaN
    tp, fp, fn, p, r, f1 = K.level_row(0, 3, 0)
    assert p == 0.0 and math.isnan(r) and math.isnan(f1)  # 0 / 0


HEAD0 = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"
HEAD1 = b"##fileformat=VCFv4.1\n##other=1\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n"


def _ln(pos, ref, alt, tag):
    return b"chr\t%s\t.\t%s\t%s\t50\tPASS\t%s\n" % (pos, ref, alt, tag)


def test_consensus_text_three_members_by_hand():
    # keys:            a = (10, A, C)   b = (10, A, G)   c = (20, C, T)   d = (5, G, A)   e = (30, T, A)
    # member 0 calls   a (on two lines), c
    # member 1 calls   a, b, d
    # member 2 calls   a, b, c, e       -> votes a 3, b 2, c 2, d 1, e 1; ascending keys: d, a, b, c, e
    m0 = HEAD0 + _ln(b"20", b"C", b"T", b"m0c") + _ln(b"10", b"A", b"C", b"m0a1") + _ln(b"10", b"A", b"C", b"m0a2")
    m1 = HEAD1 + _ln(b"10", b"A", b"G", b"m1b") + _ln(b"5", b"G", b"A", b"m1d") + _ln(b"10", b"A", b"C", b"m1a")
    m2 = HEAD1 + _ln(b"10", b"A", b"C", b"m2a") + _ln(b"10", b"A", b"G", b"m2b") + _ln(b"20", b"C", b"T", b"m2c") + _ln(b"30", b"T", b"A", b"m2e")
    texts = [m0, m1, m2]
    d, a, b, c, e = (_ln(b"5", b"G", b"A", b"m1d"), _ln(b"10", b"A", b"C", b"m0a1"), _ln(b"10", b"A", b"G", b"m1b"),
                     _ln(b"20", b"C", b"T", b"m0c"), _ln(b"30", b"T", b"A", b"m2e"))
    # k = 1: the union.  a: the FIRST of member 0's two lines; b: member 1 is the lowest member that calls it, not the first member
    assert K.consensus_text(texts, 1) == HEAD0 + d + a + b + c + e
    assert K.consensus_text(texts, 2) == HEAD0 + a + b + c
    assert K.consensus_text(texts, 3) == HEAD0 + a                  # k = n: the intersection
    assert K.vote_masks(texts) == {5 << 4 | 2 << 2 | 0: 0b010, 10 << 4 | 0 << 2 | 1: 0b111, 10 << 4 | 0 << 2 | 2: 0b110,
                                   20 << 4 | 1 << 2 | 3: 0b101, 30 << 4 | 3 << 2 | 0: 0b100}
    # member order matters for the header and the line, not for the set
    assert K.consensus_text(texts[::-1], 2) == HEAD1 + _ln(b"10", b"A", b"C", b"m2a") + _ln(b"10", b"A", b"G", b"m2b") + _ln(b"20", b"C", b"T", b"m2c")
    for k in (0, 4):
        with pytest.raises(ValueError):
            K.consensus_text(texts, k)


def test_consensus_text_skips_lines_without_a_device_key():
    odd = (HEAD0 + _ln(b"010", b"A", b"C", b"leading-zero") + _ln(b"7", b"AT", b"C", b"indel") + _ln(b"7", b"a", b"C", b"lower")
           + _ln(b"%d" % (1 << 28), b"A", b"C", b"beyond") + _ln(b"%d" % ((1 << 28) - 1), b"A", b"C", b"top") + b"chr\t7\t.\tA\n"
           + _ln(b"0", b"T", b"G", b"zero") + b"chr\t9\t.\tC\tG\t1\tPASS\tcr\r\n")
    out = K.consensus_text([odd], 1)
    assert out == HEAD0 + _ln(b"0", b"T", b"G", b"zero") + b"chr\t9\t.\tC\tG\t1\tPASS\tcr\r\n" + _ln(b"%d" % ((1 << 28) - 1), b"A", b"C", b"top")
    assert K.device_key(b"#chr\t1\t.\tA\tC") is None


def test_table_writers_byte_for_byte(tmp_path):
    p = tmp_path / "caller_consensus.tsv"
    K.write_caller_consensus(str(p), {"TM-1-1": (1, [7, 0], [0, 0]),
                                     "TA-1-10": (3, [4, 1, 2, 3] + [0] * 29, [0, 5, 1, 2] + [0] * 29)})
    assert p.read_bytes() == (b"sample\tk\tn\tTP\tFP\tFN\tPrecision\tRecall\tF1\n"
                              b"TA-1-10\t1\t3\t6\t8\t4\t0.429\t0.6\t0.5\n"
                              b"TA-1-10\t2\t3\t5\t3\t5\t0.625\t0.5\t0.556\n"
                              b"TA-1-10\t3\t3\t3\t2\t7\t0.6\t0.3\t0.4\n"
                              b"TM-1-1\t1\t1\t0\t0\t7\tNA\tNA\tNA\n")
    q = tmp_path / "caller_private.tsv"
    K.write_caller_private(str(q), {"TM-1-1": (["mycaller"], [0] * 32, [3] + [0] * 31),
                                    "TA-1-10": (["lofreq", "varscan", "clc"], [1, 0, 2] + [0] * 29, [9, 8, 7] + [0] * 29)})
    assert q.read_bytes() == (b"sample\tcaller\tprivate_TP\tprivate_FP\n"
                              b"TA-1-10\tLoFreq\t1\t9\nTA-1-10\tVarScan2\t0\t8\nTA-1-10\tCLC\t2\t7\n"
                              b"TM-1-1\tmycaller\t0\t3\n")
    assert not [f for f in tmp_path.iterdir() if ".tmp." in f.name]
    with pytest.raises(ValueError):
        K.write_caller_private(str(q), {"s": (["a", "a"], [0, 0], [0, 0])})


def test_group_limits():
    assert K.check_group(range(32)) == list(range(32))
    for bad in ([], list(range(33))):
        with pytest.raises(ValueError):
            K.check_group(bad)


# ---- CLI flag handling (no device: --dryrun and the checks in front of the engine) -------------------------------------------
def _bundle(root):
    from test_tables_workflow import _build_bundle
    _build_bundle(root)


def _cli(args):
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return subprocess.run([sys.executable, os.path.join(root, "run_benchmark.py")] + args, capture_output=True, text=True, cwd=root)


def test_cli_votes_dryrun_and_the_level_above_n(tmp_path):
    data = tmp_path / "data" / "snp"
    _bundle(str(data))
    base = ["hcmv", "-e", "variantcall", "--data", str(data), "-o", str(tmp_path / "out"), "--dryrun"]
    plain = _cli(base)
    assert plain.returncode == 0 and "caller_consensus" not in plain.stdout and "consensus_vcf" not in plain.stdout
    r = _cli(base + ["--votes"])
    assert r.returncode == 0, r.stderr
    callers = sorted({ln.split("\t")[1] for ln in r.stdout.splitlines() if ln.startswith("extractTP\t")})
    cc = [ln for ln in r.stdout.splitlines() if ln.startswith("caller_consensus\t")]
    assert len(cc) == 1 and sorted(cc[0].split("\t")[1].split(",")) == callers and len(callers) == 6
    assert "consensus_vcf" not in r.stdout
    r = _cli(base + ["--consensus-vcf", "6"])               # implies --votes; 6 of 6 callers is allowed
    assert r.returncode == 0, r.stderr
    cv = [ln for ln in r.stdout.splitlines() if ln.startswith("consensus_vcf\t")]
    assert len(cv) == 6 and all(ln.endswith("\t6") for ln in cv) and not any("-1-0" in ln or "-0-1" in ln for ln in cv)
    r = _cli(base + ["--votes", "--consensus-vcf", "7"])    # K > n: an error that names the sample
    assert r.returncode != 0 and "TA-1-1" in r.stdout and "--consensus-vcf 7" in r.stdout and "6 callers" in r.stdout
    r = _cli(base + ["--consensus-vcf", "0"])
    assert r.returncode != 0 and "at least 1" in r.stdout
    r = _cli(base + ["--votes", "--truth-side"])
    assert r.returncode != 0 and "cannot be combined" in r.stdout


def test_workflow_votes_checks_in_front_of_the_engine(tmp_path, capsys):
    from quasimodo_amd import workflow
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(33)]
    # more than 32 labels: a note and no table (the dry run stops in front of the files)
    assert workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, votes=True) is None
    out = capsys.readouterr().out
    assert "33 labels" in out and "no table is written" in out and "caller_consensus" not in out
    assert workflow.run_vareval(vcfs[:3], str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, consensus_vcf=3) is None
    out = capsys.readouterr().out
    assert "caller_consensus\tv0,v1,v2" in out and "consensus_vcf\tcustom\t3" in out
    with pytest.raises(workflow.WorkflowError, match="custom.*--consensus-vcf 4.*3 labels"):
        workflow.run_vareval(vcfs[:3], str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, consensus_vcf=4)
    with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
        workflow.run_vareval(vcfs[:3], str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, votes=True, bootstrap=10)


def test_extract_many_votes_argument_checks():
    from quasimodo_amd.extract import Job, extract_many
    mk = lambda n: [Job("s.c%d.vcf" % i, "t.vcf", "hcmv", "", "c%d" % i) for i in range(n)]
    with pytest.raises(ValueError, match="groups"):
        extract_many(mk(2), votes=True)
    with pytest.raises(ValueError, match="1 to 32"):
        extract_many(mk(33), votes=True, groups=[list(range(33))])
    with pytest.raises(ValueError, match="two vote groups"):
        extract_many(mk(3), votes=True, groups=[[0, 1], [1, 2]])
    with pytest.raises(ValueError, match="consensus level 3 with 2 members"):
        extract_many(mk(2), votes={"k": [3], "out": ["x.vcf"]}, groups=[[0, 1]])
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(mk(2), votes=True, groups=[[0, 1]], fn=True)
