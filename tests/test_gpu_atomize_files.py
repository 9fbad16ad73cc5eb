"""MNPs matched against adjacent SNVs end to end (qm_extract_files_atomize, extract_many(alleles=True, atomize=), --alleles
--atomize): a small family built from the golden allele probe -- its VCF and truth file with rows added behind
them: adjacent truth SNVs called as one MNP, a truth MNP called as SNVs, a partial MNP, a padded SNV -- against a restatement on
TEXT: the lines of the input and of the written *.filtered.vcf and *.tp.vcf through the Python atomiser."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from quasimodo_amd import atomize as at

pytestmark = pytest.mark.gpu

PROBE = os.path.join(GOLDEN, "alleles", "input", "probe.vcf")
TRUTH = os.path.join(GOLDEN, "alleles", "input", "probe.truth.vcf")
ALLELE = re.compile(rb"^[ACGT]+$")
CANON = re.compile(rb"^(0|[1-9][0-9]{0,8})$")

TRUTH_ROWS = [b"c\t150\t.\tA\tG\t30\tPASS\tTYPE=SNV", b"c\t151\t.\tC\tT\t30\tPASS\tTYPE=SNV",     # two adjacent SNVs
              b"c\t160\t.\tAC\tGT\t30\tPASS\tTYPE=MNP",                                             # an MNP the caller splits
              b"c\t170\t.\tG\tA\t30\tPASS\tTYPE=SNV",
              b"c\t180\t.\tCAT\tTAG\t30\tPASS\tTYPE=MNP"]                                           # an MNP found by one SNV only
VCF_ROWS = [b"c\t150\t.\tAC\tGT\t50\tPASS\tDP=9",          # an MNP over the two adjacent truth SNVs: rescued
            b"c\t150\trs1\tAC\tGT\t50\tPASS\tDP=9",        # ... with an ID: full, no TP_A line
            b"c\t150\t.\tACG\tGTG\t50\tPASS\tDP=9",        # ... padded behind
            b"c\t150\t.\tAC\tGA\t50\tPASS\tDP=9",          # a partial one
            b"c\t150\t.\tAC\tGT\t5\tPASS\tDP=9",           # not kept
            b"c\t160\t.\tA\tG\t50\tPASS\tDP=9",            # the truth MNP as its two SNVs
            b"c\t161\t.\tC\tT\t50\tPASS\tDP=9",
            b"c\t169\t.\tTG\tTA\t50\tPASS\tDP=9",          # a padded SNV: one atom at 170
            b"c\t170\t.\tGT\tAC\t50\tPASS\tDP=9",          # partial
            b"c\t180\t.\tC\tT\t50\tPASS\tDP=9",            # one of the two atoms of the truth MNP at 180
            b"c\t190\t.\tACGTACGTACGTA\tCGTACGTACGTAC\t50\tPASS\tDP=9",    # thirteen atoms, none hit
            b"c\t200\t.\tACGTACGTACGTAC\tCGTACGTACGTACG\t50\tPASS\tDP=9"]  # fourteen bases: LONG


def data_lines(text):
    """[(1-based line number, fields)] of the data lines"""
    return [(i + 1, ln.split(b"\t")) for i, ln in enumerate(text.split(b"\n")) if ln and ln[:1] != b"#"]


class Codes:
    """allele strings as codes: inline up to 13 bases, ids of this test's own dictionary beyond; -1 for what is no allele"""

    def __init__(self):
        self.ids = {}

    def __call__(self, s):
        if not ALLELE.match(s):
            return -1
        if len(s) <= at.INLINE_MAX:
            return at.code(s.decode())
        return at.DICT | self.ids.setdefault(s, len(self.ids))


def family(tmp_path, name):
    """the truth file with its added rows, three VCFs: the probe with the added lines behind it, the added lines alone, the
    probe alone"""
    d = tmp_path / name
    d.mkdir()
    truth_text = open(TRUTH, "rb").read() + b"\n".join(TRUTH_ROWS) + b"\n"
    (d / "truth.vcf").write_bytes(truth_text)
    probe = open(PROBE, "rb").read()
    head = b"".join(ln + b"\n" for ln in probe.split(b"\n") if ln[:1] == b"#")
    vcfs = []
    for base, text in (("s1.c.both.vcf", probe + b"\n".join(VCF_ROWS) + b"\n"), ("s2.c.added.vcf", head + b"\n".join(VCF_ROWS) + b"\n"),
                       ("s3.c.probe.vcf", probe)):
        (d / base).write_bytes(text)
        vcfs.append(str(d / base))
    return vcfs, str(d / "truth.vcf"), truth_text


def restate(vcf, filtered, tp, truth_text):
    """(rec, tru, atoms rows) of one VCF from text: kept = the lines of filtered.vcf, TP = those of tp.vcf (both written in
    input order), the columns split at tabs"""
    code = Codes()
    tr = [f for _, f in data_lines(truth_text) if CANON.match(f[1]) and ALLELE.match(f[3]) and ALLELE.match(f[4])]
    truth = ([int(f[1]) for f in tr], [code(f[3]) for f in tr], [code(f[4]) for f in tr])
    lines = data_lines(open(vcf, "rb").read())

    def member(path):
        rest = [f for _, f in data_lines(open(path, "rb").read())]
        out = []
        for _, f in lines:
            out.append(bool(rest) and rest[0] == f)
            if out[-1]:
                rest.pop(0)
        assert not rest, path
        return np.array(out, bool)
    kept, tpm = member(filtered), member(tp)
    assert not (tpm & ~kept).any()
    pos = [int(f[1]) if CANON.match(f[1]) else 0 for _, f in lines]
    ref, alt = [code(f[3]) for _, f in lines], [code(f[4]) for _, f in lines]
    flags = [1 * bool(k) | 2 * (f[2] == b".") | 4 * (not CANON.match(f[1])) | 8 * bool(t) for (_, f), k, t in zip(lines, kept, tpm)]
    rec, tru, cls, na, hm = at.counts(truth, pos, ref, alt, flags, kept, tpm)
    rows = [(no, (f[1].decode(), f[3].decode(), f[4].decode()), int(na[i]), bin(int(hm[i])).count("1"), int(hm[i]), at.CLASS_NAMES[cls[i]])
            for i, (no, f) in enumerate(lines) if kept[i] and na[i] >= 2]
    return rec, tru, rows


def _jobs(vcfs, truth, **kw):
    from quasimodo_amd.extract import Job
    return [Job(v, truth, "hcmv", "", "c", **kw) for v in vcfs]


def test_extract_many_atomize_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import _paths, extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    vcfs, truth, truth_text = family(tmp_path, "one")
    pv, pt, _ = family(tmp_path, "plain")
    plain = extract_many(_jobs(pv, pt), engine=engine, alleles=True)
    jobs = extract_many(_jobs(vcfs, truth), engine=engine, alleles=True, atomize=True)
    # without atomize= the tree is the same but for atoms/
    on, off = _tree(str(tmp_path / "one")), _tree(str(tmp_path / "plain"))
    assert off == {k: v for k, v in on.items() if not k.startswith("atoms" + os.sep)}
    assert sorted(k for k in on if k.startswith("atoms" + os.sep)) == sorted(os.path.join("atoms", os.path.basename(v)[:-4] + ".atoms.tsv") for v in vcfs)
    want = []
    for p, j in zip(plain, jobs):
        rec, tru, rows = restate(j.vcf_file, j.filtered_out, j.tp_out, truth_text)
        want.append((rec, tru))
        np.testing.assert_array_equal(j.stats["atom_rec"], rec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["atom_tru"], tru, err_msg=j.vcf_file)
        assert at.read_atoms(j.atoms_out) == rows
        assert [int(x) for x in rec[:2]] == [j.stats["n_pass"], j.stats["tp_lines"]] and int(rec[2]) >= int(rec[1])
        assert int(tru[4]) == j.stats["TP_R"] and int(tru[4]) <= int(tru[5])
        for k in p.stats:                                          # the rows of the plain call, unchanged
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
    # the added lines by hand: 150 AC>GT, its padded copy, the two SNVs of the MNP at 160, the padded SNV at 169 and the SNV at 180
    # are rescued; 150 AC>GA and 170 GT>AC are partial; 6 kept lines have two atoms or more
    r2 = dict(zip(at.R_COLS, [int(x) for x in jobs[1].stats["atom_rec"]]))
    assert (r2["kept"], r2["tp"], r2["tp_a"], r2["rescued"], r2["multi"], r2["partial"], r2["long"]) == (11, 0, 6, 6, 6, 2, 1)
    assert (r2["atoms"], r2["atoms_hit"]) == (2 + 2 + 2 + 2 + 1 + 1 + 1 + 2 + 1 + 13, 2 + 2 + 2 + 1 + 1 + 1 + 1 + 1 + 1)
    t2 = dict(zip(at.T_COLS, [int(x) for x in jobs[1].stats["atom_tru"]]))
    assert t2["found"] == 0 and t2["found_a"] == 4 and t2["atoms_found"] == 6      # 150, 151, 160 AC>GT, 170; 180 CAT>TAG lacks its T>G
    n_head = sum(ln[:1] == b"#" for ln in open(PROBE, "rb").read().split(b"\n"))
    assert [r[0] for r in at.read_atoms(jobs[1].atoms_out)] == [n_head + k for k in (1, 2, 3, 4, 9, 11)]
    assert int(jobs[2].stats["atom_rec"][3]) == 0                                  # the probe alone: nothing to rescue
    # sharded over two ranks of one device: the same rows, the same files, the same table
    svcfs, struth, _ = family(tmp_path, "two")
    sj = _jobs(svcfs, struth, atomize=True)
    for j in sj:
        _paths(j)
        j.atoms_out = at.atoms_path(j)
    sj, _ = extract_many_sharded(sj, 2, backend="gloo", same_device=True, alleles=True)
    two = _tree(str(tmp_path / "two"))
    assert {k: two.get(k) for k in on} == on
    for a, b in zip(jobs, sj):
        np.testing.assert_array_equal(a.stats["atom_rec"], np.asarray(b.stats["atom_rec"]))
        np.testing.assert_array_equal(a.stats["atom_tru"], np.asarray(b.stats["atom_tru"]))
    # the table, against the restated rows through the documented arithmetic
    t1, t2, t3 = tmp_path / "t1.tsv", tmp_path / "t2.tsv", tmp_path / "t3.tsv"
    name = lambda j: os.path.basename(j.vcf_file).split(".")[0]
    at.write_performance_atomized(str(t1), [("c", name(j), j.stats) for j in jobs])
    at.write_performance_atomized(str(t2), [("c", name(j), j.stats) for j in sj])
    at.write_performance_atomized(str(t3), [("c", name(j), {"atom_rec": w[0], "atom_tru": w[1]}) for j, w in zip(jobs, want)])
    assert t1.read_bytes() == t2.read_bytes() == t3.read_bytes() and len(t1.read_text().split("\n")) == 5
    row = dict(zip(t1.read_text().split("\n")[0].split("\t"), t1.read_text().split("\n")[2].split("\t")))
    n_ent = int(jobs[1].stats["atom_tru"][0])
    assert (row["mixture"], row["TP"], row["FP"], row["FN"]) == ("s2", "0", "11", str(n_ent))
    assert (row["TP_A"], row["FP_A"], row["FN_A"], row["Precision_A"]) == ("6", "5", str(n_ent - 4), "0.545")      # 6 / 11
    # refusals, in front of any file: without the allele-extended mode, a second pass in the call
    for kw, said in ((dict(atomize=True), "--alleles"), (dict(alleles=True, atomize=True, fn=True), "does not combine")):
        rv, rt, _ = family(tmp_path, "r%d" % len(os.listdir(tmp_path)))
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(rv, rt), engine=engine, **kw)


def test_command_line(tmp_path):
    """hcmv -e variantcall --alleles --atomize writes the table and the atoms files, and without the flag the same tree but for
    them"""
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    cmd = [sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data), "--alleles"]
    r = subprocess.run(cmd + ["-o", str(tmp_path / "on"), "--atomize"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(cmd + ["-o", str(tmp_path / "off")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    on, off = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off"))
    name = os.path.join("results", "final_tables", "caller_performance_atomized.tsv")
    mine = lambda k: k == name or (os.sep + "atoms" + os.sep) in k
    assert name in on and off == {k: v for k, v in on.items() if not mine(k)}
    lines = on[name].decode().split("\n")
    head = lines[0].split("\t")
    assert head == list(at.TABLE_HEADER[0] + at.TABLE_HEADER[1]) and lines[-1] == ""
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]
    whole = on[os.path.join("results", "final_tables", "caller_performance.tsv")].decode().split("\n")[1:-1]
    mixed = [w for w in whole if not w.split("\t")[1].endswith(("-1-0", "-0-1"))]
    assert len(rows) == len(mixed) > 0 and len([k for k in on if mine(k)]) == len(rows) + 1
    for k in on:
        if mine(k) and k != name:
            assert on[k].split(b"\n")[0].decode() == at.ATOMS_HEADER and os.path.basename(k).endswith(".atoms.tsv")
    for r_ in rows:
        assert int(r_["TP_A"]) >= int(r_["TP"]) and int(r_["FN_A"]) <= int(r_["FN"]) and int(r_["TP_A"]) - int(r_["TP"]) == int(r_["rescued"])
    assert sum(int(r_["TP"]) for r_ in rows) > 0
    # --atomize without --alleles is refused before a file is touched
    r = subprocess.run(cmd[:-1] + ["-o", str(tmp_path / "x"), "--atomize"], capture_output=True, text=True)
    assert r.returncode != 0 and "--alleles" in r.stderr + r.stdout and not (tmp_path / "x").exists()
