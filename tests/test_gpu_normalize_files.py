"""Indels and MNPs matched by normal form end to end (qm_extract_files_normalize, extract_many(alleles=True, normalize=),
--alleles --normalize): a small family built from the golden allele probe -- its VCF and truth file, a genome
synthesised so that the truth rows' REFs are its bases, respelled copies of truth indels added to the VCF -- against a restatement
on TEXT: the lines of the input and of the written *.filtered.vcf and *.tp.vcf through the Python normaliser."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from quasimodo_amd import normalize as nz

pytestmark = pytest.mark.gpu

PROBE = os.path.join(GOLDEN, "alleles", "input", "probe.vcf")
TRUTH = os.path.join(GOLDEN, "alleles", "input", "probe.truth.vcf")
ALLELE = re.compile(rb"^[ACGT]+$")
CANON = re.compile(rb"^(0|[1-9][0-9]{0,8})$")


def data_lines(text):
    """[(1-based line number, fields)] of the data lines"""
    return [(i + 1, ln.split(b"\t")) for i, ln in enumerate(text.split(b"\n")) if ln and ln[:1] != b"#"]


def genome_of(truth_text, length=800, seed=3):
    """random bases with the REF of every truth row that has one at its POS: derived from the truth rows alone"""
    rng = np.random.default_rng(seed)
    g = [b"ACGT"[i:i + 1] for i in rng.integers(0, 4, length)]
    for _, f in data_lines(truth_text):
        if ALLELE.match(f[3]) and CANON.match(f[1]):
            for k in range(len(f[3])):
                g[int(f[1]) - 1 + k] = f[3][k:k + 1]
    return b"".join(g).decode()


class Codes:
    """allele strings as codes: inline up to 13 bases, ids of this test's own dictionary beyond; -1 for what is no allele"""

    def __init__(self):
        self.ids = {}

    def __call__(self, s):
        if not ALLELE.match(s):
            return -1
        if len(s) <= nz.INLINE_MAX:
            return nz.code(s.decode())
        return nz.DICT | self.ids.setdefault(s, len(self.ids))


def family(tmp_path, name):
    """the truth file, the genome as FASTA, three VCFs: the probe with respelled truth indels behind it, the respellings alone,
    the probe alone"""
    d = tmp_path / name
    d.mkdir()
    truth_text = open(TRUTH, "rb").read()
    g = genome_of(truth_text)
    fa = d / "genome.fa"
    fa.write_text(">c synthesised\n" + "".join(g[i:i + 60] + "\n" for i in range(0, len(g), 60)))
    extra = []
    for _, f in data_lines(truth_text):
        if not (ALLELE.match(f[3]) and ALLELE.match(f[4])) or len(f[3]) == len(f[4]) == 1 or max(len(f[3]), len(f[4])) > 11:
            continue
        p, r, a = int(f[1]), f[3].decode(), f[4].decode()
        right, left = g[p - 1 + len(r)], g[p - 2]
        extra.append(b"c\t%d\t.\t%s\t%s\t50\tPASS\tDP=9" % (p, (r + right).encode(), (a + right).encode()))          # one more shared base behind
        extra.append(b"c\t%d\trs1\t%s\t%s\t50\tPASS\tDP=9" % (p - 1, (left + r).encode(), (left + a).encode()))      # in front, with an ID
        c, q, r2, a2 = nz.normalize(g, p, r, a)
        if (q, r2, a2) != (p, r, a):
            extra.append(b"c\t%d\t.\t%s\t%s\t50\tPASS\tDP=9" % (q, r2.encode(), a2.encode()))                         # the normal form itself
    assert len(extra) >= 6
    probe = open(PROBE, "rb").read()
    head = b"".join(ln + b"\n" for ln in probe.split(b"\n") if ln[:1] == b"#")
    vcfs = []
    for base, text in (("s1.c.both.vcf", probe + b"\n".join(extra) + b"\n"), ("s2.c.respelled.vcf", head + b"\n".join(extra) + b"\n"),
                       ("s3.c.probe.vcf", probe)):
        (d / base).write_bytes(text)
        vcfs.append(str(d / base))
    return vcfs, str(fa), g, truth_text


def restate(vcf, filtered, tp, g, truth_text):
    """(rec, tru, rescued rows) of one VCF from text: kept = the lines of filtered.vcf, TP = those of tp.vcf (both written in
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
    rec, tru, cls, npos, nref, nalt, row = nz.counts(g, truth, pos, ref, alt, flags, kept, tpm)
    order = nz.truth_order(*truth)
    rescued = []
    for i, (no, f) in enumerate(lines):
        if cls[i] == nz.RESCUED:
            e = order[row[i]]
            rescued.append((no, (f[1].decode(), f[3].decode(), f[4].decode()), (int(npos[i]), nz.spell(nref[i]), nz.spell(nalt[i])),
                            (e[0], nz.spell(e[1]), nz.spell(e[2]))))
    return rec, tru, rescued


def _jobs(vcfs, fa=None):
    from quasimodo_amd.extract import Job
    return [Job(v, TRUTH, "hcmv", "", "c", normalize=fa) for v in vcfs]


def test_extract_many_normalize_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import _paths, extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    vcfs, fa, g, truth_text = family(tmp_path, "one")
    plain = extract_many(_jobs(family(tmp_path, "plain")[0]), engine=engine, alleles=True)
    jobs = extract_many(_jobs(vcfs), engine=engine, alleles=True, normalize={"genomes": [fa] * 3})
    # without normalize= the tree is the same but for norm/
    on, off = _tree(str(tmp_path / "one")), _tree(str(tmp_path / "plain"))
    assert off == {k: v for k, v in on.items() if not k.startswith("norm" + os.sep)}
    assert sorted(k for k in on if k.startswith("norm" + os.sep)) == sorted(os.path.join("norm", os.path.basename(v)[:-4] + ".rescued.tsv") for v in vcfs)
    n_rescued = 0
    for p, j in zip(plain, jobs):
        rec, tru, rescued = restate(j.vcf_file, j.filtered_out, j.tp_out, g, truth_text)
        np.testing.assert_array_equal(j.stats["norm_rec"], rec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["norm_tru"], tru, err_msg=j.vcf_file)
        assert nz.read_rescued(j.rescued_out) == rescued
        assert [int(x) for x in rec[:2]] == [j.stats["n_pass"], j.stats["tp_lines"]] and int(rec[2]) >= int(rec[1])
        n_rescued += len(rescued)
        for k in p.stats:                                          # the rows of the plain call, unchanged
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
    assert n_rescued >= 6
    assert int(jobs[1].stats["norm_rec"][3]) > 0 and int(jobs[1].stats["norm_tru"][3]) > 0
    # sharded over two ranks of one device: the same rows, the same files, the same table
    svcfs, sfa, _, _ = family(tmp_path, "two")
    sj = _jobs(svcfs, sfa)
    for j in sj:
        _paths(j)
        j.rescued_out = nz.rescued_path(j)
    sj, _ = extract_many_sharded(sj, 2, backend="gloo", same_device=True, alleles=True)
    two = _tree(str(tmp_path / "two"))
    assert {k: two.get(k) for k in on} == on
    for a, b in zip(jobs, sj):
        np.testing.assert_array_equal(a.stats["norm_rec"], np.asarray(b.stats["norm_rec"]))
        np.testing.assert_array_equal(a.stats["norm_tru"], np.asarray(b.stats["norm_tru"]))
    t1, t2 = tmp_path / "t1.tsv", tmp_path / "t2.tsv"
    nz.write_performance_normalized(str(t1), [("c", os.path.basename(j.vcf_file).split(".")[0], j.stats) for j in jobs])
    nz.write_performance_normalized(str(t2), [("c", os.path.basename(j.vcf_file).split(".")[0], j.stats) for j in sj])
    assert t1.read_bytes() == t2.read_bytes() and len(t1.read_text().split("\n")) == 5
    # refusals, in front of any file: without the allele-extended mode, two genomes for one truth file, a second pass in the call
    other = tmp_path / "other.fa"
    other.write_text(">o\nACGT\n")
    for kw, said in ((dict(normalize=[fa] * 3), "--alleles"), (dict(alleles=True, normalize=[fa, str(other), fa]), "one genome"),
                     (dict(alleles=True, normalize=[fa] * 3, fn=True), "does not combine")):
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(family(tmp_path, "r%d" % len(os.listdir(tmp_path)))[0]), engine=engine, **kw)


def test_command_line(tmp_path):
    """hcmv -e variantcall --alleles --normalize writes the table and the rescued-lines files, and without the two flags the same
    tree but for them; vareval --normalize says why it has none"""
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    fas = {}
    for mix in ("TM", "TA"):                                        # a genome that spells the truth rows' REFs
        text = open(os.path.join(str(data), "nucmer", "%s.maskrepeat.variants.vcf" % mix), "rb").read()
        top = max(int(f[1]) for _, f in data_lines(text) if CANON.match(f[1]))
        g = genome_of(text, top + 100, seed=len(fas))
        fas[mix] = tmp_path / ("%s.fa" % mix)
        fas[mix].write_text(">%s\n%s\n" % (mix, g))
    cmd = [sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data), "--alleles"]
    r = subprocess.run(cmd + ["-o", str(tmp_path / "on"), "--normalize", "--merlin-ref", str(fas["TM"]), "--ad169-ref", str(fas["TA"])],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(cmd + ["-o", str(tmp_path / "off")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    on, off = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off"))
    name = os.path.join("results", "final_tables", "caller_performance_normalized.tsv")
    mine = lambda k: k == name or (os.sep + "norm" + os.sep) in k
    assert name in on and off == {k: v for k, v in on.items() if not mine(k)}
    lines = on[name].decode().split("\n")
    head = lines[0].split("\t")
    assert head == list(nz.TABLE_HEADER[0] + nz.TABLE_HEADER[1]) and lines[-1] == ""
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]
    whole = on[os.path.join("results", "final_tables", "caller_performance.tsv")].decode().split("\n")[1:-1]
    mixed = [w for w in whole if not w.split("\t")[1].endswith(("-1-0", "-0-1"))]
    assert len(rows) == len(mixed) > 0 and len([k for k in on if mine(k)]) == len(rows) + 1
    for r_ in rows:
        assert int(r_["TP_N"]) >= int(r_["TP"]) and int(r_["FN_N"]) <= int(r_["FN"]) and int(r_["TP_N"]) - int(r_["TP"]) == int(r_["rescued"])
    assert sum(int(r_["TP"]) for r_ in rows) > 0
    # --normalize without --alleles is refused before a file is touched; vareval has no allele-extended mode to normalise
    r = subprocess.run(cmd[:-1] + ["-o", str(tmp_path / "x"), "--normalize", "--merlin-ref", str(fas["TM"]), "--ad169-ref", str(fas["TA"])],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "--alleles" in r.stderr + r.stdout and not (tmp_path / "x").exists()
    cases_dir = os.path.join(GOLDEN, "custom")
    from conftest import golden_cases
    cases = [e for e in golden_cases() if e["family"] == "custom"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", os.path.join(cases_dir, cases[0]["vcf"]), "--snps",
                        os.path.join(cases_dir, cases[0]["truth"]), "-l", "a", "-o", str(tmp_path / "v"), "--normalize"], capture_output=True, text=True)
    assert r.returncode != 0 and "allele-extended" in r.stderr + r.stdout and not (tmp_path / "v").exists()
