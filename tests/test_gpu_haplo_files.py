"""Clusters of records matched by replayed haplotype end to end (qm_extract_files_haplotypes, extract_many(alleles=True, haplo=),
--alleles --haplotypes): a small family built from the golden allele probe -- its VCF and truth file with rows
added behind them that carry the two shapes the pass is for (the truth set's SNV beside a deletion against the caller's one
complex row, and the reverse) and the SNV with its base changed, against a genome written by the test -- compared with a
restatement on TEXT: the lines of the written *.filtered.vcf and *.tp.vcf and the rows of the truth file through
quasimodo_amd.haplo.counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from quasimodo_amd import haplo as hp
from quasimodo_amd.normalize import DICT
from test_gpu_normalize_files import ALLELE, CANON, data_lines, genome_of

pytestmark = pytest.mark.gpu

PROBE = os.path.join(GOLDEN, "alleles", "input", "probe.vcf")
TRUTH = os.path.join(GOLDEN, "alleles", "input", "probe.truth.vcf")
R = {name: k for k, name in enumerate(hp.R_COLS)}
T = {name: k for k, name in enumerate(hp.T_COLS)}

TRUTH_ROWS = [b"c\t1300\t.\tA\tT\t30\tPASS\tTYPE=SNV", b"c\t1300\t.\tACG\tA\t30\tPASS\tTYPE=DEL",       # split here, joined by the caller
              b"c\t1400\t.\tGCA\tT\t30\tPASS\tTYPE=CPX",                                                 # joined here, split by the caller
              b"c\t1500\t.\tA\tT\t30\tPASS\tTYPE=SNV", b"c\t1500\t.\tACG\tA\t30\tPASS\tTYPE=DEL",       # ... and the caller's base is another
              b"c\t1600\t.\tC\tG\t30\tPASS\tTYPE=SNV"]                                                   # found by spelling
VCF_ROWS = [b"c\t1300\t.\tACG\tT\t50\tPASS\tDP=9",                    # rescued, and a TP_H line
            b"c\t1400\t.\tG\tT\t50\tPASS\tDP=9",                      # rescued
            b"c\t1400\trs7\tGCA\tG\t50\tPASS\tDP=9",                  # rescued, but with an ID: no TP_H line
            b"c\t1500\t.\tACG\tC\t50\tPASS\tDP=9",                    # MISMATCH
            b"c\t1600\t.\tC\tG\t50\tPASS\tDP=9",                      # matched by spelling
            b"c\t1603\t.\tT\tA\t50\tPASS\tDP=9",                      # LONE (the genome holds T at 1603: see family())
            b"c\t1700\t.\tG\tA\t50\tPASS\tDP=9",                      # OUTSIDE (G at 1700)
            b"c\t1300\t.\tACG\tT\t5\tPASS\tDP=9"]                     # not kept


def family(tmp_path, name):
    """the truth file with its added rows, the genome as FASTA, three VCFs: the probe with the added lines behind it, the added
    lines alone, the probe alone"""
    d = tmp_path / name
    d.mkdir()
    truth_text = open(TRUTH, "rb").read() + b"\n".join(TRUTH_ROWS) + b"\n"
    (d / "truth.vcf").write_bytes(truth_text)
    g = list(genome_of(truth_text, 2000))           # (the probe's own rows end at 600: the added ones stand apart from them)
    g[1602], g[1699] = "T", "G"
    g = "".join(g)
    fa = d / "genome.fa"
    fa.write_text(">c synthesised\n" + "".join(g[i:i + 60] + "\n" for i in range(0, len(g), 60)))
    probe = open(PROBE, "rb").read()
    head = b"".join(ln + b"\n" for ln in probe.split(b"\n") if ln[:1] == b"#")
    vcfs = []
    for base, text in (("s1.c.both.vcf", probe + b"\n".join(VCF_ROWS) + b"\n"), ("s2.c.added.vcf", head + b"\n".join(VCF_ROWS) + b"\n"),
                       ("s3.c.probe.vcf", probe)):
        (d / base).write_bytes(text)
        vcfs.append(str(d / base))
    return vcfs, str(d / "truth.vcf"), str(fa), g, truth_text


class Codes:
    """allele strings as codes: inline up to 13 bases, ids of this test's own dictionary beyond; -1 for what is no allele"""

    def __init__(self):
        self.ids = {}

    def __call__(self, s):
        if not ALLELE.match(s):
            return -1
        return hp.code(s.decode()) if len(s) <= hp.INLINE_MAX else DICT | self.ids.setdefault(s, len(self.ids))


def restate(vcf, filtered, tp, genome, truth_text, gap=None):
    """(rec, tru, sites) of one VCF from text: kept = the lines of filtered.vcf, TP = those of tp.vcf (a sub-sequence of them);
    sites: what read_sites returns of the job's file, the rescued lines found again in the input VCF by their text"""
    code = Codes()
    ent = [f for _, f in data_lines(truth_text) if CANON.match(f[1]) and ALLELE.match(f[3]) and ALLELE.match(f[4]) and int(f[1]) < (1 << 28)]
    truth = tuple(np.array(x, np.int32).reshape(len(ent)) for x in ([int(f[1]) for f in ent], [code(f[3]) for f in ent], [code(f[4]) for f in ent]))
    kept = [f for _, f in data_lines(open(filtered, "rb").read())]
    rest = [f for _, f in data_lines(open(tp, "rb").read())]
    n = len(kept)
    canon = [bool(CANON.match(f[1])) for f in kept]
    pos = np.array([int(f[1]) if c and int(f[1]) < (1 << 31) else 0 for f, c in zip(kept, canon)], np.int32).reshape(n)
    ref = np.array([code(f[3]) for f in kept], np.int32).reshape(n)
    alt = np.array([code(f[4]) for f in kept], np.int32).reshape(n)
    flags = np.array([hp.F_PASS | (hp.F_IDDOT if f[2] == b"." else 0) | (0 if c else hp.F_NOKEY) for f, c in zip(kept, canon)], np.uint8).reshape(n)
    tpm = np.zeros(n, bool)
    for i, f in enumerate(kept):
        if rest and rest[0] == f:
            tpm[i] = True
            rest.pop(0)
    assert not rest, tp
    detail = []
    rec, tru, cls, site, ecls = hp.counts(genome, truth, pos, ref, alt, flags, np.ones(n, bool), tpm, gap, detail)
    order = hp.truth_order(*truth)
    lines = data_lines(open(vcf, "rb").read())
    sites = []
    for s, ws, we, what, recs, ents, x, y in detail:
        if what != hp.MATCH:
            continue
        mine = {tuple(kept[i]) for i in recs}
        found = sorted((ln, f[1].decode(), f[3].decode(), f[4].decode()) for ln, f in lines if tuple(f) in mine)
        sites.append((s, ws, we, found, [(order[j][0], hp.spell(order[j][1]), hp.spell(order[j][2])) for j in ents], x, y))
    return rec, tru, sites


def _jobs(vcfs, truth, fa=None, **kw):
    from quasimodo_amd.extract import Job
    return [Job(v, truth, "hcmv", "", "c", haplo_genome=fa, **kw) for v in vcfs]


def test_extract_many_haplo_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import _paths, extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    vcfs, truth, fa, g, truth_text = family(tmp_path, "one")
    pv, pt, _, _, _ = family(tmp_path, "plain")
    plain = extract_many(_jobs(pv, pt), engine=engine, alleles=True)
    jobs = extract_many(_jobs(vcfs, truth, fa), engine=engine, alleles=True, haplo=10)
    # without haplo= the tree is the same but for hap/
    on, off = _tree(str(tmp_path / "one")), _tree(str(tmp_path / "plain"))
    assert off == {k: v for k, v in on.items() if not k.startswith("hap" + os.sep)}
    assert sorted(k for k in on if k.startswith("hap" + os.sep)) == sorted(os.path.join("hap", os.path.basename(v)[:-4] + ".sites.tsv") for v in vcfs)
    want = []
    for p, j in zip(plain, jobs):
        rec, tru, sites = restate(j.vcf_file, j.filtered_out, j.tp_out, g, truth_text)
        want.append({"hap_rec": rec, "hap_tru": tru})
        np.testing.assert_array_equal(j.stats["hap_rec"], rec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["hap_tru"], tru, err_msg=j.vcf_file)
        assert hp.read_sites(j.sites_out) == sites and j.stats["hap_gap"] == 10
        assert [int(x) for x in rec[:2]] == [j.stats["n_pass"], j.stats["tp_lines"]] and int(rec[2]) - int(rec[1]) == int(rec[3])
        for k in p.stats:                                          # the rows of the plain call, unchanged
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
    # the added lines by hand (the VCF that holds only them)
    rec, tru = jobs[1].stats["hap_rec"], jobs[1].stats["hap_tru"]
    assert [int(rec[R[c]]) for c in ("kept", "tp", "tp_h", "rescued", "open", "outside", "lone", "mismatch")] == [7, 1, 3, 2, 5, 1, 1, 1]
    assert int(tru[T["found"]]) == 1 and int(tru[T["found_h"]]) == 4 and int(tru[T["matched"]]) == 2 and int(tru[T["tried"]]) == 3
    sites = hp.read_sites(jobs[1].sites_out)
    assert [(s[3], s[4]) for s in sites] == [([(sites[0][3][0][0], "1300", "ACG", "T")], [(1300, "ACG", "A"), (1300, "A", "T")]),      # (the table's order: by key, then by code)
                                             ([(sites[1][3][0][0], "1400", "G", "T"), (sites[1][3][1][0], "1400", "GCA", "G")], [(1400, "GCA", "T")])]
    for s in sites:
        assert s[5] == s[6] and s[2] - s[1] + 1 <= hp.MAX_WINDOW
    assert sites[0][5] == g[sites[0][1] - 1:1299] + "T" + g[1302:sites[0][2]]
    # sharded over two ranks of one device: the same rows, the same files, the same table
    svcfs, struth, sfa, _, _ = family(tmp_path, "two")
    sjobs = _jobs(svcfs, struth, sfa, haplo=10)
    for j in sjobs:                                                # (the keyword derives the paths; whole Jobs carry their own)
        _paths(j)
        j.sites_out = hp.sites_path(j)
    sj, _ = extract_many_sharded(sjobs, 2, backend="gloo", same_device=True, alleles=True)
    for a, b in zip(jobs, sj):
        np.testing.assert_array_equal(a.stats["hap_rec"], np.asarray(b.stats["hap_rec"]))
        np.testing.assert_array_equal(a.stats["hap_tru"], np.asarray(b.stats["hap_tru"]))
    assert {k: v for k, v in _tree(str(tmp_path / "two")).items() if k.startswith("hap" + os.sep)} == {k: v for k, v in on.items() if k.startswith("hap" + os.sep)}
    t1, t2, t3 = tmp_path / "t1.tsv", tmp_path / "t2.tsv", tmp_path / "t3.tsv"
    name = lambda j: os.path.basename(j.vcf_file).split(".")[0]
    hp.write_performance_haplotype(str(t1), [("c", name(j), j.stats) for j in jobs])
    hp.write_performance_haplotype(str(t2), [("c", name(j), j.stats) for j in sj])
    hp.write_performance_haplotype(str(t3), [("c", name(j), w) for j, w in zip(jobs, want)])
    assert t1.read_bytes() == t2.read_bytes() == t3.read_bytes() and len(t1.read_text().split("\n")) == 5
    # another gap: one call of its own
    ov, ot, ofa, og, otext = family(tmp_path, "three")
    for j in extract_many(_jobs(ov, ot, ofa), engine=engine, alleles=True, haplo=0):
        rec, tru, sites = restate(j.vcf_file, j.filtered_out, j.tp_out, og, otext, 0)
        np.testing.assert_array_equal(j.stats["hap_rec"], rec)
        np.testing.assert_array_equal(j.stats["hap_tru"], tru)
        assert hp.read_sites(j.sites_out) == sites
    # refusals, in front of any file: without the allele-extended mode, a second pass in the call, two gaps, no genome
    for kw, said in ((dict(haplo=10), "--alleles"), (dict(alleles=True, haplo=10, fn=True), "does not combine"), (dict(alleles=True, haplo=40), "gap")):
        rv, rt, rfa, _, _ = family(tmp_path, "r%d" % len(os.listdir(tmp_path)))
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(rv, rt, rfa), engine=engine, **kw)
        assert sorted(os.listdir(os.path.dirname(rv[0]))) == ["genome.fa", "s1.c.both.vcf", "s2.c.added.vcf", "s3.c.probe.vcf", "truth.vcf"]
    rv, rt, rfa, _, _ = family(tmp_path, "gaps")
    jobs2 = _jobs(rv, rt, rfa)
    jobs2[0].haplo, jobs2[1].haplo, jobs2[2].haplo = 10, 5, 10
    with pytest.raises(ValueError, match="share one gap"):
        extract_many(jobs2, engine=engine, alleles=True)
    with pytest.raises(ValueError, match="genome"):
        extract_many(_jobs(rv, rt), engine=engine, alleles=True, haplo=10)


def test_command_line(tmp_path):
    """hcmv -e variantcall --alleles --haplotypes --hap-gap 5 writes the table and the sites files, and without the flag the same
    tree but for them"""
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    fas = {}
    for mix in ("TM", "TA"):                                        # a genome that spells the truth rows' REFs
        text = open(os.path.join(str(data), "nucmer", "%s.maskrepeat.variants.vcf" % mix), "rb").read()
        top = max(int(f[1]) for _, f in data_lines(text) if CANON.match(f[1]))
        fas[mix] = tmp_path / ("%s.fa" % mix)
        fas[mix].write_text(">%s\n%s\n" % (mix, genome_of(text, top + 100, seed=len(fas))))
    cmd = [sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data), "--alleles"]
    refs = ["--merlin-ref", str(fas["TM"]), "--ad169-ref", str(fas["TA"])]
    r = subprocess.run(cmd + ["-o", str(tmp_path / "on"), "--haplotypes", "--hap-gap", "5"] + refs, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(cmd + ["-o", str(tmp_path / "off")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    on, off = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off"))
    name = os.path.join("results", "final_tables", "caller_performance_haplotype.tsv")
    mine = lambda k: k == name or (os.sep + "hap" + os.sep) in k
    assert name in on and off == {k: v for k, v in on.items() if not mine(k)}
    lines = on[name].decode().split("\n")
    head = lines[0].split("\t")
    assert head == list(hp.TABLE_HEADER[0] + hp.TABLE_HEADER[1]) and lines[-1] == ""
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]
    whole = on[os.path.join("results", "final_tables", "caller_performance.tsv")].decode().split("\n")[1:-1]
    mixed = [w for w in whole if not w.split("\t")[1].endswith(("-1-0", "-0-1"))]
    assert len(rows) == len(mixed) > 0 and len([k for k in on if mine(k)]) == len(rows) + 1
    for r_ in rows:
        assert int(r_["TP_H"]) >= int(r_["TP"]) and int(r_["FN_H"]) <= int(r_["FN"]) and int(r_["TP_H"]) - int(r_["TP"]) == int(r_["rescued"])
    assert sum(int(r_["TP"]) for r_ in rows) > 0
    for k in on:
        if mine(k) and k != name:
            assert on[k].decode().split("\n")[0] == hp.SITES_HEADER
    # --haplotypes without --alleles, --hap-gap alone and a gap out of range are refused before a file is touched
    for args, said in ((cmd[:-1] + ["--haplotypes"] + refs, "--alleles"), (cmd + ["--hap-gap", "5"], "--haplotypes"),
                       (cmd + ["--haplotypes", "--hap-gap", "33"] + refs, "--hap-gap")):
        r = subprocess.run(args + ["-o", str(tmp_path / "x")], capture_output=True, text=True)
        assert r.returncode != 0 and said in r.stderr + r.stdout and not (tmp_path / "x").exists(), args
    # ... and so is --haplotypes under vareval, which has no allele-extended reading of a show-snps table
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", str(tmp_path / "a.vcf"), "--snps", str(tmp_path / "a.snps"),
                        "-l", "a", "-o", str(tmp_path / "v"), "--haplotypes"], capture_output=True, text=True)
    assert r.returncode != 0 and "--haplotypes" in r.stderr + r.stdout and "allele-extended" in r.stderr + r.stdout and not (tmp_path / "v").exists()
