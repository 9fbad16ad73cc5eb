"""The subset search behind the haplotype pass end to end (qm_extract_files_hapsubsets, extract_many(alleles=True, haplo=g,
hapsub=True), --alleles --haplotypes --hap-subsets): a small family built from the golden allele probe, as
tests/test_gpu_haplo_files.py builds its own -- rows behind the probe's that make a MISMATCH site with a partial match (the
respelled pair beside an unrelated SNV line), a MISMATCH site without one, a CONFLICT site of two overlapping lines of which one
alone spells the truth, and a MATCH site -- compared with a restatement on TEXT: the lines of the written *.filtered.vcf and
*.tp.vcf and the rows of the truth file through quasimodo_amd.haplo.counts and subset_counts.  One rank, two ranks and the command
line; what --haplotypes alone writes stays byte for byte what it was, and without either flag so does the tree."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from quasimodo_amd import haplo as hp
from test_gpu_haplo_files import PROBE, TRUTH, Codes
from test_gpu_normalize_files import ALLELE, CANON, data_lines, genome_of

pytestmark = pytest.mark.gpu

U = {name: k for k, name in enumerate(hp.SUB_COLS)}

TRUTH_ROWS = [b"c\t1300\t.\tA\tT\t30\tPASS\tTYPE=SNV", b"c\t1300\t.\tACG\tA\t30\tPASS\tTYPE=DEL",       # split here, joined by the caller
              b"c\t1400\t.\tGCA\tT\t30\tPASS\tTYPE=CPX",                                                 # joined here, split by the caller
              b"c\t1500\t.\tA\tT\t30\tPASS\tTYPE=SNV", b"c\t1500\t.\tACG\tA\t30\tPASS\tTYPE=DEL",       # ... and the caller's base is another
              b"c\t1600\t.\tC\tG\t30\tPASS\tTYPE=SNV",                                                   # found by spelling
              b"c\t1800\t.\tACG\tA\t30\tPASS\tTYPE=DEL"]                                                 # respelled by the caller, beside an overlapping line
VCF_ROWS = [b"c\t1300\t.\tACG\tT\t50\tPASS\tDP=9",                    # rescued by subset, a TP_S line
            b"c\t1305\t.\tC\tT\t50\tPASS\tDP=9",                      # the unrelated SNV 5 bases on: left (C at 1305: see family())
            b"c\t1400\t.\tG\tT\t50\tPASS\tDP=9",                      # a MATCH site: not searched
            b"c\t1400\trs7\tGCA\tG\t50\tPASS\tDP=9",
            b"c\t1500\t.\tACG\tC\t50\tPASS\tDP=9",                    # MISMATCH, and no subset
            b"c\t1600\t.\tC\tG\t50\tPASS\tDP=9",                      # matched by spelling
            b"c\t1799\trs8\tTACG\tTA\t50\tPASS\tDP=9",                # rescued by subset out of a CONFLICT site, but with an ID: no TP_S line (T at 1799)
            b"c\t1802\t.\tG\tT\t50\tPASS\tDP=9",                      # ... the line that overlaps it: left
            b"c\t1300\t.\tACG\tT\t5\tPASS\tDP=9"]                     # not kept


def family(tmp_path, name):
    d = tmp_path / name
    d.mkdir()
    truth_text = open(TRUTH, "rb").read() + b"\n".join(TRUTH_ROWS) + b"\n"
    (d / "truth.vcf").write_bytes(truth_text)
    g = list(genome_of(truth_text, 2000))
    g[1304], g[1798] = "C", "T"
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


def restate(vcf, filtered, tp, genome, truth_text, gap=None):
    """(rec, tru, sub, the rows read_subsets must return) of one VCF from text: kept = the lines of filtered.vcf, TP = those of
    tp.vcf (a sub-sequence of them); the lines of a row found again in the input VCF by their text"""
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
    tried, chosen = [], []
    res = hp.counts(genome, truth, pos, ref, alt, flags, np.ones(n, bool), tpm, gap, tried)
    sub, _, _ = hp.subset_counts(genome, truth, pos, ref, alt, flags, np.ones(n, bool), tpm, gap, chosen, counted=(res, tried))
    order = hp.truth_order(*truth)
    lines = data_lines(open(vcf, "rb").read())
    window = {d[0]: (d[1], d[2]) for d in tried}
    found = lambda idx: sorted((ln, f[1].decode(), f[3].decode(), f[4].decode()) for ln, f in lines if tuple(f) in {tuple(kept[i]) for i in idx})
    entry = lambda idx: [(order[j][0], hp.spell(order[j][1]), hp.spell(order[j][2])) for j in idx]
    rows = [(s,) + window[s] + (found(inr), found(outr), entry(ine), entry(oute), x, x) for s, ms, mt, inr, outr, ine, oute, x in chosen]
    return res[0], res[1], sub, rows


def _jobs(vcfs, truth, fa=None, **kw):
    from quasimodo_amd.extract import Job
    return [Job(v, truth, "hcmv", "", "c", haplo_genome=fa, **kw) for v in vcfs]


def test_extract_many_hapsub_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import _paths, extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    vcfs, truth, fa, g, truth_text = family(tmp_path, "one")
    hv, ht, hfa, _, _ = family(tmp_path, "hap")
    pv, pt, _, _, _ = family(tmp_path, "plain")
    extract_many(_jobs(pv, pt), engine=engine, alleles=True)
    hjobs = extract_many(_jobs(hv, ht, hfa), engine=engine, alleles=True, haplo=10)
    jobs = extract_many(_jobs(vcfs, truth, fa), engine=engine, alleles=True, haplo=10, hapsub=True)
    on, hap, off = _tree(str(tmp_path / "one")), _tree(str(tmp_path / "hap")), _tree(str(tmp_path / "plain"))
    subs = lambda k: k.endswith(".subsets.tsv")
    assert hap == {k: v for k, v in on.items() if not subs(k)}                # what haplo= alone writes, byte for byte: the sites files too
    assert off == {k: v for k, v in on.items() if not k.startswith("hap" + os.sep)}
    assert sorted(k for k in on if subs(k)) == sorted(os.path.join("hap", os.path.basename(v)[:-4] + ".subsets.tsv") for v in vcfs)
    want = []
    for h, j in zip(hjobs, jobs):
        rec, tru, sub, rows = restate(j.vcf_file, j.filtered_out, j.tp_out, g, truth_text)
        want.append({"hap_rec": rec, "hap_tru": tru, "hap_sub": sub})
        np.testing.assert_array_equal(j.stats["hap_rec"], rec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["hap_tru"], tru, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["hap_sub"], sub, err_msg=j.vcf_file)
        assert hp.read_subsets(j.subsets_out) == rows and j.stats["hap_gap"] == 10
        for k in h.stats:                                          # the rows of the haplotype call, unchanged
            assert np.array_equal(h.stats[k], j.stats[k]) if isinstance(h.stats[k], np.ndarray) else h.stats[k] == j.stats[k], k
    # the added lines by hand (the VCF that holds only them): three searched sites, two of them PARTIAL
    sub = jobs[1].stats["hap_sub"]
    rec, tru = jobs[1].stats["hap_rec"], jobs[1].stats["hap_tru"]
    assert [int(sub[U[c]]) for c in ("searched", "partial", "nosubset", "rescued_s", "left_lines", "left_entries")] == [3, 2, 1, 2, 2, 0]
    assert int(sub[U["tp_s"]]) == int(rec[2]) + 1 and int(sub[U["found_s"]]) == int(tru[2]) + 3        # rs8 is no TP_S line
    rows = hp.read_subsets(jobs[1].subsets_out)
    assert [(r[3], r[4], r[5], r[6]) for r in rows] == [
        ([(rows[0][3][0][0], "1300", "ACG", "T")], [(rows[0][4][0][0], "1305", "C", "T")], [(1300, "ACG", "A"), (1300, "A", "T")], []),
        ([(rows[1][3][0][0], "1799", "TACG", "TA")], [(rows[1][4][0][0], "1802", "G", "T")], [(1800, "ACG", "A")], [])]
    for r in rows:
        assert r[7] == r[8] and r[2] - r[1] + 1 <= hp.MAX_WINDOW
    assert rows[0][7] == g[rows[0][1] - 1:1299] + "T" + g[1302:rows[0][2]]
    assert not hp.read_subsets(jobs[2].subsets_out)                # the probe alone: a header and no row
    # sharded over two ranks of one device: the same rows, the same files, the same table
    svcfs, struth, sfa, _, _ = family(tmp_path, "two")
    sjobs = _jobs(svcfs, struth, sfa, hapsub=10)                  # (Job.hapsub: the gap, in place of Job.haplo)
    for j in sjobs:                                                # (the keywords derive the paths; whole Jobs carry their own)
        _paths(j)
        j.sites_out, j.subsets_out = hp.sites_path(j), hp.subsets_path(j)
    sj, _ = extract_many_sharded(sjobs, 2, backend="gloo", same_device=True, alleles=True)
    for a, b in zip(jobs, sj):
        for k in ("hap_rec", "hap_tru", "hap_sub"):
            np.testing.assert_array_equal(a.stats[k], np.asarray(b.stats[k]))
    assert {k: v for k, v in _tree(str(tmp_path / "two")).items() if k.startswith("hap" + os.sep)} == {k: v for k, v in on.items() if k.startswith("hap" + os.sep)}
    t1, t2, t3 = tmp_path / "t1.tsv", tmp_path / "t2.tsv", tmp_path / "t3.tsv"
    name = lambda j: os.path.basename(j.vcf_file).split(".")[0]
    hp.write_performance_hapsubsets(str(t1), [("c", name(j), j.stats) for j in jobs])
    hp.write_performance_hapsubsets(str(t2), [("c", name(j), j.stats) for j in sj])
    hp.write_performance_hapsubsets(str(t3), [("c", name(j), w) for j, w in zip(jobs, want)])
    assert t1.read_bytes() == t2.read_bytes() == t3.read_bytes() and len(t1.read_text().split("\n")) == 5
    # refusals, in front of any file: without the gap and genomes of the pass, without the allele-extended mode, another pass in the call
    for kw, said in ((dict(alleles=True, hapsub=True), "needs haplo="), (dict(haplo=10, hapsub=True), "--alleles"),
                     (dict(alleles=True, haplo=10, hapsub=True, atomize=True), "does not combine"), (dict(alleles=True, haplo=40, hapsub=True), "gap")):
        rv, rt, rfa, _, _ = family(tmp_path, "r%d" % len(os.listdir(tmp_path)))
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(rv, rt, rfa), engine=engine, **kw)
        assert sorted(os.listdir(os.path.dirname(rv[0]))) == ["genome.fa", "s1.c.both.vcf", "s2.c.added.vcf", "s3.c.probe.vcf", "truth.vcf"]
    rv, rt, rfa, _, _ = family(tmp_path, "lonely")
    both = _jobs(rv, rt, rfa)
    both[0].hapsub, both[1].haplo = 10, 10                         # the pass alone for one job, with the search for another: two calls
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(both, engine=engine, alleles=True)
    gaps = _jobs(rv, rt, rfa)
    gaps[0].hapsub, gaps[1].hapsub = 10, 5
    with pytest.raises(ValueError, match="share one gap"):
        extract_many(gaps, engine=engine, alleles=True)
    with pytest.raises(ValueError, match="genome"):
        extract_many(_jobs(rv, rt), engine=engine, alleles=True, haplo=10, hapsub=True)


def test_command_line(tmp_path):
    """hcmv -e variantcall --alleles --hap-subsets (which implies --haplotypes) writes the table and the subsets files beside
    what --haplotypes writes, byte for byte; without either flag the same tree but for all of them"""
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
    for out, flags in (("sub", ["--hap-subsets", "--hap-gap", "5"] + refs), ("hap", ["--haplotypes", "--hap-gap", "5"] + refs), ("off", [])):
        r = subprocess.run(cmd + ["-o", str(tmp_path / out)] + flags, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    sub, hap, off = _tree(str(tmp_path / "sub")), _tree(str(tmp_path / "hap")), _tree(str(tmp_path / "off"))
    name = os.path.join("results", "final_tables", "caller_performance_hapsubsets.tsv")
    hname = os.path.join("results", "final_tables", "caller_performance_haplotype.tsv")
    mine = lambda k: k == name or k.endswith(".subsets.tsv")
    theirs = lambda k: k == hname or (os.sep + "hap" + os.sep) in k
    assert name in sub and hname in sub
    assert hap == {k: v for k, v in sub.items() if not mine(k)}                 # the haplotype table and the sites files: byte-identical
    assert off == {k: v for k, v in sub.items() if not mine(k) and not theirs(k)}
    lines = sub[name].decode().split("\n")
    head = lines[0].split("\t")
    assert head == list(hp.SUBSETS_TABLE_HEADER[0] + hp.SUBSETS_TABLE_HEADER[1]) and lines[-1] == ""
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]
    hrows = sub[hname].decode().split("\n")[1:-1]
    assert len(rows) == len(hrows) > 0 and len([k for k in sub if mine(k)]) == len(rows) + 1
    for r_, h_ in zip(rows, hrows):
        assert "\t".join(r_[k] for k in head[:14]) == "\t".join(h_.split("\t")[:14])
        assert int(r_["TP_S"]) >= int(r_["TP_H"]) and int(r_["FN_S"]) <= int(r_["FN_H"])
        assert int(r_["sites_searched"]) == int(r_["sites_partial"]) + int(r_["sites_nosubset"])
    for k in sub:
        if k.endswith(".subsets.tsv"):
            assert sub[k].decode().split("\n")[0] == hp.SUBSETS_HEADER
    r = subprocess.run(cmd + ["-o", str(tmp_path / "dry"), "--hap-subsets", "--dryrun"] + refs, capture_output=True, text=True)
    assert r.returncode == 0 and "caller_performance_hapsubsets.tsv" in r.stdout and "caller_performance_haplotype.tsv" in r.stdout
    # --hap-subsets without --alleles is refused before a file is touched; so is the flag under vareval
    r = subprocess.run(cmd[:-1] + ["--hap-subsets", "-o", str(tmp_path / "x")] + refs, capture_output=True, text=True)
    assert r.returncode != 0 and "--alleles" in r.stderr + r.stdout and not (tmp_path / "x").exists()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", str(tmp_path / "a.vcf"), "--snps", str(tmp_path / "a.snps"),
                        "-l", "a", "-o", str(tmp_path / "v"), "--hap-subsets"], capture_output=True, text=True)
    assert r.returncode != 0 and "--hap-subsets" in r.stderr + r.stdout and "allele-extended" in r.stderr + r.stdout and not (tmp_path / "v").exists()
