"""The four rescues combined end to end (qm_extract_files_ladder, extract_many(alleles=True, ladder=), --alleles --match-ladder;
DESIGN.md 4.23): the family tests/test_gpu_normalize_files.py builds from the golden allele probe -- its VCF and truth file, a
genome synthesised so that the truth rows' REFs are its bases, respelled copies of truth indels added to the VCF -- against a
restatement on TEXT: the lines of the input and of the written *.filtered.vcf and *.tp.vcf through quasimodo_amd.ladder, the
per-sample files and the table spelled out line by line here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from quasimodo_amd import ladder as ld
from quasimodo_amd import normalize as nz
from test_gpu_normalize_files import ALLELE, CANON, TRUTH, Codes, data_lines, family, genome_of

pytestmark = pytest.mark.gpu


def restate(vcf, filtered, tp, g, truth_text, gap=None):
    """(rec, tru, the text of the ladder file) of one VCF from text: kept = the lines of filtered.vcf, TP = those of tp.vcf (both
    written in input order; a kept TP line the columns cannot tell is one the text side selected: QM_F_TPLINE), the columns
    split at tabs"""
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
    pos = [int(f[1]) if CANON.match(f[1]) else 0 for _, f in lines]
    ref, alt = [code(f[3]) for _, f in lines], [code(f[4]) for _, f in lines]
    flags = [1 * bool(k) | 2 * (f[2] == b".") | 4 * (not CANON.match(f[1])) | 8 * bool(t) for (_, f), k, t in zip(lines, kept, tpm)]
    rec, tru, mask, emask = ld.masks(g, g, truth, pos, ref, alt, flags, kept, tpm, gap=gap, subsets=True)
    out = [ld.LADDER_HEADER]
    for (no, f), b in zip(lines, mask):
        if b & ld.M_K and not b & ld.M_S:
            t = ld.tier(b)
            out.append("line\t%d\t%s\t%s\t%s\t%s\t%s" % (no, f[1].decode(), f[3].decode(), f[4].decode(), ld.set_name(b & 15), "none" if t is None else ld.METHODS[t]))
    for (p, r, a), b in zip(nz.truth_order(*truth), emask):
        if not b & ld.M_S:
            t = ld.tier(b)
            out.append("entry\t.\t%d\t%s\t%s\t%s\t%s" % (p, nz.spell(r) or ".", nz.spell(a) or ".", ld.set_name(b & 15), "none" if t is None else ld.METHODS[t]))
    return rec, tru, "\n".join(out) + "\n"


def r3(x):
    """R's round(x, 3) on a double that is no tie in these tables, as R prints it"""
    return "%.15g" % (round(x * 1000) / 1000)


def text_row(rec, tru):
    """the 60 cells of one table row from the two count rows, spelled out"""
    rec, tru = [int(x) for x in rec], [int(x) for x in tru]
    kept, tp, ent, found = rec[0], rec[1], tru[0], tru[1]
    out = []
    for k in range(5):
        low = (1 << k) - 1
        tp_k = tp + sum(rec[2 + m] for m in range(16) if m & low)
        fn_k = ent - found - sum(tru[2 + m] for m in range(16) if m & low)
        if kept == 0:
            out += ["0", "0", str(fn_k), "NA", "NA", "NA"]
            continue
        p, r = float(r3(tp_k / kept)), (float(r3((ent - fn_k) / ent)) if ent else float("nan"))
        f1 = 2 * (p * r) / (p + r) if p + r > 0 else float("nan")
        out += [str(tp_k), str(kept - tp_k), str(fn_k), r3(p), r3(r) if r == r else "NaN", r3(f1) if f1 == f1 else "NaN"]
    return out + [str(rec[2 + m]) for m in range(1, 16)] + [str(tru[2 + m]) for m in range(1, 16)]


def _jobs(vcfs, fa=None):
    from quasimodo_amd.extract import Job
    return [Job(v, TRUTH, "hcmv", "", "c", ladder=None if fa is None else 10, ladder_genome=fa) for v in vcfs]


def test_extract_many_ladder_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import _paths, extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    vcfs, fa, g, truth_text = family(tmp_path, "one")
    plain = extract_many(_jobs(family(tmp_path, "plain")[0]), engine=engine, alleles=True)
    jobs = extract_many(_jobs(vcfs), engine=engine, alleles=True, ladder=[fa] * 3)
    # without ladder= the tree is the same but for ladder/: nothing of the four passes it runs, nothing overwritten
    on, off = _tree(str(tmp_path / "one")), _tree(str(tmp_path / "plain"))
    assert off == {k: v for k, v in on.items() if not k.startswith("ladder" + os.sep)}
    assert len(on) == len(off) + 3
    rows, rescued = [], 0
    for p, j in zip(plain, jobs):
        wrec, wtru, wtext = restate(j.vcf_file, j.filtered_out, j.tp_out, g, truth_text)
        np.testing.assert_array_equal(j.stats["ladder_rec"], wrec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["ladder_tru"], wtru, err_msg=j.vcf_file)
        assert j.ladder_out == ld.ladder_path(j) and open(j.ladder_out).read() == wtext, j.vcf_file
        for k in p.stats:                                          # the rows of the plain call, unchanged
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        assert int(wrec[0]) == j.stats["tp_lines"] + j.stats["fp_lines"] and int(wrec[1]) == j.stats["tp_lines"]
        rescued += ld.cells_with(wrec, 15)
        rows.append(("c", os.path.basename(j.vcf_file).split(".")[0], j.stats))
    assert rescued >= 6
    ld.write_performance_ladder(str(tmp_path / "t1.tsv"), rows)
    text = open(str(tmp_path / "t1.tsv")).read().split("\n")
    assert text[0] == "\t".join(ld.TABLE_HEADER[0] + ld.TABLE_HEADER[1]) and text[-1] == "" and len(text) == 1 + 3 + 1 + 1
    for ln, (c, smp, st) in zip(text[1:4], rows):
        assert ln.split("\t") == [c, smp] + text_row(st["ladder_rec"], st["ladder_tru"]), smp
    pooled = [sum(np.asarray(st[k], np.uint64) for _, _, st in rows) for k in ("ladder_rec", "ladder_tru")]
    assert text[4].split("\t") == ["c", "pooled"] + text_row(*pooled)
    # sharded over two ranks of one device: the same rows, the same files
    svcfs, sfa, _, _ = family(tmp_path, "two")
    whole = _jobs(svcfs, sfa)
    for j in whole:                                                 # (whole Jobs carry the path extract_many(ladder=) derives)
        _paths(j)
        j.ladder_out = ld.ladder_path(j)
    sj, _ = extract_many_sharded(whole, 2, backend="gloo", same_device=True, alleles=True)
    assert _tree(str(tmp_path / "two")) == on
    for a, b in zip(sj, jobs):
        np.testing.assert_array_equal(a.stats["ladder_rec"], b.stats["ladder_rec"])
        np.testing.assert_array_equal(a.stats["ladder_tru"], b.stats["ladder_tru"])
    # refusals, in front of any file: without the allele-extended mode, two genomes for one truth file, beside the passes it runs
    other = tmp_path / "other.fa"
    other.write_text(">o\nACGT\n")
    for kw, said in ((dict(ladder=[fa] * 3), "--alleles"), (dict(alleles=True, ladder=[fa, str(other), fa]), "one genome"),
                     (dict(alleles=True, ladder=[fa] * 3, normalize=[fa] * 3), "does not combine"),
                     (dict(alleles=True, ladder=[fa] * 3, atomize=True), "does not combine"),
                     (dict(alleles=True, ladder=[fa] * 3, haplo={"gap": 10, "genomes": [fa] * 3}), "does not combine"),
                     (dict(alleles=True, ladder=[fa] * 3, rescue_roc=[fa] * 3), "does not combine")):
        d = tmp_path / ("r%d" % len(os.listdir(tmp_path)))
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(family(tmp_path, d.name)[0]), engine=engine, **kw)
        assert sorted(os.listdir(str(d))) == sorted(["genome.fa", "s1.c.both.vcf", "s2.c.respelled.vcf", "s3.c.probe.vcf"])


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    from test_tables_workflow import _build_bundle
    root = tmp_path_factory.mktemp("ladder")
    data = root / "data" / "snp"
    _build_bundle(str(data))
    fas = {}
    for mix in ("TM", "TA"):                                        # a genome that spells the truth rows' REFs
        text = open(os.path.join(str(data), "nucmer", "%s.maskrepeat.variants.vcf" % mix), "rb").read()
        top = max(int(f[1]) for _, f in data_lines(text) if CANON.match(f[1]))
        fas[mix] = root / ("%s.fa" % mix)
        fas[mix].write_text(">%s\n%s\n" % (mix, genome_of(text, top + 100, seed=len(fas))))
    return root, str(data), {k: str(v) for k, v in fas.items()}


MINE = lambda k: k == os.path.join("results", "final_tables", "caller_performance_ladder.tsv") or (os.sep + "ladder" + os.sep) in k


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_files_table_and_flag_off_tree(engine, bundle, gpus):
    """--alleles --match-ladder on one rank and on two: one ladder file per mixed sample and caller and one table, the same bytes;
    without the flag the same tree but for them, and nothing of the four passes it runs appears"""
    from quasimodo_amd import workflow
    from quasimodo_amd.tables import CALLER_MAP
    from test_gpu_afprofile import _tree
    root, data, fas = bundle
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    out = root / ("on%d" % gpus)
    jobs = workflow.run_hcmv_variantcall(data, str(out), alleles=True, match_ladder=fas, **kw)
    on = _tree(str(out))
    mixed = [j for j in jobs if not os.path.basename(j.vcf_file).split(".")[0].endswith(("-1-0", "-0-1"))]
    assert len([k for k in on if MINE(k)]) == len(mixed) + 1 and len(mixed) > 0
    assert not [k for k in on if any((os.sep + d + os.sep) in k for d in ("norm", "atoms", "hap")) or "normalized.tsv" in k or "atomized.tsv" in k or "haplotype.tsv" in k]
    if gpus == 2:
        assert on == _tree(str(root / "on1"))                        # (the one-rank case ran first: the same bytes)
        return
    rest = {k: v for k, v in on.items() if not MINE(k)}
    workflow.run_hcmv_variantcall(data, str(root / "off"), alleles=True, engine=engine)
    assert _tree(str(root / "off")) == rest                          # without the flag: the tree of the parent's run
    # the files and the table against the text of the inputs and of the written VCFs
    table = on[os.path.join("results", "final_tables", "caller_performance_ladder.tsv")].decode().split("\n")
    assert table[0] == "\t".join(ld.TABLE_HEADER[0] + ld.TABLE_HEADER[1]) and table[-1] == ""
    got_rows = {tuple(ln.split("\t")[:2]): ln.split("\t")[2:] for ln in table[1:-1]}
    genomes = {mix: "".join(open(fas[mix]).read().split("\n")[1:]) for mix in fas}
    pooled = {}
    for k, j in enumerate(mixed):
        base = os.path.basename(j.vcf_file)[:-4]
        smp, ref, c = base.split(".")[:3]
        rec, tru = np.asarray(j.stats["ladder_rec"], np.uint64), np.asarray(j.stats["ladder_tru"], np.uint64)
        if k < 8:                                                     # (eight jobs spelled out from text; the rest through the table)
            wrec, wtru, wtext = restate(j.vcf_file, j.filtered_out, j.tp_out, genomes[smp[:2]], open(j.snp_file, "rb").read())
            np.testing.assert_array_equal(rec, wrec, err_msg=base)
            np.testing.assert_array_equal(tru, wtru, err_msg=base)
            assert on[os.path.join("results", "snp", "callers", c, "ladder", base + ".ladder.tsv")].decode() == wtext, base
        assert got_rows[(CALLER_MAP.get(c, c), smp)] == text_row(rec, tru), base
        acc = pooled.setdefault(c, [np.zeros(18, np.uint64), np.zeros(18, np.uint64)])
        acc[0] += rec
        acc[1] += tru
    for c, (rec, tru) in pooled.items():
        assert got_rows[(CALLER_MAP.get(c, c), "pooled")] == text_row(rec, tru), c
    assert len(got_rows) == len(mixed) + len(pooled)


def test_command_line_refusals(bundle, tmp_path):
    """--match-ladder without --alleles, beside any of the passes it runs, and under vareval: said before a file is touched"""
    root, data, fas = bundle
    refs = ["--merlin-ref", fas["TM"], "--ad169-ref", fas["TA"]]
    cmd = [sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", data]
    for extra, said in ((["--match-ladder"], "--alleles"), (["--alleles", "--match-ladder", "--normalize"], "--match-ladder cannot be combined with --normalize"),
                        (["--alleles", "--match-ladder", "--haplotypes"], "--match-ladder cannot be combined with --haplotypes"),
                        (["--alleles", "--match-ladder", "--rescue-roc"], "--match-ladder cannot be combined with --rescue-roc"),
                        (["--alleles", "--match-ladder", "--atomize"], "--atomize cannot be combined with --match-ladder"),
                        (["--alleles", "--match-ladder", "--hap-gap", "40"], "--hap-gap")):
        r = subprocess.run(cmd + ["-o", str(tmp_path / "x")] + extra + refs, capture_output=True, text=True)
        assert r.returncode != 0 and said in r.stderr + r.stdout and not (tmp_path / "x").exists(), (extra, r.stderr)
    r = subprocess.run(cmd + ["-o", str(tmp_path / "d"), "--alleles", "--match-ladder", "--hap-gap", "5", "--dryrun"] + refs, capture_output=True, text=True)
    assert r.returncode == 0 and "caller_performance_ladder.tsv" in r.stdout and not (tmp_path / "d").exists(), r.stderr
    cases_dir = os.path.join(GOLDEN, "custom")
    from conftest import golden_cases
    cases = [e for e in golden_cases() if e["family"] == "custom"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", os.path.join(cases_dir, cases[0]["vcf"]), "--snps",
                        os.path.join(cases_dir, cases[0]["truth"]), "-l", "a", "-o", str(tmp_path / "v"), "--match-ladder"], capture_output=True, text=True)
    assert r.returncode != 0 and "allele-extended" in r.stderr + r.stdout and not (tmp_path / "v").exists()
