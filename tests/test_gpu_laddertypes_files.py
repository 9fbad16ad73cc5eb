"""The match ladder per variant type and size end to end (qm_extract_files_ladder_types, extract_many(alleles=True,
ladder_types=), --alleles --ladder-by-type): the family tests/test_gpu_normalize_files.py builds from the golden
allele probe against a restatement on TEXT -- the lines of the input and of the written *.filtered.vcf and *.tp.vcf through
quasimodo_amd.ladder for the bytes, the REF and ALT strings through vartype.shape for the rows, the table spelled out cell by cell
here --, on one rank and on two with identical tables; the tree without the flag; the refusals of the command line."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from quasimodo_amd import ladder as ld
from quasimodo_amd import laddertypes as lt
from quasimodo_amd import normalize as nz
from quasimodo_amd import vartype as vt
from test_gpu_normalize_files import ALLELE, CANON, TRUTH, Codes, data_lines, family, genome_of
from test_gpu_vartype_files import text_row as type_of_text

pytestmark = pytest.mark.gpu

EDGES = (1, 2, 6)
NR = vt.n_rows(EDGES)
TABLE = os.path.join("results", "final_tables", "caller_performance_ladder_types.tsv")


def restate(vcf, filtered, tp, g, truth_text, gap=None, edges=EDGES):
    """(rec, tru) [n_rows][18] of one VCF from text: kept = the lines of filtered.vcf, TP = those of tp.vcf (both written in input
    order; a kept TP line the columns cannot tell is one the text side selected: QM_F_TPLINE); the bytes through ladder.masks, the
    row of a line and of a truth row from its REF and ALT strings"""
    code = Codes()
    tr = [f for _, f in data_lines(truth_text) if CANON.match(f[1]) and ALLELE.match(f[3]) and ALLELE.match(f[4])]
    truth = ([int(f[1]) for f in tr], [code(f[3]) for f in tr], [code(f[4]) for f in tr])
    text_of = {(int(f[1]), code(f[3]), code(f[4])): f for f in tr}
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
    _, _, mask, emask = ld.masks(g, g, truth, pos, ref, alt, flags, kept, tpm, gap=gap, subsets=True)
    rows = [type_of_text(f[1], f[3], f[4], edges) for _, f in lines]
    erows = []
    for e in nz.truth_order(*truth):
        f = text_of[e]
        erows.append(type_of_text(f[1], f[3], f[4], edges))
    return lt.counts(mask, emask, rows, erows, vt.n_rows(edges))


def r3(x):
    """R's round(x, 3) of a double as R prints it: the exact value of the double (a Fraction: 63 / 80 as a double lies below the
    tie 0.7875 and goes down), half to even where it is a tie itself"""
    q = Fraction(x) * 1000
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return "%.15g" % (n / 1000)


def ladder_text_row(rec, tru):
    """the 30 cells of one row -- TP, FP, FN, Precision, Recall, F1 by spelling and after each of the four tiers -- from its two
    count rows, spelled out"""
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
        p = float(r3(tp_k / kept))
        r = float(r3((ent - fn_k) / ent)) if ent else float("nan")
        f1 = 2 * (p * r) / (p + r) if p + r > 0 else float("nan")
        out += [str(tp_k), str(kept - tp_k), str(fn_k), r3(p), r3(r) if r == r else "NaN", r3(f1) if f1 == f1 else "NaN"]
    return out


def text_table(rec, tru, edges=EDGES):
    """the rows of one block of the table from the two count blocks, spelled out: [type, size] + 30 cells"""
    rec, tru = np.asarray(rec).astype(np.int64), np.asarray(tru).astype(np.int64)
    nb, lab, out = len(edges), vt.size_labels(edges), []
    for t, name in enumerate(vt.TYPE_NAMES):
        for b in range(nb):
            out.append([name, lab[b]] + ladder_text_row(rec[t * nb + b], tru[t * nb + b])[:30])
        out.append([name, "all"] + ladder_text_row(rec[t * nb:(t + 1) * nb].sum(axis=0), tru[t * nb:(t + 1) * nb].sum(axis=0))[:30])
    for x, name in enumerate(vt.OFFGRID_NAMES):
        cells = ladder_text_row(rec[5 * nb + x], tru[5 * nb + x])[:30]
        for k in range(5):                                             # behind the grid: plain counts, the ratios NA
            r, u = [int(v) for v in rec[5 * nb + x]], [int(v) for v in tru[5 * nb + x]]
            low = (1 << k) - 1
            tp_k = r[1] + sum(r[2 + m] for m in range(16) if m & low)
            cells[6 * k:6 * k + 6] = [str(tp_k), str(r[0] - tp_k), str(u[0] - u[1] - sum(u[2 + m] for m in range(16) if m & low)), "NA", "NA", "NA"]
        out.append([name, "NA"] + cells)
    return out


def _jobs(vcfs, fa=None):
    from quasimodo_amd.extract import Job
    return [Job(v, TRUTH, "hcmv", "", "c", ladder_types=None if fa is None else (10, EDGES), ladder_types_genome=fa) for v in vcfs]


def test_extract_many_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    vcfs, fa, g, truth_text = family(tmp_path, "one")
    plain = extract_many(_jobs(family(tmp_path, "plain")[0]), engine=engine, alleles=True)
    jobs = extract_many(_jobs(vcfs), engine=engine, alleles=True, ladder_types={"genomes": [fa] * 3, "edges": EDGES})
    # the pass writes no file of its own: without ladder_types= the tree is the same, byte for byte
    on = _tree(str(tmp_path / "one"))
    assert on == _tree(str(tmp_path / "plain"))
    rows, rescued = [], 0
    for p, j in zip(plain, jobs):
        wrec, wtru = restate(j.vcf_file, j.filtered_out, j.tp_out, g, truth_text)
        np.testing.assert_array_equal(j.stats["ladder_types_rec"], wrec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["ladder_types_tru"], wtru, err_msg=j.vcf_file)
        assert j.stats["ladder_types_edges"] == EDGES
        lt.identities(wrec, wtru, edges=EDGES)
        for k in p.stats:                                          # the rows of the plain call, unchanged
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        assert int(wrec[:, 0].sum()) == j.stats["tp_lines"] + j.stats["fp_lines"] and int(wrec[:, 1].sum()) == j.stats["tp_lines"]
        rescued += int(wrec[:, 3:].sum())
        rows.append(("c", os.path.basename(j.vcf_file).split(".")[0], j.stats))
    assert rescued >= 6
    assert sum(1 for r in jobs[0].stats["ladder_types_rec"] if r[3:].any()) >= 2           # rescued lines in several rows
    lt.write_performance_ladder_types(str(tmp_path / "t1.tsv"), rows, EDGES)
    text = open(str(tmp_path / "t1.tsv")).read().split("\n")
    per = 5 * (len(EDGES) + 1) + 4
    assert text[0] == "\t".join(lt.TABLE_HEADER) and text[-1] == "" and len(text) == 1 + 4 * per + 1
    for k, (c, smp, st) in enumerate(rows):
        want = text_table(st["ladder_types_rec"], st["ladder_types_tru"])
        assert [ln.split("\t") for ln in text[1 + k * per:1 + (k + 1) * per]] == [[c, smp] + r for r in want], smp
    pooled = [sum(np.asarray(st[k], np.uint64) for _, _, st in rows) for k in ("ladder_types_rec", "ladder_types_tru")]
    assert [ln.split("\t") for ln in text[1 + 3 * per:1 + 4 * per]] == [["c", "pooled"] + r for r in text_table(*pooled)]
    # sharded over two ranks of one device: the same blocks, the same table, the same files
    svcfs, sfa, _, _ = family(tmp_path, "two")
    sj, _ = extract_many_sharded(_jobs(svcfs, sfa), 2, backend="gloo", same_device=True, alleles=True)
    assert _tree(str(tmp_path / "two")) == on
    for a, b in zip(sj, jobs):
        np.testing.assert_array_equal(a.stats["ladder_types_rec"], b.stats["ladder_types_rec"])
        np.testing.assert_array_equal(a.stats["ladder_types_tru"], b.stats["ladder_types_tru"])
    lt.write_performance_ladder_types(str(tmp_path / "t2.tsv"), [("c", os.path.basename(j.vcf_file).split(".")[0], j.stats) for j in sj], EDGES)
    assert open(str(tmp_path / "t2.tsv"), "rb").read() == open(str(tmp_path / "t1.tsv"), "rb").read()
    # refusals, in front of any file: without the allele-extended mode, two genomes for one truth file, beside the passes it runs
    other = tmp_path / "other.fa"
    other.write_text(">o\nACGT\n")
    for kw, said in ((dict(ladder_types=[fa] * 3), "--alleles"), (dict(alleles=True, ladder_types=[fa, str(other), fa]), "one genome"),
                     (dict(alleles=True, ladder_types=[fa] * 3, ladder=[fa] * 3), "does not combine"),
                     (dict(alleles=True, ladder_types=[fa] * 3, vartype=True), "does not combine"),
                     (dict(alleles=True, ladder_types=[fa] * 3, normalize=[fa] * 3), "does not combine")):
        d = tmp_path / ("r%d" % len(os.listdir(tmp_path)))
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(family(tmp_path, d.name)[0]), engine=engine, **kw)
        assert sorted(os.listdir(str(d))) == sorted(["genome.fa", "s1.c.both.vcf", "s2.c.respelled.vcf", "s3.c.probe.vcf"])


@pytest.fixture(scope="module")
def bundle(tmp_path_factory):
    from test_tables_workflow import _build_bundle
    root = tmp_path_factory.mktemp("laddertypes")
    data = root / "data" / "snp"
    _build_bundle(str(data))
    fas = {}
    for mix in ("TM", "TA"):                                        # a genome that spells the truth rows' REFs
        text = open(os.path.join(str(data), "nucmer", "%s.maskrepeat.variants.vcf" % mix), "rb").read()
        top = max(int(f[1]) for _, f in data_lines(text) if CANON.match(f[1]))
        fas[mix] = root / ("%s.fa" % mix)
        fas[mix].write_text(">%s\n%s\n" % (mix, genome_of(text, top + 100, seed=len(fas))))
    return root, str(data), {k: str(v) for k, v in fas.items()}


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_table_and_flag_off_tree(engine, bundle, gpus):
    """--alleles --ladder-by-type on one rank and on two: one table, the same bytes; without the flag the same tree but for it, and
    nothing of the six passes it runs appears"""
    from quasimodo_amd import workflow
    from quasimodo_amd.tables import CALLER_MAP
    from test_gpu_afprofile import _tree
    root, data, fas = bundle
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    out = root / ("on%d" % gpus)
    jobs = workflow.run_hcmv_variantcall(data, str(out), alleles=True, ladder_by_type=fas, ladder_type_bins="1,2,6", **kw)
    on = _tree(str(out))
    mixed = [j for j in jobs if not os.path.basename(j.vcf_file).split(".")[0].endswith(("-1-0", "-0-1"))]
    assert TABLE in on and len(mixed) > 0
    assert not [k for k in on if any((os.sep + d + os.sep) in k for d in ("norm", "atoms", "hap", "ladder")) or "normalized.tsv" in k
                or "atomized.tsv" in k or "haplotype.tsv" in k or "performance_ladder.tsv" in k or "performance_types.tsv" in k]
    if gpus == 2:
        assert on == _tree(str(root / "on1"))                        # (the one-rank case ran first: the same bytes)
        return
    rest = {k: v for k, v in on.items() if k != TABLE}
    workflow.run_hcmv_variantcall(data, str(root / "off"), alleles=True, engine=engine)
    assert _tree(str(root / "off")) == rest                          # without the flag: the tree of the parent's run
    table = on[TABLE].decode().split("\n")
    assert table[0] == "\t".join(lt.TABLE_HEADER) and table[-1] == ""
    got = {}
    for ln in table[1:-1]:
        f = ln.split("\t")
        got.setdefault((f[0], f[1]), []).append(f[2:])
    genomes = {mix: "".join(open(fas[mix]).read().split("\n")[1:]) for mix in fas}
    pooled = {}
    for k, j in enumerate(mixed):
        base = os.path.basename(j.vcf_file)[:-4]
        smp, ref, c = base.split(".")[:3]
        rec, tru = np.asarray(j.stats["ladder_types_rec"], np.uint64), np.asarray(j.stats["ladder_types_tru"], np.uint64)
        assert rec.shape == tru.shape == (NR, 18) and j.stats["ladder_types_edges"] == EDGES
        if k < 4:                                                     # (four jobs spelled out from text; the rest through the table)
            wrec, wtru = restate(j.vcf_file, j.filtered_out, j.tp_out, genomes[smp[:2]], open(j.snp_file, "rb").read())
            np.testing.assert_array_equal(rec, wrec, err_msg=base)
            np.testing.assert_array_equal(tru, wtru, err_msg=base)
        assert got[(CALLER_MAP.get(c, c), smp)] == text_table(rec, tru), base
        acc = pooled.setdefault(c, [np.zeros((NR, 18), np.uint64), np.zeros((NR, 18), np.uint64)])
        acc[0] += rec
        acc[1] += tru
    for c, (rec, tru) in pooled.items():
        assert got[(CALLER_MAP.get(c, c), "pooled")] == text_table(rec, tru), c
    assert len(got) == len(mixed) + len(pooled)


def test_command_line_refusals(bundle, tmp_path):
    """--ladder-by-type without --alleles, beside --match-ladder, --by-type or any other pass flag, and under vareval: said before a
    file is touched; the dry run names the table"""
    root, data, fas = bundle
    refs = ["--merlin-ref", fas["TM"], "--ad169-ref", fas["TA"]]
    cmd = [sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", data]
    L = "--ladder-by-type"
    for extra, said in (([L], "--alleles"), (["--alleles", L, "--match-ladder"], "--ladder-by-type cannot be combined with --match-ladder"),
                        (["--alleles", L, "--by-type"], "--by-type cannot be combined with --ladder-by-type"),
                        (["--alleles", L, "--normalize"], "--ladder-by-type cannot be combined with --normalize"),
                        (["--alleles", L, "--atomize"], "--atomize cannot be combined with --ladder-by-type"),
                        (["--alleles", L, "--haplotypes"], "--ladder-by-type cannot be combined with --haplotypes"),
                        (["--alleles", L, "--rescue-roc"], "--ladder-by-type cannot be combined with --rescue-roc"),
                        (["--alleles", L, "--truth-side"], "--ladder-by-type cannot be combined with --truth-side"),
                        (["--alleles", L, "--votes"], "--ladder-by-type cannot be combined with --votes"),
                        (["--alleles", L, "--hap-gap", "40"], "--hap-gap"), (["--alleles", L, "--type-bins", "1,1"], "--type-bins")):
        r = subprocess.run(cmd + ["-o", str(tmp_path / "x")] + extra + refs, capture_output=True, text=True)
        assert r.returncode != 0 and said in r.stderr + r.stdout and not (tmp_path / "x").exists(), (extra, r.stderr)
    r = subprocess.run(cmd + ["-o", str(tmp_path / "d"), "--alleles", L, "--hap-gap", "5", "--type-bins", "1,2,6", "--dryrun"] + refs,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "caller_performance_ladder_types.tsv" in r.stdout and "\t5\t1,2,6" in r.stdout and not (tmp_path / "d").exists(), r.stderr
    cases_dir = os.path.join(GOLDEN, "custom")
    from conftest import golden_cases
    cases = [e for e in golden_cases() if e["family"] == "custom"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", os.path.join(cases_dir, cases[0]["vcf"]), "--snps",
                        os.path.join(cases_dir, cases[0]["truth"]), "-l", "a", "-o", str(tmp_path / "v"), L], capture_output=True, text=True)
    assert r.returncode != 0 and "allele-extended" in r.stderr + r.stdout and not (tmp_path / "v").exists()
