"""TP, FP and FN by variant type and size end to end (qm_extract_files_types, extract_many(alleles=True, vartype=), --alleles
--by-type): a small family built from the golden allele probe -- its VCF and truth file with rows added behind
them, a 20-base allele on either side among them, so that the dictionary and its shape table take part -- against a
restatement on TEXT: the lines of the written *.filtered.vcf and *.tp.vcf and the rows of the truth file, typed as strings with
vartype.shape."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from quasimodo_amd import vartype as vt

pytestmark = pytest.mark.gpu

PROBE = os.path.join(GOLDEN, "alleles", "input", "probe.vcf")
TRUTH = os.path.join(GOLDEN, "alleles", "input", "probe.truth.vcf")
ALLELE = re.compile(rb"^[ACGT]+$")
CANON = re.compile(rb"^(0|[1-9][0-9]{0,8})$")
LONG20 = b"ACGTTGCAACGTTGCAACGT"                                                                     # 20 bases: a dictionary id

TRUTH_ROWS = [b"c\t150\t.\tA\tG\t30\tPASS\tTYPE=SNV", b"c\t160\t.\tAC\tGT\t30\tPASS\tTYPE=MNP",
              b"c\t170\t.\tA\tAT\t30\tPASS\tTYPE=INS", b"c\t180\t.\tCAC\tC\t30\tPASS\tTYPE=DEL",
              b"c\t190\t.\tG\tG" + LONG20 + b"\t30\tPASS\tTYPE=INS",                                # INS 20 through the shape table
              b"c\t200\t.\tT" + LONG20 + b"\tT\t30\tPASS\tTYPE=DEL",                                # DEL 20, never called
              b"c\t210\t.\tAC\tG\t30\tPASS\tTYPE=CPX",
              b"c\t220\t.\t" + LONG20 + b"A\t" + LONG20 + b"C\t30\tPASS\tTYPE=LONGPAIR"]
VCF_ROWS = [b"c\t150\t.\tA\tG\t50\tPASS\tDP=9",                      # SNV, TP
            b"c\t150\trs1\tA\tG\t50\tPASS\tDP=9",                    # ... with an ID: kept, FP; the entry is found all the same
            b"c\t160\t.\tAC\tGT\t50\tPASS\tDP=9",                    # MNP 2, TP
            b"c\t170\t.\tA\tAA\t50\tPASS\tDP=9",                     # INS 1, another spelling: FP, the truth's INS stays missed
            b"c\t180\t.\tCAC\tC\t5\tPASS\tDP=9",                     # DEL 2, not kept
            b"c\t190\t.\tG\tG" + LONG20 + b"\t50\tPASS\tDP=9",       # INS 20, TP
            b"c\t195\t.\tC\t" + LONG20 + b"\t50\tPASS\tDP=9",        # CPX 19 (A...T against C: the last base T is no suffix of C)
            b"c\t210\t.\tAC\tG\t50\tPASS\tDP=9",                     # CPX 2, TP
            b"c\t220\t.\t" + LONG20 + b"A\t" + LONG20 + b"C\t50\tPASS\tDP=9",     # LONGPAIR, TP by spelling
            b"c\t230\t.\tACGTACGTACGTA\tA\t50\tPASS\tDP=9",          # DEL 12: thirteen bases are inline
            b"c\t240\t.\tACGTACGTACGTAC\tA\t50\tPASS\tDP=9"]         # DEL 13: fourteen are not


def data_lines(text):
    return [ln.split(b"\t") for ln in text.split(b"\n") if ln and ln[:1] != b"#"]


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


def text_row(pos, ref, alt, edges):
    """the row of one line or truth row from its text"""
    off = 5 * len(edges)
    if not CANON.match(pos) or not ALLELE.match(ref) or not ALLELE.match(alt):
        return off + vt.NOKEY
    if ref == alt:
        return off + vt.NOVAR
    if len(ref) > 13 and len(alt) > 13:
        return off + vt.LONGPAIR
    kind, size = vt.shape(ref.decode(), alt.decode())     # (the call's own dictionary holds every long allele: no NOSHAPE)
    return vt.row_of(kind, size, edges)


def restate(filtered, tp, truth_text, edges):
    """(rec, tru) of one VCF from text: kept = the lines of filtered.vcf, TP = those of tp.vcf (a sub-sequence of them)"""
    nr = vt.n_rows(edges)
    rec, tru = np.zeros((nr, 2), np.uint64), np.zeros((nr, 2), np.uint64)
    kept = data_lines(open(filtered, "rb").read())
    rest = data_lines(open(tp, "rb").read())
    spelled = set()
    for f in kept:
        row = text_row(f[1], f[3], f[4], edges)
        rec[row, 0] += 1
        if rest and rest[0] == f:
            rec[row, 1] += 1
            rest.pop(0)
        if CANON.match(f[1]) and ALLELE.match(f[3]) and ALLELE.match(f[4]) and int(f[1]) < (1 << 28):
            spelled.add((int(f[1]), f[3], f[4]))
    assert not rest, tp
    entries = {(int(f[1]), f[3], f[4]) for f in data_lines(truth_text)
               if CANON.match(f[1]) and ALLELE.match(f[3]) and ALLELE.match(f[4]) and int(f[1]) < (1 << 28)}
    for e in entries:
        row = text_row(b"%d" % e[0], e[1], e[2], edges)
        tru[row, 0] += 1
        tru[row, 1] += e in spelled
    return rec, tru


def _jobs(vcfs, truth, **kw):
    from quasimodo_amd.extract import Job
    return [Job(v, truth, "hcmv", "", "c", **kw) for v in vcfs]


def test_extract_many_vartype_one_rank_and_sharded(engine, tmp_path):
    from quasimodo_amd.extract import extract_many
    from quasimodo_amd.multigpu import extract_many_sharded
    from test_gpu_afprofile import _tree
    edges = vt.DEFAULT_EDGES
    vcfs, truth, truth_text = family(tmp_path, "one")
    pv, pt, _ = family(tmp_path, "plain")
    plain = extract_many(_jobs(pv, pt), engine=engine, alleles=True)
    jobs = extract_many(_jobs(vcfs, truth), engine=engine, alleles=True, vartype=True)
    assert _tree(str(tmp_path / "one")) == _tree(str(tmp_path / "plain"))          # the pass writes no file of its own
    names = vt.row_names(edges)
    want = []
    for p, j in zip(plain, jobs):
        rec, tru = restate(j.filtered_out, j.tp_out, truth_text, edges)
        want.append({"type_rec": rec, "type_tru": tru})
        np.testing.assert_array_equal(j.stats["type_rec"], rec, err_msg=j.vcf_file)
        np.testing.assert_array_equal(j.stats["type_tru"], tru, err_msg=j.vcf_file)
        assert j.stats["type_edges"] == edges
        assert int(rec[:, 0].sum()) == j.stats["n_pass"] and int(rec[:, 1].sum()) == j.stats["tp_lines"]
        for k in p.stats:                                          # the rows of the plain call, unchanged
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
    # the added lines by hand (the VCF that holds only them)
    rec, tru = jobs[1].stats["type_rec"], jobs[1].stats["type_tru"]
    got = {names[k]: (rec[k].tolist(), tru[k].tolist()) for k in range(len(names)) if rec[k].any()}
    assert got["SNV:1"][0] == [2, 1] and got["MNP:2"][0] == [1, 1] and got["INS:1"][0] == [1, 0]
    assert got["INS:16-50"][0] == [1, 1] and got["INS:16-50"][1][1] == 1         # (the probe's truth file has an insertion of 25 bases too)
    assert got["CPX:16-50"][0] == [1, 0] and got["CPX:2"][0] == [1, 1] and got["LONGPAIR"] == ([1, 1], [1, 1])
    assert got["DEL:6-15"][0] == [2, 0] and "DEL:2" not in got and "NOSHAPE" not in got
    assert tru[names.index("DEL:16-50")].tolist()[1] == 0 and int(tru[names.index("DEL:16-50"), 0]) >= 1       # the DEL 20 nobody called
    # sharded over two ranks of one device: the same rows, the same table
    svcfs, struth, _ = family(tmp_path, "two")
    sj, _ = extract_many_sharded(_jobs(svcfs, struth, vartype=edges), 2, backend="gloo", same_device=True, alleles=True)
    for a, b in zip(jobs, sj):
        np.testing.assert_array_equal(a.stats["type_rec"], np.asarray(b.stats["type_rec"]))
        np.testing.assert_array_equal(a.stats["type_tru"], np.asarray(b.stats["type_tru"]))
    t1, t2, t3 = tmp_path / "t1.tsv", tmp_path / "t2.tsv", tmp_path / "t3.tsv"
    name = lambda j: os.path.basename(j.vcf_file).split(".")[0]
    vt.write_performance_types(str(t1), [("c", name(j), j.stats) for j in jobs], edges)
    vt.write_performance_types(str(t2), [("c", name(j), j.stats) for j in sj], edges)
    vt.write_performance_types(str(t3), [("c", name(j), w) for j, w in zip(jobs, want)], edges)
    assert t1.read_bytes() == t2.read_bytes() == t3.read_bytes()
    lines = t1.read_text().split("\n")
    assert len(lines) == 1 + 4 * (5 * 9 + 4) + 1 and lines[0].split("\t") == list(vt.TABLE_HEADER)
    row = next(ln.split("\t") for ln in lines if ln.startswith("c\ts2\tSNV\t1\t"))
    n_snv = int(tru[0, 0])
    assert row[4:7] == ["1", "1", str(n_snv - 1)] and row[7] == "0.5"
    # other edges: one call of their own
    ov, ot, otext = family(tmp_path, "three")
    oj = extract_many(_jobs(ov, ot), engine=engine, alleles=True, vartype=[1, 2, 6])
    for j in oj:
        rec, tru = restate(j.filtered_out, j.tp_out, otext, (1, 2, 6))
        np.testing.assert_array_equal(j.stats["type_rec"], rec)
        np.testing.assert_array_equal(j.stats["type_tru"], tru)
    # refusals, in front of any file: without the allele-extended mode, a second pass in the call
    for kw, said in ((dict(vartype=True), "--alleles"), (dict(alleles=True, vartype=True, fn=True), "does not combine")):
        rv, rt, _ = family(tmp_path, "r%d" % len(os.listdir(tmp_path)))
        with pytest.raises(ValueError, match=said):
            extract_many(_jobs(rv, rt), engine=engine, **kw)


def test_command_line(tmp_path):
    """hcmv -e variantcall --alleles --by-type --type-bins 1,2,6 writes the table, and without the flag the same tree but for it"""
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    cmd = [sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data), "--alleles"]
    r = subprocess.run(cmd + ["-o", str(tmp_path / "on"), "--by-type", "--type-bins", "1,2,6"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(cmd + ["-o", str(tmp_path / "off")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    on, off = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off"))
    name = os.path.join("results", "final_tables", "caller_performance_types.tsv")
    assert name in on and off == {k: v for k, v in on.items() if k != name}
    lines = on[name].decode().split("\n")
    head = lines[0].split("\t")
    assert head == list(vt.TABLE_HEADER) and lines[-1] == ""
    rows = [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]
    whole = [w.split("\t") for w in on[os.path.join("results", "final_tables", "caller_performance.tsv")].decode().split("\n")[1:-1]]
    mixed = [w for w in whole if not w[1].endswith(("-1-0", "-0-1"))]
    per = 5 * 4 + 4
    callers = sorted({w[0] for w in mixed})
    assert len(mixed) > 0 and len(rows) == per * (len(mixed) + len(callers))
    assert {r_["size"] for r_ in rows} == {"1", "2-5", "6+", "all", "NA"}
    for w in mixed:                                                  # the marginals of a job add up to its row of caller_performance.tsv's counts
        mine = [r_ for r_ in rows if (r_["caller"], r_["mixture"]) == (w[0], w[1]) and r_["size"] in ("all", "NA")]
        assert len(mine) == 9 and sum(int(r_["TP"]) + int(r_["FP"]) for r_ in mine) > 0
    pooled = [r_ for r_ in rows if r_["mixture"] == "pooled"]
    assert sum(int(r_["TP"]) for r_ in pooled if r_["size"] in ("all", "NA")) == sum(int(r_["TP"]) for r_ in rows if r_["mixture"] != "pooled" and r_["size"] in ("all", "NA")) > 0
    # --by-type without --alleles is refused before a file is touched
    r = subprocess.run(cmd[:-1] + ["-o", str(tmp_path / "x"), "--by-type"], capture_output=True, text=True)
    assert r.returncode != 0 and "--alleles" in r.stderr + r.stdout and not (tmp_path / "x").exists()
    # ... and so is --by-type under vareval, which has no allele-extended reading of a show-snps table
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "vareval", "-v", str(tmp_path / "a.vcf"), "--snps", str(tmp_path / "a.snps"),
                        "-l", "a", "-o", str(tmp_path / "v"), "--by-type"], capture_output=True, text=True)
    assert r.returncode != 0 and "--by-type" in r.stderr + r.stdout and not (tmp_path / "v").exists()
