"""Sequence-context profiles end to end (qm_extract_files_context, extract_many(context=), --seq-context): the
golden hcmv family and the custom family over seeded planted genomes written as FASTA, against a restatement on TEXT -- the lines
of the written *.filtered.vcf, *.tp.vcf and *.fp.vcf and the golden truth file split in Python and placed with context.cells."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_cases
from quasimodo_amd import context as cx
from test_context_host import planted_genome

pytestmark = pytest.mark.gpu

W, NG = 50, 10
BASES = (b"A", b"C", b"G", b"T")
NC = cx.n_cells(NG)
LENGTHS = {"TM": 236000, "TA": 229354}             # about HCMV's size: most golden positions lie inside, some beyond TA's end


def _fastas(tmp_path):
    """{mix: path}, {mix: restated table}: two planted genomes as FASTA files with 60-base lines (the last one with '\\r\\n')"""
    paths, tabs = {}, {}
    for seed, (mix, L) in enumerate(sorted(LENGTHS.items()), 7):
        seq = planted_genome(seed, L)
        eol = b"\r\n" if mix == "TA" else b"\n"
        p = tmp_path / ("%s.fa" % mix)
        p.write_bytes(b">%s planted" % mix.encode() + eol + b"".join(seq[i:i + 60] + eol for i in range(0, L, 60)))
        paths[mix], tabs[mix] = str(p), cx.cells(seq, W, NG)
    return paths, tabs


def _data_rows(path):
    if not path:
        return []
    with open(path, "rb") as fh:
        return [ln.split(b"\t") for ln in fh.read().split(b"\n") if ln and ln[:1] != b"#"]


def text_counts(tab, filtered, tp, fp, truth_keys_text, kept_keys_text):
    """(rec [NC + 1][3], tru [NC][2]) from the TEXT of the written files and the truth file (the golden families hold no kept line
    without a comparable key: the nokey row stays zero)"""
    place = lambda pos, n: np.bincount(cx.rows_of(tab, np.array(pos, np.int64), NG), minlength=n).astype(np.uint64)
    rec = np.zeros((NC + 1, 3), np.uint64)
    for col, path in enumerate((filtered, tp, fp)):
        rec[:, col] = place([int(f[1]) for f in _data_rows(path)], NC + 1)
    # the distinct keys the bitmaps hold: both alleles one of A, C, G, T (a row with `N` or a lower-case base counts in genomediff only)
    keys = sorted(k for k in truth_keys_text if k[1] in BASES and k[2] in BASES)
    tru = np.zeros((NC, 2), np.uint64)
    tru[:, 0] = place([int(k[0]) for k in keys], NC)
    tru[:, 1] = place([int(k[0]) for k in keys if k in kept_keys_text], NC)
    return rec, tru


def _mix(job):
    return os.path.basename(job.vcf_file)[:2]


def _check_job(j, tab, genome_keys, pure):
    from quasimodo_amd import truthside as ts
    kept = ts.snp_keys(open(j.filtered_out, "rb").read())
    wrec, wtru = text_counts(tab, j.filtered_out, j.tp_out or None, j.fp_out, set() if pure else genome_keys, kept)
    rec, tru, gen = j.stats["context_rec"], j.stats["context_tru"], j.stats["context_gen"]
    np.testing.assert_array_equal(rec, wrec, err_msg=j.vcf_file)
    np.testing.assert_array_equal(tru, wtru, err_msg=j.vcf_file)
    np.testing.assert_array_equal(gen.astype(np.int64), cx.positions(tab, NG))
    assert j.stats["context_params"] == (W, NG)
    assert rec.sum(axis=0).tolist() == [j.stats["n_pass"], j.stats["tp_lines"], j.stats["fp_lines"]]
    if pure:
        assert not tru.any() and not rec[:, 1].any()
    else:
        assert tru.sum(axis=0).tolist() == [j.stats["truth_unique"], j.stats["TP_R"]]


def test_extract_many_context_matches_the_written_files(engine, tmp_path):
    from quasimodo_amd import truthside as ts
    from quasimodo_amd.extract import extract_many, is_pure_strain
    from test_gpu_afprofile import _golden_jobs
    fa, tabs = _fastas(tmp_path)
    plain = _golden_jobs(str(tmp_path / "a"))
    extract_many(plain, engine=engine)
    jobs = _golden_jobs(str(tmp_path / "b"))
    extract_many(jobs, engine=engine, context={"genomes": [fa[_mix(j)] for j in jobs], "half_window": W, "n_gc": NG})
    seen_pure = seen_hit = seen_none = False
    for p, j in zip(plain, jobs):
        for x, y in ((p.filtered_out, j.filtered_out), (p.fp_out, j.fp_out)) + (((p.tp_out, j.tp_out),) if p.tp_out else ()):
            assert open(x, "rb").read() == open(y, "rb").read()
        pure = is_pure_strain(j.vcf_file)
        _check_job(j, tabs[_mix(j)], None if pure else ts.snp_keys(open(j.snp_file, "rb").read()), pure)
        rec, tru = j.stats["context_rec"], j.stats["context_tru"]
        for k in ("context_rec", "context_tru", "context_gen", "context_params"):
            j.stats.pop(k)
        for k in p.stats:
            assert np.array_equal(np.asarray(p.stats[k]), np.asarray(j.stats[k])) if k == "roc" and p.stats[k] is not None else p.stats[k] == j.stats[k], k
        seen_pure = seen_pure or (pure and rec[:, 2].sum() > 0)
        seen_hit = seen_hit or (not pure and (tru[:NC - 1, 1] > 0).sum() >= 5)
        seen_none = seen_none or rec[NC - 1, 0] > 0
    assert seen_pure and seen_hit and seen_none
    # a job without a genome takes no part; other parameters give the other grid; the pass runs in a call of its own
    some = _golden_jobs(str(tmp_path / "c"))[:3]
    extract_many(some, engine=engine, context={"genomes": [fa[_mix(some[0])], None, fa[_mix(some[2])]], "half_window": 3, "n_gc": 4})
    assert "context_rec" not in some[1].stats and some[1].context is None
    assert some[0].stats["context_rec"].shape == (66, 3) and some[0].stats["context_params"] == (3, 4)
    assert some[0].stats["context_rec"].sum(axis=0).tolist() == [some[0].stats[k] for k in ("n_pass", "tp_lines", "fp_lines")]
    for bad in (dict(fn=True), dict(strata=[("a", [0], [10])]), dict(surface=True), dict(explain=3)):
        with pytest.raises(ValueError):
            extract_many(_golden_jobs(str(tmp_path / "d")), engine=engine, context={"genomes": [fa["TM"]] * len(jobs)}, **bad)
    with pytest.raises(ValueError):
        extract_many(_golden_jobs(str(tmp_path / "d")), engine=engine, context={"genomes": [fa["TM"]] * len(jobs), "n_gc": 16})


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    head = lines[0].split("\t")
    return head, [dict(zip(head, ln.split("\t"))) for ln in lines[1:-1]]


def _num(x):
    return 0 if x == "NA" else int(x)


HEAD = ("caller mixture homopolymer gc_bin gc_from gc_to positions calleridentify TP_lines FP_lines genomediff TP FN Precision Recall "
        "F1 FP_per_kb").split()
SNAPS = {}


@pytest.mark.parametrize("gpus", [1, 2])
def test_workflow_context_table_and_flag_off_tree(engine, tmp_path, gpus):
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_gpu_afprofile import _tree
    from test_tables_workflow import _build_bundle
    fa, tabs = _fastas(tmp_path)
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), seq_context=fa, context_window=W, context_gc_bins=NG, **kw)
    on = _tree(str(out))
    name = "results/final_tables/caller_performance_context.tsv"
    assert name in on
    if gpus == 1:                                                   # without the flag: the same tree minus the new table
        off_dir = tmp_path / "off"
        workflow.run_hcmv_variantcall(str(data), str(off_dir), engine=engine)
        assert _tree(str(off_dir)) == {k: v for k, v in on.items() if k != name}
    # the jobs' counts against the text of the written files, and the table against the writer over them
    rows = []
    for j in jobs:
        base = os.path.basename(j.vcf_file)[:-4]
        smp, _, c = base.split(".")[:3]
        pure = bool(j.stats.get("pure_strain"))
        _check_job(j, tabs[smp[:2]], None if pure else ts.snp_keys(open(j.snp_file, "rb").read()), pure)
        st = dict(j.stats)
        if not pure:
            st["context_genomediff"] = cx.truth_rows(j.snp_file, "hcmv", tabs[smp[:2]], NG)
        rows.append((c, smp, st))
    want = tmp_path / "want.tsv"
    cx.write_performance_context(str(want), rows, NG)
    assert on[name] == want.read_bytes()
    head, trows = _table(str(out / name))
    assert head == HEAD
    _, whole = _table(str(out / "results" / "final_tables" / "caller_performance.tsv"))
    by = {}
    for r in trows:
        by.setdefault((r["caller"], r["mixture"]), []).append(r)
    assert len(by) == len(whole) == len(jobs)
    for w in whole:
        mine = by[(w["caller"], w["mixture"])]
        tail = [r for r in mine if r["homopolymer"] in ("none", "nokey")]
        assert [r["homopolymer"] for r in mine[-2:]] == ["none", "nokey"] and len(tail) == 2
        fams = ([r for r in mine if r["gc_bin"] == "all"], [r for r in mine if r["homopolymer"] == "all"],
                [r for r in mine if "all" not in (r["homopolymer"], r["gc_bin"]) and r not in tail])
        assert len(fams[0]) == 16 and len(fams[1]) == NG and [r["homopolymer"] for r in fams[0]][-2:] == ["14", "15+"]
        for fam in fams:                                            # the cells and each marginal family, with none and nokey, are the whole genome
            for col in ("calleridentify", "TP", "genomediff"):
                assert sum(_num(r[col]) for r in fam + tail) == _num(w[col]), (w["caller"], w["mixture"], col)
            assert sum(_num(r["positions"]) for r in fam + tail) == LENGTHS[w["mixture"][:2]]
    SNAPS[gpus] = on[name]
    if len(SNAPS) == 2:                                             # a VCF's rows do not depend on the rank
        assert SNAPS[1] == SNAPS[2]
    # a mix without a FASTA, parameters without the flag, a second pass in the run
    with pytest.raises(workflow.WorkflowError):
        workflow.run_hcmv_variantcall(str(data), str(tmp_path / "x"), seq_context={"TM": fa["TM"], "TA": None}, engine=engine)
    with pytest.raises(workflow.WorkflowError):
        workflow.run_hcmv_variantcall(str(data), str(tmp_path / "x"), context_window=9, engine=engine)
    with pytest.raises(workflow.WorkflowError):
        workflow.run_hcmv_variantcall(str(data), str(tmp_path / "x"), seq_context=fa, context_gc_bins=16, engine=engine)
    with pytest.raises(workflow.WorkflowError):
        workflow.run_hcmv_variantcall(str(data), str(tmp_path / "x"), seq_context=fa, filter_surface=True, engine=engine)
    assert not (tmp_path / "x").exists()


def test_vareval_context(engine, tmp_path):
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_gpu_afprofile import _tree
    from test_gpu_truthside import _custom_keys
    fa, tabs = _fastas(tmp_path)
    cases = [e for e in golden_cases() if e["family"] == "custom"]
    fam = os.path.join(GOLDEN, "custom")
    vcfs = [os.path.join(fam, e["vcf"]) for e in cases]
    snps = os.path.join(fam, cases[0]["truth"])
    labels = ["c%d" % k for k in range(len(vcfs))]
    jobs = workflow.run_vareval(vcfs, snps, str(tmp_path / "on"), labels=labels, engine=engine, seq_context=fa["TM"], context_window=W, context_gc_bins=NG)
    workflow.run_vareval(vcfs, snps, str(tmp_path / "off"), labels=labels, engine=engine)
    on, off = _tree(str(tmp_path / "on")), _tree(str(tmp_path / "off"))
    name = "results/final_tables/snpcall_benchmark_context.txt"
    assert off == {k: v for k, v in on.items() if k != name} and name in on
    genome = _custom_keys(open(snps, "rb").read())
    rows = []
    for lab, j in zip(labels, jobs):
        _check_job(j, tabs["TM"], genome, False)
        rows.append((lab, None, dict(j.stats, context_genomediff=cx.truth_rows(snps, "custom", tabs["TM"], NG))))
    want = tmp_path / "want.txt"
    cx.write_performance_context(str(want), rows, NG, custom=True)
    assert on[name] == want.read_bytes()
    head, trows = _table(str(tmp_path / "on" / name))
    assert head == ["caller"] + HEAD[2:13] + ["precision", "recall", "f1", "FP_per_kb"]
    _, whole = _table(str(tmp_path / "on" / "results" / "final_tables" / "snpcall_benchmark.txt"))
    for lab, w in zip(labels, whole):
        mine = [r for r in trows if r["caller"] == lab]
        fam_rows = [r for r in mine if r["gc_bin"] == "all"] + mine[-2:]
        for col in ("calleridentify", "TP", "genomediff"):
            assert sum(_num(r[col]) for r in fam_rows) == _num(w[col]), (lab, col)
