"""The host side of the near-miss pass (quasimodo_amd.nearmiss, passes, extract_many(explain=), --explain-errors):
no device is needed for any of this."""
import pytest


def _others(n, fasta):
    """every other pass as extract_many keywords, each with its smallest valid argument"""
    return {"genomes": dict(genomes=[fasta] * n), "fn": dict(fn=True), "groups": dict(groups=[list(range(n))]),
            "profile": dict(profile={"want": [1] * n}), "strata": dict(strata=[("all", [0], [100])]), "boot": dict(boot={}),
            "votes": dict(votes=True, groups=[list(range(n))])}


def test_the_pass_table_holds_the_new_pass_and_the_kernels_id_stays():
    from quasimodo_amd import _lib, passes
    p = [x for x in passes.PASSES if x.name == "nearmiss"]
    assert len(p) == 1 and p[0].fields == ("explain",) and p[0].keywords == ("explain",) and p[0].flag == "--explain-errors" and p[0].shares == ()
    assert _lib.source_kernels_id() == "db744d8883a55744"
    assert _lib.QM_ABI_VERSION == 6
    for name in ("qm_batch_nearmiss", "qm_batch_get_nearmiss", "qm_batch_get_nearmiss_cls", "qm_batch_get_nearmiss_truth", "qm_extract_files_nearmiss"):
        assert name in _lib.EXPORTS


def test_extract_many_refuses_every_other_pass_beside_explain(tmp_path):
    from quasimodo_amd.extract import Job, extract_many
    mk = lambda: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i) for i in range(2)]
    for name, kw in _others(2, str(tmp_path / "nowhere.fa")).items():
        with pytest.raises(ValueError, match="does not combine"):
            extract_many(mk(), explain=10, **kw)
    # the same through the Job fields
    jobs = mk()
    jobs[0].explain = 3
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(jobs, fn=True)
    # the explained jobs of one call share one radius; the radius has its range
    jobs = mk()
    jobs[0].explain, jobs[1].explain = 0, 3
    with pytest.raises(ValueError, match="share one radius"):
        extract_many(jobs)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match="0 to 64"):
            extract_many(mk(), explain=bad)
    assert not any(p.is_file() for p in tmp_path.rglob("*"))       # no file was written


def test_both_workflows_refuse_every_other_flag_beside_explain_errors(tmp_path):
    from quasimodo_amd import workflow
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGT\n")
    flags = {"mutation_context": {"TM": str(fa), "TA": str(fa)}, "truth_side": True, "snp_profile": True,
             "strata": [("all", [0], [100])], "bootstrap": 10, "votes": True, "consensus_vcf": 2}
    for name, v in flags.items():
        with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
            workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), dryrun=True, explain_errors=True, **{name: v})
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(3)]
    for name in ("truth_side", "strata", "bootstrap", "votes", "consensus_vcf"):
        with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
            workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, explain_errors=True, **{name: flags[name]})
    with pytest.raises(workflow.WorkflowError, match="--explain-radius"):
        workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, explain_errors=True, explain_radius=65)
    with pytest.raises(workflow.WorkflowError, match="goes with --explain-errors"):
        workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, explain_radius=5)
    assert not (tmp_path / "out").exists() and not (tmp_path / "o").exists()


def test_dryrun_names_the_explained_jobs(tmp_path, capsys):
    from quasimodo_amd import workflow
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(2)]
    assert workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, explain_errors=True) is None
    out = capsys.readouterr().out.split("\n")
    assert "explain_errors\tv0\t10" in out and "explain_errors\tv1\t10" in out and "caller_error_classes\tv0,v1" in out


def test_why_paths_sit_beside_fp_and_tp():
    from quasimodo_amd import nearmiss as nm
    from quasimodo_amd.extract import Job, _paths
    j = Job("/r/callers/lofreq/TM-1-1.Merlin.lofreq.vcf", "/r/nucmer/TM.maskrepeat.variants.vcf", "hcmv")
    _paths(j)
    assert nm.fp_why_path(j) == "/r/callers/lofreq/why/TM-1-1.Merlin.lofreq.fp.why.tsv"
    assert nm.fn_why_path(j) == "/r/callers/lofreq/why/TM-1-1.Merlin.lofreq.fn.why.tsv"
    j = Job("/in/a.vcf", "/in/x.snps", "custom", "/o/callers", "lab")
    _paths(j)
    assert nm.fp_why_path(j) == "/o/callers/why/lab.fp.why.tsv" and nm.fn_why_path(j) == "/o/callers/why/lab.fn.why.tsv"


def test_table_writer_rounding_na_and_zero_rows(tmp_path):
    from quasimodo_amd import nearmiss as nm
    assert nm.RECORD_CLASSES == ("idcol", "allele", "refbase", "near", "isolated", "nokey")
    assert nm.TRUTH_CLASSES == ("filtered", "allele", "position", "near", "uncalled")
    path = tmp_path / "t" / "caller_error_classes.tsv"
    path.parent.mkdir()
    nm.write_caller_error_classes(str(path), [("lofreq", "TM-1-1", [1, 2, 0, 3, 0, 0], [0, 0, 0, 0, 0]),
                                              ("mycaller", "TA-1-10", [0, 0, 0, 0, 0, 0], [1, 0, 0, 2000, 1])])
    got = path.read_text().split("\n")
    assert got[0] == "caller\tmixture\tside\tclass\tcount\tshare" and got[-1] == "" and len(got) == 1 + 2 * 11 + 1
    assert got[1:7] == ["LoFreq\tTM-1-1\tFP\tidcol\t1\t0.167", "LoFreq\tTM-1-1\tFP\tallele\t2\t0.333", "LoFreq\tTM-1-1\tFP\trefbase\t0\t0",
                        "LoFreq\tTM-1-1\tFP\tnear\t3\t0.5", "LoFreq\tTM-1-1\tFP\tisolated\t0\t0", "LoFreq\tTM-1-1\tFP\tnokey\t0\t0"]
    assert got[7:12] == ["LoFreq\tTM-1-1\tFN\t%s\t0\tNA" % c for c in nm.TRUTH_CLASSES]       # an empty side
    assert got[12:18] == ["mycaller\tTA-1-10\tFP\t%s\t0\tNA" % c for c in nm.RECORD_CLASSES]
    assert got[18:23] == ["mycaller\tTA-1-10\tFN\tfiltered\t1\t0", "mycaller\tTA-1-10\tFN\tallele\t0\t0", "mycaller\tTA-1-10\tFN\tposition\t0\t0",
                          "mycaller\tTA-1-10\tFN\tnear\t2000\t0.999", "mycaller\tTA-1-10\tFN\tuncalled\t1\t0"]
    # R's round(x, 3): half to even on the scaled value (1 / 16 = 0.0625 -> 0.062, 3 / 16 = 0.1875 -> 0.188)
    rows = nm.class_rows("clc", "s", [1, 3, 12, 0, 0, 0], [0] * 5)
    assert [r[5] for r in rows[:3]] == [0.062, 0.188, 0.75] and rows[0][0] == "CLC"
    with pytest.raises(ValueError):
        nm.class_rows("clc", "s", [1, 2, 3], [0] * 5)
    assert not list(path.parent.glob("*.tmp.*"))


def test_why_file_readers(tmp_path):
    from quasimodo_amd import nearmiss as nm
    fp = tmp_path / "x.fp.why.tsv"
    fp.write_text(nm.FP_WHY_HEADER + "\n12\t100\tA\tC\t33.5\tnear\n40\t007\tG\tT\t.\tnokey\n")
    assert nm.read_fp_why(str(fp)) == [(12, "100", "A", "C", "33.5", "near"), (40, "007", "G", "T", ".", "nokey")]
    fn = tmp_path / "x.fn.why.tsv"
    fn.write_text(nm.FN_WHY_HEADER + "\n5\tA\tC\tfiltered\n9\tn\tC\t.\n")
    assert nm.read_fn_why(str(fn)) == [("5", "A", "C", "filtered"), ("9", "n", "C", ".")]
    fn.write_text(nm.FN_WHY_HEADER + "\n")
    assert nm.read_fn_why(str(fn)) == []
    for text in ("POS\tREF\n", nm.FN_WHY_HEADER + "\n5\tA\tC\tnokey\n", nm.FN_WHY_HEADER + "\n5\tA\tC\n", nm.FN_WHY_HEADER + "\n5\tA\tC\tnear"):
        fn.write_text(text)
        with pytest.raises(ValueError):
            nm.read_fn_why(str(fn))
    with pytest.raises(ValueError):
        nm.read_fp_why(str(fn))
    assert nm.check_radius(0) == 0 and nm.check_radius("64") == 64
