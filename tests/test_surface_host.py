"""The host side of the filter surface (quasimodo_amd.surface, passes, extract_many(surface=), --filter-surface):
no device is needed for any of this."""
import pytest


def _grid(nq, na, cells):
    """S [3][nq][na] of Python ints from {(i, k): (TPc, FP, U)}, everything else zero"""
    S = [[[0] * na for _ in range(nq)] for _ in range(3)]
    for (i, k), v in cells.items():
        for c in range(3):
            S[c][i][k] = v[c]
    return S


def _others(n, fasta):
    """every other pass as extract_many keywords, each with its smallest valid argument"""
    return {"genomes": dict(genomes=[fasta] * n), "fn": dict(fn=True), "groups": dict(groups=[list(range(n))]),
            "profile": dict(profile={"want": [1] * n}), "strata": dict(strata=[("all", [0], [100])]), "boot": dict(boot={}),
            "votes": dict(votes=True, groups=[list(range(n))]), "explain": dict(explain=10)}


def test_the_pass_table_holds_the_new_pass_and_the_kernels_id_stays():
    from quasimodo_amd import _lib, passes
    p = [x for x in passes.PASSES if x.name == "surface"]
    assert len(p) == 1 and p[0].fields == ("surface",) and p[0].keywords == ("surface",) and p[0].flag == "--filter-surface" and p[0].shares == ()
    assert p[0].agree == "surface: the swept jobs of one call share one QUAL step and one pair of bin counts"
    assert passes.PASSES[-1].name == "surface"
    assert _lib.source_kernels_id() == "db744d8883a55744"
    assert _lib.QM_ABI_VERSION == 6
    for name in ("qm_batch_surface", "qm_batch_get_surface", "qm_batch_surface_timings", "qm_extract_files_surface"):
        assert name in _lib.EXPORTS


def test_best_cell_unique_maximum():
    from quasimodo_amd import surface as sf
    # T' = 10.  (0, 0): P = 8/12, S = 0.8; (1, 1): P = 7/7, S = 0.7 -> F1 14/17 = 0.8235 beats 16/22 = 0.727; (2, 0): P = 1, S = 0.1
    S = _grid(3, 2, {(0, 0): (8, 4, 8), (0, 1): (7, 3, 7), (1, 0): (7, 1, 7), (1, 1): (7, 0, 7), (2, 0): (1, 0, 1)})
    assert sf.best_cell(S, 10) == (1, 1)
    assert sf.cell_numbers(S, 10, 1, 1) == (7, 0, 7, 3, 1.0, 0.7, 2 * 0.7 / 1.7)
    assert sf.cell_numbers(S, 10, 2, 1) == (0, 0, 0, 0, 0.0, 0.0, 0.0)          # no call: zeros


def test_best_cell_exact_tie_needs_integers():
    from quasimodo_amd import surface as sf
    # F1 = 2 TPc U / (TPc T' + U (TPc + FP)); with TPc = U it is 2 U / (T' + U + FP).  T' = 3 * 10^17 + 1:
    #   cell (0, 1): U = 10^17, FP = 0          -> 2 * 10^17 / (T' + 10^17)
    #   cell (1, 0): U = 2 * 10^17, FP = T'     -> 4 * 10^17 / (2 T' + 2 * 10^17): the same fraction
    #   cell (0, 0): U = 2 * 10^17, FP = T' + 1 -> smaller by about one part in 8 * 10^17
    T = 3 * 10 ** 17 + 1
    a, b = 10 ** 17, 2 * 10 ** 17
    S = _grid(2, 2, {(0, 0): (b, T + 1, b), (0, 1): (a, 0, a), (1, 0): (b, T, b)})
    f = lambda c: sf.cell_numbers(S, T, *c)[6]
    # floating point cannot tell them apart: they differ by parts in 10^18, far below the 1.1e-16 a double resolves near 0.5
    assert max(f((0, 0)), f((0, 1)), f((1, 0))) - min(f((0, 0)), f((0, 1)), f((1, 0))) < 5e-16
    assert sf.best_cell(S, T) == (0, 1)                        # (0, 0) is smaller; (0, 1) and (1, 0) tie exactly: the smaller qual_min
    S2 = _grid(2, 2, {(0, 0): (b, T + 1, b), (1, 1): (a, 0, a), (1, 0): (b, T, b)})
    assert sf.best_cell(S2, T) == (1, 0)                       # the same tie inside one QUAL row: the smaller af_min
    S3 = _grid(2, 2, {(0, 0): (b, T - 1, b), (0, 1): (a, 0, a), (1, 0): (b, T, b)})
    assert sf.best_cell(S3, T) == (0, 0)                       # ... and larger by as little wins


def test_best_cell_of_the_empty_grid():
    from quasimodo_amd import surface as sf
    assert sf.best_cell(_grid(2, 3, {}), 5) is None
    assert sf.best_cell(_grid(1, 1, {}), 0) is None
    # calls but nothing found (F1 = 0 everywhere, T' = 0 included): the first cell with a call
    assert sf.best_cell(_grid(2, 2, {(0, 1): (0, 3, 0), (1, 0): (0, 1, 0)}), 0) == (0, 1)
    rows = sf.best_filter_rows([("lofreq", "TM-1-1", _grid(6, 1, {}), [0, 0, 0, 4])], 4)
    assert rows == ["LoFreq\tTM-1-1\t0\t0.0000" + "\t0\t0\t0\t0\t0.0000\t0.0000\t0.0000" * 2 + "\t0",
                    "LoFreq\tpooled\t0\t0.0000" + "\t0\t0\t0\t0\t0.0000\t0.0000\t0.0000" * 2 + "\t0"]


def test_surface_rows_bytes_of_a_two_by_two_grid(tmp_path):
    from quasimodo_amd import surface as sf
    S = _grid(2, 2, {(0, 0): (5, 3, 4), (0, 1): (2, 1, 2), (1, 0): (3, 0, 3)})
    want = ("qual_min\taf_min\ttrue_positives_baseline\tfalse_positives\ttrue_positives_call\tfalse_negatives\tprecision\tsensitivity\tf_measure\n"
            "0\t0.0000\t4\t3\t5\t2\t0.6250\t0.6667\t0.6452\n"
            "0\t0.5000\t2\t1\t2\t4\t0.6667\t0.3333\t0.4444\n"
            "10\t0.0000\t3\t0\t3\t3\t1.0000\t0.5000\t0.6667\n"
            "10\t0.5000\t0\t0\t0\t0\t0.0000\t0.0000\t0.0000\n")
    assert "\n".join(sf.surface_rows(S, 6, 10)) + "\n" == want
    path = tmp_path / "d" / "x.surface.tsv"
    sf.write_surface(str(path), S, 6, 10)
    assert path.read_bytes() == want.encode() and not list(path.parent.glob("*.tmp.*"))
    import numpy as np
    assert sf.surface_rows(np.array(S, np.uint64), np.uint64(6), 10) == want.split("\n")[:-1]   # the engine's arrays give the same bytes


def test_pooled_choice_differs_from_both_samples(tmp_path):
    from quasimodo_amd import surface as sf
    # T' = 10 each; cells x = (0, 0), y = (1, 0), z = (2, 0): sample A is best at x, sample B at y, their sums at z
    A = _grid(3, 1, {(0, 0): (9, 1, 9), (1, 0): (1, 0, 1), (2, 0): (8, 2, 8)})     # F1: x 0.9, y 2/11, z 0.8
    B = _grid(3, 1, {(0, 0): (1, 9, 1), (1, 0): (9, 1, 9), (2, 0): (8, 2, 8)})     # F1: x 0.1, y 0.9, z 0.8
    assert sf.best_cell(A, 10) == (0, 0) and sf.best_cell(B, 10) == (1, 0)
    P, T = sf.pooled([(A, 10), (B, 10)])
    assert T == 20 and P[0] == [[10], [10], [16]] and P[1] == [[10], [1], [4]] and P[2] == [[10], [10], [16]]
    assert sf.best_cell(P, T) == (2, 0)                                             # x 0.5, y 20/31, z 0.8
    path = tmp_path / "final_tables" / "caller_best_filter.tsv"
    sf.write_caller_best_filter(str(path), [("lofreq", "TM-1-1", A, [10, 2, 0, 10]), ("lofreq", "TM-1-10", B, [10, 3, 1, 10]),
                                            ("mycaller", "TM-1-1", B, [10, 0, 0, 10])], 10)
    got = path.read_text().split("\n")
    assert got[0].split("\t") == list(sf.BEST_HEADER) and got[-1] == "" and len(got) == 1 + 5 + 1
    assert got[1] == "LoFreq\tTM-1-1\t0\t0.0000\t9\t1\t9\t1\t0.9000\t0.9000\t0.9000\t8\t2\t8\t2\t0.8000\t0.8000\t0.8000\t2"
    assert got[2] == "LoFreq\tTM-1-10\t10\t0.0000\t9\t1\t9\t1\t0.9000\t0.9000\t0.9000\t8\t2\t8\t2\t0.8000\t0.8000\t0.8000\t3"
    assert got[3] == "LoFreq\tpooled\t20\t0.0000\t16\t4\t16\t4\t0.8000\t0.8000\t0.8000\t16\t4\t16\t4\t0.8000\t0.8000\t0.8000\t5"
    assert got[4].startswith("mycaller\tTM-1-1\t10\t") and got[5].startswith("mycaller\tpooled\t10\t")


def test_parameter_limits_and_the_q_step_rule_of_the_workflows(tmp_path):
    from quasimodo_amd import surface as sf, workflow
    assert sf.params() == (4, 64, 50) and sf.params(1, 256, 16) == (1, 256, 16) and sf.params(na="64") == (4, 64, 64)
    for kw, word in ((dict(q_step=0), "q_step"), (dict(nq=0), "nq"), (dict(nq=257), "nq"), (dict(na=0), "na"), (dict(na=65), "na"),
                     (dict(nq=241, na=17), "4097 cells")):
        with pytest.raises(ValueError, match=word):
            sf.params(**kw)
    assert sf.workflow_params(5, 5, 1) == (5, 5, 1) and sf.workflow_params(20, 2, 1) == (20, 2, 1) and sf.workflow_params(1, 21, 3) == (1, 21, 3)
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(2)]
    run = lambda **kw: workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, **kw)
    hcmv = lambda **kw: workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), dryrun=True, **kw)
    for bad in (dict(surface_qual_step=3), dict(surface_qual_step=8), dict(surface_qual_step=4, surface_qual_bins=5),
                dict(surface_qual_step=20, surface_qual_bins=1), dict(surface_qual_step=40)):
        for f in (run, hcmv):
            with pytest.raises(workflow.WorkflowError, match="grid line"):     # before the bundle is read: `nodata` does not exist
                f(filter_surface=True, **bad)
    for f in (run, hcmv):
        with pytest.raises(workflow.WorkflowError, match="--filter-surface: surface: na 65"):
            f(filter_surface=True, surface_af_bins=65)
        with pytest.raises(workflow.WorkflowError, match="go with --filter-surface"):
            f(surface_qual_step=4)
    assert not (tmp_path / "out").exists() and not (tmp_path / "o").exists()


def test_extract_many_refuses_every_other_pass_beside_surface(tmp_path):
    from quasimodo_amd.extract import Job, extract_many
    mk = lambda: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i) for i in range(2)]
    for name, kw in _others(2, str(tmp_path / "nowhere.fa")).items():
        with pytest.raises(ValueError, match="does not combine"):
            extract_many(mk(), surface=True, **kw)
    # the same through the Job fields
    jobs = mk()
    jobs[0].surface = (4, 64, 50)
    with pytest.raises(ValueError, match="does not combine"):
        extract_many(jobs, fn=True)
    # the swept jobs of one call share one parameter triple; the parameters have their ranges
    jobs = mk()
    jobs[0].surface, jobs[1].surface = (4, 64, 50), (2, 64, 50)
    with pytest.raises(ValueError, match="share one QUAL step and one pair of bin counts"):
        extract_many(jobs)
    for bad, word in ((dict(q_step=0), "q_step"), (dict(nq=257), "nq"), (dict(na=65), "na"), (dict(nq=64, na=65), "na")):
        with pytest.raises(ValueError, match=word):
            extract_many(mk(), surface=bad)
    assert not any(p.is_file() for p in tmp_path.rglob("*"))       # no file was written


def test_both_workflows_refuse_every_other_flag_beside_filter_surface(tmp_path):
    from quasimodo_amd import workflow
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGT\n")
    flags = {"mutation_context": {"TM": str(fa), "TA": str(fa)}, "truth_side": True, "snp_profile": True,
             "strata": [("all", [0], [100])], "bootstrap": 10, "votes": True, "consensus_vcf": 2, "explain_errors": True}
    for name, v in flags.items():
        with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
            workflow.run_hcmv_variantcall(str(tmp_path / "nodata"), str(tmp_path / "out"), dryrun=True, filter_surface=True, **{name: v})
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(3)]
    for name in ("truth_side", "strata", "bootstrap", "votes", "consensus_vcf", "explain_errors"):
        with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
            workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, filter_surface=True, **{name: flags[name]})
    assert not (tmp_path / "out").exists() and not (tmp_path / "o").exists()


def test_dryrun_names_the_swept_jobs(tmp_path, capsys):
    from quasimodo_amd import workflow
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(2)]
    assert workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, filter_surface=True) is None
    out = capsys.readouterr().out.split("\n")
    assert "filter_surface\tv0\t4\t64\t50" in out and "filter_surface\tv1\t4\t64\t50" in out and "caller_best_filter\tv0,v1" in out
    assert workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, filter_surface=True, surface_qual_step=5,
                                surface_qual_bins=10, surface_af_bins=8) is None
    assert "filter_surface\tv1\t5\t10\t8" in capsys.readouterr().out.split("\n")
    assert workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True) is None
    assert "filter_surface" not in capsys.readouterr().out       # without the flag nothing is said
    # hcmv: one line per caller x mixed sample, none for the pure strains
    data = tmp_path / "snp"
    for c in ("clc", "lofreq"):
        (data / "vcf" / c).mkdir(parents=True)
        for s in ("TM-1-1", "TM-1-0"):
            (data / "vcf" / c / ("%s.%s.%s.vcf" % (s, workflow.SAMPLE_REF[s], c))).write_text("")
    assert workflow.run_hcmv_variantcall(str(data), str(tmp_path / "out"), callers=["clc", "lofreq"], dryrun=True, filter_surface=True) is None
    out = capsys.readouterr().out.split("\n")
    assert "filter_surface\tclc\tTM-1-1\t4\t64\t50" in out and "filter_surface\tlofreq\tTM-1-1\t4\t64\t50" in out
    assert not any(ln.startswith("filter_surface") and "TM-1-0" in ln for ln in out) and "caller_best_filter\tclc,lofreq" in out
    assert not (tmp_path / "out").exists() and not (tmp_path / "o").exists()


def test_surface_path_sits_beside_fp_and_tp():
    from quasimodo_amd import surface as sf
    from quasimodo_amd.extract import Job, _paths
    j = Job("/r/callers/lofreq/TM-1-1.Merlin.lofreq.vcf", "/r/nucmer/TM.maskrepeat.variants.vcf", "hcmv")
    _paths(j)
    assert sf.surface_path(j) == "/r/callers/lofreq/surface/TM-1-1.Merlin.lofreq.surface.tsv"
    j = Job("/in/a.vcf", "/in/x.snps", "custom", "/o/callers", "lab")
    _paths(j)
    assert sf.surface_path(j) == "/o/callers/surface/lab.surface.tsv"
