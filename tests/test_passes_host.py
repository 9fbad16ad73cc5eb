"""Which passes over a finished batch may share a call (quasimodo_amd.passes): motifs with profile, every other
pass alone -- at extract_many and at the two workflows, in front of any file or device.  The expected pairs are a literal here, not
the table's."""
import itertools

import pytest

ALLOWED = {frozenset(("genomes", "profile"))}                       # extract_many's keywords
ALLOWED_FLAGS = {frozenset(("mutation_context", "snp_profile"))}    # run_hcmv_variantcall's


def _keywords(n, fasta):
    """every pass as extract_many keywords, each with its smallest valid argument; the truth-side view in both spellings"""
    return {"genomes": [dict(genomes=[fasta] * n)],
            "truthside": [dict(fn=True), dict(groups=[list(range(n))])],
            "profile": [dict(profile={"want": [1] * n})],
            "strata": [dict(strata=[("all", [0], [100])])],
            "boot": [dict(boot={})],
            "votes": [dict(votes=True, groups=[list(range(n))])]}   # (`groups` names the vote groups then)


def test_extract_many_takes_one_pass_per_call_but_motifs_with_profile(tmp_path):
    from quasimodo_amd.extract import Job, extract_many
    mk = lambda: [Job(str(tmp_path / ("s.c%d.vcf" % i)), str(tmp_path / "t.vcf"), "hcmv", "", "c%d" % i) for i in range(2)]
    kws = _keywords(2, str(tmp_path / "nowhere.fa"))
    assert len(kws) == 6
    for a, b in itertools.combinations(kws, 2):
        for ka, kb in itertools.product(kws[a], kws[b]):
            if "groups" in ka and "groups" in kb:
                continue                                            # one keyword, one reading: with votes it names the vote groups
            if frozenset((a, b)) in ALLOWED:
                with pytest.raises(Exception) as ei:                # past the argument checks: no such file, or no device
                    extract_many(mk(), **ka, **kb)
                assert "does not combine" not in str(ei.value), (a, b)
            else:
                with pytest.raises(ValueError, match="does not combine"):
                    extract_many(mk(), **ka, **kb)
    assert not any(p.is_file() for p in tmp_path.rglob("*"))       # no file was written


def test_workflow_flags_take_one_pass_per_run_but_motifs_with_profile(tmp_path, capsys):
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    fa = tmp_path / "g.fa"
    fa.write_text(">g\nACGT\n")
    flags = {"mutation_context": {"TM": str(fa), "TA": str(fa)}, "truth_side": True, "snp_profile": True,
             "strata": [("all", [0], [100])], "bootstrap": 10, "votes": True}
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    for a, b in itertools.combinations(flags, 2):
        run = lambda d: workflow.run_hcmv_variantcall(str(d), str(tmp_path / "out"), dryrun=True, **{a: flags[a], b: flags[b]})
        if frozenset((a, b)) in ALLOWED_FLAGS:
            assert run(data) is None
        else:
            with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
                run(tmp_path / "nodata")                            # refused in front of the bundle
    vflags = {k: flags[k] for k in ("truth_side", "strata", "bootstrap", "votes")}
    vcfs = [str(tmp_path / ("v%d.vcf" % i)) for i in range(3)]
    for a, b in itertools.combinations(vflags, 2):
        with pytest.raises(workflow.WorkflowError, match="cannot be combined"):
            workflow.run_vareval(vcfs, str(tmp_path / "x.snps"), str(tmp_path / "o"), dryrun=True, **{a: vflags[a], b: vflags[b]})
    assert not (tmp_path / "out").exists() and not (tmp_path / "o").exists()
