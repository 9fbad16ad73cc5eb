"""What the two workflows and their command lines say, replayed against tests/golden/workflow_text/ (recorded by
tools/record_workflow_text.py, which holds the matrix): every dry-run line, every refusal and both --help texts, exactly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_workflow_text as rec   # noqa: E402


@pytest.mark.parametrize("name", sorted(rec.RECORDERS))
def test_the_text_of_every_case_is_the_recorded_one(name):
    want = rec.load(name)
    got = rec.record(name)
    assert sorted(got) == sorted(want)                       # the matrix itself: no case dropped, none added
    differ = [cid for cid in sorted(want) if got[cid] != want[cid]]
    assert not differ, "%d of %d cases differ, the first: %s\nrecorded: %r\nnow:      %r" % (
        len(differ), len(want), differ[0], want[differ[0]], got[differ[0]])


def test_the_workflow_table_covers_every_pass_keyword_once_and_its_orders_name_every_row():
    import inspect
    from quasimodo_amd import passes, workflow
    rows = workflow.WORKFLOW_PASSES
    names = [p.name for p in rows]
    assert sorted(names) == sorted(p.name for p in passes.PASSES)
    assert sorted(workflow.DRY_ORDER) == sorted(names) == sorted(workflow.WRITE_ORDER)
    keys = [k for p in rows for k in p.keys]
    plumbing = {"data_dir", "outpath", "callers", "engine", "dryrun", "gpus", "_body", "_backend", "_same_device", "alleles"}
    assert sorted(keys) == sorted(set(inspect.signature(workflow.run_hcmv_variantcall).parameters) - plumbing)
    custom = [k for p in rows if p.custom for k in p.keys]
    assert sorted(custom) == sorted(set(inspect.signature(workflow.run_vareval).parameters) - plumbing - {"vcfs", "snps_file", "labels"})


def test_the_matrix_holds_what_it_is_meant_to():
    """every pass and parameter keyword of the two signatures is in the matrix, so a new one cannot stay out of it unnoticed"""
    import inspect
    from quasimodo_amd import workflow
    plumbing = {"data_dir", "outpath", "callers", "engine", "dryrun", "gpus", "_body", "_backend", "_same_device", "alleles",
                "vcfs", "snps_file", "labels"}
    assert set(inspect.signature(workflow.run_hcmv_variantcall).parameters) - plumbing == set(rec.HCMV_PASSES) | set(rec.HCMV_PARAMS)
    assert set(inspect.signature(workflow.run_vareval).parameters) - plumbing == set(rec.VAREVAL_PASSES) | set(rec.VAREVAL_PARAMS)
    want = rec.load("hcmv")
    n = len(rec.HCMV_PASSES) + len(rec.HCMV_PARAMS)
    assert len(want) >= 2 * (1 + n + n * (n - 1) // 2)
