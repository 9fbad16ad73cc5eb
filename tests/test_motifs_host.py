"""Host side of the mutation-context spectra (quasimodo_amd.motifs): motif names, FASTA reading, the table
writer and the workflow's command line.  No GPU."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def test_motif_names_order_and_split():
    from quasimodo_amd.motifs import MOTIFS, alteration, context
    assert len(MOTIFS) == 96 and len(set(MOTIFS)) == 96
    assert list(MOTIFS) == sorted(MOTIFS)                      # SomaticSignatures' lexicographic order
    assert MOTIFS[:5] == ("CA A.A", "CA A.C", "CA A.G", "CA A.T", "CA C.A")
    assert MOTIFS[11] == "CA G.T" and MOTIFS[16] == "CG A.A" and MOTIFS[-1] == "TG T.T"
    assert {m[:2] for m in MOTIFS} == {"CA", "CG", "CT", "TA", "TC", "TG"}
    assert alteration("CA A.C") == "C>A" and context("CA A.C") == "A.C"
    assert alteration("TG T.G") == "T>G" and context("TG T.G") == "T.G"


def test_read_fasta(tmp_path):
    from quasimodo_amd.motifs import read_fasta
    one = tmp_path / "one.fa"
    one.write_bytes(b">Merlin some description\nACGTacgt\nNNac\n\n")
    assert read_fasta(str(one)) == b"ACGTacgtNNac"
    crlf = tmp_path / "crlf.fa"
    crlf.write_bytes(b">AD169\r\nACGT\r\nggcc\r\n")
    assert read_fasta(str(crlf)) == b"ACGTggcc"
    many = tmp_path / "many.fa"
    many.write_bytes(b">chr1\nAAAA\nCC\n>chr2 second\nGGGG\n>chr3\nTT\n")
    with pytest.raises(ValueError):
        read_fasta(str(many))
    assert read_fasta(str(many), contig="chr2") == b"GGGG"
    assert read_fasta(str(many), contig="chr1") == b"AAAACC"
    with pytest.raises(ValueError):
        read_fasta(str(many), contig="chr9")
    empty = tmp_path / "empty.fa"
    empty.write_bytes(b"")
    with pytest.raises(ValueError):
        read_fasta(str(empty))


def test_write_mutation_context_columns(tmp_path):
    from quasimodo_amd.motifs import MOTIFS, study_columns, write_mutation_context
    rows = {}
    for k, s in enumerate(("TM-1-50", "TM-0-1", "TM-1-10", "TM-1-1", "TM-1-0")):
        kept = [k * 1000 + i for i in range(98)]
        tp = [k * 100 + i for i in range(98)]
        rows[s] = [kept, tp, [a - b for a, b in zip(kept, tp)]]
    cols = study_columns(rows)
    names = [n for n, _ in cols]
    assert names == ["unmixed TM-0-1",
                     "TM-1-1", "TM-1-1 (TP)", "TM-1-1 (FP)",
                     "TM-1-10", "TM-1-10 (TP)", "TM-1-10 (FP)",
                     "TM-1-50", "TM-1-50 (TP)", "TM-1-50 (FP)"]
    p = tmp_path / "TM.clc.mutationcontext.tsv"
    write_mutation_context(str(p), cols)
    lines = p.read_text().splitlines()
    assert lines[0].split("\t") == ["motif", "alteration", "context"] + names
    assert len(lines) == 97
    assert lines[2].split("\t")[:4] == ["CA A.C", "C>A", "A.C", "1001"]        # TM-0-1 kept, column 1
    last = lines[96].split("\t")
    assert last[:3] == [MOTIFS[95], "T>G", "T.T"]
    assert last[3:] == [str(v) for v in (1095, 3095, 395, 2700, 2095, 295, 1800, 95, 95, 0)]
    assert not [f for f in os.listdir(tmp_path) if ".tmp." in f]


def _bundle(root):
    from test_tables_workflow import _build_bundle
    _build_bundle(root)


def test_cli_dryrun_prints_the_tables(tmp_path):
    data = tmp_path / "data" / "snp"
    _bundle(str(data))
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">g\nACGT\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data),
                        "-o", str(tmp_path / "out"), "--dryrun", "--mutation-context", "--merlin-ref", str(fa), "--ad169-ref", str(fa)],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    mc = sorted(ln for ln in r.stdout.splitlines() if ln.startswith("mutationcontext\t"))
    callers = sorted({ln.split("\t")[1] for ln in r.stdout.splitlines() if ln.startswith("extractTP\t")})
    assert mc == sorted("mutationcontext\t%s\t%s" % (m, c) for m in ("TA", "TM") for c in callers)
    plain = subprocess.run([sys.executable, os.path.join(ROOT, "run_benchmark.py"), "hcmv", "-e", "variantcall", "--data", str(data),
                            "-o", str(tmp_path / "out"), "--dryrun"], capture_output=True, text=True, cwd=ROOT)
    assert plain.returncode == 0 and "mutationcontext" not in plain.stdout


def test_missing_fasta_fails_before_any_engine(tmp_path, monkeypatch):
    from quasimodo_amd import workflow
    data = tmp_path / "data" / "snp"
    _bundle(str(data))

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")
    monkeypatch.setattr(workflow, "Engine", no_engine)
    with pytest.raises(workflow.WorkflowError):
        workflow.run_hcmv_variantcall(str(data), str(tmp_path / "out"),
                                      mutation_context={"TM": str(tmp_path / "nope.fa"), "TA": str(tmp_path / "nope.fa")})
    assert not (tmp_path / "out").exists()


def test_new_symbols_are_in_the_header_and_exported():
    from quasimodo_amd import _lib
    with open(os.path.join(ROOT, "include", "qmvt.h")) as fh:
        h = fh.read()
    for s in ("qm_genome_load", "qm_genome_release", "qm_batch_motifs", "qm_batch_get_motifs", "qm_extract_files_motifs"):
        assert s + "(" in h and s in _lib.EXPORTS
    for k, v in (("QM_N_MOTIFS", 96), ("QM_MOTIF_OTHER", 96), ("QM_MOTIF_REF_MISMATCH", 97), ("QM_MOTIF_COLS", 98)):
        assert "#define %s %d" % (k, v) in h and getattr(_lib, k) == v
