"""k-of-n caller consensus end to end (qm_extract_files_votes, extract_many(votes=), --votes / --consensus-vcf):
the golden hcmv family with all six callers per mixed sample and the custom family with its three labels against a restatement
on TEXT -- the pos-ref-alt strings of the expected/*.filtered.vcf files against the truth file's rows
(quasimodo_amd.truthside.snp_keys), never the engine's packing; the consensus VCF against consensus.consensus_text."""
import os
import re

import pytest

from conftest import GOLDEN, golden_cases, read_case

pytestmark = pytest.mark.gpu


def _rd(path):
    with open(path, "rb") as fh:
        return fh.read()


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = _rd(os.path.join(d, f))
    return out


def _custom_keys(text):
    """The truth keys of the custom family as text: columns 1-3 of the show-snps table, rows whose REF and ALT are each exactly one
    of A, C, G, T.  T' of the vote tables is the truth set the engine holds (QM_S_TRUTH): the two rows of this table with `N` or
    lower-case bases (custom_snp_benchmark.R:23-27 would keep them) are no keys of it and can be hit by no kept line."""
    out = set()
    for ln in text.split(b"\n"):
        f = ln.rstrip(b"\r").split(b"\t")
        if ln and not ln.startswith(b"#") and len(f) >= 3 and f[1] in (b"A", b"C", b"G", b"T") and f[2] in (b"A", b"C", b"G", b"T"):
            out.add((f[0], f[1], f[2]))
    return out


def text_votes(genome, kept_sets):
    """(tp_votes, fp_votes, private_tp, private_fp) from sets of (POS text, REF, ALT)"""
    n = len(kept_sets)
    tp, fp, ptp, pfp = [0] * 33, [0] * 33, [0] * 32, [0] * 32
    for k in genome | set().union(*kept_sets):
        who = [i for i in range(n) if k in kept_sets[i]]
        if k in genome:
            tp[len(who)] += 1
        else:
            fp[len(who)] += 1
        if len(who) == 1:
            (ptp if k in genome else pfp)[who[0]] += 1
    return tp, fp, ptp, pfp


def expected_tables(tmp, cons, priv):
    from quasimodo_amd import consensus as K
    K.write_caller_consensus(os.path.join(tmp, "want_consensus.tsv"), cons)
    K.write_caller_private(os.path.join(tmp, "want_private.tsv"), priv)
    return _rd(os.path.join(tmp, "want_consensus.tsv")), _rd(os.path.join(tmp, "want_private.tsv"))


SNAPS = {}


@pytest.mark.parametrize("gpus,k", [(1, 1), (1, 2), (1, 6), (2, 2)])
def test_hcmv_six_callers_per_sample(engine, tmp_path, gpus, k):
    from quasimodo_amd import consensus as K
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), consensus_vcf=k, **kw)
    assert len(jobs) == 60
    exp = os.path.join(GOLDEN, "hcmv", "expected")
    truth = {mix: ts.snp_keys(_rd(os.path.join(GOLDEN, "hcmv", "input", "nucmer", "%s.maskrepeat.variants.vcf" % mix))) for mix in ("TM", "TA")}
    per = {}
    for j in jobs:
        base = os.path.basename(j.vcf_file)[:-4]
        smp, ref, c = base.split(".")[:3]
        if not smp.endswith(("-1-0", "-0-1")):
            per.setdefault((smp, ref), []).append((c, _rd(os.path.join(exp, c, base + ".filtered.vcf"))))
    assert len(per) == 6 and all(len(v) == 6 for v in per.values())
    cons, priv = {}, {}
    for (smp, ref), mem in sorted(per.items()):
        tp, fp, ptp, pfp = text_votes(truth[smp[:2]], [ts.snp_keys(t) for _, t in mem])
        cons[smp] = (6, tp, fp)
        priv[smp] = ([c for c, _ in mem], ptp, pfp)
        got = _rd(str(out / "results" / "snp" / "consensus" / ("%s.%s.k%d.vcf" % (smp, ref, k))))
        assert got == K.consensus_text([t for _, t in mem], k), "%s at k = %d" % (smp, k)
    want_c, want_p = expected_tables(str(tmp_path), cons, priv)
    tables = out / "results" / "final_tables"
    assert (tables / "caller_consensus.tsv").read_bytes() == want_c
    assert (tables / "caller_private.tsv").read_bytes() == want_p
    assert sum(cons["TM-1-1"][1]) == len(truth["TM"]) and any(cons["TM-1-1"][2][1:])
    new = _tree(str(out))
    added = {f: v for f, v in new.items() if "/consensus/" in f or f.endswith(("caller_consensus.tsv", "caller_private.tsv"))}
    SNAPS[(gpus, k)] = added
    if (1, 2) in SNAPS and (2, 2) in SNAPS:
        assert SNAPS[(1, 2)] == SNAPS[(2, 2)], "two ranks write the same tables and files as one"
    if (gpus, k) == (1, 2):
        # without the flags: every file of the output tree has the same bytes, and the flags add only the two tables and the files
        off = tmp_path / "off"
        workflow.run_hcmv_variantcall(str(data), str(off), engine=engine)
        old = _tree(str(off))
        assert set(new) - set(old) == set(added) and not set(old) - set(new) and len(added) == 6 + 2
        differing = [f for f in old if old[f] != new[f]]
        assert not differing, differing
        assert len(old) > 300 and "results/final_tables/caller_performance.tsv" in old


@pytest.mark.parametrize("gpus", [1, 2])
def test_custom_three_labels(engine, tmp_path, gpus):
    from quasimodo_amd import consensus as K
    from quasimodo_amd import truthside as ts
    from quasimodo_amd import workflow
    cs = [e for e in golden_cases() if e["family"] == "custom"]
    assert len(cs) == 3
    vcfs, texts, labels = [], [], []
    for e in cs:
        vcf, truth, exp = read_case(e)
        p = tmp_path / os.path.basename(e["vcf"])
        p.write_bytes(vcf)
        vcfs.append(str(p))
        texts.append(exp["filtered"])
        labels.append(e["caller"])
    snps = tmp_path / "g1_g2.maskrepeat.snps"
    snps.write_bytes(truth)
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    for k in (1, 2, 3):
        out = tmp_path / ("o%d" % k)
        workflow.run_vareval(vcfs, str(snps), str(out), labels=labels, consensus_vcf=k, **kw)
        tp, fp, ptp, pfp = text_votes(_custom_keys(truth), [ts.snp_keys(t) for t in texts])
        want_c, want_p = expected_tables(str(tmp_path), {"custom": (3, tp, fp)}, {"custom": (labels, ptp, pfp)})
        tables = out / "results" / "final_tables"
        assert (tables / "caller_consensus.tsv").read_bytes() == want_c and (tables / "caller_private.tsv").read_bytes() == want_p
        assert _rd(str(out / "results" / "snp" / "consensus" / ("custom.k%d.vcf" % k))) == K.consensus_text(texts, k)
    plain = tmp_path / "plain"
    workflow.run_vareval(vcfs, str(snps), str(plain), labels=labels, engine=engine)
    old, new = _tree(str(plain)), _tree(str(tmp_path / "o2"))
    assert sorted(set(new) - set(old)) == ["results/final_tables/caller_consensus.tsv", "results/final_tables/caller_private.tsv",
                                          "results/snp/consensus/custom.k2.vcf"]
    assert not set(old) - set(new) and not [f for f in old if old[f] != new[f]]


@pytest.mark.parametrize("case", [e for e in golden_cases() if e["family"] == "quirks"], ids=lambda e: e["mode"])
def test_quirks_member_with_a_kept_nokey_line_is_refused_by_name(engine, tmp_path, case):
    import shutil
    from quasimodo_amd._lib import QmvtError
    from quasimodo_amd.extract import Job, extract_many
    fam = os.path.join(GOLDEN, "quirks")
    vcf = tmp_path / os.path.basename(case["vcf"])
    shutil.copyfile(os.path.join(fam, case["vcf"]), vcf)
    cons = tmp_path / "o" / "consensus.k1.vcf"
    job = Job(str(vcf), os.path.join(fam, case["truth"]), case["mode"], str(tmp_path / "o"), "q")
    with pytest.raises(QmvtError) as e:
        extract_many([job], engine=engine, votes={"k": [1], "out": [str(cons)]}, groups=[[0]])
    m = re.search(r"line (\d+)", str(e.value))
    assert e.value.code == -8 and os.path.basename(str(vcf)) in str(e.value) and m, str(e.value)
    f = _rd(str(vcf)).split(b"\n")[int(m.group(1)) - 1].split(b"\t")
    assert re.fullmatch(rb"0|[1-9][0-9]*", f[1]) is None or int(f[1]) >= 1 << 28, "the named line has a canonical POS"
    assert not cons.exists()
    # outside a group the same file goes through as before
    plain = Job(str(vcf), os.path.join(fam, case["truth"]), case["mode"], str(tmp_path / "p"), "q")
    extract_many([plain], engine=engine)
    assert _rd(plain.filtered_out) == _rd(os.path.join(fam, case["expected"]["filtered"]))
