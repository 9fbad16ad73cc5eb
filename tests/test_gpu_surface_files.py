"""The filter surface end to end (qm_extract_files_surface, extract_many(surface=), --filter-surface): the golden
hcmv family with its six callers and the custom family with its three labels against a restatement on TEXT -- the lines of the
input VCF split in Python, R's AF pattern applied with `re` as tests/test_gpu_afprofile.py does, the truth keys read from the
golden truth file, the TP lines of the kept records from the golden *.tp.vcf -- never the engine's packing."""
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, golden_cases, read_case

pytestmark = pytest.mark.gpu

BASES = (b"A", b"C", b"G", b"T")
R_PATTERN = re.compile(rb".*AF=([01]\.[0-9]+);.*$")
PLAIN = re.compile(rb"[+-]?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?")   # the numbers awk and Python read alike
Q, NQ, NA = 4, 64, 50


def _rd(path):
    with open(path, "rb") as fh:
        return fh.read()


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = _rd(os.path.join(d, f))
    return out


def _data_lines(text):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [ln for ln in lines if not ln.startswith(b"#")]


def _pos(text):
    return int(text) if re.fullmatch(rb"0|[1-9][0-9]*", text) and int(text) < 1 << 28 else None


def truth_keys(truth_text, mode):
    cols = (1, 3, 4) if mode == "hcmv" else (0, 1, 2)
    keys = set()
    for ln in _data_lines(truth_text):
        f = ln.split(b"\t")
        if len(f) > cols[2] and _pos(f[cols[0]]) is not None and f[cols[1]] in BASES and f[cols[2]] in BASES:
            keys.add((_pos(f[cols[0]]), f[cols[1]], f[cols[2]]))
    return keys


def restate(vcf_text, tp_text, truth_text, mode, q_step=Q, nq=NQ, na=NA):
    """(S [3][nq][na], extra [4]) of one job from text"""
    keys = truth_keys(truth_text, mode)
    tp_lines = set(_data_lines(tp_text))
    G = np.zeros((3, nq, na), np.int64)
    best = {}
    counted = no_af = no_bin = 0
    for ln in _data_lines(vcf_text):
        f = ln.split(b"\t")
        if len(f) < 6 or f[3] not in BASES or f[4] not in BASES:
            continue                                                     # not a single-base record
        qt = f[5]
        assert qt == b"." or PLAIN.fullmatch(qt), "the golden families spell QUAL as a decimal number or `.`: %r" % qt
        if qt == b".":
            b = nq * q_step - 1                                          # awk keeps `.`: above every threshold
        elif math.floor(float(qt)) < 0:
            no_bin += 1                                                  # no threshold of the grid keeps it
            continue
        else:
            b = min(math.floor(float(qt)), nq * q_step - 1)
        p = _pos(f[1])
        key = (p, f[3], f[4])
        found = p is not None and key in keys
        dot = f[2] == b"."
        kept = qt == b"." or float(qt) >= 20
        is_tp = ln in tp_lines if kept else found and dot               # a kept line: what the reference's fgrep selected
        m = R_PATTERN.match(f[7]) if len(f) >= 8 else None
        af = np.float32(float(m.group(1))) if m else np.float32(np.nan)
        ab = 0 if m is None else min(na - 1, int(af * np.float32(na)))   # one float32 multiply
        qb = b // q_step
        counted += 1
        no_af += m is None
        G[0 if is_tp else 1, qb, ab] += 1
        if found and dot:
            best[key] = max(best.get(key, (-1, -1)), (qb, ab))
    for cell in best.values():
        G[2][cell] += 1
    S = G[:, ::-1, ::-1].cumsum(1).cumsum(2)[:, ::-1, ::-1]
    return S, [counted, no_af, no_bin, len(keys)]


def expected_tables(tmp, rows, q_step):
    from quasimodo_amd import surface as sf
    p = os.path.join(tmp, "want_best_filter.tsv")
    sf.write_caller_best_filter(p, rows, q_step)
    return _rd(p)


def check_job(j, S, extra, path):
    """a job's rows against the restatement, its ROC and its table"""
    from quasimodo_amd import surface as sf
    g = np.asarray(j.stats["surface"]).astype(np.int64)
    assert g.shape == (3, NQ, NA) and j.stats["surface_params"] == (Q, NQ, NA)
    bad = np.argwhere(g != S)
    assert bad.size == 0, "%s: S%s is %d, restated %d" % (j.vcf_file, tuple(bad[0]), g[tuple(bad[0])], S[tuple(bad[0])])
    assert j.stats["surface_extra"] == extra, j.vcf_file
    # the cell (QUAL >= 20, AF >= 0) is the ROC of the same call at t = 20: the reference's tp / fp line counts
    roc = np.asarray(j.stats["roc"])
    assert [int(g[c, 20 // Q, 0]) for c in range(3)] == [int(roc[c, 20]) for c in range(3)], j.vcf_file
    assert int(g[0, 20 // Q, 0]) == j.stats["tp_lines"] and int(g[1, 20 // Q, 0]) == j.stats["fp_lines"]
    assert _rd(path) == ("\n".join(sf.surface_rows(g, extra[3], Q)) + "\n").encode()


SNAPS = {}


@pytest.mark.parametrize("gpus", [1, 2])
def test_hcmv_six_callers(engine, tmp_path, gpus):
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), filter_surface=True, **kw)
    assert len(jobs) == 60
    exp = os.path.join(GOLDEN, "hcmv", "expected")
    truth = {mix: _rd(os.path.join(GOLDEN, "hcmv", "input", "nucmer", "%s.maskrepeat.variants.vcf" % mix)) for mix in ("TM", "TA")}
    rows, with_af = [], 0
    for j in jobs:
        base = os.path.basename(j.vcf_file)[:-4]
        smp, _, c = base.split(".")[:3]
        path = out / "results" / "snp" / "callers" / c / "surface" / (base + ".surface.tsv")
        if smp.endswith(("-1-0", "-0-1")):
            assert not path.exists() and "surface" not in j.stats, "pure-strain samples take no part"
            continue
        S, extra = restate(_rd(os.path.join(GOLDEN, "hcmv", "input", c, base + ".vcf")), _rd(os.path.join(exp, c, "tp", base + ".tp.vcf")),
                           truth[smp[:2]], "hcmv")
        check_job(j, S, extra, str(path))
        with_af += extra[0] - extra[1]
        rows.append((c, smp, j.stats["surface"], j.stats["surface_extra"]))
    assert len(rows) == 36 and with_af > 0, "some caller of the family writes AF"
    tables = out / "results" / "final_tables"
    assert (tables / "caller_best_filter.tsv").read_bytes() == expected_tables(str(tmp_path), rows, Q)
    new = _tree(str(out))
    mine = lambda tree: {f: v for f, v in tree.items() if "/surface/" in f or f.endswith("caller_best_filter.tsv")}
    added = mine(new)
    SNAPS[gpus] = added
    if gpus == 2:
        if 1 not in SNAPS:   # this case selected alone: the one-rank files are made here
            workflow.run_hcmv_variantcall(str(data), str(tmp_path / "one"), filter_surface=True, engine=engine)
            SNAPS[1] = mine(_tree(str(tmp_path / "one")))
        assert SNAPS[1] == added and len(added) == 36 + 1, "two ranks write the same files and table as one"
    if gpus == 1:
        # without the flag: every file of the output tree has the same bytes, and the flag adds only the surface files and the table
        off = tmp_path / "off"
        plain = workflow.run_hcmv_variantcall(str(data), str(off), engine=engine)
        old = _tree(str(off))
        assert set(new) - set(old) == set(added) and not set(old) - set(new) and len(added) == 36 + 1
        differing = [f for f in old if old[f] != new[f]]
        assert not differing, differing
        assert len(old) > 300 and "results/final_tables/caller_performance.tsv" in old
        for p, j in zip(plain, jobs):                                    # stats and roc are those of a call without the flag
            for k, v in p.stats.items():
                same = (v is None and j.stats[k] is None) or np.array_equal(np.asarray(v), np.asarray(j.stats[k])) if k == "roc" else v == j.stats[k]
                assert same, (j.vcf_file, k)


@pytest.mark.parametrize("gpus", [1, 2])
def test_custom_three_labels(engine, tmp_path, gpus):
    from quasimodo_amd import workflow
    cs = [e for e in golden_cases() if e["family"] == "custom"]
    assert len(cs) == 3
    vcfs, texts, labels = [], [], []
    for e in cs:
        vcf, truth, exp = read_case(e)
        p = tmp_path / os.path.basename(e["vcf"])
        p.write_bytes(vcf)
        vcfs.append(str(p))
        texts.append((vcf, exp["tp"]))
        labels.append(e["caller"])
    snps = tmp_path / "g1_g2.maskrepeat.snps"
    snps.write_bytes(truth)
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    out = tmp_path / "o"
    jobs = workflow.run_vareval(vcfs, str(snps), str(out), labels=labels, filter_surface=True, **kw)
    rows = []
    for lab, j, (vcf, tp) in zip(labels, jobs, texts):
        S, extra = restate(vcf, tp, truth, "custom")
        check_job(j, S, extra, str(out / "results" / "snp" / "callers" / "surface" / (lab + ".surface.tsv")))
        rows.append((lab, "custom", j.stats["surface"], j.stats["surface_extra"]))
    assert (out / "results" / "final_tables" / "caller_best_filter.tsv").read_bytes() == expected_tables(str(tmp_path), rows, Q)
    plain = tmp_path / "plain"
    workflow.run_vareval(vcfs, str(snps), str(plain), labels=labels, engine=engine)
    old, new = _tree(str(plain)), _tree(str(out))
    assert sorted(set(new) - set(old)) == sorted(["results/final_tables/caller_best_filter.tsv"] +
                                                 ["results/snp/callers/surface/%s.surface.tsv" % lab for lab in labels])
    assert not set(old) - set(new) and not [f for f in old if old[f] != new[f]]


def test_extract_many_surface_another_grid_and_the_pure_strain_refusal(engine, tmp_path):
    import shutil
    from quasimodo_amd._lib import QmvtError
    from quasimodo_amd.extract import Job, extract_many
    fam = os.path.join(GOLDEN, "hcmv")
    cases = [e for e in golden_cases() if e["family"] == "hcmv"]
    mixed = [e for e in cases if not e["pure"]][:4]
    pure = [e for e in cases if e["pure"]][:1]
    assert len(mixed) == 4 and len(pure) == 1

    def jobs_of(es, root):
        out = []
        for e in es:
            d = os.path.join(root, os.path.dirname(e["vcf"]))
            os.makedirs(d, exist_ok=True)
            dst = os.path.join(d, os.path.basename(e["vcf"]))
            shutil.copyfile(os.path.join(fam, e["vcf"]), dst)
            out.append(Job(dst, os.path.join(fam, e["truth"]), "hcmv"))
        return out
    # the keyword sweeps the mixed samples and leaves the pure strain alone
    jobs = extract_many(jobs_of(mixed + pure, str(tmp_path / "a")), engine=engine, surface={"q_step": 5, "nq": 8, "na": 7})
    for e, j in zip(mixed, jobs):
        S, extra = restate(_rd(os.path.join(fam, e["vcf"])), _rd(os.path.join(fam, e["expected"]["tp"])), _rd(os.path.join(fam, e["truth"])),
                           "hcmv", 5, 8, 7)
        assert np.array_equal(np.asarray(j.stats["surface"]).astype(np.int64), S) and j.stats["surface_extra"] == extra
        assert j.stats["surface_params"] == (5, 8, 7)
        assert _rd(j.filtered_out) == _rd(os.path.join(fam, e["expected"]["filtered"]))
    assert "surface" not in jobs[-1].stats and jobs[-1].surface is None
    # a pure-strain job that asks by its own field is refused by name, in front of any output
    asked = jobs_of(mixed[:1] + pure, str(tmp_path / "b"))
    for j in asked:
        j.surface = (4, 64, 50)
    with pytest.raises(QmvtError, match="pure-strain") as e:
        extract_many(asked, engine=engine)
    assert e.value.code == -1 and os.path.basename(asked[1].vcf_file) in str(e.value)
    assert not os.path.exists(asked[0].filtered_out)
