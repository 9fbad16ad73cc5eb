"""The near-miss classes end to end (qm_extract_files_nearmiss, extract_many(explain=), --explain-errors): the
golden hcmv family with its six callers and the custom family with its three labels against a restatement on TEXT -- the lines
of the golden *.fp.vcf and *.filtered.vcf files, the input VCF's lines, the truth file's rows and truthside.fn_text -- never the
engine's packing."""
import os
import re

import pytest

from conftest import GOLDEN, golden_cases, read_case

pytestmark = pytest.mark.gpu

BASES = (b"A", b"C", b"G", b"T")


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
    """[(1-based line number, fields)] of the lines that do not start with '#'"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [(i + 1, ln.split(b"\t")) for i, ln in enumerate(lines) if not ln.startswith(b"#")]


def _pos(text):
    """the position of a canonical POS text (what gives a line a usable position), else None"""
    return int(text) if re.fullmatch(rb"0|[1-9][0-9]*", text) and int(text) < 1 << 28 else None


class Calls:
    """the lines of one input VCF as the classes see them: (pos, REF, ALT, kept), REF / ALT None when not a single base"""

    def __init__(self, vcf_text, filtered_text):
        kept_lines = {b"\t".join(f) for _, f in _data_lines(filtered_text)}
        self.at = {}
        for _, f in _data_lines(vcf_text):
            p = _pos(f[1]) if len(f) >= 5 else None
            if p is None:
                continue
            single = f[3] in BASES and f[4] in BASES
            self.at.setdefault(p, []).append((f[3] if single else None, f[4] if single else None, b"\t".join(f) in kept_lines))


def _col(f, i):
    return f[i] if i < len(f) else b""


def fp_class(f, truth_at, radius):
    """the class of one FP line from its text; truth_at: {pos: {(REF, ALT)}} of the truth set's single-base rows"""
    p = _pos(_col(f, 1))
    if p is None or _col(f, 3) not in BASES or _col(f, 4) not in BASES:
        return "nokey"
    here = truth_at.get(p, set())
    if (f[3], f[4]) in here:
        return "idcol"
    if any(r == f[3] for r, a in here):
        return "allele"
    if here:
        return "refbase"
    if any(truth_at.get(p + d) for d in range(-radius, radius + 1) if d):
        return "near"
    return "isolated"


def fn_class(p, ref, alt, calls, radius):
    """the class of one missed truth key from the text of the VCF's lines"""
    here = calls.at.get(p, [])
    if any(r == ref and a == alt and not kept for r, a, kept in here):
        return "filtered"
    if any(r == ref and a is not None and a != alt for r, a, kept in here):
        return "allele"
    if here:
        return "position"
    if any(calls.at.get(p + d) for d in range(-radius, radius + 1) if d):
        return "near"
    return "uncalled"


def restate(vcf_text, filtered_text, fp_text, truth_text, mode, radius):
    """(the fp.why text, the fn.why text, rec [6], tru [5]) of one job"""
    from quasimodo_amd import nearmiss as nm
    from quasimodo_amd import truthside as ts
    cols = (1, 3, 4) if mode == "hcmv" else (0, 1, 2)
    trows = [tuple(f[c] for c in cols) for _, f in _data_lines(truth_text) if len(f) > cols[2]]
    truth_at = {}
    for pt, r, a in trows:
        if _pos(pt) is not None and r in BASES and a in BASES:
            truth_at.setdefault(_pos(pt), set()).add((r, a))
    # the FP lines: the data lines of the golden fp.vcf, found again in the input file in order (equal lines are classified alike)
    inp = _data_lines(vcf_text)
    k, fp_rows, rec = 0, [], [0] * 6
    for _, f in _data_lines(fp_text):
        while inp[k][1] != f:
            k += 1
        c = fp_class(f, truth_at, radius)
        fp_rows.append(b"\t".join([b"%d" % inp[k][0]] + [_col(f, i) for i in (1, 3, 4, 5)] + [c.encode()]))
        rec[nm.RECORD_CLASSES.index(c)] += 1
        k += 1
    calls = Calls(vcf_text, filtered_text)
    kept = ts.snp_keys(filtered_text)
    # the missed rows: those of the missed-variant list, in its order
    if mode == "hcmv":
        missed = [(f[1], f[3], f[4]) for _, f in _data_lines(ts.fn_text(truth_text, kept))]
    else:
        missed = [t for t in trows if t[1] != b"." and t[2] != b"." and t not in kept]
    fn_rows = []
    for pt, r, a in missed:
        held = _pos(pt) is not None and r in BASES and a in BASES
        c = fn_class(_pos(pt), r, a, calls, radius) if held else "."
        fn_rows.append(b"\t".join([pt, r, a, c.encode()]))
    tru = [0] * 5
    for p, ra in truth_at.items():
        for r, a in ra:
            if (b"%d" % p, r, a) not in kept:
                tru[nm.TRUTH_CLASSES.index(fn_class(p, r, a, calls, radius))] += 1
    text = lambda head, rows: b"".join(ln + b"\n" for ln in [head.encode()] + rows)
    return text(nm.FP_WHY_HEADER, fp_rows), text(nm.FN_WHY_HEADER, fn_rows), rec, tru


def expected_table(tmp, rows):
    from quasimodo_amd import nearmiss as nm
    nm.write_caller_error_classes(os.path.join(tmp, "want_classes.tsv"), rows)
    return _rd(os.path.join(tmp, "want_classes.tsv"))


SNAPS = {}


@pytest.mark.parametrize("gpus", [1, 2])
def test_hcmv_six_callers(engine, tmp_path, gpus):
    from quasimodo_amd import nearmiss as nm
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = tmp_path / "data" / "snp"
    _build_bundle(str(data))
    out = tmp_path / "out"
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    jobs = workflow.run_hcmv_variantcall(str(data), str(out), explain_errors=True, **kw)
    assert len(jobs) == 60
    exp = os.path.join(GOLDEN, "hcmv", "expected")
    truth = {mix: _rd(os.path.join(GOLDEN, "hcmv", "input", "nucmer", "%s.maskrepeat.variants.vcf" % mix)) for mix in ("TM", "TA")}
    rows, seen = [], set()
    for j in jobs:
        base = os.path.basename(j.vcf_file)[:-4]
        smp, _, c = base.split(".")[:3]
        why = out / "results" / "snp" / "callers" / c / "why"
        if smp.endswith(("-1-0", "-0-1")):
            assert not (why / (base + ".fp.why.tsv")).exists() and "nearmiss_rec" not in j.stats, "pure-strain samples take no part"
            continue
        w_fp, w_fn, rec, tru = restate(_rd(os.path.join(GOLDEN, "hcmv", "input", c, base + ".vcf")), _rd(os.path.join(exp, c, base + ".filtered.vcf")),
                                       _rd(os.path.join(exp, c, "fp", base + ".fp.vcf")), truth[smp[:2]], "hcmv", nm.DEFAULT_RADIUS)
        assert (why / (base + ".fp.why.tsv")).read_bytes() == w_fp, base
        assert (why / (base + ".fn.why.tsv")).read_bytes() == w_fn, base
        assert j.stats["nearmiss_rec"] == rec and j.stats["nearmiss_tru"] == tru and j.stats["nearmiss_radius"] == 10, base
        assert sum(rec) == j.stats["fp_lines"] and sum(tru) == j.stats["truth_unique"] - j.stats["TP_R"]
        assert [r[5] for r in nm.read_fp_why(str(why / (base + ".fp.why.tsv")))].count("near") == rec[3]
        rows.append((c, smp, rec, tru))
        seen |= {("FP", n) for n, x in zip(nm.RECORD_CLASSES, rec) if x} | {("FN", n) for n, x in zip(nm.TRUTH_CLASSES, tru) if x}
    assert len(rows) == 36
    print("classes seen over the family: %s" % sorted(seen))
    tables = out / "results" / "final_tables"
    assert (tables / "caller_error_classes.tsv").read_bytes() == expected_table(str(tmp_path), rows)
    new = _tree(str(out))
    mine = lambda tree: {f: v for f, v in tree.items() if "/why/" in f or f.endswith("caller_error_classes.tsv")}
    added = mine(new)
    SNAPS[gpus] = added
    if gpus == 2:
        if 1 not in SNAPS:   # this case selected alone: the one-rank files are made here
            workflow.run_hcmv_variantcall(str(data), str(tmp_path / "one"), explain_errors=True, engine=engine)
            SNAPS[1] = mine(_tree(str(tmp_path / "one")))
        assert SNAPS[1] == added and len(added) == 2 * 36 + 1, "two ranks write the same files and table as one"
    if gpus == 1:
        # without the flag: every file of the output tree has the same bytes, and the flag adds only the why-files and the table
        off = tmp_path / "off"
        workflow.run_hcmv_variantcall(str(data), str(off), engine=engine)
        old = _tree(str(off))
        assert set(new) - set(old) == set(added) and not set(old) - set(new) and len(added) == 2 * 36 + 1
        differing = [f for f in old if old[f] != new[f]]
        assert not differing, differing
        assert len(old) > 300 and "results/final_tables/caller_performance.tsv" in old


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
        texts.append((vcf, exp["filtered"], exp["fp"]))
        labels.append(e["caller"])
    snps = tmp_path / "g1_g2.maskrepeat.snps"
    snps.write_bytes(truth)
    kw = dict(engine=engine) if gpus == 1 else dict(gpus=2, _backend="gloo", _same_device=True)
    for radius in ((0, 3) if gpus == 1 else (3,)):   # (two ranks: one run is enough to compare the files)
        out = tmp_path / ("o%d" % radius)
        jobs = workflow.run_vareval(vcfs, str(snps), str(out), labels=labels, explain_errors=True, explain_radius=radius, **kw)
        rows = []
        for lab, j, (vcf, filtered, fp) in zip(labels, jobs, texts):
            w_fp, w_fn, rec, tru = restate(vcf, filtered, fp, truth, "custom", radius)
            why = out / "results" / "snp" / "callers" / "why"
            assert (why / (lab + ".fp.why.tsv")).read_bytes() == w_fp, lab
            assert (why / (lab + ".fn.why.tsv")).read_bytes() == w_fn, lab
            assert j.stats["nearmiss_rec"] == rec and j.stats["nearmiss_tru"] == tru
            assert b"\t.\n" in w_fn, "the table has rows the device cannot hold"
            rows.append((lab, "custom", rec, tru))
        assert (out / "results" / "final_tables" / "caller_error_classes.tsv").read_bytes() == expected_table(str(tmp_path), rows)
    plain = tmp_path / "plain"
    workflow.run_vareval(vcfs, str(snps), str(plain), labels=labels, engine=engine)
    old, new = _tree(str(plain)), _tree(str(tmp_path / "o3"))
    assert sorted(set(new) - set(old)) == sorted(["results/final_tables/caller_error_classes.tsv"] +
                                                 ["results/snp/callers/why/%s.%s.why.tsv" % (lab, s) for lab in labels for s in ("fp", "fn")])
    assert not set(old) - set(new) and not [f for f in old if old[f] != new[f]]


@pytest.mark.parametrize("case", [e for e in golden_cases() if e["family"] == "quirks"], ids=lambda e: e["mode"])
def test_quirks_job_with_a_kept_nokey_line(engine, tmp_path, case):
    """asking for fn_why_out is refused by name; fp_why_out alone goes through and such lines are class nokey"""
    import shutil
    from quasimodo_amd import nearmiss as nm
    from quasimodo_amd._lib import QmvtError
    from quasimodo_amd.extract import Job, extract_many
    fam = os.path.join(GOLDEN, "quirks")
    vcf = tmp_path / os.path.basename(case["vcf"])
    shutil.copyfile(os.path.join(fam, case["vcf"]), vcf)
    job = Job(str(vcf), os.path.join(fam, case["truth"]), case["mode"], str(tmp_path / "o"), "q")
    with pytest.raises(QmvtError) as e:
        extract_many([job], engine=engine, explain=2)
    m = re.search(r"line (\d+)", str(e.value))
    assert e.value.code == -8 and os.path.basename(str(vcf)) in str(e.value) and m, str(e.value)
    f = _rd(str(vcf)).split(b"\n")[int(m.group(1)) - 1].split(b"\t")
    assert re.fullmatch(rb"0|[1-9][0-9]*", f[1]) is None or int(f[1]) >= 1 << 28, "the named line has a canonical POS"
    assert not os.path.exists(job.fn_why_out) and not os.path.exists(job.fp_why_out)
    # the FP side alone
    only = Job(str(vcf), os.path.join(fam, case["truth"]), case["mode"], str(tmp_path / "p"), "q", explain=2,
               fp_why_out=str(tmp_path / "p" / "q.fp.why.tsv"))
    extract_many([only], engine=engine)
    assert _rd(only.filtered_out) == _rd(os.path.join(fam, case["expected"]["filtered"]))
    w_fp, _, rec, _ = restate(_rd(str(vcf)), _rd(os.path.join(fam, case["expected"]["filtered"])), _rd(os.path.join(fam, case["expected"]["fp"])),
                              _rd(os.path.join(fam, case["truth"])), case["mode"], 2)
    assert _rd(only.fp_why_out) == w_fp and only.stats["nearmiss_rec"] == rec
    assert "nokey" in [r[5] for r in nm.read_fp_why(only.fp_why_out)] and only.fn_why_out is None
