#!/usr/bin/env python3
"""Record what the two workflows and their command lines SAY, without a device: the dry-run text or the refusal of
run_hcmv_variantcall and run_vareval over a fixed matrix of keywords, the --help text of `run_benchmark.py hcmv` and `vareval`,
and the refusals of the command line.  tests/test_workflow_text_host.py replays the matrix and compares exactly.

  python tools/record_workflow_text.py          writes tests/golden/workflow_text/{hcmv,vareval,cli}.json

The fixture is recorded at the commit BEFORE a change to workflow.py or run_benchmark.py that is meant to keep the text; a
change that is meant to alter a message records it anew and shows the difference in its diff.

The matrix: every pass keyword alone, every parameter keyword alone, every pair of those, each with `alleles` off and on (hcmv);
for each numeric parameter one value below and one above its range beside its pass; a missing FASTA per genome-taking pass.
A case is recorded as {"out": stdout} or {"error": "Class: text"}; the pairs that succeed keep a sha256 of their stdout only.
The files hold the records packed (pack / unpack below): 0.14 MB."""
import contextlib
import hashlib
import io
import itertools
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
FIXTURES = os.path.join(ROOT, "tests", "golden", "workflow_text")
TMP = "<TMP>"

# keyword -> the value that asks for it; G stands for the genomes ({"TM": fa, "TA": fa} for hcmv, the FASTA for vareval)
G = object()
STRATA = [("low", [1, 50], [10, 60]), ("high", [100], [200])]
HCMV_PASSES = {"mutation_context": G, "truth_side": True, "snp_profile": True, "strata": STRATA, "bootstrap": 10, "votes": True,
               "explain_errors": True, "filter_surface": True, "seq_context": G, "normalize": G, "atomize": True, "by_type": True,
               "haplotypes": G, "hap_subsets": True, "rescue_roc": G, "match_ladder": G, "ladder_by_type": G}
HCMV_PARAMS = {"consensus_vcf": 2, "explain_radius": 5, "surface_qual_step": 2, "surface_qual_bins": 32, "surface_af_bins": 25,
               "context_window": 20, "context_gc_bins": 5, "hap_gap": 4, "ladder_type_bins": "1,2,6"}
# (pass keywords, parameter, below, above): the parameter beside its pass, out of range on either side
HCMV_RANGES = [({"explain_errors": True}, "explain_radius", -1, 65), ({"filter_surface": True}, "surface_qual_step", 0, 3),
               ({"filter_surface": True}, "surface_qual_bins", 0, 257), ({"filter_surface": True}, "surface_af_bins", 0, 65),
               ({"seq_context": G}, "context_window", -1, 1025), ({"seq_context": G}, "context_gc_bins", 0, 16),
               ({"haplotypes": G}, "hap_gap", -1, 33), ({"haplotypes": G, "hap_subsets": True}, "hap_gap", -1, 33),
               ({"match_ladder": G}, "hap_gap", -1, 33), ({"ladder_by_type": G}, "hap_gap", -1, 33),
               ({"ladder_by_type": G}, "ladder_type_bins", "0,2", "1,2,2"), ({}, "by_type", "0,2", "1,2,2"),
               ({"ladder_by_type": G}, "ladder_type_bins", [2, 3], list(range(1, 19))), ({}, "by_type", [2, 3], list(range(1, 19))),
               ({}, "consensus_vcf", 0, 7), ({}, "bootstrap", 0, 1 << 20),
               ({}, "bootstrap", {"n_rep": 10, "window": 0}, {"n_rep": 10, "window": 1 << 31}),
               ({}, "snp_profile", {"window": 0}, {"n_pos_bins": 256, "n_af_bins": 64}),
               ({}, "strata", [("a", [5], [1])], [("a", [1], [2]), ("a", [3], [4])])]
HCMV_GENOMES = ("mutation_context", "seq_context", "normalize", "rescue_roc", "haplotypes", "match_ladder", "ladder_by_type")

VAREVAL_PASSES = {"truth_side": True, "strata": STRATA, "bootstrap": 10, "votes": True, "explain_errors": True, "filter_surface": True,
                  "seq_context": G}
VAREVAL_PARAMS = {k: v for k, v in HCMV_PARAMS.items() if k not in ("hap_gap", "ladder_type_bins")}
VAREVAL_RANGES = [r for r in HCMV_RANGES if set(r[0]) | {r[1]} <= set(VAREVAL_PASSES) | set(VAREVAL_PARAMS)]
# label sets: two VCFs; six (past the Venn group of five); thirty-three (past the vote group); a pure-strain name among them
VAREVAL_LABELS = {"2": ["a", "b"], "6": list("abcdef"), "33": ["v%02d" % i for i in range(33)], "pure": ["a", "TA-1-0"]}


def _fill(kw, genomes):
    return {k: genomes if v is G else v for k, v in kw.items()}


def _case(fn, args, kw, tmp, full):
    """one call -> its record"""
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            fn(*args, dryrun=True, **kw)
    except Exception as e:
        said = buf.getvalue().replace(tmp, TMP)
        rec = {"error": ("%s: %s" % (type(e).__name__, e)).replace(tmp, TMP)}
        if said:
            rec["out"] = said
        return rec
    out = buf.getvalue().replace(tmp, TMP)
    return {"out": out} if full else {"sha256": hashlib.sha256(out.encode()).hexdigest()}


def _say(v):
    return "G" if v is G else json.dumps(v, separators=(",", ":"))


def _matrix(passes, params, ranges):
    """[(id, keywords, full)]: the keywords still hold G"""
    one = list(passes.items()) + list(params.items())
    out = [("none", {}, True)]
    out += [(k, {k: v}, True) for k, v in one]
    out += [("%s+%s" % (a[0], b[0]), dict([a, b]), False) for a, b in itertools.combinations(one, 2)]
    for base, name, lo, hi in ranges:
        for v in (lo, hi):
            out.append(("+".join(list(base) + ["%s=%s" % (name, _say(v))]), dict(base, **{name: v}), True))
    return out


def record_hcmv(tmp):
    from quasimodo_amd import workflow
    from test_tables_workflow import _build_bundle
    data = os.path.join(tmp, "data", "snp")
    _build_bundle(data)
    fa = os.path.join(tmp, "g.fa")
    with open(fa, "w") as fh:
        fh.write(">g\nACGT\n")
    genomes = {"TM": fa, "TA": fa}
    out = {}
    for cid, kw, full in _matrix(HCMV_PASSES, HCMV_PARAMS, HCMV_RANGES):
        for alleles in (False, True):
            out["%s|alleles=%d" % (cid, alleles)] = _case(workflow.run_hcmv_variantcall, (data, os.path.join(tmp, "out")),
                                                          dict(_fill(kw, genomes), alleles=alleles), tmp, full)
    for k in HCMV_GENOMES:     # a missing FASTA: no entry for TA, a path that is no file for TM
        for what, g in (("TA=None", {"TM": fa, "TA": None}), ("TM=missing", {"TM": os.path.join(tmp, "no.fa"), "TA": fa})):
            out["%s|%s|alleles=1" % (k, what)] = _case(workflow.run_hcmv_variantcall, (data, os.path.join(tmp, "out")),
                                                       {k: g, "alleles": True}, tmp, True)
    out["callers=lofreq,clc|consensus_vcf=3"] = _case(workflow.run_hcmv_variantcall, (data, os.path.join(tmp, "out")),
                                                       {"callers": ["lofreq", "clc"], "votes": True, "consensus_vcf": 3}, tmp, True)
    for k in ("truth_side", "votes", "mutation_context", "snp_profile"):
        out["callers=lofreq,clc|%s" % k] = _case(workflow.run_hcmv_variantcall, (data, os.path.join(tmp, "out")),
                                                  dict(_fill({k: HCMV_PASSES[k]}, genomes), callers=["lofreq", "clc"]), tmp, True)
    return out


def record_vareval(tmp):
    from quasimodo_amd import workflow
    fa = os.path.join(tmp, "g.fa")
    with open(fa, "w") as fh:
        fh.write(">g\nACGT\n")
    snps = os.path.join(tmp, "g1_g2.maskrepeat.snps")
    out = {}
    for lname, labels in VAREVAL_LABELS.items():
        vcfs = [os.path.join(tmp, "in", "%s.vcf" % lab) for lab in labels]
        matrix = _matrix(VAREVAL_PASSES, VAREVAL_PARAMS, VAREVAL_RANGES if lname == "2" else [])
        for cid, kw, full in matrix:
            if lname != "2" and len(kw) > 1 and not {"votes", "truth_side", "consensus_vcf"} & set(kw):
                continue        # the other label sets differ from the first in what votes and truth_side say
            out["%s|labels=%s" % (cid, lname)] = _case(workflow.run_vareval, (vcfs, snps, os.path.join(tmp, "out")), _fill(kw, fa), tmp, full)
    vcfs = [os.path.join(tmp, "in", "%s.vcf" % lab) for lab in "ab"]
    out["seq_context|missing"] = _case(workflow.run_vareval, (vcfs, snps, os.path.join(tmp, "out")), {"seq_context": os.path.join(tmp, "no.fa")}, tmp, True)
    out["labels=3 for 2 vcfs"] = _case(workflow.run_vareval, (vcfs, snps, os.path.join(tmp, "out")), {"labels": ["x", "y", "z"]}, tmp, True)
    out["labels=x,y|explain_errors"] = _case(workflow.run_vareval, (vcfs, snps, os.path.join(tmp, "out")), {"labels": ["x", "y"], "explain_errors": True}, tmp, True)
    return out


# the command lines: (id, arguments); B stands for the bundle, O for the output directory, F for the FASTA, V for two VCF paths
HCMV_FLAGS = ("--mutation-context", "--truth-side", "--snp-profile", "--bootstrap 10", "--votes", "--consensus-vcf 2", "--explain-errors",
              "--explain-errors --explain-radius 3", "--filter-surface", "--filter-surface --surface-qual-step 2 --surface-qual-bins 32 --surface-af-bins 25",
              "--seq-context", "--seq-context --context-window 20 --context-gc-bins 5", "--normalize", "--atomize", "--rescue-roc", "--match-ladder",
              "--match-ladder --hap-gap 3", "--ladder-by-type", "--ladder-by-type --type-bins 1,2,6 --hap-gap 3", "--by-type", "--by-type --type-bins 1,2,6",
              "--by-type --ladder-by-type --type-bins 1,2,6", "--haplotypes", "--haplotypes --hap-gap 3", "--hap-subsets", "--hap-subsets --hap-gap 3",
              "--mutation-context --snp-profile --profile-window 512 --profile-pos-bins 16 --profile-af-bins 10", "--strata S1 --strata S2", "--strata-by-name S1",
              "--bootstrap 10 --bootstrap-window 512 --bootstrap-seed 7")
VAREVAL_FLAGS = ("--truth-side", "--strata S1", "--strata-by-name S1", "--bootstrap 10 --bootstrap-window 512 --bootstrap-seed 7", "--votes", "--consensus-vcf 2",
                 "--explain-errors --explain-radius 3", "--filter-surface --surface-qual-step 2", "--seq-context --context-window 20 --context-gc-bins 5")
VAREVAL_REFUSED = ("--ladder-by-type", "--match-ladder", "--rescue-roc", "--hap-subsets", "--haplotypes", "--hap-gap 3", "--by-type", "--type-bins 1,2",
                   "--atomize", "--normalize", "--normalize --atomize --by-type --haplotypes --hap-subsets --rescue-roc --match-ladder --ladder-by-type",
                   "--atomize --normalize", "--type-bins 1,2 --hap-gap 3", "--strata S1 --strata-by-name S1")


def record_cli(tmp):
    import importlib.util
    import re
    from click.testing import CliRunner
    from test_tables_workflow import _build_bundle
    spec = importlib.util.spec_from_file_location("run_benchmark", os.path.join(ROOT, "run_benchmark.py"))
    rb = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rb)
    data = os.path.join(tmp, "data", "snp")
    if not os.path.isdir(data):
        _build_bundle(data)
    fa = os.path.join(tmp, "g.fa")
    with open(fa, "w") as fh:
        fh.write(">g\nACGT\n")
    bed = os.path.join(tmp, "low.bed")
    with open(bed, "w") as fh:
        fh.write("g\t0\t10\tlow\ng\t50\t60\thigh\n")
    bed2 = os.path.join(tmp, "high.bed")
    with open(bed2, "w") as fh:
        fh.write("g\t100\t200\thigh\n")
    hcmv = ["hcmv", "-e", "variantcall", "-d", "--data", data, "-o", os.path.join(tmp, "out"), "--merlin-ref", fa, "--ad169-ref", fa]
    vareval = ["vareval", "-d", "-v", "%s,%s" % (os.path.join(tmp, "in", "a.vcf"), os.path.join(tmp, "in", "b.vcf")), "-r", "%s,%s" % (fa, fa),
               "-o", os.path.join(tmp, "out")]
    words = lambda s: [{"S1": bed, "S2": bed2}.get(w, w) for w in s.split()]
    runs = [("hcmv --help", ["hcmv", "--help"]), ("vareval --help", ["vareval", "--help"])]
    runs += [("hcmv " + f, hcmv + words(f)) for f in ("",) + HCMV_FLAGS]
    runs += [("hcmv --alleles " + f, hcmv + ["--alleles"] + words(f)) for f in ("",) + HCMV_FLAGS]
    runs += [("hcmv " + f, hcmv + words(f)) for f in ("--hap-gap 3", "--type-bins 1,2", "--strata S1 --strata-by-name S1", "--alleles --hap-gap 3",
                                                      "--alleles --type-bins 1,2", "--alleles --normalize --atomize")]
    runs += [("vareval " + f, vareval + words(f)) for f in ("",) + VAREVAL_FLAGS + VAREVAL_REFUSED]
    stamp = re.compile(r"^\d{4}-\d\d-\d\d \d\d:\d\d\t", re.M)
    out = {}
    for cid, args in runs:
        r = CliRunner().invoke(rb.cli, args, terminal_width=80)
        rec = {"exit": r.exit_code, "stdout": stamp.sub("<TIME>\t", r.stdout.replace(tmp, TMP)), "stderr": r.stderr.replace(tmp, TMP)}
        if r.exception is not None and not isinstance(r.exception, SystemExit):
            rec["exception"] = ("%s: %s" % (type(r.exception).__name__, r.exception)).replace(tmp, TMP)
        out[cid] = rec
    return out


RECORDERS = {"hcmv": record_hcmv, "vareval": record_vareval, "cli": record_cli}


def record(name):
    with tempfile.TemporaryDirectory(prefix="qmtext") as tmp:
        return RECORDERS[name](os.path.realpath(tmp))


# The fixture files are packed: the lines that every dry run of a command prints alike (its plan: one line per VCF) are kept once, as
# named blocks, and stand in the records as <name>; cases with the same record share one line.  unpack(pack(x)) == x.
BLOCKS = {"hcmv": {"<PLAN>": ("none|alleles=0", "out")},
          "vareval": {"<PLAN %s>" % n: ("none|labels=%s" % n, "out") for n in VAREVAL_LABELS},
          "cli": {"<PLAN hcmv>": ("hcmv ", "stdout"), "<PLAN vareval>": ("vareval ", "stdout")}}


def pack(name, records):
    blocks = {token: records[cid][field] for token, (cid, field) in BLOCKS[name].items()}
    assert not any(token in v for r in records.values() for v in r.values() if isinstance(v, str) for token in blocks)

    def short(v):
        for token in sorted(blocks, key=lambda t: -len(blocks[t])):
            v = v.replace(blocks[token], token) if isinstance(v, str) else v
        return v
    same = {}
    for cid in sorted(records):
        same.setdefault(json.dumps({k: short(v) for k, v in records[cid].items()}, sort_keys=True), []).append(cid)
    return {"blocks": blocks, "records": [[json.loads(r), ids] for r, ids in same.items()]}


def unpack(doc):
    def whole(v):
        for token, text in doc["blocks"].items():
            v = v.replace(token, text) if isinstance(v, str) else v
        return v
    return {cid: {k: whole(v) for k, v in r.items()} for r, ids in doc["records"] for cid in ids}


def load(name):
    with open(os.path.join(FIXTURES, name + ".json")) as fh:
        return unpack(json.load(fh))


def save(name, records):
    doc = pack(name, records)
    assert unpack(doc) == records
    os.makedirs(FIXTURES, exist_ok=True)
    with open(os.path.join(FIXTURES, name + ".json"), "w") as fh:
        fh.write('{"blocks": %s,\n"records": [\n%s\n]}\n' % (json.dumps(doc["blocks"], sort_keys=True), ",\n".join(json.dumps(e) for e in doc["records"])))


def main():
    for name in RECORDERS:
        rec = record(name)
        save(name, rec)
        print("%s: %d cases, %d without an error" % (name, len(rec), sum(1 for r in rec.values() if "error" not in r and not r.get("exit"))))


if __name__ == "__main__":
    main()
