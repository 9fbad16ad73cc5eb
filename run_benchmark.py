#!/usr/bin/env python3
"""run_benchmark.py -- the reference's CLI surface (run_benchmark.py:62-192) for the commands
that sit on the accelerated path.

  hcmv    -e variantcall   TP/FP extraction + caller_performance.tsv + FP overlap counts on the bundled VCFs
  vareval                  the same for user VCFs against a precomputed genome difference

Everything that is not this path (read mapping, variant calling, nucmer, assembly evaluation,
figures) is out of scope and reported as such; `asmeval` and `-e assembly` exit with status 2."""
import os
import sys

import click

wd = os.path.dirname(os.path.realpath(__file__))
sys.path.insert(0, wd)
VERSION = "0.4.2"
cd = os.getcwd()


def print_version(ctx, param, value):
    if not value or ctx.resilient_parsing:
        return
    click.echo("Version {}".format(VERSION))
    ctx.exit()


@click.group()
@click.option("--version", is_flag=True, callback=print_version, expose_value=False, is_eager=True, help="Print the version.")
def cli():
    pass


def common_options(f):
    for opt in reversed([
        click.option("-d", "--dryrun", is_flag=True, default=False, show_default=True, help="Print the details without run the pipeline."),
        click.option("-t", "--threads", type=int, default=2, show_default=True, help="The number of threads to use."),
        click.option("-c", "--conda_prefix", type=click.Path(exists=True), default=None, help="Accepted for compatibility; unused."),
        click.option("-o", "--outpath", type=click.Path(), default=None, help="The directory where to put the results."),
        click.option("--gpus", type=int, default=1, show_default=True, help="GPUs of this node to shard the VCFs over (one process each)."),
        click.option("--json", "json_out", type=click.Path(), default=None,
                     help="Also write the run's statistics as JSON: one row per VCF (counts, whether it was in position order) and "
                          "where the VCFs that were not went (bucket paths / radix sort)."),
    ]):
        f = opt(f)
    return f


def _write_json(path, command, jobs, workflow_fn):
    """--json: a side file; the declared outputs are untouched (metrics / logging)."""
    import json
    from quasimodo_amd.extract import extract_many
    res = getattr(workflow_fn, "last_result", None)
    paths = res.get("paths") if res else extract_many.last_paths
    rows = []
    for j in jobs or []:
        st = j.stats or {}
        row = {k: int(st[k]) for k in ("n_records", "n_pass", "tp_lines", "fp_lines", "TP_R", "FP_R", "genomediff", "truth_unique", "sorted") if k in st}
        if st.get("motifs") is not None:   # (--mutation-context) kept SNVs outside the 96 motifs, and REF mismatches
            row.update(motif_other=int(st["motifs"][0][96]), motif_ref_mismatch=int(st["motifs"][0][97]))
        rows.append(dict(vcf=j.vcf_file, filtered=j.filtered_out, tp=j.tp_out, fp=j.fp_out, pure_strain=bool(st.get("pure_strain")), **row))
    with open(os.path.join(cd, path), "w") as fh:
        json.dump({"command": command, "rows": rows, "unsorted_paths": paths,
                   "phases_seconds": None if res else extract_many.last_phases}, fh, indent=1)


def _fail(e):
    from datetime import datetime
    print("ERROR")
    print("{}\t{}\n".format(datetime.now().isoformat(" ", timespec="minutes"), e))
    raise RuntimeError(e)


def _read_strata(files, by_name):
    """--strata / --strata-by-name -> a list of (name, starts, ends), or None when neither is given"""
    if not files and not by_name:
        return None
    if files and by_name:
        raise ValueError("--strata and --strata-by-name cannot be combined")
    from quasimodo_amd.strata import read_bed, read_bed_by_name
    if by_name:
        return read_bed_by_name(os.path.join(cd, by_name))
    return [read_bed(os.path.join(cd, f)) for f in files]


def _bootstrap_opts(n_rep, window, seed):
    """--bootstrap / --bootstrap-window / --bootstrap-seed -> what the workflows take, or None without --bootstrap"""
    return None if n_rep is None else {"n_rep": n_rep, "window": window, "seed": seed}


def _hap_gap(haplotypes, hap_gap):
    """--haplotypes / --hap-gap -> the gap the workflow takes (None: its default)"""
    if hap_gap is not None and not haplotypes:
        raise click.UsageError("--hap-gap needs --haplotypes")
    return hap_gap


def _type_bins(by_type, type_bins, ladder_by_type=False):
    """--by-type / --type-bins -> what the workflow takes: None without --by-type, True for the default edges, else the edges' text"""
    if type_bins is not None and not by_type and not ladder_by_type:
        raise click.UsageError("--type-bins needs --by-type")
    return None if not by_type else True if type_bins is None else type_bins


# The options of the passes over a finished batch, once for both commands, in the order --help lists them:
# (flag, click attributes, help, the commands that have it, how its value travels to the workflow's keyword of the same name).
# %(x)s in a help text is what SAYS holds for x under the command: a table or a file name.  AS_IS: the value as given; GENOMES: the
# genome(s) of the run where the flag is set, else None; None: one of the helpers above, or the command itself, makes the keyword.
AS_IS, GENOMES = "as is", "genomes"
SWITCH = dict(is_flag=True, default=False)
NUMBER = dict(type=int, default=None)
shown = lambda default: dict(type=int, default=default, show_default=True)
SAYS = {
    "hcmv": dict(truth_side="the missed-variant lists (callers/*/fn/*.fn.vcf, nucmer/*.missed_by_all.vcf) and",
                 strata="caller_performance_strata.tsv", ci="caller_performance_ci.tsv and caller_performance_ci_pairs.tsv",
                 votes="per mixed sample) and caller_private.tsv (what each caller alone calls).", consensus="{sample}.{ref}.k{K}",
                 why="callers/*/why/*.fp.why.tsv and *.fn.why.tsv", surface="callers/*/surface/*.surface.tsv",
                 context="caller_performance_context.tsv", genome="needs the genomes: --merlin-ref / --ad169-ref or the config"),
    "vareval": dict(truth_side="callers/fn/{label}.fn.vcf and, for up to 5 labels,",
                    strata="snpcall_benchmark_strata.txt", ci="snpcall_benchmark_ci.txt",
                    votes="over the labels) and caller_private.tsv; more than 32 labels: a note, no table.", consensus="custom.k{K}",
                    why="callers/why/{label}.fp.why.tsv and {label}.fn.why.tsv", surface="callers/surface/{label}.surface.tsv",
                    context="snpcall_benchmark_context.txt", genome="the genome is the first file of -r/--refs: the one the VCFs were called against"),
}
BOTH, HCMV = ("hcmv", "vareval"), ("hcmv",)
PASS_OPTIONS = (
    ("--mutation-context", SWITCH, "Also write final_tables/{mix}.{caller}.mutationcontext.tsv (96-motif spectra of kept, TP and FP SNVs).", HCMV, GENOMES),
    ("--truth-side", SWITCH, "Also write %(truth_side)s final_tables/caller_snp_venn.tsv.", BOTH, AS_IS),
    ("--snp-profile", SWITCH, "Also write final_tables/{mix}.{caller}.snp.profile.tsv and ...afsweep.tsv (TP / FP SNVs by allele frequency and position) "
                              "and callers/*/profile/*.points.tsv.  Not together with --truth-side.", HCMV, None),
    ("--profile-window", shown(1024), "--snp-profile: positions per position bin.", HCMV, None),
    ("--profile-pos-bins", shown(256), "--snp-profile: position bins.", HCMV, None),
    ("--profile-af-bins", shown(20), "--snp-profile: allele-frequency bins (times position bins: at most 8192).", HCMV, None),
    ("--strata", dict(type=click.Path(), multiple=True),
     "BED file (repeatable, one stratum per file, named by its stem): also write final_tables/%(strata)s "
     "(TP, FP and FN counts per region; the chrom column is ignored).", BOTH, None),
    ("--strata-by-name", dict(type=click.Path(), default=None), "One BED file, one stratum per distinct value of column 4: the same table.", BOTH, None),
    ("--bootstrap", NUMBER, "Replicates of the paired block bootstrap over genome windows: also write final_tables/%(ci)s "
                            "(percentile intervals of precision, recall and F1; the same draws for every VCF).", BOTH, None),
    ("--bootstrap-window", shown(1024), "--bootstrap: positions per window.", BOTH, None),
    ("--bootstrap-seed", shown(0), "--bootstrap: seed of the draws.", BOTH, None),
    ("--votes", SWITCH, "k-of-n caller consensus: also write final_tables/caller_consensus.tsv (TP, FP, FN, precision, recall, F1 of 'at least k of the n "
                        "callers agree', %(votes)s", BOTH, AS_IS),
    ("--consensus-vcf", NUMBER, "With the vote tables, also write snp/consensus/%(consensus)s.vcf: one line per key that at least K callers call.", BOTH, AS_IS),
    ("--explain-errors", SWITCH, "Why every FP line is FP and every missed truth key missed: also write %(why)s and final_tables/caller_error_classes.tsv.", BOTH, AS_IS),
    ("--explain-radius", NUMBER, "--explain-errors: positions on either side within which a truth key (a call) counts as near [default: 10; 0 to 64].", BOTH, AS_IS),
    ("--filter-surface", SWITCH, "TP, FP and FN under every filter QUAL >= q and AF >= a: also write %(surface)s and final_tables/caller_best_filter.tsv "
                                 "(the filter of the largest F1 per caller).", BOTH, AS_IS),
    ("--surface-qual-step", NUMBER, "--filter-surface: QUAL units per grid line; must divide 20 [default: 4].", BOTH, AS_IS),
    ("--surface-qual-bins", NUMBER, "--filter-surface: QUAL grid lines [default: 64; 1 to 256].", BOTH, AS_IS),
    ("--surface-af-bins", NUMBER, "--filter-surface: AF grid lines [default: 50; 1 to 64; at most 4096 cells].", BOTH, AS_IS),
    ("--seq-context", SWITCH, "TP, FP and FN per homopolymer x local-GC cell of the genome: also write final_tables/%(context)s (%(genome)s).", BOTH, GENOMES),
    ("--context-window", NUMBER, "--seq-context: positions on either side of a call in its GC window [default: 50; 0 to 1024].", BOTH, AS_IS),
    ("--context-gc-bins", NUMBER, "--seq-context: GC bins [default: 10; 1 to 15].", BOTH, AS_IS),
    ("--alleles", SWITCH, "Allele-extended mode: records and truth rows with REF and ALT of any length [ACGT]+ take part (indels, MNPs), matched by spelling.", HCMV, AS_IS),
    ("--normalize", SWITCH, "With --alleles: also match indels and MNPs by normal form (trimmed, left-aligned against the genome): write "
                            "final_tables/caller_performance_normalized.tsv and callers/*/norm/*.rescued.tsv (%(genome)s).", HCMV, GENOMES),
    ("--atomize", SWITCH, "With --alleles: also match MNPs against adjacent SNVs, atom by atom (every equal-length substitution split into its "
                          "single-base differences, on both sides): write final_tables/caller_performance_atomized.tsv and callers/*/atoms/*.atoms.tsv.", HCMV, AS_IS),
    ("--rescue-roc", SWITCH, "With --alleles, in place of --normalize and --atomize: sweep the QUAL threshold under the matching by normal form and by atoms "
                             "(precision and recall at every QUAL >= t, as by spelling): write snp/qmvt_roc/*/*.rescue/{spelling,normalized,atomized}_roc.tsv.gz and "
                             "final_tables/caller_roc_rescue.tsv (%(genome)s).", HCMV, GENOMES),
    ("--match-ladder", SWITCH, "With --alleles, in place of --normalize, --atomize, --haplotypes and --hap-subsets, which it always runs, all four: combine them -- "
                               "TP, FP and FN by spelling and after each method in turn (normal form, atoms, haplotype, subset), cumulative, and how many lines and "
                               "truth entries every set of methods reaches: write final_tables/caller_performance_ladder.tsv and callers/*/ladder/*.ladder.tsv "
                               "(%(genome)s; --hap-gap as for --haplotypes).", HCMV, GENOMES),
    ("--ladder-by-type", SWITCH, "With --alleles, in place of --match-ladder and --by-type, both of which it always runs behind all four rescues: TP, FP and FN per "
                                 "variant type and size -- typed as the record is spelled -- by spelling and after each method in turn: write "
                                 "final_tables/caller_performance_ladder_types.tsv (%(genome)s; --hap-gap as for "
                                 "--haplotypes, --type-bins as for --by-type).", HCMV, GENOMES),
    ("--by-type", SWITCH, "With --alleles: also count TP, FP and FN by variant type (SNV, MNP, INS, DEL, complex) and size: write "
                          "final_tables/caller_performance_types.tsv.", HCMV, None),
    ("--type-bins", dict(default=None), "--by-type: the ascending lower edges of the size bins, at most 16, the first one 1 [default: 1,2,3,4,5,6,16,51].", HCMV, None),
    ("--haplotypes", SWITCH, "With --alleles: also match clusters of lines by replayed haplotype (the unmatched lines and the unmatched truth entries of a small "
                             "region, each replayed onto the genome, are rescued where the two sequences are equal): write "
                             "final_tables/caller_performance_haplotype.tsv and callers/*/hap/*.sites.tsv (%(genome)s).", HCMV, GENOMES),
    ("--hap-subsets", SWITCH, "With --alleles (implies --haplotypes): also search the regions that did not match for the largest pair of subsets of their lines and "
                              "truth entries whose replayed sequences are equal (one true FP or one missed entry beside a respelled pair no longer costs the "
                              "whole region): write final_tables/caller_performance_hapsubsets.tsv and callers/*/hap/*.subsets.tsv beside the outputs of --haplotypes.", HCMV, AS_IS),
    ("--hap-gap", NUMBER, "--haplotypes: truth entries at most twice this many bases apart share a region, whose window reaches this far on either side [default: 10; 0 to 32].", HCMV, None),
)
# What vareval lacks: the passes of the allele-extended mode.  It takes their flags all the same, to say so: in the order it refuses
# them, (flag, its companion options and their click attributes, what the mode would do -- None: the help points at the flag it
# goes with --, the flags to use with hcmv instead); NOT_HERE_HELP is the order --help lists them in.
NOT_HERE = (
    ("--ladder-by-type", (), "whose types and rescue passes could be crossed", "--alleles --ladder-by-type"),
    ("--match-ladder", (), "whose rescue passes could be combined", "--alleles --match-ladder"),
    ("--rescue-roc", (), "whose rescue passes could be swept", "--alleles --rescue-roc"),
    ("--hap-subsets", (), None, "--alleles --haplotypes --hap-subsets"),
    ("--haplotypes", (("--hap-gap", NUMBER),), "whose lines could be replayed", "--alleles --haplotypes"),
    ("--by-type", (("--type-bins", dict(default=None)),), "whose variants could be typed", "--alleles --by-type"),
    ("--atomize", (), "whose MNPs could be split", "--alleles --atomize"),
    ("--normalize", (), "to normalise", "--alleles --normalize"),
)
NOT_HERE_HELP = ("--normalize", "--atomize", "--rescue-roc", "--match-ladder", "--ladder-by-type", "--by-type", "--haplotypes", "--hap-subsets")
_name = lambda flag: flag[2:].replace("-", "_")


def pass_options(command):
    """the rows of PASS_OPTIONS that `command` has, as one decorator"""
    def decorate(f):
        for flag, attrs, text, commands, _ in reversed(PASS_OPTIONS):
            if command in commands:
                f = click.option(flag, _name(flag), help=text % SAYS[command], **attrs)(f)
        return f
    return decorate


def not_here_options(f):
    """the flags of NOT_HERE and their companions, accepted so that the command can refuse them by name"""
    rows = {row[0]: row for row in NOT_HERE}
    for flag, companions, would, _ in reversed([rows[flag] for flag in NOT_HERE_HELP]):
        for other, attrs in reversed(companions):
            f = click.option(other, _name(other), help="Not available here (see %s)." % flag, **attrs)(f)
        text = "Not available here (see --haplotypes)." if would is None else (
            "Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode %s (hcmv has it)." % would)
        f = click.option(flag, _name(flag), help=text, **SWITCH)(f)
    return f


def _forwarded(command, opt, genomes):
    """the workflow keywords that PASS_OPTIONS says travel as they are or as the run's genome(s)"""
    return {_name(flag): opt[_name(flag)] if travel == AS_IS else genomes if opt[_name(flag)] else None
            for flag, _, _, commands, travel in PASS_OPTIONS if command in commands and travel is not None}


@cli.command(help="Benchmarking for HCMV dataset")
@common_options
@click.option("-e", "--evaluation", required=True, type=click.Choice(["all", "variantcall", "assembly"]), help="The evaluation to run.")
@click.option("-s", "--slow", is_flag=True, default=False, show_default=True, help="Run the evaluation based on reads (not supported by this build).")
@click.option("--data", type=click.Path(), default=None, help="Unpacked bundle directory (default: <repo>/data/snp).")
@pass_options("hcmv")
@click.option("--merlin-ref", type=click.Path(), default=None, help="Merlin FASTA for TM (default: MerlinRef of config/config.yaml).")
@click.option("--ad169-ref", type=click.Path(), default=None, help="AD169 FASTA for TA (default: AD169Ref of config/config.yaml).")
def hcmv(evaluation, dryrun, slow, outpath, data, gpus, json_out, merlin_ref, ad169_ref, **opt):
    opt["haplotypes"] = opt["haplotypes"] or opt["hap_subsets"]   # the search runs behind the haplotype pass of the same call
    if slow:
        click.echo("--slow (reads -> VCF) is outside the accelerated path; not supported", err=True)
        sys.exit(2)
    if evaluation == "assembly":
        click.echo("assembly evaluation is outside the accelerated path; not supported", err=True)
        sys.exit(2)
    from quasimodo_amd import workflow
    cfg_file = os.path.join(wd, "config", "config.yaml")
    cfg = workflow.load_yaml(cfg_file) if os.path.exists(cfg_file) else {}
    if outpath:
        out = os.path.join(cd, outpath)
    else:   # rules/load_config.smk:5,17: config/config.yaml, relative to the workflow's directory
        out = os.path.join(wd, str(cfg.get("outpath") or "../revision_output_1"))
    genomes = None
    if any(opt[_name(flag)] for flag, _, _, _, travel in PASS_OPTIONS if travel == GENOMES):   # rules/load_config.smk:8-10: MerlinRef / AD169Ref, absolute from the workflow's directory
        pick = lambda cli, key: os.path.join(cd, cli) if cli else (os.path.join(wd, str(cfg[key])) if cfg.get(key) else None)
        genomes = {"TM": pick(merlin_ref, "MerlinRef"), "TA": pick(ad169_ref, "AD169Ref")}
    try:
        # data/snp is unpacked from data/snp.tar.gz when it is not there yet (rules/load_config.smk:28-31)
        strata_set = _read_strata(opt["strata"], opt["strata_by_name"])
        workflow.run_hcmv_variantcall.last_result = None
        jobs = workflow.run_hcmv_variantcall(data or os.path.join(wd, "data", "snp"), out, dryrun=dryrun, gpus=gpus if gpus > 1 else None,
                                             snp_profile=dict(window=opt["profile_window"], n_pos_bins=opt["profile_pos_bins"], n_af_bins=opt["profile_af_bins"])
                                             if opt["snp_profile"] else None, strata=strata_set,
                                             bootstrap=_bootstrap_opts(opt["bootstrap"], opt["bootstrap_window"], opt["bootstrap_seed"]),
                                             by_type=_type_bins(opt["by_type"], opt["type_bins"], opt["ladder_by_type"]),
                                             hap_gap=_hap_gap(opt["haplotypes"] or opt["match_ladder"] or opt["ladder_by_type"], opt["hap_gap"]),
                                             ladder_type_bins=opt["type_bins"] if opt["ladder_by_type"] and not opt["by_type"] else None,
                                             **_forwarded("hcmv", opt, genomes))
        if json_out and not dryrun:
            _write_json(json_out, "hcmv", jobs, workflow.run_hcmv_variantcall)
    except Exception as e:
        _fail(e)
    if evaluation == "all":
        click.echo("assembly evaluation skipped: outside the accelerated path", err=True)


@cli.command(help="Variants benchmark for customized dataset")
@common_options
@click.option("-v", "--vcfs", type=str, help="Comma-separated list of VCF files.")
@click.option("-l", "--labels", help="Comma-separated list of labels of VCF.", default=None)
@click.option("-r", "--refs", type=str, help="Comma-separated list of reference genome files (used to name the genome difference).")
@click.option("--novenn", is_flag=True, help="Accepted for compatibility; no figure is drawn.")
@click.option("--snps", type=click.Path(), default=None,
              help="show-snps -CTHIlr table of the two references; default <outpath>/results/snp/nucmer/<g1>_<g2>.maskrepeat.snps")
@click.option("--config", type=click.Path(exists=True), default=None,
              help="YAML with vcfs / refs / outpath / labels for what the command line leaves out (default: config/customize_data.yaml).")
@pass_options("vareval")
@not_here_options
def vareval(dryrun, vcfs, labels, refs, outpath, snps, gpus, config, json_out, **opt):
    from quasimodo_amd import workflow
    try:
        for flag, companions, _, use in NOT_HERE:
            if opt[_name(flag)] or any(opt[_name(other)] is not None for other, _ in companions):
                raise workflow.WorkflowError("%s needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                             "custom run holds single-base rows (use hcmv -e variantcall %s)" % (flag, use))
        # what the command line leaves out comes from config/customize_data.yaml (run_benchmark.py:153-166,
        # rules/load_config_custom.smk:3, eval_variant_custom.smk:3-34)
        cfg_file = config or os.path.join(wd, "config", "customize_data.yaml")
        cfg = workflow.load_yaml(cfg_file) if os.path.exists(cfg_file) else {}
        st = workflow.vareval_settings(vcfs, refs, outpath, labels, cfg, cd=cd, wd=wd)
        out = st["outpath"]
        if snps is None:
            if not st["refs"] or len(st["refs"]) != 2:
                raise workflow.PathNotGiven("The reference genome files or output directory are not specified.")
            g = [os.path.splitext(os.path.basename(r))[0] for r in st["refs"]]
            snps = os.path.join(out, "results", "snp", "nucmer", "%s_%s.maskrepeat.snps" % (g[0], g[1]))   # eval_variant_custom.smk:14-17,40
        else:
            snps = os.path.join(cd, snps)
        if opt["seq_context"] and not st["refs"]:
            raise workflow.PathNotGiven("--seq-context: the reference genome files are not specified (the first one is the genome the VCFs were called against).")
        workflow.run_vareval.last_result = None
        jobs = workflow.run_vareval(st["vcfs"], snps, out, labels=st["labels"], dryrun=dryrun, gpus=gpus if gpus > 1 else None,
                                    strata=_read_strata(opt["strata"], opt["strata_by_name"]),
                                    bootstrap=_bootstrap_opts(opt["bootstrap"], opt["bootstrap_window"], opt["bootstrap_seed"]),
                                    **_forwarded("vareval", opt, st["refs"][0] if opt["seq_context"] else None))
        if json_out and not dryrun:
            _write_json(json_out, "vareval", jobs, workflow.run_vareval)
    except Exception as e:
        _fail(e)


@cli.command(help="Assembly benchmark for customized dataset (not on the accelerated path)")
@common_options
@click.option("-s", "--scaffolds", type=str)
@click.option("-r", "--refs", type=str)
def asmeval(**kwargs):
    click.echo("asmeval is outside the accelerated path; not supported", err=True)
    sys.exit(2)


if __name__ == "__main__":
    cli()
