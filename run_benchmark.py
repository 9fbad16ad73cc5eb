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


@cli.command(help="Benchmarking for HCMV dataset")
@common_options
@click.option("-e", "--evaluation", required=True, type=click.Choice(["all", "variantcall", "assembly"]), help="The evaluation to run.")
@click.option("-s", "--slow", is_flag=True, default=False, show_default=True, help="Run the evaluation based on reads (not supported by this build).")
@click.option("--data", type=click.Path(), default=None, help="Unpacked bundle directory (default: <repo>/data/snp).")
@click.option("--mutation-context", "mutation_context", is_flag=True, default=False,
              help="Also write final_tables/{mix}.{caller}.mutationcontext.tsv (96-motif spectra of kept, TP and FP SNVs).")
@click.option("--truth-side", "truth_side", is_flag=True, default=False,
              help="Also write the missed-variant lists (callers/*/fn/*.fn.vcf, nucmer/*.missed_by_all.vcf) and final_tables/caller_snp_venn.tsv.")
@click.option("--snp-profile", "snp_profile", is_flag=True, default=False,
              help="Also write final_tables/{mix}.{caller}.snp.profile.tsv and ...afsweep.tsv (TP / FP SNVs by allele frequency and position) "
                   "and callers/*/profile/*.points.tsv.  Not together with --truth-side.")
@click.option("--profile-window", type=int, default=1024, show_default=True, help="--snp-profile: positions per position bin.")
@click.option("--profile-pos-bins", type=int, default=256, show_default=True, help="--snp-profile: position bins.")
@click.option("--profile-af-bins", type=int, default=20, show_default=True, help="--snp-profile: allele-frequency bins (times position bins: at most 8192).")
@click.option("--strata", "strata", type=click.Path(), multiple=True,
              help="BED file (repeatable, one stratum per file, named by its stem): also write final_tables/caller_performance_strata.tsv "
                   "(TP, FP and FN counts per region; the chrom column is ignored).")
@click.option("--strata-by-name", "strata_by_name", type=click.Path(), default=None,
              help="One BED file, one stratum per distinct value of column 4: the same table.")
@click.option("--bootstrap", "bootstrap", type=int, default=None,
              help="Replicates of the paired block bootstrap over genome windows: also write final_tables/caller_performance_ci.tsv and caller_performance_ci_pairs.tsv "
                   "(percentile intervals of precision, recall and F1; the same draws for every VCF).")
@click.option("--bootstrap-window", "bootstrap_window", type=int, default=1024, show_default=True, help="--bootstrap: positions per window.")
@click.option("--bootstrap-seed", "bootstrap_seed", type=int, default=0, show_default=True, help="--bootstrap: seed of the draws.")
@click.option("--votes", "votes", is_flag=True, default=False,
              help="k-of-n caller consensus: also write final_tables/caller_consensus.tsv (TP, FP, FN, precision, recall, F1 of 'at least k of the n "
                   "callers agree', per mixed sample) and caller_private.tsv (what each caller alone calls).")
@click.option("--consensus-vcf", "consensus_vcf", type=int, default=None,
              help="With the vote tables, also write snp/consensus/{sample}.{ref}.k{K}.vcf: one line per key that at least K callers call.")
@click.option("--explain-errors", "explain_errors", is_flag=True, default=False,
              help="Why every FP line is FP and every missed truth key missed: also write callers/*/why/*.fp.why.tsv and *.fn.why.tsv and final_tables/caller_error_classes.tsv.")
@click.option("--explain-radius", "explain_radius", type=int, default=None,
              help="--explain-errors: positions on either side within which a truth key (a call) counts as near [default: 10; 0 to 64].")
@click.option("--filter-surface", "filter_surface", is_flag=True, default=False,
              help="TP, FP and FN under every filter QUAL >= q and AF >= a: also write callers/*/surface/*.surface.tsv and final_tables/caller_best_filter.tsv (the filter of the largest F1 per caller).")
@click.option("--surface-qual-step", "surface_qual_step", type=int, default=None, help="--filter-surface: QUAL units per grid line; must divide 20 [default: 4].")
@click.option("--surface-qual-bins", "surface_qual_bins", type=int, default=None, help="--filter-surface: QUAL grid lines [default: 64; 1 to 256].")
@click.option("--surface-af-bins", "surface_af_bins", type=int, default=None, help="--filter-surface: AF grid lines [default: 50; 1 to 64; at most 4096 cells].")
@click.option("--seq-context", "seq_context", is_flag=True, default=False,
              help="TP, FP and FN per homopolymer x local-GC cell of the genome: also write final_tables/caller_performance_context.tsv "
                   "(needs the genomes: --merlin-ref / --ad169-ref or the config).")
@click.option("--context-window", "context_window", type=int, default=None, help="--seq-context: positions on either side of a call in its GC window [default: 50; 0 to 1024].")
@click.option("--context-gc-bins", "context_gc_bins", type=int, default=None, help="--seq-context: GC bins [default: 10; 1 to 15].")
@click.option("--alleles", "alleles", is_flag=True, default=False,
              help="Allele-extended mode: records and truth rows with REF and ALT of any length [ACGT]+ take part (indels, MNPs), matched by spelling.")
@click.option("--normalize", "normalize", is_flag=True, default=False,
              help="With --alleles: also match indels and MNPs by normal form (trimmed, left-aligned against the genome): write "
                   "final_tables/caller_performance_normalized.tsv and callers/*/norm/*.rescued.tsv (needs the genomes: --merlin-ref / --ad169-ref or the config).")
@click.option("--atomize", "atomize", is_flag=True, default=False,
              help="With --alleles: also match MNPs against adjacent SNVs, atom by atom (every equal-length substitution split into its "
                   "single-base differences, on both sides): write final_tables/caller_performance_atomized.tsv and callers/*/atoms/*.atoms.tsv.")
@click.option("--rescue-roc", "rescue_roc", is_flag=True, default=False,
              help="With --alleles, in place of --normalize and --atomize: sweep the QUAL threshold under the matching by normal form and by atoms "
                   "(precision and recall at every QUAL >= t, as by spelling): write snp/qmvt_roc/*/*.rescue/{spelling,normalized,atomized}_roc.tsv.gz and "
                   "final_tables/caller_roc_rescue.tsv (needs the genomes: --merlin-ref / --ad169-ref or the config).")
@click.option("--match-ladder", "match_ladder", is_flag=True, default=False,
              help="With --alleles, in place of --normalize, --atomize, --haplotypes and --hap-subsets, which it always runs, all four: combine them -- "
                   "TP, FP and FN by spelling and after each method in turn (normal form, atoms, haplotype, subset), cumulative, and how many lines and "
                   "truth entries every set of methods reaches: write final_tables/caller_performance_ladder.tsv and callers/*/ladder/*.ladder.tsv "
                   "(needs the genomes: --merlin-ref / --ad169-ref or the config; --hap-gap as for --haplotypes).")
@click.option("--ladder-by-type", "ladder_by_type", is_flag=True, default=False,
              help="With --alleles, in place of --match-ladder and --by-type, both of which it always runs behind all four rescues: TP, FP and FN per "
                   "variant type and size -- typed as the record is spelled -- by spelling and after each method in turn: write "
                   "final_tables/caller_performance_ladder_types.tsv (needs the genomes: --merlin-ref / --ad169-ref or the config; --hap-gap as for "
                   "--haplotypes, --type-bins as for --by-type).")
@click.option("--by-type", "by_type", is_flag=True, default=False,
              help="With --alleles: also count TP, FP and FN by variant type (SNV, MNP, INS, DEL, complex) and size: write "
                   "final_tables/caller_performance_types.tsv.")
@click.option("--type-bins", "type_bins", default=None,
              help="--by-type: the ascending lower edges of the size bins, at most 16, the first one 1 [default: 1,2,3,4,5,6,16,51].")
@click.option("--haplotypes", "haplotypes", is_flag=True, default=False,
              help="With --alleles: also match clusters of lines by replayed haplotype (the unmatched lines and the unmatched truth entries of a small "
                   "region, each replayed onto the genome, are rescued where the two sequences are equal): write "
                   "final_tables/caller_performance_haplotype.tsv and callers/*/hap/*.sites.tsv (needs the genomes: --merlin-ref / --ad169-ref or the config).")
@click.option("--hap-subsets", "hap_subsets", is_flag=True, default=False,
              help="With --alleles (implies --haplotypes): also search the regions that did not match for the largest pair of subsets of their lines and "
                   "truth entries whose replayed sequences are equal (one true FP or one missed entry beside a respelled pair no longer costs the "
                   "whole region): write final_tables/caller_performance_hapsubsets.tsv and callers/*/hap/*.subsets.tsv beside the outputs of --haplotypes.")
@click.option("--hap-gap", "hap_gap", type=int, default=None,
              help="--haplotypes: truth entries at most twice this many bases apart share a region, whose window reaches this far on either side [default: 10; 0 to 32].")
@click.option("--merlin-ref", type=click.Path(), default=None, help="Merlin FASTA for TM (default: MerlinRef of config/config.yaml).")
@click.option("--ad169-ref", type=click.Path(), default=None, help="AD169 FASTA for TA (default: AD169Ref of config/config.yaml).")
def hcmv(evaluation, dryrun=False, conda_prefix=None, slow=False, outpath=None, threads=2, data=None, gpus=1, json_out=None,
         mutation_context=False, merlin_ref=None, ad169_ref=None, truth_side=False, snp_profile=False, profile_window=1024,
         profile_pos_bins=256, profile_af_bins=20, strata=(), strata_by_name=None, bootstrap=None, bootstrap_window=1024, bootstrap_seed=0,
         votes=False, consensus_vcf=None, explain_errors=False, explain_radius=None, filter_surface=False, surface_qual_step=None,
         surface_qual_bins=None, surface_af_bins=None, seq_context=False, context_window=None, context_gc_bins=None, alleles=False,
         normalize=False, atomize=False, by_type=False, type_bins=None, haplotypes=False, hap_gap=None, hap_subsets=False, rescue_roc=False, match_ladder=False,
         ladder_by_type=False):
    haplotypes = haplotypes or hap_subsets   # the search runs behind the haplotype pass of the same call
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
    if mutation_context or seq_context or normalize or haplotypes or rescue_roc or match_ladder or ladder_by_type:   # rules/load_config.smk:8-10: MerlinRef / AD169Ref, absolute from the workflow's directory
        pick = lambda cli, key: os.path.join(cd, cli) if cli else (os.path.join(wd, str(cfg[key])) if cfg.get(key) else None)
        genomes = {"TM": pick(merlin_ref, "MerlinRef"), "TA": pick(ad169_ref, "AD169Ref")}
    try:
        # data/snp is unpacked from data/snp.tar.gz when it is not there yet (rules/load_config.smk:28-31)
        strata_set = _read_strata(strata, strata_by_name)
        workflow.run_hcmv_variantcall.last_result = None
        jobs = workflow.run_hcmv_variantcall(data or os.path.join(wd, "data", "snp"), out, dryrun=dryrun, gpus=gpus if gpus > 1 else None,
                                             mutation_context=genomes if mutation_context else None, truth_side=truth_side,
                                             seq_context=genomes if seq_context else None, context_window=context_window, context_gc_bins=context_gc_bins,
                                             snp_profile=dict(window=profile_window, n_pos_bins=profile_pos_bins, n_af_bins=profile_af_bins)
                                             if snp_profile else None, strata=strata_set,
                                             bootstrap=_bootstrap_opts(bootstrap, bootstrap_window, bootstrap_seed),
                                             votes=votes, consensus_vcf=consensus_vcf, explain_errors=explain_errors, explain_radius=explain_radius,
                                             filter_surface=filter_surface, surface_qual_step=surface_qual_step,
                                             surface_qual_bins=surface_qual_bins, surface_af_bins=surface_af_bins,
                                             alleles=alleles, normalize=genomes if normalize else None, atomize=atomize,
                                             by_type=_type_bins(by_type, type_bins, ladder_by_type), haplotypes=genomes if haplotypes else None,
                                             hap_gap=_hap_gap(haplotypes or match_ladder or ladder_by_type, hap_gap), hap_subsets=hap_subsets,
                                             rescue_roc=genomes if rescue_roc else None, match_ladder=genomes if match_ladder else None,
                                             ladder_by_type=genomes if ladder_by_type else None,
                                             ladder_type_bins=type_bins if ladder_by_type and not by_type else None)
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
@click.option("--truth-side", "truth_side", is_flag=True, default=False,
              help="Also write callers/fn/{label}.fn.vcf and, for up to 5 labels, final_tables/caller_snp_venn.tsv.")
@click.option("--strata", "strata", type=click.Path(), multiple=True,
              help="BED file (repeatable, one stratum per file, named by its stem): also write final_tables/snpcall_benchmark_strata.txt "
                   "(TP, FP and FN counts per region; the chrom column is ignored).")
@click.option("--strata-by-name", "strata_by_name", type=click.Path(), default=None,
              help="One BED file, one stratum per distinct value of column 4: the same table.")
@click.option("--bootstrap", "bootstrap", type=int, default=None,
              help="Replicates of the paired block bootstrap over genome windows: also write final_tables/snpcall_benchmark_ci.txt "
                   "(percentile intervals of precision, recall and F1; the same draws for every VCF).")
@click.option("--bootstrap-window", "bootstrap_window", type=int, default=1024, show_default=True, help="--bootstrap: positions per window.")
@click.option("--bootstrap-seed", "bootstrap_seed", type=int, default=0, show_default=True, help="--bootstrap: seed of the draws.")
@click.option("--votes", "votes", is_flag=True, default=False,
              help="k-of-n caller consensus: also write final_tables/caller_consensus.tsv (TP, FP, FN, precision, recall, F1 of 'at least k of the n "
                   "callers agree', over the labels) and caller_private.tsv; more than 32 labels: a note, no table.")
@click.option("--consensus-vcf", "consensus_vcf", type=int, default=None,
              help="With the vote tables, also write snp/consensus/custom.k{K}.vcf: one line per key that at least K callers call.")
@click.option("--explain-errors", "explain_errors", is_flag=True, default=False,
              help="Why every FP line is FP and every missed truth key missed: also write callers/why/{label}.fp.why.tsv and {label}.fn.why.tsv and final_tables/caller_error_classes.tsv.")
@click.option("--explain-radius", "explain_radius", type=int, default=None,
              help="--explain-errors: positions on either side within which a truth key (a call) counts as near [default: 10; 0 to 64].")
@click.option("--filter-surface", "filter_surface", is_flag=True, default=False,
              help="TP, FP and FN under every filter QUAL >= q and AF >= a: also write callers/surface/{label}.surface.tsv and final_tables/caller_best_filter.tsv (the filter of the largest F1 per caller).")
@click.option("--surface-qual-step", "surface_qual_step", type=int, default=None, help="--filter-surface: QUAL units per grid line; must divide 20 [default: 4].")
@click.option("--surface-qual-bins", "surface_qual_bins", type=int, default=None, help="--filter-surface: QUAL grid lines [default: 64; 1 to 256].")
@click.option("--surface-af-bins", "surface_af_bins", type=int, default=None, help="--filter-surface: AF grid lines [default: 50; 1 to 64; at most 4096 cells].")
@click.option("--seq-context", "seq_context", is_flag=True, default=False,
              help="TP, FP and FN per homopolymer x local-GC cell of the genome: also write final_tables/snpcall_benchmark_context.txt "
                   "(the genome is the first file of -r/--refs: the one the VCFs were called against).")
@click.option("--context-window", "context_window", type=int, default=None, help="--seq-context: positions on either side of a call in its GC window [default: 50; 0 to 1024].")
@click.option("--context-gc-bins", "context_gc_bins", type=int, default=None, help="--seq-context: GC bins [default: 10; 1 to 15].")
@click.option("--normalize", "normalize", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode to normalise (hcmv has it).")
@click.option("--atomize", "atomize", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode whose MNPs could be split (hcmv has it).")
@click.option("--rescue-roc", "rescue_roc", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode whose rescue passes could be swept (hcmv has it).")
@click.option("--match-ladder", "match_ladder", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode whose rescue passes could be combined (hcmv has it).")
@click.option("--ladder-by-type", "ladder_by_type", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode whose types and rescue passes could be crossed (hcmv has it).")
@click.option("--by-type", "by_type", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode whose variants could be typed (hcmv has it).")
@click.option("--type-bins", "type_bins", default=None, help="Not available here (see --by-type).")
@click.option("--haplotypes", "haplotypes", is_flag=True, default=False,
              help="Not available here: the show-snps table of a custom run holds single-base rows only, so there is no allele-extended mode whose lines could be replayed (hcmv has it).")
@click.option("--hap-gap", "hap_gap", type=int, default=None, help="Not available here (see --haplotypes).")
@click.option("--hap-subsets", "hap_subsets", is_flag=True, default=False, help="Not available here (see --haplotypes).")
def vareval(dryrun=False, conda_prefix=None, vcfs=None, labels=None, refs=None, novenn=False, outpath=None, threads=2, snps=None, gpus=1,
            config=None, json_out=None, truth_side=False, strata=(), strata_by_name=None, bootstrap=None, bootstrap_window=1024, bootstrap_seed=0,
            votes=False, consensus_vcf=None, explain_errors=False, explain_radius=None, filter_surface=False, surface_qual_step=None,
            surface_qual_bins=None, surface_af_bins=None, seq_context=False, context_window=None, context_gc_bins=None, normalize=False, atomize=False,
            by_type=False, type_bins=None, haplotypes=False, hap_gap=None, hap_subsets=False, rescue_roc=False, match_ladder=False, ladder_by_type=False):
    from quasimodo_amd import workflow
    try:
        if ladder_by_type:
            raise workflow.WorkflowError("--ladder-by-type needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --ladder-by-type)")
        if match_ladder:
            raise workflow.WorkflowError("--match-ladder needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --match-ladder)")
        if rescue_roc:
            raise workflow.WorkflowError("--rescue-roc needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --rescue-roc)")
        if hap_subsets:
            raise workflow.WorkflowError("--hap-subsets needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --haplotypes --hap-subsets)")
        if haplotypes or hap_gap is not None:
            raise workflow.WorkflowError("--haplotypes needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --haplotypes)")
        if by_type or type_bins is not None:
            raise workflow.WorkflowError("--by-type needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --by-type)")
        if atomize:
            raise workflow.WorkflowError("--atomize needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --atomize)")
        if normalize:
            raise workflow.WorkflowError("--normalize needs the allele-extended mode, which reads VCF truth sets only: the show-snps table of a "
                                         "custom run holds single-base rows (use hcmv -e variantcall --alleles --normalize)")
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
        if seq_context and not st["refs"]:
            raise workflow.PathNotGiven("--seq-context: the reference genome files are not specified (the first one is the genome the VCFs were called against).")
        workflow.run_vareval.last_result = None
        jobs = workflow.run_vareval(st["vcfs"], snps, out, labels=st["labels"], dryrun=dryrun, gpus=gpus if gpus > 1 else None,
                                    truth_side=truth_side, strata=_read_strata(strata, strata_by_name),
                                    bootstrap=_bootstrap_opts(bootstrap, bootstrap_window, bootstrap_seed),
                                    votes=votes, consensus_vcf=consensus_vcf, explain_errors=explain_errors, explain_radius=explain_radius,
                                    filter_surface=filter_surface, surface_qual_step=surface_qual_step,
                                    surface_qual_bins=surface_qual_bins, surface_af_bins=surface_af_bins,
                                    seq_context=st["refs"][0] if seq_context else None, context_window=context_window, context_gc_bins=context_gc_bins)
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
