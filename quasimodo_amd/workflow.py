"""The path's slice of the two Snakemake workflows, without Snakemake.

  hcmv -e variantcall (bundled-VCF mode): eval_variantcall.smk cp_vcf / cp_genome_diff (:62-93) ->
      rules/extract_TP.smk -> rules/vis_eval_vcf.smk snp_evaluate (table only) -> rules/compare_FP.smk
  vareval: eval_variant_custom.smk extract_TP (:58-74) -> snp_benchmark (table only, :76-92)

Everything upstream (reads -> VCF, nucmer) and every figure is out of scope:
the inputs must already exist.  Every mixed-sample VCF of a run goes through ONE engine batch."""
import glob
import os
import shutil

from .engine import Engine
from .extract import Job, extract_many, is_pure_strain
from .tables import r_hostile_rows, write_caller_performance, write_fp_overlap, write_snpcall_benchmark, write_weighted_roc
from .vcfio import scan_vcf

SAMPLE_REF = {  # rules/load_config.smk:20-23
    "TM-0-1": "Merlin", "TM-1-1": "Merlin", "TM-1-10": "Merlin", "TM-1-50": "Merlin", "TM-1-0": "TB40E",
    "TA-1-0": "TB40E", "TA-1-1": "AD169", "TA-1-10": "AD169", "TA-1-50": "AD169", "TA-0-1": "AD169"}
SNPCALLERS = ["lofreq", "varscan", "clc", "bcftools", "freebayes", "gatk"]   # eval_variantcall.smk:10
FP_COMPARED = ["lofreq", "clc", "varscan", "freebayes"]                       # rules/compare_FP.smk:1


class WorkflowError(RuntimeError):
    pass


def ensure_bundle(data_dir):
    """rules/load_config.smk:28-31: when data/snp is absent, the bundle data/snp.tar.gz is unpacked beside it (the reference
    shells `tar -xzvf data/snp.tar.gz -C data/`).  Returns data_dir; raises when neither exists."""
    data_dir = data_dir.rstrip("/")
    if os.path.isdir(data_dir):
        return data_dir
    tarball = data_dir + ".tar.gz"
    if not os.path.exists(tarball):
        raise WorkflowError("neither %s nor %s exists" % (data_dir, tarball))
    import tarfile
    parent = os.path.dirname(data_dir) or "."
    with tarfile.open(tarball, "r:gz") as tf:
        try:
            tf.extractall(parent, filter="data")   # (members that would leave `parent` are refused)
        except TypeError:                           # a Python without extraction filters: the same refusals by hand
            root = os.path.realpath(parent)
            inside = lambda p: p == root or p.startswith(root + os.sep)     # ('.' and './' members of `tar -C dir .` resolve to the root itself)
            for m in tf.getmembers():
                dest = os.path.realpath(os.path.join(parent, m.name))
                if not inside(dest):
                    raise WorkflowError("%s: member %s would be written outside %s" % (tarball, m.name, parent))
                if m.issym() or m.islnk():          # a link is fine as long as what it points at stays inside
                    target = m.linkname if m.islnk() else os.path.join(os.path.dirname(m.name), m.linkname)
                    if os.path.isabs(m.linkname) or not inside(os.path.realpath(os.path.join(parent, target))):
                        raise WorkflowError("%s: link %s points outside %s" % (tarball, m.name, parent))
                elif not (m.isfile() or m.isdir()):
                    raise WorkflowError("%s: member %s is neither a file, a directory nor a link" % (tarball, m.name))
            tf.extractall(parent)
    if not os.path.isdir(data_dir):
        raise WorkflowError("%s does not hold a directory %s" % (tarball, os.path.basename(data_dir)))
    return data_dir


def load_yaml(path):
    import yaml
    with open(path) as fh:
        return yaml.safe_load(fh) or {}


class PathNotGiven(WorkflowError):
    """eval_variant_custom.smk:6-17 / :24-28 (same messages)."""


def vareval_settings(vcfs=None, refs=None, outpath=None, labels=None, config=None, cd=None, wd=None):
    """What `run_benchmark.py vareval` runs on: the command line where it says something, config/customize_data.yaml where it
    does not (run_benchmark.py:153-166: only vcfs / refs / outpath travel from the command line, made absolute against the
    caller's directory; rules/load_config_custom.smk:3 + eval_variant_custom.smk:3-17,24-34 take the rest, and whatever the
    command line left out, from the config file, relative to the workflow's directory).
    One deliberate difference: the reference DROPS `-l/--labels` given on the command line (run_benchmark.py:157-165,
    `else: continue`) and always uses the config file's; here a command-line value wins.
    vcfs / refs / labels: comma-separated strings or None; config: the YAML as a dict.
    Returns {"vcfs": [...], "refs": [...] or None, "outpath": str, "labels": [...] or None}."""
    config = config or {}
    cd = cd or os.getcwd()
    wd = wd or cd

    def items(val, base):
        return [os.path.join(base, x.strip()) for x in val.split(",")]

    def pick(name, cli):
        if cli is not None:
            return cli, cd
        v = config.get(name)
        return (v, wd) if isinstance(v, str) else (None, wd)

    r, rbase = pick("refs", refs)
    o, obase = pick("outpath", outpath)
    if o is None:
        raise PathNotGiven("The reference genome files or output directory are not specified.")
    v, vbase = pick("vcfs", vcfs)
    if v is None:
        raise PathNotGiven("The VCF files from SNP calling are not specified.")
    lab = labels if labels is not None else config.get("labels")
    return {"vcfs": items(v, vbase), "refs": items(r, rbase) if r is not None else None, "outpath": os.path.join(obase, o.rstrip("/")),
            "labels": [x for x in lab.split(",")] if isinstance(lab, str) and lab else None}


def _fp_keys(path):
    """snpcaller_fp_compare.R:36-47: pos/ref/alt of the data rows with single-base alleles."""
    with open(path, "rb") as fh:
        sv = scan_vcf(fh.read())
    keep = (sv.ref < 4) & (sv.alt < 4) & ((sv.flags & 4) == 0)
    return sv.pos[keep], sv.ref[keep], sv.alt[keep]


def _flag_truth_rows(jobs):
    """stats["truth_r_hostile"]: rows of the job's truth file that R's read.table would not read as tab-split text
    (tables.check_r_readable); pure-strain samples never read theirs."""
    seen = {}
    for j in jobs:
        if j.stats is None or j.stats.get("pure_strain"):
            continue
        if j.snp_file not in seen:
            seen[j.snp_file] = r_hostile_rows(j.snp_file)
        j.stats["truth_r_hostile"] = seen[j.snp_file]


def fp_overlap_tables(engine, fp_files_by_sample, callers):
    out = {}
    for sample, files in fp_files_by_sample.items():
        sets = [_fp_keys(files[c]) for c in callers]
        out[sample] = engine.fp_overlap(sets)
    return out


def hcmv_rank_post(engine, jobs, indices, args):
    """What a rank of the multi-GPU workflow does with its own VCFs once they are extracted, while its engine is alive:
    the FP overlap of its samples (rules/compare_FP.smk:5-8 compares the callers of ONE sample, and the workflow dealt the
    VCFs by sample: no exchange) and the xindel sweeps of its VCFs.  Returns {"overlap": {sample: [region sizes]}}."""
    meta = [args["meta"][i] for i in indices]
    cmp_callers = args["cmp_callers"]
    out = {}
    if len(cmp_callers) >= 2:
        by_sample = {}
        for (c, s), j in zip(meta, jobs):
            if c in cmp_callers and not s.endswith(("-1-0", "-0-1")):
                by_sample.setdefault(s, {})[c] = j.fp_out
        for s, files in by_sample.items():
            if len(files) != len(cmp_callers):
                raise WorkflowError("sample %s: the compared callers are not all on one rank" % s)
            out[s] = [int(x) for x in fp_overlap_tables(engine, {s: files}, cmp_callers)[s]]
    if args.get("indel_roc", True):
        indel_roc(engine, [(c, s, j) for (c, s), j in zip(meta, jobs) if not j.stats.get("pure_strain")], args["snp_dir"])
    return {"overlap": out}


def _shared_call(**asked):
    """the passes the flags ask for may share the run's one call (passes.check_shared_call), said with the CLI's names"""
    from .passes import SharedCallError, check_shared_call
    try:
        check_shared_call({name for name, on in asked.items() if on})
    except SharedCallError as e:
        raise WorkflowError(e.for_cli()) from None


def run_hcmv_variantcall(data_dir, outpath, callers=None, engine=None, dryrun=False, gpus=None, _body=None, _backend="nccl",
                         _same_device=False, mutation_context=None, truth_side=False, snp_profile=None, strata=None, bootstrap=None,
                         votes=False, consensus_vcf=None, explain_errors=False, explain_radius=None, filter_surface=False,
                         surface_qual_step=None, surface_qual_bins=None, surface_af_bins=None, seq_context=None, context_window=None,
                         context_gc_bins=None, alleles=False, normalize=None, atomize=False, by_type=None, haplotypes=None,
                         hap_gap=None, hap_subsets=False, rescue_roc=None, match_ladder=None, ladder_by_type=None, ladder_type_bins=None):
    """data_dir: the unpacked bundle (data/snp): vcf/{caller}/{sample}.{ref}.{caller}.vcf and
    nucmer/{TM,TA}.maskrepeat.variants.vcf (rules/load_config.smk:28-36); when it is absent and <data_dir>.tar.gz exists,
    that is unpacked first (:28-31).
    gpus > 1: one process per GPU (quasimodo_amd.multigpu); the VCFs are dealt by SAMPLE (longest first), so the four
    compared callers of a sample meet on one rank and the FP overlap needs no exchange; every rank writes its own files,
    the confusion counters go through the one all-reduce, the rows come to this process for the three tables.
    mutation_context: {"TM": FASTA, "TA": FASTA} (rules/mutationcontext.smk): the motif pass runs behind the classification and
    final_tables/{mix}.{caller}.mutationcontext.tsv is written for every caller and every mix that has samples.
    truth_side: the truth set's side of the join: callers/{caller}/fn/{sample}.{ref}.{caller}.fn.vcf for every
    mixed sample, nucmer/{sample}.missed_by_all.vcf over the Venn callers (rules/vis_eval_vcf.smk:2, those of the run) and
    final_tables/caller_snp_venn.tsv.
    snp_profile: True or {"window", "n_pos_bins", "n_af_bins"} (the rule's first output): the profile pass runs
    behind the classification; final_tables/{mix}.{caller}.snp.profile.tsv and ...snp.profile.afsweep.tsv are written for every
    caller and mix (`-1-0` left out, `-0-1` as FP only) and callers/{caller}/profile/{sample}.{ref}.{caller}.points.tsv for
    every profiled sample.
    strata: a list of (name, starts, ends) BED strata (quasimodo_amd.strata): the counts per stratum are taken
    behind the classification and final_tables/caller_performance_strata.tsv is written (per caller x sample one row per
    stratum, then outside, then nokey).
    bootstrap: a replicate count or {"n_rep", "window", "n_win", "seed"} (quasimodo_amd.bootstrap): the window
    counts and the replicates are taken behind the classification; final_tables/caller_performance_ci.tsv (percentile
    intervals of Precision, Recall and F1 per caller x sample) and caller_performance_ci_pairs.tsv (the F1 difference of every
    pair of callers on a mixed sample, over the shared draws) are written.  n_win is raised to cover the truth files' largest POS.
    votes: k-of-n caller consensus (quasimodo_amd.consensus): all callers of the run form one vote group per mixed
    sample; final_tables/caller_consensus.tsv (TP, FP, FN, Precision, Recall, F1 of "at least k of n callers") and
    caller_private.tsv (what each caller alone calls) are written.  consensus_vcf=K (implies votes) also writes
    snp/consensus/{sample}.{ref}.k{K}.vcf; K above the sample's caller count is a WorkflowError that names the sample.
    explain_errors: why the FP lines are FP and the missed truth keys missed (quasimodo_amd.nearmiss), with
    explain_radius (default 10, 0 to 64): callers/{caller}/why/{sample}.{ref}.{caller}.fp.why.tsv and ...fn.why.tsv for every mixed
    sample, and final_tables/caller_error_classes.tsv.
    filter_surface: TP, FP and FN under every filter QUAL >= q and AF >= a (quasimodo_amd.surface), with
    surface_qual_step / surface_qual_bins / surface_af_bins (default 4, 64, 50; QUAL 20 must be a grid line):
    callers/{caller}/surface/{sample}.{ref}.{caller}.surface.tsv for every mixed sample and final_tables/caller_best_filter.tsv.
    seq_context: {"TM": FASTA, "TA": FASTA}, the genomes as for mutation_context, with context_window / context_gc_bins (default
    50, 10; quasimodo_amd.context): the counts per homopolymer x GC cell are taken behind the classification and
    final_tables/caller_performance_context.tsv is written (per caller x sample the cells in use, the marginals, none, nokey).
    alleles: the allele-extended mode (include/qmvt.h): indels and MNPs take part, matched by spelling.
    normalize: {"TM": FASTA, "TA": FASTA}, the genomes as for seq_context (quasimodo_amd.normalize; needs alleles,
    WorkflowError before a file is touched otherwise): indels and MNPs are also matched by normal form behind the classification;
    final_tables/caller_performance_normalized.tsv (TP, FP, FN, Precision, Recall, F1 by spelling and by normal form side by side,
    the rescued, respelled and reason counts) and callers/{caller}/norm/{sample}.{ref}.{caller}.rescued.tsv for every mixed sample.
    atomize: MNPs are also matched against adjacent SNVs, atom by atom (quasimodo_amd.atomize; needs alleles,
    WorkflowError before a file is touched otherwise): final_tables/caller_performance_atomized.tsv (TP, FP, FN, Precision, Recall,
    F1 by spelling and by atoms side by side, the rescued, multi-atom, partial and reason counts) and
    callers/{caller}/atoms/{sample}.{ref}.{caller}.atoms.tsv for every mixed sample.
    by_type: True, or the size edges as a list or as the CLI's `1,2,6` (quasimodo_amd.vartype; needs alleles,
    WorkflowError before a file is touched otherwise): TP, FP and FN by variant type and size are counted behind the
    classification and final_tables/caller_performance_types.tsv is written (per caller x mixed sample one row per type and size
    bin, a marginal per type, the four rows behind the grid, then a pooled block per caller).
    haplotypes: {"TM": FASTA, "TA": FASTA}, the genomes as for normalize, with hap_gap (default 10, 0 to 32; quasimodo_amd.haplo,
    DESIGN.md 4.20; needs alleles, WorkflowError before a file is touched otherwise): the unmatched lines and the unmatched truth
    entries of every small region are replayed onto the genome and rescued where the two sequences are equal;
    final_tables/caller_performance_haplotype.tsv (TP, FP, FN, Precision, Recall, F1 by spelling and by haplotype side by side, then
    the class counts) and callers/{caller}/hap/{sample}.{ref}.{caller}.sites.tsv for every mixed sample.
    rescue_roc: {"TM": FASTA, "TA": FASTA}, the genomes as for normalize (quasimodo_amd.rescueroc; needs alleles,
    WorkflowError before a file is touched otherwise), in place of normalize and atomize, which the run's call makes itself: the
    QUAL ROC by spelling, by normal form and by atoms side by side, snp/qmvt_roc/{caller}/{sample}.{ref}.rescue/spelling_roc.tsv.gz,
    normalized_roc.tsv.gz and atomized_roc.tsv.gz for every mixed sample, and final_tables/caller_roc_rescue.tsv (TP, FP, FN,
    Precision, Recall, F1 at QUAL >= 20 and at the threshold of the largest F1, per caller, mixture and matching, then pooled).
    match_ladder: {"TM": FASTA, "TA": FASTA}, the genomes as for normalize, with hap_gap (quasimodo_amd.ladder; needs
    alleles, WorkflowError before a file is touched otherwise), in place of normalize, atomize, haplotypes and hap_subsets, which
    the run's call makes itself, all four: final_tables/caller_performance_ladder.tsv (TP, FP, FN, Precision, Recall, F1 by spelling
    and after normal form, atoms, haplotype and subset, cumulative, then the 15 non-empty method sets of lines and of entries; per
    caller and mixture, then pooled per caller) and callers/{caller}/ladder/{sample}.{ref}.{caller}.ladder.tsv for every mixed
    sample (every kept line that is no TP by spelling and every truth entry no kept record spells, with its method set and tier).
    ladder_by_type: {"TM": FASTA, "TA": FASTA}, the genomes as for match_ladder, with hap_gap and ladder_type_bins (the size edges
    as for by_type; None: the default ones) (quasimodo_amd.laddertypes; needs alleles, WorkflowError before a file
    is touched otherwise), in place of match_ladder and by_type, both of which the run's call makes itself behind all four
    rescues: final_tables/caller_performance_ladder_types.tsv (per caller and mixture one row per type and size bin -- records
    typed as spelled --, a marginal per type, the four rows behind the grid as plain counts, each with TP, FP, FN, Precision,
    Recall, F1 by spelling and after each tier; then a pooled block per caller).
    Which of these may share a run: quasimodo_amd.passes (mutation_context with snp_profile; WorkflowError otherwise)."""
    callers = list(callers or SNPCALLERS)
    votes = bool(votes) or consensus_vcf is not None
    _shared_call(votes=votes, boot=bootstrap is not None, strata=strata is not None, motifs=mutation_context is not None,
                 truthside=truth_side, profile=snp_profile, nearmiss=explain_errors, surface=filter_surface,
                 context=seq_context is not None, normalize=normalize is not None, atomize=bool(atomize), vartype=by_type is not None and by_type is not False,
                 haplo=haplotypes is not None and not hap_subsets, hapsub=bool(hap_subsets), rescueroc=rescue_roc is not None,
                 ladder=match_ladder is not None, laddertypes=ladder_by_type is not None)
    if ladder_by_type is not None and not alleles:
        raise WorkflowError("--ladder-by-type needs --alleles: it crosses the variant types with the matching by normal form, by atoms and by haplotype, which only the allele-extended mode has")
    if ladder_type_bins is not None and ladder_by_type is None:
        raise WorkflowError("ladder_type_bins needs ladder_by_type (--type-bins needs --by-type or --ladder-by-type)")
    if match_ladder is not None and not alleles:
        raise WorkflowError("--match-ladder needs --alleles: it combines the matching by normal form, by atoms and by haplotype, which only the allele-extended mode has")
    if rescue_roc is not None and not alleles:
        raise WorkflowError("--rescue-roc needs --alleles: it sweeps the matching by normal form and by atoms, which only the allele-extended mode has")
    if hap_subsets and haplotypes is None:
        raise WorkflowError("--hap-subsets searches the sites of the haplotype pass: it needs --haplotypes (and the genomes)")
    hgap = None
    if haplotypes is not None:
        from .haplo import check_gap
        if not alleles:
            raise WorkflowError("--haplotypes needs --alleles: haplotypes are replayed from indels, MNPs and complex records, which only the allele-extended mode reads")
        try:
            hgap = check_gap(hap_gap)
        except ValueError as e:
            raise WorkflowError("--hap-gap: %s" % e) from None
    elif match_ladder is not None or ladder_by_type is not None:
        from .haplo import check_gap
        try:
            hgap = check_gap(hap_gap)
        except ValueError as e:
            raise WorkflowError("--hap-gap: %s" % e) from None
    elif hap_gap is not None:
        raise WorkflowError("--hap-gap needs --haplotypes or --match-ladder")
    ltedges = None
    if ladder_by_type is not None:
        from .vartype import check_edges, parse_edges
        try:
            ltedges = parse_edges(ladder_type_bins) if isinstance(ladder_type_bins, str) else check_edges(ladder_type_bins)
        except ValueError as e:
            raise WorkflowError("--type-bins: %s" % e) from None
    tedges = None
    if by_type is not None and by_type is not False:
        from .vartype import check_edges, parse_edges
        if not alleles:
            raise WorkflowError("--by-type needs --alleles: indels, MNPs and complex records are typed, which only the allele-extended mode reads")
        try:
            tedges = check_edges(None) if by_type is True else parse_edges(by_type) if isinstance(by_type, str) else check_edges(by_type)
        except ValueError as e:
            raise WorkflowError("--type-bins: %s" % e) from None
    if normalize is not None and not alleles:
        raise WorkflowError("--normalize needs --alleles: the normal form is taken of indels and MNPs, which only the allele-extended mode reads")
    if atomize and not alleles:
        raise WorkflowError("--atomize needs --alleles: atoms are taken of MNPs, which only the allele-extended mode reads")
    radius = _explain_radius(explain_errors, explain_radius)
    sweep = _surface_params(filter_surface, surface_qual_step, surface_qual_bins, surface_af_bins)
    cpar = _context_params(seq_context is not None, context_window, context_gc_bins)
    if consensus_vcf is not None and int(consensus_vcf) < 1:
        raise WorkflowError("--consensus-vcf %d: the level is at least 1" % int(consensus_vcf))
    if strata is not None:
        from .strata import freeze
        try:
            strata = freeze(strata)
        except ValueError as e:
            raise WorkflowError("strata: %s" % e) from None
    prof = None
    if snp_profile:
        from .afprofile import DEFAULTS
        opts = dict(DEFAULTS)
        opts.update({k: int(v) for k, v in (snp_profile.items() if isinstance(snp_profile, dict) else ()) if v is not None})
        prof = (opts["window"], opts["n_pos_bins"], opts["n_af_bins"])
        if not (1 <= prof[0] < (1 << 28) and prof[1] >= 1 and prof[2] >= 1 and prof[1] * prof[2] <= 8192):
            raise WorkflowError("snp profile: window %d, %d x %d bins (1 <= window < 2^28, at most 8192 cells)" % (prof[0], prof[2], prof[1]))
    data_dir = ensure_bundle(data_dir)
    results = os.path.join(outpath.rstrip("/"), "results")
    snp_dir = os.path.join(results, "snp")
    call_dir = os.path.join(snp_dir, "callers")
    samples = sorted(s for s in (os.path.basename(p).split(".")[0] for p in glob.glob(os.path.join(data_dir, "vcf", "clc", "*.clc.vcf")))
                     if s in SAMPLE_REF)
    if not samples:
        raise WorkflowError("no bundled VCFs under %s/vcf/clc" % data_dir)
    plan = []
    for s in samples:
        for c in callers:
            src = os.path.join(data_dir, "vcf", c, "%s.%s.%s.vcf" % (s, SAMPLE_REF[s], c))
            if not os.path.exists(src):
                raise WorkflowError("missing input %s" % src)
            plan.append((s, c, src))
    mixes = sorted({s[:2] for s in samples}, reverse=True)              # TM, TA
    for fastas, what in ((mutation_context, "mutation context"), (seq_context, "sequence context"), (normalize, "normalize"), (rescue_roc, "rescue ROC"), (haplotypes, "haplotypes"), (match_ladder, "match ladder"), (ladder_by_type, "ladder by type")):
        for mix in mixes if fastas is not None else ():
            if not fastas.get(mix) or not os.path.isfile(fastas.get(mix)):
                raise WorkflowError("%s: no genome FASTA for %s (%s)" % (what, mix, fastas.get(mix)))
    if dryrun:
        for s, c, src in plan:
            print("extractTP\t%s\t%s" % (c, src))
        if haplotypes is not None:
            print("caller_performance_haplotype.tsv\t%s\t%d" % (",".join(callers), hgap))
        if hap_subsets:
            print("caller_performance_hapsubsets.tsv\t%s\t%d" % (",".join(callers), hgap))
        if normalize is not None:
            print("caller_performance_normalized.tsv\t%s" % ",".join(callers))
        if atomize:
            print("caller_performance_atomized.tsv\t%s" % ",".join(callers))
        if rescue_roc is not None:
            for s, c, src in plan:
                if not s.endswith(("-1-0", "-0-1")):
                    print("rescue_roc\t%s\t%s" % (c, s))
            print("caller_roc_rescue.tsv\t%s" % ",".join(callers))
        if match_ladder is not None:
            print("caller_performance_ladder.tsv\t%s\t%d" % (",".join(callers), hgap))
        if ladder_by_type is not None:
            print("caller_performance_ladder_types.tsv\t%s\t%d\t%s" % (",".join(callers), hgap, ",".join(str(e) for e in ltedges)))
        if tedges is not None:
            print("caller_performance_types.tsv\t%s\t%s" % (",".join(callers), ",".join(str(e) for e in tedges)))
        if mutation_context is not None:
            for mix in mixes:
                for c in callers:
                    print("mutationcontext\t%s\t%s" % (mix, c))
        if prof is not None:
            for mix in mixes:
                for c in callers:
                    print("snp_profile\t%s\t%s" % (mix, c))
        if strata is not None:
            print("caller_performance_strata\t%s" % ",".join(s[0] for s in strata))
        if bootstrap is not None:
            print("caller_performance_ci\t%d" % _boot_params(bootstrap, [])[2])
        if cpar is not None:
            print("caller_performance_context.tsv\t%d\t%d" % cpar)
        if votes:
            _vote_plan(plan, consensus_vcf)
            print("caller_consensus\t%s" % ",".join(callers))
            if consensus_vcf is not None:
                for s in samples:
                    if not s.endswith(("-1-0", "-0-1")):
                        print("consensus_vcf\t%s\t%d" % (s, int(consensus_vcf)))
        if radius is not None:
            for s, c, src in plan:
                if not s.endswith(("-1-0", "-0-1")):
                    print("explain_errors\t%s\t%s\t%d" % (c, s, radius))
            print("caller_error_classes\t%s" % ",".join(callers))
        if sweep is not None:
            for s, c, src in plan:
                if not s.endswith(("-1-0", "-0-1")):
                    print("filter_surface\t%s\t%s\t%d\t%d\t%d" % ((c, s) + sweep))
            print("caller_best_filter\t%s" % ",".join(callers))
        if truth_side:
            from .truthside import venn_callers
            for s, c, src in plan:
                if not s.endswith(("-1-0", "-0-1")):
                    print("truthside_fn\t%s\t%s" % (c, s))
            vc = venn_callers(callers)
            for s in samples:
                if vc and not s.endswith(("-1-0", "-0-1")):
                    print("missed_by_all\t%s\t%s" % (s, ",".join(vc)))
            if vc:
                print("caller_snp_venn\t%s" % ",".join(vc))
        return None
    os.makedirs(os.path.join(snp_dir, "nucmer"), exist_ok=True)
    for mix in ("TM", "TA"):                                           # cp_genome_diff
        src = os.path.join(data_dir, "nucmer", "%s.maskrepeat.variants.vcf" % mix)
        if os.path.exists(src):
            shutil.copyfile(src, os.path.join(snp_dir, "nucmer", os.path.basename(src)))
    boot = None
    if bootstrap is not None:
        boot = _boot_params(bootstrap, [(t, "hcmv") for t in sorted(glob.glob(os.path.join(snp_dir, "nucmer", "T?.maskrepeat.variants.vcf")))])
    jobs, meta = [], []
    for s, c, src in plan:                                              # cp_vcf
        d = os.path.join(call_dir, c)
        os.makedirs(os.path.join(d, "fp"), exist_ok=True)
        dst = os.path.join(d, os.path.basename(src))
        shutil.copyfile(src, dst)
        jobs.append(Job(dst, os.path.join(snp_dir, "nucmer", "%s.maskrepeat.variants.vcf" % s[:2]), "hcmv", d, c,
                        genome=mutation_context.get(s[:2]) if mutation_context is not None and not s.endswith("-1-0") else None))
        if prof is not None and not s.endswith("-1-0"):
            jobs[-1].profile = prof
            jobs[-1].points_out = os.path.join(d, "profile", os.path.basename(src)[:-4] + ".points.tsv")
        jobs[-1].strata = strata
        jobs[-1].boot = boot
        if cpar is not None:
            jobs[-1].context, jobs[-1].context_genome = cpar, seq_context[s[:2]]
        if normalize is not None and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].normalize = normalize[s[:2]]
            jobs[-1].rescued_out = os.path.join(d, "norm", os.path.basename(src)[:-4] + ".rescued.tsv")
        if atomize and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].atomize = True
            jobs[-1].atoms_out = os.path.join(d, "atoms", os.path.basename(src)[:-4] + ".atoms.tsv")
        if tedges is not None and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].vartype = tedges
        if rescue_roc is not None and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].rescue_roc = rescue_roc[s[:2]]
        if match_ladder is not None and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].ladder, jobs[-1].ladder_genome = hgap, match_ladder[s[:2]]
            jobs[-1].ladder_out = os.path.join(d, "ladder", os.path.basename(src)[:-4] + ".ladder.tsv")
        if ladder_by_type is not None and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].ladder_types, jobs[-1].ladder_types_genome = (hgap, ltedges), ladder_by_type[s[:2]]
        if haplotypes is not None and not s.endswith(("-1-0", "-0-1")):
            jobs[-1].haplo_genome = haplotypes[s[:2]]
            jobs[-1].haplo, jobs[-1].hapsub = (None, hgap) if hap_subsets else (hgap, None)
            jobs[-1].sites_out = os.path.join(d, "hap", os.path.basename(src)[:-4] + ".sites.tsv")
            if hap_subsets:
                jobs[-1].subsets_out = os.path.join(d, "hap", os.path.basename(src)[:-4] + ".subsets.tsv")
        meta.append((c, s))
    from .vcfio import split_variants
    for kind in ("xsnp", "xindel"):                                      # extract_snp / extract_indel / extract_nucmer_*:
        for j in jobs:                                                   # both declared outputs, *.vcf and its bgzip
            split_variants(j.vcf_file, j.vcf_file[:-4] + ".%s.vcf" % kind, kind, bgz=True, tbi="if-sorted")
        for mix in ("TM", "TA"):
            t = os.path.join(snp_dir, "nucmer", "%s.maskrepeat.variants.vcf" % mix)
            if os.path.exists(t):
                split_variants(t, os.path.join(snp_dir, "nucmer", "%s.maskrepeat.%s.vcf" % (mix, kind)), kind, bgz=True, tbi="if-sorted")
    mixed = [s for s in samples if not s.endswith(("-1-0", "-0-1"))]
    if truth_side:
        from .extract import _paths, fn_path
        from .truthside import venn_callers
        vc = venn_callers(callers)
        for (c, s), j in zip(meta, jobs):
            if s in mixed:
                _paths(j)
                j.fn_out = fn_path(j)
                if c in vc:
                    j.group = s
                    j.missed_out = os.path.join(snp_dir, "nucmer", "%s.missed_by_all.vcf" % s)
    if votes:
        _vote_plan(plan, consensus_vcf)
        for (c, s), j in zip(meta, jobs):
            if s in mixed:
                j.vote_group = s
                if consensus_vcf is not None:
                    j.consensus_k = int(consensus_vcf)
                    j.consensus_out = os.path.join(snp_dir, "consensus", "%s.%s.k%d.vcf" % (s, SAMPLE_REF[s], int(consensus_vcf)))
    if radius is not None:
        _explain_jobs([j for (c, s), j in zip(meta, jobs) if s in mixed], radius)
    if sweep is not None:
        for (c, s), j in zip(meta, jobs):
            if s in mixed:
                j.surface = sweep
    cmp_callers = [c for c in FP_COMPARED if c in callers]
    tables = os.path.join(results, "final_tables")

    def write_tables(jobs):   # the tables of the rows and of every pass of the run: the same on one GPU and on several
        os.makedirs(tables, exist_ok=True)
        _flag_truth_rows(jobs)
        write_caller_performance(os.path.join(tables, "caller_performance.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        _write_snp_rocs(meta, jobs, snp_dir)
        if mutation_context is not None:
            _write_mutation_context(meta, jobs, tables, callers, mixes)
        if prof is not None:
            _write_snp_profile(meta, jobs, tables, callers, mixes, prof[0])
        if strata is not None:
            _write_strata(meta, jobs, tables, strata)
        if boot is not None:
            _write_bootstrap(meta, jobs, tables)
        if truth_side:
            _write_caller_snp_venn(meta, jobs, tables, callers, mixed)
        if votes:
            _write_votes(meta, jobs, tables, mixed)
        if radius is not None:
            _write_error_classes([(c, s, j) for (c, s), j in zip(meta, jobs) if s in mixed], tables)
        if cpar is not None:
            _write_context(os.path.join(tables, "caller_performance_context.tsv"), [(c, s, j) for (c, s), j in zip(meta, jobs)], cpar)
        if sweep is not None:
            _write_surface([(c, s, j) for (c, s), j in zip(meta, jobs) if s in mixed], tables, sweep[0])
        if normalize is not None:
            from .normalize import write_performance_normalized
            write_performance_normalized(os.path.join(tables, "caller_performance_normalized.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        if haplotypes is not None:
            from .haplo import write_performance_haplotype
            write_performance_haplotype(os.path.join(tables, "caller_performance_haplotype.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        if hap_subsets:
            from .haplo import write_performance_hapsubsets
            write_performance_hapsubsets(os.path.join(tables, "caller_performance_hapsubsets.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        if atomize:
            from .atomize import write_performance_atomized
            write_performance_atomized(os.path.join(tables, "caller_performance_atomized.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        if rescue_roc is not None:
            _write_rescue_rocs(meta, jobs, snp_dir, tables)
        if match_ladder is not None:
            from .ladder import write_performance_ladder
            write_performance_ladder(os.path.join(tables, "caller_performance_ladder.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        if ladder_by_type is not None:
            from .laddertypes import write_performance_ladder_types
            write_performance_ladder_types(os.path.join(tables, "caller_performance_ladder_types.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)], ltedges)
        if tedges is not None:
            from .vartype import write_performance_types
            write_performance_types(os.path.join(tables, "caller_performance_types.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)], tedges)
    if gpus is not None and (int(gpus) > 1 or _body):
        if engine is not None:
            raise ValueError("gpus > 1 starts one process (and one engine) per GPU: do not pass an engine")
        from .multigpu import extract_many_sharded
        groups = [[i for i, (c, s) in enumerate(meta) if s == smp] for smp in samples]
        jobs, res = extract_many_sharded(jobs, int(gpus), backend=_backend, body=_body, same_device=_same_device, groups=groups,
                                         alleles=True if alleles else None, post="quasimodo_amd.workflow:hcmv_rank_post",
                                         post_args=dict(meta=meta, cmp_callers=cmp_callers, snp_dir=snp_dir))
        write_tables(jobs)
        if mixed and len(cmp_callers) >= 2:
            reg = {}
            for e in res["extras"]:
                reg.update((e or {}).get("overlap", {}))
            missing = [s for s in mixed if s not in reg]
            if missing:
                raise WorkflowError("no FP overlap came back for %s" % ", ".join(missing))
            write_fp_overlap(os.path.join(tables, "snpcaller_fp_snp_compare.txt"), {s: reg[s] for s in mixed}, cmp_callers)
        run_hcmv_variantcall.last_result = res
        return jobs
    own = engine is None
    if own:
        engine = Engine(int(os.environ.get("QM_DEVICE", "0")))
    try:
        extract_many(jobs, engine=engine, alleles=True if alleles else None)   # extractTP, one batch
        write_tables(jobs)
        indel_roc(engine, [(c, smp, j) for (c, smp), j in zip(meta, jobs) if not j.stats.get("pure_strain")], snp_dir)
        if mixed and len(cmp_callers) >= 2:                              # compareFP (counts only)
            files = {s: {c: j.fp_out for (c, ss), j in zip(meta, jobs) if ss == s and c in cmp_callers} for s in mixed}
            reg = fp_overlap_tables(engine, files, cmp_callers)
            write_fp_overlap(os.path.join(tables, "snpcaller_fp_snp_compare.txt"), reg, cmp_callers)
    finally:
        if own:
            engine.close()
    return jobs


run_hcmv_variantcall.last_result = None


def _explain_radius(explain_errors, explain_radius):
    """the radius of --explain-errors (None: the pass is off)"""
    from .nearmiss import DEFAULT_RADIUS, check_radius
    if not explain_errors:
        if explain_radius is not None:
            raise WorkflowError("--explain-radius goes with --explain-errors")
        return None
    try:
        return check_radius(DEFAULT_RADIUS if explain_radius is None else explain_radius)
    except ValueError as e:
        raise WorkflowError("--explain-radius: %s" % e) from None


def _context_params(on, window, gc_bins):
    """the parameter pair of --seq-context (None: the pass is off)"""
    from .context import DEFAULT_GC_BINS, DEFAULT_HALF_WINDOW, check_params
    if not on:
        if window is not None or gc_bins is not None:
            raise WorkflowError("--context-window and --context-gc-bins go with --seq-context")
        return None
    try:
        return check_params(DEFAULT_HALF_WINDOW if window is None else window, DEFAULT_GC_BINS if gc_bins is None else gc_bins)
    except ValueError as e:
        raise WorkflowError("--seq-context: %s" % e) from None


def _write_context(path, rows, cpar, custom=False):
    """the sequence-context table: rows of (caller or label, sample, job); genomediff per cell from the truth
    file's rows as R counts them, placed through the numpy restatement of the genome's table (one per truth file and genome)"""
    from .context import cells, truth_rows, write_performance_context
    from .motifs import read_fasta
    tabs, seen = {}, {}
    for c, s, j in rows:
        if "context_rec" not in j.stats:
            raise WorkflowError("%s/%s: no sequence-context counts came back" % (c, s))
        if not j.stats.get("pure_strain") and j.stats.get("context_tru") is not None:
            key = (os.path.realpath(j.snp_file), j.mode, os.path.realpath(j.context_genome))
            if key not in seen:
                if key[2] not in tabs:
                    tabs[key[2]] = cells(read_fasta(j.context_genome), *cpar)
                seen[key] = truth_rows(j.snp_file, j.mode, tabs[key[2]], cpar[1])
            j.stats["context_genomediff"] = seen[key]
    write_performance_context(path, [(c, s, j.stats) for c, s, j in rows], cpar[1], custom=custom)


def _surface_params(filter_surface, q_step, nq, na):
    """the parameter triple of --filter-surface (None: the pass is off)"""
    from .surface import workflow_params
    if not filter_surface:
        if q_step is not None or nq is not None or na is not None:
            raise WorkflowError("--surface-qual-step, --surface-qual-bins and --surface-af-bins go with --filter-surface")
        return None
    try:
        return workflow_params(q_step, nq, na)
    except ValueError as e:
        raise WorkflowError("--filter-surface: %s" % e) from None


def _write_surface(rows, tables, q_step):
    """the surface table of every swept job beside its fp/ and tp/, and final_tables/caller_best_filter.tsv: (caller, sample, job)"""
    from .extract import _paths
    from .surface import TRUTH, surface_path, write_caller_best_filter, write_surface
    out = []
    for c, s, j in rows:
        if j.stats.get("pure_strain"):
            continue
        if "surface" not in j.stats:
            raise WorkflowError("%s/%s: no filter surface came back" % (c, s))
        if not j.fp_out:
            _paths(j)
        write_surface(surface_path(j), j.stats["surface"], j.stats["surface_extra"][TRUTH], q_step)
        out.append((c, s, j.stats["surface"], j.stats["surface_extra"]))
    if out:
        write_caller_best_filter(os.path.join(tables, "caller_best_filter.tsv"), out, q_step)


def _explain_jobs(jobs, radius):
    """the near-miss pass and the two why-files of every mixed-sample job"""
    from .extract import _paths
    from .nearmiss import fn_why_path, fp_why_path
    for j in jobs:
        if not is_pure_strain(j.vcf_file):
            _paths(j)
            j.explain, j.fp_why_out, j.fn_why_out = radius, fp_why_path(j), fn_why_path(j)


def _write_error_classes(rows, tables):
    """final_tables/caller_error_classes.tsv from the rows of the explained jobs: (caller, sample, job)"""
    from .nearmiss import write_caller_error_classes
    out = []
    for c, s, j in rows:
        if j.stats.get("pure_strain"):
            continue
        if "nearmiss_rec" not in j.stats:
            raise WorkflowError("%s/%s: no error classes came back" % (c, s))
        out.append((c, s, j.stats["nearmiss_rec"], j.stats["nearmiss_tru"]))
    if out:
        write_caller_error_classes(os.path.join(tables, "caller_error_classes.tsv"), out)


def _vote_plan(plan, consensus_vcf):
    """the callers of every mixed sample of the run: 1 to 32, and not fewer than the consensus level"""
    from .consensus import MAX_GROUP
    per = {}
    for s, c, _ in plan:
        if not s.endswith(("-1-0", "-0-1")):
            per.setdefault(s, []).append(c)
    for s in sorted(per):
        if len(per[s]) > MAX_GROUP:
            raise WorkflowError("sample %s: %d callers, a vote group holds at most %d" % (s, len(per[s]), MAX_GROUP))
        if consensus_vcf is not None and int(consensus_vcf) > len(per[s]):
            raise WorkflowError("sample %s: --consensus-vcf %d, but the sample has %d callers" % (s, int(consensus_vcf), len(per[s])))
    return per


def _write_votes(meta, jobs, tables, mixed):
    """final_tables/caller_consensus.tsv and caller_private.tsv from the rows of every mixed sample's vote group"""
    from .consensus import write_caller_consensus, write_caller_private
    cons, priv = {}, {}
    for s in mixed:
        mem = [(c, j) for (c, ss), j in zip(meta, jobs) if ss == s]
        st = mem[0][1].stats
        if "tp_votes" not in st or len(st.get("vote_callers") or []) != len(mem):
            raise WorkflowError("sample %s: no vote counts came back for its callers" % s)
        n = len(mem)
        cons[s] = (n, [int(x) for x in st["tp_votes"]], [int(x) for x in st["fp_votes"]])
        priv[s] = (list(st["vote_callers"]), [int(x) for x in st["private_tp"]], [int(x) for x in st["private_fp"]])
    if cons:
        write_caller_consensus(os.path.join(tables, "caller_consensus.tsv"), cons)
        write_caller_private(os.path.join(tables, "caller_private.tsv"), priv)


def _write_caller_snp_venn(meta, jobs, tables, callers, mixed):
    """final_tables/caller_snp_venn.tsv (the numbers behind final_figures/caller_snp_venndiagram.pdf): per mixed sample the
    regions of Genome + the Venn callers, from the rows of the sample's group (members in job order, put into the Venn callers' order)"""
    from .truthside import reorder_regions, venn_callers, write_caller_snp_venn
    vc = venn_callers(callers)
    if not vc or not mixed:
        return
    per = {}
    for s in mixed:
        mem = [(c, j) for (c, ss), j in zip(meta, jobs) if ss == s and c in vc]
        have = [c for c, _ in mem]
        st = mem[0][1].stats
        if len(mem) != len(vc) or "truth_regions" not in st:
            raise WorkflowError("sample %s: no truth-side regions came back for its Venn callers" % s)
        n = len(vc)
        per[s] = (reorder_regions(st["truth_regions"][:1 << n], have, vc), reorder_regions(st["fp_regions"][:1 << n], have, vc))
    write_caller_snp_venn(os.path.join(tables, "caller_snp_venn.tsv"), per, vc)


def _strata_genomediff(jobs, strata):
    """stats["strata_genomediff"] of every mixed-sample job: its truth file's rows per stratum as R counts them (one read per file)"""
    from .strata import truth_rows
    seen = {}
    for j in jobs:
        if not j.stats.get("pure_strain"):
            key = (j.snp_file, j.mode)
            if key not in seen:
                seen[key] = truth_rows(j.snp_file, j.mode, strata)
            j.stats["strata_genomediff"] = seen[key]


def _write_strata(meta, jobs, tables, strata):
    """final_tables/caller_performance_strata.tsv: the rows of caller_performance.tsv per stratum"""
    from .strata import write_performance_strata
    names = [s[0] for s in strata]
    for (c, s), j in zip(meta, jobs):
        if "strata_rec" not in j.stats:
            raise WorkflowError("%s / %s: no counts per stratum came back" % (c, s))
    _strata_genomediff(jobs, strata)
    write_performance_strata(os.path.join(tables, "caller_performance_strata.tsv"), [(c, s, names, j.stats) for (c, s), j in zip(meta, jobs)])


def _boot_params(bootstrap, truth_files):
    """(window, n_win, n_rep, seed) of a run: the defaults, what `bootstrap` (a replicate count or a dict) says, and n_win raised
    to cover the largest POS of truth_files [(path, mode)]; ValueError when that takes more than 4096 windows"""
    from .bootstrap import DEFAULTS, MAX_REP, truth_max_pos, windows_for
    opts = dict(DEFAULTS)
    if isinstance(bootstrap, dict):
        opts.update({k: int(v) for k, v in bootstrap.items() if v is not None})
    else:
        opts["n_rep"] = int(bootstrap)
    if opts["window"] < 1 or opts["window"] > (1 << 31) - 1:
        raise ValueError("bootstrap: window %d (1 to 2^31 - 1)" % opts["window"])
    if not 1 <= opts["n_rep"] <= MAX_REP:
        raise ValueError("bootstrap: %d replicates (1 to %d)" % (opts["n_rep"], MAX_REP))
    top = max([truth_max_pos(p, m) for p, m in truth_files] or [0])
    return (opts["window"], windows_for(top, opts["window"], opts["n_win"]), opts["n_rep"], opts["seed"])


def _boot_extra(jobs):
    """stats["boot_extra"] of every mixed-sample job: its truth file's rows per window as R counts them minus the device's
    distinct keys there (one read per file)"""
    from .bootstrap import TRUTH_KEYS, truth_row_windows
    seen = {}
    for j in jobs:
        if not j.stats.get("pure_strain") and j.stats.get("boot_truth", True):
            prm = j.stats["boot_params"]
            key = (j.snp_file, j.mode)
            if key not in seen:
                seen[key] = truth_row_windows(j.snp_file, j.mode, prm["window"], prm["n_win"])
            j.stats["boot_extra"] = seen[key] - j.stats["boot_cnt"][:prm["n_win"] + 1, TRUTH_KEYS].astype("int64")


def _write_bootstrap(meta, jobs, tables):
    """final_tables/caller_performance_ci.tsv and caller_performance_ci_pairs.tsv"""
    from .bootstrap import write_performance_ci, write_performance_ci_pairs
    for (c, s), j in zip(meta, jobs):
        if "boot_cnt" not in j.stats:
            raise WorkflowError("%s / %s: no bootstrap counts came back" % (c, s))
    _boot_extra(jobs)
    rows = [(c, s, j.stats) for (c, s), j in zip(meta, jobs)]
    write_performance_ci(os.path.join(tables, "caller_performance_ci.tsv"), rows)
    write_performance_ci_pairs(os.path.join(tables, "caller_performance_ci_pairs.tsv"), rows)


def _write_mutation_context(meta, jobs, tables, callers, mixes):
    """rule mutationcontext's numbers (scripts/mutation_context_profile.R without the plot): one table per mix and caller"""
    from .motifs import study_columns, write_mutation_context
    for mix in mixes:
        for c in callers:
            rows = {s: j.stats["motifs"] for (cc, s), j in zip(meta, jobs) if cc == c and s[:2] == mix and not s.endswith("-1-0")}
            if rows:
                write_mutation_context(os.path.join(tables, "%s.%s.mutationcontext.tsv" % (mix, c)), study_columns(rows))


def _write_snp_profile(meta, jobs, tables, callers, mixes, window):
    """the numbers behind {mix}.{caller}.snp.profile.pdf (varPlot of scripts/mutation_context_profile.R): two tables per mix and caller"""
    from .afprofile import sample_rows, write_af_sweep, write_profile_grid
    for mix in mixes:
        for c in callers:
            st = {s: j.stats for (cc, s), j in zip(meta, jobs) if cc == c and s[:2] == mix and not s.endswith("-1-0")}
            if st:
                rows = sample_rows(st)
                write_profile_grid(os.path.join(tables, "%s.%s.snp.profile.tsv" % (mix, c)), rows, window=window)
                write_af_sweep(os.path.join(tables, "%s.%s.snp.profile.afsweep.tsv" % (mix, c)), rows)


def _write_snp_rocs(meta, jobs, snp_dir):
    """The engine's exact-match ROC sweeps, in the column layout of RTG's weighted_roc.tsv.gz but under a directory of
    their own: results/snp/rtg/ belongs to the reference's rtg rules (rules/vis_eval_vcf.smk:5-121), whose
    haplotype-aware numbers these are not."""
    for (c, smp), j in zip(meta, jobs):
        if not j.stats.get("pure_strain") and j.stats.get("roc") is not None:
            d = os.path.join(snp_dir, "qmvt_roc", c, "%s.%s.xsnp" % (smp, SAMPLE_REF[smp]))
            os.makedirs(d, exist_ok=True)
            write_weighted_roc(os.path.join(d, "exact_roc.tsv.gz"), j.stats["roc"], j.stats["truth_unique"])


def write_job_rescue_rocs(d, stats):
    """spelling_roc.tsv.gz (the batch's own ROC, for the side by side), normalized_roc.tsv.gz and atomized_roc.tsv.gz of one job
    under d, in the layout of exact_roc.tsv.gz; returns {matching: (roc, baseline)}, None for a job without the
    rows (a pure-strain sample)"""
    import numpy as np
    from .tables import write_rescue_roc
    if stats.get("pure_strain") or "rroc_n" not in stats:
        return None
    rocs = {"spelling": (stats["roc"], int(stats["truth_unique"])), "normalized": (stats["rroc_n"], int(stats["rroc_base"][0])),
            "atomized": (stats["rroc_a"], int(stats["rroc_base"][1]))}
    os.makedirs(d, exist_ok=True)
    for m, (roc, base) in rocs.items():
        write_rescue_roc(os.path.join(d, "%s_roc.tsv.gz" % m), np.asarray(roc), base, m)
    return rocs


def _write_rescue_rocs(meta, jobs, snp_dir, tables):
    """the three ROC files of every mixed sample under snp/qmvt_roc/{caller}/{sample}.{ref}.rescue/ -- a directory of their own
    beside the exact-match ROC's -- and final_tables/caller_roc_rescue.tsv"""
    from .rescueroc import write_caller_roc_rescue
    rows = []
    for (c, smp), j in zip(meta, jobs):
        rocs = write_job_rescue_rocs(os.path.join(snp_dir, "qmvt_roc", c, "%s.%s.rescue" % (smp, SAMPLE_REF[smp])), j.stats)
        rows.append((c, smp, {"rroc": rocs} if rocs else {}))
    write_caller_roc_rescue(os.path.join(tables, "caller_roc_rescue.tsv"), rows)


def indel_roc(engine, items, snp_dir, n_bins=256):
    """The xindel counterpart of the exact-match ROC: the caller's *.xindel.vcf against the truth's *.xindel.vcf
    (extract_indel / extract_nucmer_indel, rules/vis_eval_vcf.smk:40-86) in the allele-extended mode -- REF and ALT
    matched as whole [ACGT]+ strings -- one batch for all VCFs.  Build-defined (the reference leaves indels to rtg
    vcfeval, rule rtg_indel); rows whose alleles are not [ACGT]+ (multi-allelic, lower case) take no part."""
    from .vcfio import AlleleDict, scan_truth, scan_vcf
    if not items:
        return
    adict = AlleleDict()
    tids, cols, keep = {}, [], []
    try:
        for c, smp, j in items:
            tfile = os.path.join(snp_dir, "nucmer", "%s.maskrepeat.xindel.vcf" % smp[:2])
            vfile = j.vcf_file[:-4] + ".xindel.vcf"
            if not (os.path.exists(tfile) and os.path.exists(vfile)):
                continue
            if tfile not in tids:
                with open(tfile, "rb") as fh:
                    tk = scan_truth(fh.read(), alleles=adict)
                tids[tfile] = engine.truth_load(tk.pos, tk.ref, tk.alt)
            with open(vfile, "rb") as fh:
                sv = scan_vcf(fh.read(), alleles=adict)
            cols.append(sv.columns)
            keep.append((c, smp, tids[tfile]))
        if not cols:
            return
        res, _ = engine.classify_batch(cols, [k[2] for k in keep], n_bins=n_bins, alleles=True)
        for (c, smp, tid), r in zip(keep, res):
            d = os.path.join(snp_dir, "qmvt_roc", c, "%s.%s.xindel" % (smp, SAMPLE_REF[smp]))
            os.makedirs(d, exist_ok=True)
            write_weighted_roc(os.path.join(d, "exact_roc.tsv.gz"), r["roc"], r["scalars"]["truth_unique"])
    finally:
        for t in tids.values():
            engine.truth_release(t)
        adict.close()


def run_vareval(vcfs, snps_file, outpath, labels=None, engine=None, dryrun=False, gpus=None, _body=None, _backend="nccl", _same_device=False,
                truth_side=False, strata=None, bootstrap=None, votes=False, consensus_vcf=None, explain_errors=False, explain_radius=None,
                filter_surface=False, surface_qual_step=None, surface_qual_bins=None, surface_af_bins=None, seq_context=None,
                context_window=None, context_gc_bins=None):
    """eval_variant_custom.smk with the genome difference (show-snps -CTHIlr TSV) already computed.
    gpus > 1: the VCFs are dealt to that many GPUs (one process each); the rows come back for the table.
    truth_side: callers/fn/{label}.fn.vcf for every VCF; up to five labels form one group (one rank) and
    final_tables/caller_snp_venn.tsv is written, more are told so and get their FN files only.
    strata: a list of (name, starts, ends) BED strata: final_tables/snpcall_benchmark_strata.txt is written.
    bootstrap: a replicate count or {"n_rep", "window", "n_win", "seed"}: final_tables/snpcall_benchmark_ci.txt
    is written.
    votes: the labels form one vote group: final_tables/caller_consensus.tsv and caller_private.tsv (sample
    "custom"); more than 32 labels (or pure-strain names) are told so and get no table.  consensus_vcf=K (implies votes) also writes
    snp/consensus/custom.k{K}.vcf; K above the label count is a WorkflowError.
    explain_errors, with explain_radius (default 10): callers/why/{label}.fp.why.tsv and {label}.fn.why.tsv for every VCF and
    final_tables/caller_error_classes.tsv.
    filter_surface, with surface_qual_step / surface_qual_bins / surface_af_bins (default 4, 64, 50): callers/surface/{label}.surface.tsv
    for every VCF and final_tables/caller_best_filter.tsv (sample "custom").
    seq_context: the FASTA of the genome the VCFs were called against (the first reference: the POS of the genome-difference table
    are its coordinates), with context_window / context_gc_bins (default 50, 10): final_tables/snpcall_benchmark_context.txt is
    written.
    Each of the seven runs alone (quasimodo_amd.passes; WorkflowError otherwise)."""
    from .truthside import MAX_GROUP
    from .consensus import MAX_GROUP as VOTE_MAX
    votes = bool(votes) or consensus_vcf is not None
    _shared_call(votes=votes, boot=bootstrap is not None, strata=strata is not None, truthside=truth_side, nearmiss=explain_errors, surface=filter_surface,
                 context=seq_context is not None)
    radius = _explain_radius(explain_errors, explain_radius)
    sweep = _surface_params(filter_surface, surface_qual_step, surface_qual_bins, surface_af_bins)
    cpar = _context_params(seq_context is not None, context_window, context_gc_bins)
    if cpar is not None and not os.path.isfile(seq_context):
        raise WorkflowError("sequence context: no genome FASTA (%s)" % seq_context)
    if consensus_vcf is not None and int(consensus_vcf) < 1:
        raise WorkflowError("--consensus-vcf %d: the level is at least 1" % int(consensus_vcf))
    if strata is not None:
        from .strata import freeze
        try:
            strata = freeze(strata)
        except ValueError as e:
            raise WorkflowError("strata: %s" % e) from None
    results = os.path.join(outpath.rstrip("/"), "results")
    call_dir = os.path.join(results, "snp", "callers")
    labels = list(labels) if labels else [os.path.splitext(os.path.basename(v))[0] for v in vcfs]
    if len(labels) != len(vcfs):
        raise WorkflowError("labels and vcfs differ in length")
    voted = votes and len(labels) <= VOTE_MAX and not any(is_pure_strain(v) for v in vcfs)
    if votes and not voted:
        print("votes: %d labels (or pure-strain names): a vote group holds 1 to %d mixed samples, no table is written" % (len(labels), VOTE_MAX))
    if voted and consensus_vcf is not None and int(consensus_vcf) > len(labels):
        raise WorkflowError("sample custom: --consensus-vcf %d, but there are %d labels" % (int(consensus_vcf), len(labels)))
    if dryrun:
        for lab, v in zip(labels, vcfs):
            print("extract_TP\t%s\t%s" % (lab, v))
        if cpar is not None:
            print("snpcall_benchmark_context.txt\t%d\t%d" % cpar)
        if voted:
            print("caller_consensus\t%s" % ",".join(labels))
            if consensus_vcf is not None:
                print("consensus_vcf\tcustom\t%d" % int(consensus_vcf))
        if radius is not None:
            for lab in labels:
                print("explain_errors\t%s\t%d" % (lab, radius))
            print("caller_error_classes\t%s" % ",".join(labels))
        if sweep is not None:
            for lab, v in zip(labels, vcfs):
                if not is_pure_strain(v):
                    print("filter_surface\t%s\t%d\t%d\t%d" % ((lab,) + sweep))
            print("caller_best_filter\t%s" % ",".join(labels))
        if truth_side:
            for lab in labels:
                print("truthside_fn\t%s" % lab)
            if len(labels) <= MAX_GROUP:
                print("caller_snp_venn\t%s" % ",".join(labels))
        return None
    if not os.path.exists(snps_file) or os.path.getsize(snps_file) == 0:
        raise WorkflowError("No difference between two genomes!")       # custom_snp_benchmark.R:19-21
    os.makedirs(os.path.join(call_dir, "fp"), exist_ok=True)
    boot = _boot_params(bootstrap, [(snps_file, "custom")]) if bootstrap is not None else None
    jobs = [Job(v, snps_file, "custom", call_dir, lab, strata=strata, boot=boot) for lab, v in zip(labels, vcfs)]
    if cpar is not None:
        for j in jobs:
            j.context, j.context_genome = cpar, seq_context
    grouped = truth_side and len(labels) <= MAX_GROUP and not any(is_pure_strain(v) for v in vcfs)
    if truth_side:
        from .extract import _paths, fn_path
        if not grouped:
            print("truth side: %d labels (or pure-strain names): the Venn regions are skipped, FN files are still written" % len(labels))
        for j in jobs:
            _paths(j)
            if not is_pure_strain(j.vcf_file):
                j.fn_out = fn_path(j)
                j.group = "vareval" if grouped else None
    if radius is not None:
        _explain_jobs(jobs, radius)
    if sweep is not None:
        for j in jobs:
            if not is_pure_strain(j.vcf_file):
                j.surface = sweep
    if voted:
        for j in jobs:
            j.vote_group = "custom"
            if consensus_vcf is not None:
                j.consensus_k = int(consensus_vcf)
                j.consensus_out = os.path.join(results, "snp", "consensus", "custom.k%d.vcf" % int(consensus_vcf))
    if gpus is not None and (int(gpus) > 1 or _body):
        if engine is not None:
            raise ValueError("gpus > 1 starts one process (and one engine) per GPU: do not pass an engine")
        from .multigpu import extract_many_sharded
        jobs, res = extract_many_sharded(jobs, int(gpus), backend=_backend, body=_body, same_device=_same_device,
                                         groups=[list(range(len(jobs)))] if grouped or voted else None)
        run_vareval.last_result = res
    else:
        extract_many(jobs, engine=engine)
    os.makedirs(os.path.join(results, "final_tables"), exist_ok=True)
    _flag_truth_rows(jobs)
    write_snpcall_benchmark(os.path.join(results, "final_tables", "snpcall_benchmark.txt"),
                            [(lab, j.stats) for lab, j in zip(labels, jobs)])
    if strata is not None:
        from .strata import write_performance_strata
        _strata_genomediff(jobs, strata)
        write_performance_strata(os.path.join(results, "final_tables", "snpcall_benchmark_strata.txt"),
                                 [(lab, None, [s[0] for s in strata], j.stats) for lab, j in zip(labels, jobs)], custom=True)
    if boot is not None:
        from .bootstrap import write_performance_ci
        _boot_extra(jobs)
        write_performance_ci(os.path.join(results, "final_tables", "snpcall_benchmark_ci.txt"), [(lab, None, j.stats) for lab, j in zip(labels, jobs)], custom=True)
    if cpar is not None:
        _write_context(os.path.join(results, "final_tables", "snpcall_benchmark_context.txt"), [(lab, None, j) for lab, j in zip(labels, jobs)], cpar, custom=True)
    if voted:
        _write_votes([(lab, "custom") for lab in labels], jobs, os.path.join(results, "final_tables"), ["custom"])
    if radius is not None:
        _write_error_classes([(lab, "custom", j) for lab, j in zip(labels, jobs)], os.path.join(results, "final_tables"))
    if sweep is not None:
        _write_surface([(lab, "custom", j) for lab, j in zip(labels, jobs)], os.path.join(results, "final_tables"), sweep[0])
    if grouped:
        from .truthside import write_caller_snp_venn
        n = len(labels)
        st = jobs[0].stats
        write_caller_snp_venn(os.path.join(results, "final_tables", "caller_snp_venn.tsv"),
                              {"custom": (list(st["truth_regions"][:1 << n]), list(st["fp_regions"][:1 << n]))}, labels)
    return jobs


run_vareval.last_result = None
