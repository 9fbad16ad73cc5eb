"""The path's slice of the two Snakemake workflows, without Snakemake.

  hcmv -e variantcall (bundled-VCF mode): eval_variantcall.smk cp_vcf / cp_genome_diff (:62-93) ->
      rules/extract_TP.smk -> rules/vis_eval_vcf.smk snp_evaluate (table only) -> rules/compare_FP.smk
  vareval: eval_variant_custom.smk extract_TP (:58-74) -> snp_benchmark (table only, :76-92)

Everything upstream (reads -> VCF, nucmer) and every figure is out of scope:
the inputs must already exist.  Every mixed-sample VCF of a run goes through ONE engine batch."""
import glob
import os
import shutil
from collections import namedtuple
from types import SimpleNamespace

from .context import DEFAULT_GC_BINS, DEFAULT_HALF_WINDOW, check_params
from .engine import Engine
from .extract import Job, extract_many, is_pure_strain
from .haplo import check_gap
from .nearmiss import DEFAULT_RADIUS, check_radius
from .passes import PASSES, SharedCallError, check_shared_call
from .strata import freeze
from .surface import workflow_params
from .tables import r_hostile_rows, write_caller_performance, write_fp_overlap, write_snpcall_benchmark, write_weighted_roc
from .vartype import check_edges, parse_edges
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
    alleles: the allele-extended mode (include/qmvt.h): indels and MNPs take part, matched by spelling.
    Every other keyword belongs to one pass over the finished batch: WORKFLOW_PASSES below says what each takes and writes, and
    quasimodo_amd.passes which of them may share a run (mutation_context with snp_profile; WorkflowError otherwise).  A pass that
    reads indels or MNPs needs alleles: WorkflowError before a file is touched otherwise."""
    kw = dict(locals())
    callers = list(callers or SNPCALLERS)
    passes = WORKFLOW_PASSES
    par = _checked(passes, kw)
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
    mixed = [s for s in samples if not s.endswith(("-1-0", "-0-1"))]
    tables = os.path.join(results, "final_tables")
    meta = [(c, s) for s, c, _ in plan]
    run = SimpleNamespace(custom=False, kw=kw, names=callers, units=[(c, s, src) for s, c, src in plan], meta=meta, mixed=mixed, snp_dir=snp_dir,
                          mixes=sorted({s[:2] for s in samples}, reverse=True), tables=tables, one_group=False)      # mixes: TM, TA
    _check_genomes(passes, par, run)
    _each(passes, par, "plan", run)
    if dryrun:
        for s, c, src in plan:
            print("extractTP\t%s\t%s" % (c, src))
        _each(passes, par, "dry", run, DRY_ORDER)
        return None
    os.makedirs(os.path.join(snp_dir, "nucmer"), exist_ok=True)
    for mix in ("TM", "TA"):                                           # cp_genome_diff
        src = os.path.join(data_dir, "nucmer", "%s.maskrepeat.variants.vcf" % mix)
        if os.path.exists(src):
            shutil.copyfile(src, os.path.join(snp_dir, "nucmer", os.path.basename(src)))
    run.truth_files = [(t, "hcmv") for t in sorted(glob.glob(os.path.join(snp_dir, "nucmer", "T?.maskrepeat.variants.vcf")))]
    _each(passes, par, "ready", run)
    jobs = []
    for s, c, src in plan:                                              # cp_vcf
        d = os.path.join(call_dir, c)
        os.makedirs(os.path.join(d, "fp"), exist_ok=True)
        dst = os.path.join(d, os.path.basename(src))
        shutil.copyfile(src, dst)
        jobs.append(Job(dst, os.path.join(snp_dir, "nucmer", "%s.maskrepeat.variants.vcf" % s[:2]), "hcmv", d, c))
    _onto_jobs(passes, par, run, jobs)
    from .vcfio import split_variants
    for kind in ("xsnp", "xindel"):                                      # extract_snp / extract_indel / extract_nucmer_*:
        for j in jobs:                                                   # both declared outputs, *.vcf and its bgzip
            split_variants(j.vcf_file, j.vcf_file[:-4] + ".%s.vcf" % kind, kind, bgz=True, tbi="if-sorted")
        for mix in ("TM", "TA"):
            t = os.path.join(snp_dir, "nucmer", "%s.maskrepeat.variants.vcf" % mix)
            if os.path.exists(t):
                split_variants(t, os.path.join(snp_dir, "nucmer", "%s.maskrepeat.%s.vcf" % (mix, kind)), kind, bgz=True, tbi="if-sorted")
    cmp_callers = [c for c in FP_COMPARED if c in callers]

    def write_tables(jobs):   # the tables of the rows and of every pass of the run: the same on one GPU and on several
        os.makedirs(tables, exist_ok=True)
        _flag_truth_rows(jobs)
        write_caller_performance(os.path.join(tables, "caller_performance.tsv"), [(c, s, j.stats) for (c, s), j in zip(meta, jobs)])
        _write_snp_rocs(meta, jobs, snp_dir)
        _write_tables(passes, par, run, jobs)
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


# ---- The passes of a run: one entry per pass, keyed by its name in passes.PASSES (whose flag the messages quote) ----------------
# keys      the run keywords that belong to the pass
# custom    run_vareval has it too.  Where the two workflows differ the parts below branch on run.custom: the table names
#           snpcall_benchmark_*.txt, custom=True, one genome in place of one per mix, the one group "custom" / "vareval" and the
#           "N labels ... no table is written" notes
# asks      kw -> whether the keywords ask for the pass: what passes.check_shared_call is told
# params    kw -> the checked, normalised value the other parts take (p), None when the pass is off; WorkflowError in the CLI's
#           words for a parameter without its pass, a pass without --alleles, a value out of range
# genome    (keyword, what to call it): the keyword holds the pass's FASTA -- {"TM": .., "TA": ..}, for vareval one path --, checked
#           for every mix of the run once the samples are known
# takes     VCF path -> whether a job of that sample takes part: every one, all but `-1-0`, or the mixed samples only
# plan      (run, p) -> p: vareval's one group of labels, before a line is printed; None takes the pass out of the run
# dry       (run, p): the lines --dryrun prints;   write  (run, p): its tables and files after the run
# ready     (run, p) -> p: what needs the run's truth files or callers, before the jobs are made
# onto_job  (run, job, name, sample, p) -> {Job field: value} for one job that takes part
# `run` is the driver's namespace: custom, kw, names (callers or labels), units [(name, sample, vcf)] and meta [(name, sample)] in job
# order, mixes, mixed, snp_dir, tables, truth_files, one_group and, after the run, jobs.
FLAG = {p.name: p.flag for p in PASSES}
_every = lambda vcf: True
_but_first_pure = lambda vcf: not os.path.basename(vcf).split(".")[0].endswith("-1-0")
_mixed = lambda vcf: not is_pure_strain(vcf)
_wf = namedtuple("WfPass", "name keys asks params dry onto_job write custom genome takes plan ready", defaults=(False, None, _mixed, None, None))
_given = lambda key: lambda kw: kw[key] is not None
_true = lambda key: lambda kw: bool(kw[key])
_said = lambda edges: ",".join(str(e) for e in edges)


def _allele_pass(name, asks, why, value):
    """params of a pass that only the allele-extended mode has: None unless asked for, then value(kw), or why it needs --alleles"""
    def params(kw):
        if not asks(kw):
            return None
        if not kw["alleles"]:
            raise WorkflowError("%s needs --alleles: %s" % (FLAG[name], why))
        return value(kw)
    return params


def _checked_as(says, check, *args):
    """check(*args), its ValueError said as a WorkflowError that names the option"""
    try:
        return check(*args)
    except ValueError as e:
        raise WorkflowError("%s: %s" % (says, e)) from None


def _own_params(asks, given, goes_with, says, check):
    """params of a pass with parameter keywords of its own (`given`): one of them without the pass is told what it goes with"""
    def params(kw):
        if asks(kw):
            return _checked_as(says, check, *(kw[k] for k in given))
        if any(kw[k] is not None for k in given):
            raise WorkflowError(goes_with)
    return params


# the checked --hap-gap of the haplotype pass and of the ladders that run it; the checked size edges (True or None: the default ones,
# the CLI's `1,2,6`, or a list)
_gap = lambda kw: _checked_as("--hap-gap", check_gap, kw["hap_gap"])
_edges = lambda bins: _checked_as("--type-bins", lambda: check_edges(None) if bins is True else parse_edges(bins) if isinstance(bins, str) else check_edges(bins))


# a per-job file of a pass, <caller dir>/<sub>/<vcf stem><ext>, and the rows the writers take: (caller, sample, stats) or (.., job)
_beside = lambda j, sub, ext: os.path.join(j.outdir, sub, os.path.basename(j.vcf_file)[:-4] + ext)
_stat_rows = lambda run: [(c, None if run.custom else s, j.stats) for (c, s), j in zip(run.meta, run.jobs)]
_job_rows = lambda run, takes=_every: [(c, s, j) for (c, s), j in zip(run.meta, run.jobs) if takes(j.vcf_file)]


def _say_units(run, takes, what, *more):
    """one dry-run line per job that takes part: what, caller, sample (vareval: what, label), then `more`"""
    for c, s, v in run.units:
        if takes(v):
            print("\t".join([what, c] + ([] if run.custom else [s]) + [str(m) for m in more]))


# dry: one line per mix and caller; dry: <table>, the callers, then the params as `fmt` says them
_say_mixes = lambda what: lambda run, p: [print("%s\t%s\t%s" % (what, mix, c)) for mix in run.mixes for c in run.names]
_say_table = lambda table, fmt="", say=lambda p: (): lambda run, p: print(("%s\t%s" + fmt) % ((table, ",".join(run.names)) + tuple(say(p))))


def _performance(module, writer, table, extra=lambda p: ()):
    """write: final_tables/<table> by <module>.<writer> from (caller, sample, stats), then what `extra` takes of the params"""
    def write(run, p):
        from importlib import import_module
        getattr(import_module("." + module, __package__), writer)(os.path.join(run.tables, table), _stat_rows(run), *extra(p))
    return write


# ladder_by_type: {"TM": FASTA, "TA": FASTA}, with hap_gap and ladder_type_bins (the size edges as for by_type; None: the default
# ones) (quasimodo_amd.laddertypes), in place of match_ladder and by_type, both of which the run's call makes itself
# behind all four rescues: final_tables/caller_performance_ladder_types.tsv (per caller and mixture one row per type and size bin
# -- records typed as spelled --, a marginal per type, the four rows behind the grid as plain counts, each with TP, FP, FN,
# Precision, Recall, F1 by spelling and after each tier; then a pooled block per caller).
_laddertypes_on = _allele_pass("laddertypes", _given("ladder_by_type"), "it crosses the variant types with the matching by normal form, by atoms and "
                               "by haplotype, which only the allele-extended mode has", lambda kw: (_gap(kw), _edges(kw["ladder_type_bins"])))


def _laddertypes_params(kw):
    if kw["ladder_by_type"] is None and kw["ladder_type_bins"] is not None:
        raise WorkflowError("ladder_type_bins needs ladder_by_type (--type-bins needs %s or %s)" % (FLAG["vartype"], FLAG["laddertypes"]))
    return _laddertypes_on(kw)


LADDERTYPES = _wf(
    "laddertypes", ("ladder_by_type", "ladder_type_bins"), _given("ladder_by_type"), _laddertypes_params,
    _say_table("caller_performance_ladder_types.tsv", "\t%d\t%s", lambda p: (p[0], _said(p[1]))),
    lambda run, j, c, s, p: dict(ladder_types=p, ladder_types_genome=run.kw["ladder_by_type"][s[:2]]),
    _performance("laddertypes", "write_performance_ladder_types", "caller_performance_ladder_types.tsv", lambda p: (p[1],)),
    genome=("ladder_by_type", "ladder by type"))

# match_ladder: {"TM": FASTA, "TA": FASTA}, with hap_gap (quasimodo_amd.ladder), in place of normalize, atomize,
# haplotypes and hap_subsets, which the run's call makes itself, all four: final_tables/caller_performance_ladder.tsv (TP, FP, FN,
# Precision, Recall, F1 by spelling and after normal form, atoms, haplotype and subset, cumulative, then the 15 non-empty method
# sets of lines and of entries; per caller and mixture, then pooled per caller) and
# callers/{caller}/ladder/{sample}.{ref}.{caller}.ladder.tsv for every mixed sample (every kept line that is no TP by spelling and
# every truth entry no kept record spells, with its method set and tier).
LADDER = _wf(
    "ladder", ("match_ladder",), _given("match_ladder"),
    _allele_pass("ladder", _given("match_ladder"), "it combines the matching by normal form, by atoms and by haplotype, which only the allele-extended mode has", _gap),
    _say_table("caller_performance_ladder.tsv", "\t%d", lambda p: (p,)),
    lambda run, j, c, s, p: dict(ladder=p, ladder_genome=run.kw["match_ladder"][s[:2]], ladder_out=_beside(j, "ladder", ".ladder.tsv")),
    _performance("ladder", "write_performance_ladder", "caller_performance_ladder.tsv"), genome=("match_ladder", "match ladder"))

# rescue_roc: {"TM": FASTA, "TA": FASTA} (quasimodo_amd.rescueroc), in place of normalize and atomize, which the
# run's call makes itself: the QUAL ROC by spelling, by normal form and by atoms side by side,
# snp/qmvt_roc/{caller}/{sample}.{ref}.rescue/spelling_roc.tsv.gz, normalized_roc.tsv.gz and atomized_roc.tsv.gz for every mixed
# sample, and final_tables/caller_roc_rescue.tsv (TP, FP, FN, Precision, Recall, F1 at QUAL >= 20 and at the threshold of the
# largest F1, per caller, mixture and matching, then pooled).
RESCUEROC = _wf(
    "rescueroc", ("rescue_roc",), _given("rescue_roc"),
    _allele_pass("rescueroc", _given("rescue_roc"), "it sweeps the matching by normal form and by atoms, which only the allele-extended mode has",
                 lambda kw: kw["rescue_roc"]),
    lambda run, p: (_say_units(run, _mixed, "rescue_roc"), print("caller_roc_rescue.tsv\t%s" % ",".join(run.names))),
    lambda run, j, c, s, p: dict(rescue_roc=p[s[:2]]),
    lambda run, p: _write_rescue_rocs(run.meta, run.jobs, run.snp_dir, run.tables), genome=("rescue_roc", "rescue ROC"))


# haplotypes: {"TM": FASTA, "TA": FASTA}, with hap_gap (default 10, 0 to 32; quasimodo_amd.haplo): the unmatched
# lines and the unmatched truth entries of every small region are replayed onto the genome and rescued where the two sequences are
# equal; final_tables/caller_performance_haplotype.tsv (TP, FP, FN, Precision, Recall, F1 by spelling and by haplotype side by
# side, then the class counts) and callers/{caller}/hap/{sample}.{ref}.{caller}.sites.tsv for every mixed sample.
# The entry also answers for the keywords that want a haplotype pass and find none: hap_subsets, then hap_gap (which the two
# ladders take as well).
_haplo_on = _allele_pass("haplo", _given("haplotypes"), "haplotypes are replayed from indels, MNPs and complex records, which only the allele-extended mode reads", _gap)


def _haplo_params(kw):
    if kw["haplotypes"] is None and kw["hap_subsets"]:
        raise WorkflowError("%s searches the sites of the haplotype pass: it needs %s (and the genomes)" % (FLAG["hapsub"], FLAG["haplo"]))
    if kw["haplotypes"] is None and kw["hap_gap"] is not None and kw["match_ladder"] is None and kw["ladder_by_type"] is None:
        raise WorkflowError("--hap-gap needs %s or %s" % (FLAG["haplo"], FLAG["ladder"]))
    return _haplo_on(kw)


HAPLO = _wf(
    "haplo", ("haplotypes", "hap_gap"), lambda kw: kw["haplotypes"] is not None and not kw["hap_subsets"], _haplo_params,
    _say_table("caller_performance_haplotype.tsv", "\t%d", lambda p: (p,)),
    lambda run, j, c, s, p: dict(haplo=p, haplo_genome=run.kw["haplotypes"][s[:2]], sites_out=_beside(j, "hap", ".sites.tsv")),
    _performance("haplo", "write_performance_haplotype", "caller_performance_haplotype.tsv"), genome=("haplotypes", "haplotypes"))

# hap_subsets (with haplotypes, behind whose pass it runs; in the shared-call rule it stands in place of haplo, and on the Job it
# takes the gap over from Job.haplo): the regions that did not match are searched for the largest pair of subsets whose replayed
# sequences are equal: final_tables/caller_performance_hapsubsets.tsv and
# callers/{caller}/hap/{sample}.{ref}.{caller}.subsets.tsv beside the above.
HAPSUB = _wf(
    "hapsub", ("hap_subsets",), _true("hap_subsets"), lambda kw: _gap(kw) if kw["hap_subsets"] else None,
    _say_table("caller_performance_hapsubsets.tsv", "\t%d", lambda p: (p,)),
    lambda run, j, c, s, p: dict(haplo=None, hapsub=p, subsets_out=_beside(j, "hap", ".subsets.tsv")),
    _performance("haplo", "write_performance_hapsubsets", "caller_performance_hapsubsets.tsv"))

# by_type: True, or the size edges as a list or as the CLI's `1,2,6` (quasimodo_amd.vartype): TP, FP and FN by
# variant type and size are counted behind the classification and final_tables/caller_performance_types.tsv is written (per caller
# x mixed sample one row per type and size bin, a marginal per type, the four rows behind the grid, then a pooled block per caller).
_by_type = lambda kw: kw["by_type"] is not None and kw["by_type"] is not False
VARTYPE = _wf(
    "vartype", ("by_type",), _by_type,
    _allele_pass("vartype", _by_type, "indels, MNPs and complex records are typed, which only the allele-extended mode reads", lambda kw: _edges(kw["by_type"])),
    _say_table("caller_performance_types.tsv", "\t%s", lambda p: (_said(p),)), lambda run, j, c, s, p: dict(vartype=p),
    _performance("vartype", "write_performance_types", "caller_performance_types.tsv", lambda p: (p,)))

# normalize: {"TM": FASTA, "TA": FASTA} (quasimodo_amd.normalize): indels and MNPs are also matched by normal form
# behind the classification; final_tables/caller_performance_normalized.tsv (TP, FP, FN, Precision, Recall, F1 by spelling and by
# normal form side by side, the rescued, respelled and reason counts) and callers/{caller}/norm/{sample}.{ref}.{caller}.rescued.tsv
# for every mixed sample.
NORMALIZE = _wf(
    "normalize", ("normalize",), _given("normalize"),
    _allele_pass("normalize", _given("normalize"), "the normal form is taken of indels and MNPs, which only the allele-extended mode reads", lambda kw: kw["normalize"]),
    _say_table("caller_performance_normalized.tsv"), lambda run, j, c, s, p: dict(normalize=p[s[:2]], rescued_out=_beside(j, "norm", ".rescued.tsv")),
    _performance("normalize", "write_performance_normalized", "caller_performance_normalized.tsv"), genome=("normalize", "normalize"))

# atomize: MNPs are also matched against adjacent SNVs, atom by atom (quasimodo_amd.atomize):
# final_tables/caller_performance_atomized.tsv (TP, FP, FN, Precision, Recall, F1 by spelling and by atoms side by side, the
# rescued, multi-atom, partial and reason counts) and callers/{caller}/atoms/{sample}.{ref}.{caller}.atoms.tsv for every mixed sample.
ATOMIZE = _wf(
    "atomize", ("atomize",), _true("atomize"),
    _allele_pass("atomize", _true("atomize"), "atoms are taken of MNPs, which only the allele-extended mode reads", lambda kw: True),
    _say_table("caller_performance_atomized.tsv"), lambda run, j, c, s, p: dict(atomize=True, atoms_out=_beside(j, "atoms", ".atoms.tsv")),
    _performance("atomize", "write_performance_atomized", "caller_performance_atomized.tsv"))


# explain_errors: why the FP lines are FP and the missed truth keys missed (quasimodo_amd.nearmiss), with
# explain_radius (default 10, 0 to 64): callers/{caller}/why/{sample}.{ref}.{caller}.fp.why.tsv and ...fn.why.tsv for every mixed
# sample (vareval: callers/why/{label}.fp.why.tsv and {label}.fn.why.tsv for every VCF), and final_tables/caller_error_classes.tsv.
_nearmiss_params = _own_params(_true("explain_errors"), ("explain_radius",), "--explain-radius goes with %s" % FLAG["nearmiss"], "--explain-radius",
                               lambda radius: check_radius(DEFAULT_RADIUS if radius is None else radius))


def _nearmiss_onto_job(run, j, c, s, p):
    from .extract import _paths
    from .nearmiss import fn_why_path, fp_why_path
    _paths(j)
    return dict(explain=p, fp_why_out=fp_why_path(j), fn_why_out=fn_why_path(j))


NEARMISS = _wf(
    "nearmiss", ("explain_errors", "explain_radius"), _true("explain_errors"), _nearmiss_params,
    lambda run, p: (_say_units(run, _every if run.custom else _mixed, "explain_errors", p), print("caller_error_classes\t%s" % ",".join(run.names))),
    _nearmiss_onto_job, lambda run, p: _write_error_classes(_job_rows(run, _every if run.custom else _mixed), run.tables), custom=True)


# filter_surface: TP, FP and FN under every filter QUAL >= q and AF >= a (quasimodo_amd.surface), with
# surface_qual_step / surface_qual_bins / surface_af_bins (default 4, 64, 50; QUAL 20 must be a grid line):
# callers/{caller}/surface/{sample}.{ref}.{caller}.surface.tsv for every mixed sample (vareval: callers/surface/{label}.surface.tsv
# for every VCF) and final_tables/caller_best_filter.tsv.
_surface_params = _own_params(_true("filter_surface"), ("surface_qual_step", "surface_qual_bins", "surface_af_bins"),
                              "--surface-qual-step, --surface-qual-bins and --surface-af-bins go with %s" % FLAG["surface"], FLAG["surface"], workflow_params)
SURFACE = _wf(
    "surface", ("filter_surface", "surface_qual_step", "surface_qual_bins", "surface_af_bins"), _true("filter_surface"), _surface_params,
    lambda run, p: (_say_units(run, _mixed, "filter_surface", *p), print("caller_best_filter\t%s" % ",".join(run.names))),
    lambda run, j, c, s, p: dict(surface=p),
    lambda run, p: _write_surface(_job_rows(run, _every if run.custom else _mixed), run.tables, p[0]), custom=True)


# seq_context: {"TM": FASTA, "TA": FASTA} (vareval: the FASTA of the genome the VCFs were called against, the first reference: the
# POS of the genome-difference table are its coordinates), with context_window / context_gc_bins (default 50, 10;
# quasimodo_amd.context): the counts per homopolymer x GC cell are taken behind the classification and
# final_tables/caller_performance_context.tsv (vareval: snpcall_benchmark_context.txt) is written (per caller x sample the cells in
# use, the marginals, none, nokey).
_context_params = _own_params(_given("seq_context"), ("context_window", "context_gc_bins"), "--context-window and --context-gc-bins go with %s" % FLAG["context"],
                              FLAG["context"], lambda window, gc_bins: check_params(DEFAULT_HALF_WINDOW if window is None else window, DEFAULT_GC_BINS if gc_bins is None else gc_bins))
_context_table = lambda run: "snpcall_benchmark_context.txt" if run.custom else "caller_performance_context.tsv"
CONTEXT = _wf(
    "context", ("seq_context", "context_window", "context_gc_bins"), _given("seq_context"), _context_params,
    lambda run, p: print("%s\t%d\t%d" % ((_context_table(run),) + p)),
    lambda run, j, c, s, p: dict(context=p, context_genome=run.kw["seq_context"] if run.custom else run.kw["seq_context"][s[:2]]),
    lambda run, p: _write_context(os.path.join(run.tables, _context_table(run)), [(c, None if run.custom else s, j) for c, s, j in _job_rows(run)], p, custom=run.custom),
    custom=True, genome=("seq_context", "sequence context"), takes=_every)


# votes: k-of-n caller consensus (quasimodo_amd.consensus): all callers of the run form one vote group per mixed
# sample (vareval: the labels form the one group "custom"; more than 32, or pure-strain names, are told so and get no table);
# final_tables/caller_consensus.tsv (TP, FP, FN, Precision, Recall, F1 of "at least k of n callers") and caller_private.tsv (what
# each caller alone calls).  consensus_vcf=K (implies votes) also writes snp/consensus/{sample}.{ref}.k{K}.vcf (vareval:
# custom.k{K}.vcf); K above the sample's caller count (the label count) is a WorkflowError that names the sample.  p: {"k": K or None}
_votes_asks = lambda kw: bool(kw["votes"]) or kw["consensus_vcf"] is not None


def _votes_params(kw):
    k = kw["consensus_vcf"]
    if k is not None and int(k) < 1:
        raise WorkflowError("--consensus-vcf %d: the level is at least 1" % int(k))
    return {"k": None if k is None else int(k)} if _votes_asks(kw) else None


def _votes_plan(run, p):
    from .consensus import MAX_GROUP
    if not run.custom:
        return p
    if len(run.names) > MAX_GROUP or not all(_mixed(v) for _, _, v in run.units):
        print("votes: %d labels (or pure-strain names): a vote group holds 1 to %d mixed samples, no table is written" % (len(run.names), MAX_GROUP))
        return None
    if p["k"] is not None and p["k"] > len(run.names):
        raise WorkflowError("sample custom: --consensus-vcf %d, but there are %d labels" % (p["k"], len(run.names)))
    run.one_group = True
    return p


def _votes_ready(run, p):
    if not run.custom:
        _vote_plan([(s, c, v) for c, s, v in run.units], p["k"])
    return p


def _votes_dry(run, p):
    _votes_ready(run, p)
    print("caller_consensus\t%s" % ",".join(run.names))
    for s in (["custom"] if run.custom else run.mixed) if p["k"] is not None else ():
        print("consensus_vcf\t%s\t%d" % (s, p["k"]))


def _votes_onto_job(run, j, c, s, p):
    if p["k"] is None:
        return dict(vote_group=s)
    name = "custom" if run.custom else "%s.%s" % (s, SAMPLE_REF[s])
    return dict(vote_group=s, consensus_k=p["k"], consensus_out=os.path.join(run.snp_dir, "consensus", "%s.k%d.vcf" % (name, p["k"])))


VOTES = _wf("votes", ("votes", "consensus_vcf"), _votes_asks, _votes_params, _votes_dry, _votes_onto_job,
            lambda run, p: _write_votes(run.meta, run.jobs, run.tables, ["custom"] if run.custom else run.mixed),
            custom=True, plan=_votes_plan, ready=_votes_ready)


# strata: a list of (name, starts, ends) BED strata (quasimodo_amd.strata): the counts per stratum are taken behind
# the classification and final_tables/caller_performance_strata.tsv (vareval: snpcall_benchmark_strata.txt) is written (per caller
# x sample one row per stratum, then outside, then nokey).
def _strata_write(run, p):
    if not run.custom:
        return _write_strata(run.meta, run.jobs, run.tables, p)
    from .strata import write_performance_strata
    _strata_genomediff(run.jobs, p)
    write_performance_strata(os.path.join(run.tables, "snpcall_benchmark_strata.txt"), [(c, s, [x[0] for x in p], st) for c, s, st in _stat_rows(run)], custom=True)


STRATA = _wf("strata", ("strata",), _given("strata"), lambda kw: None if kw["strata"] is None else _checked_as("strata", freeze, kw["strata"]),
             lambda run, p: None if run.custom else print("caller_performance_strata\t%s" % ",".join(s[0] for s in p)),
             lambda run, j, c, s, p: dict(strata=p), _strata_write, custom=True, takes=_every)


# snp_profile: True or {"window", "n_pos_bins", "n_af_bins"} (the rule's first output): the profile pass runs behind
# the classification; final_tables/{mix}.{caller}.snp.profile.tsv and ...snp.profile.afsweep.tsv are written for every caller and
# mix (`-1-0` left out, `-0-1` as FP only) and callers/{caller}/profile/{sample}.{ref}.{caller}.points.tsv for every profiled sample.
def _profile_params(kw):
    if not kw["snp_profile"]:
        return None
    from .afprofile import DEFAULTS
    opts = dict(DEFAULTS)
    opts.update({k: int(v) for k, v in (kw["snp_profile"].items() if isinstance(kw["snp_profile"], dict) else ()) if v is not None})
    prof = (opts["window"], opts["n_pos_bins"], opts["n_af_bins"])
    if not (1 <= prof[0] < (1 << 28) and prof[1] >= 1 and prof[2] >= 1 and prof[1] * prof[2] <= 8192):
        raise WorkflowError("snp profile: window %d, %d x %d bins (1 <= window < 2^28, at most 8192 cells)" % (prof[0], prof[2], prof[1]))
    return prof


PROFILE = _wf("profile", ("snp_profile",), _true("snp_profile"), _profile_params, _say_mixes("snp_profile"),
              lambda run, j, c, s, p: dict(profile=p, points_out=_beside(j, "profile", ".points.tsv")),
              lambda run, p: _write_snp_profile(run.meta, run.jobs, run.tables, run.names, run.mixes, p[0]), takes=_but_first_pure)


# bootstrap: a replicate count or {"n_rep", "window", "n_win", "seed"} (quasimodo_amd.bootstrap): the window counts
# and the replicates are taken behind the classification; final_tables/caller_performance_ci.tsv (percentile intervals of Precision,
# Recall and F1 per caller x sample; vareval: snpcall_benchmark_ci.txt) and, hcmv only, caller_performance_ci_pairs.tsv (the F1
# difference of every pair of callers on a mixed sample, over the shared draws).  n_win is raised to cover the truth files' largest
# POS, which is why the (window, n_win, n_rep, seed) of the jobs are made once the truth files are in place (ready).
def _boot_write(run, p):
    if not run.custom:
        return _write_bootstrap(run.meta, run.jobs, run.tables)
    from .bootstrap import write_performance_ci
    _boot_extra(run.jobs)
    write_performance_ci(os.path.join(run.tables, "snpcall_benchmark_ci.txt"), _stat_rows(run), custom=True)


BOOT = _wf("boot", ("bootstrap",), _given("bootstrap"), lambda kw: kw["bootstrap"],
           lambda run, p: None if run.custom else print("caller_performance_ci\t%d" % _boot_params(p, [])[2]),
           lambda run, j, c, s, p: dict(boot=p), _boot_write, custom=True, takes=_every, ready=lambda run, p: _boot_params(p, run.truth_files))

# mutation_context: {"TM": FASTA, "TA": FASTA} (rules/mutationcontext.smk): the motif pass runs behind the classification and
# final_tables/{mix}.{caller}.mutationcontext.tsv is written for every caller and every mix that has samples.
MOTIFS = _wf("motifs", ("mutation_context",), _given("mutation_context"), lambda kw: kw["mutation_context"], _say_mixes("mutationcontext"),
             lambda run, j, c, s, p: dict(genome=p.get(s[:2])),
             lambda run, p: _write_mutation_context(run.meta, run.jobs, run.tables, run.names, run.mixes),
             genome=("mutation_context", "mutation context"), takes=_but_first_pure)


# truth_side: the truth set's side of the join: callers/{caller}/fn/{sample}.{ref}.{caller}.fn.vcf for every mixed
# sample, nucmer/{sample}.missed_by_all.vcf over the Venn callers (rules/vis_eval_vcf.smk:2, those of the run) and
# final_tables/caller_snp_venn.tsv.  vareval: callers/fn/{label}.fn.vcf for every VCF; up to five labels form one group (one rank)
# and the Venn table is written, more are told so and get their FN files only.  p: the Venn callers; vareval: {"grouped": bool}
def _truthside_dry(run, p):
    from .truthside import MAX_GROUP, venn_callers
    _say_units(run, _every if run.custom else _mixed, "truthside_fn")
    vc = venn_callers(run.names) if not run.custom else run.names if len(run.names) <= MAX_GROUP else []
    for s in run.mixed if vc and not run.custom else ():
        print("missed_by_all\t%s\t%s" % (s, ",".join(vc)))
    if vc:
        print("caller_snp_venn\t%s" % ",".join(vc))


def _truthside_ready(run, p):
    from .truthside import MAX_GROUP, venn_callers
    if not run.custom:
        return venn_callers(run.names)
    grouped = len(run.names) <= MAX_GROUP and all(_mixed(v) for _, _, v in run.units)
    if not grouped:
        print("truth side: %d labels (or pure-strain names): the Venn regions are skipped, FN files are still written" % len(run.names))
    run.one_group = run.one_group or grouped
    return {"grouped": grouped}


def _truthside_onto_job(run, j, c, s, p):
    from .extract import _paths, fn_path
    _paths(j)
    if run.custom:
        return dict(fn_out=fn_path(j), group="vareval" if p["grouped"] else None)
    return dict(fn_out=fn_path(j), **(dict(group=s, missed_out=os.path.join(run.snp_dir, "nucmer", "%s.missed_by_all.vcf" % s)) if c in p else {}))


def _truthside_write(run, p):
    if not run.custom:
        return _write_caller_snp_venn(run.meta, run.jobs, run.tables, run.names, run.mixed)
    if p["grouped"]:
        from .truthside import write_caller_snp_venn
        n, st = len(run.names), run.jobs[0].stats
        write_caller_snp_venn(os.path.join(run.tables, "caller_snp_venn.tsv"), {"custom": (list(st["truth_regions"][:1 << n]), list(st["fp_regions"][:1 << n]))}, run.names)


TRUTHSIDE = _wf("truthside", ("truth_side",), _true("truth_side"), lambda kw: True if kw["truth_side"] else None, _truthside_dry,
                _truthside_onto_job, _truthside_write, custom=True, ready=_truthside_ready)

# The rows stand in the order their params speak: where two keywords are wrong at once, the earlier row's message is the one said.
# That is not the order of passes.PASSES; the dry-run lines and the tables have an order each of their own as well, so that a run's
# text and, where two passes share a call, its files come out as they always have.  The jobs are set up in row order: hapsub after haplo.
WORKFLOW_PASSES = (LADDERTYPES, LADDER, RESCUEROC, HAPLO, HAPSUB, VARTYPE, NORMALIZE, ATOMIZE, NEARMISS, SURFACE, CONTEXT, VOTES, STRATA,
                   PROFILE, BOOT, MOTIFS, TRUTHSIDE)
DRY_ORDER = ("haplo", "hapsub", "normalize", "atomize", "rescueroc", "ladder", "laddertypes", "vartype", "motifs", "profile", "strata", "boot",
             "context", "votes", "nearmiss", "surface", "truthside")
WRITE_ORDER = ("motifs", "profile", "strata", "boot", "truthside", "votes", "nearmiss", "context", "surface", "normalize", "haplo", "hapsub",
               "atomize", "rescueroc", "ladder", "laddertypes", "vartype")


def _checked(passes, kw):
    """{name: params} of the passes the keywords ask for, in row order, once they may share the run's one call
    (passes.check_shared_call, said with the CLI's names) and every parameter is in range"""
    try:
        check_shared_call({p.name for p in passes if p.asks(kw)})
    except SharedCallError as e:
        raise WorkflowError(e.for_cli()) from None
    par = {p.name: p.params(kw) for p in passes}
    return {name: v for name, v in par.items() if v is not None}


def _check_genomes(passes, par, run):
    """the FASTA of every pass of the run that takes one: a file, for every mix of the run"""
    for key, what in (p.genome for p in passes if p.name in par and p.genome):
        if run.custom and not os.path.isfile(run.kw[key]):
            raise WorkflowError("%s: no genome FASTA (%s)" % (what, run.kw[key]))
        for mix in () if run.custom else run.mixes:
            if not run.kw[key].get(mix) or not os.path.isfile(run.kw[key].get(mix)):
                raise WorkflowError("%s: no genome FASTA for %s (%s)" % (what, mix, run.kw[key].get(mix)))


def _each(passes, par, hook, run, order=None):
    """one optional part of every pass that is on, in row order or in `order`; plan and ready hand the params on (None: the pass
    leaves the run)"""
    for p in passes if order is None else [q for name in order for q in passes if q.name == name]:
        if p.name in par and getattr(p, hook) is not None:
            got = getattr(p, hook)(run, par[p.name])
            if hook in ("plan", "ready"):
                par[p.name] = got
                if got is None:
                    del par[p.name]


def _onto_jobs(passes, par, run, jobs):
    for p in passes:
        for (c, s, _), j in zip(run.units, jobs) if p.name in par else ():
            for field, value in p.onto_job(run, j, c, s, par[p.name]).items() if p.takes(j.vcf_file) else ():
                setattr(j, field, value)


def _write_tables(passes, par, run, jobs):
    """the tables of every pass of the run: the same on one GPU and on several"""
    run.jobs = jobs
    _each(passes, par, "write", run, WRITE_ORDER)


def run_vareval(vcfs, snps_file, outpath, labels=None, engine=None, dryrun=False, gpus=None, _body=None, _backend="nccl", _same_device=False,
                truth_side=False, strata=None, bootstrap=None, votes=False, consensus_vcf=None, explain_errors=False, explain_radius=None,
                filter_surface=False, surface_qual_step=None, surface_qual_bins=None, surface_af_bins=None, seq_context=None,
                context_window=None, context_gc_bins=None):
    """eval_variant_custom.smk with the genome difference (show-snps -CTHIlr TSV) already computed.
    gpus > 1: the VCFs are dealt to that many GPUs (one process each); the rows come back for the table.
    Every other keyword belongs to one of the passes of WORKFLOW_PASSES that a custom run has (`custom`), which says what each
    takes and writes here; each of them runs alone (quasimodo_amd.passes; WorkflowError otherwise)."""
    kw = dict(locals(), alleles=False)
    passes = tuple(p for p in WORKFLOW_PASSES if p.custom)
    par = _checked(passes, kw)
    results = os.path.join(outpath.rstrip("/"), "results")
    call_dir = os.path.join(results, "snp", "callers")
    run = SimpleNamespace(custom=True, kw=kw, snp_dir=os.path.join(results, "snp"), tables=os.path.join(results, "final_tables"), one_group=False)
    _check_genomes(passes, par, run)
    labels = list(labels) if labels else [os.path.splitext(os.path.basename(v))[0] for v in vcfs]
    if len(labels) != len(vcfs):
        raise WorkflowError("labels and vcfs differ in length")
    run.names, run.units, run.meta = labels, [(lab, "custom", v) for lab, v in zip(labels, vcfs)], [(lab, "custom") for lab in labels]
    _each(passes, par, "plan", run)
    if dryrun:
        for lab, v in zip(labels, vcfs):
            print("extract_TP\t%s\t%s" % (lab, v))
        _each(passes, par, "dry", run, DRY_ORDER)
        return None
    if not os.path.exists(snps_file) or os.path.getsize(snps_file) == 0:
        raise WorkflowError("No difference between two genomes!")       # custom_snp_benchmark.R:19-21
    os.makedirs(os.path.join(call_dir, "fp"), exist_ok=True)
    run.truth_files = [(snps_file, "custom")]
    _each(passes, par, "ready", run)
    jobs = [Job(v, snps_file, "custom", call_dir, lab) for lab, v in zip(labels, vcfs)]
    _onto_jobs(passes, par, run, jobs)
    if gpus is not None and (int(gpus) > 1 or _body):
        if engine is not None:
            raise ValueError("gpus > 1 starts one process (and one engine) per GPU: do not pass an engine")
        from .multigpu import extract_many_sharded
        jobs, res = extract_many_sharded(jobs, int(gpus), backend=_backend, body=_body, same_device=_same_device,
                                         groups=[list(range(len(jobs)))] if run.one_group else None)
        run_vareval.last_result = res
    else:
        extract_many(jobs, engine=engine)
    os.makedirs(run.tables, exist_ok=True)
    _flag_truth_rows(jobs)
    write_snpcall_benchmark(os.path.join(run.tables, "snpcall_benchmark.txt"), [(lab, j.stats) for lab, j in zip(labels, jobs)])
    _write_tables(passes, par, run, jobs)
    return jobs


run_vareval.last_result = None
