"""Host mirror of the reference worker program/extract_TP_FP_SNPs.py.

Same function names and argument meaning as the reference
(extract_tp_fp_snp :12, extract_tp_fp_custom_snp :60); the shell pipeline is
replaced by one text scan on the host + the HIP engine.  `extract_many` is the
batch form used by the rule bodies: every mixed-sample VCF of a run is
classified in ONE engine batch (the qm_batch_* entry points; files are read, scanned and written by a thread pool).

Differences from the reference, all deliberate:
  * errors raise (the CLI exits non-zero) instead of being ignored;
  * outputs are written atomically and tp/ is complete before returning
    (the reference does not wait for its tp writer, :55-57);
  * fp/ and tp/ are created when missing (the reference relies on Snakemake for fp/).
"""
import os
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

from ._lib import SCALAR_NAMES, QmvtError
from .engine import Engine
from .passes import PASSES, check_alleles, check_shared_call, requested_by
from .vcfio import scan_vcf


def is_pure_strain(vcf_file):
    """extract_TP_FP_SNPs.py:33 -- sample name ends in -1-0 / -0-1: no truth comparison."""
    return os.path.basename(vcf_file).split(".")[0].endswith(("-1-0", "-0-1"))


def _hap_gap(j):
    """the gap of the job's haplotype pass, asked for as Job.haplo or -- with the subset search behind it -- as Job.hapsub"""
    return j.hapsub if j.hapsub is not None else j.haplo


@dataclass
class Job:
    vcf_file: str
    snp_file: str
    mode: str = "hcmv"        # "hcmv" | "custom"
    outdir: str = ""
    caller: str = ""
    # filled by extract_many
    filtered_out: str = ""
    tp_out: str = ""
    fp_out: str = ""
    stats: dict = field(default_factory=dict)
    genome: str = None        # FASTA of the sample's genome: the mutation-context spectra come back in stats["motifs"]
    # the truth-side view; mixed samples only
    fn_out: str = None        # where the missed-variant list goes (extract_many(fn=True) derives it)
    group: str = None         # label of the job's group (1 to 5 jobs of one truth file): stats gain truth_regions / fp_regions
    missed_out: str = None    # where the group's missed-by-all list goes (any member may carry it)
    # the allele-frequency profile
    profile: tuple = None     # (window, n_pos_bins, n_af_bins): stats gain af_grid / af_extra (the same for every profiled job of a call)
    points_out: str = None    # where the job's Position / Frequency / type table goes
    # counts per genome region
    strata: tuple = None      # ((name, starts, ends), ...): stats gain strata_rec / strata_tru (the same set for every such job of a call)
    # paired block-bootstrap replicates
    boot: tuple = None        # (window, n_win, n_rep, seed): stats gain boot_cnt / boot_rep (the same for every such job of a call)
    # k-of-n caller consensus; mixed samples only
    vote_group: str = None    # label of the job's vote group (1 to 32 jobs of one truth file): stats gain tp_votes / fp_votes / private_*
    consensus_k: int = 0      # the group's consensus level (any member may carry it, with consensus_out); 0 = no file
    consensus_out: str = None
    # why the FP lines are FP and the missed truth keys missed; mixed samples only
    explain: int = None       # the radius (0 to 64), None = off: stats gain nearmiss_rec / nearmiss_tru (the same radius for every such job of a call)
    fp_why_out: str = None    # where the job's `line POS REF ALT QUAL class` table goes (extract_many(explain=) derives it)
    fn_why_out: str = None    # where the job's `POS REF ALT class` table of its missed truth rows goes
    # the filter surface; mixed samples only
    surface: tuple = None     # (q_step, nq, na): stats gain surface / surface_extra / surface_params (the same for every swept job of a call)
    # sequence-context profiles
    context: tuple = None     # (half_window, n_gc): stats gain context_rec / context_tru / context_gen (the same for every profiled job of a call)
    context_genome: str = None   # FASTA of the genome the VCF was called against: its positions are what the cells are made of
    # indels and MNPs matched by normal form; mixed samples, allele-extended mode only
    normalize: str = None     # FASTA of the genome the VCF was called against: stats gain norm_rec / norm_tru
    rescued_out: str = None   # where the job's rescued-lines table goes (extract_many(normalize=) derives it)
    # MNPs matched against adjacent SNVs; mixed samples, allele-extended mode only
    atomize: bool = None      # True: stats gain atom_rec / atom_tru
    atoms_out: str = None     # where the job's multi-atom lines table goes (extract_many(atomize=) derives it)
    # the QUAL ROC under normal-form and atom matching; mixed samples, allele-extended mode only
    rescue_roc: str = None    # FASTA of the genome the VCF was called against, IN PLACE OF Job.normalize / Job.atomize: stats gain rroc_n / rroc_a / rroc_base
    # TP, FP and FN by variant type and size; mixed samples, allele-extended mode only
    vartype: tuple = None     # the size edges: stats gain type_rec / type_tru / type_edges (the same edges for every typed job of a call)
    # clusters of records matched by replayed haplotype; mixed samples, allele-extended mode only
    haplo: int = None         # the gap g (0 to 32): stats gain hap_rec / hap_tru / hap_gap (the same gap for every such job of a call)
    haplo_genome: str = None  # FASTA of the genome the VCF was called against (with Job.haplo)
    sites_out: str = None     # where the job's table of MATCH sites goes (extract_many(haplo=) derives it)
    # a subset search inside the sites the haplotype pass left MISMATCH or CONFLICT; with Job.haplo
    hapsub: int = None        # the gap g, IN PLACE OF Job.haplo: the pass and the search behind it; stats gain hap_sub ([8], haplo.SUB_COLS) too
    subsets_out: str = None   # where the job's table of PARTIAL sites goes (extract_many(hapsub=True) derives it)
    # the four rescues combined; mixed samples, allele-extended mode only
    ladder: int = None        # the gap g of the haplotype pass, IN PLACE OF Job.normalize / atomize / haplo / hapsub: stats gain ladder_rec / ladder_tru
    ladder_genome: str = None  # FASTA of the genome the VCF was called against (with Job.ladder)
    ladder_out: str = None    # where the job's table of lines and entries with their method sets goes (extract_many(ladder=) derives it)
    # the match ladder per variant type and size; mixed samples, allele-extended mode only
    ladder_types: tuple = None   # (gap, size edges), IN PLACE OF Job.ladder and Job.vartype: stats gain ladder_types_rec / ladder_types_tru / ladder_types_edges
    ladder_types_genome: str = None   # FASTA of the genome the VCF was called against (with Job.ladder_types)


def _paths(job):
    """Output paths exactly as the reference derives them (:19-22,39-41 hcmv; :71-72,91 custom)."""
    if job.mode == "hcmv":
        dirname = os.path.dirname(job.vcf_file)
        base = os.path.basename(job.vcf_file)[:-4]
        job.filtered_out = job.vcf_file[:-4] + ".filtered.vcf"
        job.fp_out = os.path.join(dirname, "fp", base + ".fp.vcf")
        job.tp_out = os.path.join(dirname, "tp", base + ".tp.vcf")
    elif job.mode == "custom":
        job.filtered_out = os.path.join(job.outdir, job.caller + ".filtered.vcf")
        job.fp_out = os.path.join(job.outdir, "fp", job.caller + ".fp.vcf")
        job.tp_out = os.path.join(job.outdir, "tp", job.caller + ".tp.vcf")
    else:
        raise ValueError("data must be 'hcmv' or 'custom', got %r" % job.mode)


def fn_path(job):
    """the missed-variant list beside fp/ and tp/: fn/<x>.fn.vcf"""
    d, base = os.path.split(job.fp_out)
    return os.path.join(os.path.dirname(d), "fn", base[:-len(".fp.vcf")] + ".fn.vcf")


def _strict_default():
    return os.environ.get("QM_LENIENT", "0") in ("", "0")


def _alleles_default():
    return os.environ.get("QM_ALLELES", "0") not in ("", "0")


def _label_groups(jobs, groups, field, prefix, max_members, what, two):
    """extract_many's `groups` (lists of job indices) as labels in Job.<field>"""
    for k, g in enumerate(groups):
        if not 1 <= len(g) <= max_members:
            raise ValueError("a %s group holds 1 to %d jobs, not %d" % (what, max_members, len(g)))
        for i in g:
            if getattr(jobs[i], field) not in (None, "%s%d" % (prefix, k)):
                raise ValueError("job %d sits in two %sgroups" % (i, two))
            setattr(jobs[i], field, "%s%d" % (prefix, k))


def _group_indices(jobs, pure, field, max_members, what):
    """The labels in Job.<field>, in job order, and per job the index of its label or -1: what the engine takes.  A group holds 1 to
    max_members mixed-sample jobs."""
    labels = []
    for j, p in zip(jobs, pure):
        lab = getattr(j, field)
        if lab is not None and p:
            raise ValueError("%s: a pure-strain sample cannot be in a %s group (its truth is never read)" % (j.vcf_file, what))
        if lab is not None and lab not in labels:
            labels.append(lab)
    for lab in labels:
        k = sum(getattr(j, field) == lab for j in jobs)
        if k > max_members:
            raise ValueError("%s group %r holds %d jobs (1 to %d)" % (what, lab, k, max_members))
    return labels, [-1 if getattr(j, field) is None else labels.index(getattr(j, field)) for j in jobs]


def _mixed(j):
    return not is_pure_strain(j.vcf_file)


def _per_job(xs, jobs, said):
    """a keyword's list, one entry per job"""
    xs = list(xs)
    if len(xs) != len(jobs):
        raise ValueError(said % (len(xs), len(jobs)))
    return xs


class _Loaded:
    """load(path of a FASTA) -> genome id: every distinct file is read and loaded once, and released with the strata set behind the
    call.  One dict keyed by the path serves every pass, because no two genome-taking passes share a call (check_shared_call).
    keep: the bases stay in .seqs (the haplotype pass writes its files from them).  Without an engine nothing is loaded: the call
    holds pure-strain samples only, which read no genome."""

    def __init__(self, engine):
        self.engine, self.ids, self.seqs, self.sid = engine, {}, {}, None

    def __call__(self, path, keep=False):
        if self.engine is not None and path not in self.ids:
            from .motifs import read_fasta
            seq = read_fasta(path)
            if keep:
                seq = self.seqs[path] = bytes(seq)
            self.ids[path] = self.engine.genome_load(seq)
        return self.ids.get(path, -1)

    def strata(self, frozen):
        self.sid = self.engine.strata_load(frozen)
        return self.sid

    def release(self):
        for gid in self.ids.values():
            self.engine.genome_release(gid)
        if self.sid is not None:
            self.engine.strata_release(self.sid)


# ---- the passes, each from its keyword to its Job fields to the dict Engine.extract_files takes ----------------
# name: the pass in quasimodo_amd.passes; key: Engine.extract_files' keyword for it.
# onto_jobs(jobs, **kw): called when the pass's keyword is given (kw: all of extract_many's).  Puts it onto the Job fields, the derived output paths included.
# spec(jobs, pure, load): the dict the engine takes, or None when no job asks; load: a _Loaded.  outs: the keys of that dict that hold output paths,
#   whose directories must exist.  on_pure: the pass runs on pure-strain samples too, so a call of those alone needs an engine for it.
# after(rows, jobs, spec, alleles): what the pass adds to the rows behind the call.
PassIO = namedtuple("PassIO", "name key onto_jobs spec outs on_pure after", defaults=((), False, None))


def _votes_onto_jobs(jobs, votes, groups, **kw):
    from .consensus import MAX_GROUP as VMAX
    if groups is None:
        raise ValueError("votes: groups (lists of job indices) are needed")
    opt = votes if isinstance(votes, dict) else {}
    ks, outs = list(opt.get("k") or [0] * len(groups)), list(opt.get("out") or [None] * len(groups))
    if len(ks) != len(groups) or len(outs) != len(groups):
        raise ValueError("votes: %d levels / %d files for %d groups" % (len(ks), len(outs), len(groups)))
    _label_groups(jobs, groups, "vote_group", "v", VMAX, "vote", "vote ")
    for k, g in enumerate(groups):
        if not 0 <= int(ks[k]) <= len(g):
            raise ValueError("vote group %d: consensus level %d with %d members" % (k, int(ks[k]), len(g)))
        for i in g:
            jobs[i].consensus_k, jobs[i].consensus_out = int(ks[k]), outs[k]


def _groups_onto_jobs(jobs, groups, votes, **kw):
    from .truthside import MAX_GROUP
    if groups is not None and not votes:   # (with votes= they are the vote groups)
        _label_groups(jobs, groups, "group", "g", MAX_GROUP, "truth-side", "")


def _votes_spec(jobs, pure, load):
    from .consensus import MAX_GROUP as VMAX
    if not any(j.vote_group is not None for j in jobs):
        return None
    labels, index = _group_indices(jobs, pure, "vote_group", VMAX, "vote")
    vt = {"group": index, "k": [], "out": []}
    for lab in labels:
        mem = [j for j in jobs if j.vote_group == lab]
        k = next((j.consensus_k for j in mem if j.consensus_k), 0)
        out = next((j.consensus_out for j in mem if j.consensus_out), None)
        if k > len(mem):
            raise ValueError("vote group %r: consensus level %d with %d members" % (lab, k, len(mem)))
        vt["k"].append(k if out else 0)
        vt["out"].append(out if k else None)
    return vt


def _votes_after(rows, jobs, spec, alleles):
    for r, j in zip(rows, jobs):
        if j.vote_group is not None:
            r["vote_callers"] = [m.caller for m in jobs if m.vote_group == j.vote_group]


def _fn_onto_jobs(jobs, fn, **kw):
    for j in jobs:
        if fn and j.fn_out is None and _mixed(j):
            _paths(j)
            j.fn_out = fn_path(j)


def _truthside_spec(jobs, pure, load):
    from .truthside import MAX_GROUP
    if not any((j.fn_out or j.group is not None) and not p for j, p in zip(jobs, pure)):
        return None
    labels, index = _group_indices(jobs, pure, "group", MAX_GROUP, "truth-side")
    missed = [next((j.missed_out for j in jobs if j.group == lab and j.missed_out), None) for lab in labels]
    return {"fn": [None if p else j.fn_out for j, p in zip(jobs, pure)], "group": index, "missed": missed}


def _explain_onto_jobs(jobs, explain, **kw):
    from .nearmiss import check_radius, fn_why_path, fp_why_path
    radius = check_radius(explain)
    for j in filter(_mixed, jobs):
        _paths(j)
        j.explain = radius
        j.fp_why_out, j.fn_why_out = j.fp_why_out or fp_why_path(j), j.fn_why_out or fn_why_path(j)


def _nearmiss_spec(jobs, pure, load):
    from .nearmiss import check_radius
    on = [j.explain is not None and not p for j, p in zip(jobs, pure)]
    return {"radius": check_radius(next(j.explain for j, w in zip(jobs, on) if w)), "want": [int(w) for w in on],
            "fp_why": [j.fp_why_out if w else None for j, w in zip(jobs, on)],
            "fn_why": [j.fn_why_out if w else None for j, w in zip(jobs, on)]} if any(on) else None


def _surface_onto_jobs(jobs, surface, **kw):
    from .surface import params
    spar = params(**(surface if isinstance(surface, dict) else {}))
    for j in filter(_mixed, jobs):
        j.surface = spar


def _surface_spec(jobs, pure, load):
    from .surface import params
    on = [j.surface is not None for j in jobs]
    return dict(zip(("q_step", "nq", "na"), params(*next(j.surface for j in jobs if j.surface is not None))), want=[int(w) for w in on]) if any(on) else None


def _context_onto_jobs(jobs, context, **kw):
    from .context import DEFAULT_GC_BINS, DEFAULT_HALF_WINDOW, check_params
    cpar = check_params(context.get("half_window", DEFAULT_HALF_WINDOW), context.get("n_gc", DEFAULT_GC_BINS))
    for j, g in zip(jobs, _per_job(context["genomes"], jobs, "context: %d genomes entries for %d jobs")):
        j.context, j.context_genome = (cpar, g) if g else (None, None)


def _context_spec(jobs, pure, load):
    from .context import check_params
    on = [j.context is not None for j in jobs]
    for j, w in zip(jobs, on):
        if w and not j.context_genome:
            raise ValueError("%s: Job.context without Job.context_genome (the FASTA the VCF was called against)" % j.vcf_file)
    return dict(zip(("half_window", "n_gc"), check_params(*next(j.context for j in jobs if j.context is not None))),
                genomes=[load(j.context_genome) if w else -1 for j, w in zip(jobs, on)]) if any(on) else None


def _normalize_onto_jobs(jobs, normalize, **kw):
    from .normalize import rescued_path
    for j, g in zip(jobs, _per_job(normalize["genomes"] if isinstance(normalize, dict) else normalize, jobs, "normalize: %d genomes entries for %d jobs")):
        j.normalize = g if g and _mixed(j) else None
        if j.normalize:
            _paths(j)
            j.rescued_out = j.rescued_out or rescued_path(j)


def _rescue_roc_onto_jobs(jobs, rescue_roc, **kw):
    for j, g in zip(jobs, _per_job(rescue_roc["genomes"] if isinstance(rescue_roc, dict) else rescue_roc, jobs, "rescue_roc: %d genomes entries for %d jobs")):
        j.rescue_roc = g if g and _mixed(j) else None


def _ladder_onto_jobs(jobs, ladder, **kw):
    """ladder= (the genomes, or the genomes and the gap): all four rescue passes and the ladder behind them, asked for in place of them"""
    from .haplo import check_gap
    from .ladder import ladder_path
    opt = ladder if isinstance(ladder, dict) else {"genomes": ladder}
    gap = check_gap(opt.get("gap"))
    for j, g in zip(jobs, _per_job(opt["genomes"], jobs, "ladder: %d genomes entries for %d jobs")):
        j.ladder, j.ladder_genome = (gap, g) if g and _mixed(j) else (None, None)
        if j.ladder is not None:
            _paths(j)
            j.ladder_out = j.ladder_out or ladder_path(j)


def _ladder_spec(jobs, pure, load):
    from .haplo import check_gap
    on = [j.ladder is not None for j in jobs]
    if not any(on):
        return None
    return {"gap": check_gap(next(j.ladder for j in jobs if j.ladder is not None)), "subsets": True,
            "genomes": [load(j.ladder_genome) if w else -1 for j, w in zip(jobs, on)], "want": [int(w) for w in on],
            "out": [j.ladder_out if w else None for j, w in zip(jobs, on)]}


def _ladder_types_onto_jobs(jobs, ladder_types, **kw):
    """ladder_types= {"genomes": ..., "gap": ..., "edges": ...}: the four rescue passes, the type pass, the ladder and their cross"""
    from .haplo import check_gap
    from .vartype import check_edges
    opt = ladder_types if isinstance(ladder_types, dict) else {"genomes": ladder_types}
    par = (check_gap(opt.get("gap")), check_edges(opt.get("edges")))
    for j, g in zip(jobs, _per_job(opt["genomes"], jobs, "ladder_types: %d genomes entries for %d jobs")):
        j.ladder_types, j.ladder_types_genome = (par, g) if g and _mixed(j) else (None, None)


def _ladder_types_spec(jobs, pure, load):
    from .haplo import check_gap
    from .vartype import check_edges
    on = [j.ladder_types is not None and not p for j, p in zip(jobs, pure)]
    if not any(on):
        return None
    gap, edges = next(j.ladder_types for j in jobs if j.ladder_types is not None)
    return {"gap": check_gap(gap), "edges": check_edges(edges), "subsets": True,
            "genomes": [load(j.ladder_types_genome) if w else -1 for j, w in zip(jobs, on)], "want": [int(w) for w in on]}


def _atomize_onto_jobs(jobs, atomize, **kw):
    from .atomize import atoms_path
    awant = [True] * len(jobs) if atomize is True else [bool(w) for w in atomize]
    for j, w in zip(jobs, _per_job(awant, jobs, "atomize: %d entries for %d jobs")):
        j.atomize = True if w and _mixed(j) else None
        if j.atomize:
            _paths(j)
            j.atoms_out = j.atoms_out or atoms_path(j)


def _vartype_onto_jobs(jobs, vartype, **kw):
    from .vartype import check_edges
    tedges = check_edges(None if vartype is True else vartype)
    for j in jobs:
        j.vartype = tedges if _mixed(j) else None


def _vartype_spec(jobs, pure, load):
    from .vartype import check_edges
    on = [j.vartype is not None and not p for j, p in zip(jobs, pure)]
    return {"edges": check_edges(next(j.vartype for j in jobs if j.vartype is not None)), "want": [int(w) for w in on]} if any(on) else None


def _haplo_onto_jobs(jobs, haplo, hapsub, **kw):
    """haplo= (the gap, or the gap and the genomes), and with hapsub=True the subset search behind the pass, asked for in place of it"""
    if hapsub and (haplo is None or haplo is False):
        raise ValueError("hapsub (--hap-subsets) searches the sites of the haplotype pass: it needs haplo= (the gap, or the gap and the genomes) in the same call")
    from .haplo import check_gap, sites_path, subsets_path
    hopt = haplo if isinstance(haplo, dict) else {"gap": None if haplo is True else haplo}
    hgap = check_gap(hopt.get("gap"))
    hgen = hopt["genomes"] if hopt.get("genomes") is not None else [j.haplo_genome for j in jobs]
    for j, g in zip(jobs, _per_job(hgen, jobs, "haplo: %d genomes entries for %d jobs")):
        on, j.haplo_genome = (hgap, g) if g and _mixed(j) else (None, None)
        j.haplo, j.hapsub = (None, on) if hapsub else (on, None)
        if on is not None:
            _paths(j)
            j.sites_out = j.sites_out or sites_path(j)
            if hapsub:
                j.subsets_out = j.subsets_out or subsets_path(j)
    if not any(_hap_gap(j) is not None for j in jobs) and any(_mixed(j) for j in jobs):
        raise ValueError("haplo: no job names the genome its VCF was called against (Job.haplo_genome, or haplo={'genomes': [...]})")


def _haplo_spec(jobs, pure, load, subsets=False):
    """the dict of the haplotype pass; when a job asks for the search behind it (the pass table let none ask for haplo beside it), the
    dict goes under hapsub with the subsets files, and nothing under haplo"""
    from .haplo import check_gap
    on = [_hap_gap(j) is not None for j in jobs]
    if not any(on) or any(j.hapsub is not None for j in jobs) != subsets:
        return None
    hps = {"gap": check_gap(next(_hap_gap(j) for j, w in zip(jobs, on) if w)),
           "genomes": [load(j.haplo_genome, keep=True) if w else -1 for j, w in zip(jobs, on)],
           "sites": [j.sites_out if w else None for j, w in zip(jobs, on)]}
    hps["seqs"] = [load.seqs.get(j.haplo_genome) if w and (j.sites_out or (j.hapsub is not None and j.subsets_out)) else None for j, w in zip(jobs, on)]
    return dict(hps, subsets=[j.subsets_out if j.hapsub is not None else None for j in jobs]) if subsets else hps


def _boot_onto_jobs(jobs, boot, **kw):
    from .bootstrap import DEFAULTS
    par = tuple(int(boot.get(k, DEFAULTS[k])) for k in ("window", "n_win", "n_rep", "seed"))
    for j in jobs:
        j.boot = par


def _agreed(jobs, field, names=(), **more):
    """the parameter tuple the jobs agreed on in Job.<field> under its names and who wants the pass, or None when no job does"""
    par = next((getattr(j, field) for j in jobs if getattr(j, field)), None)
    return dict(zip(names, par), want=[1 if getattr(j, field) else 0 for j in jobs], **{k: f(par) for k, f in more.items()}) if par else None


def _boot_after(rows, jobs, spec, alleles):
    for r in rows:
        if "boot_cnt" in r:
            r["boot_params"] = {k: spec[k] for k in ("window", "n_win", "n_rep", "seed")}
            r["boot_truth"] = not alleles


def _strata_onto_jobs(jobs, strata, **kw):
    from .strata import freeze
    frozen = freeze(strata)
    for j in jobs:
        j.strata = frozen


def _genomes_onto_jobs(jobs, genomes, **kw):
    for j, g in zip(jobs, _per_job(genomes, jobs, "genomes: %d entries for %d jobs")):
        j.genome = g


def _profile_onto_jobs(jobs, profile, **kw):
    want = list(profile["want"])
    pts = list(profile.get("points") or [None] * len(jobs))
    if len(want) != len(jobs) or len(pts) != len(jobs):
        raise ValueError("profile: %d want / %d points entries for %d jobs" % (len(want), len(pts), len(jobs)))
    par = (int(profile.get("window", 1024)), int(profile.get("n_pos_bins", 256)), int(profile.get("n_af_bins", 20)))
    for j, w, pt in zip(jobs, want, pts):
        j.profile = par if w else None
        j.points_out = pt if w else None


# In the order extract_many has always applied the keywords: when two of them are wrong at once, the earlier one speaks.  That is
# not the order of passes.PASSES (which decides the wording of check_shared_call).  So truthside stands twice: its `groups` are
# labelled where votes' are, its fn files derived last (the first row has no spec).  hapsub=True goes onto the jobs with haplo=.
PASS_IO = (
    PassIO("votes", "votes", _votes_onto_jobs, _votes_spec, ("out",), after=_votes_after),
    PassIO("truthside", None, _groups_onto_jobs, None),
    PassIO("nearmiss", "nearmiss", _explain_onto_jobs, _nearmiss_spec, ("fp_why", "fn_why")),
    PassIO("surface", "surface", _surface_onto_jobs, _surface_spec),
    PassIO("context", "context", _context_onto_jobs, _context_spec, on_pure=True),
    PassIO("normalize", "normalize", _normalize_onto_jobs, lambda jobs, pure, load: {
        "genomes": [load(j.normalize) if j.normalize else -1 for j in jobs],
        "rescued": [j.rescued_out if j.normalize else None for j in jobs]} if any(j.normalize for j in jobs) else None, ("rescued",)),
    PassIO("rescueroc", "rescue_roc", _rescue_roc_onto_jobs, lambda jobs, pure, load: {
        "genomes": [load(j.rescue_roc) if j.rescue_roc else -1 for j in jobs], "want": [1 if j.rescue_roc else 0 for j in jobs]} if any(j.rescue_roc for j in jobs) else None),
    PassIO("ladder", "ladder", _ladder_onto_jobs, _ladder_spec, ("out",)),
    PassIO("laddertypes", "ladder_types", _ladder_types_onto_jobs, _ladder_types_spec),
    PassIO("atomize", "atomize", _atomize_onto_jobs, lambda jobs, pure, load: {
        "want": [1 if j.atomize else 0 for j in jobs], "atoms": [j.atoms_out if j.atomize else None for j in jobs]} if any(j.atomize for j in jobs) else None, ("atoms",)),
    PassIO("vartype", "vartype", _vartype_onto_jobs, _vartype_spec),
    PassIO("haplo", "haplo", _haplo_onto_jobs, _haplo_spec, ("sites",)),
    PassIO("hapsub", "hapsub", _haplo_onto_jobs, lambda jobs, pure, load: _haplo_spec(jobs, pure, load, True), ("sites", "subsets")),
    PassIO("boot", "boot", _boot_onto_jobs, lambda jobs, pure, load: _agreed(jobs, "boot", ("window", "n_win", "n_rep", "seed")), on_pure=True, after=_boot_after),
    PassIO("strata", "strata", _strata_onto_jobs, lambda jobs, pure, load: _agreed(jobs, "strata", id=load.strata), on_pure=True),
    PassIO("motifs", "genomes", _genomes_onto_jobs, lambda jobs, pure, load: [load(j.genome) if j.genome else -1 for j in jobs] if any(j.genome for j in jobs) else None, on_pure=True),
    PassIO("profile", "profile", _profile_onto_jobs, lambda jobs, pure, load: _agreed(
        jobs, "profile", ("window", "n_pos_bins", "n_af_bins"), points=lambda par: [j.points_out if j.profile else None for j in jobs]), ("points",), on_pure=True),
    PassIO("truthside", "truthside", _fn_onto_jobs, _truthside_spec, ("fn", "missed")),
)


# extract_files is called with the keyword of every pass, None where none is asked for -- but for these, which go only when asked for
# (the call of a run without them is the call it has always been)
_WHEN_ASKED = ("ladder", "ladder_types")


def _one_genome_per_truth(jobs, field, who, what):
    """VCFs of one truth file name one genome in Job.<field>"""
    by_truth = {}
    for j in jobs:
        g, truth = getattr(j, field), os.path.realpath(j.snp_file)
        if g and by_truth.setdefault(truth, (g, j.vcf_file))[0] != g:
            raise ValueError("%s: %s and %s share the truth file %s and name the genomes %s and %s (%s)" % (who, by_truth[truth][1], j.vcf_file, j.snp_file, by_truth[truth][0], g, what))


def extract_many(jobs, engine=None, strict=None, n_bins=256, alleles=None, gpus=None, truth_slots=None, n_slots=0, global_dev=None,
                 genomes=None, fn=False, groups=None, profile=None, strata=None, boot=None, votes=None, explain=None,
                 surface=None, context=None, normalize=None, atomize=None, vartype=None, haplo=None, hapsub=None, rescue_roc=None, ladder=None,
                 ladder_types=None):
    """Classify and write filtered / tp / fp VCFs for a list of Job.  Returns the jobs
    with .stats filled (line counts, R-path counts, ROC rows).
    gpus > 1: the VCFs are dealt to that many GPUs of this node, one process each (quasimodo_amd.multigpu).
    alleles=True (or QM_ALLELES=1): the allele-extended mode -- every record whose REF and ALT are
    [ACGT]+ takes part, not only single bases (a build-defined widening of the reference's filter,
    include/qmvt.h; hcmv mode only).
    truth_slots / n_slots / global_dev: this call is one rank's share of a multi-GPU run (Engine.extract_files).
    genomes: per job a FASTA path (one sequence) or None (default: Job.genome): the jobs that have one get
    stats["motifs"], their [3][98] mutation-context rows (kept, TP, FP; quasimodo_amd.motifs).  Every distinct FASTA is
    loaded once and released before this returns.
    fn=True: every mixed-sample job also gets fn/<x>.fn.vcf (Job.fn_out), the rows of its truth file no kept record carries.
    groups: lists of job indices (1 to 5 mixed-sample jobs of one truth file each; default: the jobs' Job.group labels): the
    members' stats gain truth_regions / fp_regions (quasimodo_amd.truthside.venn_counts), members in job order.  Over several
    GPUs a group must sit on one rank (WorkflowError otherwise).
    profile: {"want": [0/1 per job], "window": 1024, "n_pos_bins": 256, "n_af_bins": 20, "points": [path or None per job]}
    (default: the jobs' Job.profile / Job.points_out): the wanted jobs get stats["af_grid"] ([2][n_af_bins][n_pos_bins]: TP, FP
    SNVs by allele frequency and position) and stats["af_extra"] ([2][3]: no AF, outside, in the grid; quasimodo_amd.afprofile),
    and their points files are written.
    strata: a list of (name, starts, ends) BED strata (quasimodo_amd.strata; default: the jobs' Job.strata): every job gets
    stats["strata_rec"] ([S + 2][3]: kept, TP, FP lines per stratum, then outside, nokey) and stats["strata_tru"] ([S + 1][2]:
    truth keys and hit ones per stratum, then outside; None in the allele-extended mode; zero for pure-strain samples).
    boot: {"window": 1024, "n_win": 256, "n_rep": 1000, "seed": 0} (quasimodo_amd.bootstrap; default: the jobs' Job.boot): every
    job gets stats["boot_cnt"] ([n_win + 2][4]: kept lines, TP lines, truth keys, hit keys per window, then outside, nokey),
    stats["boot_rep"] ([n_rep][4]: the bootstrap replicates of the four sums, the same draws for every job, call, rank and
    device), stats["boot_params"] and stats["boot_truth"] (False in the allele-extended mode: columns 2 and 3 are zero).
    votes: True or {"k": [level or 0 per group], "out": [path or None per group]} (quasimodo_amd.consensus; default: the jobs'
    Job.vote_group / consensus_k / consensus_out): `groups` then names the VOTE groups (1 to 32 mixed-sample jobs of one truth
    file each, a job in at most one): the members' stats gain tp_votes / fp_votes ([33]), private_tp / private_fp ([32]),
    vote_member (the job's index in its group) and vote_callers (the members' Job.caller, in member order = job order), and the
    groups with a level get their consensus VCF.  Over several GPUs a group must sit on one rank (WorkflowError otherwise).
    explain: a radius, 0 to 64 (quasimodo_amd.nearmiss; default: the jobs' Job.explain / fp_why_out / fn_why_out): every
    mixed-sample job gets stats["nearmiss_rec"] ([6]: its FP lines per class idcol, allele, refbase, near, isolated, nokey) and
    stats["nearmiss_tru"] ([5]: its missed truth keys per class filtered, allele, position, near, uncalled), and
    why/<x>.fp.why.tsv and why/<x>.fn.why.tsv beside fp/ and tp/.
    surface: True or {"q_step": 4, "nq": 64, "na": 50} (quasimodo_amd.surface; default: the jobs' Job.surface): every mixed-sample
    job gets stats["surface"] ([3][nq][na]: TP records, FP records and found truth keys under QUAL >= i * q_step and AF >= k / na),
    stats["surface_extra"] ([4]: counted records, counted records without AF, records without a quality bin, T') and
    stats["surface_params"].
    context: {"genomes": [FASTA path or None per job], "half_window": 50, "n_gc": 10} (quasimodo_amd.context; default: the jobs'
    Job.context / Job.context_genome): the jobs with a genome get stats["context_rec"] ([16 n_gc + 2][3]: kept, TP, FP lines per
    homopolymer x GC cell, then none, nokey), stats["context_tru"] ([16 n_gc + 1][2]: truth keys and hit ones; None in the
    allele-extended mode; zero for pure-strain samples), stats["context_gen"] ([16 n_gc + 1]: the genome's positions per cell) and
    stats["context_params"].  Every distinct FASTA is loaded once and released before this returns.
    normalize: {"genomes": [FASTA path or None per job]} or that list itself (quasimodo_amd.normalize; default: the
    jobs' Job.normalize / Job.rescued_out; alleles=True only, ValueError otherwise): every mixed-sample job with a genome gets
    stats["norm_rec"] ([12]: kept, TP, TP_N, rescued, respelled, single-base lines and the lines per reason a record has no normal
    form) and stats["norm_tru"] ([5]: truth entries, distinct forms, forms found, found by form only, entries without a normal
    form), and norm/<x>.rescued.tsv beside fp/ and tp/.  VCFs of one truth file name one genome.
    atomize: True, or one truth value per job (quasimodo_amd.atomize; default: the jobs' Job.atomize /
    Job.atoms_out; alleles=True only, ValueError otherwise): every wanted mixed-sample job gets stats["atom_rec"] ([13]: kept, TP,
    TP_A, rescued, multi-atom and partial lines, atoms, atoms hit and the lines per reason a record is not atomisable) and
    stats["atom_tru"] ([6]: truth entries, atomisable ones, distinct atoms, atoms found, entries found by spelling and by atoms),
    and atoms/<x>.atoms.tsv beside fp/ and tp/.
    vartype: True (the default size edges 1,2,3,4,5,6,16,51) or the ascending lower edges of the size bins (quasimodo_amd.vartype,
    DESIGN.md 4.19; default: the jobs' Job.vartype; alleles=True only, ValueError otherwise): every mixed-sample job gets
    stats["type_rec"] ([5 n_bins + 4][2]: per type x size row, then NOKEY, NOVAR, LONGPAIR, NOSHAPE, the kept lines and the TP
    lines among them), stats["type_tru"] (the same rows: truth entries and the found ones) and stats["type_edges"].
    rescue_roc: {"genomes": [FASTA path or None per job]} or that list itself (quasimodo_amd.rescueroc; default: the
    jobs' Job.rescue_roc; alleles=True only, ValueError otherwise), in place of normalize and atomize, which the call runs itself:
    every mixed-sample job with a genome gets stats["rroc_n"] and stats["rroc_a"] ([3][n_bins]: TP(t), FP(t), U(t) under QUAL >= t
    by normal form and by atoms, beside stats["roc"] by spelling) and stats["rroc_base"] ([2]: the distinct forms and the entries
    of its truth set; FN(t) = base - U(t)).  VCFs of one truth file name one genome.
    ladder: [FASTA path or None per job] or {"genomes": that list, "gap": None or 0 .. 32} (quasimodo_amd.ladder, DESIGN.md 4.23;
    default: the jobs' Job.ladder / Job.ladder_genome / Job.ladder_out; alleles=True only, ValueError otherwise), in place of
    normalize, atomize, haplo and hapsub, which the call runs itself: every mixed-sample job with a genome gets
    stats["ladder_rec"] ([18]: kept, TP lines, then the 16 cells of the method bits over the kept lines that are no TP by
    spelling; cell 0 is the final FP) and stats["ladder_tru"] ([18]: entries, entries a kept record spells, then the 16 cells
    over the others; cell 0 is the final FN), and ladder/<x>.ladder.tsv beside fp/ and tp/.  VCFs of one truth file name one genome.
    ladder_types: {"genomes": [FASTA path or None per job], "gap": None or 0 .. 32, "edges": None or the size edges} or the list of
    genomes itself (quasimodo_amd.laddertypes; default: the jobs' Job.ladder_types / Job.ladder_types_genome;
    alleles=True only, ValueError otherwise), in place of ladder and vartype, which the call runs itself with all four rescues:
    every mixed-sample job with a genome gets stats["ladder_types_rec"] and stats["ladder_types_tru"] ([5 n_bins + 4][18]: the
    rows of vartype -- records typed as spelled --, the columns of ladder) and stats["ladder_types_edges"].  VCFs of one truth
    file name one genome.
    Which of these may share a call: quasimodo_amd.passes -- genomes with profile, every other pass alone (ValueError)."""
    kw = dict(genomes=genomes, fn=fn, groups=groups, profile=profile, strata=strata, boot=boot, votes=votes, explain=explain, surface=surface,
              context=context, normalize=normalize, atomize=atomize, vartype=vartype, haplo=haplo, hapsub=hapsub, rescue_roc=rescue_roc, ladder=ladder,
              ladder_types=ladder_types)
    given = {"motifs": genomes is not None, "truthside": bool(fn) or (groups is not None and not votes), "profile": profile is not None,
             "strata": strata is not None, "boot": boot is not None, "votes": bool(votes), "nearmiss": explain is not None,
             "surface": surface is not None and surface is not False, "context": context is not None, "normalize": normalize is not None,
             "atomize": atomize is not None and atomize is not False, "vartype": vartype is not None and vartype is not False,
             "haplo": haplo is not None and haplo is not False and not hapsub, "hapsub": bool(hapsub), "rescueroc": rescue_roc is not None,
             "ladder": ladder is not None, "laddertypes": ladder_types is not None}
    # the keywords onto the jobs ...
    for p in PASS_IO:
        if given[p.name]:
            p.onto_jobs(jobs, **kw)
    # ... which may share the call, and agree on the parameters of a pass
    check_shared_call({name for name, g in given.items() if g} | requested_by(jobs))
    for p in PASSES:
        if p.agree and len({getattr(j, p.fields[0]) for j in jobs if getattr(j, p.fields[0]) is not None}) > 1:
            raise ValueError(p.agree)
    strict = _strict_default() if strict is None else strict
    alleles = _alleles_default() if alleles is None else bool(alleles)
    check_alleles(requested_by(jobs), alleles)
    for j in jobs:
        if _hap_gap(j) is not None and not j.haplo_genome:
            raise ValueError("%s: Job.haplo without Job.haplo_genome (the FASTA the VCF was called against)" % j.vcf_file)
    _one_genome_per_truth([j for j in jobs if _hap_gap(j) is not None], "haplo_genome", "haplo", "the sites of a truth set belong to one genome")
    _one_genome_per_truth(jobs, "normalize", "normalize", "a normalised truth set belongs to one genome")
    _one_genome_per_truth(jobs, "rescue_roc", "rescue_roc", "a normalised truth set belongs to one genome")
    for j in jobs:
        if j.ladder is not None and not j.ladder_genome:
            raise ValueError("%s: Job.ladder without Job.ladder_genome (the FASTA the VCF was called against)" % j.vcf_file)
    _one_genome_per_truth([j for j in jobs if j.ladder is not None], "ladder_genome", "ladder", "a normalised truth set belongs to one genome")
    for j in jobs:
        if j.ladder_types is not None and not j.ladder_types_genome:
            raise ValueError("%s: Job.ladder_types without Job.ladder_types_genome (the FASTA the VCF was called against)" % j.vcf_file)
    _one_genome_per_truth([j for j in jobs if j.ladder_types is not None], "ladder_types_genome", "ladder_types", "a normalised truth set belongs to one genome")
    if gpus is not None and int(gpus) > 1:
        if engine is not None:
            raise ValueError("gpus > 1 starts one process (and one engine) per GPU: do not pass an engine")
        from .multigpu import extract_many_sharded
        plan = None
        if any(j.group is not None or j.vote_group is not None for j in jobs):   # the members of a group go to one rank
            by = {}
            for i, j in enumerate(jobs):
                by.setdefault(("g", j.group) if j.group is not None else ("v", j.vote_group) if j.vote_group is not None else ("j", i), []).append(i)
            plan = list(by.values())
        return extract_many_sharded(jobs, int(gpus), n_bins=n_bins, alleles=alleles, strict=strict, groups=plan)[0]
    if alleles and any(j.mode != "hcmv" for j in jobs):
        raise ValueError("the allele-extended mode needs VCF truth sets (hcmv mode)")
    own = engine is None
    for job in jobs:
        _paths(job)
    if not jobs:
        return jobs
    pure = [is_pure_strain(j.vcf_file) for j in jobs]
    if engine is None:
        # a context is needed even for a batch of pure-strain samples only when something is to be classified
        need = not all(pure) or any(getattr(j, f) for io in PASS_IO if io.on_pure for p in PASSES if p.name == io.name for f in p.fields for j in jobs)
        engine = Engine(int(os.environ.get("QM_DEVICE", "0"))) if need else None
    load = _Loaded(engine)
    try:
        specs = {p.key: p.spec(jobs, pure, load) for p in PASS_IO if p.spec}
        for path in [x for p in PASS_IO if engine is not None and specs.get(p.key) for k in p.outs for x in specs[p.key][k] if x]:
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        for job, p in zip(jobs, pure):
            os.makedirs(os.path.dirname(job.fp_out) or ".", exist_ok=True)
            os.makedirs(os.path.dirname(job.filtered_out) or ".", exist_ok=True)
            if not p:
                os.makedirs(os.path.dirname(job.tp_out) or ".", exist_ok=True)
        fj = [dict(vcf=j.vcf_file, truth=None if p else j.snp_file, mode=j.mode, pure=p, filtered=j.filtered_out,
                   tp=None if p else j.tp_out, fp=j.fp_out) for j, p in zip(jobs, pure)]
        extract_many.last_paths = None
        if engine is None:
            rows = _pure_only(fj, strict)
        else:
            before = engine.path_stats_total()
            rows, phases = engine.extract_files(fj, n_bins=n_bins, alleles=alleles, strict=strict, truth_slots=truth_slots, n_slots=n_slots,
                                                global_dev=global_dev, **{k: v for k, v in specs.items() if v is not None or k not in _WHEN_ASKED})
            for p in PASS_IO:
                if p.after and specs[p.key] is not None:
                    p.after(rows, jobs, specs[p.key], alleles)
            extract_many.last_phases = phases
            # where the VCFs found out of order went (bucket paths / radix sort: a silent fall onto the slow path shows here)
            extract_many.last_paths = {k: v - before[k] for k, v in engine.path_stats_total().items()}
    finally:
        if engine is not None:
            load.release()
        if own and engine is not None:
            engine.close()
    for job, p, r in zip(jobs, pure, rows):
        job.stats = r
        job.stats.update(pure_strain=p)
        if p:
            job.tp_out = ""
            job.stats["roc"] = None
    return jobs


extract_many.last_phases = None
extract_many.last_paths = None


def _pure_only(file_jobs, strict):
    """Pure-strain samples need no device (extract_TP_FP_SNPs.py:33-36: fp is a copy of filtered): when a call holds
    nothing else, no context is created and the host side of the library does the work."""
    rows = []
    for j in file_jobs:
        with open(j["vcf"], "rb") as fh:
            sv = scan_vcf(fh.read())
        if sv.n_refused and strict:
            raise QmvtError(-8, "%s line %d: a kept line holds a NUL or bytes that are not valid UTF-8 -- the reference's answer for it depends on the "
                                "locale Python exports to grep; set QM_LENIENT=1 to classify it by its columns" % (j["vcf"], sv.first_refused_line))
        cls = (sv.flags & 1).astype(np.uint8)
        sv.write(j["filtered"], cls, 0)
        sv.write(j["fp"], cls, 0)
        npass = int(cls.sum())
        r = dict(zip(SCALAR_NAMES, (npass, 0, npass, 0, 0, 1, sv.n_records, 0)))
        r.update(n_lines=sv.n_lines, n_refused=sv.n_refused, genomediff=0, header_kept=sv.header_kept, host_decided=0, roc=None,
                 r_hostile=sv.n_r_hostile)
        rows.append(r)
    return rows


def extract_tp_fp_snp(vcf_file, snp_file, engine=None, strict=None):
    """Extract the TP and FP SNPs of one caller VCF (hcmv mode).
    @param vcf_file: caller VCF.  @param snp_file: truth VCF written by mummer2vcf.py.
    Outputs next to the input: <x>.filtered.vcf, fp/<x>.fp.vcf, tp/<x>.tp.vcf (:19-22,39-41)."""
    return extract_many([Job(vcf_file, snp_file, "hcmv")], engine=engine, strict=strict)[0]


def extract_tp_fp_custom_snp(vcf_file, snp_file, outdir, caller, engine=None, strict=None):
    """Custom (vareval) mode: truth is the show-snps TSV; outputs under outdir (:71-72,91)."""
    return extract_many([Job(vcf_file, snp_file, "custom", outdir, caller)], engine=engine, strict=strict)[0]
