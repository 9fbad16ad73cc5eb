"""The opt-in passes over a finished batch: one description per pass, and the one rule for which of them
may share a call -- motifs with profile; every other pass runs in a call of its own."""
from collections import namedtuple

# name: the pass, and Engine.extract_files' keyword but for motifs (`genomes`); fields: the Job fields that ask for it;
# keywords: extract_many's; flag: the CLI's, for messages; agree: what to say when the jobs of a call name different parameter
# tuples in Job.<name> (None: the pass has none); shares: the passes it may share a call with
Pass = namedtuple("Pass", "name fields keywords flag agree shares")
PASSES = (
    Pass("motifs", ("genome",), ("genomes",), "--mutation-context", None, ("profile",)),
    Pass("truthside", ("fn_out", "group"), ("fn", "groups"), "--truth-side", None, ()),
    Pass("profile", ("profile",), ("profile",), "--snp-profile",
         "profile: the profiled jobs of one call share one window and one pair of bin counts", ("motifs",)),
    Pass("strata", ("strata",), ("strata",), "--strata", "strata: the stratified jobs of one call share one strata set", ()),
    Pass("boot", ("boot",), ("boot",), "--bootstrap",
         "boot: the resampled jobs of one call share one window, window count, replicate count and seed", ()),
    Pass("votes", ("vote_group",), ("votes",), "--votes", None, ()),
    Pass("nearmiss", ("explain",), ("explain",), "--explain-errors", "explain: the explained jobs of one call share one radius", ()),
    Pass("normalize", ("normalize",), ("normalize",), "--normalize", None, ()),
    Pass("haplo", ("haplo",), ("haplo",), "--haplotypes", "haplo: the jobs of one call share one gap", ()),
    # the haplotype pass AND the subset search behind it, from one call: asked for in place of haplo, never beside it
    Pass("hapsub", ("hapsub",), ("hapsub",), "--hap-subsets", "hapsub: the jobs of one call share one gap", ()),
    # the QUAL sweep of normalize AND atomize, which it runs itself: asked for in place of them, never beside them
    Pass("rescueroc", ("rescue_roc",), ("rescue_roc",), "--rescue-roc", None, ()),
    # the four rescue passes, which it runs itself, combined: asked for in place of them, never beside them
    Pass("ladder", ("ladder",), ("ladder",), "--match-ladder", "ladder: the jobs of one call share one gap", ()),
    # the four rescue passes, the type pass and the ladder, all of which it runs itself, crossed: asked for in place of them
    Pass("laddertypes", ("ladder_types",), ("ladder_types",), "--ladder-by-type",
         "ladder_types: the jobs of one call share one gap and one list of size edges", ()),
    Pass("atomize", ("atomize",), ("atomize",), "--atomize", None, ()),
    Pass("vartype", ("vartype",), ("vartype",), "--by-type", "vartype: the typed jobs of one call share one list of size edges", ()),
    Pass("context", ("context",), ("context",), "--seq-context",
         "context: the profiled jobs of one call share one half window and one GC bin count", ()),
    Pass("surface", ("surface",), ("surface",), "--filter-surface",
         "surface: the swept jobs of one call share one QUAL step and one pair of bin counts", ()),
)


class SharedCallError(ValueError):
    """two passes that do not share a call; .flags: their CLI names"""

    def __init__(self, a, b):
        said = lambda p: p.name if p.keywords == (p.name,) else "%s (%s)" % (p.name, " / ".join(p.keywords))
        ValueError.__init__(self, "%s does not combine with %s in one call: it runs in a call of its own" % (said(a), said(b)))
        self.flags = (a.flag, b.flag)

    def for_cli(self):
        return "%s cannot be combined with %s: it runs in a call of its own." % self.flags


def check_shared_call(requested):
    """requested: names of the passes one call is asked for.  Raises SharedCallError for the first pair that may not share it
    (the later pass of PASSES named first)."""
    want = [p for p in PASSES if p.name in requested]
    for i, a in enumerate(want):
        for b in want[:i]:
            if b.name not in a.shares:
                raise SharedCallError(a, b)


# The passes that read indels, MNPs or complex records, which only the allele-extended mode holds, in the order they are asked about,
# and what a single-base batch lacks for each: Pass.needs_alleles (None for every other pass).  A column beside the table, not a
# seventh field of it: the tests of the passes compare whole six-field rows.
NEEDS_ALLELES = {
    "normalize": "a single-base batch holds no indels or MNPs",
    "atomize": "a single-base batch holds no MNPs",
    "vartype": "a single-base batch holds SNVs only",
    "haplo": "a single-base batch holds no indels, MNPs or complex records to replay",
    "hapsub": "a single-base batch holds no indels, MNPs or complex records to replay",   # (it runs the haplotype pass)
    "rescueroc": "a single-base batch has no rescue passes to sweep",
    "ladder": "a single-base batch has no rescue passes to combine",
    "laddertypes": "a single-base batch has neither types nor rescue passes to cross",
}
Pass.needs_alleles = property(lambda p: NEEDS_ALLELES.get(p.name))


def check_alleles(requested, alleles):
    """ValueError, before a file is touched, for the first pass of NEEDS_ALLELES that is requested without the allele-extended mode"""
    for p in (p for name in NEEDS_ALLELES for p in PASSES if p.name == name):
        if p.name in requested and not alleles:
            raise ValueError("%s (%s) needs the allele-extended mode (--alleles): %s" % (p.name, p.flag, p.needs_alleles))


def requested_by(jobs):
    """the passes the fields of these Jobs ask for"""
    return {p.name for p in PASSES if any(getattr(j, f) not in (None, "") for j in jobs for f in p.fields)}
