"""extract_many from its keywords (or the Job fields) to the one call of Engine.extract_files, pass by pass, against a recording
stand-in for the engine: the dicts the engine receives, the genomes and strata loaded and released, the directories made, the Job
fields afterwards, what the rows gain, and every refusal in front of the call, word for word.  No device: extract_many calls
path_stats_total, genome_load / genome_release, strata_load / strata_release, extract_files and close of its engine, nothing else."""
import dataclasses
import os

import pytest

from quasimodo_amd import extract
from quasimodo_amd.extract import Job, extract_many

SEQ = {"a.fa": b"ACGTACGT", "b.fa": b"TTTTGGGG"}
PASS_KEYS = ("genomes", "truthside", "profile", "strata", "boot", "votes", "nearmiss", "surface", "context", "normalize", "atomize",
             "vartype", "haplo", "hapsub", "rescue_roc")
COMMON = ("vcf_file", "snp_file", "mode", "outdir", "caller", "filtered_out", "tp_out", "fp_out", "stats")
DEFAULT = {f.name: f.default for f in dataclasses.fields(Job) if f.name not in COMMON}
EDGES = (1, 2, 3, 4, 5, 6, 16, 51)


class Stand:
    """the seven methods extract_many calls; genome ids count from 100 in load order, the strata id is 7"""

    def __init__(self, fail=False):
        self.fail, self.loads, self.gone, self.strata, self.strata_gone, self.closed, self.kw, self.fj = fail, [], [], [], [], 0, None, None

    def path_stats_total(self):
        return {"unsorted": 0}

    def genome_load(self, seq):
        self.loads.append(bytes(seq))
        return 99 + len(self.loads)

    def genome_release(self, gid):
        self.gone.append(gid)

    def strata_load(self, strata):
        self.strata.append(strata)
        return 7

    def strata_release(self, sid):
        self.strata_gone.append(sid)

    def extract_files(self, fj, **kw):
        self.fj, self.kw = fj, kw
        if self.fail:
            raise RuntimeError("the call failed")
        boot = kw.get("boot")
        return [dict({"roc": "R%d" % k}, **({"boot_cnt": "B%d" % k} if boot and boot["want"][k] else {})) for k in range(len(fj))], {"engine": 0.0}

    def close(self):
        self.closed += 1


def mk(tmp):
    for name, seq in SEQ.items():
        (tmp / name).write_bytes(b">" + name.encode() + b" x\n" + seq[:5] + b"\n" + seq[5:] + b"\n")
    t = str(tmp / "t.vcf")
    return [Job(str(tmp / "TM-1-1.x.c0.vcf"), t, caller="c0"), Job(str(tmp / "TM-1-1.x.c1.vcf"), t, caller="c1"),
            Job(str(tmp / "TM-1-0.x.c0.vcf"), t, caller="c0"), Job(str(tmp / "TM-0-1.x.c0.vcf"), t, caller="c0")]


def absolute(x, tmp):
    """the case tables write paths relative to tmp_path, as strings that end in .fa / .tsv / .vcf"""
    if isinstance(x, str) and x.endswith((".fa", ".tsv", ".vcf")):
        return str(tmp / x)
    if isinstance(x, (list, tuple)):
        return type(x)(absolute(y, tmp) for y in x)
    if isinstance(x, dict):
        return {k: absolute(v, tmp) for k, v in x.items()}
    return x


def relative(x, tmp):
    if isinstance(x, str):
        return x.replace(str(tmp) + os.sep, "")
    if isinstance(x, (list, tuple)):
        return type(x)(relative(y, tmp) for y in x)
    if isinstance(x, dict):
        return {k: relative(v, tmp) for k, v in x.items()}
    return x


W0, W1 = "why/TM-1-1.x.c0", "why/TM-1-1.x.c1"
HAP = {"gap": 3, "genomes": [100, 100, -1, -1], "sites": ["hap/TM-1-1.x.c0.sites.tsv", "hap/TM-1-1.x.c1.sites.tsv", None, None],
       "seqs": [SEQ["a.fa"], SEQ["a.fa"], None, None]}
HAPJ = [dict(haplo=3, haplo_genome="a.fa", sites_out="hap/TM-1-1.x.c0.sites.tsv"), dict(haplo=3, haplo_genome="a.fa", sites_out="hap/TM-1-1.x.c1.sites.tsv"), {}, {}]
SUBJ = [dict(hapsub=3, haplo_genome="a.fa", sites_out="hap/TM-1-1.x.c0.sites.tsv", subsets_out="hap/TM-1-1.x.c0.subsets.tsv"),
        dict(hapsub=3, haplo_genome="a.fa", sites_out="hap/TM-1-1.x.c1.sites.tsv", subsets_out="hap/TM-1-1.x.c1.subsets.tsv"), {}, {}]
BOOT = {"window": 1024, "n_win": 256, "n_rep": 1000, "seed": 0}
STRATA = (("all", (0,), (100,)),)
NORMJ = [dict(normalize="a.fa", rescued_out="norm/TM-1-1.x.c0.rescued.tsv"), dict(normalize="a.fa", rescued_out="norm/TM-1-1.x.c1.rescued.tsv"), {}, {}]
NORM = {"genomes": [100, 100, -1, -1], "rescued": ["norm/TM-1-1.x.c0.rescued.tsv", "norm/TM-1-1.x.c1.rescued.tsv", None, None]}
RROC = {"genomes": [100, 100, -1, -1], "want": [1, 1, 0, 0]}
ATOMJ = [dict(atomize=True, atoms_out="atoms/TM-1-1.x.c0.atoms.tsv"), dict(atomize=True, atoms_out="atoms/TM-1-1.x.c1.atoms.tsv"), {}, {}]
WHYJ = [dict(explain=3, fp_why_out=W0 + ".fp.why.tsv", fn_why_out=W0 + ".fn.why.tsv"), dict(explain=3, fp_why_out=W1 + ".fp.why.tsv", fn_why_out=W1 + ".fn.why.tsv"), {}, {}]
VOTE_ROWS = [{"vote_callers": ["c0", "c1"]}, {"vote_callers": ["c0", "c1"]}, {}, {}]
BOOT_ROWS = [{"boot_cnt": "B%d" % k, "boot_params": BOOT, "boot_truth": True} for k in range(4)]

# id, alleles, the keywords of extract_many (kw) or the Job fields set directly (fields, per job), then what is observed: spec -- the
# pass keywords Engine.extract_files receives that are not None; loads -- the bases of each genome_load; dirs -- the directories made
# besides fp/ and tp/; jobs -- the pass fields of each Job that differ from the default afterwards; rows -- what each row gains
CASES = [
    dict(id="motifs", kw=dict(genomes=["a.fa", "b.fa", "a.fa", None]), spec={"genomes": [100, 101, 100, -1]}, loads=["a.fa", "b.fa"],
         jobs=[{"genome": "a.fa"}, {"genome": "b.fa"}, {"genome": "a.fa"}, {}]),
    dict(id="motifs-fields", fields=[{}, {}, {"genome": "b.fa"}, {}], spec={"genomes": [-1, -1, 100, -1]}, loads=["b.fa"], jobs=[{}, {}, {"genome": "b.fa"}, {}]),
    dict(id="motifs-with-profile", kw=dict(genomes=["a.fa", None, None, None], profile={"want": [1, 0, 1, 0], "points": ["pts/p0.tsv", None, "pts2/p2.tsv", None]}),
         spec={"genomes": [100, -1, -1, -1], "profile": {"window": 1024, "n_pos_bins": 256, "n_af_bins": 20, "want": [1, 0, 1, 0], "points": ["pts/p0.tsv", None, "pts2/p2.tsv", None]}},
         loads=["a.fa"], dirs={"pts", "pts2"},
         jobs=[{"genome": "a.fa", "profile": (1024, 256, 20), "points_out": "pts/p0.tsv"}, {}, {"profile": (1024, 256, 20), "points_out": "pts2/p2.tsv"}, {}]),
    dict(id="profile", kw=dict(profile={"want": [1, 1, 0, 0], "window": 512, "n_pos_bins": 8, "n_af_bins": 4}),
         spec={"profile": {"window": 512, "n_pos_bins": 8, "n_af_bins": 4, "want": [1, 1, 0, 0], "points": [None] * 4}},
         jobs=[{"profile": (512, 8, 4)}, {"profile": (512, 8, 4)}, {}, {}]),
    dict(id="profile-fields", fields=[{}, {"profile": (64, 2, 3), "points_out": "p/x.tsv"}, {"profile": (64, 2, 3)}, {"points_out": "q/unused.tsv"}],
         spec={"profile": {"window": 64, "n_pos_bins": 2, "n_af_bins": 3, "want": [0, 1, 1, 0], "points": [None, "p/x.tsv", None, None]}}, dirs={"p"},
         jobs=[{}, {"profile": (64, 2, 3), "points_out": "p/x.tsv"}, {"profile": (64, 2, 3)}, {"points_out": "q/unused.tsv"}]),
    dict(id="fn", kw=dict(fn=True), spec={"truthside": {"fn": ["fn/TM-1-1.x.c0.fn.vcf", "fn/TM-1-1.x.c1.fn.vcf", None, None], "group": [-1] * 4, "missed": []}},
         dirs={"fn"}, jobs=[{"fn_out": "fn/TM-1-1.x.c0.fn.vcf"}, {"fn_out": "fn/TM-1-1.x.c1.fn.vcf"}, {}, {}]),
    dict(id="groups", kw=dict(groups=[[0], [1]]), spec={"truthside": {"fn": [None] * 4, "group": [0, 1, -1, -1], "missed": [None, None]}},
         jobs=[{"group": "g0"}, {"group": "g1"}, {}, {}]),
    dict(id="fn-and-groups", kw=dict(fn=True, groups=[[0, 1]]),
         spec={"truthside": {"fn": ["fn/TM-1-1.x.c0.fn.vcf", "fn/TM-1-1.x.c1.fn.vcf", None, None], "group": [0, 0, -1, -1], "missed": [None]}}, dirs={"fn"},
         jobs=[{"fn_out": "fn/TM-1-1.x.c0.fn.vcf", "group": "g0"}, {"fn_out": "fn/TM-1-1.x.c1.fn.vcf", "group": "g0"}, {}, {}]),
    dict(id="truthside-fields", fields=[{"group": "x", "missed_out": "miss/m.vcf"}, {"group": "x", "fn_out": "fnx/f.vcf"}, {"fn_out": "pure/f.vcf"}, {}],
         spec={"truthside": {"fn": [None, "fnx/f.vcf", None, None], "group": [0, 0, -1, -1], "missed": ["miss/m.vcf"]}}, dirs={"miss", "fnx"},
         jobs=[{"group": "x", "missed_out": "miss/m.vcf"}, {"group": "x", "fn_out": "fnx/f.vcf"}, {"fn_out": "pure/f.vcf"}, {}]),
    dict(id="strata", kw=dict(strata=[("all", [0], [100])]), spec={"strata": {"id": 7, "want": [1, 1, 1, 1]}}, strata=[STRATA], jobs=[{"strata": STRATA}] * 4),
    dict(id="strata-fields", fields=[{}, {"strata": STRATA}, {"strata": STRATA}, {}], spec={"strata": {"id": 7, "want": [0, 1, 1, 0]}}, strata=[STRATA],
         jobs=[{}, {"strata": STRATA}, {"strata": STRATA}, {}]),
    dict(id="boot", kw=dict(boot={}), spec={"boot": dict(BOOT, want=[1, 1, 1, 1])}, jobs=[{"boot": (1024, 256, 1000, 0)}] * 4, rows=BOOT_ROWS),
    dict(id="boot-params-alleles", alleles=True, kw=dict(boot={"n_rep": 10, "seed": 3, "window": "32"}),
         spec={"boot": {"window": 32, "n_win": 256, "n_rep": 10, "seed": 3, "want": [1, 1, 1, 1]}}, jobs=[{"boot": (32, 256, 10, 3)}] * 4,
         rows=[{"boot_cnt": "B%d" % k, "boot_params": {"window": 32, "n_win": 256, "n_rep": 10, "seed": 3}, "boot_truth": False} for k in range(4)]),
    dict(id="boot-fields", fields=[{"boot": (8, 4, 2, 1)}, {}, {}, {"boot": (8, 4, 2, 1)}], spec={"boot": {"window": 8, "n_win": 4, "n_rep": 2, "seed": 1, "want": [1, 0, 0, 1]}},
         jobs=[{"boot": (8, 4, 2, 1)}, {}, {}, {"boot": (8, 4, 2, 1)}],
         rows=[{"boot_cnt": "B0", "boot_params": {"window": 8, "n_win": 4, "n_rep": 2, "seed": 1}, "boot_truth": True}, {}, {},
               {"boot_cnt": "B3", "boot_params": {"window": 8, "n_win": 4, "n_rep": 2, "seed": 1}, "boot_truth": True}]),
    dict(id="votes-true", kw=dict(votes=True, groups=[[0, 1]]), spec={"votes": {"group": [0, 0, -1, -1], "k": [0], "out": [None]}},
         jobs=[{"vote_group": "v0"}, {"vote_group": "v0"}, {}, {}], rows=VOTE_ROWS),
    dict(id="votes-dict", kw=dict(votes={"k": [2], "out": ["cons/c.vcf"]}, groups=[[0, 1]]), spec={"votes": {"group": [0, 0, -1, -1], "k": [2], "out": ["cons/c.vcf"]}},
         dirs={"cons"}, jobs=[{"vote_group": "v0", "consensus_k": 2, "consensus_out": "cons/c.vcf"}] * 2 + [{}, {}], rows=VOTE_ROWS),
    dict(id="votes-level-without-file", kw=dict(votes={"k": [1, 0]}, groups=[[1], [0]]), spec={"votes": {"group": [0, 1, -1, -1], "k": [0, 0], "out": [None, None]}},
         jobs=[{"vote_group": "v1"}, {"vote_group": "v0", "consensus_k": 1}, {}, {}], rows=[{"vote_callers": ["c0"]}, {"vote_callers": ["c1"]}, {}, {}]),
    dict(id="votes-fields", fields=[{"vote_group": "a", "consensus_out": "cons/a.vcf"}, {"vote_group": "a", "consensus_k": 1}, {}, {}],
         spec={"votes": {"group": [0, 0, -1, -1], "k": [1], "out": ["cons/a.vcf"]}}, dirs={"cons"},
         jobs=[{"vote_group": "a", "consensus_out": "cons/a.vcf"}, {"vote_group": "a", "consensus_k": 1}, {}, {}], rows=VOTE_ROWS),
    dict(id="explain", kw=dict(explain=3), dirs={"why"}, jobs=WHYJ,
         spec={"nearmiss": {"radius": 3, "want": [1, 1, 0, 0], "fp_why": [W0 + ".fp.why.tsv", W1 + ".fp.why.tsv", None, None], "fn_why": [W0 + ".fn.why.tsv", W1 + ".fn.why.tsv", None, None]}}),
    dict(id="explain-fields", fields=[{"explain": 0, "fp_why_out": "w/fp.tsv"}, {}, {"explain": 0, "fn_why_out": "pure/fn.tsv"}, {}], dirs={"w"},
         spec={"nearmiss": {"radius": 0, "want": [1, 0, 0, 0], "fp_why": ["w/fp.tsv", None, None, None], "fn_why": [None] * 4}},
         jobs=[{"explain": 0, "fp_why_out": "w/fp.tsv"}, {}, {"explain": 0, "fn_why_out": "pure/fn.tsv"}, {}]),
    dict(id="surface-true", kw=dict(surface=True), spec={"surface": {"q_step": 4, "nq": 64, "na": 50, "want": [1, 1, 0, 0]}}, jobs=[{"surface": (4, 64, 50)}] * 2 + [{}, {}]),
    dict(id="surface-dict", kw=dict(surface={"q_step": 2, "nq": 8}), spec={"surface": {"q_step": 2, "nq": 8, "na": 50, "want": [1, 1, 0, 0]}},
         jobs=[{"surface": (2, 8, 50)}] * 2 + [{}, {}]),
    dict(id="surface-fields", fields=[{}, {"surface": (1, 2, 3)}, {"surface": (1, 2, 3)}, {}], spec={"surface": {"q_step": 1, "nq": 2, "na": 3, "want": [0, 1, 1, 0]}},
         jobs=[{}, {"surface": (1, 2, 3)}, {"surface": (1, 2, 3)}, {}]),
    dict(id="context", kw=dict(context={"genomes": ["a.fa", "a.fa", "b.fa", None]}), spec={"context": {"half_window": 50, "n_gc": 10, "genomes": [100, 100, 101, -1]}},
         loads=["a.fa", "b.fa"], jobs=[{"context": (50, 10), "context_genome": "a.fa"}] * 2 + [{"context": (50, 10), "context_genome": "b.fa"}, {}]),
    dict(id="context-params", kw=dict(context={"genomes": [None, "b.fa", None, None], "half_window": 5, "n_gc": 2}),
         spec={"context": {"half_window": 5, "n_gc": 2, "genomes": [-1, 100, -1, -1]}}, loads=["b.fa"], jobs=[{}, {"context": (5, 2), "context_genome": "b.fa"}, {}, {}]),
    dict(id="context-fields", fields=[{"context": (7, 3), "context_genome": "b.fa"}, {"context_genome": "a.fa"}, {}, {"context": (7, 3), "context_genome": "b.fa"}],
         spec={"context": {"half_window": 7, "n_gc": 3, "genomes": [100, -1, -1, 100]}}, loads=["b.fa"],
         jobs=[{"context": (7, 3), "context_genome": "b.fa"}, {"context_genome": "a.fa"}, {}, {"context": (7, 3), "context_genome": "b.fa"}]),
    dict(id="normalize-list", alleles=True, kw=dict(normalize=["a.fa", "a.fa", "b.fa", None]), spec={"normalize": NORM}, loads=["a.fa"], dirs={"norm"}, jobs=NORMJ),
    dict(id="normalize-dict", alleles=True, kw=dict(normalize={"genomes": ["a.fa", "a.fa", "b.fa", None]}), spec={"normalize": NORM}, loads=["a.fa"], dirs={"norm"}, jobs=NORMJ),
    dict(id="normalize-fields", alleles=True, fields=[{}, {"normalize": "b.fa"}, {}, {}], spec={"normalize": {"genomes": [-1, 100, -1, -1], "rescued": [None] * 4}},
         loads=["b.fa"], jobs=[{}, {"normalize": "b.fa"}, {}, {}]),
    dict(id="rescue-roc-list", alleles=True, kw=dict(rescue_roc=["a.fa", "a.fa", "b.fa", None]), spec={"rescue_roc": RROC}, loads=["a.fa"], jobs=[{"rescue_roc": "a.fa"}] * 2 + [{}, {}]),
    dict(id="rescue-roc-dict", alleles=True, kw=dict(rescue_roc={"genomes": ["a.fa", "a.fa", "b.fa", None]}), spec={"rescue_roc": RROC}, loads=["a.fa"],
         jobs=[{"rescue_roc": "a.fa"}] * 2 + [{}, {}]),
    dict(id="rescue-roc-fields", alleles=True, fields=[{"rescue_roc": "b.fa"}, {}, {}, {}], spec={"rescue_roc": {"genomes": [100, -1, -1, -1], "want": [1, 0, 0, 0]}},
         loads=["b.fa"], jobs=[{"rescue_roc": "b.fa"}, {}, {}, {}]),
    dict(id="atomize-true", alleles=True, kw=dict(atomize=True), dirs={"atoms"}, jobs=ATOMJ,
         spec={"atomize": {"want": [1, 1, 0, 0], "atoms": ["atoms/TM-1-1.x.c0.atoms.tsv", "atoms/TM-1-1.x.c1.atoms.tsv", None, None]}}),
    dict(id="atomize-list", alleles=True, kw=dict(atomize=[0, 1, 1, 1]), dirs={"atoms"}, jobs=[{}, ATOMJ[1], {}, {}],
         spec={"atomize": {"want": [0, 1, 0, 0], "atoms": [None, "atoms/TM-1-1.x.c1.atoms.tsv", None, None]}}),
    dict(id="atomize-fields", alleles=True, fields=[{"atomize": True}, {"atoms_out": "unused/a.tsv"}, {}, {}], spec={"atomize": {"want": [1, 0, 0, 0], "atoms": [None] * 4}},
         jobs=[{"atomize": True}, {"atoms_out": "unused/a.tsv"}, {}, {}]),
    dict(id="vartype-true", alleles=True, kw=dict(vartype=True), spec={"vartype": {"edges": EDGES, "want": [1, 1, 0, 0]}}, jobs=[{"vartype": EDGES}] * 2 + [{}, {}]),
    dict(id="vartype-edges", alleles=True, kw=dict(vartype=[1, 2, 4]), spec={"vartype": {"edges": (1, 2, 4), "want": [1, 1, 0, 0]}}, jobs=[{"vartype": (1, 2, 4)}] * 2 + [{}, {}]),
    dict(id="vartype-fields", alleles=True, fields=[{}, {"vartype": (1, 9)}, {"vartype": (1, 9)}, {}], spec={"vartype": {"edges": (1, 9), "want": [0, 1, 0, 0]}},
         jobs=[{}, {"vartype": (1, 9)}, {"vartype": (1, 9)}, {}]),
    dict(id="haplo-dict", alleles=True, kw=dict(haplo={"gap": 3, "genomes": ["a.fa", "a.fa", "b.fa", None]}), spec={"haplo": HAP}, loads=["a.fa"], dirs={"hap"}, jobs=HAPJ),
    dict(id="haplo-gap", alleles=True, fields=[{"haplo_genome": "a.fa"}, {"haplo_genome": "a.fa"}, {"haplo_genome": "b.fa"}, {}], kw=dict(haplo=3), spec={"haplo": HAP},
         loads=["a.fa"], dirs={"hap"}, jobs=HAPJ),
    dict(id="haplo-true", alleles=True, fields=[{"haplo_genome": "b.fa"}, {}, {}, {}], kw=dict(haplo=True), loads=["b.fa"], dirs={"hap"},
         spec={"haplo": {"gap": 10, "genomes": [100, -1, -1, -1], "sites": ["hap/TM-1-1.x.c0.sites.tsv", None, None, None], "seqs": [SEQ["b.fa"], None, None, None]}},
         jobs=[dict(haplo=10, haplo_genome="b.fa", sites_out="hap/TM-1-1.x.c0.sites.tsv"), {}, {}, {}]),
    dict(id="haplo-fields", alleles=True, fields=[{"haplo": 0, "haplo_genome": "a.fa"}, {"haplo": 0, "haplo_genome": "a.fa", "sites_out": "s/x.tsv"}, {"haplo_genome": "b.fa"}, {}],
         spec={"haplo": {"gap": 0, "genomes": [100, 100, -1, -1], "sites": [None, "s/x.tsv", None, None], "seqs": [None, SEQ["a.fa"], None, None]}}, loads=["a.fa"], dirs={"s"},
         jobs=[{"haplo": 0, "haplo_genome": "a.fa"}, {"haplo": 0, "haplo_genome": "a.fa", "sites_out": "s/x.tsv"}, {"haplo_genome": "b.fa"}, {}]),
    dict(id="hapsub", alleles=True, kw=dict(hapsub=True, haplo={"gap": 3, "genomes": ["a.fa", "a.fa", "b.fa", None]}), loads=["a.fa"], dirs={"hap"}, jobs=SUBJ,
         spec={"hapsub": dict(HAP, subsets=["hap/TM-1-1.x.c0.subsets.tsv", "hap/TM-1-1.x.c1.subsets.tsv", None, None])}),
    dict(id="hapsub-gap", alleles=True, fields=[{"haplo_genome": "a.fa"}, {"haplo_genome": "a.fa"}, {}, {}], kw=dict(hapsub=True, haplo=3), loads=["a.fa"], dirs={"hap"}, jobs=SUBJ,
         spec={"hapsub": dict(HAP, subsets=["hap/TM-1-1.x.c0.subsets.tsv", "hap/TM-1-1.x.c1.subsets.tsv", None, None])}),
    dict(id="hapsub-fields", alleles=True, fields=[{"hapsub": 1, "haplo_genome": "b.fa", "subsets_out": "s/sub.tsv"}, {"hapsub": 1, "haplo_genome": "b.fa"}, {}, {}], loads=["b.fa"], dirs={"s"},
         spec={"hapsub": {"gap": 1, "genomes": [100, 100, -1, -1], "sites": [None] * 4, "seqs": [SEQ["b.fa"], None, None, None], "subsets": ["s/sub.tsv", None, None, None]}},
         jobs=[{"hapsub": 1, "haplo_genome": "b.fa", "subsets_out": "s/sub.tsv"}, {"hapsub": 1, "haplo_genome": "b.fa"}, {}, {}]),
    dict(id="nothing", spec={}, jobs=[{}] * 4),
]


def run(case, tmp, eng):
    jobs = mk(tmp)
    for j, f in zip(jobs, case.get("fields") or ()):
        for k, v in absolute(f, tmp).items():
            setattr(j, k, v)
    out = extract_many(jobs, engine=eng, strict=True, alleles=case.get("alleles", False), **absolute(case.get("kw") or {}, tmp))
    assert out is jobs
    return jobs


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_what_the_engine_is_asked(case, tmp_path):
    eng = Stand()
    jobs = run(case, tmp_path, eng)
    want = dict({k: None for k in PASS_KEYS}, n_bins=256, alleles=case.get("alleles", False), strict=True, truth_slots=None, n_slots=0, global_dev=None)
    want.update(case["spec"])
    assert relative(eng.kw, tmp_path) == want
    pure = [False, False, True, True]
    assert relative(eng.fj, tmp_path) == [
        dict(vcf=n + ".vcf", truth=None if p else "t.vcf", mode="hcmv", pure=p, filtered=n + ".filtered.vcf", tp=None if p else "tp/" + n + ".tp.vcf", fp="fp/" + n + ".fp.vcf")
        for n, p in zip(("TM-1-1.x.c0", "TM-1-1.x.c1", "TM-1-0.x.c0", "TM-0-1.x.c0"), pure)]
    # every distinct FASTA once, with its bases; every id given out released once; the caller's engine stays open
    assert eng.loads == [SEQ[f] for f in case.get("loads", [])]
    assert sorted(eng.gone) == list(range(100, 100 + len(eng.loads)))
    assert eng.strata == case.get("strata", []) and eng.strata_gone == [7] * len(eng.strata)
    assert eng.closed == 0
    assert {p.name for p in tmp_path.iterdir() if p.is_dir()} == {"fp", "tp"} | case.get("dirs", set())
    assert not [p for p in tmp_path.rglob("*") if p.is_file() and p.name not in SEQ]
    for j, f, p, k in zip(jobs, case["jobs"], pure, range(4)):
        assert relative({n: getattr(j, n) for n in DEFAULT if getattr(j, n) != DEFAULT[n]}, tmp_path) == f
        assert j.tp_out == ("" if p else str(tmp_path / "tp" / (os.path.basename(j.vcf_file)[:-4] + ".tp.vcf")))
        assert j.stats == dict((case.get("rows") or [{}] * 4)[k], roc=None if p else "R%d" % k, pure_strain=p)
    assert extract_many.last_paths == {"unsorted": 0} and extract_many.last_phases == {"engine": 0.0}


@pytest.mark.parametrize("case", [c for c in CASES if c.get("loads") or c.get("strata")], ids=lambda c: c["id"])
def test_released_when_the_call_fails(case, tmp_path):
    eng = Stand(fail=True)
    with pytest.raises(RuntimeError, match="the call failed"):
        run(case, tmp_path, eng)
    assert eng.loads == [SEQ[f] for f in case.get("loads", [])] and sorted(eng.gone) == list(range(100, 100 + len(eng.loads)))
    assert eng.strata_gone == [7] * len(case.get("strata", [])) and eng.closed == 0


A, V0, V1 = "a.fa", "TM-1-1.x.c0.vcf", "TM-1-1.x.c1.vcf"
AGREE = {"profile": "profile: the profiled jobs of one call share one window and one pair of bin counts", "strata": "strata: the stratified jobs of one call share one strata set",
         "boot": "boot: the resampled jobs of one call share one window, window count, replicate count and seed", "explain": "explain: the explained jobs of one call share one radius",
         "haplo": "haplo: the jobs of one call share one gap", "hapsub": "hapsub: the jobs of one call share one gap",
         "vartype": "vartype: the typed jobs of one call share one list of size edges", "context": "context: the profiled jobs of one call share one half window and one GC bin count",
         "surface": "surface: the swept jobs of one call share one QUAL step and one pair of bin counts"}
TWO = {"profile": ((1, 2, 3), (1, 2, 4)), "strata": (STRATA, STRATA + STRATA), "boot": ((1, 2, 3, 4), (1, 2, 3, 5)), "explain": (1, 2), "haplo": (1, 2), "hapsub": (1, 2),
       "vartype": ((1, 2), (1, 3)), "context": ((1, 2), (1, 3)), "surface": ((1, 2, 3), (1, 2, 4))}
ALLELES = "needs the allele-extended mode (--alleles): a single-base batch "
GENOMES = "%s: TM-1-1.x.c0.vcf and TM-1-1.x.c1.vcf share the truth file t.vcf and name the genomes a.fa and b.fa (%s)"
HAPSUB = "hapsub (--hap-subsets) searches the sites of the haplotype pass: it needs haplo= (the gap, or the gap and the genomes) in the same call"
# id, keywords, Job fields, alleles, the message (paths relative to tmp_path)
REFUSALS = [
    ("votes-without-groups", dict(votes=True), None, False, "votes: groups (lists of job indices) are needed"),
    ("votes-lengths", dict(votes={"k": [1, 1]}, groups=[[0, 1]]), None, False, "votes: 2 levels / 1 files for 1 groups"),
    ("votes-empty-group", dict(votes=True, groups=[[]]), None, False, "a vote group holds 1 to 32 jobs, not 0"),
    ("votes-two-groups", dict(votes=True, groups=[[0], [0, 1]]), None, False, "job 0 sits in two vote groups"),
    ("votes-level", dict(votes={"k": [3]}, groups=[[0, 1]]), None, False, "vote group 0: consensus level 3 with 2 members"),
    ("votes-level-fields", {}, [{"vote_group": "a", "consensus_k": 2}, {}, {}, {}], False, "vote group 'a': consensus level 2 with 1 members"),
    ("votes-pure", dict(votes=True, groups=[[0, 2]]), None, False, "TM-1-0.x.c0.vcf: a pure-strain sample cannot be in a vote group (its truth is never read)"),
    ("groups-size", dict(groups=[[0, 1, 0, 1, 0, 1]]), None, False, "a truth-side group holds 1 to 5 jobs, not 6"),
    ("groups-two", dict(groups=[[0, 1], [1]]), None, False, "job 1 sits in two groups"),
    ("groups-pure", dict(groups=[[0, 3]]), None, False, "TM-0-1.x.c0.vcf: a pure-strain sample cannot be in a truth-side group (its truth is never read)"),
    ("explain-radius", dict(explain=99), None, False, "explain: radius 99 (0 to 64)"),
    ("surface-step", dict(surface={"q_step": 0}), None, False, "surface: q_step 0 (1 to 65536)"),
    ("context-length", dict(context={"genomes": [A]}), None, False, "context: 1 genomes entries for 4 jobs"),
    ("context-window", dict(context={"genomes": [A] * 4, "half_window": -1}), None, False, "context: half window -1 (0 to 1024)"),
    ("context-fields", {}, [{"context": (5, 2)}, {}, {}, {}], False, "TM-1-1.x.c0.vcf: Job.context without Job.context_genome (the FASTA the VCF was called against)"),
    ("normalize-length", dict(normalize=[A]), None, True, "normalize: 1 genomes entries for 4 jobs"),
    ("rescue-roc-length", dict(rescue_roc={"genomes": [A, A]}), None, True, "rescue_roc: 2 genomes entries for 4 jobs"),
    ("atomize-length", dict(atomize=[True]), None, True, "atomize: 1 entries for 4 jobs"),
    ("vartype-edges", dict(vartype=[2, 3]), None, True, "vartype: the first size edge is 2 (it must be 1: every variant has a size of at least 1)"),
    ("hapsub-without-haplo", dict(hapsub=True), None, True, HAPSUB),
    ("hapsub-haplo-false", dict(hapsub=True, haplo=False), None, True, HAPSUB),
    ("haplo-gap", dict(haplo=33), None, True, "haplo: the gap is an integer from 0 to 32, not 33"),
    ("haplo-length", dict(haplo={"genomes": [A]}), None, True, "haplo: 1 genomes entries for 4 jobs"),
    ("haplo-no-genome", dict(haplo=3), None, True, "haplo: no job names the genome its VCF was called against (Job.haplo_genome, or haplo={'genomes': [...]})"),
    ("haplo-fields", {}, [{"haplo": 3}, {}, {}, {}], True, "TM-1-1.x.c0.vcf: Job.haplo without Job.haplo_genome (the FASTA the VCF was called against)"),
    ("hapsub-fields", {}, [{}, {"hapsub": 3}, {}, {}], True, "TM-1-1.x.c1.vcf: Job.haplo without Job.haplo_genome (the FASTA the VCF was called against)"),
    ("genomes-length", dict(genomes=[A]), None, False, "genomes: 1 entries for 4 jobs"),
    ("profile-length", dict(profile={"want": [1], "points": [None] * 3}), None, False, "profile: 1 want / 3 points entries for 4 jobs"),
    ("haplo-two-genomes", dict(haplo={"genomes": [A, "b.fa", None, None]}), None, True, GENOMES % ("haplo", "the sites of a truth set belong to one genome")),
    ("hapsub-two-genomes", dict(hapsub=True, haplo={"genomes": [A, "b.fa", None, None]}), None, True, GENOMES % ("haplo", "the sites of a truth set belong to one genome")),
    ("normalize-two-genomes", dict(normalize=[A, "b.fa", None, None]), None, True, GENOMES % ("normalize", "a normalised truth set belongs to one genome")),
    ("rescue-roc-two-genomes", dict(rescue_roc=[A, "b.fa", None, None]), None, True, GENOMES % ("rescue_roc", "a normalised truth set belongs to one genome")),
    ("normalize-mode", dict(normalize=[A] * 4), None, False, "normalize (--normalize) " + ALLELES + "holds no indels or MNPs"),
    ("atomize-mode", dict(atomize=True), None, False, "atomize (--atomize) " + ALLELES + "holds no MNPs"),
    ("vartype-mode", dict(vartype=True), None, False, "vartype (--by-type) " + ALLELES + "holds SNVs only"),
    ("haplo-mode", dict(haplo={"genomes": [A] * 4}), None, False, "haplo (--haplotypes) " + ALLELES + "holds no indels, MNPs or complex records to replay"),
    ("hapsub-mode", dict(hapsub=True, haplo={"genomes": [A] * 4}), None, False, "hapsub (--hap-subsets) " + ALLELES + "holds no indels, MNPs or complex records to replay"),
    ("rescue-roc-mode", dict(rescue_roc=[A] * 4), None, False, "rescueroc (--rescue-roc) " + ALLELES + "has no rescue passes to sweep"),
    ("shared-call", dict(fn=True, explain=3), None, False, "nearmiss (explain) does not combine with truthside (fn / groups) in one call: it runs in a call of its own"),
    ("shared-call-fields", dict(surface=True), [{"boot": (1, 2, 3, 4)}, {}, {}, {}], False, "surface does not combine with boot in one call: it runs in a call of its own"),
    ("custom-mode-alleles", {}, [{"mode": "custom"}, {}, {}, {}], True, "the allele-extended mode needs VCF truth sets (hcmv mode)"),
    ("mode", {}, [{"mode": "other"}, {}, {}, {}], False, "data must be 'hcmv' or 'custom', got 'other'"),
    # two wrong at once: the one that spoke first still speaks first
    ("order-explain-before-atomize", dict(explain=99, atomize=[True]), None, True, "explain: radius 99 (0 to 64)"),
    ("order-normalize-before-haplo", dict(haplo=33, normalize=[A]), None, True, "normalize: 1 genomes entries for 4 jobs"),
    ("order-hapsub-before-genomes", dict(genomes=[A], hapsub=True), None, True, HAPSUB),
    ("order-keywords-before-shared-call", dict(fn=True, profile={"want": [1]}), None, False, "profile: 1 want / 4 points entries for 4 jobs"),
    ("order-shared-call-before-agree", dict(fn=True), [{"explain": 1}, {"explain": 2}, {}, {}], False,
     "nearmiss (explain) does not combine with truthside (fn / groups) in one call: it runs in a call of its own"),
    ("order-agree-before-mode", {}, [{"vartype": (1, 2)}, {"vartype": (1, 3)}, {}, {}], False, AGREE["vartype"]),
    ("order-mode-before-genome", {}, [{"haplo": 3}, {}, {}, {}], False, "haplo (--haplotypes) " + ALLELES + "holds no indels, MNPs or complex records to replay"),
    ("order-genomes-before-gpus", dict(normalize=[A, "b.fa", None, None], gpus=2), None, True, GENOMES % ("normalize", "a normalised truth set belongs to one genome")),
] + [("agree-" + f, {}, [{f: a}, {f: b}, {}, {}], True, AGREE[f]) for f, (a, b) in TWO.items()]


@pytest.mark.parametrize("name,kw,fields,alleles,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_word_for_word(name, kw, fields, alleles, message, tmp_path):
    eng = Stand()
    jobs = mk(tmp_path)
    for j, f in zip(jobs, fields or ()):
        for k, v in absolute(f, tmp_path).items():
            setattr(j, k, v)
    with pytest.raises(ValueError) as ei:
        extract_many(jobs, engine=None if "gpus" in kw else eng, strict=True, alleles=alleles, **absolute(kw, tmp_path))
    assert relative(str(ei.value), tmp_path) == message
    assert eng.kw is None and eng.loads == eng.gone and eng.closed == 0
    assert not [p for p in tmp_path.iterdir() if p.is_dir()]                     # said before a directory is made


def test_an_engine_and_several_gpus(tmp_path):
    with pytest.raises(ValueError) as ei:
        extract_many(mk(tmp_path), engine=Stand(), gpus=2)
    assert str(ei.value) == "gpus > 1 starts one process (and one engine) per GPU: do not pass an engine"


def test_pure_strain_jobs_alone_need_no_engine(tmp_path, monkeypatch):
    made = []

    def engine(device):
        made.append(device)
        return Stand()
    monkeypatch.setattr(extract, "Engine", engine)
    monkeypatch.delenv("QM_DEVICE", raising=False)
    text = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\nc\t3\t.\tA\tC\t50\tPASS\t.\n"
    for j in mk(tmp_path)[2:]:
        open(j.vcf_file, "w").write(text)
    jobs = extract_many(mk(tmp_path)[2:], strict=True)
    assert made == [] and extract_many.last_paths is None
    for j in jobs:
        assert j.stats["pure_strain"] is True and j.stats["roc"] is None and j.stats["fp_lines"] == 1 and j.tp_out == ""
        assert open(j.fp_out).read() == open(j.filtered_out).read() and not os.path.exists(str(tmp_path / "tp"))
    # the passes that also run on pure-strain samples ask for a context; the ones for mixed samples only do not
    for kw in (dict(explain=3), dict(surface=True), dict(fn=True), dict(atomize=True, alleles=True), dict(vartype=True, alleles=True),
               dict(normalize=["a.fa", "a.fa"], alleles=True), dict(rescue_roc=["a.fa", "a.fa"], alleles=True), dict(haplo={"genomes": ["a.fa", "a.fa"]}, alleles=True)):
        extract_many(mk(tmp_path)[2:], strict=True, **absolute(kw, tmp_path))
        assert made == []
    for n, kw in enumerate((dict(strata=[("all", [0], [100])]), dict(boot={}), dict(genomes=["a.fa", None]), dict(profile={"want": [1, 0]}),
                            dict(context={"genomes": [None, "b.fa"]}))):
        jobs = extract_many(mk(tmp_path)[2:], strict=True, **absolute(kw, tmp_path))
        assert made == [0] * (n + 1) and jobs[0].stats == {"roc": None, "pure_strain": True, **({"boot_cnt": "B0", "boot_params": BOOT, "boot_truth": True} if "boot" in kw else {})}
