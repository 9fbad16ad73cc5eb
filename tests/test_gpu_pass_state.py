"""The state every pass over a finished batch keeps (PassState in qmvt_batch.h, the helpers that handle it in qmvt_api.cpp;
DESIGN.md 4.13): what it made behind the latest run, whether it recorded timing marks, and the event its getters wait for.  One
table row per pass -- all sixteen of them -- says how the pass is enqueued, how its result is fetched, how its timings are read,
and the refusals of the library WORD FOR WORD: the strings below are the library's own, so a change of the host code that moves
a check, a message or the point where a pass forgets its result shows here, whatever the kernels compute.

Nothing depends on a kernel's result: two batches of two VCFs of 100 records each (a single-base one, an allele-extended one whose
truth set holds indels and an MNP) are enough, on an engine of the module's own -- the refusals of a genome id print how many
genomes the context holds, and only a context nobody else loads genomes into makes that number known."""
import math

import numpy as np
import pytest

import quasimodo_amd
import test_gpu_normalize as TN
from conftest import random_columns, random_truth
from quasimodo_amd import _lib
from quasimodo_amd._lib import ERRORS, QmvtError

pytestmark = pytest.mark.gpu

QM_E_INVAL, QM_E_STATE = -1, -6
N_REC = 100
GENOME_LEN = 2000                                  # of the single-base batch; the allele-extended one lives on TN.G600
BAD_GENOME = 99


def refused(fn, code, message):
    """fn() is refused with this code and exactly this message"""
    with pytest.raises(QmvtError) as ei:
        fn()
    assert ei.value.code == code and str(ei.value) == "%s (%d): %s" % (ERRORS[code], code, message), str(ei.value)


class World:
    """the module's engine, the inputs of the two batches and what they name"""

    def __init__(self):
        self.engine = quasimodo_amd.Engine(0)
        e, rng = self.engine, np.random.default_rng(4131)
        # single-base: one truth set for both VCFs, a genome for the first, frequencies for the first, three strata
        self.truth = random_truth(rng, 300, GENOME_LEN)
        self.tid = e.truth_load(*self.truth)
        self.cols = [random_columns(rng, N_REC, GENOME_LEN, self.truth) for _ in range(2)]
        self.af = rng.random(N_REC).astype(np.float32)
        self.gid = e.genome_load(bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, GENOME_LEN)]))
        self.sid = e.strata_load([("lo", [0], [800]), ("mid", [500, 1200], [900, 1500]), ("hi", [1400], [2 ** 31 - 1])])
        # allele-extended: 40 drawn entries (indels, most of them in repeats), a deletion and an MNP spelled out; both VCFs share the
        # truth set, the first names the genome, the second passes -1
        g = TN.G600
        tvs = TN.truth_variants(g, rng, 40)
        tvs += [(30, g[29:32], g[29]), (40, g[39:41], "".join("ACGT"[("ACGT".index(x) + 1) % 4] for x in g[39:41]))]
        self.xtid = e.truth_load(*TN.codes(tvs))
        self.xcols = [TN.record_columns(g, rng, N_REC, tvs, True) for _ in range(2)]
        self.xgid = e.genome_load(g.encode())
        self.gone = e.genome_load(b"ACGTACGTAC")   # a third genome, released: the context holds three slots from here on
        e.genome_release(self.gone)
        self.n_genomes = 3
        self.gids, self.xgids = [self.gid, -1], [self.xgid, -1]

    def make(self, kind):
        """a finished batch of its kind"""
        if kind == "single":
            b = self.engine.batch([N_REC] * 2, [self.tid] * 2)
            for v, c in enumerate(self.cols):
                b.upload(v, *c)
            b.upload_af(0, self.af)
        else:
            b = self.engine.batch([N_REC] * 2, [self.xtid] * 2, alleles=True)
            for v, c in enumerate(self.xcols):
                b.upload(v, *c)
        b.run()
        b.finish()
        return b

    def close(self):
        self.engine.close()


@pytest.fixture(scope="module")
def world(qmlib):
    w = World()
    yield w
    w.close()


@pytest.fixture
def batch_of(world):
    made = []

    def make(kind):
        made.append(world.make(kind))
        return made[-1]
    yield make
    for b in made:
        b.close()


class Row:
    """one pass: the batch it runs on, the passes it needs in front, the call that enqueues it, its getter and the getter's
    refusal while nothing was made behind the latest run; with timing marks: the timings method, how many values it returns, its
    refusal with timing off and its refusal behind a new run"""

    def __init__(self, kind, needs, enqueue, get, none, timings=None, n_ms=0, off=None, t_none=None):
        self.kind, self.needs, self.enqueue, self.get, self.none = kind, needs, enqueue, get, none
        self.timings, self.n_ms, self.off, self.t_none = timings, n_ms, off, t_none


def rows(w):
    latest = lambda getter, call: "%s: no %s behind the latest run" % (getter, call)
    off = lambda name: "%s: timing is off" % name
    both = _lib.QM_RROC_NORM | _lib.QM_RROC_ATOM
    return {
        "motifs": Row("single", [], lambda b: b.motifs(w.gids), lambda b: b.motif_counts(), latest("qm_batch_get_motifs", "qm_batch_motifs")),
        "af_profile": Row("single", [], lambda b: b.af_profile(64, 32, 10), lambda b: b.af_profile_counts(),
                          latest("qm_batch_get_af_profile", "qm_batch_af_profile")),
        "truth_hits": Row("single", [], lambda b: b.truth_hits(), lambda b: b.truth_hit_bits(0),
                          latest("qm_batch_get_truth_hits", "qm_batch_truth_hits")),
        "strata": Row("single", ["truth_hits"], lambda b: b.strata(w.sid, truth=True), lambda b: b.strata_counts(),
                      latest("qm_batch_get_strata", "qm_batch_strata")),
        # (Batch.boot_counts sizes its arrays by the Batch.boot in front of it and refuses by itself without one)
        "boot": Row("single", ["truth_hits"], lambda b: b.boot(64, 32, 10, seed=7, truth=True),
                    lambda b: b.boot_counts() if b._boot else b._ck(b._L.qm_batch_get_boot(b._h, None, None)),
                    latest("qm_batch_get_boot", "qm_batch_boot")),
        # (Batch.vote_counts asks qm_batch_vote_groups first: the getter itself, which copies nothing into NULL)
        "votes": Row("single", ["truth_hits"], lambda b: b.votes([[0, 1]]), lambda b: b._ck(b._L.qm_batch_get_votes(b._h, None, None, None, None, None)),
                     latest("qm_batch_get_votes", "qm_batch_votes"), lambda b: b.vote_timings(), 4,
                     "qm_batch_vote_timings: timing is off or no qm_batch_votes behind the latest run",
                     "qm_batch_vote_timings: timing is off or no qm_batch_votes behind the latest run"),
        "nearmiss": Row("single", ["truth_hits"], lambda b: b.nearmiss(3), lambda b: b.nearmiss_counts(),
                        latest("qm_batch_get_nearmiss", "qm_batch_nearmiss"), lambda b: b.nearmiss_timings(), 2,
                        off("qm_batch_nearmiss_timings"), latest("qm_batch_nearmiss_timings", "qm_batch_nearmiss")),
        "surface": Row("single", [], lambda b: b.surface(4, 32, 10, fetch=False), lambda b: b.surface_counts(),
                       latest("qm_batch_get_surface", "qm_batch_surface"), lambda b: b.surface_timings(), 3,
                       off("qm_batch_surface_timings"), latest("qm_batch_surface_timings", "qm_batch_surface")),
        "context": Row("single", ["truth_hits"], lambda b: b.context(w.gids, 50, 10, truth=True, fetch=False), lambda b: b.context_counts(),
                       latest("qm_batch_get_context", "qm_batch_context"), lambda b: b.context_timings(), 3,
                       off("qm_batch_context_timings"), latest("qm_batch_context_timings", "qm_batch_context")),
        "normalize": Row("alleles", [], lambda b: b.normalize(w.xgids, columns=True, fetch=False), lambda b: b.normalize_counts(),
                         latest("qm_batch_get_normalize", "qm_batch_normalize"), lambda b: b.normalize_timings(), 3,
                         off("qm_batch_normalize_timings"), latest("qm_batch_normalize_timings", "qm_batch_normalize")),
        "atomize": Row("alleles", [], lambda b: b.atomize(columns=True, fetch=False), lambda b: b.atomize_counts(),
                       latest("qm_batch_get_atomize", "qm_batch_atomize"), lambda b: b.atomize_timings(), 3,
                       off("qm_batch_atomize_timings"), latest("qm_batch_atomize_timings", "qm_batch_atomize")),
        "types": Row("alleles", [], lambda b: b.vartype(columns=True, fetch=False), lambda b: b.vartype_counts(),
                     latest("qm_batch_get_types", "qm_batch_types"), lambda b: b.vartype_timings(), 2,
                     off("qm_batch_types_timings"), latest("qm_batch_types_timings", "qm_batch_types")),
        "haplotypes": Row("alleles", [], lambda b: b.haplotypes(w.xgids, columns=True, fetch=False), lambda b: b.haplotype_counts(),
                          latest("qm_batch_get_haplotypes", "qm_batch_haplotypes"), lambda b: b.haplotype_timings(), 5,
                          off("qm_batch_haplotype_timings"), latest("qm_batch_haplotype_timings", "qm_batch_haplotypes")),
        # (with no haplotype pass behind the latest run the search's getters say so first: in front of the pass and behind a new
        #  run that is what they answer; "behind the latest qm_batch_haplotypes" is test_a_producer_called_again_...'s)
        "hapsubsets": Row("alleles", ["haplotypes"], lambda b: b.hapsubsets(columns=True, fetch=False), lambda b: b.hapsubset_counts(),
                          latest("qm_batch_get_hapsubsets", "qm_batch_haplotypes"), lambda b: b.hapsubset_timings(), 1,
                          off("qm_batch_hapsubset_timings"), latest("qm_batch_hapsubset_timings", "qm_batch_haplotypes")),
        "rescue_roc": Row("alleles", ["normalize", "atomize"], lambda b: b.rescue_roc(both, fetch=False), lambda b: b.rescue_roc_counts(both),
                          latest("qm_batch_get_rescue_roc", "qm_batch_rescue_roc") + " of its producers", lambda b: b.rescue_roc_timings(), 4,
                          off("qm_batch_rescue_roc_timings"), latest("qm_batch_rescue_roc_timings", "qm_batch_rescue_roc") + " of its producers"),
    }


PASSES = ["motifs", "af_profile", "truth_hits", "strata", "boot", "votes", "nearmiss", "surface", "context",
          "normalize", "atomize", "types", "haplotypes", "hapsubsets", "rescue_roc"]


def test_the_table_has_every_pass(world):
    assert sorted(rows(world)) == sorted(PASSES) and len(PASSES) == 15


@pytest.mark.parametrize("name", PASSES)
def test_made_timed_and_forgotten(world, batch_of, name):
    table = rows(world)
    row = table[name]
    b = batch_of(row.kind)
    refused(lambda: row.get(b), QM_E_STATE, row.none)                    # 1: nothing made yet
    for need in row.needs:
        table[need].enqueue(b)
    row.enqueue(b)
    row.get(b)                                                           # 2: served
    if row.timings:
        refused(lambda: row.timings(b), QM_E_STATE, row.off)             # 4: made, but without marks
        b.set_timing(True)
        row.enqueue(b)
        ms = row.timings(b)
        assert len(ms) == row.n_ms and all(math.isfinite(x) and x >= 0 for x in ms.values()), ms
        row.get(b)
    b.run()
    if row.timings:
        refused(lambda: row.timings(b), QM_E_STATE, row.t_none)          # 4: the marks belong to the run before
    b.finish()
    refused(lambda: row.get(b), QM_E_STATE, row.none)                    # 3: and so does the result


def test_a_producer_called_again_takes_its_consumers_result_back(world, batch_of):
    """normalize and atomize each clear their half of the rescue ROC, haplotypes clears the subset search"""
    t, b = rows(world), batch_of("alleles")
    N, A = _lib.QM_RROC_NORM, _lib.QM_RROC_ATOM
    swept = "qm_batch_get_rescue_roc: the latest qm_batch_rescue_roc did not sweep by %s"
    for again, lost, kept, how in (("normalize", N, A, "normal form"), ("atomize", A, N, "atoms")):
        for p in ("normalize", "atomize", "rescue_roc"):
            t[p].enqueue(b)
        assert all(x is not None for x in b.rescue_roc_counts(N | A))
        t[again].enqueue(b)
        refused(lambda: b.rescue_roc_counts(lost), QM_E_STATE, swept % how)
        refused(lambda: b.rescue_roc_counts(N | A), QM_E_STATE, swept % how)
        rn, ra, base = b.rescue_roc_counts(kept)                          # the other half alone is still served
        assert (rn is None) == (kept == A) and (ra is None) == (kept == N) and base.shape == (2, 2)
    t["normalize"].enqueue(b)                                             # (atomize was the last one called again: now both are gone)
    refused(lambda: b.rescue_roc_counts(N | A), QM_E_STATE, t["rescue_roc"].none)
    refused(lambda: b.rescue_roc_timings(), QM_E_STATE, t["rescue_roc"].t_none)
    stale = "%s: no qm_batch_hapsubsets behind the latest qm_batch_haplotypes"
    t["haplotypes"].enqueue(b)
    refused(lambda: b.hapsubset_counts(), QM_E_STATE, stale % "qm_batch_get_hapsubsets")   # (none yet, the same words)
    t["hapsubsets"].enqueue(b)
    assert b.hapsubset_counts().shape == (2, _lib.QM_HAPSUB_COLS)
    t["haplotypes"].enqueue(b)
    refused(lambda: b.hapsubset_counts(), QM_E_STATE, stale % "qm_batch_get_hapsubsets")
    refused(lambda: b.hapsubsetted(0), QM_E_STATE, stale % "qm_batch_get_hapsubsetted")
    refused(lambda: b.hapsubset_timings(), QM_E_STATE, stale % "qm_batch_hapsubset_timings")
    assert b.haplotype_counts()[0].shape == (2, _lib.QM_HAP_R_COLS)      # (its own result stands)


GENOME_CALLS = {
    "qm_batch_motifs": ("single", lambda b, g: b.motifs(g)),
    "qm_batch_context": ("single", lambda b, g: b.context(g, 50, 10, fetch=False)),
    "qm_batch_normalize": ("alleles", lambda b, g: b.normalize(g, fetch=False)),
    "qm_batch_haplotypes": ("alleles", lambda b, g: b.haplotypes(g, fetch=False)),
}


@pytest.mark.parametrize("call", sorted(GENOME_CALLS))
def test_genome_ids_are_checked(world, batch_of, call):
    kind, enqueue = GENOME_CALLS[call]
    b = batch_of(kind)
    live = world.gid if kind == "single" else world.xgid
    refused(lambda: enqueue(b, [live, BAD_GENOME]), QM_E_INVAL, "%s: VCF 1 names genome %d (have %d)" % (call, BAD_GENOME, world.n_genomes))
    refused(lambda: enqueue(b, [live, -2]), QM_E_INVAL, "%s: VCF 1 names genome -2 (have %d)" % (call, world.n_genomes))
    refused(lambda: enqueue(b, [live, world.gone]), QM_E_STATE, "%s: VCF 1 names released genome %d" % (call, world.gone))
    enqueue(b, [live, -1])                                               # (and the call that names what there is goes through)


@pytest.mark.parametrize("call,why", [("qm_batch_normalize", "a normalised truth set belongs to one genome"),
                                      ("qm_batch_haplotypes", "the sites of a truth set belong to one genome")],
                         ids=["qm_batch_normalize", "qm_batch_haplotypes"])
def test_vcfs_of_one_truth_set_name_one_genome(world, batch_of, call, why):
    b = batch_of("alleles")
    refused(lambda: GENOME_CALLS[call][1](b, [world.xgid, world.gid]), QM_E_INVAL,
            "%s: VCF 0 and VCF 1 share truth set %d and name genomes %d and %d (%s)" % (call, world.xtid, world.xgid, world.gid, why))


def test_batches_that_ran_every_pass_and_none_are_destroyed(world):
    """(the events of every pass and its timing marks go with the batch; a batch that never ran a pass has none)"""
    t = rows(world)
    for kind in ("single", "alleles"):
        b = world.make(kind)
        b.set_timing(True)
        for name in PASSES:
            if t[name].kind == kind:
                t[name].enqueue(b)
        b.close()
        world.engine.batch([N_REC] * 2, [world.tid if kind == "single" else world.xtid] * 2, alleles=kind == "alleles").close()
    b = world.make("single")                                             # the engine is whole behind them
    try:
        t["motifs"].enqueue(b)
        assert t["motifs"].get(b).shape == (2, 3, _lib.QM_MOTIF_COLS)
    finally:
        b.close()
