"""The haplotype pass (qm_batch_haplotypes) on streams of the caller's: its row of PASS_EVENTS, with the tools of
tests/test_gpu_pass_streams.py (Hip, World, Pass, the comparisons) as tests/test_gpu_vartype_streams.py uses them.

One thing differs from the other passes and the cases say so where they stand.  The pass reads ONE number back in its middle (how
many (VCF, open site) pairs there are sizes their lists): the call waits on the host for its own stream there, so a stall in front
of it is over when the call returns (`landed`, not `flying`), and what is still in flight behind the call -- k_hap_pairs,
k_hap_claim, k_hap_replay -- is microseconds of work that no bounded stall can be put in front of.  What these cases pin is
therefore: the wait itself, on the right stream and on no other; the host-side rules of the row (a run forgets the pass, the
second call waits for the first, upload waits for the pass); and the answers, with producer and consumer on different streams,
against a reference run wholly on the context's stream and tied to quasimodo_amd.haplo.counts."""
import numpy as np
import pytest

import test_gpu_haplo as TH
from quasimodo_amd import haplo as hp
from test_gpu_pass_streams import Hip, Pass, World, base_results, refused, same

pytestmark = pytest.mark.gpu

OTHER_GAP = 0


@pytest.fixture(scope="module")
def gpu(engine):
    h = Hip(engine)
    yield h
    h.close()


class Haplo(World):
    """the batch of test_gpu_haplo; alter(): the shuffled family backwards"""
    ALTERED = 1

    def __init__(self, engine):
        self.engine = engine
        self.s = TH.Setup(engine)
        self.s.b.close()
        self.with_genome = [v for v, g in enumerate(self.s.genome_of) if g >= 0]
        fetch = lambda b: (b.haplotype_counts(), [b.haplotyped(v) for v in self.with_genome])
        enqueue = lambda b, st, o: b.haplotypes(self.s.genome_of, OTHER_GAP if o else None, columns=True, stream=st, fetch=False)
        self.passes = {"haplo": Pass(enqueue, fetch, lambda b: b.haplotype_timings(), has_other=True)}
        self.reference()

    def make(self):
        s = self.s
        b = self.engine.batch([len(c[0]) for c in s.cols], [s.tids[w] for w in s.which], alleles=True)
        for v, c in enumerate(s.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        return b

    def alter(self, b):
        b.upload(self.ALTERED, *[x[::-1].copy() for x in self.s.cols[self.ALTERED]])

    def anchor(self, b, variant, r):
        s = self.s
        for name, gap in (("haplo", None), ("haplo/other", OTHER_GAP)):
            (rec, tru), cols = r[name]
            for k, v in enumerate(self.with_genome):
                c = [x[::-1] for x in s.cols[v]] if v == self.ALTERED and variant == 2 else s.cols[v]
                cls = r["base"]["cls"][v]
                w = s.which[v]
                want = hp.counts(s.fam[w].genome, s.truths[w], c[0], c[1], c[2], c[4], (cls & 1).astype(bool), (cls & 2).astype(bool), gap)
                same(((rec[v], tru[v]), cols[k]), (want[:2], want[2:]), "%s of VCF %d, variant %d" % (name, v, variant))

    def close(self):
        s = self.s
        for t in s.tids:
            self.engine.truth_release(t)
        for g in s.gids:
            self.engine.genome_release(g)


@pytest.fixture(scope="module")
def world(engine, gpu):
    w = Haplo(engine)
    yield w
    w.close()


@pytest.fixture
def fresh(world, gpu):
    """a fresh finished batch of the world; closed behind the test once both streams are dry"""
    made = []

    def make():
        made.append(world.make())
        return made[-1]
    yield make
    gpu.drain()
    for b in made:
        b.close()


def test_pass_on_a_callers_stream_waits_for_that_stream_once(gpu, world, fresh):
    b, p = fresh(), world.passes["haplo"]
    b.set_timing(True)
    gpu.stall(gpu.A)
    ev = gpu.mark(gpu.A)
    gpu.stall(gpu.B)
    gpu.stall(gpu.B)                                         # (twice: still going when A's one stall and the pass are done)
    evb = gpu.mark(gpu.B)
    p.enqueue(b, gpu.A, False)
    gpu.landed(ev, "the readback of the pair count, on the pass's stream")
    gpu.flying(evb, "the pass on A: it waited for B as well")
    got = p.fetch(b)
    same(got, world.ref[1]["haplo"], "haplo")
    ms = p.timings(b)
    assert set(ms) == {"hap_sites_ms", "hap_records_ms", "hap_truth_ms", "hap_claim_ms", "hap_replay_ms"} and all(x >= 0 for x in ms.values()), ms
    same(base_results(b), world.ref[1]["base"], "the batch behind haplo")


def test_same_pass_twice_on_two_streams(gpu, world, fresh):
    """the second call (another gap, on B) finds the first (on A) done or waits for it on the host (pass_stream) before its memsets
    touch the outputs both write: the getter returns the second call's answer, also when both streams have run dry"""
    b, p = fresh(), world.passes["haplo"]
    p.enqueue(b, gpu.A, False)
    p.enqueue(b, gpu.B, True)
    same(p.fetch(b), world.ref[1]["haplo/other"], "the second haplo")
    gpu.drain()
    same(p.fetch(b), world.ref[1]["haplo/other"], "the second haplo, both streams dry")
    p.enqueue(b, gpu.A, False)
    same(p.fetch(b), world.ref[1]["haplo"], "the usual gap again, on A")


def test_run_on_another_stream_behind_the_pass(gpu, world, fresh):
    """The pass on A, its answer fetched; the pass again on A, then qm_batch_run and qm_batch_finish on B, ordered behind the
    pass's event (the new row of PASS_EVENTS): no answer can be fetched behind the run, the batch is what the reference is, the
    first answer is what it was and a pass behind the new run gives it again."""
    b, p = fresh(), world.passes["haplo"]
    p.enqueue(b, gpu.A, False)
    first = p.fetch(b)
    same(first, world.ref[1]["haplo"], "the first haplo")
    p.enqueue(b, gpu.A, False)
    b.run(stream=gpu.B)
    refused(lambda: p.fetch(b))
    b.finish(stream=gpu.B)
    refused(lambda: p.fetch(b))
    same(base_results(b), world.ref[1]["base"], "the batch run again behind haplo")
    same(first, world.ref[1]["haplo"], "the first answer, intact")
    p.enqueue(b, gpu.B, False)
    same(p.fetch(b), first, "a fresh haplo behind the new run")


def test_upload_and_run_behind_the_pass(gpu, world, fresh):
    """other columns for one VCF behind the pass on A, then run and finish: everything equals the reference for the new columns,
    and no result of the pass can be fetched until it runs again"""
    b, p = fresh(), world.passes["haplo"]
    p.enqueue(b, gpu.A, False)
    world.alter(b)                                           # blocking: returns when the passes in flight are done (include/qmvt.h)
    b.run()
    refused(lambda: p.fetch(b))
    b.finish()
    refused(lambda: p.fetch(b))
    same(base_results(b), world.ref[2]["base"], "the new columns behind haplo")
    p.enqueue(b, None, False)
    same(p.fetch(b), world.ref[2]["haplo"], "a fresh haplo over the new columns")


def test_run_and_finish_on_a_pass_on_b(gpu, world, fresh):
    b, p = fresh(), world.passes["haplo"]
    gpu.stall(gpu.A)
    b.run(stream=gpu.A)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "qm_batch_run on A")
    b.finish(stream=gpu.A)                                   # "Wait for the stream"
    gpu.landed(ev, "the run behind qm_batch_finish")
    p.enqueue(b, gpu.B, False)
    same(p.fetch(b), world.ref[1]["haplo"], "haplo on B")
    same(base_results(b), world.ref[1]["base"], "the batch run on A")
