"""The variant-type pass (qm_batch_types) on streams of the caller's: its row of PASS_EVENTS gets the checks
tests/test_gpu_pass_streams.py gives the other rows, by that module's method -- a bounded stall in front of the producer on the
producer's stream, `flying` where a call must not have waited on the host, `landed` where it must have -- and with its tools
(Hip, World, Pass, the comparisons).  The batch is test_gpu_vartype's (VCFs of 0, 1, 255, 256, 257 and 70 000 records, shuffled);
the reference is a second, identical batch run wholly on the context's stream and tied to quasimodo_amd.vartype.counts."""
import numpy as np
import pytest

import test_gpu_vartype as TV
from quasimodo_amd import vartype as vt
from test_gpu_pass_streams import Hip, Pass, World, base_results, refused, same

pytestmark = pytest.mark.gpu

OTHER_EDGES = (1, 2, 6)


@pytest.fixture(scope="module")
def gpu(engine):
    h = Hip(engine)
    yield h
    h.close()


class Types(World):
    """alter(): the large VCF backwards"""
    SEED, ALTERED = 79, 5

    def __init__(self, engine):
        self.engine = engine
        b, self.cols, _, self.truths, self.tids, self.shapes = TV.make_batch(engine, self.SEED, False)
        b.close()
        fetch = lambda b: (b.vartype_counts(), [b.vartyped(v) for v in range(b.n_vcf)])
        enqueue = lambda b, st, o: b.vartype(OTHER_EDGES if o else None, self.shapes, columns=True, stream=st, fetch=False)
        self.passes = {"vartype": Pass(enqueue, fetch, lambda b: b.vartype_timings(), has_other=True)}
        self.reference()

    def make(self):
        b = self.engine.batch(TV.SIZES, [self.tids[w] for w in TV.WHICH], alleles=True)
        for v, c in enumerate(self.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        return b

    def alter(self, b):
        b.upload(self.ALTERED, *[x[::-1].copy() for x in self.cols[self.ALTERED]])

    def anchor(self, b, variant, r):
        for name, edges in (("vartype", vt.DEFAULT_EDGES), ("vartype/other", OTHER_EDGES)):
            (rec, tru), rows = r[name]
            for v, (c, w) in enumerate(zip(self.cols, TV.WHICH)):
                if variant == 2 and v != self.ALTERED or v == self.ALTERED and variant == 1:
                    continue                              # (every VCF once: the large one as altered, its rows in the order it then has)
                c = [x[::-1] for x in c] if v == self.ALTERED else c
                cls = r["base"]["cls"][v]
                wrec, wtru, wrow = vt.counts(self.truths[w], c[0], c[1], c[2], c[4], (cls & 1).astype(bool), (cls & 2).astype(bool), edges, self.shapes)
                np.testing.assert_array_equal(rec[v], wrec, err_msg="%s rec of VCF %d" % (name, v))
                np.testing.assert_array_equal(tru[v], wtru, err_msg="%s tru of VCF %d" % (name, v))
                np.testing.assert_array_equal(rows[v], wrow, err_msg="%s rows of VCF %d" % (name, v))

    def close(self):
        for t in self.tids:
            self.engine.truth_release(t)


@pytest.fixture(scope="module")
def world(engine, gpu):
    w = Types(engine)
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


def test_pass_on_a_callers_stream_and_its_getter(gpu, world, fresh):
    b, p = fresh(), world.passes["vartype"]
    b.set_timing(True)
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "vartype")                                # asynchronous but for its small copies, which A does not hold up
    got = p.fetch(b)                                         # blocking: waits for the pass's event, recorded on A
    gpu.landed(ev, "vartype's getter")
    same(got, world.ref[1]["vartype"], "vartype")
    ms = p.timings(b)
    assert set(ms) == {"type_records_ms", "type_truth_ms"} and all(x >= 0 for x in ms.values()), ms
    same(base_results(b), world.ref[1]["base"], "the batch behind vartype")


def test_same_pass_twice_on_two_streams(gpu, world, fresh):
    """the second call (other edges, on B) waits on the host for the first (on A behind a stall) before its memsets touch the
    outputs both write: the getter returns the second call's answer, also when both streams have run dry"""
    b, p = fresh(), world.passes["vartype"]
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "the first vartype")
    p.enqueue(b, gpu.B, True)                                # blocking by pass_stream()
    gpu.landed(ev, "the first vartype behind the second call")
    same(p.fetch(b), world.ref[1]["vartype/other"], "the second vartype")
    gpu.drain()
    same(p.fetch(b), world.ref[1]["vartype/other"], "the second vartype, both streams dry")


def test_run_on_another_stream_waits_for_the_pass_in_flight(gpu, world, fresh):
    """The pass on A, its answer fetched; the pass again on A behind a stall, then qm_batch_run and qm_batch_finish on B: the run
    returns at once and is ordered behind the pass on the device (the new row of PASS_EVENTS), so the pass is done when the
    finish comes back; the first answer is what it was and a pass behind the new run gives it again."""
    b, p = fresh(), world.passes["vartype"]
    p.enqueue(b, gpu.A, False)
    first = p.fetch(b)
    same(first, world.ref[1]["vartype"], "the first vartype")
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    b.run(stream=gpu.B)
    gpu.flying(ev, "vartype behind qm_batch_run")          # asynchronous: the wait is the stream's
    refused(lambda: p.fetch(b))
    b.finish(stream=gpu.B)
    gpu.landed(ev, "vartype behind qm_batch_finish")       # the run (and so the stream finish waits for) came behind the pass
    refused(lambda: p.fetch(b))
    same(base_results(b), world.ref[1]["base"], "the batch run again behind vartype")
    same(first, world.ref[1]["vartype"], "the first answer, intact")
    p.enqueue(b, gpu.B, False)
    same(p.fetch(b), first, "a fresh vartype behind the new run")


def test_upload_and_run_behind_the_pass_in_flight(gpu, world, fresh):
    """other columns for one VCF behind the pass stalled on A, then run and finish: everything equals the reference for the new
    columns, and no result of the pass can be fetched until it runs again"""
    b, p = fresh(), world.passes["vartype"]
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "vartype")
    world.alter(b)                                           # blocking: returns when the passes in flight are done (include/qmvt.h)
    gpu.landed(ev, "vartype behind qm_batch_upload")
    b.run()
    refused(lambda: p.fetch(b))
    b.finish()
    refused(lambda: p.fetch(b))
    same(base_results(b), world.ref[2]["base"], "the new columns behind vartype")
    p.enqueue(b, None, False)
    same(p.fetch(b), world.ref[2]["vartype"], "a fresh vartype over the new columns")


def test_run_and_finish_on_a_pass_on_b(gpu, world, fresh):
    b, p = fresh(), world.passes["vartype"]
    gpu.stall(gpu.A)
    b.run(stream=gpu.A)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "qm_batch_run on A")
    b.finish(stream=gpu.A)                                   # "Wait for the stream"
    gpu.landed(ev, "the run behind qm_batch_finish")
    gpu.stall(gpu.B)
    p.enqueue(b, gpu.B, False)
    ev = gpu.mark(gpu.B)
    gpu.flying(ev, "vartype on B")
    same(p.fetch(b), world.ref[1]["vartype"], "vartype on B")
    same(base_results(b), world.ref[1]["base"], "the batch run on A")
