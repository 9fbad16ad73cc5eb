"""The ladder (qm_batch_ladder) on streams of the caller's: its row of PASSES (the wait list of everything that
rewrites what passes read), with the tools of tests/test_gpu_pass_streams.py that tests/test_gpu_rescueroc_streams.py uses (Hip:
two streams with hardware queues of their own, a bounded stall, `flying` where a call must not have waited on the host, `landed`
where it must have; the comparisons).  The pass reads nothing back: a call returns at once, so a stall in front of it on its
stream holds it in flight.  The answers, with producers and consumer on different streams, against a reference run wholly on the
context's stream (which tests/test_gpu_ladder.py ties to the restatement)."""
import numpy as np
import pytest

from haplo_family import truth_codes
from ladder_family import LadderFamily
from quasimodo_amd import ladder as ld
from test_gpu_ladder import Run
from test_gpu_pass_streams import Hip, base_results, refused, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(engine):
    h = Hip(engine)
    yield h
    h.close()


@pytest.fixture(scope="module")
def world(engine, gpu):
    f = LadderFamily(9)
    truth = truth_codes(f.truth)
    rng = np.random.default_rng(9)
    cols = [f.columns(), f.columns(rng), f.columns(keep=range(0, len(f.recs), 3))]
    run = Run(engine, [f.genome], [truth], cols, [0, 0, 0], hap_none=(2,))
    run.ref = run.b.ladder(subsets=True)
    assert all(ld.cells_with(run.ref[0][0], m) > 0 for m in (ld.M_N, ld.M_A, ld.M_H, ld.M_B))
    run.base_ref = base_results(run.b)
    yield run
    gpu.drain()
    run.close()


def produce(run, sn=None, sa=None, sh=None, ss=None):
    b = run.b
    b.normalize(run.gids_n, columns=True, stream=sn, fetch=False)
    b.atomize(columns=True, stream=sa, fetch=False)
    b.haplotypes(run.gids_h, columns=True, stream=sh, fetch=False)
    b.hapsubsets(columns=True, stream=ss, fetch=False)


def test_the_ladder_on_a_second_stream_behind_its_producers(gpu, world):
    """normalize and the haplotype pass on A, atomize and the search on B, the ladder on the context's stream, then on A behind
    all four on B: the ladder's stream waits for the four done events, the getter for the ladder's"""
    b = world.b
    produce(world, gpu.A, gpu.B, gpu.A, gpu.B)
    b.ladder(subsets=True, fetch=False)
    same(b.ladder_counts(), world.ref, "the ladder behind producers on A and B")
    produce(world, gpu.B, gpu.B, gpu.B, gpu.B)
    b.ladder(subsets=True, stream=gpu.A, fetch=False)
    same(b.ladder_counts(), world.ref, "the ladder on A behind all four producers on B")
    gpu.drain()
    same(b.ladder_counts(), world.ref, "both streams dry")


def test_the_ladder_behind_a_stalled_producer(gpu, world):
    """atomize behind a stall on A, the ladder on B: the call returns while the producer is held up, and its rows are right"""
    b = world.b
    produce(world)
    b.ladder(subsets=True)                                   # (its buffers exist: the calls below allocate nothing)
    gpu.stall(gpu.A)
    b.atomize(columns=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    b.ladder(subsets=True, stream=gpu.B, fetch=False)
    gpu.flying(ev, "atomize behind qm_batch_ladder")        # asynchronous: the wait for the producer's event is the stream's
    same(b.ladder_counts(), world.ref, "the ladder on B behind atomize stalled on A")
    gpu.landed(ev, "atomize behind the ladder's getter")


def test_a_run_behind_the_ladder_waits_for_it(gpu, world):
    """qm_batch_run on the context's stream behind a ladder stalled on A (its row of PASSES): the run returns at once and is
    ordered behind the ladder on the device, so the ladder is done when qm_batch_finish comes back"""
    b = world.b
    produce(world)
    b.ladder(subsets=True)
    gpu.stall(gpu.A)
    b.ladder(subsets=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    b.run()
    gpu.flying(ev, "the ladder behind qm_batch_run")        # asynchronous: the wait is the stream's
    refused(b.ladder_counts)
    b.finish()
    gpu.landed(ev, "the ladder behind qm_batch_finish")     # the run came behind the ladder
    refused(b.ladder_counts)
    same(base_results(b), world.base_ref, "the batch run again behind the ladder")
    produce(world)
    same(b.ladder(subsets=True), world.ref, "a fresh ladder behind the new run")


@pytest.mark.parametrize("producer", ["normalize", "atomize", "haplotypes", "hapsubsets"])
def test_a_producer_call_behind_the_ladder_waits_and_forgets_its_rows(gpu, world, producer):
    """The next call of a producer rewrites what a ladder in flight reads: it waits for the ladder's event on the host first.  The
    rows are gone until the ladder runs again and then are what they were."""
    b = world.b
    produce(world)
    b.ladder(subsets=True)
    gpu.stall(gpu.A)
    b.ladder(subsets=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "the ladder stalled on A")
    if producer == "normalize":
        b.normalize(world.gids_n, columns=True, stream=gpu.B, fetch=False)
    elif producer == "atomize":
        b.atomize(columns=True, stream=gpu.B, fetch=False)
    elif producer == "haplotypes":
        b.haplotypes(world.gids_h, columns=True, stream=gpu.B, fetch=False)
    else:
        b.hapsubsets(columns=True, stream=gpu.B, fetch=False)
    gpu.landed(ev, "the ladder behind the next call of " + producer)
    refused(b.ladder_counts)
    if producer == "haplotypes":
        b.hapsubsets(columns=True, stream=gpu.B, fetch=False)
    b.ladder(subsets=True, stream=gpu.B, fetch=False)
    same(b.ladder_counts(), world.ref, "the ladder again")
