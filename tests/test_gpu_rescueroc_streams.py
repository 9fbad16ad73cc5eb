"""The rescue-ROC sweep (qm_batch_rescue_roc) on streams of the caller's: its row of PASS_EVENTS (ev_rroc), with the
tools of tests/test_gpu_pass_streams.py that tests/test_gpu_vartype_streams.py uses (Hip: two streams with hardware queues of
their own, a bounded stall, `flying` where a call must not have waited on the host, `landed` where it must have; the
comparisons).  The sweep reads nothing back: a call returns at once, so a stall in front of it on its stream holds it in flight.
The answers, with producers and consumer on different streams, against a reference run wholly on the context's stream (which
tests/test_gpu_rescueroc.py ties to the restatement)."""
import pytest

import rescueroc_family as fam
from quasimodo_amd import _lib
from quasimodo_amd._lib import QmvtError
from test_gpu_pass_streams import Hip, base_results, refused, same
from test_gpu_rescueroc import Run

pytestmark = pytest.mark.gpu

SIZES, WHICH = [0, 1, 257, 20000], [0, 1, 1, 0]


@pytest.fixture(scope="module")
def gpu(engine):
    h = Hip(engine)
    yield h
    h.close()


@pytest.fixture(scope="module")
def world(engine, gpu):
    tvs, truths, cols = fam.family(61, False, sizes=SIZES, which=WHICH, truth_n=[400, 65])
    run = Run(engine, fam.GENOMES, truths, cols, WHICH)
    run.ref = (run.roc_n, run.roc_a, run.base)
    assert int(run.roc_n[3][0][0]) > int(run.roc[3][0][0]) and int(run.roc_a[3][0][0]) > int(run.roc[3][0][0])
    run.base_ref = base_results(run.b)
    yield run
    gpu.drain()
    run.close()


def test_the_sweep_on_a_second_stream_behind_its_producers(gpu, world):
    """normalize on A, atomize on B, the sweep on the context's stream, then on A behind producers on B: the sweep's stream waits
    for ev_norm and ev_atom, the getter for ev_rroc"""
    b = world.b
    b.normalize(world.want_gids, columns=True, stream=gpu.A, fetch=False)
    b.atomize(columns=True, stream=gpu.B, fetch=False)
    b.rescue_roc(fetch=False)
    same(b.rescue_roc_counts(), world.ref, "the sweep behind normalize on A and atomize on B")
    b.normalize(world.want_gids, columns=True, stream=gpu.B, fetch=False)
    b.atomize(columns=True, stream=gpu.B, fetch=False)
    b.rescue_roc(stream=gpu.A, fetch=False)
    same(b.rescue_roc_counts(), world.ref, "the sweep on A behind both producers on B")
    gpu.drain()
    same(b.rescue_roc_counts(), world.ref, "both streams dry")


def test_the_sweep_behind_a_stalled_producer(gpu, world):
    """normalize behind a stall on A, the sweep on B: the call returns while the producer is held up, and its rows are right"""
    b = world.b
    b.normalize(world.want_gids, columns=True)
    b.atomize(columns=True)
    b.rescue_roc()                                           # (its buffers exist: the calls below allocate nothing)
    gpu.stall(gpu.A)
    b.normalize(world.want_gids, columns=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    b.rescue_roc(stream=gpu.B, fetch=False)
    gpu.flying(ev, "normalize behind qm_batch_rescue_roc")  # asynchronous: the wait for ev_norm is the stream's
    same(b.rescue_roc_counts(), world.ref, "the sweep on B behind normalize stalled on A")
    gpu.landed(ev, "normalize behind the sweep's getter")


def test_a_run_behind_the_sweep_waits_for_it(gpu, world):
    """qm_batch_run on the context's stream behind a sweep stalled on A (the ev_rroc row of PASS_EVENTS): the run returns at once
    and is ordered behind the sweep on the device, so the sweep is done when qm_batch_finish comes back"""
    b = world.b
    b.normalize(world.want_gids, columns=True)
    b.atomize(columns=True)
    b.rescue_roc()
    gpu.stall(gpu.A)
    b.rescue_roc(stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    b.run()
    gpu.flying(ev, "the sweep behind qm_batch_run")        # asynchronous: the wait is the stream's
    refused(b.rescue_roc_counts)
    b.finish()
    gpu.landed(ev, "the sweep behind qm_batch_finish")     # the run came behind the sweep
    refused(b.rescue_roc_counts)
    refused(b.normalize_counts)
    same(base_results(b), world.base_ref, "the batch run again behind the sweep")
    b.normalize(world.want_gids, columns=True)
    b.atomize(columns=True)
    same(b.rescue_roc(), world.ref, "a fresh sweep behind the new run")


@pytest.mark.parametrize("producer", ["normalize", "atomize"])
def test_a_producer_call_behind_the_sweep_waits_and_forgets_its_matching(gpu, world, producer):
    """The next call of a producer rewrites what a sweep in flight reads: it waits for ev_rroc on the host first.  The rows of its
    matching are gone until the sweep runs again and then are what they were; the other matching's stay."""
    b = world.b
    b.normalize(world.want_gids, columns=True)
    b.atomize(columns=True)
    b.rescue_roc()
    gpu.stall(gpu.A)
    b.rescue_roc(stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "the sweep stalled on A")
    if producer == "normalize":
        b.normalize(world.want_gids, columns=True, stream=gpu.B, fetch=False)
        gone, kept, k = _lib.QM_RROC_NORM, _lib.QM_RROC_ATOM, 1
    else:
        b.atomize(columns=True, stream=gpu.B, fetch=False)
        gone, kept, k = _lib.QM_RROC_ATOM, _lib.QM_RROC_NORM, 0
    gpu.landed(ev, "the sweep behind the next call of " + producer)
    with pytest.raises(QmvtError, match="did not sweep by"):
        b.rescue_roc_counts(gone)
    same(b.rescue_roc_counts(kept)[k], world.ref[k], "the other matching's rows")
    b.rescue_roc(stream=gpu.B, fetch=False)
    same(b.rescue_roc_counts(), world.ref, "the sweep again")
