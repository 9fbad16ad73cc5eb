"""The match ladder per variant type and size (qm_batch_ladder_types) on streams of the caller's, with the tools
of tests/test_gpu_pass_streams.py that tests/test_gpu_ladder_streams.py uses (Hip: two streams with hardware queues of their own,
a bounded stall, `flying` where a call must not have waited on the host, `landed` where it must have; the comparisons).  The
pass reads nothing back: a call returns at once, so a stall in front of it on its stream holds it in flight.  The answers, with
producers and consumer on different streams, against a reference run wholly on the context's stream (which
tests/test_gpu_laddertypes.py ties to the restatement)."""
import numpy as np
import pytest

from haplo_family import truth_codes
from ladder_family import LadderFamily
from quasimodo_amd import ladder as ld
from test_gpu_laddertypes import Run
from test_gpu_pass_streams import Hip, refused, same

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
    run.rescues()
    produce(run)
    run.ref = run.b.ladder_types()
    assert all(run.ref[0][0][:, ld.CELL0 + m].any() for m in (ld.M_N, ld.M_A, ld.M_H, ld.M_B))
    yield run
    gpu.drain()
    run.close()


def produce(run, st=None, sl=None):
    """the two producers, each on its stream (None: the context's)"""
    run.b.vartype(columns=True, stream=st, fetch=False)
    run.b.ladder(subsets=True, columns=True, stream=sl, fetch=False)


def test_the_pass_on_a_second_stream_behind_its_producers(gpu, world):
    """types on A and the ladder on B, the pass on the context's stream; then both on B and the pass on A: its stream waits for
    the two done events, the getter for the pass's"""
    b = world.b
    produce(world, gpu.A, gpu.B)
    b.ladder_types(fetch=False)
    same(b.ladder_type_counts(), world.ref, "the pass behind types on A and the ladder on B")
    produce(world, gpu.B, gpu.B)
    b.ladder_types(stream=gpu.A, fetch=False)
    same(b.ladder_type_counts(), world.ref, "the pass on A behind both producers on B")
    gpu.drain()
    same(b.ladder_type_counts(), world.ref, "both streams dry")


@pytest.mark.parametrize("producer", ["types", "ladder"])
def test_the_pass_behind_a_stalled_producer(gpu, world, producer):
    """one producer behind a stall on A, the pass on B: the call returns while the producer is held up, and its blocks are right"""
    b = world.b
    produce(world)
    b.ladder_types()                                         # (its buffers exist: the calls below allocate nothing)
    gpu.stall(gpu.A)
    if producer == "types":
        b.vartype(columns=True, stream=gpu.A, fetch=False)
    else:
        b.ladder(subsets=True, columns=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    b.ladder_types(stream=gpu.B, fetch=False)
    gpu.flying(ev, producer + " behind qm_batch_ladder_types")   # asynchronous: the wait for the producer's event is the stream's
    same(b.ladder_type_counts(), world.ref, "the pass on B behind %s stalled on A" % producer)
    gpu.landed(ev, producer + " behind the pass's getter")


@pytest.mark.parametrize("producer", ["types", "ladder", "atomize"])
def test_a_producer_call_behind_the_pass_waits_and_forgets_its_rows(gpu, world, producer):
    """The next call of types or of the ladder -- or of a rescue underneath -- rewrites what a pass in flight reads: it waits for
    the pass's event on the host first.  The blocks are gone until the pass runs again and then are what they were."""
    b = world.b
    produce(world)
    b.ladder_types()
    gpu.stall(gpu.A)
    b.ladder_types(stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "the pass stalled on A")
    if producer == "types":
        b.vartype(columns=True, stream=gpu.B, fetch=False)
    elif producer == "ladder":
        b.ladder(subsets=True, columns=True, stream=gpu.B, fetch=False)
    else:
        b.atomize(columns=True, stream=gpu.B, fetch=False)
    gpu.landed(ev, "the pass behind the next call of " + producer)
    refused(b.ladder_type_counts)
    if producer == "atomize":
        b.ladder(subsets=True, columns=True, stream=gpu.B, fetch=False)
    b.ladder_types(stream=gpu.B, fetch=False)
    same(b.ladder_type_counts(), world.ref, "the pass again")
