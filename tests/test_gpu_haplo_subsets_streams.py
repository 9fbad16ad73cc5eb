"""The subset search (qm_batch_hapsubsets) on streams of the caller's: its row of PASS_EVENTS (ev_hapsub), with the
tools of tests/test_gpu_haplo_streams.py and tests/test_gpu_pass_streams.py (Hip, the comparisons).  Unlike the haplotype pass the
search reads nothing back: a call returns at once, so a bounded stall in front of it on its stream holds it in flight and the
waits can be pinned -- the run behind it on the device, the next haplotype call behind it on the host.  The answers, with
producer and consumer on different streams, against a reference run wholly on the context's stream (which
tests/test_gpu_haplo_subsets.py ties to the restatement)."""
import pytest

import test_gpu_haplo_subsets as TS
from test_gpu_haplo_streams import gpu   # noqa: F401  (the fixture: two streams with hardware queues of their own)
from test_gpu_pass_streams import base_results, refused, same

pytestmark = pytest.mark.gpu

OTHER_GAP = 0


@pytest.fixture(scope="module")
def world(engine, gpu):   # noqa: F811
    s = TS.Setup(engine)
    s.with_genome = [v for v, vc in enumerate(s.e.vcfs) if vc[3]]
    s.ref = {}
    for gap in (None, OTHER_GAP):
        s.b.haplotypes(s.genome_of, gap=gap, columns=True)
        hap = (s.b.haplotype_counts(), [s.b.haplotyped(v) for v in s.with_genome])
        s.b.hapsubsets(columns=True)
        s.ref[gap] = (hap, TS.fetch(s.b, s.with_genome))
    assert int(s.ref[None][1][0][s.e.index("main")][TS.U["partial"]]) == 13
    assert s.ref[None][1][0].tolist() != s.ref[OTHER_GAP][1][0].tolist()
    s.base = base_results(s.b)
    yield s
    gpu.drain()
    s.close()


def test_the_search_on_a_second_stream_behind_the_pass(gpu, world):   # noqa: F811
    """the pass on A, the search on B: the search's stream waits for ev_haplo, the getter for ev_hapsub"""
    b = world.b
    b.haplotypes(world.genome_of, columns=True, stream=gpu.A, fetch=False)
    b.hapsubsets(columns=True, stream=gpu.B, fetch=False)
    same(TS.fetch(b, world.with_genome), world.ref[None][1], "the search on B behind the pass on A")
    same((b.haplotype_counts(), [b.haplotyped(v) for v in world.with_genome]), world.ref[None][0], "the pass behind the search")
    b.haplotypes(world.genome_of, gap=OTHER_GAP, columns=True, stream=gpu.B, fetch=False)
    b.hapsubsets(columns=True, narrow_hash=True, stream=gpu.A, fetch=False)
    same(TS.fetch(b, world.with_genome), world.ref[OTHER_GAP][1], "the other gap: the pass on B, the search on A")
    gpu.drain()
    same(TS.fetch(b, world.with_genome), world.ref[OTHER_GAP][1], "both streams dry")


def test_a_run_behind_the_search_waits_for_it(gpu, world):   # noqa: F811
    """qm_batch_run on the context's stream behind a search stalled on A (the ev_hapsub row of PASS_EVENTS): the run returns at
    once and is ordered behind the search on the device, so the search is done when qm_batch_finish comes back; its results and
    the pass's are behind the latest run"""
    b = world.b
    b.haplotypes(world.genome_of, columns=True)
    b.hapsubsets(columns=True)                               # (its buffers exist: the stalled call below allocates nothing)
    gpu.stall(gpu.A)
    b.hapsubsets(columns=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    b.run()
    gpu.flying(ev, "the search behind qm_batch_run")       # asynchronous: the wait is the stream's
    refused(b.hapsubset_counts)
    b.finish()
    gpu.landed(ev, "the search behind qm_batch_finish")    # the run came behind the search
    refused(b.hapsubset_counts)
    refused(b.haplotype_counts)
    same(base_results(b), world.base, "the batch run again behind the search")
    b.haplotypes(world.genome_of, columns=True)
    b.hapsubsets(columns=True)
    same(TS.fetch(b, world.with_genome), world.ref[None][1], "a fresh search behind the new run")


def test_a_haplotype_call_behind_the_search_waits_and_forgets_it(gpu, world):   # noqa: F811
    """The next qm_batch_haplotypes rewrites what a search in flight reads (the pair lists, the class bytes, the descriptors it
    copies from the host): it waits for ev_hapsub on the host before it touches them.  Its own answers are the first ones again,
    the search's are gone until it runs again and then are what they were."""
    b = world.b
    b.haplotypes(world.genome_of, columns=True)
    b.hapsubsets(columns=True)
    gpu.stall(gpu.A)
    b.hapsubsets(columns=True, stream=gpu.A, fetch=False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "the search stalled on A")
    b.haplotypes(world.genome_of, gap=OTHER_GAP, columns=True, stream=gpu.B, fetch=False)
    gpu.landed(ev, "the search behind the next qm_batch_haplotypes")
    with pytest.raises(TS.QmvtError, match="no qm_batch_hapsubsets behind the latest qm_batch_haplotypes"):
        b.hapsubset_counts()
    same((b.haplotype_counts(), [b.haplotyped(v) for v in world.with_genome]), world.ref[OTHER_GAP][0], "the pass at the other gap")
    b.hapsubsets(columns=True, stream=gpu.B, fetch=False)
    same(TS.fetch(b, world.with_genome), world.ref[OTHER_GAP][1], "the search at the other gap")
    b.haplotypes(world.genome_of, columns=True, stream=gpu.A, fetch=False)
    same((b.haplotype_counts(), [b.haplotyped(v) for v in world.with_genome]), world.ref[None][0], "the first answers of the pass again")
    b.hapsubsets(columns=True, stream=gpu.A, fetch=False)
    same(TS.fetch(b, world.with_genome), world.ref[None][1], "the first answers of the search again")
