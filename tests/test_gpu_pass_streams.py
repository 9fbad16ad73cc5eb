"""The batch passes on streams of the caller's, and the ordering between streams that qmvt_api.cpp keeps from the two tables of
qmvt_batch.h, PASSES and READS (include/qmvt.h at qm_batch_run): pass_open()'s host wait, the readers' wait for
the hit bitmaps' event (pass_wait), the wait list of everything that rewrites what passes read (wait_passes), the getters' wait
for their pass.

The method.  A missing wait between two streams shows only while the producer is still running when the consumer is enqueued.
Every case therefore puts a BOUNDED STALL in front of the producer, on the producer's stream: work that is long, touches nothing
of the batch, and ends by itself (nothing the host must release, so nothing that can hang the card).

The stall used: a run of hipMemsetAsync calls over a scratch allocation of this module's own (STALL_BYTES each), through the
ctypes handle of the HIP runtime the library is linked against (_hip_runtime of test_gpu_allele_byte, its function list extended
here).  torch.cuda._sleep is not used: the torch wheel carries a HIP runtime of its own under the library's soname, so which copy
a process ends up with depends on what was imported first, and a stream handle of one runtime means nothing to the other.  How
many memsets make STALL_MS is measured once per module with a HIP event pair, and so is one whole stall.

The streams: two of the test's own, created with hipStreamNonBlocking like the context's, so that the small blocking hipMemcpy
calls inside votes, strata, boot, context, normalize, atomize and af_profile do not join them by themselves -- and CHOSEN BY
MEASUREMENT among eight candidates so that their hardware queues do not do it either (Hip._pick_streams says how and why).

No silent pass.  `flying(ev)` asserts that an event recorded behind the producer still reports hipErrorNotReady:
  * behind every ASYNCHRONOUS consumer call, when it has returned;
  * in front of every BLOCKING consumer call (a getter, qm_batch_upload, the second call of one pass, whose pass_stream() waits on
    the host for the first), with `landed(ev)` behind it: the call did wait.
A case whose producer was already done fails.  Two cases cannot hold an overlap behind the consumer by the header's own words and
say so where they stand: the blocking upload of case 5 ("the blocking ones ... return when those passes are done") and the
upload + run + finish of case 3 (the same sentence; qm_batch_finish: "Wait for the stream").

The reference of every comparison is a second, identical batch on the same engine, run wholly on the context's stream with a
getter (a host wait) behind every call.  Three of its answers are tied to a restatement here, so the module does not rest on the
library alone: the hit bitmaps (quasimodo_amd.truthside.snp_keys over the kept rows as text), the atomize counts
(quasimodo_amd.atomize.counts) and the normalize counts (quasimodo_amd.normalize.counts).  Everything is an integer: every
comparison is exact."""
import ctypes as C
import math
import time

import numpy as np
import pytest

import test_gpu_atomize as TA
import test_gpu_normalize as TN
from conftest import random_columns, random_truth
from quasimodo_amd import atomize as at
from quasimodo_amd import normalize as nz
from quasimodo_amd import truthside as ts
from quasimodo_amd._lib import SCALAR_NAMES, QmvtError
from test_gpu_allele_byte import _hip_runtime

pytestmark = pytest.mark.gpu

QM_E_STATE = -6
HIP_SUCCESS, HIP_NOT_READY = 0, 600                # hipSuccess, hipErrorNotReady
HIP_STREAM_NON_BLOCKING = 1                        # as the context's own streams (qm_init)
HIP_EVENT_DISABLE_TIMING = 2

# The length of a stall.  Measured on one MI355X (LABNOTES.md, "pass streams"), host time on the context's stream: the slowest
# asynchronous consumer call 0.16 ms (qm_batch_votes, first use: it allocates and copies its tables), the slowest blocking one
# 5.4 ms (qm_batch_finish of the allele-extended batch with its 70 000 shuffled records; the atomize getters 3.1 ms).  20 x the
# slowest of all is 108 ms: above the floor of 20 ms, under the cap of 200.
STALL_MS = 110.0
STALL_CAP_MS = 200.0
STALL_BYTES = 1 << 30                              # one memset of the stall
LANDED_GRACE_MS = 5.0
PROBE_MEMSETS = 64                                 # the short stall that finds which streams share a hardware queue: about 10 ms


# ---- the HIP runtime: streams, events, the stall ---------------------------------------------------------------------------
class Hip:
    def __init__(self, engine):
        hip = _hip_runtime()
        sig = {"hipStreamCreateWithFlags": [C.c_void_p, C.c_uint], "hipEventCreateWithFlags": [C.c_void_p, C.c_uint],
               "hipEventCreate": [C.c_void_p], "hipEventRecord": [C.c_void_p, C.c_void_p], "hipEventQuery": [C.c_void_p],
               "hipEventSynchronize": [C.c_void_p], "hipEventDestroy": [C.c_void_p],
               "hipEventElapsedTime": [C.POINTER(C.c_float), C.c_void_p, C.c_void_p],
               "hipMalloc": [C.c_void_p, C.c_size_t], "hipFree": [C.c_void_p], "hipMemcpy": [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int],
               "hipMemsetAsync": [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]}
        for fn, args in sig.items():
            getattr(hip, fn).restype = C.c_int
            getattr(hip, fn).argtypes = args
        self.hip = hip
        self.events = []
        self.scratch = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.scratch), STALL_BYTES) == 0 and self.scratch.value
        self.A = self.B = None
        self.A, self.B = self._pick_streams(engine)
        # how many memsets make STALL_MS (and a tenth more): sixteen of them between two events, once, behind a first run that
        # loads the fill kernel
        self.n_memsets = 16
        self.stall_ms(self.A)
        per = self.stall_ms(self.A) / 16
        self.n_memsets = max(int(math.ceil(1.1 * STALL_MS / per)), 1)
        self.measured_ms = self.stall_ms(self.A)   # one whole stall, as the cases enqueue it

    def _stream(self):
        st = C.c_void_p()
        assert self.hip.hipStreamCreateWithFlags(C.byref(st), HIP_STREAM_NON_BLOCKING) == 0 and st.value
        return st.value

    def _held_up(self, stream, fn):
        """does the host call fn() wait for work on `stream`?  (a stall of about PROBE_MS there; held up: half of that)"""
        self.n_memsets = PROBE_MEMSETS
        ev = [C.c_void_p(), C.c_void_p()]
        for x in ev:
            assert self.hip.hipEventCreate(C.byref(x)) == 0
        assert self.hip.hipEventRecord(ev[0], stream) == 0
        self.stall(stream)
        assert self.hip.hipEventRecord(ev[1], stream) == 0
        t0 = time.perf_counter()
        fn()
        took = (time.perf_counter() - t0) * 1e3
        assert self.hip.hipEventSynchronize(ev[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
        for x in ev:
            assert self.hip.hipEventDestroy(x) == 0
        return took > 0.5 * ms.value

    def _pick_streams(self, engine):
        """Two streams of the test's own whose HARDWARE QUEUES make the cases decisive.  The runtime spreads a process's streams
        over GPU_MAX_HW_QUEUES queues (4 unless the environment says otherwise), and a queue runs what it is given in order,
        whatever streams it came from.  Here the null stream (the library's small blocking hipMemcpy calls), the context's two
        streams and the two of this module make five.  A stream that shares its queue with the null stream makes every blocking
        copy inside an entry point wait for the stall; one that shares it with the stream of its consumer orders the two by
        itself and hides a missing wait.  Measured, not assumed: of eight candidates,
          A is the first that holds up neither a blocking copy nor a run + finish on the context's streams,
          B the first other one that holds up no blocking copy and is not held up behind A.
        (B may share a queue with one of the context's streams: no case has them race.)"""
        tid = engine.truth_load(np.array([1], np.int32), np.array([0], np.int32), np.array([1], np.int32))
        b = engine.batch([256], [tid])
        host = np.zeros(8, np.uint8)
        try:
            z = np.zeros(256, np.int32)
            b.upload(0, z + 1, z, z + 1, z.astype(np.float32), z.astype(np.uint8))
            b.run()
            b.finish()
            copy = lambda: self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.scratch, 8, 2)   # hipMemcpyDeviceToHost
            rerun = lambda: (b.run(), b.finish())
            cand = [self._stream() for _ in range(8)]
            self._held_up(cand[0], copy)                 # (loads the fill kernel)
            free = [x for x in cand if not self._held_up(x, copy)]
            a = next((x for x in free if not self._held_up(x, rerun)), None)
            assert a is not None, "no stream with a hardware queue apart from the null stream's and the context's (GPU_MAX_HW_QUEUES < 4?)"

            def behind_a(x):
                ev = C.c_void_p()
                assert self.hip.hipEventCreate(C.byref(ev)) == 0
                try:
                    return self._held_up(a, lambda: (self.hip.hipEventRecord(ev, x), self.hip.hipEventSynchronize(ev)))
                finally:
                    assert self.hip.hipEventDestroy(ev) == 0
            bb = next((x for x in free if x != a and not behind_a(x)), None)
            assert bb is not None, "no second stream with a hardware queue apart from the first one's and the null stream's"
            for x in cand:
                if x not in (a, bb):
                    assert self.hip.hipStreamDestroy(x) == 0
            return a, bb
        finally:
            b.close()
            engine.truth_release(tid)

    def stall(self, stream):
        """the bounded stall: n_memsets memsets of the scratch allocation on `stream`; returns at once"""
        for _ in range(self.n_memsets):
            assert self.hip.hipMemsetAsync(self.scratch, 0, STALL_BYTES, stream) == 0

    def stall_ms(self, stream):
        e = [C.c_void_p(), C.c_void_p()]
        for x in e:
            assert self.hip.hipEventCreate(C.byref(x)) == 0
        assert self.hip.hipEventRecord(e[0], stream) == 0
        self.stall(stream)
        assert self.hip.hipEventRecord(e[1], stream) == 0 and self.hip.hipEventSynchronize(e[1]) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), e[0], e[1]) == 0
        for x in e:
            assert self.hip.hipEventDestroy(x) == 0
        return float(ms.value)

    def mark(self, stream):
        """an event recorded on `stream` now: behind everything enqueued there so far"""
        e = C.c_void_p()
        assert self.hip.hipEventCreateWithFlags(C.byref(e), HIP_EVENT_DISABLE_TIMING) == 0
        assert self.hip.hipEventRecord(e, stream) == 0
        self.events.append(e)
        return e

    def flying(self, ev, what):
        """the overlap held: what was enqueued in front of `ev` is not done"""
        rc = self.hip.hipEventQuery(ev)
        assert rc in (HIP_SUCCESS, HIP_NOT_READY), "hipEventQuery: %d" % rc
        assert rc == HIP_NOT_READY, "%s: the producer was already done, the case tested nothing" % what

    def landed(self, ev, what):
        """What was enqueued in front of `ev` was done when the call in front of this returned.  (`ev` sits on its stream
        straight behind the event that call waited for and may retire a moment after it: asked for up to LANDED_GRACE_MS,
        an eighth of what a stall that is still going would take.)"""
        t0 = time.perf_counter()
        rc = self.hip.hipEventQuery(ev)
        while rc == HIP_NOT_READY and (time.perf_counter() - t0) * 1e3 < LANDED_GRACE_MS:
            rc = self.hip.hipEventQuery(ev)
        assert rc == HIP_SUCCESS, "%s: still in flight (hipEventQuery: %d)" % (what, rc)

    def drain(self):
        for st in (self.A, self.B):
            assert self.hip.hipStreamSynchronize(st) == 0
        for e in self.events:
            assert self.hip.hipEventDestroy(e) == 0
        self.events = []

    def close(self):
        self.drain()
        assert self.hip.hipFree(self.scratch) == 0
        for st in (self.A, self.B):
            assert self.hip.hipStreamDestroy(st) == 0


@pytest.fixture(scope="module")
def gpu(engine):
    h = Hip(engine)
    yield h
    h.close()


def test_the_stall_is_as_long_as_the_module_says(gpu):
    """one whole stall between two HIP events: at least STALL_MS, so 20 x the slowest consumer call, and under the cap"""
    print("stall: %d memsets of %d MiB, %.1f ms on the device" % (gpu.n_memsets, STALL_BYTES >> 20, gpu.measured_ms))
    assert 20.0 <= STALL_MS <= gpu.measured_ms <= STALL_CAP_MS


# ---- comparing whatever a getter returns --------------------------------------------------------------------------------------
def flat(x):
    if x is None:
        return []
    if isinstance(x, dict):
        return [a for k in sorted(x) for a in flat(x[k])]
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in flat(y)]
    return [np.asarray(x)]


def same(got, want, what):
    got, want = flat(got), flat(want)
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg="%s, array %d" % (what, i))


def refused(fn):
    with pytest.raises(QmvtError) as ei:
        fn()
    assert ei.value.code == QM_E_STATE and "latest run" in str(ei.value), str(ei.value)


# ---- a pass: how it is enqueued (with its usual parameters or with others), fetched, timed -------------------------------------
class Pass:
    def __init__(self, enqueue, fetch, timings=None, reads_hits=False, has_other=False):
        self.enqueue, self.fetch, self.timings, self.reads_hits, self.has_other = enqueue, fetch, timings, reads_hits, has_other


def base_results(b):
    """what run + finish leave: class bytes, the TP line indices in front of each VCF's idx region and the FP ones at its end
    (what lies between is not defined), ROC rows, scalars, per-truth sums"""
    sc = b.scalars()
    tp, fp = SCALAR_NAMES.index("tp_lines"), SCALAR_NAMES.index("fp_lines")
    idx = [b.idx(v) for v in range(b.n_vcf)]
    return {"cls": [b.cls(v) for v in range(b.n_vcf)], "tp_idx": [np.sort(x[:int(sc[v, tp])]) for v, x in enumerate(idx)],
            "fp_idx": [np.sort(x[len(x) - int(sc[v, fp]):]) for v, x in enumerate(idx)], "roc": b.roc(), "scalars": sc,
            "global": b.global_counts()[np.unique(b.truth_ids)]}   # (the rows of its own truth sets: the context may hold others)


class World:
    """the inputs of one kind of batch: make() a finished batch of them on the context's stream, alter() one VCF's columns,
    the passes it accepts, and the reference answers ref[variant][name] (variant 1: as made; 2: altered, run and finished)"""

    def reference(self):
        self.ref = {}
        b = self.make()
        try:
            for variant in (1, 2):
                if variant == 2:
                    self.alter(b)
                    b.run()
                    b.finish()
                r = {"base": base_results(b)}
                for name, p in self.passes.items():           # (truth_hits comes first: its readers follow)
                    p.enqueue(b, None, False)
                    r[name] = p.fetch(b)
                    if p.has_other:
                        p.enqueue(b, None, True)
                        r[name + "/other"] = p.fetch(b)
                        p.enqueue(b, None, False)             # leave the usual answer behind, as the cases do
                self.anchor(b, variant, r)
                self.ref[variant] = r
        finally:
            b.close()

    def anchor(self, b, variant, r):
        pass


# ---- the single-base world -----------------------------------------------------------------------------------------------------
GENOME_LEN = 50_000
SIZES = [0, 1, 257, 70_000]                        # the empty VCF; 257: across the alignment of a VCF; 70 000: spans, workgroups
SORTED = [True, True, False, True]
WHICH = [0, 1, 0, 1]                               # two truth sets, each shared by two VCFs
WITH_AF = [2, 3]
ALTERED = 3                                        # the VCF whose columns alter() replaces: shuffled ones, through the bucket path
GROUPS, OTHER_GROUPS = [[0, 2], [1, 3]], [[3, 1]]
BASES = (b"A", b"C", b"G", b"T")


def truth_keys(truth):
    tp, tr, ta = (np.asarray(x, np.int64) for x in truth)
    ok = (tr >= 0) & (tr < 4) & (ta >= 0) & (ta < 4)
    return np.unique((tp[ok] << 4) | (tr[ok] << 2) | ta[ok])


def hits_by_truthside(cols, truth):
    """the hit bits of one VCF by the text rule of quasimodo_amd.truthside: its kept rows that have a key, written as VCF rows;
    a truth key is hit when snp_keys of that text holds it"""
    pos, ref, alt, _, fl = cols
    ok = (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4) & ((fl & 1) != 0) & ((fl & 4) == 0)
    text = b"\n".join(b"x\t%d\t.\t%s\t%s\t.\t.\t." % (p, BASES[r], BASES[a]) for p, r, a in zip(pos[ok].tolist(), ref[ok].tolist(), alt[ok].tolist()))
    keys = ts.snp_keys(text)
    return np.array([(b"%d" % (k >> 4), BASES[(k >> 2) & 3], BASES[k & 3]) in keys for k in truth_keys(truth).tolist()], bool)


class SingleBase(World):
    def __init__(self, engine):
        self.engine = engine
        rng = np.random.default_rng(9001)
        self.truths = [random_truth(rng, 3000, GENOME_LEN), random_truth(rng, 5000, GENOME_LEN)]
        self.tids = [engine.truth_load(*t) for t in self.truths]
        self.cols = [random_columns(rng, n, GENOME_LEN, self.truths[w], sorted_=s) for n, w, s in zip(SIZES, WHICH, SORTED)]
        self.other_cols = random_columns(rng, SIZES[ALTERED], GENOME_LEN, self.truths[WHICH[ALTERED]], frac_truth=0.5, sorted_=False)
        self.af = {v: np.where(rng.random(SIZES[v]) < 0.1, np.nan, rng.random(SIZES[v])).astype(np.float32) for v in WITH_AF}
        self.gid = engine.genome_load(bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, GENOME_LEN)]))
        self.gids = [self.gid, -1, self.gid, self.gid]
        self.sid = engine.strata_load([("lo", [0], [20_000]), ("mid", [10_000, 30_000], [25_000, 40_000]), ("hi", [35_000], [2 ** 31 - 1])])
        engine.genome_context(self.gid, 50, 10)    # the table qm_batch_context would build and wait for (include/qmvt.h)
        g, s = self.gids, self.sid
        hits = lambda b: ([b.truth_hit_bits(v) for v in range(b.n_vcf)], [b.intruth_mask(v) for v in range(b.n_vcf)],
                          b.truth_regions(GROUPS, union=True))
        votes = lambda b: (b.vote_counts(), [b.vote_keys(k) for k in range(len(b.vote_counts()["nokey"]))])
        nearmiss = lambda b: (b.nearmiss_counts(), [b.nearmiss_classes(v) for v in range(b.n_vcf)], [b.nearmiss_truth(v) for v in range(b.n_vcf)])
        self.passes = {
            "truth_hits": Pass(lambda b, st, o: b.truth_hits(stream=st), hits),
            "motifs": Pass(lambda b, st, o: b.motifs(g, stream=st), lambda b: b.motif_counts()),
            "af_profile": Pass(lambda b, st, o: b.af_profile(1024, 64, 10, stream=st), lambda b: b.af_profile_counts()),
            "strata": Pass(lambda b, st, o: b.strata(s, truth=True, stream=st), lambda b: b.strata_counts(), reads_hits=True),
            "boot": Pass(lambda b, st, o: b.boot(512, 128, 50, seed=11 if o else 7, truth=True, stream=st), lambda b: b.boot_counts(),
                         reads_hits=True, has_other=True),
            "votes": Pass(lambda b, st, o: b.votes(OTHER_GROUPS if o else GROUPS, stream=st), votes, lambda b: b.vote_timings(),
                          reads_hits=True, has_other=True),
            "nearmiss": Pass(lambda b, st, o: b.nearmiss(3, stream=st), nearmiss, lambda b: b.nearmiss_timings(), reads_hits=True),
            "surface": Pass(lambda b, st, o: b.surface(8 if o else 4, 32, 10, stream=st, fetch=False), lambda b: b.surface_counts(),
                            lambda b: b.surface_timings(), has_other=True),
            "context": Pass(lambda b, st, o: b.context(g, 50, 10, truth=True, stream=st, fetch=False), lambda b: b.context_counts(),
                            lambda b: b.context_timings(), reads_hits=True),
        }
        self.reference()

    def make(self):
        b = self.engine.batch(SIZES, [self.tids[w] for w in WHICH])
        for v, c in enumerate(self.cols):
            b.upload(v, *c)
        for v, a in self.af.items():
            b.upload_af(v, a)
        b.run()
        b.finish()
        return b

    def alter(self, b):
        b.upload(ALTERED, *self.other_cols)

    def anchor(self, b, variant, r):
        cols = list(self.cols)
        if variant == 2:
            cols[ALTERED] = self.other_cols
        for v, c in enumerate(cols):
            np.testing.assert_array_equal(r["truth_hits"][0][v], hits_by_truthside(c, self.truths[WHICH[v]]), err_msg="hit bitmap of VCF %d" % v)

    def close(self):
        for t in self.tids:
            self.engine.truth_release(t)
        self.engine.genome_release(self.gid)
        self.engine.strata_release(self.sid)


# ---- the allele-extended worlds: the batches of test_gpu_atomize and test_gpu_normalize ---------------------------------------
class Atoms(World):
    """test_gpu_atomize.make_batch (VCFs of 0, 1, 255, 256, 257 and 70 000 records, shuffled); alter(): the large VCF backwards"""
    SEED, ALTERED = 77, 5

    def __init__(self, engine):
        self.engine = engine
        b, self.cols, self.truths, self.tids = TA.make_batch(engine, self.SEED, False)
        b.close()
        fetch = lambda b: (b.atomize_counts(), [b.atomized(v) for v in range(b.n_vcf)])
        self.passes = {"atomize": Pass(lambda b, st, o: b.atomize(columns=True, stream=st, fetch=False), fetch, lambda b: b.atomize_timings())}
        # (the reference's first qm_batch_atomize is "the first call that meets a truth set": it "counts its atoms once, and
        #  waits for that number" (include/qmvt.h), so no call of a case does)
        self.reference()

    def make(self):
        b = self.engine.batch(TA.SIZES, [self.tids[w] for w in TA.WHICH], alleles=True)
        for v, c in enumerate(self.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        return b

    def alter(self, b):
        b.upload(self.ALTERED, *[x[::-1].copy() for x in self.cols[self.ALTERED]])

    def anchor(self, b, variant, r):
        rec, tru = r["atomize"][0]
        for v, (c, w) in enumerate(zip(self.cols, TA.WHICH)):
            if variant == 2 and v != self.ALTERED or v == self.ALTERED and variant == 1:
                continue                                  # (every VCF once: the large one as altered, its rows in the order it then has)
            c = [x[::-1] for x in c] if v == self.ALTERED else c
            cls = r["base"]["cls"][v]
            wrec, wtru = at.counts(self.truths[w], c[0], c[1], c[2], c[4], (cls & 1).astype(bool), (cls & 2).astype(bool))[:2]
            np.testing.assert_array_equal(rec[v], wrec, err_msg="atomize rec of VCF %d" % v)
            np.testing.assert_array_equal(tru[v], wtru, err_msg="atomize tru of VCF %d" % v)

    def close(self):
        for t in self.tids:
            self.engine.truth_release(t)


class Forms(World):
    """test_gpu_normalize.make_batch (sorted); alter(): the VCF of 3 000 records backwards"""
    SEED, ALTERED = 78, 0

    def __init__(self, engine):
        self.engine = engine
        b, self.cols, self.truths, self.genomes, self.tids, self.gids, self.want_gids = TN.make_batch(engine, self.SEED, True)
        b.close()
        fetch = lambda b: (b.normalize_counts(), [b.normalized(v) if self.want_gids[v] >= 0 else None for v in range(b.n_vcf)])
        self.passes = {"normalize": Pass(lambda b, st, o: b.normalize(self.want_gids, columns=True, stream=st, fetch=False), fetch,
                                         lambda b: b.normalize_timings())}
        self.reference()

    def make(self):
        b = self.engine.batch(TN.SIZES, [self.tids[w] for w in TN.WHICH], alleles=True)
        for v, c in enumerate(self.cols):
            b.upload(v, *c)
        b.run()
        b.finish()
        return b

    def alter(self, b):
        b.upload(self.ALTERED, *[x[::-1].copy() for x in self.cols[self.ALTERED]])

    def anchor(self, b, variant, r):
        rec, tru = r["normalize"][0]
        for v, (c, w) in enumerate(zip(self.cols, TN.WHICH)):
            if v == TN.NO_GENOME or variant == 2 and v != self.ALTERED or v == self.ALTERED and variant == 1:
                continue
            c = [x[::-1] for x in c] if v == self.ALTERED else c
            cls = r["base"]["cls"][v]
            wrec, wtru = nz.counts(self.genomes[w], self.truths[w], c[0], c[1], c[2], c[4], (cls & 1).astype(bool), (cls & 2).astype(bool))[:2]
            np.testing.assert_array_equal(rec[v], wrec, err_msg="normalize rec of VCF %d" % v)
            np.testing.assert_array_equal(tru[v], wtru, err_msg="normalize tru of VCF %d" % v)

    def close(self):
        for t in self.tids:
            self.engine.truth_release(t)
        for g in self.gids:
            self.engine.genome_release(g)


@pytest.fixture(scope="module")
def worlds(engine, gpu):
    w = {}
    try:
        w["single"] = SingleBase(engine)
        w["atoms"] = Atoms(engine)
        w["forms"] = Forms(engine)
        yield w
    finally:
        for x in w.values():
            x.close()


@pytest.fixture
def batch_of(worlds, gpu):
    """batch_of(kind): (the world, a fresh finished batch of it); the batch is closed behind the test once both streams are dry"""
    made = []

    def make(kind):
        b = worlds[kind].make()
        made.append(b)
        return worlds[kind], b
    yield make
    gpu.drain()
    for b in made:
        b.close()


EVERY_PASS = [("single", n) for n in ("truth_hits", "motifs", "af_profile", "strata", "boot", "votes", "nearmiss", "surface", "context")] + \
             [("forms", "normalize"), ("atoms", "atomize")]
HIT_READERS = ["strata", "boot", "context", "votes", "nearmiss"]
ids = lambda cases: ["%s" % c[1] for c in cases]


# ---- case 1: every pass on a stream of the caller's, its getter straight behind it --------------------------------------------
@pytest.mark.parametrize("kind,name", EVERY_PASS, ids=ids(EVERY_PASS))
def test_pass_on_a_callers_stream_and_its_getter(gpu, batch_of, kind, name):
    w, b = batch_of(kind)
    p = w.passes[name]
    b.set_timing(True)
    if p.reads_hits:
        b.truth_hits()                                   # (on the context's stream; the reader on A waits for its event)
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    if name != "nearmiss":                               # (Batch.nearmiss is the enqueue and the getter in one)
        gpu.flying(ev, name)
    got = p.fetch(b)                                     # blocking: waits for the pass's event, recorded on A
    gpu.landed(ev, name + "'s getter")
    same(got, w.ref[1][name], name)
    if p.timings:
        ms = p.timings(b)
        assert ms and all(x >= 0 for x in ms.values()), ms
    same(base_results(b), w.ref[1]["base"], "the batch behind " + name)   # the pass changed nothing of the batch


def test_nearmiss_enqueued_alone_is_in_flight(gpu, batch_of):
    """Batch.nearmiss fetches at once; the entry point by itself returns with the pass still behind the stall"""
    w, b = batch_of("single")
    b.truth_hits()
    gpu.stall(gpu.A)
    b._ck(b._L.qm_batch_nearmiss(b._h, 3, C.c_void_p(gpu.A)))
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "qm_batch_nearmiss")
    same(w.passes["nearmiss"].fetch(b), w.ref[1]["nearmiss"], "nearmiss")
    gpu.landed(ev, "nearmiss's getter")


# ---- case 2: the hit bitmaps made on A, read on B --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", HIT_READERS)
def test_reader_on_b_waits_for_truth_hits_on_a(gpu, batch_of, name):
    """(the bitmaps of the first columns are in place when the pass over the second ones is stalled: a reader that did not wait
    would read those, not zeros or what an earlier batch left at that address)"""
    w, b = batch_of("single")
    p = w.passes[name]
    b.truth_hits()
    w.alter(b)
    b.run()
    b.finish()
    gpu.stall(gpu.A)
    b.truth_hits(stream=gpu.A)
    ev = gpu.mark(gpu.A)
    if name == "nearmiss":
        b._ck(b._L.qm_batch_nearmiss(b._h, 3, C.c_void_p(gpu.B)))
    else:
        p.enqueue(b, gpu.B, False)
    gpu.flying(ev, "truth_hits in front of " + name)    # the reader was enqueued while the bitmaps were not made yet
    got = p.fetch(b)
    gpu.landed(ev, "truth_hits behind %s's getter" % name)   # ... and its getter, which waits for B alone, came back behind A
    same(got, w.ref[2][name], name)


def test_blocking_readers_wait_for_truth_hits_on_a(gpu, batch_of):
    """truth_regions, truth_hit_bits and intruth_mask wait on the host for the pass, on whatever stream it is"""
    w, b = batch_of("single")
    b.truth_hits()                                       # (the first bitmaps in place, as above)
    w.alter(b)
    b.run()
    b.finish()
    for k, read in enumerate((lambda: b.truth_regions(GROUPS, union=True), lambda: [b.truth_hit_bits(v) for v in range(b.n_vcf)],
                              lambda: [b.intruth_mask(v) for v in range(b.n_vcf)])):
        gpu.stall(gpu.A)
        b.truth_hits(stream=gpu.A)
        ev = gpu.mark(gpu.A)
        gpu.flying(ev, "truth_hits")
        got = read()
        gpu.landed(ev, "truth_hits behind its blocking reader")
        same(got, w.ref[2]["truth_hits"][(2, 0, 1)[k]], "blocking reader %d" % k)


# ---- case 3: the producer rewrites under its readers ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", HIT_READERS)
def test_truth_hits_rewrites_behind_its_readers(gpu, batch_of, name):
    """The reader enqueued on B behind a stall reads the first bitmaps although other columns are uploaded, run and finished
    and qm_batch_truth_hits(A) rewrites the bitmaps meanwhile; a reader enqueued after that reads the second.  Then, without a new
    run: qm_batch_truth_hits(A) behind a reader stalled on B waits for it on A."""
    w, b = batch_of("single")
    p = w.passes[name]
    raw = lambda st: b._ck(b._L.qm_batch_nearmiss(b._h, 3, C.c_void_p(st))) if name == "nearmiss" else p.enqueue(b, st, False)
    b.truth_hits()
    gpu.stall(gpu.B)
    raw(gpu.B)
    ev = gpu.mark(gpu.B)
    gpu.flying(ev, name)
    # No overlap can be held behind this: include/qmvt.h, "the blocking ones (qm_batch_upload, qm_batch_synth, qm_batch_upload_af)
    # return when those passes are done", and qm_batch_finish: "Wait for the stream".  What is asserted is that wait.
    w.alter(b)
    gpu.landed(ev, "%s behind qm_batch_upload" % name)
    first = p.fetch(b)                                   # (the flags of the run before still stand: fetched before the new run)
    same(first, w.ref[1][name], "%s enqueued before the new run" % name)
    b.run()
    b.finish()
    b.truth_hits(stream=gpu.A)
    raw(gpu.B)
    same(p.fetch(b), w.ref[2][name], "%s enqueued after the new run" % name)
    same(w.passes["truth_hits"].fetch(b), w.ref[2]["truth_hits"], "the second bitmaps")
    # without a new run: the reader stalled on B, the producer on A straight behind it
    gpu.stall(gpu.B)
    raw(gpu.B)
    ev = gpu.mark(gpu.B)
    b.truth_hits(stream=gpu.A)
    ev_a = gpu.mark(gpu.A)
    gpu.flying(ev, "%s in front of the second truth_hits" % name)
    assert gpu.hip.hipEventSynchronize(ev_a) == 0        # the producer is done ...
    gpu.landed(ev, "%s, which truth_hits on A waits for" % name)   # ... so the reader it had to wait for is, too
    same(p.fetch(b), w.ref[2][name], "%s under the rewrite" % name)
    same(w.passes["truth_hits"].fetch(b), w.ref[2]["truth_hits"], "the bitmaps rewritten")


# ---- case 4: the same pass twice, on two streams ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["surface", "boot", "votes"])
def test_same_pass_twice_on_two_streams(gpu, batch_of, name):
    """the second call (other parameters, on B) waits on the host for the first (on A behind a stall) before its memsets touch
    the outputs both write: the getter returns the second call's answer, also when both streams have run dry"""
    w, b = batch_of("single")
    p = w.passes[name]
    b.truth_hits()
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "the first " + name)
    p.enqueue(b, gpu.B, True)                            # blocking by pass_stream(): "waits for the previous ... of the batch"
    gpu.landed(ev, "the first %s behind the second call" % name)
    same(p.fetch(b), w.ref[1][name + "/other"], "the second " + name)
    gpu.drain()
    same(p.fetch(b), w.ref[1][name + "/other"], "the second %s, both streams dry" % name)


# ---- case 5: a new run behind a pass in flight -----------------------------------------------------------------------------------
FETCH_FALSE = [("single", "surface"), ("single", "context"), ("single", "motifs"), ("forms", "normalize"), ("atoms", "atomize")]


@pytest.mark.parametrize("kind,name", FETCH_FALSE, ids=ids(FETCH_FALSE))
def test_run_waits_for_a_pass_in_flight(gpu, batch_of, kind, name):
    """qm_batch_run on the context's stream behind a pass stalled on A: the run returns at once and is ordered behind the pass
    on the device, so the pass is done when qm_batch_finish comes back; its results are behind the latest run"""
    w, b = batch_of(kind)
    p = w.passes[name]
    if p.reads_hits:
        b.truth_hits()
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    b.run()
    gpu.flying(ev, name + " behind qm_batch_run")       # asynchronous: the wait is the stream's
    refused(lambda: p.fetch(b))
    b.finish()
    gpu.landed(ev, name + " behind qm_batch_finish")    # the run (and so the stream finish waits for) came behind the pass
    refused(lambda: p.fetch(b))
    same(base_results(b), w.ref[1]["base"], "the batch run again behind " + name)
    if p.reads_hits:
        b.truth_hits()
    p.enqueue(b, None, False)
    same(p.fetch(b), w.ref[1][name], "a fresh " + name)


@pytest.mark.parametrize("kind,name", FETCH_FALSE, ids=ids(FETCH_FALSE))
def test_upload_and_run_behind_a_pass_in_flight(gpu, batch_of, kind, name):
    """other columns for one VCF behind a pass stalled on A, then run and finish: everything equals the reference for the new
    columns, and no result of the pass can be fetched"""
    w, b = batch_of(kind)
    p = w.passes[name]
    if p.reads_hits:
        b.truth_hits()
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, name)
    # No overlap can be held behind this: include/qmvt.h, "the blocking ones (qm_batch_upload, qm_batch_synth, qm_batch_upload_af)
    # return when those passes are done".  What is asserted is that wait.
    w.alter(b)
    gpu.landed(ev, "%s behind qm_batch_upload" % name)
    b.run()
    refused(lambda: p.fetch(b))
    b.finish()
    refused(lambda: p.fetch(b))
    same(base_results(b), w.ref[2]["base"], "the new columns behind " + name)
    for n2, p2 in w.passes.items():                      # every pass of the world afresh (truth_hits first)
        p2.enqueue(b, None, False)
        same(p2.fetch(b), w.ref[2][n2], "a fresh %s over the new columns" % n2)


def test_upload_af_and_upload_async_wait_for_a_pass_in_flight(gpu, batch_of):
    """the two other writers of columns: qm_batch_upload_af on the host, qm_batch_upload_async on its stream"""
    w, b = batch_of("single")
    p = w.passes["surface"]
    gpu.stall(gpu.A)
    p.enqueue(b, gpu.A, False)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "surface")
    b.upload_af(WITH_AF[0], w.af[WITH_AF[0]])            # blocking (the same frequencies again)
    gpu.landed(ev, "surface behind qm_batch_upload_af")
    same(p.fetch(b), w.ref[1]["surface"], "surface")
    hip, cols, ptrs = gpu.hip, w.cols[2], []
    for x in cols:                                       # page-locked copies of VCF 2's own columns
        q = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(q), max(x.nbytes, 1), 0) == 0 and q.value
        C.memmove(q, x.ctypes.data, x.nbytes)
        ptrs.append(q)
    try:
        gpu.stall(gpu.A)
        p.enqueue(b, gpu.A, False)
        ev = gpu.mark(gpu.A)
        b._ck(b._L.qm_batch_upload_async(b._h, 2, *ptrs, C.c_void_p(gpu.B)))
        ev_b = gpu.mark(gpu.B)
        gpu.flying(ev, "surface behind qm_batch_upload_async")
        assert hip.hipEventSynchronize(ev_b) == 0        # the copies are done ...
        gpu.landed(ev, "surface, which the copies on B wait for")   # ... so the pass they had to wait for is, too
    finally:
        gpu.drain()
        for q in ptrs:
            assert hip.hipHostFree(q) == 0
    b.run()
    b.finish()
    same(base_results(b), w.ref[1]["base"], "the same columns uploaded again")


# ---- case 6: run and finish on a stream of the caller's, the passes on another -------------------------------------------------
@pytest.mark.parametrize("kind", ["single", "forms", "atoms"])
def test_run_and_finish_on_a_passes_on_b(gpu, batch_of, kind):
    w, b = batch_of(kind)
    b.set_timing(True)
    gpu.stall(gpu.A)
    b.run(stream=gpu.A)
    ev = gpu.mark(gpu.A)
    gpu.flying(ev, "qm_batch_run on A")
    b.finish(stream=gpu.A)                               # "Wait for the stream"
    gpu.landed(ev, "the run behind qm_batch_finish")
    assert all(x >= 0 for x in b.timings().values())
    gpu.stall(gpu.B)
    for name, p in w.passes.items():
        if name == "nearmiss":
            continue
        p.enqueue(b, gpu.B, False)
    ev = gpu.mark(gpu.B)
    gpu.flying(ev, "the passes on B")
    for name, p in w.passes.items():
        if name == "nearmiss":
            p.enqueue(b, gpu.B, False)
        same(p.fetch(b), w.ref[1][name], name + " on B")
    same(base_results(b), w.ref[1]["base"], "the batch run on A")
