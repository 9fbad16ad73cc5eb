"""The derived allele byte of a batch without QM_BATCH_ALLELES: the kernels that read the single-base columns read
one byte per record -- ref << 2 | alt for two single bases, 0x10 otherwise -- instead of the two int32 codes.  Codes whose low
bits look like a single base but are not one (257, -256 + 2, 0x40000001, ...) must not pass for one on any path, and every
writer of the codes (qm_batch_upload, qm_batch_upload_async, qm_batch_synth) must keep the byte in step with them."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_columns, random_truth
from test_gpu_parity import check_vcf

pytestmark = pytest.mark.gpu

EDGE = np.array([-2**31, -257, -256 + 2, -1, 0, 1, 2, 3, 4, 255, 256, 257, 259, 0x40000000 | 1, 2**31 - 1], np.int64)


def with_pass(ref, alt, qual, flags):
    """the PASS bit the host path sets for these codes"""
    snp = (ref >= 0) & (ref < 4) & (alt >= 0) & (alt < 4)
    return ((flags & np.uint8(0xfe)) | (snp & (np.floor(qual) >= 20)).astype(np.uint8)).astype(np.uint8)


def edge_columns(rng, n, L, truth, sorted_=True):
    """random_columns with a fifth of the codes replaced: edge codes, and single bases moved by a multiple of 256 (the same low
    byte, not a single base)."""
    pos, ref, alt, qual, flags = random_columns(rng, n, L, truth, sorted_=sorted_)

    def spoil(c):
        c = c.astype(np.int64)
        k = rng.random(n)
        c = np.where(k < 0.1, rng.choice(EDGE, n), c)
        shifted = (c & 3) + rng.choice(np.array([256, -256, 1 << 20, 0x40000000, -(1 << 30)], np.int64), n)
        c = np.where((k >= 0.1) & (k < 0.2), shifted, c)
        return c.astype(np.int32)

    ref, alt = spoil(ref), spoil(alt)
    return pos, ref, alt, qual, with_pass(ref, alt, qual, flags)


def results(b, v, n):
    from quasimodo_amd.engine import SCALAR_NAMES
    sc = dict(zip(SCALAR_NAMES, b.scalars()[v].tolist()))
    reg = b.idx(v)
    return {"cls": b.cls(v), "roc": b.roc()[v], "scalars": sc, "tp_idx": reg[:sc["tp_lines"]].copy(), "fp_idx": reg[n - sc["fp_lines"]:].copy()}


def check_batch(b, oracle, cols, truth, tid, sorted_flags):
    want = np.zeros((3, 256), np.uint64)
    for v, c in enumerate(cols):
        r = results(b, v, len(c[0]))
        check_vcf(oracle, r, c, truth, expect_sorted=sorted_flags[v])
        want += r["roc"]
    assert np.array_equal(b.global_counts()[tid], want)


def test_edge_codes_on_sorted_vcfs_and_the_radix_sort(engine, oracle):
    """Sorted VCFs read the byte in k_classify (main loop and the single-record paths: equal-position runs across tiles and
    repeated keys); small unsorted ones take the radix sort, whose first pass reads it."""
    rng = np.random.default_rng(7101)
    L = 30_000
    truth = random_truth(rng, 3_000, L)
    tid = engine.truth_load(*truth)
    sizes = [50_000, 3_000, 257, 5_000]
    order = [True, True, False, False]
    cols = [edge_columns(rng, n, L, truth, sorted_=s) for n, s in zip(sizes, order)]
    b = engine.batch(sizes, [tid] * len(sizes))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run(); b.finish()
    check_batch(b, oracle, cols, truth, tid, order)
    assert b.path_stats()["radix"] == 2
    b.close()
    engine.truth_release(tid)


@pytest.mark.parametrize("path", ["", "radix", "two_level", "partitions", "wide"])
def test_edge_codes_on_a_shuffled_vcf_under_every_forced_path(engine, oracle, monkeypatch, path):
    """A shuffled VCF large enough for every bucket path, and a sorted one beside it, under each QM_UNSORTED_PATH ("": the
    path table's own choice): the scatters read the byte."""
    monkeypatch.setenv("QM_UNSORTED_PATH", path)
    rng = np.random.default_rng(7202)
    L = 4_000_000 if path == "two_level" else 400_000   # (the two levels size a partition's buckets for 128 ... 256 of them in use)
    truth = random_truth(rng, 30_000, L)
    tid = engine.truth_load(*truth)
    sizes = [120_000, 20_000]
    order = [False, True]
    cols = [edge_columns(rng, n, L, truth, sorted_=s) for n, s in zip(sizes, order)]
    b = engine.batch(sizes, [tid] * len(sizes))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    b.run(); b.finish()
    check_batch(b, oracle, cols, truth, tid, order)
    ps = b.path_stats()
    assert ps["unsorted"] == 1, ps
    if path == "radix":
        assert ps["radix"] == 1, ps
    if path == "two_level":
        assert ps["bucket_two_level"] == 1, ps
    b.close()
    engine.truth_release(tid)


def test_reupload_with_only_the_alleles_changed(engine, oracle):
    """The same positions, QUALs and ID flags, other allele codes: the runs after the re-upload must see the new codes (the byte
    is derived again; the batch's memory of out-of-order VCFs is dropped with the upload), a sorted and a shuffled VCF alike."""
    rng = np.random.default_rng(7303)
    L = 200_000
    truth = random_truth(rng, 10_000, L)
    tid = engine.truth_load(*truth)
    sizes = [40_000, 40_000]
    order = [True, False]
    cols = [edge_columns(rng, n, L, truth, sorted_=s) for n, s in zip(sizes, order)]
    b = engine.batch(sizes, [tid] * len(sizes))
    for v, c in enumerate(cols):
        b.upload(v, *c)
    for _ in range(2):
        b.run(); b.finish()
        check_batch(b, oracle, cols, truth, tid, order)
    for v, (pos, ref, alt, qual, flags) in enumerate(cols):
        # every single base becomes another one or an edge code, every other code a single base
        nref = np.where((ref >= 0) & (ref < 4), (ref + 1) & 3, ref & 3).astype(np.int32)
        nalt = np.where((alt >= 0) & (alt < 4), np.where(rng.random(len(alt)) < 0.5, (alt + 2) & 3, rng.choice(EDGE, len(alt))), alt & 3).astype(np.int32)
        cols[v] = (pos, nref, nalt, qual, with_pass(nref, nalt, qual, flags))
        b.upload(v, *cols[v])
    for _ in range(2):
        b.run(); b.finish()
        check_batch(b, oracle, cols, truth, tid, order)
    b.close()
    engine.truth_release(tid)


def _hip_runtime():
    """the HIP runtime the library is linked against (by its soname: the copy already loaded for it), for a stream of the test's own"""
    import re
    from quasimodo_amd import _lib
    _lib.lib()
    with open(_lib.library_path(), "rb") as f:
        soname = re.search(rb"libamdhip64\.so[.0-9]*", f.read()).group(0).decode()
    hip = C.CDLL(soname)
    for fn in ("hipStreamCreate", "hipStreamSynchronize", "hipStreamDestroy", "hipHostMalloc", "hipHostFree"):
        getattr(hip, fn).restype = C.c_int
    hip.hipHostMalloc.argtypes = [C.c_void_p, C.c_size_t, C.c_uint]
    hip.hipHostFree.argtypes = [C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    return hip


def test_async_upload_on_a_stream_of_its_own(engine, oracle):
    """qm_batch_upload_async from page-locked memory on a non-default stream derives the byte on that stream behind the copies:
    after a wait for that stream the run sees the new codes, for a first upload and for an upload of other records."""
    from quasimodo_amd import _lib
    hip = _hip_runtime()
    rng = np.random.default_rng(7404)
    L = 200_000
    truth = random_truth(rng, 10_000, L)
    tid = engine.truth_load(*truth)
    sizes = [60_000, 30_000, 2_000]
    order = [True, False, True]
    b = engine.batch(sizes, [tid] * len(sizes))
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0 and st.value
    lib = _lib.lib()
    for rep in range(2):
        cols = [edge_columns(rng, n, L, truth, sorted_=s) for n, s in zip(sizes, order)]
        bufs = []
        for v, c in enumerate(cols):
            ptrs = []
            for x in c:   # page-locked copies of the columns
                p = C.c_void_p()
                assert hip.hipHostMalloc(C.byref(p), max(x.nbytes, 1), 0) == 0 and p.value
                C.memmove(p, x.ctypes.data, x.nbytes)
                ptrs.append(p)
            bufs += ptrs
            assert lib.qm_batch_upload_async(b._h, v, *ptrs, st) == 0
        assert hip.hipStreamSynchronize(st) == 0
        for p in bufs:
            assert hip.hipHostFree(p) == 0
        b.run(); b.finish()
        check_batch(b, oracle, cols, truth, tid, order)
    assert hip.hipStreamDestroy(st) == 0
    b.close()
    engine.truth_release(tid)


@pytest.mark.parametrize("shuffled", [False, True])
def test_synthetic_batch_writes_the_byte(engine, oracle, shuffled):
    """qm_batch_synth writes the byte beside the codes: a synthetic batch against the oracle on the codes read back, then an
    upload of edge codes over one of its VCFs."""
    from oracle.synth import synth_truth_keys
    rng = np.random.default_rng(7505)
    L, T, N = 400_000, 8_000, 80_000
    tid = engine.truth_synth(L, T, 5)
    tk = synth_truth_keys(L, T, 5)
    b = engine.batch([N, N], [tid, tid])
    b.synth(L, T, 5, 77, shuffled=shuffled)
    b.run(); b.finish()
    cols = [b.columns(v) for v in range(2)]
    check_batch(b, oracle, cols, tk, tid, [not shuffled] * 2)
    cols[1] = edge_columns(rng, N, L, tk, sorted_=True)
    b.upload(1, *cols[1])
    b.run(); b.finish()
    check_batch(b, oracle, cols, tk, tid, [not shuffled, True])
    b.close()
    engine.truth_release(tid)
