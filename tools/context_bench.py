"""Time the sequence-context pass (qm_batch_context; k_context_build / k_context_records / k_context_truth) on a
batch of BASELINE configs[2]'s shape -- 1 000 synthetic VCFs of 10^6 records, position-sorted and shuffled -- against a random
5 Mb genome, and, IN THE SAME PROCESS on the same batch, the stratification pass under one stratum (k_strata_records) and the
allele-frequency profile pass (k_af_profile) as yardsticks.  One run + finish, then N x (pass + device synchronise) each: the
kernels' milliseconds between HIP events (qm_batch_context_timings) and, for all three passes alike, the host clock around the
call.  The arm of k_context_records is a build (-DQM_CX_VARIANT=1: the wave-aggregated one): run the tool once per library
(QM_LIBQMVT names the other build) and name the arm with --arm.  Prints one JSON line per order.

    python tools/context_bench.py [--arm lds_atomics] [--vcfs 1000] [--records 1000000] [--calls 20] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

I32MAX = (1 << 31) - 1


def timed(calls, warmup, enqueue, wait, after=None):
    for _ in range(warmup):
        enqueue()
        wait()
    ts, extra = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        enqueue()
        wait()
        ts.append(time.perf_counter() - t0)
        if after:
            extra.append(after())
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", default="lds_atomics")
    ap.add_argument("--vcfs", type=int, default=1000)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--half-window", type=int, default=50)
    ap.add_argument("--gc-bins", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    from quasimodo_amd import _lib
    rng = np.random.default_rng(2025)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    af = rng.random(a.records).astype(np.float32)
    n = a.vcfs * a.records
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, 50_000, 3)
        gid = eng.genome_load(genome)
        sid = eng.strata_load([("all", [0], [I32MAX])])
        gids = [gid] * a.vcfs
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
            b.synth(a.genome, 50_000, 3, 3000, shuffled=shuffled)
            for v in range(a.vcfs):
                b.upload_af(v, af)
            b.set_timing(True)
            b.run()
            b.finish()
            b.truth_hits()
            torch.cuda.synchronize()
            sc = b.scalars()
            kept = int(sc[:, 0].sum())
            # the first call builds the table (other parameters first, so that every process pays a build)
            b.context(gids, 1, 1, fetch=False)
            b.context(gids, a.half_window, a.gc_bins, fetch=False)
            torch.cuda.synchronize()
            build_ms = b.context_timings()["context_build_ms"]
            p_ms, _, _ = timed(a.calls, a.warmup, lambda: b.af_profile(-(-a.genome // 256), 256, 20), torch.cuda.synchronize)
            s_ms, _, _ = timed(a.calls, a.warmup, lambda: b.strata(sid), torch.cuda.synchronize)
            r_ms, r_min, _ = timed(a.calls, a.warmup, lambda: b.context(gids, a.half_window, a.gc_bins, fetch=False), torch.cuda.synchronize)
            t_ms, _, ev = timed(a.calls, a.warmup, lambda: b.context(gids, a.half_window, a.gc_bins, truth=True, fetch=False),
                                torch.cuda.synchronize, b.context_timings)
            rec, tru, gen = b.context_counts()
            assert (rec[:, :, 0].sum(axis=1) == sc[:, 0]).all() and (tru[:, :, 0].sum(axis=1) == sc[:, 7]).all() and int(gen[0].sum()) == a.genome
            # bytes the record kernels must read per record: the two mask bits; under a kept bit pos 4 and flags 1, and the context pass
            # one table byte more (the 16-byte pos loads of a group with any kept bit bring the whole group)
            c_bytes = 2 * n // 8 + 4 * n + 2 * kept
            k_rec = float(np.median([e["context_records_ms"] for e in ev]))
            rows.append({"arm": a.arm, "kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(),
                         "order": "shuffled" if shuffled else "sorted", "records": n, "kept": kept, "genome": a.genome,
                         "half_window": a.half_window, "gc_bins": a.gc_bins, "calls": a.calls,
                         "cells_in_use": int((gen[0] > 0).sum()), "hottest_cell_share": round(float(rec[:, :, 0].sum(axis=0).max()) / max(kept, 1), 3),
                         "k_context_build_ms": round(build_ms, 3), "k_context_records_ms_median": round(k_rec, 3),
                         "k_context_truth_ms_median": round(float(np.median([e["context_truth_ms"] for e in ev])), 3),
                         "context_records_call_ms_median": round(r_ms, 3), "context_records_call_ms_min": round(r_min, 3),
                         "context_records_and_truth_call_ms_median": round(t_ms, 3),
                         "strata_one_stratum_call_ms_median": round(s_ms, 3), "af_profile_call_ms_median": round(p_ms, 3),
                         "context_bytes_per_record": round(c_bytes / n, 2), "context_TBps": round(c_bytes / (k_rec * 1e-3) / 1e12, 2),
                         "context_over_strata": round(r_ms / s_ms, 3), "context_over_profile": round(r_ms / p_ms, 3)})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.strata_release(sid)
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
