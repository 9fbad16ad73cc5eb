"""Time the truth-side pass (qm_batch_truth_hits, k_truth_hits) on a batch of BASELINE configs[2]'s shape --
1 000 synthetic VCFs of 10^6 records, sorted -- and on the same batch shuffled.  One run + finish per batch, then per variant a
warm-up and N x (qm_batch_truth_hits + wait), wall clock around the synchronised call, the median reported.  The arms that
lost the A/B (LABNOTES round 9) are build variants: a library built with -DQM_TS_VARIANT=1|2|3 (qmvt_truthside.h), named through
QM_LIBQMVT, is timed by the same command.  k_truth_regions (200 groups of five) is timed once per batch; --motif adds
k_motif on the same batch, --probe qm_bw_probe's read rate.  Prints one JSON line per batch.

    python tools/truthside_bench.py [--vcfs 1000] [--records 1000000] [--calls 9] [--motif] [--probe]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(f, calls, warmup):
    for _ in range(warmup):
        f()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, min(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=1000)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--truth", type=int, default=50_000)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--motif", action="store_true")
    ap.add_argument("--probe", action="store_true")
    a = ap.parse_args()
    if a.calls < 5:
        ap.error("--calls: the median of at least 5 calls")
    import quasimodo_amd as q
    n = a.vcfs * a.records
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 3)
        probe = eng.bw_probe(4 << 30, 5) if a.probe else None
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
            b.synth(a.genome, a.truth, 3, 3000, shuffled=shuffled)
            b.run()
            b.finish()
            sc = b.scalars()
            kept = int(sc[:, 0].sum())
            row = {"batch": "shuffled" if shuffled else "sorted", "records": n, "kept": kept, "calls": a.calls}

            def call():
                b.truth_hits()
                b.truth_hit_bits(0)           # waits for the pass, copies one small bitmap

            ms, mn = timed(call, a.calls, a.warmup)
            # bytes the pass must read and write: pos 4 + allele byte 1 + kept bit + record-mask bit per record; flags 1 and the
            # TP bit under a kept bit (8 records at a time)
            floor = n * 5 + 2 * n // 8
            row["truth_hits"] = {"ms_median": round(ms, 3), "ms_min": round(mn, 3), "floor_GBps": round(floor / (ms * 1e-3) / 1e9, 1)}
            b.truth_hits()
            tp_r = sum(int(b.truth_hit_bits(v).sum()) for v in range(min(a.vcfs, 8)))
            assert tp_r == int(sc[:min(a.vcfs, 8), 3].sum()), "popcount(hits) != TP_R"
            groups = [list(range(g, g + 5)) for g in range(0, a.vcfs - a.vcfs % 5, 5)]
            if groups:
                t0 = time.perf_counter()
                reg = b.truth_regions(groups)
                row["regions_ms_once"] = round((time.perf_counter() - t0) * 1e3, 3)
                row["region_groups"] = len(groups)
                assert (reg.sum(axis=1) == sc[0, 7]).all()
            if a.motif:
                rng = np.random.default_rng(2024)
                gid = eng.genome_load(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes())

                def mcall():
                    b.motifs([gid] * a.vcfs)
                    b.motif_counts()

                ms, mn = timed(mcall, a.calls, a.warmup)
                row["k_motif"] = {"ms_median": round(ms, 3), "ms_min": round(mn, 3)}
                eng.genome_release(gid)
            if probe:
                row["bw_probe"] = {k: round(v, 1) for k, v in probe.items()}
            print(json.dumps(row), flush=True)
            b.close()


if __name__ == "__main__":
    main()
