"""Time the ladder (qm_batch_ladder; k_ladder_records, k_ladder_truth) on the shape of tools/rroc_bench.py --
synthetic VCFs of 2 * 10^6 records, 30 % of them with longer alleles, position-sorted and shuffled, against a random genome.  One
run + finish, the four producers with their columns, then N x (ladder + device synchronise) with and without the mask column: the
kernels' milliseconds between HIP events (qm_batch_ladder_timings) and the host clock around the call.  k_rroc_records<N>, the
project's streaming kernel of the same frame, is timed in the same process for the side by side.  Prints one JSON line per order.

    python tools/ladder_bench.py [--vcfs 500] [--records 2000000] [--calls 10] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes k_ladder_records must move per record: the flag byte, the class bytes of the three passes and of the search, two mask
# bits in; with the columns one mask byte out.  (The 18 cells stay in registers and LDS.)
BYTES_IN, BYTES_OUT = 1 + 4 + 0.25, 1
BYTES_RROC_N = 4 * 4 + 1          # tools/rroc_bench.py: QUAL, REF, ALT and the truth row 4 each, the flag byte


def timed(calls, warmup, enqueue, wait, after):
    for _ in range(warmup):
        enqueue()
        wait()
    ts, extra = [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        enqueue()
        wait()
        ts.append(time.perf_counter() - t0)
        extra.append(after())
    return float(np.median(ts)) * 1e3, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=500)
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--truth", type=int, default=200_000)
    ap.add_argument("--indel-pct", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    from quasimodo_amd import _lib
    from quasimodo_amd import ladder as ld
    rng = np.random.default_rng(2025)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    n = a.vcfs * a.records
    med = lambda ev, k: float(np.median([e[k] for e in ev]))
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 5, indel_pct=a.indel_pct)
        gid = eng.genome_load(genome)
        gids = [gid] * a.vcfs
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs, alleles=True)
            b.synth(a.genome, a.truth, 5, 5000, shuffled=shuffled, indel_pct=a.indel_pct)
            b.set_timing(True)
            b.run()
            b.finish()
            torch.cuda.synchronize()
            nrec, ntru = b.normalize(gids, columns=True)
            arec, atru = b.atomize(columns=True)
            hrec, htru = b.haplotypes(gids, columns=True)
            sub = b.hapsubsets(columns=True)
            producers = b.device_bytes
            _, rev = timed(a.calls, a.warmup, lambda: b.rescue_roc(which=_lib.QM_RROC_NORM, fetch=False), torch.cuda.synchronize, b.rescue_roc_timings)
            swept = b.device_bytes
            c_ms, ev = timed(a.calls, a.warmup, lambda: b.ladder(subsets=True, fetch=False), torch.cuda.synchronize, b.ladder_timings)
            plain = b.device_bytes
            cc_ms, cev = timed(a.calls, a.warmup, lambda: b.ladder(subsets=True, columns=True, fetch=False), torch.cuda.synchronize, b.ladder_timings)
            rec, tru = b.ladder_counts()
            for v in range(a.vcfs):                      # the identities against the producers' own rows
                ld.identities(rec[v], tru[v], norm=(nrec[v], ntru[v]), atom=(arec[v], atru[v]), hap=(hrec[v], htru[v]), sub=sub[v])
            k, kc = {name: med(ev, name) for name in ev[0]}, {name: med(cev, name) for name in cev[0]}
            k_rroc = med(rev, "rroc_norm_records_ms")
            tbps = lambda bytes_per, ms: round(bytes_per * n / (ms * 1e-3) / 1e12, 3)
            cum = ld.cumulative(rec.sum(axis=0), tru.sum(axis=0))
            rows.append({"kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(),
                         "order": "shuffled" if shuffled else "sorted", "vcfs": a.vcfs, "records": n, "genome": a.genome,
                         "truth_entries": int(tru[0][0]), "indel_pct": a.indel_pct, "calls": a.calls,
                         "tp_fp_fn_by_tier": {name: list(c) for name, c in zip(("spelling",) + ld.METHODS, cum)},
                         "k_ladder_records_ms_median": round(k["ladder_records_ms"], 3), "k_ladder_truth_ms_median": round(k["ladder_truth_ms"], 3),
                         "k_ladder_records_with_columns_ms_median": round(kc["ladder_records_ms"], 3),
                         "k_ladder_truth_with_columns_ms_median": round(kc["ladder_truth_ms"], 3),
                         "k_rroc_records_norm_ms_median": round(k_rroc, 3),
                         "ladder_call_ms_median": round(c_ms, 3), "ladder_call_with_columns_ms_median": round(cc_ms, 3),
                         "bytes_per_record": {"ladder": BYTES_IN, "ladder_with_columns": BYTES_IN + BYTES_OUT, "rroc_norm": BYTES_RROC_N},
                         "TBps": {"ladder": tbps(BYTES_IN, k["ladder_records_ms"]), "ladder_with_columns": tbps(BYTES_IN + BYTES_OUT, kc["ladder_records_ms"]),
                                  "rroc_norm": tbps(BYTES_RROC_N, k_rroc)},
                         "records_per_ns": {"ladder": round(n / (k["ladder_records_ms"] * 1e6), 1), "rroc_norm": round(n / (k_rroc * 1e6), 1)},
                         "ladder_device_bytes": int(plain - swept), "ladder_columns_device_bytes": int(b.device_bytes - plain),
                         "producer_device_bytes": int(producers)})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
