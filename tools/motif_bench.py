"""Time the mutation-context pass (qm_batch_motifs, k_motif) on a batch of BASELINE configs[2]'s shape:
1 000 sorted synthetic VCFs of 10^6 records, a seeded random 5 Mb genome.  One run + finish, then N x (qm_batch_motifs +
synchronise).  Prints one JSON line.  Under rocprofv3 --kernel-trace --stats (tools/trace_kernels.sh) it gives k_motif's time.

    python tools/motif_bench.py [--vcfs 1000] [--records 1000000] [--calls 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=1000)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import quasimodo_amd as q
    rng = np.random.default_rng(2024)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, 50_000, 3)
        b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
        b.synth(a.genome, 50_000, 3, 3000)
        b.run()
        b.finish()
        gid = eng.genome_load(genome)
        gids = [gid] * a.vcfs
        for _ in range(a.warmup):
            b.motifs(gids)
            b.motif_counts()
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            b.motifs(gids)
            b.motif_counts()
            ts.append(time.perf_counter() - t0)
        m = b.motif_counts()
        sc = b.scalars()
        assert (m[:, 0, :97].sum(axis=1) == sc[:, 0]).all()
        n = a.vcfs * a.records
        # bytes the pass must read: pos 4, allele byte 1, flags 1, two mask bits; the genome and the output are noise beside it
        nbytes = n * (4 + 1 + 1) + 2 * n // 8
        ms = float(np.median(ts)) * 1e3
        print(json.dumps({"records": n, "calls": a.calls, "ms_per_call_median": round(ms, 3), "ms_min": round(min(ts) * 1e3, 3),
                          "bytes_read": nbytes, "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1),
                          "kept": int(sc[:, 0].sum()), "other": int(m[:, 0, 96].sum()), "ref_mismatch": int(m[:, 0, 97].sum())}))
        eng.genome_release(gid)
        b.close()


if __name__ == "__main__":
    main()
