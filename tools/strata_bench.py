"""Time the stratification pass (qm_batch_strata, k_strata_records) on a batch of BASELINE configs[2]'s shape --
1 000 synthetic VCFs of 10^6 records, position-sorted and shuffled -- under three strata sets: (a) one stratum over everything
(every lane on one counter), (b) 8 disjoint strata of 200 intervals each (the LDS table), (c) 32 overlapping strata with more
than 4096 segments (the global table); and, IN THE SAME PROCESS on the same batch, the allele-frequency profile pass
(k_af_profile) and the mutation-context pass (k_motif) as yardsticks.  One run + finish, then N x (pass + device synchronise)
each.  Prints one JSON line per order and strata set.

    python tools/strata_bench.py [--vcfs 1000] [--records 1000000] [--calls 20] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

I32MAX = (1 << 31) - 1


def timed(calls, warmup, enqueue, wait):
    for _ in range(warmup):
        enqueue()
        wait()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        enqueue()
        wait()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, min(ts) * 1e3


def strata_sets(genome, rng):
    whole = [("all", [0], [I32MAX])]
    # 8 x 200 disjoint intervals: the genome cut into 1 600 pieces, every second half of a piece left outside
    piece = genome // 1600
    eight = [("s%d" % k, [(200 * k + i) * piece for i in range(200)], [(200 * k + i) * piece + piece // 2 for i in range(200)]) for k in range(8)]
    # 32 overlapping strata of 160 random intervals each: about 10 000 segments
    wide = []
    for k in range(32):
        s = rng.integers(0, genome - 1, 160)
        wide.append(("w%d" % k, s, np.minimum(s + rng.integers(1, genome // 2000, 160), genome)))   # short: few merge
    return [("one_stratum", whole), ("eight_disjoint_lds", eight), ("thirty_two_overlapping_global", wide)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=1000)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    rng = np.random.default_rng(2025)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    af = rng.random(a.records).astype(np.float32)
    n = a.vcfs * a.records
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, 50_000, 3)
        gid = eng.genome_load(genome)
        sets = [(name, s, eng.strata_load(s)) for name, s in strata_sets(a.genome, rng)]
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
            b.synth(a.genome, 50_000, 3, 3000, shuffled=shuffled)
            for v in range(a.vcfs):
                b.upload_af(v, af)
            b.run()
            b.finish()
            sc = b.scalars()
            kept = int(sc[:, 0].sum())
            p_ms, _ = timed(a.calls, a.warmup, lambda: b.af_profile(-(-a.genome // 256), 256, 20), torch.cuda.synchronize)
            m_ms, _ = timed(a.calls, a.warmup, lambda: b.motifs([gid] * a.vcfs), torch.cuda.synchronize)
            # bytes the passes must read per record: the two mask bits; under a kept bit pos 4 and flags 1 (strata) / pos 4, af 4,
            # allele byte 1 (profile); the 16-byte pos loads of a group with any kept bit bring the whole group
            s_bytes = 2 * n // 8 + 4 * n + kept
            p_bytes = n * (4 + 4 + 1) + 2 * n // 8
            b.truth_hits()
            torch.cuda.synchronize()
            assert eng.strata_info(sets[1][2])[1] <= 4096 < eng.strata_info(sets[2][2])[1]   # the LDS table, the global table
            for name, s, sid in sets:
                r_ms, r_min = timed(a.calls, a.warmup, lambda: b.strata(sid), torch.cuda.synchronize)
                t_ms, _ = timed(a.calls, a.warmup, lambda: b.strata(sid, truth=True), torch.cuda.synchronize)
                rec, tru = b.strata_counts()
                assert int(rec[:, -1, 0].sum()) + int(rec[:, -2, 0].sum()) <= kept and (rec[:, :, 0] == rec[:, :, 1] + rec[:, :, 2]).all()
                if name == "one_stratum":
                    assert (rec[:, :, 0].sum(axis=1) == sc[:, 0]).all() and (tru[:, :, 0].sum(axis=1) == sc[:, 7]).all()
                rows.append({"order": "shuffled" if shuffled else "sorted", "strata_set": name, "n_strata": len(s),
                             "segments": eng.strata_info(sid)[1], "records": n, "kept": kept, "calls": a.calls,
                             "records_ms_per_call_median": round(r_ms, 3), "records_ms_min": round(r_min, 3),
                             "records_and_truth_ms_per_call_median": round(t_ms, 3),
                             "strata_bytes_per_record": round(s_bytes / n, 2), "strata_TBps": round(s_bytes / (r_ms * 1e-3) / 1e12, 2),
                             "profile_ms_per_call_median": round(p_ms, 3), "profile_TBps": round(p_bytes / (p_ms * 1e-3) / 1e12, 2),
                             "motif_ms_per_call_median": round(m_ms, 3), "strata_over_profile": round(r_ms / p_ms, 3)})
                print(json.dumps(rows[-1]), flush=True)
            b.close()
        for _, _, sid in sets:
            eng.strata_release(sid)
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
