"""Time the bootstrap pass (qm_batch_boot: k_boot_records, k_boot_truth, k_boot_resample) on the synthetic
10^9-record batch -- 6 250 VCFs of 160 000 records, position-sorted and shuffled -- at 256 windows x 1000 replicates and at
4096 windows x 2000 replicates; and, IN THE SAME PROCESS on the same batch, the stratification pass with one stratum
(k_strata_records) and the batch's own step (run + finish) as yardsticks.  One run + finish, then N x (pass + device
synchronise) each: the counting pass alone (n_rep = 0), with the truth side, and with the replicates; the resample's time is
the difference to the counting pass.  Prints one JSON line per order and shape.

    python tools/boot_bench.py [--vcfs 6250] [--records 160000] [--calls 10] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

I32MAX = (1 << 31) - 1
SHAPES = [(256, 1000), (4096, 2000)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=6250)
    ap.add_argument("--records", type=int, default=160_000)
    ap.add_argument("--genome", type=int, default=4_800_000)
    ap.add_argument("--truth", type=int, default=40_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    # what the synthetic generator asks of its sizes (qm_batch_synth)
    if a.genome % a.records or a.genome % a.truth or (a.genome // a.truth) % (a.genome // a.records):
        ap.error("--records and --truth must divide --genome, and genome / records must divide genome / truth")
    n = a.vcfs * a.records
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 3)
        sid = eng.strata_load([("all", [0], [I32MAX])])
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
            b.synth(a.genome, a.truth, 3, 3000, shuffled=shuffled)
            def step():
                b.run()
                b.finish()
            step_ms, _ = timed(a.calls, a.warmup, step, torch.cuda.synchronize)
            sc = b.scalars()
            kept = int(sc[:, 0].sum())
            b.truth_hits()
            torch.cuda.synchronize()
            s_ms, _ = timed(a.calls, a.warmup, lambda: b.strata(sid), torch.cuda.synchronize)
            # bytes the counting pass must read per record: the two mask bits; under a kept bit pos 4 and flags 1; the 16-byte
            # pos loads of a group with any kept bit bring the whole group
            c_bytes = 2 * n // 8 + 4 * n + kept
            for n_win, n_rep in SHAPES:
                window = -(-a.genome // n_win)
                c_ms, c_min = timed(a.calls, a.warmup, lambda: b.boot(window, n_win, 0), torch.cuda.synchronize)
                t_ms, _ = timed(a.calls, a.warmup, lambda: b.boot(window, n_win, 0, truth=True), torch.cuda.synchronize)
                r_ms, _ = timed(max(2, a.calls // 3), 1, lambda: b.boot(window, n_win, n_rep, seed=1), torch.cuda.synchronize)
                cnt, rep = b.boot_counts()
                assert (cnt[:, :, 0].sum(axis=1) == sc[:, 0]).all() and (cnt[:, :, 1].sum(axis=1) == sc[:, 1]).all()
                assert (rep[:, :, 0] >= cnt[:, n_win:, 0].sum(axis=1)[:, None]).all()
                macs = a.vcfs * n_rep * n_win * 4
                rows.append({"order": "shuffled" if shuffled else "sorted", "n_win": n_win, "n_rep": n_rep, "window": window, "vcfs": a.vcfs,
                             "records": n, "kept": kept, "calls": a.calls, "batch_step_ms_median": round(step_ms, 3),
                             "counts_ms_per_call_median": round(c_ms, 3), "counts_ms_min": round(c_min, 3),
                             "counts_and_truth_ms_per_call_median": round(t_ms, 3), "counts_and_resample_ms_per_call_median": round(r_ms, 3),
                             "resample_ms": round(r_ms - c_ms, 3), "resample_Gmac_per_s": round(macs / max(r_ms - c_ms, 1e-6) / 1e6, 1),
                             "cnt_MiB": round(a.vcfs * (n_win + 2) * 32 / 2 ** 20, 1), "rep_MiB": round(a.vcfs * n_rep * 32 / 2 ** 20, 1),
                             "counts_bytes_per_record": round(c_bytes / n, 2), "counts_TBps": round(c_bytes / (c_ms * 1e-3) / 1e12, 2),
                             "strata_one_stratum_ms_per_call_median": round(s_ms, 3), "counts_over_strata": round(c_ms / s_ms, 3),
                             "resample_over_batch_step": round((r_ms - c_ms) / step_ms, 2)})
                print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.strata_release(sid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
