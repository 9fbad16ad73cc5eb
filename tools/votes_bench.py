"""Time the consensus pass (qm_batch_votes: k_vote_truth, k_vote_keys, four radix passes, k_vote_heads / k_vote_scan /
k_vote_runs) on the synthetic 10^9-record batch -- 6 250 VCFs of 160 000 records, position-sorted and shuffled --
with the VCFs dealt to groups of 5, 6 and 32 consecutive members; and, IN THE SAME PROCESS on the same batch, the batch's own
step (run + finish) and the truth-side pass (qm_batch_truth_hits) as yardsticks.  One run + finish + truth_hits, then
N x (pass + device synchronise) per group size.  The batch's timing is on, so every call records HIP events on its stream
around k_vote_truth, k_vote_keys (+ k_vote_segs), the four radix passes and the run kernels (qm_batch_vote_timings): the
medians of those are the per-stage times, with no host copy between the events; the wall clock around the call and a device
synchronise (which holds the call's small blocking table copies) is reported beside them.  qm_bw_probe's read and copy rates of
the same process stand beside the bytes each stage must move.  With --yardstick the n = 5 numbers are also made the older way, qm_batch_truth_regions plus Engine.fp_overlap
over host-gathered keys, for the first --yardstick-groups groups (the host gather of 10^9 records is not what one wants to
wait for), and compared.  Prints one JSON line per order and group size.

    python tools/votes_bench.py [--vcfs 6250] [--records 160000] [--calls 10] [--yardstick] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = (5, 6, 32)


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
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--yardstick-groups", type=int, default=8)
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
        bw = {k: round(v, 1) for k, v in eng.bw_probe(1 << 30, 5).items()}
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
            b.synth(a.genome, a.truth, 3, 3000, shuffled=shuffled)
            def step():
                b.run()
                b.finish()
            step_ms, _ = timed(a.calls, a.warmup, step, torch.cuda.synchronize)
            sc = b.scalars()
            b.set_timing(True)
            th_ms, _ = timed(a.calls, a.warmup, b.truth_hits, torch.cuda.synchronize)
            for size in SIZES:
                groups = [list(range(g * size, (g + 1) * size)) for g in range(a.vcfs // size)]
                if not groups:
                    continue
                members = [v for g in groups for v in g]
                kept = int(sc[members, 0].sum())
                stages = []
                def one():
                    b.votes(groups)
                def wait():
                    torch.cuda.synchronize()
                    stages.append(b.vote_timings())
                v_ms, v_min = timed(a.calls, a.warmup, one, wait)
                stages = stages[a.warmup:]
                med = {k: float(np.median([x[k] for x in stages])) for k in stages[0]}
                cnt = b.vote_counts()
                cc = np.arange(33, dtype=np.int64)
                assert (cnt["tp_votes"].sum(axis=1) == a.truth).all()
                tp_r = np.array([sc[g, 3].sum() for g in groups])
                fp_r = np.array([sc[g, 4].sum() for g in groups])
                assert ((cnt["tp_votes"].astype(np.int64) * cc).sum(axis=1) == tp_r).all()
                assert ((cnt["fp_votes"].astype(np.int64) * cc).sum(axis=1) == fp_r).all()
                pairs = int(fp_r.sum())   # (the synthetic VCFs hold no key twice: the pairs are the members' FP_R keys)
                recs = len(members) * a.records
                # bytes that must move: k_vote_keys reads two mask bits per record, and pos 4 + allele 1 + flags 1 under a kept bit
                # (the 16-byte loads of a group with any kept bit bring the whole group), and writes 8 per pair; a radix pass
                # reads 8 per pair for its histogram and 8 for its scatter and writes 8; the run kernels read 4 + 8 and write
                # at most 8 per pair
                keys_bytes = 2 * recs // 8 + 6 * recs + 8 * pairs
                sort_bytes = 4 * 24 * pairs
                runs_bytes = 20 * pairs
                row = {"order": "shuffled" if shuffled else "sorted", "group_size": size, "groups": len(groups), "vcfs": a.vcfs,
                       "records": n, "member_records": recs, "kept": kept, "pairs": pairs, "distinct_keys": int(cnt["fp_votes"].sum()),
                       "calls": a.calls, "batch_step_ms_median": round(step_ms, 3), "truth_hits_ms_median": round(th_ms, 3),
                       "votes_ms_per_call_median": round(v_ms, 3), "votes_ms_min": round(v_min, 3),
                       "bytes_vote_keys": keys_bytes, "bytes_sort": sort_bytes, "bytes_runs": runs_bytes,
                       "votes_TBps_of_those_bytes": round((keys_bytes + sort_bytes + runs_bytes) / (v_ms * 1e-3) / 1e12, 3),
                       "votes_over_batch_step": round(v_ms / step_ms, 2),
                       "stage_ms_median": {k: round(v, 4) for k, v in med.items()}, "stages_sum_ms": round(sum(med.values()), 3),
                       "vote_keys_TBps": round(keys_bytes / (med["vote_keys_ms"] * 1e-3) / 1e12, 3),
                       "sort_TBps": round(sort_bytes / (med["sort_ms"] * 1e-3) / 1e12, 3),
                       "vote_runs_TBps": round(runs_bytes / (med["vote_runs_ms"] * 1e-3) / 1e12, 3),
                       "bw_probe_GBps": bw}
                if a.yardstick and size == 5:
                    yg = groups[:a.yardstick_groups]
                    t0 = time.perf_counter()
                    reg = b.truth_regions(yg)
                    fpr = []
                    for g in yg:
                        sets = []
                        for v in g:
                            pos, ref, alt, _, _ = b.columns(v)
                            sel = ((b.cls(v) & 1) != 0) & ~b.intruth_mask(v)
                            sets.append((pos[sel], ref[sel], alt[sel]))
                        fpr.append(eng.fp_overlap(sets))
                    y_ms = (time.perf_counter() - t0) * 1e3
                    pc = np.array([bin(m).count("1") for m in range(32)])
                    for i in range(len(yg)):
                        for c in range(6):
                            assert int(cnt["tp_votes"][i][c]) == int(reg[i][pc == c].sum())
                            assert int(cnt["fp_votes"][i][c]) == int(np.asarray(fpr[i])[(pc == c) & (np.arange(32) > 0)].sum())
                    row.update({"yardstick_groups": len(yg), "yardstick_ms_per_group": round(y_ms / len(yg), 3),
                                "votes_ms_per_group": round(v_ms / len(groups), 5)})
                rows.append(row)
                print(json.dumps(row), flush=True)
            b.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
