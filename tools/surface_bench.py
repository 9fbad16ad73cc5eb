"""Time the filter surface pass (qm_batch_surface: k_surface_records, k_surface_truth, k_surface_sums) on a
synthetic batch of 10^9 records -- 6 250 VCFs of 160 000 records, position-sorted and shuffled, at the default grid (4, 64, 50)
and at (1, 64, 64) -- and, IN THE SAME PROCESS on the same batch, k_truth_hits (one exact lookup per looked-up record) and
k_af_profile (the same streamed pos / af columns) as yardsticks.  The batch's timing is on, so every call records HIP events on
its stream around the three kernels (qm_batch_surface_timings); the yardsticks are enqueued on a stream of this process between
two HIP events of its own.  Every VCF gets the same column of uniform allele frequencies with one NaN in 16.  Warm-up, then the
median of --calls calls.  qm_bw_probe's rates of the same process stand beside the bytes the pass must read.  Prints one JSON
line per order and grid.

    python tools/surface_bench.py [--shapes 6250x160000] [--calls 10] [--out profiles/x.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRIDS = ((4, 64, 50), (1, 64, 64))


def event_ms(torch, stream, calls, warmup, enqueue):
    """median milliseconds of `enqueue` between two HIP events on `stream`"""
    ts = []
    for i in range(warmup + calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        enqueue()
        b.record(stream)
        b.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="6250x160000")
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--truth", type=int, default=40_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-check", action="store_true", help="do not compare the AF >= 0 column with the ROC (A/B builds that leave work out)")
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 3)
        bw = {k: round(v, 1) for k, v in eng.bw_probe(1 << 30, 5).items()}
        stream = torch.cuda.Stream()
        raw = stream.cuda_stream
        for shape in a.shapes.split(","):
            vcfs, records = (int(x) for x in shape.split("x"))
            if a.genome % records or a.genome % a.truth or (a.genome // a.truth) % (a.genome // records):
                ap.error("records and --truth must divide --genome, and genome / records must divide genome / truth (%s)" % shape)
            n = vcfs * records
            rng = np.random.default_rng(16)
            af = rng.random(records, dtype=np.float32)
            af[rng.random(records) < 1 / 16] = np.nan
            for shuffled in (False, True):
                b = eng.batch([records] * vcfs, [tid] * vcfs)
                b.synth(a.genome, a.truth, 3, 3000, shuffled=shuffled)
                for v in range(vcfs):
                    b.upload_af(v, af)
                b.run()
                b.finish()
                roc = b.roc()
                b.set_timing(True)
                th_ms = event_ms(torch, stream, a.calls, a.warmup, lambda: b.truth_hits(stream=raw))
                af_ms = event_ms(torch, stream, a.calls, a.warmup, lambda: b.af_profile(1024, 256, 20, stream=raw))
                # what the pass must read per record: pos 4 + allele byte 1 + flags 1 + qual 4 + af 4 bytes; it writes tables only
                read_bytes = 14 * n
                for q_step, nq, na in GRIDS:
                    st = []
                    for i in range(a.warmup + a.calls):
                        S, extra = b.surface(q_step, nq, na, stream=raw)
                        if i >= a.warmup:
                            st.append(b.surface_timings())
                    med = {k: float(np.median([x[k] for x in st])) for k in st[0]}
                    # the whole call between two events: the clears of the best codes and the tables in front of the kernels included
                    call_ms = event_ms(torch, stream, a.calls, a.warmup, lambda: b.surface(q_step, nq, na, stream=raw, fetch=False))
                    lines = [i for i in range(nq) if i * q_step < b.n_bins]
                    assert a.no_check or all((S[:, c, lines, 0] == roc[:, c, [i * q_step for i in lines]]).all() for c in range(3)), "the AF >= 0 column is the ROC"
                    row = {"shape": shape, "order": "shuffled" if shuffled else "sorted", "q_step": q_step, "nq": nq, "na": na, "records": n,
                           "warmup": a.warmup, "calls": a.calls, "counted": int(extra[:, 0].sum()), "no_af": int(extra[:, 1].sum()),
                           "tp": int(S[:, 0, 0, 0].sum()), "fp": int(S[:, 1, 0, 0].sum()), "found_keys": int(S[:, 2, 0, 0].sum()),
                           "best_bytes": int(4 * extra[:, 3].sum()),
                           "surface_records_ms": round(med["surface_records_ms"], 4), "surface_truth_ms": round(med["surface_truth_ms"], 4),
                           "surface_sums_ms": round(med["surface_sums_ms"], 4), "surface_call_ms": round(call_ms, 4), "truth_hits_ms": round(th_ms, 4), "af_profile_ms": round(af_ms, 4),
                           "read_bytes": read_bytes, "surface_records_read_TBps": round(read_bytes / (med["surface_records_ms"] * 1e-3) / 1e12, 3),
                           "records_over_truth_hits": round(med["surface_records_ms"] / th_ms, 2),
                           "records_over_af_profile": round(med["surface_records_ms"] / af_ms, 2), "bw_probe_GBps": bw}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                b.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
