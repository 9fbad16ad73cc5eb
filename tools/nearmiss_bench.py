"""Time the near-miss pass (qm_batch_nearmiss: k_nearmiss_records, k_nearmiss_truth) on synthetic batches of 10^9
records -- 6 250 VCFs of 160 000 records and 1 000 VCFs of 1 000 000, position-sorted and shuffled, radius 0, 10 and 64 -- and, IN
THE SAME PROCESS on the same batch, k_truth_hits and k_motif as yardsticks.  The batch's timing is on, so every call records
HIP events on its stream around the two kernels (qm_batch_nearmiss_timings); the yardsticks are enqueued on a stream of this
process between two HIP events of its own.  Warm-up, then the median of --calls calls.  qm_bw_probe's rates of the same process
stand beside the bytes the pass must read.  Prints one JSON line per shape, order and radius.

    python tools/nearmiss_bench.py [--shapes 6250x160000,1000x1000000] [--calls 10] [--out profiles/x.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADII = (0, 10, 64)


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
    ap.add_argument("--shapes", default="6250x160000,1000x1000000")
    ap.add_argument("--genome", type=int, default=4_000_000)
    ap.add_argument("--truth", type=int, default=40_000)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 3)
        gid = eng.genome_load(np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1).integers(0, 4, a.genome)].tobytes())
        bw = {k: round(v, 1) for k, v in eng.bw_probe(1 << 30, 5).items()}
        stream = torch.cuda.Stream()
        raw = stream.cuda_stream
        for shape in a.shapes.split(","):
            vcfs, records = (int(x) for x in shape.split("x"))
            if a.genome % records or a.genome % a.truth or (a.genome // a.truth) % (a.genome // records):
                ap.error("records and --truth must divide --genome, and genome / records must divide genome / truth (%s)" % shape)
            n = vcfs * records
            for shuffled in (False, True):
                b = eng.batch([records] * vcfs, [tid] * vcfs)
                b.synth(a.genome, a.truth, 3, 3000, shuffled=shuffled)
                b.run()
                b.finish()
                sc = b.scalars()
                b.set_timing(True)
                th_ms = event_ms(torch, stream, a.calls, a.warmup, lambda: b.truth_hits(stream=raw))
                mo_ms = event_ms(torch, stream, a.calls, a.warmup, lambda: b.motifs([gid] * vcfs, stream=raw))
                # what the pass must read: pos 4 + allele byte 1 + flags 1 bytes per record and two mask bits; it writes one class byte
                read_bytes = 6 * n + 2 * n // 8
                for radius in RADII:
                    st = []
                    for i in range(a.warmup + a.calls):
                        rec, tru = b.nearmiss(radius, stream=raw)
                        if i >= a.warmup:
                            st.append(b.nearmiss_timings())
                    med = {k: float(np.median([x[k] for x in st])) for k in st[0]}
                    assert (rec.sum(axis=1).astype(np.int64) == sc[:, 2]).all() and (tru.sum(axis=1).astype(np.int64) == sc[:, 7] - sc[:, 3]).all()
                    row = {"shape": shape, "order": "shuffled" if shuffled else "sorted", "radius": radius, "records": n, "warmup": a.warmup, "calls": a.calls,
                           "fp_lines": int(sc[:, 2].sum()), "rec_classes": [int(x) for x in rec.sum(axis=0)], "tru_classes": [int(x) for x in tru.sum(axis=0)],
                           "nearmiss_records_ms": round(med["nearmiss_records_ms"], 4), "nearmiss_truth_ms": round(med["nearmiss_truth_ms"], 4),
                           "truth_hits_ms": round(th_ms, 4), "motif_ms": round(mo_ms, 4), "read_bytes": read_bytes, "written_bytes": n,
                           "nearmiss_records_read_TBps": round(read_bytes / (med["nearmiss_records_ms"] * 1e-3) / 1e12, 3),
                           "records_over_truth_hits": round(med["nearmiss_records_ms"] / th_ms, 2), "bw_probe_GBps": bw}
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                b.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
