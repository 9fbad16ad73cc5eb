"""Time the rescue-ROC sweep (qm_batch_rescue_roc; k_rroc_records<N>, k_rroc_records<A>, k_rroc_units) on the
shape of tools/norm_bench.py -- synthetic VCFs of 2 * 10^6 records, 30 % of them with longer alleles, position-sorted and
shuffled, against a random genome.  One run + finish, the two producers with their columns (their record kernels timed in the
same process, medians of N calls, for the side by side), then N x (sweep + device synchronise): the kernels' milliseconds between
HIP events (qm_batch_rescue_roc_timings) and the host clock around the call.  Prints one JSON line per order.

    python tools/rroc_bench.py [--vcfs 500] [--records 2000000] [--calls 10] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes a record kernel must move per record.  By normal form: QUAL, REF, ALT and the truth row 4 each, the flag byte.  By atoms:
# QUAL, POS, REF, ALT 4 each, the flag byte, the 16-bit hit mask.  (The histograms stay in LDS; the best cells and the tables
# they are found through are touched per HIT, not per record, and are left out.)
BYTES_N, BYTES_A = 4 * 4 + 1, 4 * 4 + 1 + 2
# the producers with their columns, as tools/norm_bench.py and the atom pass's section count them
BYTES_NORM_COLS, BYTES_ATOM_COLS = 12 + 1 + 1 + 0.25 + 16, 12 + 1 + 0.25 + 4


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
            before = b.device_bytes
            _, nev = timed(a.calls, a.warmup, lambda: b.normalize(gids, columns=True, fetch=False), torch.cuda.synchronize, b.normalize_timings)
            _, aev = timed(a.calls, a.warmup, lambda: b.atomize(columns=True, fetch=False), torch.cuda.synchronize, b.atomize_timings)
            producers = b.device_bytes
            c_ms, ev = timed(a.calls, a.warmup, lambda: b.rescue_roc(fetch=False), torch.cuda.synchronize, b.rescue_roc_timings)
            roc_n, roc_a, base = b.rescue_roc_counts()
            roc = b.roc()
            assert (roc_n[:, 0] + roc_n[:, 1] == roc[:, 0] + roc[:, 1]).all() and (roc_a[:, 0] + roc_a[:, 1] == roc[:, 0] + roc[:, 1]).all()
            assert (roc_n[:, 0] >= roc[:, 0]).all() and (roc_a[:, 0] >= roc[:, 0]).all()
            k = {name: med(ev, name) for name in ev[0]}
            k_norm, k_atom = med(nev, "norm_records_ms"), med(aev, "atom_records_ms")
            tbps = lambda bytes_per, ms: round(bytes_per * n / (ms * 1e-3) / 1e12, 3)
            rows.append({"kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(),
                         "order": "shuffled" if shuffled else "sorted", "vcfs": a.vcfs, "records": n, "genome": a.genome,
                         "truth_forms": int(base[0][0]), "truth_entries": int(base[0][1]), "indel_pct": a.indel_pct, "calls": a.calls,
                         "tp_t20": {"spelling": int(roc[:, 0, 20].sum()), "normalized": int(roc_n[:, 0, 20].sum()), "atomized": int(roc_a[:, 0, 20].sum())},
                         "found_t20": {"spelling": int(roc[:, 2, 20].sum()), "normalized": int(roc_n[:, 2, 20].sum()), "atomized": int(roc_a[:, 2, 20].sum())},
                         "k_rroc_records_norm_ms_median": round(k["rroc_norm_records_ms"], 3),
                         "k_rroc_units_norm_ms_median": round(k["rroc_norm_units_ms"], 3),
                         "k_rroc_records_atom_ms_median": round(k["rroc_atom_records_ms"], 3),
                         "k_rroc_units_atom_ms_median": round(k["rroc_atom_units_ms"], 3),
                         "k_norm_records_with_columns_ms_median": round(k_norm, 3), "k_atom_records_with_columns_ms_median": round(k_atom, 3),
                         "rescue_roc_call_ms_median": round(c_ms, 3),
                         "bytes_per_record": {"rroc_norm": BYTES_N, "rroc_atom": BYTES_A, "norm_with_columns": BYTES_NORM_COLS, "atom_with_columns": BYTES_ATOM_COLS},
                         "TBps": {"rroc_norm": tbps(BYTES_N, k["rroc_norm_records_ms"]), "rroc_atom": tbps(BYTES_A, k["rroc_atom_records_ms"]),
                                  "norm_with_columns": tbps(BYTES_NORM_COLS, k_norm), "atom_with_columns": tbps(BYTES_ATOM_COLS, k_atom)},
                         "sweep_device_bytes": int(b.device_bytes - producers), "producer_device_bytes": int(producers - before)})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
