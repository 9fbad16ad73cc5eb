"""Time the atomisation pass (qm_batch_atomize; k_atom_truth, k_atom_records, k_atom_found) on an allele-extended
batch of BASELINE configs[4]'s shape -- synthetic VCFs of 2 * 10^6 records, 30 % of them with longer alleles, position-sorted and
shuffled: the workload of tools/norm_bench.py.  One run + finish, then N x (pass + device synchronise): the kernels' milliseconds
between HIP events (qm_batch_atomize_timings) and the host clock around the call, without and with the per-record columns.  The
yardstick is k_norm_records on the same records in the same process (qm_batch_normalize against a random genome, as norm_bench
runs it).  Prints one JSON line per order.

    python tools/atom_bench.py [--vcfs 500] [--records 2000000] [--calls 10] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--vcfs", type=int, default=500)
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--truth", type=int, default=200_000)
    ap.add_argument("--indel-pct", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    from quasimodo_amd import _lib
    from quasimodo_amd.atomize import R_COLS, T_COLS
    rng = np.random.default_rng(2025)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    n = a.vcfs * a.records
    rows = []
    med = lambda ev, k: float(np.median([e[k] for e in ev]))
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 5, indel_pct=a.indel_pct)
        gid = eng.genome_load(genome)
        gids = [gid] * a.vcfs
        n_atoms = int(eng.truth_atoms(tid).shape[0])
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs, alleles=True)
            b.synth(a.genome, a.truth, 5, 5000, shuffled=shuffled, indel_pct=a.indel_pct)
            b.set_timing(True)
            b.run()
            b.finish()
            torch.cuda.synchronize()
            sc = b.scalars()
            c_ms, c_min, ev = timed(a.calls, a.warmup, lambda: b.atomize(fetch=False), torch.cuda.synchronize, b.atomize_timings)
            rec, tru = b.atomize_counts()
            assert (rec[:, 0] == sc[:, 0].astype(np.uint64)).all() and (rec[:, 1] == sc[:, 1].astype(np.uint64)).all() and (rec[:, 2] >= rec[:, 1]).all()
            assert (tru[:, 4] == sc[:, 3].astype(np.uint64)).all() and (tru[:, 4] <= tru[:, 5]).all() and int(tru[0][2]) == n_atoms
            w_ms, _, wev = timed(a.calls, a.warmup, lambda: b.atomize(columns=True, fetch=False), torch.cuda.synchronize, b.atomize_timings)
            _, _, nev = timed(a.calls, a.warmup, lambda: b.normalize(gids, fetch=False), torch.cuda.synchronize, b.normalize_timings)
            # bytes the record kernel must move per record: pos, ref, alt 4 each, flags 1, two mask bits; with the columns it
            # writes a class byte, an atom count and a 16-bit hit mask more
            c_bytes = n * (12 + 1) + 2 * n // 8
            k_rec, k_rec_cols, k_norm = med(ev, "atom_records_ms"), med(wev, "atom_records_ms"), med(nev, "norm_records_ms")
            rows.append({"kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(),
                         "order": "shuffled" if shuffled else "sorted", "vcfs": a.vcfs, "records": n,
                         "truth_entries": int(tru[0][0]), "truth_atoms": n_atoms, "indel_pct": a.indel_pct, "calls": a.calls,
                         "rec_sums": dict(zip(R_COLS, (int(x) for x in rec.sum(axis=0)))), "tru_vcf0": dict(zip(T_COLS, (int(x) for x in tru[0]))),
                         "k_atom_truth_ms_median": round(med(ev, "atom_truth_ms"), 3),
                         "k_atom_records_ms_median": round(k_rec, 3),
                         "k_atom_found_ms_median": round(med(ev, "atom_found_ms"), 3),
                         "k_atom_records_with_columns_ms_median": round(k_rec_cols, 3),
                         "atomize_call_ms_median": round(c_ms, 3), "atomize_call_ms_min": round(c_min, 3),
                         "atomize_with_columns_call_ms_median": round(w_ms, 3),
                         "k_norm_records_ms_median_same_records": round(k_norm, 3),
                         "bytes_per_record": round(c_bytes / n, 2), "records_TBps": round(c_bytes / (k_rec * 1e-3) / 1e12, 3),
                         "records_with_columns_TBps": round((c_bytes + 4 * n) / (k_rec_cols * 1e-3) / 1e12, 3)})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
