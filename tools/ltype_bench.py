"""Time the match ladder per variant type and size (qm_batch_ladder_types; k_ltype_records, k_ltype_truth) on the
shape of tools/ladder_bench.py -- synthetic VCFs of 2 * 10^6 records, 30 % of them with longer alleles, position-sorted and
shuffled, against a random genome.  One run + finish, the four rescues with their columns, then N x (call + device synchronise)
of the type pass with its row bytes, of the ladder with its mask bytes and of the cross: the kernels' milliseconds between HIP
events (qm_batch_*_timings) and the host clock around the call.  k_ladder_records and k_type_records, the two producers whose
columns the new kernel reads, are its yardsticks and are timed in the same process.  Prints one JSON line per order.

    python tools/ltype_bench.py [--vcfs 500] [--records 2000000] [--calls 10] [--out profiles/x.json]

A build of the other variant of k_ltype_records (make LTFLAGS=-DQM_LTYPE_MERGE=0: one LDS atomic per kept record; loaded through
QM_LIBQMVT) is timed by the same command; --variant names it in the output."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bytes the record kernels must move per record.  k_ltype_records: the row byte and the mask byte in (the cells stay in LDS).
# k_ladder_records with the mask column: the flag byte, four class bytes and two mask bits in, the mask byte out.  k_type_records
# with the row bytes: POS, REF and ALT 4 each, the flag byte and two mask bits in, the row byte out.
BYTES_LTYPE, BYTES_LADDER, BYTES_TYPES = 2, 1 + 4 + 0.25 + 1, 12 + 1 + 0.25 + 1


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
    ap.add_argument("--variant", default="merged", help="what the loaded library's k_ltype_records is: merged (the tree's build) or plain")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    from quasimodo_amd import _lib
    from quasimodo_amd import ladder as ld
    from quasimodo_amd import laddertypes as lt
    from quasimodo_amd import vartype as vt
    rng = np.random.default_rng(2025)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    n = a.vcfs * a.records
    med = lambda ev, k: float(np.median([e[k] for e in ev]))
    names = vt.row_names(vt.DEFAULT_EDGES)
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
            b.normalize(gids, columns=True, fetch=False)
            b.atomize(columns=True, fetch=False)
            b.haplotypes(gids, columns=True, fetch=False)
            b.hapsubsets(columns=True, fetch=False)
            _, tev = timed(a.calls, a.warmup, lambda: b.vartype(columns=True, fetch=False), torch.cuda.synchronize, b.vartype_timings)
            _, lev = timed(a.calls, a.warmup, lambda: b.ladder(subsets=True, columns=True, fetch=False), torch.cuda.synchronize, b.ladder_timings)
            producers = b.device_bytes
            c_ms, ev = timed(a.calls, a.warmup, lambda: b.ladder_types(fetch=False), torch.cuda.synchronize, b.ladder_type_timings)
            rec, tru = b.ladder_type_counts()
            lrec, ltru = b.ladder_counts()
            trec, ttru = b.vartype_counts()
            for v in range(a.vcfs):                      # the identities against the producers' own rows
                lt.identities(rec[v], tru[v], ladder=(lrec[v], ltru[v]), types=(trec[v], ttru[v]), edges=vt.DEFAULT_EDGES)
            k_lt, k_ltt = med(ev, "ltype_records_ms"), med(ev, "ltype_truth_ms")
            k_ld, k_ty = med(lev, "ladder_records_ms"), med(tev, "type_records_ms")
            tbps = lambda bytes_per, ms: round(bytes_per * n / (ms * 1e-3) / 1e12, 3)
            kept = int(rec[:, :, ld.KEPT].sum())
            hot = int(rec[:, names.index("SNV:1"), ld.TP].sum())
            rows.append({"kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(), "k_ltype_records_variant": a.variant,
                         "order": "shuffled" if shuffled else "sorted", "vcfs": a.vcfs, "records": n, "genome": a.genome,
                         "truth_entries": int(tru[0][:, ld.KEPT].sum()), "indel_pct": a.indel_pct, "calls": a.calls,
                         "kept_records": kept, "hot_cell_share_of_kept": round(hot / max(kept, 1), 4),
                         "k_ltype_records_ms_median": round(k_lt, 3), "k_ltype_truth_ms_median": round(k_ltt, 3),
                         "k_ladder_records_with_columns_ms_median": round(k_ld, 3), "k_type_records_with_columns_ms_median": round(k_ty, 3),
                         "ladder_types_call_ms_median": round(c_ms, 3),
                         "bytes_per_record": {"ltype": BYTES_LTYPE, "ladder_with_columns": BYTES_LADDER, "types_with_columns": BYTES_TYPES},
                         "TBps": {"ltype": tbps(BYTES_LTYPE, k_lt), "ladder_with_columns": tbps(BYTES_LADDER, k_ld), "types_with_columns": tbps(BYTES_TYPES, k_ty)},
                         "records_per_ns": {"ltype": round(n / (k_lt * 1e6), 1), "ladder_with_columns": round(n / (k_ld * 1e6), 1),
                                            "types_with_columns": round(n / (k_ty * 1e6), 1)},
                         "ladder_types_device_bytes": int(b.device_bytes - producers)})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
