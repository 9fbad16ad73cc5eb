"""Time the variant-type pass (qm_batch_types; k_type_records, k_type_truth) on an allele-extended batch of
BASELINE configs[4]'s shape -- synthetic VCFs of 2 * 10^6 records, 30 % of them with longer alleles, position-sorted and shuffled:
the workload of tools/atom_bench.py.  One run + finish, then N x (pass + device synchronise): the kernels' milliseconds between
HIP events (qm_batch_types_timings) and the host clock around the call, without and with the per-record row bytes.  The yardstick
is k_atom_records on the same records in the same process: it streams the same three columns, flags and masks.  Prints one JSON
line per order.

    python tools/vartype_bench.py [--vcfs 100] [--records 2000000] [--calls 10] [--order both] [--out profiles/x.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from atom_bench import timed   # noqa: E402  (the script beside this one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=100)
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--truth", type=int, default=200_000)
    ap.add_argument("--indel-pct", type=int, default=30)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--order", choices=["both", "sorted", "shuffled"], default="both", help="one order only: for a counter run of its own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    from quasimodo_amd import _lib
    from quasimodo_amd.vartype import DEFAULT_EDGES, row_names
    n = a.vcfs * a.records
    rows = []
    med = lambda ev, k: float(np.median([e[k] for e in ev]))
    names = row_names(DEFAULT_EDGES)
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 5, indel_pct=a.indel_pct)
        for shuffled in [o == "shuffled" for o in ("sorted", "shuffled") if a.order in ("both", o)]:
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs, alleles=True)
            b.synth(a.genome, a.truth, 5, 5000, shuffled=shuffled, indel_pct=a.indel_pct)
            b.set_timing(True)
            b.run()
            b.finish()
            torch.cuda.synchronize()
            sc = b.scalars()
            c_ms, c_min, ev = timed(a.calls, a.warmup, lambda: b.vartype(fetch=False), torch.cuda.synchronize, b.vartype_timings)
            rec, tru = b.vartype_counts()
            assert (rec[:, :, 0].sum(axis=1) == sc[:, 0].astype(np.uint64)).all() and (rec[:, :, 1].sum(axis=1) == sc[:, 1].astype(np.uint64)).all()
            w_ms, _, wev = timed(a.calls, a.warmup, lambda: b.vartype(columns=True, fetch=False), torch.cuda.synchronize, b.vartype_timings)
            _, _, aev = timed(a.calls, a.warmup, lambda: b.atomize(fetch=False), torch.cuda.synchronize, b.atomize_timings)
            _, atru = b.atomize_counts()
            assert (tru[:, :, 1].sum(axis=1) == atru[:, 4]).all()      # the found entries, by two kernels
            # bytes the record kernel must move per record: pos, ref, alt 4 each, flags 1, two mask bits; with the columns one row byte more
            c_bytes = n * (12 + 1) + 2 * n // 8
            k_rec, k_rec_cols, k_atom = med(ev, "type_records_ms"), med(wev, "type_records_ms"), med(aev, "atom_records_ms")
            kept = rec[:, :, 0].sum(axis=0)
            rows.append({"kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(),
                         "order": "shuffled" if shuffled else "sorted", "vcfs": a.vcfs, "records": n,
                         "truth_entries": int(tru[0][:, 0].sum()), "indel_pct": a.indel_pct, "calls": a.calls,
                         "kept_by_row": {names[k]: int(x) for k, x in enumerate(kept) if x},
                         "k_type_records_ms_median": round(k_rec, 3), "k_type_truth_ms_median": round(med(ev, "type_truth_ms"), 3),
                         "k_type_records_with_columns_ms_median": round(k_rec_cols, 3),
                         "vartype_call_ms_median": round(c_ms, 3), "vartype_call_ms_min": round(c_min, 3),
                         "vartype_with_columns_call_ms_median": round(w_ms, 3),
                         "k_atom_records_ms_median_same_records": round(k_atom, 3),
                         "bytes_per_record": round(c_bytes / n, 2), "records_TBps": round(c_bytes / (k_rec * 1e-3) / 1e12, 3),
                         "records_with_columns_TBps": round((c_bytes + n) / (k_rec_cols * 1e-3) / 1e12, 3),
                         "atom_records_TBps": round(c_bytes / (k_atom * 1e-3) / 1e12, 3)})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
