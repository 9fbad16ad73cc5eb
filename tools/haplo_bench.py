"""Time the haplotype pass (qm_batch_haplotypes; qmvt_haplo.hip) on an allele-extended batch of BASELINE
configs[4]'s shape -- synthetic VCFs of 2 * 10^6 records, 30 % of them with longer alleles, position-sorted and shuffled: the
workload of tools/vartype_bench.py, with the random genome of tools/norm_bench.py.  One run + finish, then N x (pass + device
synchronise): the milliseconds of the pass's five parts between HIP events (qm_batch_haplotype_timings) and the host clock around
the call.  The yardstick is k_norm_records on the same records in the same process: it streams the same three columns, flags and
masks and checks REF against the same genome.  Synthetic alleles are drawn without the genome: most records leave at the REF
check, as they do in 4.17, so few lines reach a site and fewer a replay -- the numbers of tried sites say how few.  Prints one
JSON line per order.

--subsets adds the subset search behind the pass (qm_batch_hapsubsets; k_hap_subsets) on the same batch: the
milliseconds of the search between HIP events beside k_hap_replay's on the same pairs -- both are one wave per pair over the same
lists --, the whole call beside the whole haplotype call, both hash modes, and the counts: how many of the workload's MISMATCH and
CONFLICT sites hold a partial match.  --worst N times the search alone on N pairs of one degenerate site, 8 forms against 8 inside
one run of 12 A: once where the optimum is 8 + 7 and seven T masks replay alike, once where no subset matches; in the narrow-hash
mode nearly every candidate of equal length is verified symbol by symbol.

    python tools/haplo_bench.py [--vcfs 100] [--records 2000000] [--calls 10] [--gap 10] [--order both] [--subsets] [--worst 100000]
                                [--out profiles/x.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from atom_bench import timed   # noqa: E402  (the script beside this one)

PARTS = ("hap_sites_ms", "hap_records_ms", "hap_truth_ms", "hap_claim_ms", "hap_replay_ms")


def worst_case(eng, pairs, calls, warmup, sync):
    """`pairs` (VCF, site) pairs of one degenerate site: 100 VCFs of pairs / 100 sites, one block of 100 bases per site"""
    from quasimodo_amd.haplo import SUB_COLS, code
    n_vcf = 100
    n_sites = max(pairs // n_vcf, 1)
    block = "G" * 40 + "C" + "A" * 12 + "G" * 47
    genome = (block * n_sites).encode()
    rows = []
    for name, entries in (("partial_8_7", [(0, "C", "CA"), (1, "AA", "AAA"), (2, "AA", "AAA"), (4, "A", "AAA")] + [(k, "A", "AA") for k in range(9, 13)]),
                          ("nosubset", [(k, "A", "AC") for k in range(1, 9)])):
        lines = [(k, "A", "AA") for k in range(1, 9)]
        cols = lambda side: [np.array([41 + 100 * s + k for s in range(n_sites) for k, _, _ in side], np.int32),
                             np.array([code(r) for s in range(n_sites) for _, r, _ in side], np.int32),
                             np.array([code(x) for s in range(n_sites) for _, _, x in side], np.int32)]
        tid, gid = eng.truth_load(*cols(entries)), eng.genome_load(genome)
        pos, ref, alt = cols(lines)
        b = eng.batch([len(pos)] * n_vcf, [tid] * n_vcf, alleles=True)
        for v in range(n_vcf):
            b.upload(v, pos, ref, alt, np.full(len(pos), 50, np.float32), np.full(len(pos), 3, np.uint8))   # PASS, ID '.'
        b.set_timing(True)
        b.run()
        b.finish()
        b.haplotypes([gid] * n_vcf)
        row = {"worst_case": name, "pairs": n_vcf * n_sites, "hap_replay_ms": round(b.haplotype_timings()["hap_replay_ms"], 3)}
        for mode, narrow in (("normal", False), ("narrow_hash", True)):
            c_ms, _, ev = timed(calls, warmup, lambda: b.hapsubsets(narrow_hash=narrow, fetch=False), sync, b.hapsubset_timings)
            row["hap_subsets_ms_median_" + mode] = round(float(np.median([e["hap_subsets_ms"] for e in ev])), 3)
            row["hapsubsets_call_ms_median_" + mode] = round(c_ms, 3)
            row["sub_sums_" + mode] = dict(zip(SUB_COLS, (int(x) for x in b.hapsubset_counts().sum(axis=0))))
        assert row["sub_sums_normal"] == row["sub_sums_narrow_hash"] and row["sub_sums_normal"]["searched"] == n_vcf * n_sites
        rows.append(row)
        print(json.dumps(row), flush=True)
        b.close()
        eng.truth_release(tid)
        eng.genome_release(gid)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vcfs", type=int, default=100)
    ap.add_argument("--records", type=int, default=2_000_000)
    ap.add_argument("--genome", type=int, default=10_000_000)
    ap.add_argument("--truth", type=int, default=200_000)
    ap.add_argument("--indel-pct", type=int, default=30)
    ap.add_argument("--gap", type=int, default=10)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--order", choices=["both", "sorted", "shuffled"], default="both", help="one order only: for a counter run of its own")
    ap.add_argument("--subsets", action="store_true", help="the subset search behind the pass (DESIGN.md 4.21)")
    ap.add_argument("--worst", type=int, default=0, help="with --subsets: pairs of the degenerate 8 x 8 site, timed on their own")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    from quasimodo_amd import _lib
    from quasimodo_amd.haplo import R_COLS, T_COLS
    rng = np.random.default_rng(2025)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    n = a.vcfs * a.records
    rows = []
    med = lambda ev, k: float(np.median([e[k] for e in ev]))
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, a.truth, 5, indel_pct=a.indel_pct)
        gid = eng.genome_load(genome)
        gids = [gid] * a.vcfs
        for shuffled in [o == "shuffled" for o in ("sorted", "shuffled") if a.order in ("both", o)]:
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs, alleles=True)
            b.synth(a.genome, a.truth, 5, 5000, shuffled=shuffled, indel_pct=a.indel_pct)
            b.set_timing(True)
            b.run()
            b.finish()
            torch.cuda.synchronize()
            sc = b.scalars()
            c_ms, c_min, ev = timed(a.calls, a.warmup, lambda: b.haplotypes(gids, a.gap, fetch=False), torch.cuda.synchronize, b.haplotype_timings)
            rec, tru = b.haplotype_counts()
            assert (rec[:, 0] == sc[:, 0].astype(np.uint64)).all() and (rec[:, 1] == sc[:, 1].astype(np.uint64)).all()
            assert (rec[:, 2] - rec[:, 1] == rec[:, 3]).all() and (tru[:, 2] >= tru[:, 1]).all()
            _, _, nev = timed(a.calls, a.warmup, lambda: b.normalize(gids, fetch=False), torch.cuda.synchronize, b.normalize_timings)
            # bytes k_hap_records must move per record: pos, ref, alt 4 each, flags 1, two mask bits, the class byte and the site it writes
            c_bytes = n * (12 + 1 + 1 + 4) + 2 * n // 8
            parts = {k: round(med(ev, k), 3) for k in PARTS}
            k_rec, k_norm = parts["hap_records_ms"], med(nev, "norm_records_ms")
            rows.append({"kernels_id": _lib.kernel_source_id(), "build_id": eng._L.qm_build_id().decode(),
                         "order": "shuffled" if shuffled else "sorted", "vcfs": a.vcfs, "records": n, "genome": a.genome, "gap": a.gap,
                         "indel_pct": a.indel_pct, "calls": a.calls,
                         "rec_sums": dict(zip(R_COLS, (int(x) for x in rec.sum(axis=0)))), "tru_vcf0": dict(zip(T_COLS, (int(x) for x in tru[0]))),
                         "tried_sites": int(tru[:, 6].sum()), "matched_sites": int(tru[:, 7].sum()),
                         "parts_ms_median": parts, "pass_ms_median_sum_of_parts": round(sum(parts.values()), 3),
                         "haplotypes_call_ms_median": round(c_ms, 3), "haplotypes_call_ms_min": round(c_min, 3),
                         "k_norm_records_ms_median_same_records": round(k_norm, 3),
                         "k_hap_records_over_k_norm_records": round(k_rec / k_norm, 3),
                         "pass_over_k_norm_records": round(sum(parts.values()) / k_norm, 3),
                         "bytes_per_record": round(c_bytes / n, 2), "records_TBps": round(c_bytes / (k_rec * 1e-3) / 1e12, 3)})
            if a.subsets:
                from quasimodo_amd.haplo import SUB_COLS
                b.haplotypes(gids, a.gap, fetch=False)
                for mode, narrow in (("normal", False), ("narrow_hash", True)):
                    s_ms, _, sev = timed(a.calls, a.warmup, lambda: b.hapsubsets(narrow_hash=narrow, fetch=False), torch.cuda.synchronize, b.hapsubset_timings)
                    sub = b.hapsubset_counts()
                    k_sub = float(np.median([e["hap_subsets_ms"] for e in sev]))
                    rows[-1]["subsets_" + mode] = {"hap_subsets_ms_median": round(k_sub, 3), "hapsubsets_call_ms_median": round(s_ms, 3),
                                                   "k_hap_subsets_over_k_hap_replay": round(k_sub / max(parts["hap_replay_ms"], 1e-6), 3),
                                                   "call_over_haplotypes_call": round(s_ms / c_ms, 3),
                                                   "sub_sums": dict(zip(SUB_COLS, (int(x) for x in sub.sum(axis=0))))}
                assert rows[-1]["subsets_normal"]["sub_sums"] == rows[-1]["subsets_narrow_hash"]["sub_sums"]
                ss = rows[-1]["subsets_normal"]["sub_sums"]
                assert ss["searched"] == ss["partial"] + ss["nosubset"] and ss["tp_s"] >= rows[-1]["rec_sums"]["tp_h"]
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.genome_release(gid)
        if a.subsets and a.worst:
            rows += worst_case(eng, a.worst, a.calls, a.warmup, torch.cuda.synchronize)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
