"""Time the allele-frequency profile pass (qm_batch_af_profile, k_af_profile) on a batch of BASELINE configs[2]'s
shape -- 1 000 synthetic VCFs of 10^6 records, position-sorted and shuffled -- with allele frequencies drawn uniformly, and,
IN THE SAME PROCESS, the mutation-context pass (k_motif) on the same batch as the yardstick.  A sorted VCF touches a few position
columns of the grid per workgroup, a shuffled one all of them: the second run shows what the full-grid flush costs.  One run +
finish, then N x (pass + device synchronise) each; the copy-back of the grids is timed once, apart.  Prints one JSON line per order.

    python tools/afprofile_bench.py [--vcfs 1000] [--records 1000000] [--calls 20] [--out profiles/x.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    ap.add_argument("--vcfs", type=int, default=1000)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pos-bins", type=int, default=256)
    ap.add_argument("--af-bins", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import quasimodo_amd as q
    rng = np.random.default_rng(2024)
    genome = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, a.genome)].tobytes()
    af = rng.random(a.records).astype(np.float32)          # one column, uploaded to every VCF (the positions differ per VCF)
    window = -(-a.genome // a.pos_bins)                      # the whole genome inside the grid
    n = a.vcfs * a.records
    rows = []
    with q.Engine(0) as eng:
        tid = eng.truth_synth(a.genome, 50_000, 3)
        gid = eng.genome_load(genome)
        gids = [gid] * a.vcfs
        for shuffled in (False, True):
            b = eng.batch([a.records] * a.vcfs, [tid] * a.vcfs)
            b.synth(a.genome, 50_000, 3, 3000, shuffled=shuffled)
            for v in range(a.vcfs):
                b.upload_af(v, af)
            b.run()
            b.finish()
            # the wait is a device synchronise, not the getter: the profile's getter copies n_vcf * 2 * cells * 8 bytes back
            # (82 MB at the defaults), which is not the pass
            p_ms, p_min = timed(a.calls, a.warmup, lambda: b.af_profile(window, a.pos_bins, a.af_bins), torch.cuda.synchronize)
            t0 = time.perf_counter()
            b.af_profile_counts()
            get_ms = (time.perf_counter() - t0) * 1e3
            m_ms, m_min = timed(a.calls, a.warmup, lambda: b.motifs(gids), torch.cuda.synchronize)
            grid, extra = b.af_profile_counts()
            sc = b.scalars()
            assert (extra.sum(axis=(1, 2)) == sc[:, 0]).all() and (grid.sum(axis=(2, 3)) == extra[:, :, 2]).all()
            # bytes the passes must read per record: the two mask bits; under a kept bit pos 4, af 4, allele byte 1 (profile) /
            # pos 4, allele byte 1, flags 1 (motifs); the genome and the outputs are noise beside it
            p_bytes = n * (4 + 4 + 1) + 2 * n // 8
            m_bytes = n * (4 + 1 + 1) + 2 * n // 8
            rows.append({"order": "shuffled" if shuffled else "sorted", "records": n, "calls": a.calls, "window": window,
                         "n_pos_bins": a.pos_bins, "n_af_bins": a.af_bins,
                         "profile_ms_per_call_median": round(p_ms, 3), "profile_ms_min": round(p_min, 3), "profile_get_ms": round(get_ms, 3),
                         "profile_bytes_per_record": round(p_bytes / n, 2), "profile_GBps": round(p_bytes / (p_ms * 1e-3) / 1e9, 1),
                         "motif_ms_per_call_median": round(m_ms, 3), "motif_ms_min": round(m_min, 3),
                         "motif_bytes_per_record": round(m_bytes / n, 2), "motif_GBps": round(m_bytes / (m_ms * 1e-3) / 1e9, 1),
                         "profile_over_motif": round(p_ms / m_ms, 3), "kept": int(sc[:, 0].sum()), "in_grid": int(extra[:, :, 2].sum())})
            print(json.dumps(rows[-1]), flush=True)
            b.close()
        eng.genome_release(gid)
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(rows, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
