#!/usr/bin/env python3
"""Two builds of libqmvt.so -- k_classify_pair with and without its plain path (make PAIRFLAGS=-DQM_PAIR_PLAIN=0) -- on the same
generated VCFs, compared bit for bit: class masks, ROC rows, scalars, class bits and both index lists (which are placed by the
tile counts), sorted and per contig (24 ascending runs).  Each build runs in a fresh child process through QM_LIBQMVT.

usage: python3 tools/pair_plain_ab.py <libqmvt.so A> <libqmvt.so B> [n_vcf] [records]"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
L, T, TSEED, SEED = 5_000_000, 100_000, 3, 3000


def child(out, nv, n):
    import ctypes as C
    sys.path.insert(0, ROOT)
    import quasimodo_amd as q
    res = {}
    with q.Engine(0) as eng:
        tid = eng.truth_synth(L, T, TSEED)
        for runs in (0, 24):
            b = eng.batch([n] * nv, [tid] * nv)
            b.synth(L, T, TSEED, SEED, shuffled=runs)
            b.run(); b.finish()
            sc = b.scalars()
            res["roc%d" % runs], res["scal%d" % runs] = b.roc(), sc
            for v in range(nv):
                kept, tp = np.zeros((n + 63) // 64, np.uint64), np.zeros((n + 63) // 64, np.uint64)
                b._ck(b._L.qm_batch_get_masks(b._h, v, kept.ctypes.data_as(C.c_void_p), tp.ctypes.data_as(C.c_void_p)))
                idx = b.idx(v)
                res["kept%d_%d" % (runs, v)], res["tp%d_%d" % (runs, v)], res["cls%d_%d" % (runs, v)] = kept, tp, b.cls(v)
                res["tpidx%d_%d" % (runs, v)], res["fpidx%d_%d" % (runs, v)] = idx[:int(sc[v, 1])], idx[n - int(sc[v, 2]):]
            b.close()
    np.savez(out, **res)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    nv = int(sys.argv[3]) if len(sys.argv) > 3 else 8
    n = int(sys.argv[4]) if len(sys.argv) > 4 else 200_000
    with tempfile.TemporaryDirectory() as tmp:
        got = []
        for i, lib in enumerate(libs):
            out = os.path.join(tmp, "arm%d.npz" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, str(nv), str(n)],
                           env=dict(os.environ, QM_LIBQMVT=lib), check=True, timeout=600)
            with np.load(out) as z:
                got.append({k: z[k] for k in z.files})
    a, b = got
    bad = [k for k in sorted(a) if k not in b or not np.array_equal(a[k], b[k])] + [k for k in sorted(b) if k not in a]
    kept = sum(int(a["scal0"][v, 0]) for v in range(nv))
    print("pair_plain_ab: %d VCFs x %d records, sorted and 24 runs: %d arrays compared, %d differ%s; kept records (sorted) %d"
          % (nv, n, len(a), len(bad), (": " + ", ".join(bad[:8])) if bad else "", kept), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
