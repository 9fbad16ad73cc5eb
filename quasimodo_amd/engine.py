"""Engine / Batch: thin object layer over the C ABI (include/qmvt.h)."""
import ctypes as C
import os
import weakref

import numpy as np

from . import _lib
from ._lib import SCALAR_NAMES, QmvtError, SynthCfg, check

# include/qmvt.h QM_PATH_*: where the VCFs a finish found out of order went
PATH_NAMES = ("unsorted", "bucket_direct", "bucket_hashed", "radix", "radix_after_overflow", "bucket_chunks", "overflow_chunks",
              "radix_chunks", "bucket_two_level", "bucket_partitions")


def surface_params(q_step, nq, na):
    """the parameter triple of the filter surface as ints; ValueError names the argument outside its limits"""
    q_step, nq, na = int(q_step), int(nq), int(na)
    if not 1 <= q_step <= _lib.QM_SF_MAX_QUAL_STEP:
        raise ValueError("surface: q_step %d (1 to %d)" % (q_step, _lib.QM_SF_MAX_QUAL_STEP))
    if not 1 <= nq <= _lib.QM_SF_MAX_QUAL_BINS:
        raise ValueError("surface: nq %d (1 to %d)" % (nq, _lib.QM_SF_MAX_QUAL_BINS))
    if not 1 <= na <= _lib.QM_SF_MAX_AF_BINS:
        raise ValueError("surface: na %d (1 to %d)" % (na, _lib.QM_SF_MAX_AF_BINS))
    if nq * na > _lib.QM_SF_MAX_CELLS:
        raise ValueError("surface: nq * na = %d cells (at most %d)" % (nq * na, _lib.QM_SF_MAX_CELLS))
    return q_step, nq, na


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


# -- what the _files_<pass> builders make of a spec's lists.  None of these raises: each builder says its own lengths, with the
# len() of what it was given, before it hands out an array of max(n, 1) entries (never an empty buffer).
def _want(ws):   # a want list as uint8
    return _c([int(bool(w)) for w in ws] or [0], np.uint8)


def _ids(ids):   # genome or group ids as int32, None as -1
    return _c([-1 if g is None else int(g) for g in ids] or [-1], np.int32)


def _path_array(paths, n):   # n paths (None: no file) as a c_char_p array
    return (C.c_char_p * max(n, 1))(*[None if x is None else os.fsencode(x) for x in paths])


def _rows(n, *shape, dtype=np.uint64):   # the zeroed table the library fills: one row of `shape` per job or group
    return np.zeros((max(n, 1),) + shape, dtype)


def _mixed(wanted, job):   # the job asked for the pass and is no pure-strain sample (whose truth is never read: its row gains nothing)
    return bool(wanted) and not job.get("pure")


class Engine:
    """One context per process and GPU (qm_init).  Raises QmvtError(QM_E_NODEVICE)
    when no HIP device is usable -- there is no CPU path."""

    def __init__(self, device=0):
        self._L = _lib.lib()
        h = C.c_void_p()
        check(self._L.qm_init(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self._batches = weakref.WeakSet()   # a batch must not outlive its context (qm_batch_destroy uses it)
        self._genome_len = {}               # genome id -> bases, as loaded (genome_context sizes its array by it)

    def close(self):
        if getattr(self, "_h", None):
            for b in list(self._batches):
                b.close()
            self._L.qm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- truth sets -----------------------------------------------------------
    def truth_load(self, pos, ref, alt):
        pos, ref, alt = _c(pos, np.int32), _c(ref, np.int32), _c(alt, np.int32)
        tid = C.c_int(-1)
        check(self._L.qm_truth_load(self._h, _p(pos), _p(ref), _p(alt), pos.shape[0], C.byref(tid)), self._h)
        return tid.value

    def truth_synth(self, genome_len, truth_n, truth_seed, indel_pct=0):
        tid = C.c_int(-1)
        check(self._L.qm_truth_synth_ext(self._h, int(genome_len), int(truth_n), int(truth_seed), int(indel_pct), C.byref(tid)), self._h)
        return tid.value

    def truth_size(self, tid, alleles=False):
        """distinct single-base keys; alleles=True: distinct valid keys of any allele length"""
        n = C.c_int64()
        check((self._L.qm_truth_size_ext if alleles else self._L.qm_truth_size)(self._h, int(tid), C.byref(n)), self._h)
        return n.value

    def truth_release(self, tid):
        """free a truth set's HBM; its id may be reused by a later load"""
        check(self._L.qm_truth_release(self._h, int(tid)), self._h)

    @property
    def n_truth(self):
        return self._L.qm_truth_count(self._h)

    # -- genomes (mutation-context spectra) ---------------------
    def genome_load(self, seq):
        """one contig's raw bytes (motifs.read_fasta) into HBM; returns its id"""
        seq = bytes(seq)
        gid = C.c_int(-1)
        check(self._L.qm_genome_load(self._h, seq, len(seq), C.byref(gid)), self._h)
        self._genome_len[gid.value] = len(seq)
        return gid.value

    def genome_release(self, gid):
        check(self._L.qm_genome_release(self._h, int(gid)), self._h)

    def genome_context(self, gid, w=50, ng=10):
        """qm_genome_context: (cells uint8 [L] -- the context cell of every position, context.NONE_BYTE where it has none --,
        gen uint64 [16 ng + 1] -- positions per cell) of a loaded genome, by the kernel the pass uses; context.cells restates it"""
        from .context import check_params
        w, ng = check_params(w, ng)
        L = int(self._genome_len.get(int(gid), 0))   # (an id never loaded: the library refuses it)
        cells, gen = np.zeros(L, np.uint8), np.zeros(16 * ng + 1, np.uint64)
        check(self._L.qm_genome_context(self._h, int(gid), w, ng, _p(cells), _p(gen)), self._h)
        return cells, gen

    def truth_entries(self, tid):
        """qm_truth_entries: (pos, ref, alt) int32 -- the allele-extended entries of a truth set in the order of its table"""
        cap = max(self.truth_size(tid, alleles=True), 1)
        pos, ref, alt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int64()
        check(self._L.qm_truth_entries(self._h, int(tid), _p(pos), _p(ref), _p(alt), cap, C.byref(n)), self._h)
        return pos[:n.value], ref[:n.value], alt[:n.value]

    def truth_normalized(self, tid, gid):
        """qm_truth_normalized: (pos, ref, alt) int32 -- the distinct forms (normalize.py) of a truth set's
        allele-extended entries against a loaded genome, sorted by (pos, ref, alt), from the kernels the pass uses"""
        cap = max(self.truth_size(tid, alleles=True), 1)
        pos, ref, alt = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int64()
        check(self._L.qm_truth_normalized(self._h, int(tid), int(gid), _p(pos), _p(ref), _p(alt), cap, C.byref(n)), self._h)
        return pos[:n.value], ref[:n.value], alt[:n.value]

    def truth_sites(self, tid, gid, gap=None):
        """qm_truth_sites: (first_entry, lo, hi) int32 -- the sites (haplo.py) of a truth set's allele-extended
        entries against a loaded genome: the first entry and the window of each, from the kernels the pass uses"""
        from .haplo import check_gap
        cap = max(self.truth_size(tid, alleles=True), 1)
        first, lo, hi = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        n = C.c_int64()
        check(self._L.qm_truth_sites(self._h, int(tid), int(gid), check_gap(gap), _p(first), _p(lo), _p(hi), cap, C.byref(n)), self._h)
        return first[:n.value], lo[:n.value], hi[:n.value]

    def truth_atoms(self, tid):
        """qm_truth_atoms: uint32 -- the atom set (atomize.py) of a truth set's allele-extended entries, each atom
        (pos << 4) | (ref << 2) | alt, sorted ascending, from the kernel the pass uses"""
        n = C.c_int64()
        rc = self._L.qm_truth_atoms(self._h, int(tid), None, 0, C.byref(n))      # (how many: QM_E_RANGE unless there is none)
        if rc not in (0, -5):                                                    # QM_E_RANGE
            check(rc, self._h)
        keys = np.zeros(max(n.value, 1), np.uint32)
        check(self._L.qm_truth_atoms(self._h, int(tid), _p(keys), keys.shape[0], C.byref(n)), self._h)
        return keys[:n.value]

    # -- strata sets (counts per genome region) -------------------
    def strata_load(self, strata):
        """strata: list of (name, starts, ends) BED intervals (quasimodo_amd.strata); returns the set's id"""
        from .strata import check as check_strata
        st = check_strata(strata)
        offs = np.zeros(len(st) + 1, np.int64)
        offs[1:] = np.cumsum([s.shape[0] for _, s, _ in st])
        start = _c(np.concatenate([s for _, s, _ in st] + [np.zeros(1, np.int64)]), np.int32)   # (never an empty buffer)
        end = _c(np.concatenate([e for _, _, e in st] + [np.zeros(1, np.int64)]), np.int32)
        sid = C.c_int(-1)
        check(self._L.qm_strata_load(self._h, len(st), _p(offs), _p(start), _p(end), C.byref(sid)), self._h)
        return sid.value

    def strata_info(self, sid):
        """(strata, segments of the flattened table)"""
        info = np.zeros(2, np.int64)
        check(self._L.qm_strata_info(self._h, int(sid), _p(info)), self._h)
        return int(info[0]), int(info[1])

    def strata_segments(self, sid):
        """the flattened table as the library built it: (breakpoints int32 [m], masks uint32 [m]); strata.flatten restates it"""
        m = self.strata_info(sid)[1]
        b, k = np.zeros(m, np.int32), np.zeros(m, np.uint32)
        check(self._L.qm_strata_segments(self._h, int(sid), _p(b), _p(k)), self._h)
        return b, k

    def strata_release(self, sid):
        check(self._L.qm_strata_release(self._h, int(sid)), self._h)

    # -- one-shot ---------------------------------------------------------------
    def classify_batch(self, columns, truth_ids, n_bins=256, alleles=False):
        """columns: list of (pos, ref, alt, qual, flags) per VCF.  Returns (per-VCF result dicts,
        per-truth sums): what qm_classify_batch computes (include/qmvt.h), through the resident-batch
        entry points so that each VCF's arrays are uploaded from where they are (no concatenation).
        alleles=True: the allele-extended mode (QM_BATCH_ALLELES)."""
        n_vcf = len(columns)
        if n_vcf == 0:
            return [], np.zeros((max(self.n_truth, 1), 3, n_bins), np.uint64)
        sizes = [int(np.asarray(c[0]).shape[0]) for c in columns]
        b = Batch(self, sizes, truth_ids, n_bins, alleles)
        try:
            for v, c in enumerate(columns):
                b.upload(v, *c)
            b.run()
            b.finish()
            roc, scal, glob = b.roc(), b.scalars(), b.global_counts()
            out = []
            for v in range(n_vcf):
                s = dict(zip(SCALAR_NAMES, scal[v].tolist()))
                reg = b.idx(v)
                out.append({"cls": b.cls(v), "roc": roc[v].copy(), "scalars": s,
                            "tp_idx": reg[:s["tp_lines"]].copy(), "fp_idx": reg[sizes[v] - s["fp_lines"]:].copy()})
        finally:
            b.close()
        return out, glob

    def classify_batch_oneshot(self, columns, truth_ids, n_bins=256, alleles=False):
        """The same through the single C call qm_classify_batch(_ext) on concatenated host buffers."""
        n_vcf = len(columns)
        sizes = [int(np.asarray(c[0]).shape[0]) for c in columns]
        offs = np.zeros(n_vcf + 1, np.int64)
        offs[1:] = np.cumsum(sizes)
        N = int(offs[-1])
        cat = lambda k, dt: _c(np.concatenate([np.asarray(c[k], dtype=dt) for c in columns]) if n_vcf else np.zeros(0, dt), dt)
        pos, ref, alt = cat(0, np.int32), cat(1, np.int32), cat(2, np.int32)
        qual, flags = cat(3, np.float32), cat(4, np.uint8)
        tids = _c(truth_ids, np.int32)
        cls = np.zeros(max(N, 1), np.uint8)
        idx = np.zeros(max(N, 1), np.int32)
        roc = np.zeros((n_vcf, 3, n_bins), np.uint64)
        scal = np.zeros((n_vcf, _lib.QM_N_SCALARS), np.int64)
        glob = np.zeros((max(self.n_truth, 1), 3, n_bins), np.uint64)
        check(self._L.qm_classify_batch_ext(self._h, n_vcf, _p(offs), _p(pos), _p(ref), _p(alt), _p(qual), _p(flags), _p(tids),
                                            int(n_bins), _lib.QM_BATCH_ALLELES if alleles else 0, _p(cls), _p(roc), _p(scal),
                                            _p(idx), _p(glob)), self._h)
        out = []
        for v in range(n_vcf):
            a, b = int(offs[v]), int(offs[v + 1])
            s = dict(zip(SCALAR_NAMES, scal[v].tolist()))
            reg = idx[a:b]
            out.append({"cls": cls[a:b].copy(), "roc": roc[v].copy(), "scalars": s,
                        "tp_idx": reg[:s["tp_lines"]].copy(), "fp_idx": reg[(b - a) - s["fp_lines"]:].copy()})
        return out, glob

    def bench_synth(self, n_vcf, records, genome_len, truth_n, truth_seed=3, seed=3000, n_bins=256, steps=5, shuffled=False, indel_pct=0):
        """qm_bench_synth: one self-contained synthetic run inside the library."""
        cfg = SynthCfg(int(genome_len), int(seed), int(truth_seed), int(truth_n), int(bool(shuffled)), int(indel_pct))
        r = _lib.BenchResult()
        check(self._L.qm_bench_synth(self._h, C.byref(cfg), int(n_vcf), int(records), int(n_bins), int(steps), C.byref(r)), self._h)
        return {k: getattr(r, k) for k, _ in r._fields_ if k != "reserved"}

    def extract_files(self, file_jobs, n_bins=256, alleles=False, strict=True, truth_slots=None, n_slots=0, global_dev=None, genomes=None,
                      truthside=None, profile=None, strata=None, boot=None, votes=None, nearmiss=None, surface=None, context=None, normalize=None,
                      atomize=None, vartype=None, haplo=None, hapsub=None, rescue_roc=None, ladder=None, ladder_types=None):
        """qm_extract_files(_ex): files in, files out, everything between in the library (host threads + ONE engine batch).
        file_jobs: list of dicts vcf / truth / mode ("hcmv" | "custom") / pure / filtered / tp / fp.
        truth_slots / n_slots / global_dev (device pointer, int): one rank of a multi-GPU run -- the per-truth-file sums of
        this call's VCFs land in rows truth_slots[j] of the caller's [n_slots][3][n_bins] uint64 device buffer (cleared first).
        genomes: per-job genome ids (genome_load) or None / -1; when any job has one, qm_extract_files_motifs runs and every row
        gains `motifs` ([3][QM_MOTIF_COLS] uint64: kept, TP, FP).
        truthside: {"fn": [path or None per job], "group": [group id or -1 per job], "missed": [path or None per group]} --
        qm_extract_files_truthside: the missed-variant lists are written, the rows of grouped jobs gain
        `truth_regions` and `fp_regions` (int64 [32] each, the same for every member; members in job order).
        profile: {"want": [0/1 per job], "window": 1024, "n_pos_bins": 256, "n_af_bins": 20, "points": [path or None per job]} --
        qm_extract_files_profile: wanted rows gain `af_grid` ([2][n_af_bins][n_pos_bins] uint64: TP, FP) and
        `af_extra` ([2][QM_AFP_EXTRA]); the points files are written.
        strata: {"id": strata_load id, "want": [0/1 per job]} -- qm_extract_files_strata: wanted rows gain
        `strata_rec` ([S + 2][3] uint64: kept, TP, FP lines per stratum, outside, nokey) and `strata_tru` ([S + 1][2]: truth keys,
        hit ones; None in the allele-extended mode).
        boot: {"want": [0/1 per job], "window": 1024, "n_win": 256, "n_rep": 1000, "seed": 0} -- qm_extract_files_boot (DESIGN.md
        4.11): wanted rows gain `boot_cnt` ([n_win + 2][4] uint64: kept lines, TP lines, truth keys, hit keys per window, then
        outside, nokey) and `boot_rep` ([n_rep][4], the bootstrap replicates of the four sums).
        votes: {"group": [group id or -1 per job], "k": [consensus level or 0 per group], "out": [path or None per group]} --
        qm_extract_files_votes: the rows of grouped jobs gain `tp_votes`, `fp_votes` ([33] uint64), `private_tp`,
        `private_fp` ([32]; the same for every member, members in job order) and `vote_member` (the job's index in its group);
        the consensus VCFs of the groups with a level are written.
        nearmiss: {"radius": 0 .. 64, "want": [0/1 per job], "fp_why": [path or None per job], "fn_why": [path or None per job]} --
        qm_extract_files_nearmiss: wanted mixed-sample rows gain `nearmiss_rec` ([6] ints: the FP lines per class
        nearmiss.RECORD_CLASSES) and `nearmiss_tru` ([5]: the missed truth keys per class nearmiss.TRUTH_CLASSES); the why-files
        are written.
        surface: {"want": [0/1 per job], "q_step": 4, "nq": 64, "na": 50} -- qm_extract_files_surface: wanted rows
        gain `surface` ([3][nq][na] uint64: TP records, FP records, found truth keys under QUAL >= i * q_step and AF >= k / na),
        `surface_extra` ([QM_SF_EXTRA] ints: counted, counted without AF, left out, T') and `surface_params` (q_step, nq, na).
        context: {"genomes": [genome_load id or None / -1 per job], "half_window": 50, "n_gc": 10} -- qm_extract_files_context
        (DESIGN.md 4.16): the rows of jobs with a genome gain `context_rec` ([16 n_gc + 2][3] uint64: kept, TP, FP lines per cell,
        none, nokey), `context_tru` ([16 n_gc + 1][2]: truth keys, hit ones; None in the allele-extended mode), `context_gen`
        ([16 n_gc + 1]: positions of the genome per cell) and `context_params` (half_window, n_gc).
        normalize: {"genomes": [genome_load id or None / -1 per job], "rescued": [path or None per job]} --
        qm_extract_files_normalize (alleles=True only): the rows of mixed-sample jobs with a genome gain `norm_rec`
        ([12] uint64, columns normalize.R_COLS) and `norm_tru` ([5], normalize.T_COLS); the rescued-lines files are written.
        atomize: {"want": [0/1 per job], "atoms": [path or None per job]} -- qm_extract_files_atomize (alleles=True
        only): wanted rows gain `atom_rec` ([13] uint64, columns atomize.R_COLS) and `atom_tru` ([6], atomize.T_COLS); the atoms
        files are written.
        vartype: {"want": [0/1 per job], "edges": None or the size edges} -- qm_extract_files_types (alleles=True
        only): wanted mixed-sample rows gain `type_rec` and `type_tru` ([n_rows][2] uint64, rows vartype.row_names(edges)) and
        `type_edges`.
        haplo: {"genomes": [genome_load id or None / -1 per job], "gap": None or 0 .. 32, "sites": [path or None per job], "seqs":
        [the genome's bytes per job that names a sites file]} -- qm_extract_files_haplotypes (alleles=True only):
        the rows of mixed-sample jobs with a genome gain `hap_rec` ([16] uint64, columns haplo.R_COLS), `hap_tru` ([8],
        haplo.T_COLS) and `hap_gap`; the sites files are written.
        hapsub: the dict of haplo plus "subsets": [path or None per job] -- qm_extract_files_hapsubsets, in place
        of haplo: the same rows and sites files, `hap_sub` ([8] uint64, columns haplo.SUB_COLS) and the subsets files.
        rescue_roc: {"genomes": [genome_load id or None / -1 per job], "want": [0/1 per job]} -- qm_extract_files_rescue_roc
        (alleles=True only), in place of normalize and atomize, which it runs itself: wanted mixed-sample rows gain
        `rroc_n`, `rroc_a` ([3][n_bins] uint64: TP(t), FP(t), U(t) by normal form and by atoms, laid out like `roc`) and `rroc_base`
        ([2]: the distinct forms and the entries of the truth set).
        ladder: {"genomes": [genome_load id or None / -1 per job], "want": [0/1 per job], "gap": None or 0 .. 32, "subsets": True,
        "out": [path or None per job]} -- qm_extract_files_ladder (alleles=True only), in place of normalize,
        atomize, haplo and hapsub, which it runs itself: wanted mixed-sample rows gain `ladder_rec` and `ladder_tru` ([18] uint64,
        columns ladder.COLS / ladder.T_COLS); the ladder files are written.
        ladder_types: {"genomes": [genome_load id or None / -1 per job], "want": [0/1 per job], "gap": None or 0 .. 32, "subsets":
        True, "edges": None or the size edges} -- qm_extract_files_ladder_types (alleles=True only), in place of
        ladder and vartype, which it runs itself behind the four rescues: wanted mixed-sample rows gain `ladder_types_rec` and
        `ladder_types_tru` ([n_rows][18] uint64: rows vartype.row_names(edges), columns ladder.COLS / ladder.T_COLS) and
        `ladder_types_edges`.
        Which of these may share a call: quasimodo_amd.passes (ValueError otherwise).
        Returns (list of per-VCF dicts: scalars by name + n_lines, genomediff, header_kept, host_decided, roc; phase seconds)."""
        from .passes import check_alleles, check_shared_call
        n = len(file_jobs)
        gids = None if genomes is None else _c([-1 if g is None else int(g) for g in genomes], np.int32)
        if gids is not None and gids.shape[0] != n:
            raise ValueError("genomes: %d entries for %d jobs" % (gids.shape[0], n))
        if gids is not None and not (gids >= 0).any():
            gids = None
        specs = {"motifs": gids, "truthside": truthside, "profile": profile, "strata": strata, "boot": boot, "votes": votes, "nearmiss": nearmiss, "context": context, "normalize": normalize, "atomize": atomize, "haplo": haplo, "hapsub": hapsub, "vartype": vartype, "surface": surface, "rescueroc": rescue_roc, "ladder": ladder, "laddertypes": ladder_types}
        requested = {name for name, spec in specs.items() if spec is not None}
        check_shared_call(requested)
        check_alleles(requested, alleles)
        arr = (_lib.FileJob * max(n, 1))()
        enc = lambda p: None if p is None else os.fsencode(p)
        for k, j in enumerate(file_jobs):
            arr[k] = _lib.FileJob(enc(j["vcf"]), enc(j.get("truth")), 1 if j.get("mode", "hcmv") == "custom" else 0, int(bool(j.get("pure"))),
                                  enc(j["filtered"]), enc(j.get("tp")), enc(j["fp"]))
        st = (_lib.FileStats * max(n, 1))()
        roc = np.zeros((max(n, 1), 3, n_bins), np.uint64)
        ph = (C.c_double * 8)()
        slots = None if truth_slots is None else _c(list(truth_slots) + [0] * (1 if n == 0 else 0), np.int32)
        args = (self._h, n, arr, int(n_bins), _lib.QM_BATCH_ALLELES if alleles else 0, int(bool(strict)), st, _p(roc), ph,
                _p(slots), int(n_slots), C.c_void_p(global_dev) if global_dev else None)
        # the call's pass (check_shared_call left one; motifs may come with profile, whose entry point takes both)
        entry, extra, unpack = self._L.qm_extract_files_ex, (), lambda k: {}
        for name, spec in specs.items():
            if spec is not None and not (name == "motifs" and profile is not None):
                entry, extra, unpack = getattr(self, "_files_" + name)(n, spec, gids=gids, alleles=alleles, file_jobs=file_jobs, n_bins=int(n_bins))
        check(entry(*args, *extra), self._h)
        rows = []
        for k in range(n):
            r = dict(zip(SCALAR_NAMES, list(st[k].scalars)))
            r.update(n_lines=st[k].n_lines, n_refused=st[k].n_refused, genomediff=st[k].genomediff,
                     header_kept=(st[k].header_kept, st[k].header_kept_tp), host_decided=st[k].host_decided, r_hostile=st[k].r_hostile,
                     roc=roc[k].copy())
            r.update(unpack(k))
            rows.append(r)
        phases = dict(zip(("map_count", "truth_beside", "batch_layout", "tokenise_upload", "engine", "masks_back", "write", "release"), list(ph)))
        return rows, phases

    # -- the passes of extract_files: (entry point, its arguments behind the common ones, row k -> what the job's row gains) --
    def _files_motifs(self, n, spec, gids=None, **kw):   # (spec: the genome ids themselves)
        motifs = _rows(n, 3, _lib.QM_MOTIF_COLS)
        return self._L.qm_extract_files_motifs, (_p(gids), _p(motifs)), lambda k: {"motifs": motifs[k].copy()}

    def _files_profile(self, n, profile, gids=None, **kw):
        want = _want(profile["want"])
        pts = list(profile.get("points") or [None] * n)
        if (n and want.shape[0] != n) or len(pts) != n:
            raise ValueError("profile: %d want / %d points entries for %d jobs" % (len(profile["want"]), len(pts), n))
        nA, nP = int(profile.get("n_af_bins", 20)), int(profile.get("n_pos_bins", 256))
        if nA < 1 or nP < 1 or nA * nP > _lib.QM_AFP_MAX_CELLS:
            raise ValueError("profile: %d x %d bins (at most %d cells)" % (nA, nP, _lib.QM_AFP_MAX_CELLS))
        afg, afx = _rows(n, 2, nA, nP), _rows(n, 2, _lib.QM_AFP_EXTRA)
        pa = _lib.ProfileArgs(_p(want), int(profile.get("window", 1024)), nP, nA, 0, _p(afg), _p(afx), _path_array(pts, n))
        motifs = None if gids is None else _rows(n, 3, _lib.QM_MOTIF_COLS)

        def unpack(k):
            r = {} if motifs is None else {"motifs": motifs[k].copy()}
            return dict(r, af_grid=afg[k].copy(), af_extra=afx[k].copy()) if want[k] else r
        return self._L.qm_extract_files_profile, (_p(gids), _p(motifs), C.byref(pa)), unpack

    def _files_truthside(self, n, truthside, **kw):
        grp = _ids(truthside["group"])
        ng = len(truthside.get("missed") or []) or (int(grp.max()) + 1 if n else 0)
        if len(truthside["fn"]) != n or (n and grp.shape[0] != n):
            raise ValueError("truthside: %d fn / %d group entries for %d jobs" % (len(truthside["fn"]), grp.shape[0], n))
        regs, fregs = _rows(ng, _lib.QM_TRUTH_REGIONS), _rows(ng, _lib.QM_TRUTH_REGIONS, dtype=np.int64)
        ta = _lib.TruthSideArgs(_path_array(truthside["fn"], n), _p(grp), ng, 0, _p(regs), _p(fregs), _path_array(truthside.get("missed") or [None] * ng, ng))
        unpack = lambda k: {"truth_regions": regs[grp[k]].astype(np.int64), "fp_regions": fregs[grp[k]].copy()} if grp[k] >= 0 else {}
        return self._L.qm_extract_files_truthside, (C.byref(ta),), unpack

    def _files_strata(self, n, strata, alleles=False, **kw):
        swant = _want(strata["want"])
        if n and swant.shape[0] != n:
            raise ValueError("strata: %d want entries for %d jobs" % (len(strata["want"]), n))
        S = self.strata_info(strata["id"])[0]
        srec, stru = _rows(n, S + 2, 3), _rows(n, S + 1, 2)
        sa = _lib.StrataArgs(int(strata["id"]), 0, _p(swant), _p(srec), _p(stru))
        unpack = lambda k: {"strata_rec": srec[k].copy(), "strata_tru": None if alleles else stru[k].copy()} if swant[k] else {}
        return self._L.qm_extract_files_strata, (C.byref(sa),), unpack

    def _files_context(self, n, context, alleles=False, **kw):
        from .context import check_params, n_cells
        w, ng = check_params(context.get("half_window", 50), context.get("n_gc", 10))
        cgid = _ids(context["genomes"])
        if n and cgid.shape[0] != n:
            raise ValueError("context: %d genomes entries for %d jobs" % (len(context["genomes"]), n))
        nc = n_cells(ng)
        crec, ctru, cgen = _rows(n, nc + 1, 3), _rows(n, nc, 2), _rows(n, nc)
        ca = _lib.ContextArgs(w, ng, _p(cgid), _p(crec), _p(ctru), _p(cgen))
        ca.keep = cgid   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"context_rec": crec[k].copy(), "context_tru": None if alleles else ctru[k].copy(), "context_gen": cgen[k].copy(),
                            "context_params": (w, ng)} if cgid[k] >= 0 else {}
        return self._L.qm_extract_files_context, (C.byref(ca),), unpack

    def _files_normalize(self, n, normalize, file_jobs=(), **kw):
        ngid = _ids(normalize["genomes"])
        paths = list(normalize.get("rescued") or [None] * n)
        if (n and ngid.shape[0] != n) or len(paths) != n:
            raise ValueError("normalize: %d genomes / %d rescued entries for %d jobs" % (len(normalize["genomes"]), len(paths), n))
        nrec, ntru, out_arr = _rows(n, _lib.QM_NORM_R_COLS), _rows(n, _lib.QM_NORM_T_COLS), _path_array(paths, n)
        na = _lib.NormalizeArgs(_p(ngid), _p(nrec), _p(ntru), out_arr)
        na.keep = (ngid, out_arr)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"norm_rec": nrec[k].copy(), "norm_tru": ntru[k].copy()} if _mixed(ngid[k] >= 0, file_jobs[k]) else {}
        return self._L.qm_extract_files_normalize, (C.byref(na),), unpack

    def _files_atomize(self, n, atomize, **kw):
        awant = _want(atomize["want"])
        paths = list(atomize.get("atoms") or [None] * n)
        if (n and awant.shape[0] != n) or len(paths) != n:
            raise ValueError("atomize: %d want / %d atoms entries for %d jobs" % (len(atomize["want"]), len(paths), n))
        arec, atru, out_arr = _rows(n, _lib.QM_ATOM_R_COLS), _rows(n, _lib.QM_ATOM_T_COLS), _path_array(paths, n)
        aa = _lib.AtomizeArgs(_p(awant), _p(arec), _p(atru), out_arr)
        aa.keep = (awant, out_arr)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"atom_rec": arec[k].copy(), "atom_tru": atru[k].copy()} if awant[k] else {}
        return self._L.qm_extract_files_atomize, (C.byref(aa),), unpack

    def _files_rescue_roc(self, n, rescue_roc, file_jobs=(), n_bins=256, **kw):
        rgid, rwant = _ids(rescue_roc["genomes"]), _want(rescue_roc["want"])
        if n and (rgid.shape[0] != n or rwant.shape[0] != n):
            raise ValueError("rescue_roc: %d genomes / %d want entries for %d jobs" % (len(rescue_roc["genomes"]), len(rescue_roc["want"]), n))
        rn, ra, base = _rows(n, 3, n_bins), _rows(n, 3, n_bins), _rows(n, 2)
        args = _lib.RescueRocArgs(_p(rgid), _p(rwant), _p(rn), _p(ra), _p(base))
        args.keep = (rgid, rwant)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"rroc_n": rn[k].copy(), "rroc_a": ra[k].copy(), "rroc_base": base[k].copy()} if _mixed(rwant[k], file_jobs[k]) else {}
        return self._L.qm_extract_files_rescue_roc, (C.byref(args),), unpack

    _files_rescueroc = _files_rescue_roc   # (the pass's name in quasimodo_amd.passes)

    def _files_ladder(self, n, ladder, file_jobs=(), **kw):
        from .haplo import check_gap
        lgid, lwant = _ids(ladder["genomes"]), _want(ladder["want"])
        paths = list(ladder.get("out") or [None] * n)
        if (n and (lgid.shape[0] != n or lwant.shape[0] != n)) or len(paths) != n:
            raise ValueError("ladder: %d genomes / %d want / %d out entries for %d jobs" % (len(ladder["genomes"]), len(ladder["want"]), len(paths), n))
        rec, tru, out_arr = _rows(n, _lib.QM_LADDER_COLS), _rows(n, _lib.QM_LADDER_COLS), _path_array(paths, n)
        args = _lib.LadderArgs(_p(lgid), check_gap(ladder.get("gap")), 1 if ladder.get("subsets", True) else 0, _p(lwant), _p(rec), _p(tru), out_arr)
        args.keep = (lgid, lwant, out_arr)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"ladder_rec": rec[k].copy(), "ladder_tru": tru[k].copy()} if _mixed(lwant[k], file_jobs[k]) else {}
        return self._L.qm_extract_files_ladder, (C.byref(args),), unpack

    def _files_ladder_types(self, n, ladder_types, file_jobs=(), **kw):
        from .haplo import check_gap
        from .vartype import check_edges, n_rows
        edges = check_edges(ladder_types.get("edges"))
        lgid, lwant = _ids(ladder_types["genomes"]), _want(ladder_types["want"])
        if n and (lgid.shape[0] != n or lwant.shape[0] != n):
            raise ValueError("ladder_types: %d genomes / %d want entries for %d jobs" % (len(ladder_types["genomes"]), len(ladder_types["want"]), n))
        e = _c(edges, np.int32)
        rec, tru = _rows(n, n_rows(edges), _lib.QM_LADDER_COLS), _rows(n, n_rows(edges), _lib.QM_LADDER_COLS)
        args = _lib.LadderTypesArgs(_p(lgid), check_gap(ladder_types.get("gap")), 1 if ladder_types.get("subsets", True) else 0, _p(lwant), _p(e),
                                    len(edges), 0, _p(rec), _p(tru))
        args.keep = (lgid, lwant, e)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: ({"ladder_types_rec": rec[k].copy(), "ladder_types_tru": tru[k].copy(), "ladder_types_edges": edges}
                            if _mixed(lwant[k], file_jobs[k]) else {})
        return self._L.qm_extract_files_ladder_types, (C.byref(args),), unpack

    _files_laddertypes = _files_ladder_types   # (the pass's name in quasimodo_amd.passes)

    def _files_vartype(self, n, vartype, file_jobs=(), **kw):
        from .vartype import check_edges, n_rows
        edges = check_edges(vartype.get("edges"))
        twant = _want(vartype["want"])
        if n and twant.shape[0] != n:
            raise ValueError("vartype: %d want entries for %d jobs" % (len(vartype["want"]), n))
        e = _c(edges, np.int32)
        trec, ttru = _rows(n, n_rows(edges), 2), _rows(n, n_rows(edges), 2)
        ta = _lib.TypesArgs(_p(e), len(edges), 0, _p(twant), _p(trec), _p(ttru))
        ta.keep = (e, twant)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"type_rec": trec[k].copy(), "type_tru": ttru[k].copy(), "type_edges": edges} if _mixed(twant[k], file_jobs[k]) else {}
        return self._L.qm_extract_files_types, (C.byref(ta),), unpack

    def _files_haplo(self, n, spec, file_jobs=(), subsets=False, **kw):
        """spec: the dict `haplo` takes (gap, genomes, sites, seqs); subsets (_files_hapsub): plus "subsets": [path or None per job] -- the
        haplotype pass and the search behind it from one call; a job that names either file needs its genome's bytes in `seqs`"""
        from .haplo import check_gap
        gap = check_gap(spec.get("gap"))
        hgid = _ids(spec["genomes"])
        paths, seqs, subs = (list(spec.get(key) or [None] * n) for key in ("sites", "seqs", "subsets"))
        short = (n and hgid.shape[0] != n) or len(paths) != n or len(seqs) != n
        if subsets and (short or len(subs) != n):
            raise ValueError("hapsub: %d genomes / %d sites / %d seqs / %d subsets entries for %d jobs" % (len(spec["genomes"]), len(paths), len(seqs), len(subs), n))
        if short:
            raise ValueError("haplo: %d genomes / %d sites / %d seqs entries for %d jobs" % (len(spec["genomes"]), len(paths), len(seqs), n))
        hrec, htru, out_arr = _rows(n, _lib.QM_HAP_R_COLS), _rows(n, _lib.QM_HAP_T_COLS), _path_array(paths, n)
        seqs = [None if x is None else bytes(x) for x in seqs]
        seq_arr = (C.c_char_p * max(n, 1))(*seqs)
        lens = _c([0 if x is None else len(x) for x in seqs] or [0], np.int64)
        common = (_p(hgid), gap, 0, _p(hrec), _p(htru), out_arr, seq_arr, _p(lens))
        took = lambda k: _mixed(hgid[k] >= 0, file_jobs[k])
        if not subsets:
            ha = _lib.HaplotypesArgs(*common)
            ha.keep = (hgid, out_arr, seqs, seq_arr, lens)   # (read during the call; the other arrays live in unpack)
            unpack = lambda k: {"hap_rec": hrec[k].copy(), "hap_tru": htru[k].copy(), "hap_gap": gap} if took(k) else {}
            return self._L.qm_extract_files_haplotypes, (C.byref(ha),), unpack
        hsub, sub_arr = _rows(n, _lib.QM_HAPSUB_COLS), _path_array(subs, n)
        ha = _lib.HapsubArgs(*common, _p(hsub), sub_arr)
        ha.keep = (hgid, out_arr, sub_arr, seqs, seq_arr, lens)   # (read during the call; the other arrays live in unpack)
        unpack = lambda k: {"hap_rec": hrec[k].copy(), "hap_tru": htru[k].copy(), "hap_gap": gap, "hap_sub": hsub[k].copy()} if took(k) else {}
        return self._L.qm_extract_files_hapsubsets, (C.byref(ha),), unpack

    def _files_hapsub(self, n, hapsub, file_jobs=(), **kw):
        return Engine._files_haplo(self, n, hapsub, file_jobs, subsets=True)

    def _files_boot(self, n, boot, **kw):
        bwant = _want(boot["want"])
        if n and bwant.shape[0] != n:
            raise ValueError("boot: %d want entries for %d jobs" % (len(boot["want"]), n))
        bw, bn, br = int(boot.get("window", 1024)), int(boot.get("n_win", 256)), int(boot.get("n_rep", 1000))
        if bw < 1 or not 1 <= bn <= _lib.QM_BOOT_MAX_WINDOWS or not 0 <= br <= _lib.QM_BOOT_MAX_REP:
            raise ValueError("boot: window %d, n_win %d (1 to %d), n_rep %d (0 to %d)" % (bw, bn, _lib.QM_BOOT_MAX_WINDOWS, br, _lib.QM_BOOT_MAX_REP))
        bcnt, brep = _rows(n, bn + 2, 4), _rows(n, max(br, 1), 4)
        ba = _lib.BootArgs(bw, bn, br, 0, int(boot.get("seed", 0)) & ((1 << 64) - 1), _p(bwant), _p(bcnt), _p(brep))
        unpack = lambda k: {"boot_cnt": bcnt[k].copy(), "boot_rep": brep[k, :br].copy()} if bwant[k] else {}
        return self._L.qm_extract_files_boot, (C.byref(ba),), unpack

    def _files_votes(self, n, votes, **kw):
        vgrp = _ids(votes["group"])
        if n and vgrp.shape[0] != n:
            raise ValueError("votes: %d group entries for %d jobs" % (vgrp.shape[0], n))
        vng = (int(vgrp.max()) + 1) if n else 0
        vk = _c(list(votes.get("k") or [0] * vng) or [0], np.int32)
        vout = list(votes.get("out") or [None] * vng)
        if vng and (vk.shape[0] != vng or len(vout) != vng):
            raise ValueError("votes: %d levels / %d files for %d groups" % (vk.shape[0], len(vout), vng))
        vtab = [_rows(vng, w) for w in (_lib.QM_VOTE_SLOTS, _lib.QM_VOTE_SLOTS, _lib.QM_VOTE_GROUP_MAX, _lib.QM_VOTE_GROUP_MAX)]
        va = _lib.VotesArgs(_p(vgrp), vng, 0, _p(vtab[0]), _p(vtab[1]), _p(vtab[2]), _p(vtab[3]), _p(vk), _path_array(vout, vng))
        va.keep = vk   # (the levels are read during the call; the other arrays live in unpack)

        def unpack(k):
            g = int(vgrp[k])
            return {} if g < 0 else dict(zip(("tp_votes", "fp_votes", "private_tp", "private_fp"), (t[g].copy() for t in vtab)),
                                         vote_member=int((vgrp[:k] == g).sum()))
        return self._L.qm_extract_files_votes, (C.byref(va),), unpack

    def _files_nearmiss(self, n, nearmiss, file_jobs=(), **kw):
        nwant = _want(nearmiss["want"])
        fpw, fnw = (list(nearmiss.get(k) or [None] * n) for k in ("fp_why", "fn_why"))
        if (n and nwant.shape[0] != n) or len(fpw) != n or len(fnw) != n:
            raise ValueError("nearmiss: %d want / %d fp_why / %d fn_why entries for %d jobs" % (len(nearmiss["want"]), len(fpw), len(fnw), n))
        radius = int(nearmiss["radius"])
        if not 0 <= radius <= _lib.QM_NM_MAX_RADIUS:
            raise ValueError("nearmiss: radius %d (0 to %d)" % (radius, _lib.QM_NM_MAX_RADIUS))
        nrec, ntru = _rows(n, _lib.QM_NM_R_CLASSES), _rows(n, _lib.QM_NM_T_CLASSES)
        na = _lib.NearmissArgs(_p(nwant), radius, 0, _p(nrec), _p(ntru), _path_array(fpw, n), _path_array(fnw, n))
        unpack = lambda k: {"nearmiss_rec": [int(x) for x in nrec[k]], "nearmiss_tru": [int(x) for x in ntru[k]],
                            "nearmiss_radius": radius} if _mixed(nwant[k], file_jobs[k]) else {}
        return self._L.qm_extract_files_nearmiss, (C.byref(na),), unpack

    def _files_surface(self, n, surface, **kw):
        swant = _want(surface["want"])
        if n and swant.shape[0] != n:
            raise ValueError("surface: %d want entries for %d jobs" % (len(surface["want"]), n))
        q, nq, na = surface_params(surface.get("q_step", 4), surface.get("nq", 64), surface.get("na", 50))
        S, ex = _rows(n, 3, nq, na), _rows(n, _lib.QM_SF_EXTRA)
        sa = _lib.SurfaceArgs(_p(swant), q, nq, na, 0, _p(S), _p(ex))
        unpack = lambda k: {"surface": S[k].copy(), "surface_extra": [int(x) for x in ex[k]], "surface_params": (q, nq, na)} if swant[k] else {}
        return self._L.qm_extract_files_surface, (C.byref(sa),), unpack

    def path_stats_total(self):
        """qm_path_stats_total: where the VCFs found out of order went, summed over every batch this context has finished
        (PATH_NAMES); take the difference around a call."""
        out = np.zeros(len(PATH_NAMES), np.int64)
        check(self._L.qm_path_stats_total(self._h, _p(out)), self._h)
        return dict(zip(PATH_NAMES, (int(x) for x in out)))

    def bw_probe(self, nbytes=4 << 30, reps=5):
        """qm_bw_probe: GB/s this GPU streams read-only, copying (read + written) and write-only"""
        out = (C.c_double * 3)()
        check(self._L.qm_bw_probe(self._h, int(nbytes), int(reps), out), self._h)
        return {"read_GBps": out[0], "copy_GBps": out[1], "write_GBps": out[2]}

    def fp_overlap(self, key_sets):
        """key_sets: list of (pos, ref, alt) arrays, one per caller.  Returns region
        counts indexed by membership mask (snpcaller_fp_compare.R:36-47)."""
        n = len(key_sets)
        offs = np.zeros(n + 1, np.int64)
        offs[1:] = np.cumsum([np.asarray(k[0]).shape[0] for k in key_sets])
        cat = lambda j: _c(np.concatenate([np.asarray(k[j], np.int32) for k in key_sets]) if n else np.zeros(0, np.int32), np.int32)
        pos, ref, alt = cat(0), cat(1), cat(2)
        reg = np.zeros(1 << n, np.int64)
        check(self._L.qm_fp_overlap(self._h, n, _p(offs), _p(pos), _p(ref), _p(alt), _p(reg)), self._h)
        return reg

    def batch(self, n_records, truth_ids, n_bins=256, alleles=False):
        return Batch(self, n_records, truth_ids, n_bins, alleles)


class Batch:
    """Resident batch: columns stay in HBM across runs (qm_batch_*)."""

    def __init__(self, engine, n_records, truth_ids, n_bins=256, alleles=False):
        self.engine = engine
        self._L = engine._L
        self.n_records = _c(n_records, np.int64)
        self.truth_ids = _c(truth_ids, np.int32)
        self.n_vcf = int(self.n_records.shape[0])
        self.n_bins = int(n_bins)
        h = C.c_void_p()
        self.alleles = bool(alleles)
        check(self._L.qm_batch_create_ext(engine._h, self.n_vcf, _p(self.n_records), _p(self.truth_ids), self.n_bins,
                                          _lib.QM_BATCH_ALLELES if alleles else 0, C.byref(h)), engine._h)
        self._h = h
        self._boot = None   # (n_win, n_rep) of the latest boot() that the library accepted
        engine._batches.add(self)

    def close(self):
        if getattr(self, "_h", None):
            self._L.qm_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        return check(rc, self.engine._h)

    def upload(self, v, pos, ref, alt, qual, flags):
        a = (_c(pos, np.int32), _c(ref, np.int32), _c(alt, np.int32), _c(qual, np.float32), _c(flags, np.uint8))
        if any(x.shape[0] != int(self.n_records[v]) for x in a):
            raise ValueError("column length != n_records[%d]" % v)
        self._ck(self._L.qm_batch_upload(self._h, int(v), *[_p(x) for x in a]))

    def synth(self, genome_len, truth_n, truth_seed, seed, shuffled=False, indel_pct=0):
        """truth_seed=None: every VCF is generated against the synthetic truth set it was assigned (per-VCF truth sets)"""
        ts = 0xffffffffffffffff if truth_seed is None else int(truth_seed)
        cfg = SynthCfg(int(genome_len), int(seed), ts, int(truth_n), int(shuffled), int(indel_pct))   # True = 1: permuted; R >= 2: R ascending runs
        self._ck(self._L.qm_batch_synth(self._h, C.byref(cfg)))

    def set_timing(self, on=True):
        self._ck(self._L.qm_batch_set_timing(self._h, int(on)))

    def run(self, stream=None, global_dev=None):
        """Enqueue classify -> finalize -> compact.  stream: raw hipStream_t (int) or None;
        global_dev: device pointer (int) of a [n_truth][3][n_bins] uint64 buffer or None."""
        self._ck(self._L.qm_batch_run(self._h, C.c_void_p(stream) if stream else None,
                                      C.c_void_p(global_dev) if global_dev else None))

    def finish(self, stream=None):
        self._ck(self._L.qm_batch_finish(self._h, C.c_void_p(stream) if stream else None))

    def _pass_timings(self, entry, names):
        """the qm_batch_*_timings of one pass: its milliseconds under their names"""
        ms = (C.c_float * len(names))()
        self._ck(entry(self._h, ms))
        return dict(zip(names, ms))

    def timings(self):
        ms = (C.c_float * 4)()
        self._ck(self._L.qm_batch_timings(self._h, ms))
        return {"classify_ms": ms[0], "finalize_ms": ms[1], "compact_ms": ms[2], "total_ms": ms[3]}

    def cls(self, v):
        out = np.zeros(max(int(self.n_records[v]), 1), np.uint8)
        self._ck(self._L.qm_batch_get_cls(self._h, int(v), _p(out)))
        return out[:int(self.n_records[v])]

    def idx(self, v):
        out = np.zeros(max(int(self.n_records[v]), 1), np.int32)
        self._ck(self._L.qm_batch_get_idx(self._h, int(v), _p(out)))
        return out[:int(self.n_records[v])]

    def roc(self):
        out = np.zeros((self.n_vcf, 3, self.n_bins), np.uint64)
        self._ck(self._L.qm_batch_get_roc(self._h, _p(out)))
        return out

    def scalars(self):
        out = np.zeros((self.n_vcf, _lib.QM_N_SCALARS), np.int64)
        self._ck(self._L.qm_batch_get_scalars(self._h, _p(out)))
        return out

    @property
    def n_truth(self):
        """rows of the per-truth sums: truth-set slots of the context when the batch was created"""
        return int(self._L.qm_batch_n_truth(self._h))

    def global_counts(self):
        out = np.zeros((self.n_truth, 3, self.n_bins), np.uint64)
        self._ck(self._L.qm_batch_get_global(self._h, _p(out)))
        return out

    def columns(self, v):
        n = int(self.n_records[v])
        pos, ref, alt = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        qual, flags = np.zeros(n, np.float32), np.zeros(n, np.uint8)
        self._ck(self._L.qm_batch_get_columns(self._h, int(v), _p(pos), _p(ref), _p(alt), _p(qual), _p(flags)))
        return pos, ref, alt, qual, flags

    def motifs(self, genome_ids, stream=None):
        """qm_batch_motifs: enqueue the mutation-context pass of the finished batch (genome_ids: one genome id or -1 per VCF)"""
        g = _c(genome_ids, np.int32)
        if g.shape[0] != self.n_vcf:
            raise ValueError("genome_ids: %d entries for %d VCFs" % (g.shape[0], self.n_vcf))
        self._ck(self._L.qm_batch_motifs(self._h, _p(g), C.c_void_p(stream) if stream else None))

    def motif_counts(self):
        """qm_batch_get_motifs: [n_vcf][3][QM_MOTIF_COLS] uint64 (rows kept, TP, FP; columns motifs.MOTIFS, outside, REF mismatch)"""
        out = np.zeros((self.n_vcf, 3, _lib.QM_MOTIF_COLS), np.uint64)
        self._ck(self._L.qm_batch_get_motifs(self._h, _p(out)))
        return out

    # -- allele-frequency profiles --------------------------------
    def upload_af(self, v, af):
        """qm_batch_upload_af: the allele frequencies of VCF v (float32 [n_records[v]], NaN = none), after its columns"""
        a = _c(af, np.float32)
        if a.shape[0] != int(self.n_records[v]):
            raise ValueError("column length != n_records[%d]" % v)
        self._ck(self._L.qm_batch_upload_af(self._h, int(v), _p(a) if a.shape[0] else _p(np.zeros(1, np.float32))))

    def af_profile(self, window=1024, n_pos_bins=256, n_af_bins=20, stream=None):
        """qm_batch_af_profile: enqueue the AF x position pass of the finished batch"""
        self._ck(self._L.qm_batch_af_profile(self._h, int(window), int(n_pos_bins), int(n_af_bins), C.c_void_p(stream) if stream else None))
        self._af_shape = (int(n_af_bins), int(n_pos_bins))

    def af_profile_counts(self):
        """qm_batch_get_af_profile: (grid [n_vcf][2][n_af_bins][n_pos_bins], extra [n_vcf][2][QM_AFP_EXTRA]) uint64; class 0 = TP,
        1 = FP; extra columns QM_AFP_NO_AF, QM_AFP_OUTSIDE, QM_AFP_N_GRID"""
        nA, nP = getattr(self, "_af_shape", (1, 1))
        grid = np.zeros((self.n_vcf, 2, nA, nP), np.uint64)
        extra = np.zeros((self.n_vcf, 2, _lib.QM_AFP_EXTRA), np.uint64)
        self._ck(self._L.qm_batch_get_af_profile(self._h, _p(grid), _p(extra)))
        return grid, extra

    # -- counts per genome region ---------------------------------
    def strata(self, strata_id, truth=False, stream=None):
        """qm_batch_strata: enqueue the record side of the finished batch; truth=True: the truth side too (needs truth_hits)"""
        what = _lib.QM_STRATA_RECORDS | (_lib.QM_STRATA_TRUTH if truth else 0)
        self._ck(self._L.qm_batch_strata(self._h, int(strata_id), what, C.c_void_p(stream) if stream else None))
        self._strata = (self.engine.strata_info(strata_id)[0], bool(truth))

    def strata_counts(self):
        """qm_batch_get_strata: (rec [n_vcf][S + 2][3] uint64 -- kept, TP, FP lines; rows the strata, outside, nokey --,
        tru [n_vcf][S + 1][2] -- truth keys, hit ones; rows the strata, outside -- or None when the truth side was not made)"""
        S, truth = getattr(self, "_strata", (1, False))
        rec = np.zeros((self.n_vcf, S + 2, 3), np.uint64)
        tru = np.zeros((self.n_vcf, S + 1, 2), np.uint64) if truth else None
        self._ck(self._L.qm_batch_get_strata(self._h, _p(rec), _p(tru)))
        return rec, tru

    # -- paired block-bootstrap replicates ------------------------
    def boot(self, window=1024, n_win=256, n_rep=1000, seed=0, truth=False, stream=None):
        """qm_batch_boot: enqueue the window counts of the finished batch's record side and n_rep replicates of their sums;
        truth=True: the truth side too (needs truth_hits)"""
        what = _lib.QM_BOOT_RECORDS | (_lib.QM_BOOT_TRUTH if truth else 0)
        self._ck(self._L.qm_batch_boot(self._h, int(window), int(n_win), int(n_rep), int(seed) & ((1 << 64) - 1), what,
                                       C.c_void_p(stream) if stream else None))
        self._boot = (int(n_win), int(n_rep))   # (a refused call leaves the library's latest pass, and this, as they were)

    def boot_counts(self):
        """qm_batch_get_boot: (cnt [n_vcf][n_win + 2][4] uint64 -- kept lines, TP lines, truth keys, hit keys; rows the windows,
        outside, nokey --, rep [n_vcf][n_rep][4]: the replicates of the four sums)"""
        if self._boot is None:   # the host arrays are sized by the pass this wrapper enqueued: none, so nothing to copy into
            raise QmvtError(-6, "boot_counts: no Batch.boot on this batch")
        n_win, n_rep = self._boot
        cnt = np.zeros((self.n_vcf, n_win + 2, 4), np.uint64)
        rep = np.zeros((self.n_vcf, n_rep, 4), np.uint64)
        self._ck(self._L.qm_batch_get_boot(self._h, _p(cnt), _p(rep) if n_rep and self.n_vcf else None))
        return cnt, rep

    # -- the truth-side view -------------------------------------
    def truth_hits(self, stream=None):
        """qm_batch_truth_hits: enqueue the truth-side pass of the finished batch (hit bitmaps + the in-truth record mask)"""
        self._ck(self._L.qm_batch_truth_hits(self._h, C.c_void_p(stream) if stream else None))

    def truth_hit_bits(self, v):
        """qm_batch_get_truth_hits: bool[T'] -- entry k: some kept record of VCF v carries key k of the truth set's sorted
        distinct keys (pos << 4 | ref << 2 | alt); its sum is the device's QM_S_TP_R"""
        t = self.engine.truth_size(int(self.truth_ids[int(v)]))
        w = np.zeros((t + 31) // 32, np.uint32)
        self._ck(self._L.qm_batch_get_truth_hits(self._h, int(v), _p(w), int(w.shape[0])))
        bits = np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)
        if bits[t:].any():
            raise RuntimeError("qm_batch_get_truth_hits: bits set beyond T' = %d" % t)
        return bits[:t]

    def intruth_mask(self, v):
        """qm_batch_get_intruth_mask: bool[n] -- record r of VCF v is kept, has a comparable key, and the key is in the truth set"""
        n = int(self.n_records[int(v)])
        w = np.zeros((n + 63) // 64, np.uint64)
        self._ck(self._L.qm_batch_get_intruth_mask(self._h, int(v), _p(w) if n else _p(np.zeros(1, np.uint64))))
        return np.unpackbits(w.view(np.uint8), bitorder="little").astype(bool)[:n]

    def truth_regions(self, groups, union=False):
        """qm_batch_truth_regions.  groups: lists of 1..5 VCF ids that share a truth set.  Returns int64 [n_groups][32]:
        [g][m] = truth keys whose membership mask over group g is m (bit i = groups[g][i] hit it; slot 0 = missed by all).
        union=True: also a list of bool[T'] per group, the keys some member hit."""
        groups = [[int(v) for v in g] for g in groups]
        offs = np.zeros(len(groups) + 1, np.int32)
        offs[1:] = np.cumsum([len(g) for g in groups])
        ids = _c([v for g in groups for v in g] or [0], np.int32)
        reg = np.zeros((max(len(groups), 1), _lib.QM_TRUTH_REGIONS), np.uint64)
        ts, uni = [], None
        if union:
            for g in groups:   # (a group the library will refuse gets no room: it fails before it writes)
                ok = g and all(0 <= v < self.n_vcf for v in g)
                ts.append(self.engine.truth_size(int(self.truth_ids[g[0]])) if ok else 0)
            uni = np.zeros(max(sum((t + 31) // 32 for t in ts), 1), np.uint32)
        self._ck(self._L.qm_batch_truth_regions(self._h, len(groups), _p(offs), _p(ids), _p(reg), _p(uni) if union else None))
        reg = reg[:len(groups)].astype(np.int64)
        if not union:
            return reg
        out, o = [], 0
        for t in ts:
            nw = (t + 31) // 32
            out.append(np.unpackbits(uni[o:o + nw].view(np.uint8), bitorder="little").astype(bool)[:t])
            o += nw
        return reg, out

    # -- k-of-n caller consensus ----------------------------------
    def votes(self, groups, stream=None):
        """qm_batch_votes: enqueue the vote pass of the finished batch (needs truth_hits).  groups: lists of 1..32 VCF ids that
        share a truth set, a VCF in at most one of them."""
        groups = [[int(v) for v in g] for g in groups]
        offs = np.zeros(len(groups) + 1, np.int32)
        offs[1:] = np.cumsum([len(g) for g in groups])
        ids = _c([v for g in groups for v in g] or [0], np.int32)
        self._ck(self._L.qm_batch_votes(self._h, len(groups), _p(offs), _p(ids), C.c_void_p(stream) if stream else None))

    def vote_counts(self):
        """qm_batch_get_votes: dict of tp_votes, fp_votes [n_groups][33], private_tp, private_fp [n_groups][32] (uint64) and
        nokey [n_groups] (int64).  [g][c] = keys of group g that exactly c members call (tp: truth keys, c = 0 missed by all;
        fp: distinct keys outside the truth set); private_*[g][i] = keys only member i calls."""
        ng = self._ck(self._L.qm_batch_vote_groups(self._h))   # the library's count: the arrays fit whoever enqueued the pass
        m = max(ng, 1)
        out = {"tp_votes": np.zeros((m, _lib.QM_VOTE_SLOTS), np.uint64), "fp_votes": np.zeros((m, _lib.QM_VOTE_SLOTS), np.uint64),
               "private_tp": np.zeros((m, _lib.QM_VOTE_GROUP_MAX), np.uint64), "private_fp": np.zeros((m, _lib.QM_VOTE_GROUP_MAX), np.uint64),
               "nokey": np.zeros(m, np.int64)}
        self._ck(self._L.qm_batch_get_votes(self._h, _p(out["tp_votes"]), _p(out["fp_votes"]), _p(out["private_tp"]), _p(out["private_fp"]),
                                            _p(out["nokey"])))
        return {k: v[:ng] for k, v in out.items()}

    def vote_timings(self):
        """qm_batch_vote_timings (set_timing on): milliseconds of the latest votes() between HIP events, stage by stage"""
        return self._pass_timings(self._L.qm_batch_vote_timings, ("vote_truth_ms", "vote_keys_ms", "sort_ms", "vote_runs_ms"))

    def vote_keys(self, g):
        """qm_batch_get_vote_keys: (ukeys, umasks) uint32 -- the ascending distinct keys pos << 4 | ref << 2 | alt of group g
        outside the truth set, and per key the mask of the members that call it (bit i = member i)"""
        n = C.c_int64(0)
        self._ck(self._L.qm_batch_get_vote_keys(self._h, int(g), None, None, 0, C.byref(n)))
        keys, masks = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32)
        self._ck(self._L.qm_batch_get_vote_keys(self._h, int(g), _p(keys), _p(masks), int(keys.shape[0]), C.byref(n)))
        return keys[:n.value], masks[:n.value]

    # -- the filter surface ---------------------------------------
    def surface(self, q_step=4, nq=64, na=50, stream=None, fetch=True):
        """qm_batch_surface + qm_batch_get_surface: (S [n_vcf][3][nq][na], extra [n_vcf][QM_SF_EXTRA]) uint64 -- TP records, FP
        records and found truth keys of every VCF under the filter QUAL >= i * q_step and AF >= k / na; extra: counted records,
        counted records without AF, single-base records without a quality bin, T'.  fetch=False: enqueue only (surface_counts()
        waits and copies)"""
        self._ck(self._L.qm_batch_surface(self._h, int(q_step), int(nq), int(na), C.c_void_p(stream) if stream else None))
        self._sf_shape = (int(nq), int(na))
        return self.surface_counts() if fetch else None

    def surface_counts(self):
        """qm_batch_get_surface: the tables of the latest surface()"""
        nq, na = getattr(self, "_sf_shape", (1, 1))
        S = np.zeros((max(self.n_vcf, 1), 3, nq, na), np.uint64)
        extra = np.zeros((max(self.n_vcf, 1), _lib.QM_SF_EXTRA), np.uint64)
        self._ck(self._L.qm_batch_get_surface(self._h, _p(S), _p(extra)))
        return S[:self.n_vcf], extra[:self.n_vcf]

    def surface_timings(self):
        """qm_batch_surface_timings (set_timing on): milliseconds of the latest surface() between HIP events, kernel by kernel"""
        return self._pass_timings(self._L.qm_batch_surface_timings, ("surface_records_ms", "surface_truth_ms", "surface_sums_ms"))

    # -- sequence-context profiles ----------------------------------
    def context(self, genome_ids, half_window=50, n_gc=10, truth=False, stream=None, fetch=True):
        """qm_batch_context + qm_batch_get_context: the counts of the finished batch per homopolymer x GC cell (genome_ids: one
        genome id or -1 per VCF); truth=True: the truth side too (needs truth_hits).  fetch=False: enqueue only
        (context_counts() waits and copies)"""
        from .context import check_params
        w, ng = check_params(half_window, n_gc)
        g = _c(genome_ids, np.int32)
        if g.shape[0] != self.n_vcf:
            raise ValueError("genome_ids: %d entries for %d VCFs" % (g.shape[0], self.n_vcf))
        what = _lib.QM_CX_RECORDS | (_lib.QM_CX_TRUTH if truth else 0)
        self._ck(self._L.qm_batch_context(self._h, _p(g) if self.n_vcf else _p(np.zeros(1, np.int32)), w, ng, what,
                                          C.c_void_p(stream) if stream else None))
        self._context = (ng, bool(truth))   # (a refused call leaves the library's latest pass, and this, as they were)
        return self.context_counts() if fetch else None

    def context_counts(self):
        """qm_batch_get_context: (rec [n_vcf][n_cells + 1][3] uint64 -- kept, TP, FP lines; rows the cells hp * n_gc + gc_bin,
        NONE, nokey --, tru [n_vcf][n_cells][2] -- truth keys, hit ones -- or None when the truth side was not made,
        gen [n_vcf][n_cells] -- positions per cell of each VCF's genome); n_cells = 16 n_gc + 1"""
        ng, truth = getattr(self, "_context", (1, False))
        nc, nv = 16 * ng + 1, max(self.n_vcf, 1)
        rec = np.zeros((nv, nc + 1, 3), np.uint64)
        tru = np.zeros((nv, nc, 2), np.uint64) if truth else None
        gen = np.zeros((nv, nc), np.uint64)
        self._ck(self._L.qm_batch_get_context(self._h, _p(rec), _p(tru), _p(gen)))
        return rec[:self.n_vcf], None if tru is None else tru[:self.n_vcf], gen[:self.n_vcf]

    def context_timings(self):
        """qm_batch_context_timings (set_timing on): milliseconds of the latest context() between HIP events"""
        return self._pass_timings(self._L.qm_batch_context_timings, ("context_build_ms", "context_records_ms", "context_truth_ms"))

    # -- indels and MNPs matched by normal form ------------------------
    def normalize(self, genome_ids, columns=False, stream=None, fetch=True):
        """qm_batch_normalize + qm_batch_get_normalize (allele-extended batches): (rec [n_vcf][12], tru [n_vcf][5]) uint64, columns
        normalize.R_COLS / normalize.T_COLS (genome_ids: one genome id or -1 per VCF); columns=True keeps every record's form for
        normalized().  fetch=False: enqueue only (normalize_counts() waits and copies)"""
        g = _c(genome_ids, np.int32)
        if g.shape[0] != self.n_vcf:
            raise ValueError("genome_ids: %d entries for %d VCFs" % (g.shape[0], self.n_vcf))
        self._ck(self._L.qm_batch_normalize(self._h, _p(g) if self.n_vcf else _p(np.zeros(1, np.int32)),
                                            _lib.QM_NORM_COLUMNS if columns else 0, C.c_void_p(stream) if stream else None))
        return self.normalize_counts() if fetch else None

    def normalize_counts(self):
        """qm_batch_get_normalize: the counts of the latest normalize()"""
        rec = np.zeros((max(self.n_vcf, 1), _lib.QM_NORM_R_COLS), np.uint64)
        tru = np.zeros((max(self.n_vcf, 1), _lib.QM_NORM_T_COLS), np.uint64)
        self._ck(self._L.qm_batch_get_normalize(self._h, _p(rec), _p(tru)))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def normalized(self, v, columns=True):
        """qm_batch_get_normalized: (pos, ref, alt int32 [n] -- every record's form as allele codes --, cls uint8 [n] -- the class
        bytes normalize.CLASS_NAMES --, truth_row int32 [n] -- the smallest truth entry index with that form, -1 for none) of VCF
        v in input order; columns=False: (cls,) alone, for a normalize() that kept no columns"""
        n = int(self.n_records[int(v)])
        cls = np.zeros(max(n, 1), np.uint8)
        if not columns:
            self._ck(self._L.qm_batch_get_normalized(self._h, int(v), None, None, None, _p(cls), None))
            return (cls[:n],)
        cols = [np.zeros(max(n, 1), np.int32) for _ in range(4)]
        self._ck(self._L.qm_batch_get_normalized(self._h, int(v), _p(cols[0]), _p(cols[1]), _p(cols[2]), _p(cls), _p(cols[3])))
        return cols[0][:n], cols[1][:n], cols[2][:n], cls[:n], cols[3][:n]

    def normalize_timings(self):
        """qm_batch_normalize_timings (set_timing on): milliseconds of the latest normalize() between HIP events"""
        return self._pass_timings(self._L.qm_batch_normalize_timings, ("norm_truth_ms", "norm_records_ms", "norm_found_ms"))

    # -- MNPs matched against adjacent SNVs ----------------------------
    def atomize(self, columns=False, stream=None, fetch=True):
        """qm_batch_atomize + qm_batch_get_atomize (allele-extended batches): (rec [n_vcf][13], tru [n_vcf][6]) uint64, columns
        atomize.R_COLS / atomize.T_COLS; columns=True keeps every record's class byte, atom count and hit mask for atomized().
        fetch=False: enqueue only (atomize_counts() waits and copies)"""
        self._ck(self._L.qm_batch_atomize(self._h, _lib.QM_ATOM_COLUMNS if columns else 0, C.c_void_p(stream) if stream else None))
        return self.atomize_counts() if fetch else None

    def atomize_counts(self):
        """qm_batch_get_atomize: the counts of the latest atomize()"""
        rec = np.zeros((max(self.n_vcf, 1), _lib.QM_ATOM_R_COLS), np.uint64)
        tru = np.zeros((max(self.n_vcf, 1), _lib.QM_ATOM_T_COLS), np.uint64)
        self._ck(self._L.qm_batch_get_atomize(self._h, _p(rec), _p(tru)))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def atomized(self, v):
        """qm_batch_get_atomized: (cls uint8 [n] -- the class bytes atomize.CLASS_NAMES --, n_atoms uint8 [n], hit_mask uint16
        [n]) of VCF v in input order, after an atomize(columns=True)"""
        n = int(self.n_records[int(v)])
        cls, na, hm = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint16)
        self._ck(self._L.qm_batch_get_atomized(self._h, int(v), _p(cls), _p(na), _p(hm)))
        return cls[:n], na[:n], hm[:n]

    def atomize_timings(self):
        """qm_batch_atomize_timings (set_timing on): milliseconds of the latest atomize() between HIP events"""
        return self._pass_timings(self._L.qm_batch_atomize_timings, ("atom_truth_ms", "atom_records_ms", "atom_found_ms"))

    # -- TP, FP and FN by variant type and size ------------------------
    def vartype(self, edges=None, shapes=None, columns=False, stream=None, fetch=True):
        """qm_batch_types + qm_batch_get_types (allele-extended batches): (rec, tru) uint64 [n_vcf][n_rows][2] -- per row
        (vartype.row_names(edges)) the kept records and the TP lines among them, the truth entries and the found ones.  edges:
        the ascending lower edges of the size bins (None: vartype.DEFAULT_EDGES); shapes: the (len, head, tail) rows of the
        dictionary ids (AlleleDict.shapes, vartype.shapes_of) or None; columns=True keeps every record's row byte for vartyped().
        fetch=False: enqueue only (vartype_counts() waits and copies)"""
        from .vartype import check_edges
        e = _c(check_edges(edges), np.int32)
        ln, head, tail = (None, None, None) if shapes is None else (_c(shapes[0], np.int32), _c(shapes[1], np.uint32), _c(shapes[2], np.uint32))
        n = 0 if shapes is None else int(ln.shape[0])
        if shapes is not None and not (head.shape[0] == tail.shape[0] == n):
            raise ValueError("vartype: shape columns of %d, %d and %d rows" % (n, head.shape[0], tail.shape[0]))
        self._ck(self._L.qm_batch_types(self._h, _p(e), int(e.shape[0]), _p(ln) if n else None, _p(head) if n else None, _p(tail) if n else None, n,
                                        _lib.QM_TYPE_COLUMNS if columns else 0, C.c_void_p(stream) if stream else None))
        self._type_rows = 5 * int(e.shape[0]) + 4
        return self.vartype_counts() if fetch else None

    def vartype_counts(self):
        """qm_batch_get_types: the counts of the latest vartype()"""
        nr = getattr(self, "_type_rows", _lib.QM_TYPE_MAX_ROWS)
        rec = np.zeros((max(self.n_vcf, 1), nr, 2), np.uint64)
        tru = np.zeros((max(self.n_vcf, 1), nr, 2), np.uint64)
        self._ck(self._L.qm_batch_get_types(self._h, _p(rec), _p(tru)))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def vartyped(self, v):
        """qm_batch_get_typed: the row (uint8 [n]) of every record of VCF v in input order, after a vartype(columns=True)"""
        n = int(self.n_records[int(v)])
        row = np.zeros(max(n, 1), np.uint8)
        self._ck(self._L.qm_batch_get_typed(self._h, int(v), _p(row)))
        return row[:n]

    def vartype_timings(self):
        """qm_batch_types_timings (set_timing on): milliseconds of the latest vartype() between HIP events"""
        return self._pass_timings(self._L.qm_batch_types_timings, ("type_records_ms", "type_truth_ms"))

    # -- clusters of records matched by replayed haplotype ----------------
    def haplotypes(self, genome_ids, gap=None, columns=False, stream=None, fetch=True):
        """qm_batch_haplotypes + qm_batch_get_haplotypes (allele-extended batches): (rec [n_vcf][16], tru [n_vcf][8]) uint64,
        columns haplo.R_COLS / haplo.T_COLS (genome_ids: one genome id or -1 per VCF; gap: 0 .. haplo.MAX_GAP, None:
        haplo.DEFAULT_GAP); columns=True keeps the class bytes and site indices for haplotyped().  fetch=False: enqueue only
        (haplotype_counts() waits and copies)"""
        from .haplo import check_gap
        g = _c(genome_ids, np.int32)
        if g.shape[0] != self.n_vcf:
            raise ValueError("genome_ids: %d entries for %d VCFs" % (g.shape[0], self.n_vcf))
        self._ck(self._L.qm_batch_haplotypes(self._h, _p(g) if self.n_vcf else _p(np.zeros(1, np.int32)), check_gap(gap),
                                             _lib.QM_HAP_COLUMNS if columns else 0, C.c_void_p(stream) if stream else None))
        return self.haplotype_counts() if fetch else None

    def haplotype_counts(self):
        """qm_batch_get_haplotypes: the counts of the latest haplotypes()"""
        rec = np.zeros((max(self.n_vcf, 1), _lib.QM_HAP_R_COLS), np.uint64)
        tru = np.zeros((max(self.n_vcf, 1), _lib.QM_HAP_T_COLS), np.uint64)
        self._ck(self._L.qm_batch_get_haplotypes(self._h, _p(rec), _p(tru)))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def haplotyped(self, v):
        """qm_batch_get_haplotyped: (cls uint8 [n] -- the class bytes haplo.CLASS_NAMES --, site int32 [n] -- the site of every
        usable record, -1 for none --, entry_cls uint8 [entries] -- a class byte per entry of the VCF's truth set) of VCF v in
        input order, after a haplotypes(columns=True)"""
        n = int(self.n_records[int(v)])
        ne = self.engine.truth_size(int(self.truth_ids[int(v)]), alleles=True)
        cls, site, ecls = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.int32), np.zeros(max(ne, 1), np.uint8)
        self._ck(self._L.qm_batch_get_haplotyped(self._h, int(v), _p(cls), _p(site), _p(ecls)))
        return cls[:n], site[:n], ecls[:ne]

    def haplotype_timings(self):
        """qm_batch_haplotype_timings (set_timing on): milliseconds of the latest haplotypes() between HIP events"""
        return self._pass_timings(self._L.qm_batch_haplotype_timings, ("hap_sites_ms", "hap_records_ms", "hap_truth_ms", "hap_claim_ms", "hap_replay_ms"))

    # -- a subset search inside the mismatched sites of the haplotype pass --
    def hapsubsets(self, columns=False, narrow_hash=False, stream=None, fetch=True):
        """qm_batch_hapsubsets + qm_batch_get_hapsubsets behind a haplotypes(): sub [n_vcf][8] uint64, columns haplo.SUB_COLS.
        columns=True (needs haplotypes(columns=True)) keeps the second class bytes for hapsubsetted(); narrow_hash=True is the
        self-check mode (hashes of 4 bits: the same results, bit for bit).  fetch=False: enqueue only (hapsubset_counts() waits
        and copies)"""
        what = (_lib.QM_HAPSUB_COLUMNS if columns else 0) | (_lib.QM_HAPSUB_NARROW_HASH if narrow_hash else 0)
        self._ck(self._L.qm_batch_hapsubsets(self._h, what, C.c_void_p(stream) if stream else None))
        return self.hapsubset_counts() if fetch else None

    def hapsubset_counts(self):
        """qm_batch_get_hapsubsets: the counts of the latest hapsubsets()"""
        sub = np.zeros((max(self.n_vcf, 1), _lib.QM_HAPSUB_COLS), np.uint64)
        self._ck(self._L.qm_batch_get_hapsubsets(self._h, _p(sub)))
        return sub[:self.n_vcf]

    def hapsubsetted(self, v, columns=True):
        """qm_batch_get_hapsubsetted: (cls_s uint8 [n], entry_cls_s uint8 [entries] -- the class bytes of haplotyped(v) but inside
        PARTIAL sites, where they are haplo.SUBSET or haplo.LEFT; None both without columns --, site int32 [m], smask uint8 [m],
        tmask uint8 [m] -- the PARTIAL sites of VCF v, ascending, and the masks of their optima over haplo.forms)"""
        n = int(self.n_records[int(v)])
        ne = self.engine.truth_size(int(self.truth_ids[int(v)]), alleles=True)
        cls, ecls = (np.zeros(max(n, 1), np.uint8), np.zeros(max(ne, 1), np.uint8)) if columns else (None, None)
        m = C.c_int64(0)
        self._ck(self._L.qm_batch_get_hapsubsetted(self._h, int(v), _p(cls) if columns else None, _p(ecls) if columns else None,
                                                   None, None, None, 0, C.byref(m)))
        k = int(m.value)
        site, sm, tm = np.zeros(max(k, 1), np.int32), np.zeros(max(k, 1), np.uint8), np.zeros(max(k, 1), np.uint8)
        self._ck(self._L.qm_batch_get_hapsubsetted(self._h, int(v), None, None, _p(site), _p(sm), _p(tm), k, C.byref(m)))
        return (cls[:n] if columns else None), (ecls[:ne] if columns else None), site[:k], sm[:k], tm[:k]

    def hapsubset_timings(self):
        """qm_batch_hapsubset_timings (set_timing on): milliseconds of the latest hapsubsets() between HIP events"""
        return self._pass_timings(self._L.qm_batch_hapsubset_timings, ("hap_subsets_ms",))

    # -- the QUAL ROC under normal-form and atom matching ---------------
    def rescue_roc(self, which=_lib.QM_RROC_NORM | _lib.QM_RROC_ATOM, stream=None, fetch=True):
        """qm_batch_rescue_roc + qm_batch_get_rescue_roc behind a normalize(columns=True) (QM_RROC_NORM) and / or an
        atomize(columns=True) (QM_RROC_ATOM): (roc_n, roc_a uint64 [n_vcf][3][n_bins] -- TP(t), FP(t), U(t) as roc() lays them
        out; None for a matching not asked for --, base uint64 [n_vcf][2] -- the forms and the entries of every VCF's truth
        set; FN_X(t) = base_X - U_X(t)).  fetch=False: enqueue only (rescue_roc_counts() waits and copies)"""
        self._ck(self._L.qm_batch_rescue_roc(self._h, int(which), C.c_void_p(stream) if stream else None))
        return self.rescue_roc_counts(which) if fetch else None

    def rescue_roc_counts(self, which=_lib.QM_RROC_NORM | _lib.QM_RROC_ATOM):
        """qm_batch_get_rescue_roc: the rows of the latest rescue_roc()"""
        shape = (max(self.n_vcf, 1), 3, self.n_bins)
        rn = np.zeros(shape, np.uint64) if which & _lib.QM_RROC_NORM else None
        ra = np.zeros(shape, np.uint64) if which & _lib.QM_RROC_ATOM else None
        base = np.zeros((max(self.n_vcf, 1), 2), np.uint64)
        self._ck(self._L.qm_batch_get_rescue_roc(self._h, _p(rn) if rn is not None else None, _p(ra) if ra is not None else None, _p(base)))
        return (rn[:self.n_vcf] if rn is not None else None), (ra[:self.n_vcf] if ra is not None else None), base[:self.n_vcf]

    def rescue_roc_timings(self):
        """qm_batch_rescue_roc_timings (set_timing on): milliseconds of the latest rescue_roc() between HIP events, kernel by kernel"""
        return self._pass_timings(self._L.qm_batch_rescue_roc_timings, ("rroc_norm_records_ms", "rroc_norm_units_ms", "rroc_atom_records_ms", "rroc_atom_units_ms"))

    # -- the four rescues combined: final TP, FP, FN and the Venn of methods --
    def ladder(self, subsets=False, columns=False, fetch=True, stream=None):
        """qm_batch_ladder + qm_batch_get_ladder behind normalize(columns=True), atomize(columns=True), haplotypes(columns=True)
        and -- subsets=True -- hapsubsets(columns=True): (rec, tru uint64 [n_vcf][18], columns ladder.COLS -- kept, TP lines and
        the 16 cells of the method bits over the kept lines that are no TP by spelling; entries, spelled-alike entries and the
        16 cells over the others).  columns=True keeps the mask bytes for laddered().  fetch=False: enqueue only
        (ladder_counts() waits and copies)"""
        what = (_lib.QM_LADDER_SUBSETS if subsets else 0) | (_lib.QM_LADDER_COLUMNS if columns else 0)
        self._ck(self._L.qm_batch_ladder(self._h, what, C.c_void_p(stream) if stream else None))
        return self.ladder_counts() if fetch else None

    def ladder_counts(self):
        """qm_batch_get_ladder: the counts of the latest ladder()"""
        rec = np.zeros((max(self.n_vcf, 1), _lib.QM_LADDER_COLS), np.uint64)
        tru = np.zeros((max(self.n_vcf, 1), _lib.QM_LADDER_COLS), np.uint64)
        self._ck(self._L.qm_batch_get_ladder(self._h, _p(rec), _p(tru)))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def laddered(self, v):
        """qm_batch_get_laddered: (mask uint8 [n] -- the mask byte of every record of VCF v in input order, bits ladder.S, K, N,
        A, H, B --, entry_mask uint8 [entries] -- that of every entry of its truth set), after a ladder(columns=True)"""
        n = int(self.n_records[int(v)])
        ne = self.engine.truth_size(int(self.truth_ids[int(v)]), alleles=True)
        mask, emask = np.zeros(max(n, 1), np.uint8), np.zeros(max(ne, 1), np.uint8)
        self._ck(self._L.qm_batch_get_laddered(self._h, int(v), _p(mask), _p(emask)))
        return mask[:n], emask[:ne]

    def ladder_timings(self):
        """qm_batch_ladder_timings (set_timing on): milliseconds of the latest ladder() between HIP events, kernel by kernel"""
        return self._pass_timings(self._L.qm_batch_ladder_timings, ("ladder_records_ms", "ladder_truth_ms"))

    # -- the match ladder per variant type and size ---------------------
    def ladder_types(self, fetch=True, stream=None):
        """qm_batch_ladder_types + qm_batch_get_ladder_types behind a vartype(columns=True) and a ladder(columns=True): (rec, tru
        uint64 [n_vcf][n_rows][18]) -- the rows of that vartype() (vartype.row_names(edges); records typed as spelled), the
        columns of the ladder (ladder.COLS / ladder.T_COLS).  fetch=False: enqueue only (ladder_type_counts() waits and
        copies)"""
        self._ck(self._L.qm_batch_ladder_types(self._h, C.c_void_p(stream) if stream else None))
        return self.ladder_type_counts() if fetch else None

    def ladder_type_counts(self):
        """qm_batch_get_ladder_types: the counts of the latest ladder_types()"""
        nr = C.c_int(0)
        self._ck(self._L.qm_batch_get_ladder_types(self._h, None, None, C.byref(nr)))
        rec = np.zeros((max(self.n_vcf, 1), max(nr.value, 1), _lib.QM_LADDER_COLS), np.uint64)
        tru = np.zeros_like(rec)
        self._ck(self._L.qm_batch_get_ladder_types(self._h, _p(rec), _p(tru), None))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def ladder_type_timings(self):
        """qm_batch_ladder_types_timings (set_timing on): milliseconds of the latest ladder_types() between HIP events, kernel by kernel"""
        return self._pass_timings(self._L.qm_batch_ladder_types_timings, ("ltype_records_ms", "ltype_truth_ms"))

    # -- near-miss classes of FP lines and missed truth keys --------
    def nearmiss(self, radius, stream=None):
        """qm_batch_nearmiss + qm_batch_get_nearmiss (needs truth_hits): (rec [n_vcf][6], tru [n_vcf][5]) uint64 -- the FP lines
        of every VCF per class nearmiss.RECORD_CLASSES, its missed truth keys per class nearmiss.TRUTH_CLASSES"""
        self._ck(self._L.qm_batch_nearmiss(self._h, int(radius), C.c_void_p(stream) if stream else None))
        return self.nearmiss_counts()

    def nearmiss_counts(self):
        """qm_batch_get_nearmiss: the counts of the latest nearmiss()"""
        rec = np.zeros((max(self.n_vcf, 1), _lib.QM_NM_R_CLASSES), np.uint64)
        tru = np.zeros((max(self.n_vcf, 1), _lib.QM_NM_T_CLASSES), np.uint64)
        self._ck(self._L.qm_batch_get_nearmiss(self._h, _p(rec), _p(tru)))
        return rec[:self.n_vcf], tru[:self.n_vcf]

    def nearmiss_timings(self):
        """qm_batch_nearmiss_timings (set_timing on): milliseconds of the latest nearmiss() between HIP events, kernel by kernel"""
        return self._pass_timings(self._L.qm_batch_nearmiss_timings, ("nearmiss_records_ms", "nearmiss_truth_ms"))

    def nearmiss_classes(self, v):
        """qm_batch_get_nearmiss_cls: uint8[n] -- the class of every FP line of VCF v in input order, 255 for the other records"""
        n = int(self.n_records[int(v)])
        out = np.zeros(max(n, 1), np.uint8)
        self._ck(self._L.qm_batch_get_nearmiss_cls(self._h, int(v), _p(out)))
        return out[:n]

    def nearmiss_truth(self, v):
        """qm_batch_get_nearmiss_truth: uint8[T'] -- the class of every missed key of VCF v's truth set (sorted distinct keys),
        255 for the keys it hit"""
        t = self.engine.truth_size(int(self.truth_ids[int(v)]))
        out = np.zeros(max(t, 1), np.uint8)
        self._ck(self._L.qm_batch_get_nearmiss_truth(self._h, int(v), _p(out)))
        return out[:t]

    def path_stats(self):
        """qm_batch_path_stats: where the VCFs the last finish found out of order went"""
        out = np.zeros(len(PATH_NAMES), np.int64)
        self._ck(self._L.qm_batch_path_stats(self._h, _p(out)))
        return dict(zip(PATH_NAMES, (int(x) for x in out)))

    @property
    def device_bytes(self):
        return int(self._L.qm_batch_device_bytes(self._h))
