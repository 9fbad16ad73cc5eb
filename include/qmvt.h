/*
 * qmvt.h -- C ABI of libqmvt.so, the MI355X (gfx950) variant-truth engine.
 *
 * The reference (hzi-bifo/Quasimodo v0.4.2) has no FFI for this path: its
 * boundary is a per-VCF process,
 *     python program/extract_TP_FP_SNPs.py <vcf> <truth> {hcmv,custom} <outdir> <caller>
 * (program/extract_TP_FP_SNPs.py:124-140, invoked by rules/extract_TP.smk:20 and
 * eval_variant_custom.smk:73) that shells out to awk/grep.  Each entry point
 * below names the reference stage it replaces.  All signatures are plain C:
 * pointers + sizes, no C++/torch types.  Return value: 0 = QM_OK, negative =
 * error (text via qm_last_error).  The library never falls back to a CPU
 * implementation of the classification: without a usable HIP device every
 * compute entry point fails with QM_E_NODEVICE.
 *
 * Column encoding (one record = one VCF data line):
 *   pos   int32  POS, 0 <= pos < 2^28 (canonical decimal spelling on the text side)
 *   ref   int32  0..3 = A,C,G,T; any other value = not a single-base allele
 *   alt   int32  same
 *   qual  float  "effective QUAL": floor(qual) >= t  <=>  the record passes the
 *                awk test `$6>=t` (t = 0..n_bins-1); '.' and passing non-numeric
 *                spellings are +inf, failing ones -inf
 *   flags uint8  bit0 QM_F_PASS  = line kept by the A2 filter (extract_TP_FP_SNPs.py:24)
 *                bit1 QM_F_IDDOT = ID column is exactly "." (a key match makes the line a TP line);
 *                                  cleared by qm_vcf_hostpath for a line it found NOT selected
 *                bit2 QM_F_NOKEY = the line has no comparable key (POS is not a canonical
 *                                  decimal): it can never be in the truth set; the packer
 *                                  gives it the previous record's pos so order is kept
 *                bit3 QM_F_TPLINE = the text side (qm_vcf_hostpath) found the line selected by
 *                                  `fgrep -wf` where the columns cannot tell (pattern aligned at
 *                                  other columns, POS spelled non-canonically, ...): a TP LINE
 *                                  whatever its key says; unique-key (R path) counts ignore it
 */
#ifndef QMVT_H
#define QMVT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QM_ABI_VERSION 6

#define QM_OK 0
#define QM_E_INVAL (-1)     /* bad argument */
#define QM_E_NODEVICE (-2)  /* no HIP device / HIP runtime failure at init */
#define QM_E_HIP (-3)       /* a HIP call failed */
#define QM_E_NOMEM (-4)
#define QM_E_RANGE (-5)     /* position outside [0, 2^28) */
#define QM_E_STATE (-6)     /* call order violated */
#define QM_E_IO (-7)
#define QM_E_NONCANON (-8)  /* text input the engine refuses to guess about (strict mode) */
#define QM_E_LIMIT (-9)     /* allele-extended batch: too many records at one position */
#define QM_E_UNSORTED (-10) /* qm_bgzf_write_tbi: sequences not in blocks or positions stepping backwards (tabix refuses such a VCF too) */
#define QM_E_COMM (-11)     /* the collective library (RCCL) is missing or one of its calls failed */

/* ---- allele-extended mode (QM_BATCH_ALLELES) ---------------------------------------------
 * BASELINE.json configs[4] (mixed SNP + indel, variable-length alleles).  The reference drops
 * every non-single-base record at its A2 filter, so this mode is a build-defined widening and is
 * OFF by default: `$4~/^[ACGT]$/&&$5~/^[ACGT]$/` becomes `$4~/^[ACGT]+$/&&$5~/^[ACGT]+$/`, in the
 * caller filter and in the truth pattern list alike; everything else (ID == ".", QUAL clause,
 * line / unique-key counts, ROC) is unchanged, and records with single-base alleles are
 * classified exactly as without the mode.
 * Allele codes (ref / alt columns, int32): two alleles are the same string iff their codes are equal.
 *   0..3                          one base A,C,G,T
 *   len << 26 | bases             2..13 bases inline: base k (0-based, A=0 C=1 G=2 T=3) in bits 2k+1..2k
 *   0x40000000 | id               longer alleles: id from a qm_dict (interned strings)
 *   negative, or 4..0x07ffffff    not an allele that takes part (as without the mode) */
#define QM_BATCH_ALLELES 1u
#define QM_ALLELE_NONE (-1)
#define QM_ALLELE_INLINE_MAX 13
#define QM_ALLELE_DICT 0x40000000

#define QM_F_PASS 1u
#define QM_F_IDDOT 2u
#define QM_F_NOKEY 4u
#define QM_F_TPLINE 8u

#define QM_CLS_KEPT 1u /* out_cls bit0: line is in <x>.filtered.vcf */
#define QM_CLS_TP 2u   /* out_cls bit1: line is in tp/<x>.tp.vcf (else, if kept, fp/) */

#define QM_MAX_BINS 256
#define QM_POS_LIMIT (1 << 28)

/* mutation-context spectra (qm_batch_motifs): per VCF [3][QM_MOTIF_COLS] uint64, rows kept / TP / FP (kept = TP + FP).
 * Columns 0..95: the 96 SomaticSignatures motifs "<ref><alt> <l>.<r>" in lexicographic order (REF folded to C / T, the
 * context reverse-complemented with it): 16 k + 4 base(l) + base(r), k = index of REF ALT in CA CG CT TA TC TG, A=0 C=1 G=2 T=3.
 * QM_MOTIF_OTHER: kept SNVs outside the 96 (QM_F_NOKEY, a flank outside the genome or not ACGTacgt, REF == ALT).
 * QM_MOTIF_REF_MISMATCH: of those in 0..95, the ones whose genome base differs from the VCF's REF (a diagnostic on top). */
#define QM_N_MOTIFS 96
#define QM_MOTIF_OTHER 96
#define QM_MOTIF_REF_MISMATCH 97
#define QM_MOTIF_COLS 98

/* allele-frequency profiles (qm_batch_af_profile): per VCF and class (0 = TP, 1 = FP) a grid
 * [n_af_bins][n_pos_bins] and QM_AFP_EXTRA further counts; every counted record is in exactly one of the three. */
#define QM_AFP_NO_AF 0    /* the record's allele frequency is NaN (INFO carries none the rule's pattern takes) */
#define QM_AFP_OUTSIDE 1  /* af < 0, af > 1, pos < 1 or (pos - 1) / window >= n_pos_bins */
#define QM_AFP_N_GRID 2   /* counted in the grid: the grid's total */
#define QM_AFP_EXTRA 3
#define QM_AFP_MAX_CELLS 8192 /* n_af_bins * n_pos_bins at most */

/* per-VCF scalar slots (int64 each) */
enum {
  QM_S_NPASS = 0,    /* kept lines = R `calleridentify` (caller_performance_compare.R:82) */
  QM_S_TP_LINES = 1, /* data lines of tp.vcf  (fgrep -wf,  extract_TP_FP_SNPs.py:50) */
  QM_S_FP_LINES = 2, /* data lines of fp.vcf  (fgrep -wvf, extract_TP_FP_SNPs.py:52) */
  QM_S_TP_R = 3,     /* |unique(snp) & truth|  (caller_performance_compare.R:94) */
  QM_S_FP_R = 4,     /* |unique(snp) \ truth|  (caller_performance_compare.R:95) */
  QM_S_SORTED = 5,   /* 1 = positions non-decreasing as given, 0 = went through the radix sort */
  QM_S_NREC = 6,     /* records in the VCF */
  QM_S_TRUTH = 7,    /* distinct truth keys T' of the truth set used (FN_R = T' - TP_R) */
  QM_N_SCALARS = 8
};

typedef struct qm_ctx qm_ctx;
typedef struct qm_batch qm_batch;

/* ---- lifecycle ------------------------------------------------------------ */
int qm_abi_version(void);
/* Which sources this library was built from: first 16 hex digits of the sha256 over the device code's sources
 * (qmvt_kernels.hip, qmvt_dev.h: what a kernel profile belongs to) / over every source of the library, taken by the Makefile
 * at build time.  "unknown" for a build that did not go through it (A/B builds).  The host package compares them with the
 * sources in the tree, so that a stale binary is rebuilt -- and can never be quoted with another build's profile. */
const char* qm_kernels_id(void);
const char* qm_build_id(void);
/* One context per process and GPU.  device_id indexes HIP devices (cuda:N in torch). */
int qm_init(int device_id, qm_ctx** out);
void qm_destroy(qm_ctx* ctx);
/* Last error text of this thread (ctx may be NULL for errors raised before a ctx exists). */
const char* qm_last_error(qm_ctx* ctx);

/* ---- truth sets ------------------------------------------------------------
 * Replaces the `awk ... {print $2,".",$4,$5}` pattern list fed to fgrep
 * (extract_TP_FP_SNPs.py:47-48 hcmv, :92-93 custom): the engine keeps the set of
 * single-base (pos,ref,alt) keys, sorted and de-duplicated, in HBM together
 * with a coarse position index.  Host arrays are copied; rows whose ref/alt is
 * not 0..3 are ignored (they can never match a kept line). */
int qm_truth_load(qm_ctx* ctx, const int32_t* pos, const int32_t* ref, const int32_t* alt, int64_t n,
                  int* truth_id);
int qm_truth_size(qm_ctx* ctx, int truth_id, int64_t* n_unique);
/* distinct valid (pos, ref, alt) entries of any allele length: T' of allele-extended batches */
int qm_truth_size_ext(qm_ctx* ctx, int truth_id, int64_t* n_unique);
/* number of truth-set slots of the context (released ones included: ids are stable) */
int qm_truth_count(qm_ctx* ctx);
/* Frees a truth set's device memory.  Its id may be handed out again by a later load; a batch created
 * against the released set refuses to run (QM_E_STATE). */
int qm_truth_release(qm_ctx* ctx, int truth_id);

/* ---- genomes ----------------------------------------------------------------
 * Replaces the BSgenome-style reference lookup of rule mutationcontext (rules/mutationcontext.smk,
 * scripts/mutation_context_profile.R: the mix's Merlin / AD169 FASTA read for SomaticSignatures' mutationContext): one
 * contig's raw bytes (no header, no newlines; POS p is seq[p-1]; ACGTacgt are bases, any other byte is "no base"), packed
 * on the host, kept in HBM.  len > QM_POS_LIMIT: QM_E_RANGE.  Ids follow the rules of truth sets: a released id may be
 * handed out again by a later load, and a qm_batch_motifs that names a released id returns QM_E_STATE. */
int qm_genome_load(qm_ctx* ctx, const uint8_t* seq, int64_t len, int* genome_id);
int qm_genome_release(qm_ctx* ctx, int genome_id);

/* ---- one-shot, host buffers -------------------------------------------------
 * What n_vcf invocations of the reference script compute (A2 flags in, A4/A5
 * split + A6 counts + ROC out).  VCF v owns records rec_offsets[v]..rec_offsets[v+1].
 * Unsorted VCFs are radix-sorted on the GPU transparently.  Blocking.
 *   out_cls      [N]                QM_CLS_* per record, input order        (may be NULL)
 *   out_roc      [n_vcf][3][n_bins] cumulative TP(t), FP(t), U(t); FN(t) = T' - U(t)
 *   out_scalars  [n_vcf][QM_N_SCALARS]
 *   out_idx      [N]  per VCF region: TP line indices ascending from the front,
 *                     FP line indices ascending ending at the back           (may be NULL)
 *   out_global   [n_truth_sets][3][n_bins] sums over the VCFs of each truth set (may be NULL)
 */
int qm_classify_batch(qm_ctx* ctx, int n_vcf, const int64_t* rec_offsets, const int32_t* pos,
                      const int32_t* ref, const int32_t* alt, const float* qual, const uint8_t* flags,
                      const int32_t* truth_id_per_vcf, int n_bins, uint8_t* out_cls, uint64_t* out_roc,
                      int64_t* out_scalars, int32_t* out_idx, uint64_t* out_global);
/* The same with a batch mode (0 or QM_BATCH_ALLELES). */
int qm_classify_batch_ext(qm_ctx* ctx, int n_vcf, const int64_t* rec_offsets, const int32_t* pos,
                          const int32_t* ref, const int32_t* alt, const float* qual, const uint8_t* flags,
                          const int32_t* truth_id_per_vcf, int n_bins, unsigned mode, uint8_t* out_cls,
                          uint64_t* out_roc, int64_t* out_scalars, int32_t* out_idx, uint64_t* out_global);

/* ---- resident batches (columns live in HBM across runs) -------------------- */
int qm_batch_create(qm_ctx* ctx, int n_vcf, const int64_t* n_records, const int32_t* truth_id_per_vcf,
                    int n_bins, qm_batch** out);
int qm_batch_create_ext(qm_ctx* ctx, int n_vcf, const int64_t* n_records, const int32_t* truth_id_per_vcf,
                        int n_bins, unsigned mode, qm_batch** out);
void qm_batch_destroy(qm_batch* b);
int qm_batch_upload(qm_batch* b, int vcf, const int32_t* pos, const int32_t* ref, const int32_t* alt,
                    const float* qual, const uint8_t* flags);

#define QM_SYNTH_TRUTH_PER_VCF 0xffffffffffffffffull
typedef struct qm_synth_cfg {
  int64_t genome_len;   /* L: positions 1..L                                  */
  uint64_t seed;        /* VCF v uses seed + v                                 */
  uint64_t truth_seed;  /* must equal the seed passed to qm_truth_synth, or QM_SYNTH_TRUTH_PER_VCF: every VCF is
                           generated against the synthetic truth set it was assigned at qm_batch_create */
  int64_t truth_n;      /* T of that truth set                                  */
  int32_t shuffled;     /* 0 = position sorted, 1 = records permuted, R >= 2 = R ascending runs one behind the other
                           (a VCF of R contigs: run c holds the generated records c, c + R, c + 2 R, ...; needs R <= records) */
  int32_t indel_pct;    /* 0 = single-base records only (configs 3/4); > 0: that share of the
                           generated records / truth entries carries longer alleles (config 5;
                           allele-extended batches only; must equal qm_truth_synth_ext's) */
} qm_synth_cfg;
/* Synthetic workload of BASELINE.json configs 3/4, generated on the device
 * (DESIGN.md "Synthetic generator").  Every VCF of the batch is filled. */
int qm_truth_synth(qm_ctx* ctx, int64_t genome_len, int64_t truth_n, uint64_t truth_seed, int* truth_id);
int qm_truth_synth_ext(qm_ctx* ctx, int64_t genome_len, int64_t truth_n, uint64_t truth_seed, int indel_pct, int* truth_id);
int qm_batch_synth(qm_batch* b, const qm_synth_cfg* cfg);

/* One self-contained synthetic run for harnesses that are not Python: truth set +
 * batch of n_vcf x records_per_vcf generated on the device, one warm-up, `steps` timed runs of the
 * whole path on the context's stream (wall clock around them; per-kernel times from HIP events). */
typedef struct qm_bench_result {
  int64_t records;               /* per step */
  double seconds_per_step;
  double classifications_per_s;
  float classify_ms, finalize_ms, compact_ms;
  int32_t reserved;
  int64_t kept, tp_lines, fp_lines;   /* sums over the batch (same every step) */
  int64_t device_bytes;
} qm_bench_result;
int qm_bench_synth(qm_ctx* ctx, const qm_synth_cfg* cfg, int n_vcf, int64_t records_per_vcf, int n_bins, int steps,
                   qm_bench_result* out);

/* Enqueue the whole path on `stream` (a hipStream_t; NULL = the context's own
 * stream): classify -> finalize (ROC suffix sums, tile offsets, per-truth sums)
 * -> compaction of TP/FP line indices.  Asynchronous.  If global_dev is not
 * NULL it must be a device buffer of [qm_batch_n_truth(b)][3][n_bins] uint64 that
 * receives the per-truth sums (the caller all-reduces it across ranks).
 *
 * Ordering against the passes over a finished batch (qm_batch_motifs ... qm_batch_haplotypes below), each of which may have been
 * enqueued on a stream of the caller's: a call that rewrites what passes read (qm_batch_run, qm_batch_upload,
 * qm_batch_upload_async, qm_batch_synth, qm_batch_upload_af) is ordered behind every pass of the batch still in flight, on
 * whatever stream.  The asynchronous ones (qm_batch_run, qm_batch_upload_async) make their stream wait for the passes' events;
 * the blocking ones (qm_batch_upload, qm_batch_synth, qm_batch_upload_af) return when those passes are done.  A pass left in
 * flight this way still completes, but its results belong to the run before: its getter answers QM_E_STATE.  A batch that never
 * ran a pass pays nothing for this.  (qm_batch_finish takes the stream of the run it finishes.) */
int qm_batch_run(qm_batch* b, void* stream, void* global_dev);
/* Wait for the stream, then redo VCFs found unsorted through the radix-sort path. */
int qm_batch_finish(qm_batch* b, void* stream);
/* Per-kernel device time, averaged over the (up to 32 latest) qm_batch_run calls made
 * since qm_batch_set_timing(b, 1); HIP events recorded on the run's stream:
 * ms[0]=classify ms[1]=finalize ms[2]=compact ms[3]=whole run. */
int qm_batch_set_timing(qm_batch* b, int on);
int qm_batch_timings(qm_batch* b, float* ms4);

/* qm_batch_upload from page-locked host memory, asynchronous on `stream` (NULL = the context's own). */
int qm_batch_upload_async(qm_batch* b, int vcf, const int32_t* pos, const int32_t* ref, const int32_t* alt,
                          const float* qual, const uint8_t* flags, void* stream);
int qm_batch_get_cls(qm_batch* b, int vcf, uint8_t* out_cls);
/* the class masks as they sit in HBM: bit r of word r / 64 = record r; (n + 63) / 64 words per mask */
int qm_batch_get_masks(qm_batch* b, int vcf, uint64_t* kept, uint64_t* tp);
int qm_batch_get_idx(qm_batch* b, int vcf, int32_t* out_idx);
int qm_batch_get_roc(qm_batch* b, uint64_t* out_roc /*[n_vcf][3][n_bins]*/);
int qm_batch_get_scalars(qm_batch* b, int64_t* out /*[n_vcf][QM_N_SCALARS]*/);
int qm_batch_get_global(qm_batch* b, uint64_t* out /*[qm_batch_n_truth(b)][3][n_bins]*/);
int qm_batch_get_columns(qm_batch* b, int vcf, int32_t* pos, int32_t* ref, int32_t* alt, float* qual,
                         uint8_t* flags);
/* The 96-motif spectra of the kept, TP and FP SNVs of every VCF (rule mutationcontext: mutationContext(unify = TRUE,
 * check = FALSE) + motifMatrix over the filtered / tp / fp VCFs, scripts/mutation_context_profile.R), read from the finished
 * batch's columns and class masks in input order.  genome_id_per_vcf: host array [n_vcf], -1 = no genome (the VCF's rows are
 * zero).  Counted: kept records whose REF and ALT are single bases.  Asynchronous on `stream` (NULL = the context's own);
 * QM_E_STATE unless the latest qm_batch_run was finished.  The output is allocated on the first call. */
int qm_batch_motifs(qm_batch* b, const int32_t* genome_id_per_vcf, void* stream);
/* Waits for the latest qm_batch_motifs, then copies [n_vcf][3][QM_MOTIF_COLS] uint64; QM_E_STATE if the batch ran since. */
int qm_batch_get_motifs(qm_batch* b, uint64_t* out);
/* ---- allele-frequency profiles --------------------------------------------------------------------------
 * The numbers behind `{mix}.{caller}.snp.profile.pdf` of rule mutationcontext (scripts/mutation_context_profile.R:19-46,
 * filterVCF + varPlot: genome position against allele frequency of every TP and FP SNV).
 * qm_batch_upload_af: the allele frequencies of one VCF (qm_vcf_scan_af's column; NaN = none), [n_records of vcf] floats, into
 * an optional device column that is allocated on the first call; blocking.  The VCF is then marked as having frequencies;
 * qm_batch_upload, qm_batch_upload_async and qm_batch_synth of the VCF clear the mark (upload the frequencies after the
 * columns).  A batch that never calls it allocates nothing.
 * qm_batch_af_profile: one streaming pass over the finished batch in input order, asynchronous on `stream` (NULL = the
 * context's own).  Counted: the records qm_batch_motifs counts (kept, single-base REF and ALT), class 0 = TP, 1 = FP.  A counted
 * record goes to QM_AFP_NO_AF (af is NaN), else to QM_AFP_OUTSIDE (af < 0, af > 1, pos < 1, (pos - 1) / window >= n_pos_bins),
 * else to QM_AFP_N_GRID and cell [min(n_af_bins - 1, (int)(af * (float)n_af_bins))][(pos - 1) / window] of the grid.  VCFs
 * without the mark keep zero rows.  1 <= window < 2^28, 1 <= n_af_bins, 1 <= n_pos_bins, n_af_bins * n_pos_bins <=
 * QM_AFP_MAX_CELLS: QM_E_INVAL otherwise.  QM_E_STATE unless the latest qm_batch_run was finished.  May be repeated with
 * other bin counts.
 * qm_batch_get_af_profile: waits for the latest qm_batch_af_profile, then copies its counts (`extra` may be NULL);
 * QM_E_STATE if the batch ran since or no profile was made. */
int qm_batch_upload_af(qm_batch* b, int vcf, const float* af);
int qm_batch_af_profile(qm_batch* b, int32_t window, int32_t n_pos_bins, int32_t n_af_bins, void* stream);
int qm_batch_get_af_profile(qm_batch* b, uint64_t* grid /*[n_vcf][2][n_af_bins][n_pos_bins]*/,
                            uint64_t* extra /*[n_vcf][2][QM_AFP_EXTRA]*/);
/* ---- counts per genome region: BED strata ---------------------------------------------------------------
 * A strata set is 1 .. QM_STRATA_MAX strata; stratum s is the union of the BED intervals start[offsets[s] .. offsets[s + 1]) /
 * end[...] (0-based, half-open: the interval holds the 1-based POS values p with start < p <= end; intervals may overlap or
 * touch, strata may overlap each other).  There is no contig column: only POS decides membership, as everywhere in the engine.
 * qm_strata_load flattens the set into sorted breakpoints b[0] = INT32_MIN < b[1] < ... < b[m - 1] with masks M[i] (bit s =
 * stratum s) valid on [b[i], b[i + 1]), the last segment running to INT32_MAX, equal neighbours merged:
 * mask(p) = M[upper_bound(b, p) - 1] for every int32 p.  QM_E_INVAL: n_strata outside 1 .. QM_STRATA_MAX, start < 0,
 * end <= start (end > 2^31 - 1 cannot be said in int32: the text readers refuse it); QM_E_LIMIT: m > QM_STRATA_MAX_SEGMENTS.
 * Ids are stable; a released slot is reused by a later load; a released id is QM_E_INVAL everywhere.
 * qm_strata_info: info[0] = n_strata, info[1] = m.  qm_strata_segments: the flattened table, m entries each.
 * qm_batch_strata: asynchronous on `stream` (NULL = the context's own); `what` = QM_STRATA_RECORDS, QM_STRATA_TRUTH or both.
 *   Records: one streaming pass over the finished batch in input order.  Counted: every record with its kept bit (the
 *   population of QM_S_NPASS, indels of an allele-extended batch included); TP by the TP mask.  rec[v][S + 2][3] = kept, TP and
 *   FP lines; rows 0 .. S - 1 the strata, row S `outside` (mask 0), row S + 1 `nokey`: a counted record with QM_F_NOKEY goes
 *   there only (its pos is not consulted), every other one to each stratum of mask(pos), or to `outside`.
 *   Truth: tru[v][S + 1][2], rows the strata then `outside`; column 0 = the distinct keys of v's truth set in the row, by the
 *   key's position; column 1 = those with their bit in v's hit bitmap (FN = column 0 - column 1).  Needs a
 *   qm_batch_truth_hits behind the latest run (so: single-base batches only), QM_E_STATE otherwise.
 *   QM_E_STATE unless the latest qm_batch_run was finished.  The outputs are allocated on the first call; may be repeated with
 *   another strata set.
 * qm_batch_get_strata: waits for the latest qm_batch_strata, then copies (either pointer may be NULL); QM_E_STATE if the batch
 * ran since or the half that is asked for was not made. */
#define QM_STRATA_MAX 32
#define QM_STRATA_LDS_SEGMENTS 4096      /* tables up to here are looked up in LDS, larger ones in global memory */
#define QM_STRATA_MAX_SEGMENTS (1 << 22)
#define QM_STRATA_RECORDS 1u
#define QM_STRATA_TRUTH 2u
int qm_strata_load(qm_ctx* ctx, int n_strata, const int64_t* offsets /*[n_strata+1]*/, const int32_t* start, const int32_t* end,
                   int* strata_id);
int qm_strata_info(qm_ctx* ctx, int strata_id, int64_t* info /*[2]: n_strata, n_segments*/);
int qm_strata_segments(qm_ctx* ctx, int strata_id, int32_t* breakpoints, uint32_t* masks);
int qm_strata_release(qm_ctx* ctx, int strata_id);
int qm_batch_strata(qm_batch* b, int strata_id, unsigned what, void* stream);
int qm_batch_get_strata(qm_batch* b, uint64_t* rec /*[n_vcf][S+2][3] or NULL*/, uint64_t* tru /*[n_vcf][S+1][2] or NULL*/);
/* ---- paired block-bootstrap replicates over genome windows ---------------------------------------------
 * Windows: a position p >= 1 with (p - 1) / window < n_win lies in window (p - 1) / window; every other position is `outside`.
 * Counts: cnt[v][n_win + 2][4], rows the windows, then `outside`, then `nokey`; column 0 = kept lines (every record with its
 * kept bit, the population of QM_S_NPASS; a counted record with QM_F_NOKEY goes to `nokey` only, its pos is not consulted),
 * column 1 = TP lines (those with the TP bit), column 2 = the distinct keys of v's truth set by the key's position (`nokey`: 0),
 * column 3 = those with their bit in v's hit bitmap.  The definitions of qm_batch_strata: a one-stratum set covering
 * 1 .. 2^31 - 1 gives the same sums.
 * Draws: replicate b draws n_win window indices, j = 0 .. n_win - 1, all arithmetic mod 2^64:
 *   x = seed + 0x9E3779B97F4A7C15 * (b * n_win + j + 1)
 *   z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 *   idx(b, j) = ((z >> 32) * n_win) >> 32
 * mult[b][w] = #{j : idx(b, j) = w}.  The draws depend on (seed, b, n_win) only: every VCF, batch, rank and device sees the same.
 * Replicates: rep[v][b][c] = sum_w mult[b][w] * cnt[v][w][c] + cnt[v][n_win][c] + cnt[v][n_win + 1][c] (`outside` and `nokey`
 * are not resampled).
 * qm_batch_boot: the kernels are enqueued on `stream` (NULL = the context's own) and not waited for; with QM_BOOT_TRUTH the
 *   call itself blocks for one small host-to-device copy (the per-VCF key and bitmap pointers, 24 bytes per VCF), as
 *   qm_batch_strata does for its rows, and it waits for the previous qm_batch_boot of the batch before it reuses the outputs.
 *   `what` = QM_BOOT_RECORDS, QM_BOOT_TRUTH or both; the
 *   columns of a side that was not asked for are zero.  QM_E_INVAL: window < 1, n_win outside 1 .. QM_BOOT_MAX_WINDOWS, n_rep
 *   outside 0 .. QM_BOOT_MAX_REP (0: counts only), `what` without a side.  QM_E_STATE unless the latest qm_batch_run was
 *   finished; QM_BOOT_TRUTH needs a qm_batch_truth_hits behind that run (so: single-base batches only), QM_E_STATE otherwise.
 *   The outputs are allocated on the first call; may be repeated with other parameters.
 * qm_batch_get_boot: waits for the latest qm_batch_boot, then copies (either pointer may be NULL); QM_E_STATE if the batch ran
 *   since or none was made.
 * qm_boot_draws: host only, the same hash: mult[n_rep][n_win]. */
#define QM_BOOT_MAX_WINDOWS 4096
#define QM_BOOT_MAX_REP 16384
#define QM_BOOT_RECORDS 1u
#define QM_BOOT_TRUTH 2u
int qm_batch_boot(qm_batch* b, int32_t window, int32_t n_win, int32_t n_rep, uint64_t seed, unsigned what, void* stream);
int qm_batch_get_boot(qm_batch* b, uint64_t* cnt /*[n_vcf][n_win+2][4] or NULL*/, uint64_t* rep /*[n_vcf][n_rep][4] or NULL*/);
int qm_boot_draws(uint64_t seed, int32_t n_win, int32_t n_rep, uint16_t* mult /*[n_rep][n_win]*/);
/* ---- the truth-side view ------------------------------------------------------------------------------
 * The sets behind scripts/caller_performance_compare.R:110-119,510-549 (`Genome` against the callers' distinct single-base
 * keys) seen from the truth set: which truth keys a VCF's kept records hit, which records carry a key of the truth set, and,
 * for groups of VCFs of one truth set, how many truth keys lie in every region of their Venn diagram.
 * qm_batch_truth_hits: one pass over the finished batch's columns in input order (sorted and unsorted VCFs alike), asynchronous
 * on `stream` (NULL = the context's own).  QM_E_STATE unless the latest qm_batch_run was finished, when a truth set of the batch
 * was released, and for an allele-extended batch (single-base batches only).  The outputs are allocated on the first call. */
#define QM_TRUTH_GROUP_MAX 5
#define QM_TRUTH_REGIONS 32
int qm_batch_truth_hits(qm_batch* b, void* stream);
/* The hit bitmap of one VCF: n_words = (T' + 31) / 32 words (T' = QM_S_TRUTH of the VCF), bit k & 31 of word k / 32 set iff some
 * record of the VCF is kept, has a comparable key (no QM_F_NOKEY) and that key is entry k of the truth set's sorted distinct keys
 * pos << 4 | ref << 2 | alt.  The ID column plays no part: the popcount is the device's QM_S_TP_R.  Bits at and beyond T' are 0.
 * Waits for the latest qm_batch_truth_hits; QM_E_STATE if the batch ran since (or none was made), QM_E_INVAL for another n_words. */
int qm_batch_get_truth_hits(qm_batch* b, int vcf, uint32_t* bits, int64_t n_words);
/* The record mask of one VCF, laid out like qm_batch_get_masks' ((n + 63) / 64 words): the bit is set iff the record is kept, has
 * a comparable key and the key is in the truth set.  kept & ~mask: the records whose distinct keys QM_S_FP_R counts. */
int qm_batch_get_intruth_mask(qm_batch* b, int vcf, uint64_t* mask);
/* Group g holds the VCFs vcf_ids[group_offsets[g] .. group_offsets[g + 1]): 1 to QM_TRUTH_GROUP_MAX distinct VCFs of this batch
 * that share one truth set (anything else: QM_E_INVAL).  regions[g][m] = the truth keys whose membership mask over the group's
 * VCFs is m (bit i = member i hit it): slot 0 = keys no member hit, slots at and above 1 << n are 0, the slots sum to T'.
 * union_bits (may be NULL): per group, one behind the other, the (T' + 31) / 32 words of the OR of its members' bitmaps.
 * Blocking.  QM_E_STATE without a qm_batch_truth_hits behind the latest run. */
int qm_batch_truth_regions(qm_batch* b, int n_groups, const int32_t* group_offsets, const int32_t* vcf_ids,
                           uint64_t* regions /*[n_groups][QM_TRUTH_REGIONS]*/, uint32_t* union_bits);
/* ---- k-of-n caller consensus --------------------------------------------------------------------------
 * For groups of 1 to QM_VOTE_GROUP_MAX VCFs of one truth set (members in the order given; a VCF sits in at most one group, VCFs
 * outside every group take no part): how many members call every key.  Member i calls key K = pos << 4 | ref << 2 | alt iff one
 * of its records is kept, has a comparable key (no QM_F_NOKEY) and carries K; the ID column plays no part and a key on several
 * lines of one member counts once.  mask(K): bit i set iff member i calls K; votes(K) = its popcount.
 *   tp_votes[g][c], c = 0 .. n: truth keys with exactly c votes (c = 0: missed by all); the row sums to T'.
 *   fp_votes[g][c], c = 1 .. n: distinct keys outside the truth set with exactly c votes; slot 0 is 0.
 *   private_tp[g][i], private_fp[g][i]: the keys with votes = 1 that member i calls.
 *   Slots at and above n + 1 (vote tables) and n (private tables) are 0.
 *   nokey[g]: kept QM_F_NOKEY records of the group's members; they are skipped.
 * qm_batch_votes: asynchronous on `stream` (NULL = the context's own) but for small blocking copies of its tables; it waits for
 *   the previous qm_batch_votes of the batch before it reuses the outputs, which are allocated on the first call.  QM_E_STATE
 *   unless the latest qm_batch_run was finished and a qm_batch_truth_hits lies behind it (so: single-base batches only).
 *   QM_E_INVAL: a group of 0 or more than QM_VOTE_GROUP_MAX members, a VCF in two groups (or twice in one), members of
 *   different truth sets, a VCF id out of range.  May be repeated with other groups.
 * qm_batch_get_votes: waits for the latest qm_batch_votes, then copies (any pointer may be NULL); QM_E_STATE if the batch ran
 *   since or none was made.
 * qm_batch_get_vote_keys: the ascending distinct keys of group `group` outside the truth set and their masks; *n_out = how
 *   many (keys = masks = NULL: the count alone).  QM_E_INVAL if `capacity` is smaller. */
#define QM_VOTE_GROUP_MAX 32
#define QM_VOTE_SLOTS 33
int qm_batch_votes(qm_batch* b, int n_groups, const int32_t* group_offsets, const int32_t* vcf_ids, void* stream);
int qm_batch_get_votes(qm_batch* b, uint64_t* tp_votes /*[n_groups][QM_VOTE_SLOTS]*/, uint64_t* fp_votes /*[n_groups][QM_VOTE_SLOTS]*/,
                       uint64_t* private_tp /*[n_groups][QM_VOTE_GROUP_MAX]*/, uint64_t* private_fp /*[n_groups][QM_VOTE_GROUP_MAX]*/,
                       int64_t* nokey /*[n_groups]*/);
int qm_batch_get_vote_keys(qm_batch* b, int group, uint32_t* keys, uint32_t* masks, int64_t capacity, int64_t* n_out);
/* groups of the latest qm_batch_votes (what sizes qm_batch_get_votes' arrays), or QM_E_STATE as qm_batch_get_votes */
int qm_batch_vote_groups(qm_batch* b);
/* with qm_batch_set_timing on: milliseconds of the latest qm_batch_votes between HIP events on its stream -- [0] k_vote_truth,
 * [1] k_vote_keys + k_vote_segs, [2] the four radix passes, [3] k_vote_heads + k_vote_scan + k_vote_runs.  Waits for the pass. */
int qm_batch_vote_timings(qm_batch* b, float* ms4);
/* ---- near-miss classes: why a line is FP and a truth key FN --------------------------------------------
 * One parameter, `radius`, 0 .. QM_NM_MAX_RADIUS.  A record has a comparable key iff it has neither QM_F_NOKEY nor alleles that
 * are not single bases (key = pos << 4 | ref << 2 | alt), and a usable position iff it has no QM_F_NOKEY.
 * Record side: every FP line of a VCF (kept, no TP line; QM_S_FP_LINES of them) gets the first class that applies --
 *   QM_NM_R_IDCOL    comparable key, and the key is in the truth set: FP by its text alone (the ID column is not `.`)
 *   QM_NM_R_ALLELE   comparable key; the truth set has a key with the same pos and ref base and another alt
 *   QM_NM_R_REFBASE  comparable key; the truth set has keys at the same pos, none with this ref base
 *   QM_NM_R_NEAR     comparable key, no truth key at pos, a truth key with 1 <= |dpos| <= radius
 *   QM_NM_R_ISOLATED comparable key, none of the above
 *   QM_NM_R_NOKEY    no comparable key (pos is not consulted)
 * Truth side: every distinct truth key whose bit in the VCF's hit bitmap is clear gets the first class that applies (records
 * with QM_F_NOKEY are ignored) --
 *   QM_NM_T_FILTERED some record that is not kept carries exactly this comparable key
 *   QM_NM_T_ALLELE   some record, kept or not, with a comparable key has the same pos and ref base and another alt
 *   QM_NM_T_POSITION some record with a usable position sits at the same pos (another ref base, or alleles that are not single bases)
 *   QM_NM_T_NEAR     some record with a usable position has 1 <= |dpos| <= radius
 *   QM_NM_T_UNCALLED none of the above
 * A hit key, and a record that is no FP line, has QM_NM_NONE.
 * qm_batch_nearmiss: asynchronous on `stream` (NULL = the context's own); it waits for the previous qm_batch_nearmiss of the
 *   batch before it reuses the outputs, which are allocated on the first call.  QM_E_INVAL for a radius outside
 *   0 .. QM_NM_MAX_RADIUS; QM_E_STATE unless the latest qm_batch_run was finished and a qm_batch_truth_hits lies behind it
 *   (so: single-base batches only).  May be repeated with another radius.
 * qm_batch_get_nearmiss: waits for the pass, then copies the counts (either pointer may be NULL); rec[v] sums to QM_S_FP_LINES
 *   of VCF v, tru[v] to T' minus the popcount of its hit bitmap.  QM_E_STATE if the batch ran since or no pass was made, as
 *   for the two getters below.
 * qm_batch_get_nearmiss_cls: one class byte per record of the VCF, in input order.
 * qm_batch_get_nearmiss_truth: one class byte per key of the VCF's truth set's sorted distinct keys (T' of them), decoded on the
 *   host from the VCF's four bit planes and its hit bitmap. */
#define QM_NM_MAX_RADIUS 64
#define QM_NM_R_CLASSES 6
#define QM_NM_T_CLASSES 5
#define QM_NM_NONE 255
enum { QM_NM_R_IDCOL = 0, QM_NM_R_ALLELE = 1, QM_NM_R_REFBASE = 2, QM_NM_R_NEAR = 3, QM_NM_R_ISOLATED = 4, QM_NM_R_NOKEY = 5 };
enum { QM_NM_T_FILTERED = 0, QM_NM_T_ALLELE = 1, QM_NM_T_POSITION = 2, QM_NM_T_NEAR = 3, QM_NM_T_UNCALLED = 4 };
int qm_batch_nearmiss(qm_batch* b, int32_t radius, void* stream);
int qm_batch_get_nearmiss(qm_batch* b, uint64_t* rec /*[n_vcf][QM_NM_R_CLASSES] or NULL*/, uint64_t* tru /*[n_vcf][QM_NM_T_CLASSES] or NULL*/);
int qm_batch_get_nearmiss_cls(qm_batch* b, int vcf, uint8_t* out /*[n_records]*/);
int qm_batch_get_nearmiss_truth(qm_batch* b, int vcf, uint8_t* out /*[T']*/);
/* with qm_batch_set_timing on: milliseconds of the latest qm_batch_nearmiss between HIP events on its stream -- [0]
 * k_nearmiss_records, [1] k_nearmiss_truth.  Waits for the pass. */
int qm_batch_nearmiss_timings(qm_batch* b, float* ms2);

/* ---- the filter surface: TP, FP and FN at every QUAL x AF threshold (build-defined, opt-in, single-base batches
 * only) ----
 * Parameters: q_step >= 1 (at most QM_SF_MAX_QUAL_STEP), 1 <= nq <= QM_SF_MAX_QUAL_BINS, 1 <= na <= QM_SF_MAX_AF_BINS,
 * nq * na <= QM_SF_MAX_CELLS.  Per record: snp = both allele codes single bases; j = the index of its key in its VCF's truth
 * set when snp and not QM_F_NOKEY; is_tp = (j found and QM_F_IDDOT) or (snp and QM_F_TPLINE); b = the ROC's quality bin with
 * nq * q_step bins (NaN or floor(qual) < 0: none; clamped to the last), qb = b / q_step; ab = 0 when af is NaN or < 0 (every
 * record of a VCF without qm_batch_upload_af has no af), else min(na - 1, (int)(af * (float)na)) with one float multiply.
 * Counted: the records with snp and a bin, whatever QM_F_PASS says -- into cell [qb][ab] of the TP grid when is_tp, of the FP
 * grid otherwise.  Every truth key is counted once in the U grid, in the lexicographically largest (qb, ab) among its counted
 * records with j found and QM_F_IDDOT (the ROC's best record, with one more tie-break); keys without such a record nowhere.
 * S[v][c][i][k] (c: QM_SF_TP, QM_SF_FP, QM_SF_U) = the sum of grid c over qb >= i and ab >= k: the count under the filter
 * QUAL >= i * q_step and AF >= k / na.  FN = T' - S[U].  extra[v]: QM_SF_COUNTED, QM_SF_NO_AF (counted, af NaN),
 * QM_SF_NO_BIN (snp records left out because they have no bin), QM_SF_TRUTH (T').
 * qm_batch_surface: asynchronous on `stream` (NULL = the context's own); waits for the previous qm_batch_surface of the batch.
 *   QM_E_INVAL for a parameter outside the limits (the message names it); QM_E_STATE unless the latest qm_batch_run was
 *   finished, and for an allele-extended batch.  The first call allocates one u32 per (VCF, truth key) and the grids, counted
 *   in qm_batch_device_bytes; may be repeated with other parameters.
 * qm_batch_get_surface: waits for the pass, then copies (either pointer may be NULL).
 * qm_batch_surface_timings (qm_batch_set_timing on): milliseconds between HIP events -- [0] k_surface_records, [1]
 *   k_surface_truth, [2] k_surface_sums. */
#define QM_SF_MAX_QUAL_BINS 256
#define QM_SF_MAX_AF_BINS 64
#define QM_SF_MAX_CELLS 4096
#define QM_SF_MAX_QUAL_STEP 65536
enum { QM_SF_TP = 0, QM_SF_FP = 1, QM_SF_U = 2 };
enum { QM_SF_COUNTED = 0, QM_SF_NO_AF = 1, QM_SF_NO_BIN = 2, QM_SF_TRUTH = 3 };
#define QM_SF_EXTRA 4
int qm_batch_surface(qm_batch* b, int32_t q_step, int32_t nq, int32_t na, void* stream);
int qm_batch_get_surface(qm_batch* b, uint64_t* S /*[n_vcf][3][nq][na] or NULL*/, uint64_t* extra /*[n_vcf][QM_SF_EXTRA] or NULL*/);
int qm_batch_surface_timings(qm_batch* b, float* ms3);

/* ---- sequence-context profiles: TP, FP and FN per homopolymer x GC cell (build-defined, opt-in) ----
 * G is one contig of qm_genome_load, length L; POS p is G[p], 1 <= p <= L.  Parameters: half window w, 0 .. QM_CX_MAX_HALF_WINDOW,
 * and GC bins ng, 1 .. QM_CX_MAX_GC_BINS.  All integer:
 *   run(i) = 0 when i < 1, i > L or G[i] is no base (not ACGTacgt), else the length of the maximal block of consecutive
 *     positions around i whose base codes equal G[i]'s (case-insensitive);
 *   hp(p) = min(15, max(run(p - 1), run(p), run(p + 1)))  -- a call next to a run is in its context; row 0: no base at or next to p;
 *   nb, gc = the positions of [max(1, p - w), min(L, p + w)] that hold a base, those of them that are C or G;
 *   cell(p) = hp(p) * ng + min(ng - 1, gc * ng / nb) when nb > 0, else NONE.
 * NONE is byte QM_CX_NONE in the table and index 16 ng in every output array; n_cells = 16 ng + 1.
 * qm_genome_context: builds the table of a genome for (w, ng) with the kernel the pass uses, or reuses the one the genome holds
 *   (one per genome, rebuilt when the parameters change, freed by qm_genome_release; the genome owns it, no batch counts it),
 *   and copies out cells[L] (cells[p - 1] = cell(p)) and gen[n_cells] = the positions 1 .. L per cell (sum L); either may be NULL.
 * qm_batch_context: asynchronous on `stream` (NULL = the context's own) but for building a table, which is waited for; `what` =
 *   QM_CX_RECORDS, QM_CX_TRUTH or both; genome_id_per_vcf[v] = the genome of VCF v or -1 (its rows stay zero).
 *   Records: rec[v][n_cells + 1][3] = kept, TP and FP lines of qm_batch_strata's record population; a counted record with
 *   QM_F_NOKEY goes to the last row `nokey` only (its pos is not consulted), every other one to cell(pos), NONE when pos < 1 or
 *   pos > L.  The rows of a VCF with a genome sum to (QM_S_NPASS, QM_S_TP_LINES, QM_S_FP_LINES).
 *   Truth: tru[v][n_cells][2]; column 0 = the distinct keys of v's truth set by cell(key >> 4) in v's genome, column 1 = those
 *   with their bit in v's hit bitmap; the columns sum to QM_S_TRUTH and QM_S_TP_R.  Needs a qm_batch_truth_hits behind the
 *   latest run and a single-base batch (QM_E_STATE otherwise).
 *   QM_E_INVAL for a parameter outside the limits (the message names it); QM_E_STATE unless the latest qm_batch_run was finished,
 *   and for a released genome.  The first call allocates the outputs, counted in qm_batch_device_bytes.
 * qm_batch_get_context: waits for the pass, then copies (any pointer may be NULL); gen_per_vcf[v][n_cells] = the positions per
 *   cell of v's genome.  QM_E_STATE if the batch ran since, or for a side the latest call did not make.
 * qm_batch_context_timings (qm_batch_set_timing on): milliseconds between HIP events -- [0] building tables (0 when every
 *   table was cached), [1] k_context_records, [2] k_context_truth. */
#define QM_CX_MAX_HALF_WINDOW 1024
#define QM_CX_MAX_GC_BINS 15
#define QM_CX_NONE 255
#define QM_CX_RECORDS 1u
#define QM_CX_TRUTH 2u
int qm_genome_context(qm_ctx* ctx, int genome_id, int32_t w, int32_t ng, uint8_t* cells /*[len] or NULL*/, uint64_t* gen /*[16*ng+1] or NULL*/);
int qm_batch_context(qm_batch* b, const int32_t* genome_id_per_vcf, int32_t w, int32_t ng, unsigned what, void* stream);
int qm_batch_get_context(qm_batch* b, uint64_t* rec /*[n_vcf][16*ng+2][3] or NULL*/, uint64_t* tru /*[n_vcf][16*ng+1][2] or NULL*/,
                         uint64_t* gen_per_vcf /*[n_vcf][16*ng+1] or NULL*/);
int qm_batch_context_timings(qm_batch* b, float* ms3);

/* ---- indels and MNPs matched by normal form (build-defined, opt-in, QM_BATCH_ALLELES batches only) ----
 * A variant is (p, R, A), R and A in [ACGT]+; G is one contig of qm_genome_load, G[p] 1-based, ACGTacgt are bases.
 * Normalisable: both alleles have inline codes (1 .. QM_ALLELE_INLINE_MAX bases), no QM_F_NOKEY, R != A, 1 <= p and
 *   p + len(R) - 1 <= L, and G[p .. p + len(R) - 1] spells R.  Otherwise the record keeps its spelling and is counted under the
 *   first reason that applies: LONG (an allele without an inline code), NOKEY, NOVAR (R == A), RANGE, REFMISMATCH, and NOBASE
 *   (the walk below met a position without a base).
 * Normal form: repeat until nothing changes -- (1) if R and A end in the same base, and both have at least 2 bases or p > 1,
 *   drop that base from both; (2) if either allele is now empty, prepend G[p - 1] to both and decrement p --, then, while both
 *   alleles have at least 2 bases and the same first base, drop it from both and increment p.  No cap on the shift.
 * form(v) = the normal form, or the spelling of a variant that has none.  The normalised truth set of (truth set, genome) = the
 *   distinct forms of the truth set's allele-extended entries; VCFs that share a truth set must name one genome (QM_E_INVAL).
 * Per record: hitN = it has valid allele codes, no QM_F_NOKEY, and its form is in the normalised truth set; a TP_N line is kept
 *   and (hitN and QM_F_IDDOT, or QM_F_TPLINE).  The kept set is the batch's.
 * rec[v][QM_NORM_R_COLS], over the kept records: QM_NORM_R_KEPT, _TP (the batch's TP lines), _TP_N, _RESCUED (TP_N and no TP
 *   line), _RESPELLED (the normal form differs from the spelling), _SINGLE (respelled into two single bases), then one column
 *   per reason in the order above.
 * tru[v][QM_NORM_T_COLS]: QM_NORM_T_ENTRIES (allele-extended truth entries), _FORMS (distinct forms), _FOUND (forms of a kept
 *   record with hitN, the ID column ignored), _FORM_ONLY (found forms none of whose entries is spelled like a kept record), _BAD
 *   (entries that are not normalisable).  A VCF whose genome id is -1 keeps zero rows.
 * Class byte per record, kept or not: QM_NORM_C_RESCUED for a rescued line, else QM_NORM_C_UNCHANGED / _RESPELLED or the
 *   reason.  With QM_NORM_COLUMNS the pass also keeps every record's form as int32 codes (the input columns where it has no
 *   normal form) and truth_row = the smallest index, in the order of the truth set's allele-extended table (sorted by
 *   pos << 4 | nibble, ref, alt), of an entry with the record's form, -1 without hitN.
 * qm_batch_normalize: asynchronous on `stream` (NULL = the context's own) but for one small blocking copy; it builds the tables
 *   it needs on that stream at every call.  QM_E_STATE unless the latest qm_batch_run was finished, for a batch without
 *   QM_BATCH_ALLELES, and for a released genome or truth set.  The first call allocates the outputs (qm_batch_device_bytes).
 * qm_batch_get_normalize / qm_batch_get_normalized: wait for the pass, then copy; any pointer may be NULL.  QM_E_STATE if the
 *   batch ran since, for a VCF that named no genome, and for columns the latest call did not keep.
 * qm_batch_normalize_timings (qm_batch_set_timing on): milliseconds between HIP events -- [0] the tables (k_norm_truth,
 *   k_norm_insert, k_norm_fill), [1] k_norm_records, [2] k_norm_found.
 * qm_truth_normalized: the distinct forms of a truth set against a genome, sorted by (pos, ref, alt); *n_out = how many,
 *   QM_E_RANGE (with *n_out set) when capacity is smaller.
 * qm_truth_entries: the allele-extended entries of a truth set in the order of its table (what truth_row indexes), the same way. */
#define QM_NORM_R_COLS 12
#define QM_NORM_T_COLS 5
#define QM_NORM_COLUMNS 2u
enum { QM_NORM_R_KEPT = 0, QM_NORM_R_TP = 1, QM_NORM_R_TP_N = 2, QM_NORM_R_RESCUED = 3, QM_NORM_R_RESPELLED = 4, QM_NORM_R_SINGLE = 5,
       QM_NORM_R_LONG = 6, QM_NORM_R_NOKEY = 7, QM_NORM_R_NOVAR = 8, QM_NORM_R_RANGE = 9, QM_NORM_R_REFMISMATCH = 10, QM_NORM_R_NOBASE = 11 };
enum { QM_NORM_T_ENTRIES = 0, QM_NORM_T_FORMS = 1, QM_NORM_T_FOUND = 2, QM_NORM_T_FORM_ONLY = 3, QM_NORM_T_BAD = 4 };
enum { QM_NORM_C_UNCHANGED = 0, QM_NORM_C_RESPELLED = 1, QM_NORM_C_RESCUED = 2, QM_NORM_C_LONG = 3, QM_NORM_C_NOKEY = 4, QM_NORM_C_NOVAR = 5,
       QM_NORM_C_RANGE = 6, QM_NORM_C_REFMISMATCH = 7, QM_NORM_C_NOBASE = 8 };
int qm_batch_normalize(qm_batch* b, const int32_t* genome_id_per_vcf, unsigned what /*0 or QM_NORM_COLUMNS*/, void* stream);
int qm_batch_get_normalize(qm_batch* b, uint64_t* rec /*[n_vcf][QM_NORM_R_COLS] or NULL*/, uint64_t* tru /*[n_vcf][QM_NORM_T_COLS] or NULL*/);
int qm_batch_get_normalized(qm_batch* b, int vcf, int32_t* pos, int32_t* ref, int32_t* alt, uint8_t* cls, int32_t* truth_row /*[n] each, or NULL*/);
int qm_batch_normalize_timings(qm_batch* b, float* ms3);
int qm_truth_normalized(qm_ctx* ctx, int truth_id, int genome_id, int32_t* pos, int32_t* ref, int32_t* alt, int64_t capacity, int64_t* n_out);
int qm_truth_entries(qm_ctx* ctx, int truth_id, int32_t* pos, int32_t* ref, int32_t* alt, int64_t capacity, int64_t* n_out);

/* ---- MNPs matched against adjacent SNVs (build-defined, opt-in, QM_BATCH_ALLELES batches only) ----
 * A variant is (p, R, A) with allele codes as above.  Atomisable: both alleles have inline codes (1 .. QM_ALLELE_INLINE_MAX
 *   bases), no QM_F_NOKEY, len(R) == len(A), R != A, p >= 0 and p + len(R) - 1 < 2^28.  Otherwise the record keeps its exact-match
 *   verdict and is counted under the first reason that applies: LONG (an allele without an inline code), NOKEY, NOVAR (R == A),
 *   UNEQUAL (indels and complex records of different lengths), RANGE.
 * Atoms of an atomisable variant: for every k with R[k] != A[k] the single-base variant (p + k, R[k], A[k]), 1 to 13 of them,
 *   each one 32-bit word (pos << 4) | (ref << 2) | alt.  An SNV is its own atom.  No genome takes part.
 * Atom set of a truth set: the distinct atoms of its atomisable allele-extended entries (the entries and order of
 *   qm_truth_entries); the entries that are not atomisable stay in the matching by spelling only.
 * Per record: n_atoms; hit_mask, bit k set if the atom at offset k is in the atom set; n_hit its popcount.  hitA = all atoms hit
 *   for an atomisable record, the batch's exact hit for any other.  A TP_A line is kept and (hitA and QM_F_IDDOT, or
 *   QM_F_TPLINE); an exact TP line is always a TP_A line.  rescued = TP_A and no TP line; partial = kept, atomisable and
 *   0 < n_hit < n_atoms.
 * rec[v][QM_ATOM_R_COLS], over the kept records: QM_ATOM_R_KEPT, _TP (the batch's TP lines), _TP_A, _RESCUED, _MULTI (atomisable
 *   with at least 2 atoms), _PARTIAL, _ATOMS / _ATOMS_HIT (sums of n_atoms / n_hit over the atomisable kept records), then one
 *   column per reason in the order above.
 * tru[v][QM_ATOM_T_COLS]: QM_ATOM_T_ENTRIES (allele-extended truth entries), _ATOMISABLE, _ATOMS (distinct atoms), _ATOMS_FOUND
 *   (atoms carried by an atomisable kept record, the ID column ignored), _FOUND (entries spelled like a kept record with valid
 *   codes and no QM_F_NOKEY, the ID ignored), _FOUND_A (atomisable entries whose atoms are all found, plus the entries that are
 *   not atomisable and FOUND).  FOUND <= FOUND_A; without kept QM_F_NOKEY records FOUND == QM_S_TP_R.
 * With QM_ATOM_COLUMNS the pass also keeps per record, kept or not: a class byte (QM_ATOM_C_RESCUED for a rescued line, else
 *   _FULL / _PARTIAL / _NONE by n_hit for an atomisable record, else the reason), n_atoms as uint8 (0 where the record is not
 *   atomisable) and hit_mask as uint16.
 * qm_batch_atomize: asynchronous on `stream` (NULL = the context's own) but for one small blocking copy; it builds the sets on
 *   that stream at every call (the first call that meets a truth set counts its atoms once, and waits for that number).
 *   QM_E_STATE unless the latest qm_batch_run was finished, for a batch without QM_BATCH_ALLELES, and for a released truth set.
 *   The first call allocates the outputs (qm_batch_device_bytes).
 * qm_batch_get_atomize / qm_batch_get_atomized: wait for the pass, then copy; any pointer may be NULL.  QM_E_STATE if the batch
 *   ran since, and for columns the latest call did not keep.
 * qm_batch_atomize_timings (qm_batch_set_timing on): milliseconds between HIP events -- [0] the sets (k_atom_truth),
 *   [1] k_atom_records, [2] k_atom_found.
 * qm_truth_atoms: the atom set of a truth set, sorted ascending; *n_out = how many, QM_E_RANGE (with *n_out set) when capacity
 *   is smaller. */
#define QM_ATOM_R_COLS 13
#define QM_ATOM_T_COLS 6
#define QM_ATOM_COLUMNS 2u
enum { QM_ATOM_R_KEPT = 0, QM_ATOM_R_TP = 1, QM_ATOM_R_TP_A = 2, QM_ATOM_R_RESCUED = 3, QM_ATOM_R_MULTI = 4, QM_ATOM_R_PARTIAL = 5,
       QM_ATOM_R_ATOMS = 6, QM_ATOM_R_ATOMS_HIT = 7, QM_ATOM_R_LONG = 8, QM_ATOM_R_NOKEY = 9, QM_ATOM_R_NOVAR = 10, QM_ATOM_R_UNEQUAL = 11,
       QM_ATOM_R_RANGE = 12 };
enum { QM_ATOM_T_ENTRIES = 0, QM_ATOM_T_ATOMISABLE = 1, QM_ATOM_T_ATOMS = 2, QM_ATOM_T_ATOMS_FOUND = 3, QM_ATOM_T_FOUND = 4, QM_ATOM_T_FOUND_A = 5 };
enum { QM_ATOM_C_FULL = 0, QM_ATOM_C_PARTIAL = 1, QM_ATOM_C_NONE = 2, QM_ATOM_C_RESCUED = 3, QM_ATOM_C_LONG = 4, QM_ATOM_C_NOKEY = 5,
       QM_ATOM_C_NOVAR = 6, QM_ATOM_C_UNEQUAL = 7, QM_ATOM_C_RANGE = 8 };
int qm_batch_atomize(qm_batch* b, unsigned what /*0 or QM_ATOM_COLUMNS*/, void* stream);
int qm_batch_get_atomize(qm_batch* b, uint64_t* rec /*[n_vcf][QM_ATOM_R_COLS] or NULL*/, uint64_t* tru /*[n_vcf][QM_ATOM_T_COLS] or NULL*/);
int qm_batch_get_atomized(qm_batch* b, int vcf, uint8_t* cls, uint8_t* n_atoms, uint16_t* hit_mask /*[n] each, or NULL*/);
int qm_batch_atomize_timings(qm_batch* b, float* ms3);
int qm_truth_atoms(qm_ctx* ctx, int truth_id, uint32_t* keys, int64_t capacity, int64_t* n_out);

/* ---- TP, FP and FN by variant type and size (build-defined, opt-in, QM_BATCH_ALLELES batches only) ----
 * Type and size of a variant (R, A), R != A, m = min(|R|, |A|): cp = the longest common prefix, at most m; cs = the longest common
 *   suffix of what is left, at most m - cp (the prefix goes first); tr = |R| - cp - cs, ta = |A| - cp - cs.  tr == 0: QM_TYPE_INS
 *   of size ta; ta == 0: QM_TYPE_DEL of size tr; tr == ta == 1: QM_TYPE_SNV of size 1; tr == ta >= 2: QM_TYPE_MNP of size tr (the
 *   trimmed span); otherwise QM_TYPE_CPX of size max(tr, ta).  No genome takes part.
 * Long alleles (dictionary ids) are typed through a shape table with one row per id (qm_dict_shapes): len >= 14, head = the
 *   first QM_ALLELE_INLINE_MAX bases, tail = the last ones, 2 bits per base, base k at bits 2 k.  A pair with ONE long allele is
 *   decided exactly by it (the other allele has at most 13 bases, so neither trim looks further).
 * Rows: sizes are binned by n_bins (1 .. QM_TYPE_MAX_BINS) ascending lower edges, edges[0] == 1; bin b holds edges[b] <= size <
 *   edges[b + 1], the last bin is open.  A typed variant lies in row type * n_bins + bin; four rows follow the grid, the first
 *   that applies wins: 5 n_bins + QM_TYPE_X_NOKEY (QM_F_NOKEY or an invalid code), _NOVAR (equal codes), _LONGPAIR (both alleles
 *   long: counted, not guessed), _NOSHAPE (a long allele without a row in the table, or no table).  n_rows = 5 n_bins + 4.
 * rec[v][n_rows][2]: the kept records of the row, and those of them that are TP lines by the batch's own masks.
 * tru[v][n_rows][2]: the allele-extended entries of the VCF's truth set in the row (the entries of qm_truth_entries; never in
 *   NOKEY), and those of them spelled like a kept record with valid codes and no QM_F_NOKEY (QM_ATOM_T_FOUND by another route).
 * With QM_TYPE_COLUMNS the pass also keeps the row of every record, kept or not, as one byte.
 * qm_batch_types: asynchronous on `stream` (NULL = the context's own) but for the small blocking copies of the table and the
 *   descriptors; the shape arrays are read during the call only (NULL / n_shapes = 0: no table).  QM_E_INVAL for edges that do
 *   not ascend from 1, n_bins outside 1 .. QM_TYPE_MAX_BINS and a shape row with len < 14; QM_E_STATE unless the latest
 *   qm_batch_run was finished, for a batch without QM_BATCH_ALLELES, and for a released truth set.  The first call allocates the
 *   outputs (qm_batch_device_bytes).
 * qm_batch_get_types / qm_batch_get_typed: wait for the pass, then copy ([n_vcf][n_rows][2] with the n_rows of the latest call;
 *   either pointer may be NULL).  QM_E_STATE if the batch ran since, and for row bytes the latest call did not keep
 *   (QM_TYPE_COLUMNS).
 * qm_batch_types_timings (qm_batch_set_timing on): milliseconds between HIP events -- [0] k_type_records, [1] k_type_truth. */
#define QM_TYPE_MAX_BINS 16
#define QM_TYPE_MAX_ROWS 84
#define QM_TYPE_COLUMNS 2u
enum { QM_TYPE_SNV = 0, QM_TYPE_MNP = 1, QM_TYPE_INS = 2, QM_TYPE_DEL = 3, QM_TYPE_CPX = 4 };
enum { QM_TYPE_X_NOKEY = 0, QM_TYPE_X_NOVAR = 1, QM_TYPE_X_LONGPAIR = 2, QM_TYPE_X_NOSHAPE = 3 };
int qm_batch_types(qm_batch* b, const int32_t* edges, int n_bins, const int32_t* len, const uint32_t* head, const uint32_t* tail,
                   int64_t n_shapes, unsigned what /*0 or QM_TYPE_COLUMNS*/, void* stream);
int qm_batch_get_types(qm_batch* b, uint64_t* rec /*[n_vcf][n_rows][2] or NULL*/, uint64_t* tru /*[n_vcf][n_rows][2] or NULL*/);
int qm_batch_get_typed(qm_batch* b, int vcf, uint8_t* row /*[n]*/);
int qm_batch_types_timings(qm_batch* b, float* ms2);

/* ---- clusters of records matched by replayed haplotype (build-defined, opt-in, QM_BATCH_ALLELES batches only) ----
 * The bounded core of rtg vcfeval / hap.py xcmp: the unmatched records of a small region and the unmatched truth entries of the
 * same region are each replayed onto the genome; both sides are rescued when the two sequences are equal.  All or nothing per
 * region.  The classification, its masks and its counts stay untouched.
 * G: one contig of qm_genome_load, 1-based, length L, read as qm_batch_normalize reads it (lower case counts as its base); every
 *   byte that is no base is one symbol of its own (code 15), equal to itself only.
 * Usable: a variant (p, R, A) with inline codes for both alleles, no QM_F_NOKEY, R != A, 1 <= p and p + |R| - 1 <= L, and G
 *   spelling R.  Otherwise it is counted under the first reason that applies: LONG, NOKEY, NOVAR, RANGE, REFMISMATCH.
 * Trimmed form (q, r, a) of a usable variant, with cp and cs of qm_batch_types (prefix first and greedy, then suffix): q = p + cp,
 *   r = R[cp : |R| - cs], a = A[cp : |A| - cs]; one of r, a may be empty.  Footprint: lo = q, hi = max(q, q + |r| - 1).
 * Sites of a (truth set, genome, gap g), 0 <= g <= QM_HAP_MAX_GAP: the usable allele-extended entries in the table's order; the
 *   next entry joins the current site iff its lo <= (the largest hi so far) + 2 g, else it opens a new site.  A site's window is
 *   [max(1, min lo - g), min(L + 1, max hi + g)]; a site whose window is longer than QM_HAP_MAX_WINDOW is TOOLONG for every VCF.
 *   Window ends never descend.  A footprint [lo, hi] lies in the first site whose window ends at or behind hi, if that window
 *   starts at or before lo (windows of different sites are disjoint, but where a common prefix moved an entry's footprint behind
 *   the next entry's: then the first such site is the one).
 * Per VCF: an entry is FOUND when a kept record with valid codes and no QM_F_NOKEY spells it (qm_batch_types' found), and open
 *   when it is usable and not FOUND.  A record is MATCHED_SPELLING when it has valid codes, no QM_F_NOKEY and spells an entry;
 *   it is open when it is kept, usable, not MATCHED_SPELLING and its footprint lies in a site's window; a kept, usable, unmatched
 *   record in no window is OUTSIDE.  Open records of a TOOLONG site are TOOLONG; an open record of a site without an open entry
 *   is LONE.
 * A site with an open record and an open entry that is not TOOLONG is tried: TOOMANY when either side has more than
 *   QM_HAP_MAX_ITEMS open lines or entries; otherwise identical spellings of a side collapse, the variants of a side are sorted by
 *   (q, |r|), and the site is CONFLICT when for two neighbours of a side q_next < q_prev + |r_prev|, or q_next == q_prev and
 *   |r_next| == 0.  The replay of a side over the window [ws, we]: cur = ws; per variant G[cur .. q - 1], then a, cur = q + |r|;
 *   at the end G[cur .. min(we, L)].  MATCH iff the two replays are equal in length and in every symbol, else MISMATCH.
 * In a MATCH site every open record is rescued (class RESCUED) and every open entry is found by haplotype.  hitH = hit by
 *   spelling, or rescued; a TP_H line is kept and (hitH and QM_F_IDDOT, or QM_F_TPLINE): qm_batch_normalize's rule with hitN
 *   replaced by hitH; an exact TP line is always a TP_H line.
 * rec[v][QM_HAP_R_COLS] over the kept records: KEPT, TP (the batch's own), TP_H, RESCUED (TP_H lines that are no TP lines), OPEN
 *   (all open records, whatever became of them), then the records per class OUTSIDE .. REFMISMATCH.
 * tru[v][QM_HAP_T_COLS]: ENTRIES, FOUND, FOUND_H (FOUND plus found by haplotype), OPEN, UNUSABLE, SITES, TRIED, MATCHED (sites).
 * With QM_HAP_COLUMNS the pass also hands out a class byte per record, kept or not (QM_HAP_C_*; NOTKEPT: usable, unmatched and
 *   not kept), the site of every usable record (-1: none), and per VCF a class byte per truth entry (MATCHED_SPELLING: found;
 *   RESCUED: found by haplotype; LONE: open, its site was not tried; the site's class; or the reason it is not usable).
 * Out of scope: a subset search inside a site (one true FP beside a respelled pair leaves the site MISMATCH), alleles of more
 *   than QM_ALLELE_INLINE_MAX bases, phasing and genotypes, FP_R and the ROC after rescue, genomes of several contigs, vareval,
 *   single-base batches (QM_E_STATE).
 * qm_batch_haplotypes: genome_id_per_vcf[v] = a genome id or -1 (the VCF's rows stay zero); asynchronous on `stream` (NULL = the
 *   context's own) but for the blocking copy of the descriptors and ONE 8-byte readback, the number of (VCF, open site) pairs,
 *   which sizes their lists.  The site tables are rebuilt on the stream at every call.  QM_E_INVAL for a gap outside 0 ..
 *   QM_HAP_MAX_GAP and when VCFs that share a truth set name different genomes; QM_E_RANGE for a batch of more than 65535 VCFs
 *   (one grid dimension holds them) and for more than (2^31 - 1) / 11 (VCF, open site) pairs (the lists are indexed in 32 bits); QM_E_STATE unless the latest qm_batch_run was
 *   finished, for a batch without QM_BATCH_ALLELES, and for a released truth set or genome.
 *   A search behind the previous call (qm_batch_hapsubsets, maybe on another stream) is waited for on the HOST first, not on the
 *   stream: this call regrows and refills from the host, with a blocking copy of the per-VCF descriptors, what that search still
 *   reads.  A haplotype call behind a search in flight therefore holds the calling thread until the search is done.
 * qm_batch_get_haplotypes / qm_batch_get_haplotyped: wait for the pass, then copy (any pointer may be NULL).  QM_E_STATE if the
 *   batch ran since, for a VCF that named no genome, and without QM_HAP_COLUMNS in the latest call.
 * qm_batch_haplotype_timings (qm_batch_set_timing on): milliseconds between HIP events -- [0] the site tables, [1]
 *   k_hap_records, [2] k_hap_truth, k_hap_rank and the readback, [3] k_hap_pairs and k_hap_claim, [4] k_hap_replay.
 * qm_truth_sites: the sites of a truth set, in order: the first entry (index into qm_truth_entries) and the window of each. */
#define QM_HAP_R_COLS 16
#define QM_HAP_T_COLS 8
#define QM_HAP_MAX_GAP 32
#define QM_HAP_DEFAULT_GAP 10
#define QM_HAP_MAX_WINDOW 256
#define QM_HAP_MAX_ITEMS 8
#define QM_HAP_COLUMNS 2u
enum { QM_HAP_R_KEPT = 0, QM_HAP_R_TP = 1, QM_HAP_R_TP_H = 2, QM_HAP_R_RESCUED = 3, QM_HAP_R_OPEN = 4, QM_HAP_R_OUTSIDE = 5, QM_HAP_R_LONE = 6,
       QM_HAP_R_MISMATCH = 7, QM_HAP_R_CONFLICT = 8, QM_HAP_R_TOOMANY = 9, QM_HAP_R_TOOLONG = 10, QM_HAP_R_LONG = 11, QM_HAP_R_NOKEY = 12,
       QM_HAP_R_NOVAR = 13, QM_HAP_R_RANGE = 14, QM_HAP_R_REFMISMATCH = 15 };
enum { QM_HAP_T_ENTRIES = 0, QM_HAP_T_FOUND = 1, QM_HAP_T_FOUND_H = 2, QM_HAP_T_OPEN = 3, QM_HAP_T_UNUSABLE = 4, QM_HAP_T_SITES = 5,
       QM_HAP_T_TRIED = 6, QM_HAP_T_MATCHED = 7 };
enum { QM_HAP_C_MATCHED_SPELLING = 0, QM_HAP_C_RESCUED = 1, QM_HAP_C_OUTSIDE = 2, QM_HAP_C_LONE = 3, QM_HAP_C_MISMATCH = 4,
       QM_HAP_C_CONFLICT = 5, QM_HAP_C_TOOMANY = 6, QM_HAP_C_TOOLONG = 7, QM_HAP_C_LONG = 8, QM_HAP_C_NOKEY = 9, QM_HAP_C_NOVAR = 10,
       QM_HAP_C_RANGE = 11, QM_HAP_C_REFMISMATCH = 12, QM_HAP_C_NOTKEPT = 13 };
int qm_batch_haplotypes(qm_batch* b, const int32_t* genome_id_per_vcf, int gap, unsigned what /*0 or QM_HAP_COLUMNS*/, void* stream);
int qm_batch_get_haplotypes(qm_batch* b, uint64_t* rec /*[n_vcf][QM_HAP_R_COLS] or NULL*/, uint64_t* tru /*[n_vcf][QM_HAP_T_COLS] or NULL*/);
int qm_batch_get_haplotyped(qm_batch* b, int vcf, uint8_t* cls /*[n]*/, int32_t* site /*[n]*/, uint8_t* entry_cls /*[entries]*/);
int qm_batch_haplotype_timings(qm_batch* b, float* ms5);

/* ---- a subset search inside the mismatched sites of the haplotype pass (build-defined, opt-in) ----
 * Behind a qm_batch_haplotypes, with its gap and genomes.  A site is SEARCHED for a VCF when the pass tried it and its outcome is
 * MISMATCH or CONFLICT; every other site and class stays as it is.
 * Forms: each side is reduced to its distinct trimmed forms (q, r, a) -- spellings that trim to one form collapse, a chosen form
 *   rescues every line that spells it --, ordered by (q, |r|, |a|, a as a string over A<C<G<T); bit k of a side's mask is its
 *   k-th form.  A subset is admissible when no two of its forms conflict: for a before b, q_b < q_a + |r_a|, or q_b = q_a and
 *   |r_b| = 0.
 * The optimum: over all pairs (S, T) of non-empty admissible subsets of the line forms and of the entry forms whose replays over
 *   the site's window are equal (in length and in every symbol; a byte that is no base is a symbol of its own), the largest
 *   |S| + |T|, then the larger |T|, then the smallest S mask, then the smallest T mask.  A searched site with an optimum is
 *   PARTIAL, one without is NOSUBSET.  Hashes only order the work: every answer is verified symbol by symbol.
 * In a PARTIAL site the open lines whose form is in S are rescued by subset, the open entries whose form is in T are found by
 *   subset; the others are left.  hitS = hit by spelling, rescue by haplotype or rescue by subset; a TP_S line is kept and
 *   satisfies (hitS and QM_F_IDDOT, or QM_F_TPLINE).
 * sub[v][QM_HAPSUB_COLS]: SEARCHED, PARTIAL, NOSUBSET (sites), TP_S (TP_H plus the lines the subset rescue gains), RESCUED_S
 *   (lines rescued by subset, whatever their ID), FOUND_S (FOUND_H plus the entries found by subset), LEFT_LINES, LEFT_ENTRIES
 *   (over PARTIAL sites).
 * With QM_HAPSUB_COLUMNS (needs QM_HAP_COLUMNS in the haplotype call) the search hands out second class bytes per record and per
 *   truth entry: the pass's own but inside PARTIAL sites, where they are QM_HAP_C_SUBSET or QM_HAP_C_LEFT.  The arrays, rec and
 *   tru of the pass itself are never touched.  QM_HAPSUB_NARROW_HASH is a self-check: hashes of 4 bits, so that nearly every
 *   candidate collides and the answer rests on the verification alone; its results equal the normal mode's bit for bit.
 * qm_batch_hapsubsets: asynchronous on `stream` (NULL = the context's own), ordered behind the haplotype call on whatever stream;
 *   QM_E_INVAL for any other bit of `what`; QM_E_STATE without a qm_batch_haplotypes behind the latest run, if a truth set or a
 *   genome of that call was released, and for QM_HAPSUB_COLUMNS without QM_HAP_COLUMNS.  A new qm_batch_haplotypes waits for a
 *   search still in flight and forgets its results.
 * qm_batch_get_hapsubsets / qm_batch_get_hapsubsetted: wait for the search, then copy (any pointer may be NULL).  The second one
 *   returns the two class arrays (QM_E_STATE without QM_HAPSUB_COLUMNS) and, per PARTIAL site of the VCF, sites ascending, the
 *   site index and the two masks; *n_out = their number, QM_E_RANGE if it is more than `capacity`.
 * qm_batch_hapsubset_timings (qm_batch_set_timing on): milliseconds of the latest search between HIP events. */
#define QM_HAPSUB_COLS 8
#define QM_HAPSUB_COLUMNS 2u
#define QM_HAPSUB_NARROW_HASH 4u
enum { QM_HAPSUB_SEARCHED = 0, QM_HAPSUB_PARTIAL = 1, QM_HAPSUB_NOSUBSET = 2, QM_HAPSUB_TP_S = 3, QM_HAPSUB_RESCUED_S = 4,
       QM_HAPSUB_FOUND_S = 5, QM_HAPSUB_LEFT_LINES = 6, QM_HAPSUB_LEFT_ENTRIES = 7 };
enum { QM_HAP_C_SUBSET = 14, QM_HAP_C_LEFT = 15 };
int qm_batch_hapsubsets(qm_batch* b, unsigned what /*0, QM_HAPSUB_COLUMNS, QM_HAPSUB_NARROW_HASH or both*/, void* stream);
int qm_batch_get_hapsubsets(qm_batch* b, uint64_t* sub /*[n_vcf][QM_HAPSUB_COLS]*/);
int qm_batch_get_hapsubsetted(qm_batch* b, int vcf, uint8_t* cls_s /*[n]*/, uint8_t* entry_cls_s /*[entries]*/, int32_t* site_s /*[capacity]*/,
                              uint8_t* smask /*[capacity]*/, uint8_t* tmask /*[capacity]*/, int64_t capacity, int64_t* n_out);
int qm_batch_hapsubset_timings(qm_batch* b, float* ms1);
/* The QUAL ROC under normal-form and atom matching: the 256-threshold sweep of qm_batch_get_roc, with the hit of
 * qm_batch_normalize (hitN) or of qm_batch_atomize (hitA) in place of the hit by spelling.  It reads what those passes left in
 * the batch and normalises or atomises nothing again.  Build-defined, parity unpinned, as both passes are.
 * Universe, as in qm_batch_get_roc of an allele-extended batch: records with two valid allele codes and a QUAL bin b >= 0
 *   (floor(QUAL) clamped to n_bins - 1; NaN and QUAL < 0 have none), kept or not.
 * By normal form: tpN = (hitN and QM_F_IDDOT) or QM_F_TPLINE; TP_N_hist[b]++ if tpN, else FP_N_hist[b]++.  The truth-side unit
 *   is the form; its best is the highest b over the records with hitN and QM_F_IDDOT whose form it is; U_N_hist[b] = forms whose
 *   best is b.  Baseline: QM_NORM_T_FORMS.  A VCF that named no genome in qm_batch_normalize has zero rows and a zero baseline.
 * By atoms: hitA = all atoms in the atom set for an atomisable record, the hit by spelling (valid codes, no QM_F_NOKEY, the
 *   spelling in the truth set's allele-extended table) for any other; tpA and the two histograms as above.  The truth-side unit
 *   is the allele-extended entry.  Carriers are the records of the universe with QM_F_IDDOT and without QM_F_NOKEY: an
 *   atomisable carrier raises the best of every atom of its hit mask (a partial record's too), any other carrier the best of the
 *   entry it is spelled like.  The best of an atomisable entry is the minimum over its atoms (none if an atom has none), that of
 *   any other entry its own.  Baseline: QM_ATOM_T_ENTRIES.
 * roc_n / roc_a [v][3][n_bins]: the suffix sums TP(t), FP(t), U(t) in the layout of qm_batch_get_roc; base[v][2]: the two
 *   baselines (0 for a matching not swept); FN_X(t) = base_X - U_X(t).
 * qm_batch_rescue_roc: asynchronous on `stream` (NULL = the context's own), ordered behind both producers on whatever stream.
 *   QM_E_INVAL for which = 0 or any other bit; QM_E_STATE for a single-base batch, if a truth set was released, and if the batch
 *   has not finished qm_batch_normalize(.., QM_NORM_COLUMNS) (QM_RROC_NORM) or qm_batch_atomize(QM_ATOM_COLUMNS) (QM_RROC_ATOM)
 *   since its latest run.  A new call of a producer waits for a sweep still in flight and forgets that matching's rows.
 * qm_batch_get_rescue_roc: waits for the sweep, then copies (any pointer may be NULL; QM_E_STATE for the rows of a matching the
 *   latest sweep did not make).
 * qm_batch_rescue_roc_timings (qm_batch_set_timing on): milliseconds between HIP events of k_rroc_records and k_rroc_units by
 *   normal form, then by atoms (0 for a matching not swept). */
#define QM_RROC_NORM 1u
#define QM_RROC_ATOM 2u
int qm_batch_rescue_roc(qm_batch* b, unsigned which /*QM_RROC_NORM | QM_RROC_ATOM*/, void* stream);
int qm_batch_get_rescue_roc(qm_batch* b, uint64_t* roc_n /*[n_vcf][3][n_bins]*/, uint64_t* roc_a /*[n_vcf][3][n_bins]*/, uint64_t* base /*[n_vcf][2]*/);
int qm_batch_rescue_roc_timings(qm_batch* b, float* ms4);
/* The four rescues combined: final TP, FP and FN when everything the engine knows is applied, and the Venn of
 * methods.  It reads what qm_batch_normalize, qm_batch_atomize, qm_batch_haplotypes and -- with QM_LADDER_SUBSETS --
 * qm_batch_hapsubsets left in the batch and normalises, atomises and replays nothing again.  Build-defined, parity unpinned, as
 * the four passes are.
 * Per record one mask byte, 0 for a record that is not kept, else: QM_LADDER_M_K always; QM_LADDER_M_S if the record is one of
 *   the batch's TP lines; QM_LADDER_M_N if its class byte of the normalisation pass is QM_NORM_C_RESCUED; QM_LADDER_M_A if that of
 *   the atomisation pass is QM_ATOM_C_RESCUED; QM_LADDER_M_H if that of the haplotype pass is QM_HAP_C_RESCUED and it has
 *   QM_F_IDDOT and is no TP line; QM_LADDER_M_B if the search's second class byte is QM_HAP_C_SUBSET and it has QM_F_IDDOT and is
 *   no TP line (always 0 without QM_LADDER_SUBSETS).  N, A, H and B are never set with S, H and B never together.  A VCF that named
 *   no genome (-1) in the normalisation call has N zero throughout, one that named none in the haplotype call H and B.
 * Per truth entry of a VCF (allele-extended table order) one mask byte: S if the entry is spelled like a kept record with valid
 *   codes and no QM_F_NOKEY (QM_ATOM_T_FOUND); N if its form was found by a kept record; A if it is atomisable and every one of
 *   its atoms is carried by a kept atomisable record; H if its entry class is QM_HAP_C_RESCUED; B if its second entry class is
 *   QM_HAP_C_SUBSET (0 without QM_LADDER_SUBSETS).  The bits are raw: S usually implies N.
 * rec[v][QM_LADDER_COLS]: QM_LADDER_KEPT, QM_LADDER_TP, then 16 cells: cell m (column QM_LADDER_CELL0 + m) = the kept lines that
 *   are no TP lines and whose low four bits are m; cell 0 is the final FP.  tru[v][QM_LADDER_COLS]: the entries, those with S, then
 *   16 cells over the entries without S; cell 0 is the final FN.
 * qm_batch_ladder: asynchronous on `stream` (NULL = the context's own), ordered behind its producers on whatever stream.
 *   QM_E_INVAL for any other bit in `what`; QM_E_STATE for a single-base batch, if a truth set was released, and if the batch has
 *   not finished, since its latest run, qm_batch_normalize(.., QM_NORM_COLUMNS), qm_batch_atomize(QM_ATOM_COLUMNS),
 *   qm_batch_haplotypes(.., QM_HAP_COLUMNS) or -- for QM_LADDER_SUBSETS -- qm_batch_hapsubsets(QM_HAPSUB_COLUMNS): the first one
 *   missing, in that order, is named.  A new call of a producer waits for a ladder still in flight and forgets its rows.
 * qm_batch_get_ladder: waits for the pass, then copies (either pointer may be NULL).
 * qm_batch_get_laddered: the mask bytes of one VCF (either pointer may be NULL); QM_E_STATE without QM_LADDER_COLUMNS in the
 *   latest call.
 * qm_batch_ladder_timings (qm_batch_set_timing on): milliseconds between HIP events of k_ladder_records and k_ladder_truth. */
#define QM_LADDER_SUBSETS 1u
#define QM_LADDER_COLUMNS 2u
#define QM_LADDER_COLS 18
enum { QM_LADDER_KEPT = 0, QM_LADDER_TP = 1, QM_LADDER_CELL0 = 2 };      /* truth side: the entries, those with S, the cells */
enum { QM_LADDER_M_N = 1, QM_LADDER_M_A = 2, QM_LADDER_M_H = 4, QM_LADDER_M_B = 8, QM_LADDER_M_K = 64, QM_LADDER_M_S = 128 };
int qm_batch_ladder(qm_batch* b, unsigned what /*0, QM_LADDER_SUBSETS, QM_LADDER_COLUMNS or both*/, void* stream);
int qm_batch_get_ladder(qm_batch* b, uint64_t* rec /*[n_vcf][QM_LADDER_COLS]*/, uint64_t* tru /*[n_vcf][QM_LADDER_COLS]*/);
int qm_batch_get_laddered(qm_batch* b, int vcf, uint8_t* mask /*[n]*/, uint8_t* entry_mask /*[entries]*/);
int qm_batch_ladder_timings(qm_batch* b, float* ms2);
/* The match ladder per variant type and size: the rows of the latest qm_batch_types crossed with the 18
 * columns of the latest qm_batch_ladder.  It reads the row byte per record that qm_batch_types(.., QM_TYPE_COLUMNS) left and
 * the mask byte per record and per (VCF, truth entry) that qm_batch_ladder(.., QM_LADDER_COLUMNS) left; nothing is normalised,
 * atomised, replayed or typed by new rules.  Build-defined, parity unpinned, as its two producers are.
 * Rows: those of the latest qm_batch_types call, n_rows = 5 n_bins + 4 (at most QM_TYPE_MAX_ROWS), with its edges, its shape
 *   table and its four off-grid rows.  A record's row is its row byte: records are typed AS SPELLED, so a respelled deletion
 *   counts in the row of its spelling, whatever normal form rescued it.  A truth entry's row is the row of its (ref, alt) codes
 *   without QM_F_NOKEY, as in tru of qm_batch_get_types: truth entries never land in QM_TYPE_X_NOKEY.
 * Columns: the ladder's (QM_LADDER_KEPT, QM_LADDER_TP, QM_LADDER_CELL0 + m).
 * rec[v][row][QM_LADDER_COLS], over the records of VCF v with that row byte whose mask byte is not 0 (the kept ones): all of
 *   them; those with QM_LADDER_M_S; cell m = those without S whose low four bits are m (cell 0: the row's final FP).
 * tru[v][row][QM_LADDER_COLS], over the entries of v's truth set in that row: all of them; those with S; the 16 cells over
 *   the entries without S (cell 0: the row's final FN).  A VCF without a genome in the normalisation or the haplotype call takes
 *   part with the bits it has.
 * Summed over the rows, both are rec and tru of qm_batch_get_ladder; columns 0 and 1 of every row are the row's pair of
 *   qm_batch_get_types (its "found" and the ladder's S are one rule); in every row the 16 cells sum to column 0 - column 1.
 *   The tier order and the cumulative TP, FP and FN after every tier stay a convention of the host (quasimodo_amd.ladder).
 * qm_batch_ladder_types: asynchronous on `stream` (NULL = the context's own), ordered behind its producers on whatever stream.
 *   QM_E_STATE for a single-base batch, if a truth set was released, and if the batch has not finished, since its latest run,
 *   qm_batch_types(.., QM_TYPE_COLUMNS) or qm_batch_ladder(.., QM_LADDER_COLUMNS): the first one missing, in that order, is
 *   named.  A new call of either, or of any of the ladder's four producers, waits for this pass still in flight and forgets its
 *   rows.
 * qm_batch_get_ladder_types: waits for the pass, then copies (any pointer may be NULL); n_rows_out: the rows of a VCF's block.
 * qm_batch_ladder_types_timings (qm_batch_set_timing on): milliseconds between HIP events of k_ltype_records and k_ltype_truth. */
int qm_batch_ladder_types(qm_batch* b, void* stream);
int qm_batch_get_ladder_types(qm_batch* b, uint64_t* rec /*[n_vcf][n_rows][QM_LADDER_COLS]*/, uint64_t* tru /*[n_vcf][n_rows][QM_LADDER_COLS]*/,
                              int* n_rows_out);
int qm_batch_ladder_types_timings(qm_batch* b, float* ms2);
int qm_truth_sites(qm_ctx* ctx, int truth_id, int genome_id, int gap, int32_t* first_entry, int32_t* lo, int32_t* hi, int64_t capacity,
                   int64_t* n_out);
/* Where the VCFs that the last qm_batch_finish found out of order went (a sorted batch reports zeros).  The bucket path
 * has capacity limits (a bucket's records, the truth keys of its positions, the VCF's size); a VCF beyond them is redone by
 * the radix sort -- correct, several times slower -- and these counters say how often that happened. */
enum {
  QM_PATH_UNSORTED = 0,              /* VCFs found out of order */
  QM_PATH_DIRECT = 1,                /* ... joined bucket by bucket with two bits per position in LDS (k_join_lean) */
  QM_PATH_HASHED = 2,                /* ... joined bucket by bucket through hashed tables (k_classify_hash: wide key ranges) */
  QM_PATH_RADIX = 3,                 /* ... radix-sorted because the bucket path does not take them (size, allele-extended batch) */
  QM_PATH_RADIX_AFTER_OVERFLOW = 4,  /* ... radix-sorted after a bucket of their chunk overflowed */
  QM_PATH_BUCKET_CHUNKS = 5, QM_PATH_OVERFLOW_CHUNKS = 6, QM_PATH_RADIX_CHUNKS = 7,
  QM_PATH_DIRECT2 = 8,               /* ... too large for 256 buckets: dealt to partitions of 2^27 keys by a first scatter (two levels), then as QM_PATH_DIRECT */
  QM_PATH_PARTITIONS = 9,            /* ... too large or too wide for 256 buckets: every partition (256 buckets of 2^15 positions, or of 2^17: up to 32 768 records each) a segment of ONE scatter that reads the columns */
  QM_N_PATH_STATS = 10
};
int qm_batch_path_stats(qm_batch* b, int64_t* out /*[QM_N_PATH_STATS]*/);
/* The same counters summed over every qm_batch_finish of every batch of the context since qm_init, the batches that
 * qm_extract_files / qm_classify_batch make for themselves included: callers take the difference around a call. */
int qm_path_stats_total(qm_ctx* ctx, int64_t* out /*[QM_N_PATH_STATS]*/);
/* Device address of the per-truth sums of the last run ([qm_batch_n_truth(b)][3][n_bins] uint64; the caller's global_dev when
 * qm_batch_run was given one): valid until the batch runs again or is destroyed.  For callers that hand the counters to a
 * collective without a trip through the host. */
int qm_batch_global_device(qm_batch* b, void** dev);
/* ---- the path's one exchange: the all-reduce of the confusion counters (SURVEY.md 8b's all-reduced `out_global`, 8e) ----
 * Replaces nothing in the reference (its per-VCF processes never add anything up: R does, from files); it is what makes the
 * sums of a batch sharded over GPUs one number.  RCCL directly -- ncclCommInitAll / ncclCommInitRank, ONE
 * ncclAllReduce(ncclUint64, ncclSum) in place on the batch's per-truth sums ([qm_batch_n_truth][3][n_bins] uint64: the buffer
 * qm_batch_global_device names) -- so that a host that is not Python has the collective too (the Python host may keep
 * torch.distributed on the same buffer).  librccl is opened when a communicator is first asked for (QM_RCCL_LIB names another
 * file); a build or a box without it fails there with QM_E_COMM and nowhere else.  Unmeasured beyond one device (no multi-GPU
 * box was available to any round; two ranks on one card are refused by RCCL).
 *
 * qm_comm_create: one process, n contexts on n DISTINCT devices (one host thread per context: examples/qm_multi.c).
 * qm_comm_create_rank: one process per GPU; rank 0 makes the id with qm_comm_make_id and hands its 128 bytes to the others
 *   (a file, the environment, MPI: the caller's).
 * qm_allreduce_counters: every member calls it once per step, behind qm_batch_finish; the all-reduce is enqueued on `stream`
 *   (NULL = the context's own) behind the batch's run, and the call returns when THIS member's copy of the sums is complete
 *   (qm_batch_get_global / qm_batch_global_device then hold the sums over all members).  Batches of all members must have the same
 *   n_truth and n_bins.  From one process, call it from one thread per member (a member blocks until all have arrived).
 * qm_comm_collectives: collectives this communicator has issued for `ctx`'s member (tests: exactly one per step). */
typedef struct qm_comm qm_comm;
typedef struct qm_comm_id { char bytes[128]; } qm_comm_id;
int qm_comm_create(qm_ctx* const* ctxs, int n, qm_comm** out);
int qm_comm_make_id(qm_comm_id* out);
int qm_comm_create_rank(qm_ctx* ctx, int rank, int n_ranks, const qm_comm_id* id, qm_comm** out);
int qm_allreduce_counters(qm_batch* b, qm_comm* comm, void* stream);
int64_t qm_comm_collectives(const qm_comm* comm, const qm_ctx* ctx);
void qm_comm_destroy(qm_comm* comm);

/* Bytes the engine holds in HBM for this batch. */
int64_t qm_batch_device_bytes(qm_batch* b);
/* Rows of the per-truth sums ([n][3][n_bins]; qm_batch_get_global, qm_batch_run's global_dev): the number of
 * truth-set slots the context had when the batch was created.  Truth sets loaded later do not change it. */
int qm_batch_n_truth(qm_batch* b);

/* What this GPU streams with 16-byte accesses per lane over `bytes` of HBM (>= 1 MiB; use a size far beyond the 256 MiB
 * Infinity Cache), `reps` passes each: gbps[0] = read only, gbps[1] = copy (bytes read + bytes written per second),
 * gbps[2] = write only.  The measured denominators bench.py quotes beside the data sheet's 8 TB/s. */
int qm_bw_probe(qm_ctx* ctx, int64_t bytes, int reps, double* gbps /*[3]*/);

/* ---- FP overlap (rules/compare_FP.smk + scripts/snpcaller_fp_compare.R:36-47) -
 * n_sets (<= 5) key lists (fp.vcf rows as packed columns); regions[m] = number
 * of distinct keys whose membership mask is m.  regions has 1 << n_sets slots. */
int qm_fp_overlap(qm_ctx* ctx, int n_sets, const int64_t* set_offsets, const int32_t* pos,
                  const int32_t* ref, const int32_t* alt, int64_t* regions);

/* ---- host text side (no GPU): tokenizer / packer / writers ------------------
 * Replaces the three awk passes + `grep -E "^#"` per VCF
 * (extract_TP_FP_SNPs.py:24-32,50,52) with one scan.  qm_vcf_scan fills, for
 * every line of the text (header lines included), its byte offset; for data
 * lines the packed columns.  Returns QM_OK or a negative code.  line_kind: */
#define QM_LINE_DATA 0          /* data line, described completely by its columns */
#define QM_LINE_HEADER 1        /* begins with '#' */
#define QM_LINE_DATA_HOST 2     /* single-base data line whose fgrep answer the columns cannot give (POS not a
                                   canonical decimal, or a "\t.\t" that a pattern could sit on after the ALT column):
                                   qm_vcf_hostpath decides it and writes the decision into its flags */
#define QM_LINE_HEADER_KEPT 3   /* '#' line that also satisfies the A2 filter: awk does not skip it, so the reference
                                   emits it in the header block AND among the kept lines (and then in tp or fp) */
#define QM_LINE_HEADER_KEPT_TP 4 /* the same once qm_vcf_hostpath found it selected by fgrep -wf */
#define QM_LINE_REFUSED 5       /* kept data line holding a NUL or an INVALID UTF-8 sequence: grep answers "binary file matches" under the
                                   locale Python exports to it (PEP 538); strict callers stop with QM_E_NONCANON.  Valid UTF-8 is text: such
                                   a single-base line is QM_LINE_DATA_HOST (word characters by iswalnum on C.UTF-8, as grep -w asks) */
#define QM_LINE_HEADER_REFUSED 6 /* the same for a '#' line that satisfies the A2 filter */
typedef struct qm_vcf_cols {
  int64_t n_lines;      /* all lines */
  int64_t n_data;       /* data lines = records */
  int64_t n_host;       /* lines for qm_vcf_hostpath (kinds 2 and 3) */
  int64_t n_refused;    /* kinds 5 and 6 */
  int64_t first_refused_line; /* 1-based, 0 = none */
  int64_t n_nokey_kept; /* kept data lines without a comparable key (QM_F_NOKEY): qm_vcf_hostpath counts their keys as text */
  /* (ABI 4) kept data lines that hold '#', ' or ": the reference's counting step reads <x>.filtered.vcf with R's read.table
   * (scripts/caller_performance_compare.R:29-39, custom_snp_benchmark.R:45-48: comment.char = "#", quote = "\"'"), which cuts a
   * line at a '#', lets a quote swallow tabs and newlines up to the next one, and turns a file it then cannot parse into an
   * EMPTY one (tryCatch -> NA row).  The three output files are unaffected (they are the shell pipeline's bytes); the R-path
   * counts (QM_S_TP_R / FP_R / NPASS) assume lines split at their tabs alone.  Strict table writers refuse such a file. */
  int64_t n_r_hostile;
  int64_t first_r_hostile_line; /* 1-based, 0 = none */
} qm_vcf_cols;
typedef struct qm_dict qm_dict;
int64_t qm_vcf_count_lines(const uint8_t* text, size_t len);
int qm_vcf_scan(const uint8_t* text, size_t len, int64_t cap_lines, int64_t* line_off /*cap+1*/,
                uint8_t* line_kind, int32_t* pos, int32_t* ref, int32_t* alt, float* qual, uint8_t* flags,
                qm_vcf_cols* info);
/* Truth text -> key columns.  mode 0 = VCF as written by mummer2vcf.py
 * (columns 2,4,5), mode 1 = 12-column show-snps TSV (columns 1,2,3).
 * out_counts[0] = rows R counts as `genomediff`, [1] = keys emitted (rows that are not comments, with a
 * canonical position and single-base alleles: the only patterns a line can match through its columns),
 * [2] = rows whose pattern can match no such line (they live in qm_patterns only), [3] = rows refused
 * (always 0 since round 6: a canonical pattern is ASCII, the row's other columns never reach it), [4] = '#' rows that awk turns into a pattern all the same. */
int64_t qm_truth_scan(const uint8_t* text, size_t len, int mode, int64_t cap, int32_t* pos, int32_t* ref,
                      int32_t* alt, int64_t* out_counts /*[5]*/);
/* Allele-extended tokenising (QM_BATCH_ALLELES): the filter's `^[ACGT]$` becomes `^[ACGT]+$`, ref / alt
 * carry allele codes, alleles longer than QM_ALLELE_INLINE_MAX bases are interned in `dict`, which the
 * truth set and every VCF of a batch must share.  dict == NULL is qm_vcf_scan / qm_truth_scan.
 * qm_truth_scan_ext takes mode 0 (VCF) only.  qm_dict is thread safe. */
qm_dict* qm_dict_create(void);
void qm_dict_destroy(qm_dict* d);
int64_t qm_dict_size(qm_dict* d);
/* code of an allele string; QM_ALLELE_NONE unless it is [ACGT]+ (and, beyond 13 bases, d != NULL) */
int32_t qm_allele_code(qm_dict* d, const uint8_t* s, size_t n);
/* spelling of a code into out[cap]; returns its length, -1 if the code is no allele / does not fit */
int64_t qm_allele_spell(qm_dict* d, int32_t code, uint8_t* out, size_t cap);
/* The shape rows of ids first .. first + cap - 1 (as far as the dictionary holds them) for qm_batch_types: the allele's length,
 * its first QM_ALLELE_INLINE_MAX bases and its last ones, 2 bits per base, base k at bits 2 k.  Returns the rows written. */
int64_t qm_dict_shapes(qm_dict* d, int64_t first, int64_t cap, int32_t* len, uint32_t* head, uint32_t* tail);
int qm_vcf_scan_ext(const uint8_t* text, size_t len, int64_t cap_lines, int64_t* line_off, uint8_t* line_kind,
                    int32_t* pos, int32_t* ref, int32_t* alt, float* qual, uint8_t* flags, qm_vcf_cols* info,
                    qm_dict* dict);
int64_t qm_truth_scan_ext(const uint8_t* text, size_t len, int mode, int64_t cap, int32_t* pos, int32_t* ref,
                          int32_t* alt, int64_t* out_counts /*[5]*/, qm_dict* dict);

/* The allele frequency of every data line as rule mutationcontext reads it (scripts/mutation_context_profile.R:26:
 * `as.numeric(gsub(".*AF=([01]\\.[0-9]+);.*$", "\\1", INFO, perl=T))`), from a text that qm_vcf_scan / qm_vcf_scan_ext has
 * scanned: one float per data line (kinds QM_LINE_DATA, QM_LINE_DATA_HOST, QM_LINE_REFUSED), in record order.  INFO is the
 * 8th tab-separated field (up to the next tab or the line's end; a '\r' in front of the newline belongs to it).  The value
 * comes from the LAST place in the field where `AF=` is followed by 0 or 1, '.', one or more digits and ';' (the pattern's
 * leading `.*` is greedy: `MAF=0.2;` counts, `AF=0.5` at the field's end without ';' does not); its text is converted as a
 * correctly rounded double and then rounded to float.  No such place, or fewer than 8 fields: quiet NaN.  (R hands an INFO
 * field without a match to as.numeric whole, so a field that is itself a number becomes a frequency there; here it is NaN:
 * DESIGN.md 4.9.)  info[0] = data lines with a value, info[1] = data lines with fewer than 8 fields.  The inputs are not
 * modified. */
int qm_vcf_scan_af(const uint8_t* text, size_t len, int64_t n_lines, const int64_t* line_off,
                   const uint8_t* line_kind, float* af /*[n_data]*/, int64_t* info /*[2]*/);

/* ---- host path for what the columns cannot describe -----------
 * qm_patterns is the pattern list the reference feeds to `fgrep -wf` (extract_TP_FP_SNPs.py:47-53, :92-98), kept as
 * TEXT: one pattern X \t . \t Y \t Z per truth row that satisfies the awk program, '#' rows included.  mode as
 * qm_truth_scan; ext != 0 widens `^[ACGT]$` to `^[ACGT]+$` (allele-extended mode, mode 0 only).
 * info[0] = distinct patterns, [1] = patterns whose Y / Z are not one character each, [2] = canonical keys that only
 * '#' rows carry (fgrep sees them, R does not), [3] = rows refused (a NUL or an invalid UTF-8 sequence inside the pattern's fields).  When [1] or [2] is non-zero the
 * columns alone cannot reproduce the reference for ANY line compared with this truth set: qm_vcf_hostpath then
 * decides every single-base data line from the text. */
typedef struct qm_patterns qm_patterns;
qm_patterns* qm_patterns_create(const uint8_t* truth_text, size_t len, int mode, int ext);
void qm_patterns_destroy(qm_patterns* p);
int qm_patterns_info(const qm_patterns* p, int64_t* info /*[4]*/);
/* Exact `fgrep -w` (GNU grep 3.7: a pattern occurrence with a non-word character or the line edge on both sides) for
 * the lines of one scanned VCF that need it: kind QM_LINE_DATA_HOST lines get QM_F_TPLINE set or QM_F_IDDOT cleared
 * in `flags` (indexed by data line), QM_LINE_HEADER_KEPT lines become QM_LINE_HEADER_KEPT_TP when selected.  Run it
 * between qm_vcf_scan and the upload of the columns; the device then counts and lists these lines like any other.
 * R's unique-key counts (caller_performance_compare.R:84-99) take the key of a line as TEXT; for kept lines without
 * a comparable key the device counts distinct (carried pos, ref, alt) instead, so out[2..4] carry the exchange:
 * out[0] = lines decided here, [1] = of them selected, [2] = what the device will add to FP_R for the QM_F_NOKEY
 * lines, [3] = their distinct text keys found in the truth file as R reads it (add to TP_R), [4] = the other
 * distinct text keys (add to FP_R after subtracting [2]).  pos / ref / alt: the scan's columns. */
int qm_vcf_hostpath(const qm_patterns* p, const uint8_t* text, size_t len, int64_t n_lines, const int64_t* line_off,
                    uint8_t* line_kind, const int32_t* pos, const int32_t* ref, const int32_t* alt, uint8_t* flags,
                    int64_t* out /*[5]*/);

/* Writes header lines + selected data lines, verbatim, newline-terminated
 * (SURVEY Q7).  select: 0 = kept (filtered.vcf), 1 = TP, 2 = FP.  QM_LINE_HEADER_KEPT(_TP) lines appear in the
 * header block and again, in input order, among the selected lines.  Atomic (temp file + rename). */
int qm_vcf_write(const char* path, const uint8_t* text, size_t len, int64_t n_lines, const int64_t* line_off,
                 const uint8_t* line_kind, const uint8_t* cls /*per data line*/, int select);
/* SNP / indel splitters of rules/vis_eval_vcf.smk:35,50,66,81 (`extract_snp`, `extract_indel`,
 * `extract_nucmer_snp`, `extract_nucmer_indel`): every '#' line, plus every line whose REF/ALT
 * satisfy the rule's awk pattern, in input order ('#' lines that also satisfy it appear twice,
 * as awk prints them).  mode 0 = xsnp, 1 = xindel.  flavour 0 reads `{2,}` as a POSIX interval
 * (gawk), flavour 1 as literal text (mawk 1.3.4 20200120).  Atomic (temp file + rename). */
int qm_vcf_split_write(const char* path, const uint8_t* text, size_t len, int mode, int flavour, int64_t* n_written);
/* ---- files in, files out: the reference's per-VCF worker for MANY VCFs in one call ------------------------------
 * What n_jobs invocations of `python program/extract_TP_FP_SNPs.py <vcf> <truth> {hcmv,custom} <outdir> <caller>`
 * (extract_TP_FP_SNPs.py:124-140; rules/extract_TP.smk:20, eval_variant_custom.smk:73) do: inputs are mapped,
 * tokenised by host threads straight into page-locked buffers and uploaded while the next file is tokenised, the
 * host path decides what the columns cannot describe, ONE engine batch classifies every mixed-sample VCF, the class
 * masks come back (2 bits per record) and the three files of every VCF are gathered from the mapped input with
 * writev.  Output paths are the caller's (the reference derives them, :19-22,39-41 / :71-72,91); their directories
 * must exist.  pure != 0: pure-strain sample (:33-36): fp is a copy of filtered, no tp file, the truth is never read.
 * strict != 0: QM_E_NONCANON for kept lines / truth rows holding a NUL or an invalid UTF-8 sequence (their reference answer depends
 * on the locale); 0: such lines are classified by their columns.  mode: 0 or QM_BATCH_ALLELES.
 * stats[j] / roc[j][3][n_bins] (either may be NULL): the per-VCF rows; phase_seconds[8] (may be NULL): map + count,
 * truth sets (on a thread beside the former), batch layout, tokenise + host path + uploads, engine, masks back, write,
 * release. */
typedef struct qm_file_job {
  const char* vcf_path;
  const char* truth_path;   /* may be NULL when pure */
  int32_t mode;             /* 0: truth VCF (hcmv), 1: show-snps table (custom) */
  int32_t pure;
  const char* filtered_out;
  const char* tp_out;       /* may be NULL when pure */
  const char* fp_out;
} qm_file_job;
typedef struct qm_file_stats {
  int64_t scalars[QM_N_SCALARS];   /* QM_S_*; TP_R / FP_R with the text keys of QM_F_NOKEY lines exchanged in */
  int64_t n_lines, n_refused, genomediff;
  int64_t header_kept, header_kept_tp;   /* '#' lines that pass the A2 filter (awk emits them among the kept lines too) */
  int64_t host_decided;                  /* lines decided by the host path */
  int64_t r_hostile;                     /* (ABI 4) qm_vcf_cols.n_r_hostile: kept lines R's read.table would not read as tab-split text */
} qm_file_stats;
int qm_extract_files(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                     qm_file_stats* stats, uint64_t* roc, double* phase_seconds);
/* The same for one rank of a multi-GPU run (rules/extract_TP.smk:17-20 runs one process per VCF; here one process per GPU
 * takes a share of them): global_dev, a DEVICE buffer of [n_slots][3][n_bins] uint64, receives the per-truth-file sums of this
 * call's VCFs -- cleared first; VCF j adds to row truth_slot[j] (the caller's layout: every rank uses the same row for the
 * same truth file; pure-strain jobs are ignored; jobs that name the same truth file must name the same row) -- ready for the
 * one all-reduce of the confusion counters (RCCL).  n_jobs == 0 is allowed: the buffer is cleared, nothing else happens.
 * truth_slot / global_dev NULL: qm_extract_files. */
int qm_extract_files_ex(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                        qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                        void* global_dev);
/* qm_extract_files_ex plus rule mutationcontext over its outputs (rules/mutationcontext.smk): genome_id[j] (a
 * qm_genome_load id, -1 = none) and motifs[j][3][QM_MOTIF_COLS] (qm_batch_motifs' rows; zero for jobs without a genome).
 * Mixed-sample jobs: the motif pass runs behind the classification.  Pure-strain jobs that name a genome join the batch
 * against an empty truth set: kept = the filter's verdict, TP = none, FP = kept (extract_TP_FP_SNPs.py:33-36); their files,
 * stats and ROC rows are those of qm_extract_files_ex. */
int qm_extract_files_motifs(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                            qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                            void* global_dev, const int32_t* genome_id, uint64_t* motifs);

/* qm_extract_files_ex plus the truth-side view over its batch (single-base mode only: QM_E_STATE otherwise).
 * fn_out[j] (or NULL): a missed-variant list for job j -- the header ('#') lines of its truth file, then, in file order, every
 * data row whose key the reference would have put into `Genome` (make_snp_vector, scripts/caller_performance_compare.R:29-55:
 * single-base REF and ALT; custom mode: custom_snp_benchmark.R:23-27) and that is not among the VCF's kept single-base keys; a
 * key on several rows is written on each.  Pure-strain jobs write none (the reference never reads their truth).
 * group[j]: -1 or a group id < n_groups; a group holds 1 to QM_TRUTH_GROUP_MAX mixed-sample jobs of one truth file, its members
 * in job order (anything else: QM_E_INVAL).  regions[g][m]: qm_batch_truth_regions' slots.  fp_regions[g][m] (may be NULL):
 * qm_fp_overlap's slots over the members' kept keys that are NOT in the truth set (the regions without the `Genome` bit).
 * missed_out[g] (array or entries may be NULL): the list of the rows no member hit.
 * R compares keys as text.  A VCF that asks for a list or sits in a group and holds a kept line without a comparable key
 * (QM_F_NOKEY) is refused with QM_E_NONCANON and a message that names the line: its text key has no place in the bitmaps. */
typedef struct qm_truthside_args {
  const char* const* fn_out;      /* [n_jobs] */
  const int32_t* group;           /* [n_jobs] */
  int32_t n_groups;
  int32_t reserved;
  uint64_t* regions;              /* [n_groups][QM_TRUTH_REGIONS] */
  int64_t* fp_regions;            /* [n_groups][QM_TRUTH_REGIONS] or NULL */
  const char* const* missed_out;  /* [n_groups] or NULL */
} qm_truthside_args;
int qm_extract_files_truthside(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                               qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                               void* global_dev, const qm_truthside_args* ts);

/* qm_extract_files_ex plus the k-of-n consensus over its batch (single-base mode only: QM_E_STATE otherwise).
 * group[j]: -1 or a group id < n_groups; a group holds 1 to QM_VOTE_GROUP_MAX mixed-sample jobs of one truth file, its members in
 * job order (anything else: QM_E_INVAL).  Behind the batch's finish the call runs qm_batch_truth_hits and qm_batch_votes; the four
 * tables are qm_batch_get_votes' rows.  consensus_k[g] (array may be NULL; 0 = no file; above the group's size: QM_E_INVAL) with
 * consensus_out[g]: the group's consensus VCF at that level -- the '#' lines of the first member's filtered file, then one line
 * per key that at least k members call, in ascending key order (pos << 4 | ref << 2 | alt; keys inside and outside the truth set
 * interleaved): the first kept line carrying the key in the lowest-numbered member that calls it, byte for byte.  Atomic (temp
 * file + rename).  A group member that holds a kept line without a comparable key (QM_F_NOKEY) is refused with QM_E_NONCANON and
 * a message that names the file and the line, as qm_extract_files_truthside does.  The VCF outputs, stats and roc are those of
 * qm_extract_files_ex. */
typedef struct qm_votes_args {
  const int32_t* group;             /* [n_jobs] */
  int32_t n_groups;
  int32_t reserved;
  uint64_t* tp_votes;               /* [n_groups][QM_VOTE_SLOTS] */
  uint64_t* fp_votes;               /* [n_groups][QM_VOTE_SLOTS] */
  uint64_t* private_tp;             /* [n_groups][QM_VOTE_GROUP_MAX] */
  uint64_t* private_fp;             /* [n_groups][QM_VOTE_GROUP_MAX] */
  const int32_t* consensus_k;       /* [n_groups] or NULL */
  const char* const* consensus_out; /* [n_groups] or NULL */
} qm_votes_args;
int qm_extract_files_votes(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                           qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                           void* global_dev, const qm_votes_args* votes);

/* qm_extract_files_ex plus the near-miss classes over its batch (single-base mode only: QM_E_STATE otherwise).
 * Jobs with want[j] != 0 take part (pure-strain jobs never do); one radius per call (outside 0 .. QM_NM_MAX_RADIUS: QM_E_INVAL).
 * Behind the batch's finish the call runs qm_batch_truth_hits and qm_batch_nearmiss; rec / tru: qm_batch_get_nearmiss' rows per
 * job (zero for jobs that take no part).
 * fp_why_out[j] (array or entries may be NULL): "#line\tPOS\tREF\tALT\tQUAL\tclass\n", then one row per FP line of the VCF in
 * file order -- the 1-based line number in the input file, the line's own text of the four columns, the class name (idcol,
 * allele, refbase, near, isolated, nokey).
 * fn_why_out[j] (array or entries may be NULL): "#POS\tREF\tALT\tclass\n", then exactly the rows fn_out of
 * qm_extract_files_truthside would hold for the job, in the same order, as their POS / REF / ALT text and the class name of
 * their key (filtered, allele, position, near, uncalled); `.` for a row the device cannot hold.
 * Both files are written atomically (temp file + rename).  A job that asks for fn_why_out and holds a kept line without a
 * comparable key (QM_F_NOKEY) is refused with QM_E_NONCANON and a message that names the file and the line, as
 * qm_extract_files_truthside does and for its reason; fp_why_out alone is not refused, such lines are class nokey.
 * The VCF outputs, stats and roc are those of qm_extract_files_ex. */
typedef struct qm_nearmiss_args {
  const uint8_t* want;              /* [n_jobs] 0/1 */
  int32_t radius;
  int32_t reserved;
  uint64_t* rec;                    /* [n_jobs][QM_NM_R_CLASSES] */
  uint64_t* tru;                    /* [n_jobs][QM_NM_T_CLASSES] */
  const char* const* fp_why_out;    /* [n_jobs] or NULL */
  const char* const* fn_why_out;    /* [n_jobs] or NULL */
} qm_nearmiss_args;
int qm_extract_files_nearmiss(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                              qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                              void* global_dev, const qm_nearmiss_args* nearmiss);

/* qm_extract_files_ex plus the filter surface over its batch (single-base mode only: QM_E_STATE otherwise).
 * Jobs with want[j] != 0 have their INFO column scanned (qm_vcf_scan_af) and uploaded beside the other columns, as in
 * qm_extract_files_profile, and get their rows: S[j][3][nq][na] and extra[j][QM_SF_EXTRA] of qm_batch_get_surface; the others
 * get zero rows.  A pure-strain job that asks is refused by name (QM_E_INVAL): it has no truth set.  One parameter triple per
 * call, checked as qm_batch_surface checks it.  The VCF outputs, stats and roc are those of qm_extract_files_ex. */
typedef struct qm_surface_args {
  const uint8_t* want;              /* [n_jobs] 0/1 */
  int32_t q_step, nq, na, reserved;
  uint64_t* S;                      /* [n_jobs][3][nq][na] */
  uint64_t* extra;                  /* [n_jobs][QM_SF_EXTRA] */
} qm_surface_args;
int qm_extract_files_surface(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                             qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                             void* global_dev, const qm_surface_args* surface);

/* qm_extract_files_motifs plus the allele-frequency profile: both halves of rule mutationcontext in one call.
 * genome_id / motifs may be NULL (no spectra).  Jobs with want[j] != 0 have their INFO column scanned (qm_vcf_scan_af) and
 * uploaded beside the other columns; the profile pass runs behind the classification (and behind the motif pass).  Wanted
 * pure-strain jobs join the batch against an empty truth set, as those that name a genome do: everything kept is FP.
 * grid / extra: qm_batch_af_profile's rows per job (zero for jobs that are not wanted).  points_out[j] (array or entries may be
 * NULL): the data frame R plots, "Position\tFrequency\ttype\n", then every counted record, the FP ones first, then the TP
 * ones, each in file order (rbind(fp_snp, tp_snp)): the line's POS text, the text the pattern captured or NA, FP / TP.
 * Atomic (temp file + rename).  The VCF outputs, stats and roc are those of qm_extract_files_ex. */
typedef struct qm_profile_args {
  const uint8_t* want;            /* [n_jobs] 0/1 */
  int32_t window, n_pos_bins, n_af_bins, reserved;
  uint64_t* grid;                 /* [n_jobs][2][n_af_bins][n_pos_bins] */
  uint64_t* extra;                /* [n_jobs][2][QM_AFP_EXTRA] */
  const char* const* points_out;  /* [n_jobs] or entries NULL */
} qm_profile_args;
int qm_extract_files_profile(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                             qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                             void* global_dev, const int32_t* genome_id, uint64_t* motifs, const qm_profile_args* profile);

/* qm_extract_files_ex plus the counts per stratum over its batch.  Jobs with want[j] != 0 get their rows:
 * rec[j][S + 2][3] and tru[j][S + 1][2] of qm_batch_get_strata, S the size of strata set `strata_id`; the others get zero rows.
 * Single-base mode: truth hits and both halves run behind the batch's finish; QM_BATCH_ALLELES: the record side only (tru stays
 * zero).  Wanted pure-strain jobs join the batch against an empty truth set, as in qm_extract_files_motifs: everything kept is
 * FP, their tru rows are zero.  The VCF outputs, stats and roc are those of qm_extract_files_ex. */
typedef struct qm_strata_args {
  int32_t strata_id;
  int32_t reserved;
  const uint8_t* want;            /* [n_jobs] 0/1 */
  uint64_t* rec;                  /* [n_jobs][S + 2][3] */
  uint64_t* tru;                  /* [n_jobs][S + 1][2] */
} qm_strata_args;
int qm_extract_files_strata(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                            qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                            void* global_dev, const qm_strata_args* strata);

/* qm_extract_files_ex plus the counts per sequence-context cell over its batch.  Jobs with genome_id[j] >= 0 (a
 * qm_genome_load id: the genome the VCF was called against) get their rows: rec[j][16 ng + 2][3], tru[j][16 ng + 1][2] and
 * gen[j][16 ng + 1] of qm_batch_get_context for half window w and ng GC bins; the others (-1) get zero rows.  Single-base mode:
 * truth hits and both halves run behind the batch's finish; QM_BATCH_ALLELES: the record side only (tru stays zero).  Wanted
 * pure-strain jobs join the batch against an empty truth set, as in qm_extract_files_strata: everything kept is FP, their tru rows
 * are zero.  The VCF outputs, stats and roc are those of qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_context_args {
  int32_t w, ng;
  const int32_t* genome_id;       /* [n_jobs], -1 = the job is not profiled */
  uint64_t* rec;                  /* [n_jobs][16 ng + 2][3] */
  uint64_t* tru;                  /* [n_jobs][16 ng + 1][2] */
  uint64_t* gen;                  /* [n_jobs][16 ng + 1] */
} qm_context_args;
int qm_extract_files_context(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                             qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                             void* global_dev, const qm_context_args* context);

/* qm_extract_files_ex plus the normalisation pass over its batch; mode must be QM_BATCH_ALLELES (QM_E_STATE
 * otherwise).  Mixed-sample jobs with genome_id[j] >= 0 (a qm_genome_load id: the genome the VCF was called against) get their
 * rows rec[j][QM_NORM_R_COLS] and tru[j][QM_NORM_T_COLS] of qm_batch_get_normalize; the others (-1, pure-strain samples) get zero
 * rows.  rescued_out (may be NULL, entries may be NULL): per job a file `#line POS REF ALT NORM_POS NORM_REF NORM_ALT TRUTH_POS
 * TRUTH_REF TRUTH_ALT`, one row per rescued line in file order -- the 1-based line number, the line's own text of the three
 * columns, its normal form, and the truth entry of the smallest index with that form --, written atomically (temp file + rename).
 * The VCF outputs, stats and roc are those of qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_normalize_args {
  const int32_t* genome_id;         /* [n_jobs], -1 = the job takes no part */
  uint64_t* rec;                    /* [n_jobs][QM_NORM_R_COLS] */
  uint64_t* tru;                    /* [n_jobs][QM_NORM_T_COLS] */
  const char* const* rescued_out;   /* [n_jobs] or NULL */
} qm_normalize_args;
int qm_extract_files_normalize(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                               qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                               void* global_dev, const qm_normalize_args* normalize);

/* qm_extract_files_ex plus the atomisation pass over its batch; mode must be QM_BATCH_ALLELES (QM_E_STATE
 * otherwise).  Jobs with want[j] != 0 get their rows rec[j][QM_ATOM_R_COLS] and tru[j][QM_ATOM_T_COLS] of qm_batch_get_atomize;
 * the others get zero rows.  A wanted pure-strain job joins the batch against an empty truth set: its tru row stays zero and
 * every kept line is FP.  atoms_out (may be NULL, entries may be NULL): per job a file `#line POS REF ALT N_ATOMS N_HIT HIT_MASK
 * CLASS`, one row per kept atomisable line with at least 2 atoms in file order -- the 1-based line number, the line's own text
 * of the three columns, the atom count, the hit count, the hit mask in hexadecimal and the class name --, written atomically
 * (temp file + rename).  The VCF outputs, stats and roc are those of qm_extract_files_ex.  Combines with none of the other
 * opt-in views. */
typedef struct qm_atomize_args {
  const uint8_t* want;              /* [n_jobs] */
  uint64_t* rec;                    /* [n_jobs][QM_ATOM_R_COLS] */
  uint64_t* tru;                    /* [n_jobs][QM_ATOM_T_COLS] */
  const char* const* atoms_out;     /* [n_jobs] or NULL */
} qm_atomize_args;
int qm_extract_files_atomize(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                             qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                             void* global_dev, const qm_atomize_args* atomize);

/* qm_extract_files_ex plus the variant-type pass over its batch; mode must be QM_BATCH_ALLELES (QM_E_STATE
 * otherwise).  The shape table is built from the call's own dictionary once every file is tokenised.  Mixed-sample jobs with
 * want[j] != 0 get their rows rec[j][n_rows][2] and tru[j][n_rows][2] of qm_batch_get_types (n_rows = 5 n_bins + 4); the others,
 * pure-strain jobs among them, get zero rows.  The VCF outputs, stats and roc are those of qm_extract_files_ex.  Combines with
 * none of the other opt-in views. */
typedef struct qm_types_args {
  const int32_t* edges;             /* [n_bins] */
  int32_t n_bins;
  int32_t reserved;
  const uint8_t* want;              /* [n_jobs] */
  uint64_t* rec;                    /* [n_jobs][5 n_bins + 4][2] */
  uint64_t* tru;                    /* [n_jobs][5 n_bins + 4][2] */
} qm_types_args;
int qm_extract_files_types(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                           qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                           void* global_dev, const qm_types_args* types);

/* qm_extract_files_ex plus the haplotype pass over its batch; mode must be QM_BATCH_ALLELES (QM_E_STATE
 * otherwise).  Mixed-sample jobs with genome_id[j] >= 0 (a qm_genome_load id: the genome the VCF was called against) get their
 * rows rec[j][QM_HAP_R_COLS] and tru[j][QM_HAP_T_COLS] of qm_batch_get_haplotypes; the others (-1, pure-strain samples) get zero
 * rows.  sites_out (may be NULL, entries may be NULL): per job a file `#site WIN_LO WIN_HI LINES ENTRIES REPLAY_LINES
 * REPLAY_TRUTH`, one row per MATCH site in site order -- the site's index and window, its rescued lines as `line:POS:REF:ALT`
 * joined by `;` (the 1-based line number and the line's own text of the three columns, in file order), its entries found by
 * haplotype as `POS:REF:ALT` in the table's order, and the two replayed strings (bases the genome does not hold print as N) --,
 * written atomically (temp file + rename).  A job that names a file names its genome's bytes too: genome_seq[j] (genome_len[j]
 * of them, the ones handed to qm_genome_load; read during the call only) -- the device keeps the packed genome, the host none.
 * The VCF outputs, stats and roc are those of qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_haplotypes_args {
  const int32_t* genome_id;         /* [n_jobs], -1 = the job takes no part */
  int32_t gap;                      /* 0 .. QM_HAP_MAX_GAP, one for the call */
  int32_t reserved;
  uint64_t* rec;                    /* [n_jobs][QM_HAP_R_COLS] */
  uint64_t* tru;                    /* [n_jobs][QM_HAP_T_COLS] */
  const char* const* sites_out;     /* [n_jobs] or NULL */
  const uint8_t* const* genome_seq; /* [n_jobs] or NULL (then sites_out is NULL too) */
  const int64_t* genome_len;        /* [n_jobs] or NULL */
} qm_haplotypes_args;
int qm_extract_files_haplotypes(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                                void* global_dev, const qm_haplotypes_args* haplotypes);

/* qm_extract_files_haplotypes plus the subset search behind the pass: the first fields are those of
 * qm_haplotypes_args and give what that call gives -- rec, tru and the sites files, byte for byte --; sub[j][QM_HAPSUB_COLS] is
 * the job's row of qm_batch_get_hapsubsets.  subsets_out (may be NULL, entries may be NULL): per job a file `#site WIN_LO WIN_HI
 * RESCUED LEFT_LINES FOUND LEFT_ENTRIES REPLAY_LINES REPLAY_TRUTH`, one row per PARTIAL site in site order -- the lines rescued by
 * subset and the lines left as `line:POS:REF:ALT` joined by `;`, the entries found by subset and the entries left as
 * `POS:REF:ALT`, an empty list as `.`, and the replays of the two chosen subsets --, written atomically.  A job that names either
 * file names its genome's bytes too. */
typedef struct qm_hapsub_args {
  const int32_t* genome_id;         /* [n_jobs], -1 = the job takes no part */
  int32_t gap;                      /* 0 .. QM_HAP_MAX_GAP, one for the call */
  int32_t reserved;
  uint64_t* rec;                    /* [n_jobs][QM_HAP_R_COLS] */
  uint64_t* tru;                    /* [n_jobs][QM_HAP_T_COLS] */
  const char* const* sites_out;     /* [n_jobs] or NULL */
  const uint8_t* const* genome_seq; /* [n_jobs] or NULL (then both lists of files are NULL too) */
  const int64_t* genome_len;        /* [n_jobs] or NULL */
  uint64_t* sub;                    /* [n_jobs][QM_HAPSUB_COLS] */
  const char* const* subsets_out;   /* [n_jobs] or NULL */
} qm_hapsub_args;
int qm_extract_files_hapsubsets(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                                void* global_dev, const qm_hapsub_args* hapsubsets);

/* qm_extract_files_ex plus the QUAL ROC under normal-form and atom matching over its batch; mode must be
 * QM_BATCH_ALLELES (QM_E_STATE otherwise).  The call runs qm_batch_normalize and qm_batch_atomize with their columns itself and
 * hands out none of their rows or files.  Mixed-sample jobs with want[j] != 0 get roc_n[j][3][n_bins], roc_a[j][3][n_bins] and
 * base[j][2] of qm_batch_get_rescue_roc (genome_id[j]: a qm_genome_load id, or -1: the rows by normal form and their baseline
 * stay zero); the others, pure-strain jobs among them, get zero rows.  The VCF outputs, stats and roc are those of
 * qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_rescue_roc_args {
  const int32_t* genome_id;         /* [n_jobs], -1 = no genome */
  const uint8_t* want;              /* [n_jobs] */
  uint64_t* roc_n;                  /* [n_jobs][3][n_bins] */
  uint64_t* roc_a;                  /* [n_jobs][3][n_bins] */
  uint64_t* base;                   /* [n_jobs][2] */
} qm_rescue_roc_args;
int qm_extract_files_rescue_roc(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                                void* global_dev, const qm_rescue_roc_args* rescue_roc);

/* qm_extract_files_ex plus the four rescues combined over its batch; mode must be QM_BATCH_ALLELES (QM_E_STATE
 * otherwise).  The call runs qm_batch_normalize, qm_batch_atomize, qm_batch_haplotypes (gap: 0 .. QM_HAP_MAX_GAP) and -- subsets
 * != 0 -- qm_batch_hapsubsets with their columns itself and hands out none of their rows or files.  Mixed-sample jobs with
 * want[j] != 0 get rec[j][QM_LADDER_COLS] and tru[j][QM_LADDER_COLS] of qm_batch_get_ladder (genome_id[j]: a qm_genome_load id,
 * named in the normalisation and in the haplotype call; -1: the bits N, H and B stay zero); the others, pure-strain jobs among
 * them, get zero rows.  ladder_out (NULL, or per job NULL or a path): `#kind line POS REF ALT METHODS TIER`, one row per kept line
 * that is no TP line in file order (kind `line`, the 1-based line number, the line's own text of the three columns, its method
 * set as letters of NAHB joined by `+` or `none`, its tier normalized / atomized / haplotype / subset or `none`), then one row
 * per truth entry no kept record spells in table order (kind `entry`, `.`, the entry).  The VCF outputs, stats and roc are those
 * of qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_ladder_args {
  const int32_t* genome_id;         /* [n_jobs], -1 = no genome */
  int32_t gap;
  int32_t subsets;
  const uint8_t* want;              /* [n_jobs] */
  uint64_t* rec;                    /* [n_jobs][QM_LADDER_COLS] */
  uint64_t* tru;                    /* [n_jobs][QM_LADDER_COLS] */
  const char* const* ladder_out;    /* NULL, or [n_jobs] */
} qm_ladder_args;
int qm_extract_files_ladder(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                            qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                            void* global_dev, const qm_ladder_args* ladder);

/* qm_extract_files_ex plus the match ladder per variant type and size over its batch; mode must be
 * QM_BATCH_ALLELES (QM_E_STATE otherwise).  The call runs the four rescues with their columns as qm_extract_files_ladder does,
 * then qm_batch_types with its row bytes (the shape table from the call's own dictionary, as in qm_extract_files_types) and
 * qm_batch_ladder with its mask bytes, and hands out none of their rows or files.  Mixed-sample jobs with want[j] != 0 get
 * rec[j][n_rows][QM_LADDER_COLS] and tru[j][n_rows][QM_LADDER_COLS] of qm_batch_get_ladder_types (n_rows = 5 n_bins + 4;
 * genome_id[j] as in qm_ladder_args); the others, pure-strain jobs among them, get zero rows.  The VCF outputs, stats and roc are
 * those of qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_ladder_types_args {
  const int32_t* genome_id;         /* [n_jobs], -1 = no genome */
  int32_t gap;
  int32_t subsets;
  const uint8_t* want;              /* [n_jobs] */
  const int32_t* edges;             /* [n_bins] */
  int32_t n_bins;
  int32_t reserved;
  uint64_t* rec;                    /* [n_jobs][5 n_bins + 4][QM_LADDER_COLS] */
  uint64_t* tru;                    /* [n_jobs][5 n_bins + 4][QM_LADDER_COLS] */
} qm_ladder_types_args;
int qm_extract_files_ladder_types(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                  qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                                  void* global_dev, const qm_ladder_types_args* ladder_types);

/* qm_extract_files_ex plus the bootstrap pass over its batch.  Jobs with want[j] != 0 get their rows:
 * cnt[j][n_win + 2][4] and rep[j][n_rep][4] of qm_batch_get_boot; the others get zero rows.  Single-base mode: truth hits and
 * both sides run behind the batch's finish; QM_BATCH_ALLELES: the record side only (columns 2 and 3 stay zero).  Wanted
 * pure-strain jobs join the batch against an empty truth set, as in qm_extract_files_strata.  The VCF outputs, stats and roc
 * are those of qm_extract_files_ex.  Combines with none of the other opt-in views. */
typedef struct qm_boot_args {
  int32_t window, n_win, n_rep;
  int32_t reserved;
  uint64_t seed;
  const uint8_t* want;            /* [n_jobs] 0/1 */
  uint64_t* cnt;                  /* [n_jobs][n_win + 2][4] */
  uint64_t* rep;                  /* [n_jobs][n_rep][4] (may be NULL when n_rep = 0) */
} qm_boot_args;
int qm_extract_files_boot(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                          qm_file_stats* stats, uint64_t* roc, double* phase_seconds, const int32_t* truth_slot, int n_slots,
                          void* global_dev, const qm_boot_args* boot);

/* `bgzip -c` (the *.vcf.gz outputs the same rules declare, rules/vis_eval_vcf.smk:29,36 ...): BGZF = gzip members of at
 * most 64 KiB with a 'BC' extra field + the EOF member; zcat and tabix / htslib read it.  level -1 = zlib's default (6,
 * bgzip's default).  Atomic. */
int qm_bgzf_write(const char* path, const uint8_t* data, size_t len, int level);

/* `bgzip -c x.vcf > x.vcf.gz && tabix -p vcf x.vcf.gz` (rules/vis_eval_vcf.smk:36-37, 51-52, 67-68, 82-83): <path> as
 * qm_bgzf_write writes it and <path>.tbi, the tabix index of its data lines (sequence = column 1, begin = POS - 1, end =
 * begin + len(REF) or INFO's END=; bins of the UCSC scheme with a 16 kb linear index over BGZF virtual offsets; htslib's
 * pseudo-bin 37450 per sequence; itself BGZF-compressed).  QM_E_UNSORTED when the sequences do not come in blocks or a
 * position steps backwards -- `tabix` stops on such a file as well --, QM_E_RANGE for coordinates beyond 2^29, QM_E_INVAL
 * for a data line without CHROM / POS; nothing is written then.  Atomic per file. */
int qm_bgzf_write_tbi(const char* path, const uint8_t* data, size_t len, int level);

/* ---- truth-set builder ------------------------------------------------------------------------------
 * `mummer2vcf.py -s <table> [--input-header] [-n] [-t SNP|INDEL] [--output-header] -g <ref.fa>` of rules/genome_diff.smk:22-24
 * (program/mummer2vcf.py:69-357): a MUMmer `show-snps -T` table and the reference FASTA in, the truth VCF out (SNVs of one
 * position collapsed into a multi-allelic ALT, runs of insertions / deletions merged and anchored on the base in front of them,
 * rows ordered by contig and position).  Restated from the reference's text -- Biopython is not in the build image, the
 * reference cannot run there: parity unpinned, hand-derived cases only.  table / fasta: the files' bytes; reference_name: what
 * `##reference=` shall say (the path given to -g); file_date: "YYYYMMDD" for `##fileDate=` or NULL for today; *out: the VCF,
 * malloc'ed, to be released with qm_free.  QM_E_INVAL: a row with fewer than 12 columns or a P1 that is no integer, an indel on
 * a contig the FASTA does not hold; QM_E_RANGE: an indel beyond its contig's end. */
#define QM_M2V_NO_NS 1u          /* -n */
#define QM_M2V_OUTPUT_HEADER 2u  /* --output-header */
#define QM_M2V_INPUT_HEADER 4u   /* --input-header: the table's first four lines are its header */
#define QM_M2V_ONLY_SNP 8u       /* -t SNP */
#define QM_M2V_ONLY_INDEL 16u    /* -t INDEL */
int qm_mummer2vcf(const uint8_t* table, size_t table_len, const uint8_t* fasta, size_t fasta_len, const char* reference_name,
                  unsigned flags, const char* file_date, uint8_t** out, size_t* out_len);
void qm_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* QMVT_H */
