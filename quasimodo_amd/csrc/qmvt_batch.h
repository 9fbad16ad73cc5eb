// qmvt_batch.h -- what every host unit of libqmvt.so sees (internal; the C ABI is include/qmvt.h): the error path, the device
// allocations, contexts with their truth sets, genomes and strata sets, the table of passes and of who reads whom, the batch, and
// the helpers that one unit defines and another calls.
#ifndef QMVT_BATCH_H
#define QMVT_BATCH_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "../../include/qmvt.h"
#include "qmvt_dev.h"
#include "qmvt_classify_pair.h"
#include "qmvt_motif.h"
#include "qmvt_afprofile.h"
#include "qmvt_truthside.h"
#include "qmvt_strata.h"
#include "qmvt_context.h"
#include "qmvt_votes.h"
#include "qmvt_boot.h"
#include "qmvt_nearmiss.h"
#include "qmvt_surface.h"
#include "qmvt_norm.h"
#include "qmvt_atom.h"
#include "qmvt_types.h"
#include "qmvt_haplo.h"
#include "qmvt_rroc.h"
#include "qmvt_ladder.h"
#include "qmvt_ltypes.h"

using namespace qm;

#pragma GCC visibility push(hidden)
int fail(int code, const char* fmt, ...);   // qmvt_api.cpp: the message of qm_last_error
#pragma GCC visibility pop

#define HIPCHK(...) /* (variadic: a call with template arguments holds commas) */             \
  do {                                                                                        \
    hipError_t e_ = (__VA_ARGS__);                                                            \
    if (e_ != hipSuccess) return fail(QM_E_HIP, "%s failed: %s (%s:%d)", #__VA_ARGS__, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

struct Truth {
  uint32_t* d_keys = nullptr;
  int32_t* d_tidx = nullptr;
  int32_t shift = 0, nb = 0;
  int64_t n = 0;
  // allele-extended table (every valid entry, single-base ones included)
  uint32_t* d_xkeys = nullptr;
  int32_t *d_xref = nullptr, *d_xalt = nullptr, *d_xtidx = nullptr;
  int32_t xshift = 0, xnb = 0;
  int64_t xn = 0;
  int64_t atom_total = -1;   // the atoms of the atomisable entries, repeats included; -1: not counted yet
  // how a synthetic truth set was generated (qm_truth_synth*): lets qm_batch_synth generate every VCF of a batch
  // against the truth set it is assigned to
  bool synthetic = false;
  int64_t syn_L = 0, syn_T = 0;
  uint64_t syn_seed = 0;
  int syn_pct = 0;
  // qm_truth_release: the slot stays (ids are stable) and may be reused by a later load; `gen` tells a batch that was
  // created against an earlier tenant of the slot that its truth set is gone
  bool released = false;
  uint32_t gen = 0;
};

// a genome of qm_genome_load: the 4-bit packed sequence k_motif gathers its 3-base windows from.  Slots follow
// the rules of truth sets: stable ids, a released slot is reused by a later load.
struct Genome {
  uint32_t* d_words = nullptr;
  int64_t len = 0;
  bool released = false;
  // the sequence-context table of qm_genome_context / qm_batch_context, built at first use and kept per
  // (half window, GC bins): one cell byte per position (len rounded up to 16), the positions per cell; freed with the genome
  uint8_t* d_ctab = nullptr;
  unsigned long long* d_cgen = nullptr;   // [CX_MAX_CELLS]
  int32_t cx_w = -1, cx_ng = -1;          // what the table was built with (-1: not built)
};

// a strata set of qm_strata_load: the flattened segment table on both sides, and, for tables too large for LDS,
// the coarse index over the int32 positions.  Slots follow the rules of genomes.
struct Strata {
  std::vector<int32_t> bp;
  std::vector<uint32_t> masks;
  int32_t* d_bp = nullptr;
  uint32_t* d_masks = nullptr;
  int32_t* d_cidx = nullptr;
  int32_t shift = 0, n_strata = 0;
  bool released = false;
};

struct qm_ctx {
  int dev = 0;
  hipStream_t stream = nullptr;
  hipStream_t aux = nullptr;     // the run's row sums beside its compaction; the hashed join of a bucket chunk beside its scatter
  std::vector<Truth> truths;
  TruthDev* d_truths = nullptr;  // device copy of the descriptors
  int d_truths_cap = 0;
  int64_t path_total[QM_N_PATH_STATS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // qm_path_stats_total: every finish of every batch of this context
  std::vector<Genome> genomes;
  std::vector<Strata> strata;
};

template <typename T>
static int dalloc(T** p, size_t count) {
  *p = nullptr;
  if (count == 0) count = 1;
  const size_t bytes = count * sizeof(T);
  hipError_t e = hipMalloc((void**)p, bytes);
  if (e != hipSuccess) return fail(QM_E_NOMEM, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
  return QM_OK;
}
#define DALLOC(p, n)                 \
  do {                               \
    int rc_ = dalloc(&(p), (n));     \
    if (rc_ != QM_OK) return rc_;    \
  } while (0)

// A device array a batch owns: the pointer and how many elements it holds, freed with its owner.  It reads as a T* wherever launch
// parameters are filled in.  grow() is the only place an array is allocated, freed or counted (*bytes: qm_batch::dev_bytes).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  int64_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(p); }
  operator T*() const { return p; }
  // At least `need` elements (a first use allocates whatever it asks for); the contents do not survive growing.
  // (Growing an array frees the old one.  A speculative bucket chunk returns with its last kernels still queued -- they read d_segs,
  // the cursors' "bad" word, the rows -- and the NEXT chunk of the same finish may grow exactly those: the device is drained first,
  // explicitly.  hipFree would do so implicitly; the code must not depend on that.  ADVICE round 5.)
  int grow(int64_t need, int64_t* bytes) {
    if (p && need <= cap) return QM_OK;
    if (p) (void)hipDeviceSynchronize();
    (void)hipFree(p);
    p = nullptr;
    *bytes -= cap * (int64_t)sizeof(T);
    cap = 0;
    const int rc = dalloc(&p, (size_t)need);
    if (rc != QM_OK) return rc;
    *bytes += need * (int64_t)sizeof(T);
    cap = need;
    return QM_OK;
  }
};

struct Layout {
  std::vector<VcfDesc> vcfs;
  std::vector<SpanDesc> spans;
  std::vector<int32_t> tile_vcf;
  int64_t n_pad = 0;     // records allocated
  int64_t n_total = 0;   // records present
  int64_t max_n = 0;
};

// the paths of a VCF found out of order (route())
enum class Path : uint8_t { Radix, OneLevel, TwoLevel, Partitions, Wide };

// ---- the passes over a finished batch (include/qmvt.h at qm_batch_run) ----
enum PassId { P_MOTIFS, P_AFP, P_TRUTH, P_STRATA, P_BOOT, P_VOTES, P_NEARMISS, P_SURFACE, P_CONTEXT, P_NORM, P_ATOM, P_TYPES, P_HAPLO,
              P_HAPSUB, P_RROC, P_LADDER, P_LTYPES, N_PASSES };
constexpr int PASS_MAX_MARKS = 6;   // qm_batch_haplotypes'
// What a batch keeps of every pass, qm_batch::pass[id].  Both kinds of event are created at first use: a batch that never ran a
// pass holds none, and whatever walks the passes (wait_passes, the reset in qm_batch_run, batch_free) makes no HIP call for it.
struct PassState {
  hipEvent_t done = nullptr;              // behind the last kernel of the latest call, on whatever stream it was enqueued (no timing)
  hipEvent_t mark[PASS_MAX_MARKS] = {};   // qm_batch_set_timing: around its kernels (pass_marks, pass_mark)
  bool timed = false;                     // the latest call recorded them
  unsigned made = 0;                      // what the latest call made behind the latest run (1, or the pass's own bits); 0: nothing
};
// One row per pass, indexed by PassId: the entry point that enqueues it (as the getters' refusals name it), its timing marks
// (0: the pass has no qm_batch_*_timings) and since when its result counts ("no <name> behind the latest <since>").
// A new pass adds its PassId and its row HERE, a row of READS for every pass it reads, and nothing else: the members of qm_batch,
// batch_free, the reset in qm_batch_run, wait_passes and what a producer called again does about its readers follow from the two tables.
struct PassInfo { const char* name; int marks; const char* since; };
#pragma GCC visibility push(hidden)   // one PASSES and one READS in the library, neither in its dynamic symbol table
inline const PassInfo PASSES[N_PASSES] = {
    {"qm_batch_motifs", 0, "run"},     {"qm_batch_af_profile", 0, "run"}, {"qm_batch_truth_hits", 0, "run"},
    {"qm_batch_strata", 0, "run"},     {"qm_batch_boot", 0, "run"},       {"qm_batch_votes", 5, "run"},
    {"qm_batch_nearmiss", 3, "run"},   {"qm_batch_surface", 4, "run"},    {"qm_batch_context", 4, "run"},
    {"qm_batch_normalize", 4, "run"},  {"qm_batch_atomize", 4, "run"},    {"qm_batch_types", 3, "run"},
    {"qm_batch_haplotypes", 6, "run"}, {"qm_batch_hapsubsets", 2, "qm_batch_haplotypes"},
    {"qm_batch_rescue_roc", 5, "run of its producers"},                   {"qm_batch_ladder", 3, "run of its producers"},
    {"qm_batch_ladder_types", 3, "run of its producers"},
};
// (P_HAPLO: qm_batch_haplotypes waits on the host for its own stream at its readback, so only its last three kernels can be in
// flight behind the call; no test holds them up, the ordering effect of that row is not pinned by any -- tests/test_gpu_haplo_streams.py)

// Which pass reads which, one row per edge.  need: the bits of the producer's made the reader asks for (~0u: that it ran); call:
// the producer's call as the reader's refusal prints it (pass_needs).  forget: the bits of the READER's made that go when the
// producer is called again: it rewrites and may regrow what the reader reads, so it first waits on the host for the reader
// (pass_open, in the order of the rows).  None for the readers of P_TRUTH: the bitmaps of one run are the same whoever asks for
// them again, and that pass orders itself behind them on the stream (wait_passes).  A reader decides per call which edges it uses.
struct PassRead { PassId reader, producer; unsigned need, forget; const char* call; };
inline constexpr PassRead READS[] = {
    {P_STRATA, P_TRUTH, ~0u, 0, "a qm_batch_truth_hits"},   {P_BOOT, P_TRUTH, ~0u, 0, "a qm_batch_truth_hits"},
    {P_VOTES, P_TRUTH, ~0u, 0, "a qm_batch_truth_hits"},    {P_NEARMISS, P_TRUTH, ~0u, 0, "a qm_batch_truth_hits"},
    {P_CONTEXT, P_TRUTH, ~0u, 0, "a qm_batch_truth_hits"},
    {P_RROC, P_NORM, QM_NORM_COLUMNS, QM_RROC_NORM, "qm_batch_normalize(.., QM_NORM_COLUMNS)"},
    {P_LADDER, P_NORM, QM_NORM_COLUMNS, ~0u, "qm_batch_normalize(.., QM_NORM_COLUMNS)"},
    {P_RROC, P_ATOM, QM_ATOM_COLUMNS, QM_RROC_ATOM, "qm_batch_atomize(QM_ATOM_COLUMNS)"},
    {P_LADDER, P_ATOM, QM_ATOM_COLUMNS, ~0u, "qm_batch_atomize(QM_ATOM_COLUMNS)"},
    {P_HAPSUB, P_HAPLO, ~0u, ~0u, "qm_batch_haplotypes"},   // (refused by pass_ran and a sentence of the search's own)
    {P_LADDER, P_HAPLO, QM_HAP_COLUMNS, ~0u, "qm_batch_haplotypes(.., QM_HAP_COLUMNS)"},
    {P_LADDER, P_HAPSUB, QM_HAPSUB_COLUMNS, ~0u, "qm_batch_hapsubsets(QM_HAPSUB_COLUMNS)"},
    {P_LTYPES, P_TYPES, QM_TYPE_COLUMNS, ~0u, "qm_batch_types(.., QM_TYPE_COLUMNS)"},
    {P_LTYPES, P_LADDER, QM_LADDER_COLUMNS, ~0u, "qm_batch_ladder(.., QM_LADDER_COLUMNS)"},
    // (never asked for nor waited for by qm_batch_ladder_types: its ladder stands behind them.  The rows say what a rescue called
    // again does: it forgets the ladder it fed, and with it the cross of that ladder's mask bytes -- forgetting is per edge, not
    // passed on from reader to reader)
    {P_LTYPES, P_NORM, ~0u, ~0u, "qm_batch_normalize"},     {P_LTYPES, P_ATOM, ~0u, ~0u, "qm_batch_atomize"},
    {P_LTYPES, P_HAPLO, ~0u, ~0u, "qm_batch_haplotypes"},   {P_LTYPES, P_HAPSUB, ~0u, ~0u, "qm_batch_hapsubsets"},
};
#pragma GCC visibility pop
// The row of an edge, -1 without one: a pass that refuses for, or waits for, a pass it is not said to read does not compile.
constexpr int read_row(int reader, int producer) {
  for (int i = 0; i < (int)(sizeof READS / sizeof READS[0]); ++i)
    if (READS[i].reader == reader && READS[i].producer == producer) return i;
  return -1;
}
constexpr bool reads_sound() {
  for (const PassRead& r : READS)
    if (r.reader == r.producer || r.reader >= N_PASSES || r.producer >= N_PASSES || !r.need) return false;
  return true;
}
static_assert(reads_sound(), "READS: a pass reads itself, names no pass or needs nothing");

struct qm_batch {
  qm_ctx* ctx = nullptr;
  int n_vcf = 0, n_bins = 256;
  Layout L;
  // Every device array is a DevBuf: it is counted in dev_bytes where it grows and freed with the batch.
  // columns (or, for the radix-sort scratch batch, the packed key / info pairs)
  DevBuf<uint32_t> pkey, pinf;
  DevBuf<int32_t> pos, ref, alt;
  DevBuf<float> qual;
  DevBuf<uint8_t> flags;
  // batches without QM_BATCH_ALLELES: allele_byte(ref, alt) per record (qmvt_dev.h), what the kernels read instead of the two
  // codes; every writer of ref / alt keeps it up to date
  DevBuf<uint8_t> anib;
  // outputs / workspace
  DevBuf<uint64_t> mask_pass, mask_tp;
  DevBuf<int32_t> idx;
  DevBuf<uint32_t> tile_tp, tile_fp, tile_tp_off, tile_fp_off, vcf_tot;
  DevBuf<uint32_t> span_hist, span_scal, vcf_flags, vcf_posor;
  // bucket path of the unsorted VCFs: one "span" row per (segment, bucket), fake VCF descriptors for k_finalize
  DevBuf<uint32_t> bk_hist, bk_scal;
  DevBuf<VcfDesc> d_bk_vcfs;
  DevBuf<uint64_t> bk_xent;         // allele-extended batches: the second stream's regions (16-byte entries), its cursors and row descriptors
  DevBuf<uint32_t> bk_xcursor;
  DevBuf<HashRowX> bk_xrows;
  DevBuf<uint64_t> bk_ent;          // the bucket regions: [segment][256][8][SortSeg.bk_cap] packed records
  DevBuf<uint32_t> bk_cursor;       // [segment][256][8] fill counts, then one flag word per segment
  DevBuf<int32_t> d_bk_tile_seg;
  DevBuf<HashRow> bk_rows;          // one descriptor per (segment, bucket)
  // rows (ROC, scalars, flags) of the VCFs a bucket chunk redoes, before they are copied under the original VCFs
  DevBuf<uint64_t> bk_roc;
  DevBuf<int64_t> bk_rscal;
  DevBuf<uint32_t> bk_vflags;
  // two-level bucket path (large VCFs): level-1 descriptors, counts, offsets, cursors, entries; VCF-level segment table
  DevBuf<PartSeg> p_segs;
  DevBuf<int32_t> p_tile_seg;
  DevBuf<uint32_t> p_cnt, p_off, p_cursor, p_flags;
  DevBuf<uint64_t> p_ent;
  DevBuf<SortSeg> d_vsegs;
  DevBuf<int32_t> d_vparts;         // partitions in use per VCF
  DevBuf<uint32_t> p_half;
  // throw-away outputs of the rescan after a sort (kept: an allocation per finish costs more than the rescan)
  DevBuf<uint64_t> rs_roc;
  DevBuf<int64_t> rs_scal;
  DevBuf<uint32_t> rs_flags;
  // Which chunk's tables the shared arrays hold (d_segs, d_tile_seg, d_bk_tile_seg, d_ktile_*, d_bk_vcfs, d_vsegs, d_vparts, p_*): the
  // path that built them, its VCFs, what else they follow from (their position bits; the two levels' counts) and what the path needs
  // to launch over them again.  A path that finds its own chunk here uploads nothing (empty vcfs: nothing known).
  struct Tables {
    Path path = Path::Radix;
    std::vector<int> vcfs;
    std::vector<uint32_t> key;
    int nseg = 0;
    int64_t nbt = 0, nkt = 0;        // scatter tiles, K1 tiles
    std::vector<int> seg_vcf;        // the VCF of every segment
  } tables;
  DevBuf<uint64_t> roc, global_acc;
  DevBuf<int64_t> scalars;
  DevBuf<VcfDesc> d_vcfs;
  DevBuf<SpanDesc> d_spans;
  DevBuf<int32_t> d_tile_vcf;
  DevBuf<uint8_t> cls_scratch;     // max_n bytes
  int64_t dev_bytes = 0;           // written by DevBuf::grow, and where the scratch batch comes and goes (ensure_sub)
  // sort path scratch (lazy): one chunk of unsorted VCFs at a time
  qm_batch* sub = nullptr;               // sorted copies of the chunk's VCFs
  std::vector<int64_t> sub_sig;          // record counts the scratch batch was built for
  std::vector<int32_t> sub_tids;         // truth ids its layout was uploaded with
  DevBuf<uint32_t> sk[2], sv[2], si[2], shist, sorbits;
  DevBuf<SortSeg> d_segs;
  DevBuf<int32_t> d_tile_seg, d_ktile_seg, d_ktile_local;
  // Ordering between the context's two streams (no timing).  The run: [0] behind the flags' k_finalize, [1] behind the rows'.
  // The hashed join of a one-level chunk (onelevel_chunk): [p] behind the scatter of range p, ev_join behind the last join.
  static constexpr int JOIN_PARTS = 4;
  hipEvent_t ev_sync[JOIN_PARTS] = {};
  hipEvent_t ev_join = nullptr;
  // behind the k_finalize part of the run that writes the per-VCF flags (and their host-mapped mirrors): qm_batch_finish waits for
  // THIS, not for the whole stream -- what it then queues (the bucket path of the VCFs found out of order) is built and launched
  // while the run's compaction and row sums are still going, and starts right behind them
  hipEvent_t ev_flags = nullptr;
  bool flags_recorded = false;
  // one-level chunks whose flags (overflow, bad position, highest bucket) nobody has looked at yet: their last kernels were queued
  // without a round trip through the host (k_sort_copy_rows looks at the chunk's "bad" word itself); qm_batch_finish settles them
  // behind its last wait (settle_pending) and redoes a chunk that did not fit then
  struct Pending { std::vector<int> vs; int off; int nbk_launch; bool tight, direct; };
  std::vector<Pending> pend;
  int pend_segs = 0;   // mirror words handed out to the chunks of this finish
  // timing
  bool timing = false;
  static constexpr int EV_RING = 32;   // per-kernel events of the latest runs
  static constexpr int EV_PER_RUN = 2 + 5;   // [0] start [1] end, classify start / end, finalize end, compact start / end
  hipEvent_t ev[EV_RING][EV_PER_RUN] = {};
  int64_t timed_runs = 0;
  bool ran = false, finished = false;
  bool ext = false;   // allele-extended: any valid allele code takes part (build-defined widening, config 5)
  uint64_t* last_global = nullptr;
  // The per-truth sums are laid out for the truth sets that existed when the batch was created: later loads on the
  // same context change neither the size of global_acc nor what qm_batch_get_global copies.
  int n_truth = 1;
  std::vector<std::pair<int, uint32_t>> truth_gens;   // (truth id, generation) of every truth set a VCF names
  // host memory the device can write: [16 words, unused since the summary word went][n_vcf flags][n_vcf position bits][n_vcf
  // bucket-row flags][n_vcf highest buckets] -- k_finalize's mirrors of the per-VCF words qm_batch_finish looks at (no copies)
  uint32_t* h_summary = nullptr;
  uint32_t* d_summary = nullptr;
  // where the unsorted VCFs of the last qm_batch_finish went (qm_batch_path_stats)
  int64_t path_stats[QM_N_PATH_STATS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  // What a finish found stays known while the columns stay the same (only qm_batch_upload* / qm_batch_synth write them): a VCF found out
  // of order is not streamed by the optimistic pass again, and qm_batch_finish queues its bucket path behind the run without first
  // waiting for the flags (a host round trip of ~ 0.15 ms per step).  QM_MEMO=0: off.
  std::vector<uint8_t> known;         // per VCF: 1 = out of order, as the last finish found it
  std::vector<uint32_t> known_posor;  // its position bits (vcf_posor of that finish)
  // The position bits a VCF is remembered with come from what the optimistic pass SAW before it left (the first 256 records of a
  // span): an estimate that can lie below the VCF's highest position -- the scatter then flags the chunk, the radix sort redoes it,
  // and with the batch's memory on the same would happen on every run.  The radix sort's first pass ORs ALL keys of its chunk
  // (sorbits): those bits are kept here and join the estimate of the chunk's VCFs, so the next finish sizes their buckets for
  // what they really hold.  Cleared with the batch's memory.
  std::vector<uint32_t> posor_seen;
  std::vector<uint32_t> known_nbk;    // 1 + the highest bucket its records reached on the one-level bucket path (0: not known)
  int n_known = 0;
  bool known_dirty = false;           // the device copy is stale
  DevBuf<uint8_t> d_known;
  bool run_used_known = false;        // the run in flight was launched with d_known
  // The passes over the finished batch: the events, timing marks and "made behind the latest run" word of each (PassState).  What
  // follows, pass by pass, is the data of the pass alone.
  PassState pass[N_PASSES];
  // qm_batch_motifs (lazy: a batch that never asks allocates nothing): the [n_vcf][3][QM_MOTIF_COLS] counts, the per-VCF genome
  // descriptors (page-locked: copied on the call's stream; the pass's event says when the copy and the pass are done)
  DevBuf<uint64_t> d_motifs;
  DevBuf<GenomeRef> d_mgen;
  GenomeRef* h_mgen = nullptr;
  // qm_batch_upload_af / qm_batch_af_profile (lazy, DESIGN.md 4.9: a batch that never uploads frequencies allocates nothing): the
  // af column laid out like pos, the per-VCF "has af" marks (host: set by qm_batch_upload_af, cleared by every writer of the
  // VCF's columns; device: the copy the latest pass read), the [n_vcf][2][n_af][n_pos] grids and [n_vcf][2][QM_AFP_EXTRA] extras
  DevBuf<float> d_af;
  std::vector<uint8_t> h_afmark;      // [n_vcf], sized with the batch: threads that upload different VCFs touch different bytes
  std::mutex af_mu;                   // the first qm_batch_upload_af allocates the column
  DevBuf<uint8_t> d_afmark;
  DevBuf<uint64_t> d_afgrid, d_afextra;
  int32_t afp_cells = 0;              // n_af * n_pos of the latest qm_batch_af_profile
  // qm_batch_truth_hits (lazy): the per-VCF hit bitmaps one behind the other (h_hit_off[v] = first word of VCF v,
  // h_hit_off[n_vcf] = all), the record mask (the size of mask_pass), the lookup counter
  DevBuf<uint32_t> d_hits;
  DevBuf<uint64_t> d_intruth;
  DevBuf<int64_t> d_hit_off;
  std::vector<int64_t> h_hit_off, h_hit_tn;   // h_hit_tn[v]: T' of VCF v's truth set when the bitmaps were sized
  bool hit_off_uploaded = false, intruth_cleared = false, hits_enqueued = false;
  // qm_batch_strata (lazy): [n_vcf][S + 2][2] kept / TP lines, [n_vcf][S + 1][2] truth keys / hit ones, the bit
  // planes of every distinct truth set one behind the other, the per-VCF rows of k_strata_truth
  DevBuf<uint64_t> d_srec, d_stru;
  DevBuf<uint32_t> d_splanes;
  DevBuf<StrataTruthRow> d_srows;
  int32_t strata_S = 0;               // strata of the latest qm_batch_strata
  // qm_batch_boot (lazy): [n_vcf][n_win + 2][4] counts, [n_vcf][n_rep][4] replicates, the per-VCF rows of
  // k_boot_truth
  DevBuf<uint64_t> d_bcnt, d_brep;
  DevBuf<BootTruthRow> d_brows;
  int32_t boot_nwin = 0, boot_nrep = 0;   // of the latest qm_batch_boot
  // qm_batch_votes (lazy): the (key, member) pair buffers of the radix sort (the second pair holds the distinct keys
  // and their masks afterwards), its histograms and tables, the per-group descriptors, cursors, counts and the five output
  // tables one behind the other
  DevBuf<uint32_t> vt_k[2], vt_v[2], vt_hist, vt_thd, vt_cursor;   // vt_cursor: [n_groups] pairs written, then [n_groups] distinct keys
  DevBuf<SortSeg> vt_segs;
  DevBuf<int32_t> vt_tile_seg, vt_slot;
  DevBuf<VoteGroup> vt_groups;
  DevBuf<uint64_t> vt_out;
  std::vector<int64_t> vt_koff;       // first pair of every group of the latest qm_batch_votes
  int32_t votes_groups = 0;
  // qm_batch_nearmiss (lazy): the four bit planes, each laid out like d_hits (plane p of VCF v starts at word
  // p * h_hit_off[n_vcf] + h_hit_off[v]), one class byte per record laid out like pos, the [n_vcf][6] and [n_vcf][5] counts one
  // behind the other, the T' of every VCF for k_nearmiss_truth
  DevBuf<uint32_t> nm_planes;
  DevBuf<uint8_t> nm_rcls;
  DevBuf<uint64_t> nm_out;
  DevBuf<int64_t> nm_tn;
  bool nm_tn_uploaded = false;
  // qm_batch_surface (lazy): one u32 per (VCF, truth key) -- the best cell code of the key's records; row v starts
  // at h_sf_off[v] --, the [n_vcf][3][nq * na] grids (suffix sums once k_surface_sums ran) and [n_vcf][QM_SF_EXTRA] extras one
  // behind the other, the pass's own copy of the "has af" marks
  DevBuf<uint32_t> sf_best;
  DevBuf<int64_t> sf_off;
  DevBuf<uint64_t> sf_out;
  DevBuf<uint8_t> sf_mark;
  std::vector<int64_t> h_sf_off;      // [n_vcf + 1], from the truth sets' T' at the first call
  bool sf_off_uploaded = false;
  int32_t sf_cells = 0;               // nq * na of the latest qm_batch_surface
  // qm_batch_context (lazy): [n_vcf][16 ng + 2][2] kept / TP lines, [n_vcf][16 ng + 1][2] truth keys / hit ones,
  // [n_vcf][16 ng + 1] positions per cell (copies of the genomes' counts as the pass saw them), the per-VCF tables and the rows
  // of k_context_truth
  DevBuf<uint64_t> cx_rec, cx_tru, cx_gen;
  DevBuf<ContextTab> cx_tabs;
  DevBuf<ContextTruthRow> cx_rows;
  bool cx_built = false;              // ... and built a table (else its build time is 0)
  int32_t cx_ng = 0;                  // GC bins of the latest qm_batch_context
  // qm_batch_normalize (lazy): the tables of the (truth set, genome) pairs the VCFs name in one pool, the per-VCF
  // descriptors and bitmaps, [n_vcf][QM_NORM_R_COLS] / [n_vcf][QM_NORM_T_COLS] counts, a class byte per record and, on request,
  // the normalised columns with the truth row of every record's form
  DevBuf<uint32_t> nz_pool, nz_bits;
  DevBuf<NormVcf> nz_vcfs;
  DevBuf<uint64_t> nz_rec, nz_tru;
  DevBuf<uint8_t> nz_cls;
  DevBuf<int32_t> nz_cols;            // [4][n_pad]: pos, ref, alt, row
  std::vector<uint8_t> nz_has;        // [n_vcf] the VCF named a genome
  // qm_batch_atomize (lazy): the atom sets of the batch's truth sets in one pool, the per-VCF descriptors and
  // bitmaps, [n_vcf][QM_ATOM_R_COLS] / [n_vcf][QM_ATOM_T_COLS] counts and, on request, a class byte, an atom count and a hit mask
  // per record
  DevBuf<uint32_t> at_pool, at_bits;
  DevBuf<AtomVcf> at_vcfs;
  DevBuf<uint64_t> at_rec, at_tru;
  DevBuf<uint8_t> at_cls;             // [2][n_pad]: class bytes, atom counts
  DevBuf<uint16_t> at_hm;             // [n_pad]
  // qm_batch_types (lazy): the per-VCF descriptors and the pass's own found bitmaps, [n_vcf][n_rows][2] counts of
  // records and of truth entries, the shape table ([3][n]: len, head, tail) and, on request, a row byte per record
  DevBuf<uint32_t> ty_bits, ty_shapes;
  DevBuf<TypeVcf> ty_vcfs;
  DevBuf<uint64_t> ty_rec, ty_tru;
  DevBuf<uint8_t> ty_row;             // [n_pad]
  int32_t ty_rows = 0;                // n_rows of the latest qm_batch_types
  TypeBins ty_bins = {};              // ... its size bins and the rows of its shape table in ty_shapes: what types a truth entry
  int64_t ty_nshapes = 0;             //     again (qm_batch_ladder_types)
  // qm_batch_haplotypes (lazy): the site tables of the (truth set, genome) pairs the VCFs name in one pool, the
  // per-VCF descriptors and bitmaps, [n_vcf][QM_HAP_R_COLS] / [n_vcf][QM_HAP_T_COLS] counts, a class byte and a site index per
  // record, the open lines of every (VCF, open site) pair and, on request, a class byte per (VCF, truth entry)
  DevBuf<uint32_t> hp_pool, hp_bits;
  DevBuf<HapVcf> hp_vcfs;
  DevBuf<uint64_t> hp_rec, hp_tru;
  DevBuf<unsigned long long> hp_total;
  DevBuf<uint8_t> hp_cls, hp_ecls;    // [n_pad]; the entries of every VCF's truth set, VCF after VCF
  DevBuf<int32_t> hp_site;            // [n_pad]
  DevBuf<int32_t> hp_pairs;           // [pairs][QM_HAP_MAX_ITEMS + 3]
  std::vector<uint8_t> hp_has;        // [n_vcf] the VCF named a genome
  std::vector<int64_t> hp_eoff;       // [n_vcf + 1] the VCF's entries in hp_ecls
  std::vector<int32_t> hp_gids;       // [n_vcf] the genome ids of the latest qm_batch_haplotypes
  int64_t hp_npairs = 0;              // the (VCF, open site) pairs it read back
  // qm_batch_hapsubsets (lazy): [n_vcf][QM_HAPSUB_COLS] counts, a word per pair (searched or not, the two masks)
  // and, on request, second class bytes per record and per (VCF, truth entry)
  DevBuf<uint64_t> hs_sub;
  DevBuf<uint32_t> hs_res;
  DevBuf<uint8_t> hs_cls, hs_ecls;
  bool hs_listed = false;             // hs_list holds the PARTIAL pairs of the latest search
  std::vector<int32_t> hs_list;       // (VCF, site, S mask, T mask) per PARTIAL pair, VCF after VCF, sites ascending
  // qm_batch_rescue_roc (lazy): the 16-bit best cells of every VCF's units in one pool (by normal form: a cell per
  // truth entry; by atoms: a cell per slot of the atom set and per entry), the per-VCF descriptors, [2][n_vcf][3][n_bins] rows
  // (suffix sums once k_rroc_units ran) and [n_vcf][2] baselines one behind the other
  DevBuf<uint32_t> rr_best;
  DevBuf<RrocVcf> rr_vcfs;
  DevBuf<uint64_t> rr_out;
  // qm_batch_ladder (lazy): the per-VCF descriptors, [n_vcf][QM_LADDER_COLS] counts of records and of truth entries
  // one behind the other and, on request, a mask byte per record and per (VCF, truth entry)
  DevBuf<LadderVcf> ld_vcfs;
  DevBuf<uint64_t> ld_out;
  DevBuf<uint8_t> ld_mask, ld_emask;   // [n_pad]; the entries of every VCF's truth set, VCF after VCF
  std::vector<int64_t> ld_eoff;        // [n_vcf + 1] the VCF's entries in ld_emask
  // qm_batch_ladder_types (lazy): [n_vcf][n_rows][QM_LADDER_COLS] counts of records and of truth entries one
  // behind the other; the per-VCF descriptors it reads are the ones its two producers left (ty_vcfs, ld_vcfs)
  DevBuf<uint64_t> lt_out;
  int32_t lt_rows = 0;                 // n_rows of the latest qm_batch_ladder_types
};

#define NEED_FINISHED(b, name) \
  if (!(b) || !(b)->finished) return fail(QM_E_STATE, name ": call qm_batch_run + qm_batch_finish first")

// ---- defined in one unit, called from another: hidden, so that the library exports what it exported as one file ----
#pragma GCC visibility push(hidden)
// qmvt_api.cpp
void build_layout(const int64_t* n_records, const int32_t* truth_ids, int n_vcf, Layout& L);
bool memo_on();
void forget_known(qm_batch* b, int v);
void batch_free(qm_batch* b);
int upload_layout(qm_batch* b);
int batch_alloc(qm_ctx* c, int n_vcf, const int64_t* n_records, const int32_t* truth_ids, int n_bins, qm_batch** out,
                bool packed = false, bool packed_alleles = false, bool alleles = false);
ClassifyParams classify_params(qm_batch* b);
FinalizeParams finalize_params(qm_batch* b, uint64_t* global);
CompactParams compact_params(qm_batch* b);
#pragma GCC visibility pop

#endif  // QMVT_BATCH_H
