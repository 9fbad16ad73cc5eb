// qmvt_pipeline.cpp -- qm_extract_files: the whole per-VCF worker of the reference
// (program/extract_TP_FP_SNPs.py:12-57 hcmv, :60-105 custom) for MANY VCFs in one call, files in, files out:
//
//   map the inputs  ->  tokenise (host threads, straight into page-locked column buffers)  ->  host path for the
//   lines the columns cannot describe  ->  asynchronous upload of each VCF as soon as it is tokenised  ->  ONE
//   engine batch (classify, finalize, compact)  ->  class masks back (2 bits per record)  ->  the three output
//   files of every VCF, gathered from the mapped input with writev (host threads).
//
// Replaces, per VCF: three awk passes + grep over the input, two awk passes over the truth file, fgrep -wf and
// fgrep -wvf (extract_TP_FP_SNPs.py:24-32,47-57), and the `>` redirections.  Nothing here classifies on the CPU:
// without a HIP device qm_init has already failed.
#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/qmvt.h"

// from qmvt_host.cpp (same library, not part of the public ABI)
void qm_host_count_lines(const uint8_t* text, size_t len, int64_t* n_lines, int64_t* n_data);
int qm_host_scan_threads(const uint8_t* text, size_t len, int64_t cap_lines, int64_t* line_off, uint8_t* line_kind, int32_t* pos,
                         int32_t* ref, int32_t* alt, float* qual, uint8_t* flags, qm_vcf_cols* info, qm_dict* dict, int nthreads);
int qm_host_write_masks(const char* path, const uint8_t* text, size_t len, int64_t n_lines, const int64_t* line_off,
                        const uint8_t* line_kind, const uint64_t* kept, const uint64_t* tp, const uint8_t* flags, int select);
int qm_host_threads(void);
int qm_host_af_text(const uint8_t* line, size_t n, const uint8_t** cb, const uint8_t** ce);   // what the rule's AF pattern captures in a data line
void qm_set_error(const char* msg);   // qmvt_api.cpp: what qm_last_error returns
int qm_device_add_u64(qm_ctx* ctx, uint64_t* dst, const uint64_t* src, int64_t n);   // qmvt_api.cpp: dst[i] += src[i] on the device, blocking
int qm_device_zero(qm_ctx* ctx, void* dst, size_t bytes);                              // qmvt_api.cpp: on the context's device, blocking

namespace {

double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// user + system seconds of the whole process so far (QM_FILES_TRACE: what a phase cost in CPU time, the currency of a box with a CPU quota)
double cpu_now() {
  struct rusage u;
  if (getrusage(RUSAGE_SELF, &u) != 0) return 0.0;
  return (double)u.ru_utime.tv_sec + (double)u.ru_stime.tv_sec + 1e-6 * ((double)u.ru_utime.tv_usec + (double)u.ru_stime.tv_usec);
}

struct Mapped {
  const uint8_t* p = nullptr;
  size_t n = 0;
  bool ok = false;
  Mapped() = default;
  Mapped(const Mapped&) = delete;
  Mapped& operator=(const Mapped&) = delete;
  Mapped(Mapped&& o) noexcept : p(o.p), n(o.n), ok(o.ok) { o.p = nullptr; o.n = 0; o.ok = false; }
  void open_file(const char* path) {
    const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return;
    struct stat st;
    if (fstat(fd, &st) != 0) { ::close(fd); return; }
    n = (size_t)st.st_size;
    if (n == 0) { ok = true; ::close(fd); return; }
    void* m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
    ::close(fd);
    if (m == MAP_FAILED) { n = 0; return; }
    (void)madvise(m, n, MADV_SEQUENTIAL | MADV_WILLNEED);
    p = (const uint8_t*)m;
    ok = true;
  }
  ~Mapped() { if (p) munmap((void*)p, n); }
};

template <typename F> void parallel_for(int n, int nthreads, F f) {
  if (n <= 0) return;
  nthreads = std::max(1, std::min(nthreads, n));
  if (nthreads == 1) { for (int i = 0; i < n; ++i) f(i); return; }
  std::atomic<int> next{0};
  std::vector<std::thread> th;
  for (int t = 0; t < nthreads; ++t)
    th.emplace_back([&]() { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) f(i); });
  for (auto& x : th) x.join();
}

// page-locked column buffers, kept by the process across calls (pinning memory costs more than filling it)
struct PinnedArena {
  uint8_t* base = nullptr;
  size_t cap = 0;
  bool pinned = false;
  uint8_t* get(size_t need) {
    if (need <= cap) return base;
    release();
    need = need + need / 4 + (1 << 20);
    void* p = nullptr;
    if (hipHostMalloc(&p, need, hipHostMallocDefault) == hipSuccess) { base = (uint8_t*)p; cap = need; pinned = true; return base; }
    (void)hipGetLastError();
    base = (uint8_t*)malloc(need);   // pageable: the copies still work, only slower
    cap = base ? need : 0;
    pinned = false;
    return base;
  }
  void release() {
    if (base) { if (pinned) (void)hipHostFree(base); else free(base); }
    base = nullptr; cap = 0;
  }
  ~PinnedArena() { release(); }
};
// One arena per context (= per device): calls on different contexts -- a thread and a context per GPU, examples/qm_multi.c --
// tokenise, upload and write side by side; two calls on ONE context take turns.  The table itself is never destroyed: at
// process exit the HIP runtime may be gone before static destructors run; qm_destroy releases a context's arena.
struct CtxArena { PinnedArena arena; std::mutex mu; };
std::map<qm_ctx*, CtxArena*>& g_arenas = *new std::map<qm_ctx*, CtxArena*>();
std::mutex* g_arenas_mu = new std::mutex();
CtxArena* arena_of(qm_ctx* ctx) {
  std::lock_guard<std::mutex> g(*g_arenas_mu);
  CtxArena*& a = g_arenas[ctx];
  if (!a) a = new CtxArena();
  return a;
}

struct JobState {
  Mapped vcf;
  int64_t n_lines = 0, n_data = 0;
  std::vector<int64_t> line_off;
  std::vector<uint8_t> line_kind;
  int32_t *pos = nullptr, *ref = nullptr, *alt = nullptr;
  float* qual = nullptr;
  uint8_t* flags = nullptr;
  uint64_t *kept = nullptr, *tp = nullptr;   // class masks, (n_data + 63) / 64 words each
  qm_vcf_cols info{};
  int64_t ex[5] = {0, 0, 0, 0, 0};
  std::vector<float> af;   // (profiled jobs) qm_vcf_scan_af's column
  int truth = -1;      // index into the call's distinct truth files
  int batch_v = -1;    // VCF index inside the engine batch (mixed samples only)
  int rc = QM_OK;
  std::string err;     // the message that belongs to rc (qm_last_error is per thread: copied on the worker that failed)
};

struct TruthState {
  std::string path;
  int mode = 0;
  Mapped file;
  qm_patterns* pats = nullptr;
  int64_t info[4] = {0, 0, 0, 0}, counts[5] = {0, 0, 0, 0, 0};
  int tid = -1;
  int rc = QM_OK;
  std::vector<uint32_t> keys;   // (truth-side calls) the sorted distinct single-base keys, as the device holds them
};

int fail(int code, const std::string& msg) { qm_set_error(msg.c_str()); return code; }

// ---- missed-variant lists ----
bool ts_canon_pos(const uint8_t* s, size_t n, uint32_t* out) {   // "0" or [1-9][0-9]*, value < 2^28: qmvt_host.cpp's rule
  if (n == 0 || n > 9 || (n > 1 && s[0] == '0')) return false;
  uint32_t v = 0;
  for (size_t i = 0; i < n; ++i) { if (s[i] < '0' || s[i] > '9') return false; v = v * 10 + (uint32_t)(s[i] - '0'); }
  if (v >= (uint32_t)QM_POS_LIMIT) return false;
  *out = v;
  return true;
}
int ts_base(const uint8_t* s, size_t n) {
  if (n != 1) return -1;
  switch (s[0]) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}
int write_all_atomic(const char* path, const std::string& data) {
  const std::string tmp = std::string(path) + ".tmp." + std::to_string((long)getpid());
  FILE* fh = fopen(tmp.c_str(), "wb");
  if (!fh) return QM_E_IO;
  const bool ok = data.empty() || fwrite(data.data(), 1, data.size(), fh) == data.size();
  if (fclose(fh) != 0 || !ok || rename(tmp.c_str(), path) != 0) { (void)unlink(tmp.c_str()); return QM_E_IO; }
  return QM_OK;
}
// The truth file's '#' lines, then, in file order, every data row whose key the reference puts into `Genome` (mode 0: single-base
// REF and ALT, caller_performance_compare.R:29-55; mode 1: neither SUB column '.', custom_snp_benchmark.R:23-27) and whose bit
// in `bits` (over the truth set's sorted distinct keys) is clear.  A row whose key the device cannot hold (POS spelled
// non-canonically, a longer allele in mode 1) could only be matched by a kept line without a comparable key; the caller refuses
// VCFs that have such lines, so the row is a missed one.
// (the rule itself: row(text, length, fields, field lengths, k) for every such row, k = the key's index among the truth set's
// sorted distinct keys or -1 when the device cannot hold it; head gets the '#' lines)
template <typename F> void missed_rows(const TruthState& t, const uint32_t* bits, std::string& head, F row) {
  const uint8_t* text = t.file.p;
  const size_t len = t.file.n;
  size_t off = 0;
  while (off < len) {
    const uint8_t* s = text + off;
    const uint8_t* e = (const uint8_t*)memchr(s, '\n', len - off);
    const size_t n = e ? (size_t)(e - s) : len - off;
    off += n + 1;
    if (n && s[0] == '#') { head.append((const char*)s, n); head.push_back('\n'); continue; }
    const uint8_t* f[6]; size_t fl[6]; int nf = 0;
    const uint8_t* q = s;
    while (nf < 6) {
      const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(s + n - q));
      f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(s + n - q); ++nf;
      if (!tb) break;
      q = tb + 1;
    }
    const int ix = t.mode == 0 ? 1 : 0, iy = t.mode == 0 ? 3 : 1, iz = t.mode == 0 ? 4 : 2;
    if (nf <= iz) continue;
    const int y = ts_base(f[iy], fl[iy]), z = ts_base(f[iz], fl[iz]);
    const bool in_genome = t.mode == 0 ? (y >= 0 && z >= 0) : (n > 0 && !(fl[iy] == 1 && f[iy][0] == '.') && !(fl[iz] == 1 && f[iz][0] == '.'));
    if (!in_genome) continue;
    bool hit = false;
    int64_t k = -1;
    uint32_t p = 0;
    if (y >= 0 && z >= 0 && ts_canon_pos(f[ix], fl[ix], &p)) {
      const uint32_t key = (p << 4) | ((uint32_t)y << 2) | (uint32_t)z;
      const auto it = std::lower_bound(t.keys.begin(), t.keys.end(), key);
      if (it != t.keys.end() && *it == key) {
        k = (int64_t)(it - t.keys.begin());
        if (bits) hit = (bits[(size_t)k >> 5] >> (k & 31)) & 1u;
      }
    }
    if (!hit) row(s, n, f, fl, k);
  }
}
int write_fn_file(const char* path, const TruthState& t, const uint32_t* bits) {
  std::string head, rows;
  missed_rows(t, bits, head, [&](const uint8_t* s, size_t n, const uint8_t* const*, const size_t*, int64_t) { rows.append((const char*)s, n); rows.push_back('\n'); });
  return write_all_atomic(path, head + rows);
}

// ---- why-files of the near-miss pass ----
const char* const NM_R_NAMES[QM_NM_R_CLASSES] = {"idcol", "allele", "refbase", "near", "isolated", "nokey"};
const char* const NM_T_NAMES[QM_NM_T_CLASSES] = {"filtered", "allele", "position", "near", "uncalled"};
// `#POS REF ALT class`, then exactly the rows the missed-variant list of the job holds, in its order: their POS / REF / ALT text
// and the class of their key (tcls: one byte per sorted distinct key); `.` for a row the device cannot hold
int write_fn_why_file(const char* path, const TruthState& t, const uint32_t* bits, const uint8_t* tcls) {
  std::string head, rows = "#POS\tREF\tALT\tclass\n";
  const int ix = t.mode == 0 ? 1 : 0, iy = t.mode == 0 ? 3 : 1, iz = t.mode == 0 ? 4 : 2;
  missed_rows(t, bits, head, [&](const uint8_t*, size_t, const uint8_t* const* f, const size_t* fl, int64_t k) {
    for (int i : {ix, iy, iz}) { rows.append((const char*)f[i], fl[i]); rows.push_back('\t'); }
    rows.append(k >= 0 && tcls[k] < QM_NM_T_CLASSES ? NM_T_NAMES[tcls[k]] : ".");
    rows.push_back('\n');
  });
  return write_all_atomic(path, rows);
}

// `Position Frequency type` of every counted record (kept by the class mask, single-base REF and ALT) of one profiled job: the
// FP records, then the TP records, each in file order -- rbind(fp_snp, tp_snp) of varPlot (scripts/mutation_context_profile.R:
// 29-40).  Position is the line's POS text, Frequency the text the rule's pattern captured or NA.
int write_points_file(const char* path, const JobState& s) {
  std::string out[2];   // [FP, TP]
  const uint8_t* text = s.vcf.p;
  const size_t len = s.vcf.n;
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    const uint8_t k = s.line_kind[(size_t)i];
    if (!(k == QM_LINE_DATA || k == QM_LINE_DATA_HOST || k == QM_LINE_REFUSED)) continue;
    const int64_t r = rec++;
    if (!((s.kept[r >> 6] >> (r & 63)) & 1ull) || (uint32_t)(s.ref[r] | s.alt[r]) >= 4u) continue;
    const int tp = (int)((s.tp[r >> 6] >> (r & 63)) & 1ull);
    size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], len);
    if (e > b && text[e - 1] == '\n') --e;
    const uint8_t* t1 = (const uint8_t*)memchr(text + b, '\t', e - b);
    if (!t1) continue;   // (a kept line has its five columns)
    const uint8_t* p0 = t1 + 1;
    const uint8_t* t2 = (const uint8_t*)memchr(p0, '\t', (size_t)(text + e - p0));
    std::string& o = out[tp];
    o.append((const char*)p0, (size_t)((t2 ? t2 : text + e) - p0));
    o.push_back('\t');
    const uint8_t *cb, *ce;
    if (qm_host_af_text(text + b, e - b, &cb, &ce) > 0) o.append((const char*)cb, (size_t)(ce - cb));
    else o.append("NA");
    o.append(tp ? "\tTP\n" : "\tFP\n");
  }
  return write_all_atomic(path, "Position\tFrequency\ttype\n" + out[0] + out[1]);
}

}  // namespace

// called by qm_destroy: the page-locked buffers of a context go with it
void qm_pipeline_ctx_destroyed(qm_ctx* ctx) {
  CtxArena* a = nullptr;
  {
    std::lock_guard<std::mutex> g(*g_arenas_mu);
    auto it = g_arenas.find(ctx);
    if (it != g_arenas.end()) { a = it->second; g_arenas.erase(it); }
  }
  if (a) { { std::lock_guard<std::mutex> g(a->mu); a->arena.release(); } delete a; }
}

namespace {

// ---- the passes over the finished batch of one call (how a pass is wired) ----
// What a call was asked for beyond the three files: every qm_extract_files_* wrapper fills the fields of its pass.
struct Passes {
  const int32_t* genome_id = nullptr;   // the motif pass: a genome id or -1 per job, with motifs_out
  uint64_t* motifs_out = nullptr;
  const qm_profile_args* pa = nullptr; const qm_strata_args* sa = nullptr; const qm_boot_args* ba = nullptr;
  const qm_truthside_args* ts = nullptr; const qm_votes_args* va = nullptr; const qm_nearmiss_args* nm = nullptr;
  const qm_surface_args* sf = nullptr; const qm_context_args* cx = nullptr; const qm_normalize_args* nz = nullptr;
  const qm_atomize_args* at = nullptr; const qm_types_args* ty = nullptr; const qm_haplotypes_args* hp = nullptr;
  const qm_hapsub_args* hs = nullptr; const qm_rescue_roc_args* rr = nullptr; const qm_ladder_args* ld = nullptr;
  const qm_ladder_types_args* lt = nullptr;
  bool has_genome(int j) const { return genome_id && genome_id[j] >= 0; }
  bool wants_profile(int j) const { return pa && pa->want[j] != 0; }
  bool wants_strata(int j) const { return sa && sa->want[j] != 0; }
  bool wants_boot(int j) const { return ba && ba->want[j] != 0; }
  bool wants_surface(int j) const { return sf && sf->want[j] != 0; }
  bool wants_context(int j) const { return cx && cx->genome_id[j] >= 0; }
  bool wants_af(int j) const { return wants_profile(j) || wants_surface(j); }   // the INFO column is scanned and uploaded
  // the passes a pure-strain job joins the batch for (against an empty truth set, for its rows of the pass only: its files,
  // stats and ROC rows are made as for any pure-strain job); every mixed-sample job is in the batch anyway
  bool wants_atomize(int j) const { return at && at->want[j] != 0; }
  bool any_batch_only(int j) const { return has_genome(j) || wants_profile(j) || wants_strata(j) || wants_boot(j) || wants_context(j) || wants_atomize(j); }
};

// what a pass sees of the call: the finished batch and the jobs behind its VCFs
struct PassCtx {
  qm_ctx* ctx; qm_batch* batch; int n_jobs; const qm_file_job* jobs;
  const std::vector<JobState>& J; const std::vector<TruthState>& T;
  size_t nv;   // VCFs in the batch
  bool ext; int nthr;
  qm_dict* dict;   // the long alleles of the call's files (allele-extended calls), complete once stage one is
  // the one rule for errors: a pass that fails sets err
  int lib(int rc, std::string& err) const { if (rc != QM_OK) err = qm_last_error(ctx); return rc; }
  template <typename W> bool any(W want) const { for (int j = 0; j < n_jobs; ++j) if (want(j)) return true; return false; }
  // the batch's row of every wanted job (src, one row of w words per VCF of the batch) into the job's row of the caller's array
  template <typename W> void scatter_rows(uint64_t* dst, const std::vector<uint64_t>& src, size_t w, W want) const {
    for (int j = 0; j < n_jobs && w; ++j)
      if (want(j)) memcpy(dst + (size_t)j * w, &src[(size_t)J[(size_t)j].batch_v * w], sizeof(uint64_t) * w);
  }
  const TruthState& truth_of(int j) const { return T[(size_t)J[(size_t)j].truth]; }
};

bool is_header(uint8_t k) { return k == QM_LINE_HEADER || k == QM_LINE_HEADER_KEPT || k == QM_LINE_HEADER_KEPT_TP || k == QM_LINE_HEADER_REFUSED; }

// the first kept line (1-based) without a comparable key, 0 when there is none
int64_t first_nokey_kept_line(const JobState& s) {
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    if ((s.flags[rec] & QM_F_PASS) && (s.flags[rec] & QM_F_NOKEY)) return i + 1;
    ++rec;
  }
  return 0;
}
// R keys a kept line by its TEXT; a kept line without a comparable key has none the hit bitmaps could hold: the passes that read
// them refuse the VCF by name (`pass`: "the vote pass", "the truth-side view")
int refuse_nokey(const char* vcf_path, const JobState& s, const char* pass, std::string& err) {
  err = std::string(vcf_path) + " line " + std::to_string(first_nokey_kept_line(s)) + ": a kept line has no comparable key (POS is not a canonical decimal) -- " +
        pass + " compares keys, not text, and does not take this VCF";
  return QM_E_NONCANON;
}

// the jobs of every group, and the same as the offsets and batch VCF ids qm_batch_truth_regions / qm_batch_votes take
struct GroupTables { std::vector<std::vector<int>> members; std::vector<int32_t> goff, gids; };
GroupTables group_tables(const PassCtx& c, const int32_t* group, int n_groups) {
  GroupTables g;
  g.members.resize((size_t)n_groups);
  for (int j = 0; j < c.n_jobs; ++j) if (group[j] >= 0) g.members[(size_t)group[j]].push_back(j);
  g.goff.push_back(0);
  for (const auto& m : g.members) {
    for (int j : m) g.gids.push_back(c.J[(size_t)j].batch_v);
    g.goff.push_back((int32_t)g.gids.size());
  }
  return g;
}

// the mutation-context spectra, on the columns and masks still in HBM
int motifs_pass(const PassCtx& c, const Passes& P, std::string& err) {
  auto want = [&](int j) { return P.has_genome(j); };
  if (!P.motifs_out || !c.any(want)) return QM_OK;
  std::vector<int32_t> gid(c.nv, -1);
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) gid[(size_t)c.J[(size_t)j].batch_v] = P.genome_id[j];
  std::vector<uint64_t> mo(c.nv * 3 * QM_MOTIF_COLS);
  int rc = qm_batch_motifs(c.batch, gid.data(), nullptr);
  if (rc == QM_OK) rc = qm_batch_get_motifs(c.batch, mo.data());
  if (rc == QM_OK) c.scatter_rows(P.motifs_out, mo, 3 * QM_MOTIF_COLS, want);
  return c.lib(rc, err);
}

// the allele-frequency profile, behind the motif pass on the same columns and masks
int profile_pass(const PassCtx& c, const qm_profile_args* pa, std::string& err) {
  auto want = [&](int j) { return pa->want[j] != 0; };
  if (!pa || !c.any(want)) return QM_OK;
  const size_t cells = (size_t)pa->n_pos_bins * (size_t)pa->n_af_bins;
  std::vector<uint64_t> gr(c.nv * 2 * cells), ex(c.nv * 2 * QM_AFP_EXTRA);
  int rc = qm_batch_af_profile(c.batch, pa->window, pa->n_pos_bins, pa->n_af_bins, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_af_profile(c.batch, gr.data(), ex.data());
  if (rc == QM_OK) { c.scatter_rows(pa->grid, gr, 2 * cells, want); c.scatter_rows(pa->extra, ex, 2 * QM_AFP_EXTRA, want); }
  return c.lib(rc, err);
}

// the counts per stratum, on the columns, masks and truth keys still in HBM
int strata_pass(const PassCtx& c, const qm_strata_args* sa, std::string& err) {
  auto want = [&](int j) { return sa->want[j] != 0; };
  if (!sa || !c.any(want)) return QM_OK;
  int64_t si[2] = {0, 0};
  int rc = qm_strata_info(c.ctx, sa->strata_id, si);
  const size_t rw = 3 * (size_t)(si[0] + 2), tw = 2 * (size_t)(si[0] + 1);
  std::vector<uint64_t> rec(c.nv * rw), tru(c.nv * tw);
  if (rc == QM_OK && !c.ext) rc = qm_batch_truth_hits(c.batch, nullptr);
  if (rc == QM_OK) rc = qm_batch_strata(c.batch, sa->strata_id, c.ext ? QM_STRATA_RECORDS : (QM_STRATA_RECORDS | QM_STRATA_TRUTH), nullptr);
  if (rc == QM_OK) rc = qm_batch_get_strata(c.batch, rec.data(), c.ext ? nullptr : tru.data());
  if (rc == QM_OK) { c.scatter_rows(sa->rec, rec, rw, want); if (!c.ext) c.scatter_rows(sa->tru, tru, tw, want); }
  return c.lib(rc, err);
}

// the counts per sequence-context cell, on the columns, masks and truth keys still in HBM
int context_pass(const PassCtx& c, const Passes& P, std::string& err) {
  const qm_context_args* cx = P.cx;
  auto want = [&](int j) { return P.wants_context(j); };
  if (!cx || !c.any(want)) return QM_OK;
  const size_t nc = (size_t)(16 * cx->ng + 1), rw = 3 * (nc + 1), tw = 2 * nc;
  std::vector<int32_t> gid(c.nv, -1);
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) gid[(size_t)c.J[(size_t)j].batch_v] = cx->genome_id[j];
  std::vector<uint64_t> rec(c.nv * rw), tru(c.nv * tw), gen(c.nv * nc);
  int rc = c.ext ? QM_OK : qm_batch_truth_hits(c.batch, nullptr);
  if (rc == QM_OK) rc = qm_batch_context(c.batch, gid.data(), cx->w, cx->ng, c.ext ? QM_CX_RECORDS : (QM_CX_RECORDS | QM_CX_TRUTH), nullptr);
  if (rc == QM_OK) rc = qm_batch_get_context(c.batch, rec.data(), c.ext ? nullptr : tru.data(), gen.data());
  if (rc == QM_OK) { c.scatter_rows(cx->rec, rec, rw, want); if (!c.ext) c.scatter_rows(cx->tru, tru, tw, want); c.scatter_rows(cx->gen, gen, nc, want); }
  return c.lib(rc, err);
}

// the bootstrap replicates, on the columns, masks and truth keys still in HBM
int boot_pass(const PassCtx& c, const qm_boot_args* ba, std::string& err) {
  auto want = [&](int j) { return ba->want[j] != 0; };
  if (!ba || !c.any(want)) return QM_OK;
  const size_t cw = 4 * (size_t)(ba->n_win + 2), rw = 4 * (size_t)ba->n_rep;
  std::vector<uint64_t> cnt(c.nv * cw), rep(c.nv * rw);
  int rc = c.ext ? QM_OK : qm_batch_truth_hits(c.batch, nullptr);
  if (rc == QM_OK) rc = qm_batch_boot(c.batch, ba->window, ba->n_win, ba->n_rep, ba->seed, c.ext ? QM_BOOT_RECORDS : (QM_BOOT_RECORDS | QM_BOOT_TRUTH), nullptr);
  if (rc == QM_OK) rc = qm_batch_get_boot(c.batch, cnt.data(), rw ? rep.data() : nullptr);
  if (rc == QM_OK) { c.scatter_rows(ba->cnt, cnt, cw, want); c.scatter_rows(ba->rep, rep, rw, want); }
  return c.lib(rc, err);
}

// the callers' side of one group's Venn: the keys of the members' kept records outside the in-truth record mask, through qm_fp_overlap
int fp_regions_of(const PassCtx& c, const std::vector<int>& members, int64_t* out, std::string& err) {
  std::vector<int64_t> so(1, 0);
  std::vector<int32_t> kp, kr, ka;
  for (int j : members) {
    const JobState& s = c.J[(size_t)j];
    std::vector<uint64_t> kept((size_t)(s.n_data + 63) / 64 + 1), tpm(kept.size()), in(kept.size());
    int rc = qm_batch_get_masks(c.batch, s.batch_v, kept.data(), tpm.data());
    if (rc == QM_OK) rc = qm_batch_get_intruth_mask(c.batch, s.batch_v, in.data());
    if (rc != QM_OK) return c.lib(rc, err);
    for (int64_t r = 0; r < s.n_data; ++r)
      if (((kept[(size_t)r >> 6] & ~in[(size_t)r >> 6]) >> (r & 63)) & 1ull) { kp.push_back(s.pos[r]); kr.push_back(s.ref[r]); ka.push_back(s.alt[r]); }
    so.push_back((int64_t)kp.size());
  }
  int64_t reg[QM_TRUTH_REGIONS] = {0};
  int32_t dummy = 0;
  const int rc = qm_fp_overlap(c.ctx, (int)members.size(), so.data(), kp.empty() ? &dummy : kp.data(), kr.empty() ? &dummy : kr.data(),
                               ka.empty() ? &dummy : ka.data(), reg);
  if (rc == QM_OK) memcpy(out, reg, sizeof reg);
  return c.lib(rc, err);
}

// the truth-side view: the missed-variant lists of the jobs, the Venn regions and missed-by-all lists of the groups
int truthside_pass(const PassCtx& c, const qm_truthside_args* ts, std::string& err) {
  if (!ts) return QM_OK;
  auto listed = [&](int j) { return !c.jobs[j].pure && ts->fn_out[j]; };
  for (int j = 0; j < c.n_jobs; ++j)
    if (!c.jobs[j].pure && (ts->fn_out[j] || ts->group[j] >= 0) && c.J[(size_t)j].info.n_nokey_kept)
      return refuse_nokey(c.jobs[j].vcf_path, c.J[(size_t)j], "the truth-side view", err);
  int rc = qm_batch_truth_hits(c.batch, nullptr);
  std::vector<std::vector<uint32_t>> hitbits((size_t)c.n_jobs), unibits((size_t)ts->n_groups);
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    if (!listed(j)) continue;
    hitbits[(size_t)j].assign((c.truth_of(j).keys.size() + 31) / 32, 0u);
    rc = qm_batch_get_truth_hits(c.batch, c.J[(size_t)j].batch_v, hitbits[(size_t)j].data(), (int64_t)hitbits[(size_t)j].size());
  }
  if (rc != QM_OK) return c.lib(rc, err);
  const GroupTables G = group_tables(c, ts->group, ts->n_groups);
  if (ts->n_groups > 0) {
    auto words_of = [&](size_t g) { return (c.truth_of(G.members[g][0]).keys.size() + 31) / 32; };
    size_t uw = 0;
    for (size_t g = 0; g < G.members.size(); ++g) uw += words_of(g);
    std::vector<uint32_t> uni(uw + 1, 0u);
    rc = qm_batch_truth_regions(c.batch, ts->n_groups, G.goff.data(), G.gids.data(), ts->regions, uni.data());
    if (rc != QM_OK) return c.lib(rc, err);
    size_t o = 0;
    for (size_t g = 0; g < G.members.size(); ++g) {
      unibits[g].assign(uni.begin() + (long)o, uni.begin() + (long)(o + words_of(g)));
      o += words_of(g);
    }
    for (size_t g = 0; g < G.members.size() && ts->fp_regions; ++g) {
      rc = fp_regions_of(c, G.members[g], ts->fp_regions + g * QM_TRUTH_REGIONS, err);
      if (rc != QM_OK) return rc;
    }
  }
  // the lists: one per job that asked, one per group that asked (missed by every member)
  struct FTask { const char* path; const TruthState* t; const uint32_t* bits; };
  std::vector<FTask> F;
  for (int j = 0; j < c.n_jobs; ++j)
    if (listed(j)) F.push_back({ts->fn_out[j], &c.truth_of(j), hitbits[(size_t)j].data()});
  for (size_t g = 0; g < G.members.size(); ++g)
    if (ts->missed_out && ts->missed_out[g]) F.push_back({ts->missed_out[g], &c.truth_of(G.members[g][0]), unibits[g].data()});
  std::vector<int> frc(F.size(), QM_OK);
  parallel_for((int)F.size(), c.nthr, [&](int k) { frc[(size_t)k] = write_fn_file(F[(size_t)k].path, *F[(size_t)k].t, F[(size_t)k].bits); });
  for (size_t k = 0; k < F.size(); ++k)
    if (frc[k] != QM_OK) { err = std::string("cannot write ") + F[k].path; return frc[k]; }
  return QM_OK;
}

// ---- k-of-n consensus over groups of jobs ----
// The consensus VCF of one group at level k: the '#' lines of the first member as its filtered file holds them, then one line per
// key with votes >= k in ascending key order -- the votes from the device (hit bitmaps for the truth keys, the distinct keys and
// masks for the others), the line from the host: the first kept line carrying the key in the lowest-numbered member that calls
// it, byte for byte.  Atomic.
int write_consensus(const PassCtx& c, int g, const std::vector<int>& m, int k, const char* path, std::string& err) {
  const TruthState& t = c.truth_of(m[0]);
  int rc = QM_OK;
  // votes: the truth keys from the members' hit bitmaps, the others from the pass's distinct keys and masks
  std::vector<uint32_t> want;
  {
    const size_t nw = (t.keys.size() + 31) / 32;
    std::vector<uint8_t> cnt(t.keys.size(), 0);
    std::vector<uint32_t> bits(nw + 1, 0u);
    for (int j : m) {
      rc = qm_batch_get_truth_hits(c.batch, c.J[(size_t)j].batch_v, bits.data(), (int64_t)nw);
      if (rc != QM_OK) return c.lib(rc, err);
      for (size_t i = 0; i < t.keys.size(); ++i) cnt[i] += (uint8_t)((bits[i >> 5] >> (i & 31)) & 1u);
    }
    for (size_t i = 0; i < t.keys.size(); ++i) if ((int)cnt[i] >= k) want.push_back(t.keys[i]);
    int64_t nu = 0;
    rc = qm_batch_get_vote_keys(c.batch, g, nullptr, nullptr, 0, &nu);
    std::vector<uint32_t> uk((size_t)nu + 1), um((size_t)nu + 1);
    if (rc == QM_OK) rc = qm_batch_get_vote_keys(c.batch, g, uk.data(), um.data(), nu, &nu);
    if (rc != QM_OK) return c.lib(rc, err);
    for (int64_t i = 0; i < nu; ++i) if (__builtin_popcount(um[(size_t)i]) >= k) want.push_back(uk[(size_t)i]);
    std::sort(want.begin(), want.end());
  }
  // lines: the first kept line of every key in the lowest-numbered member that carries it
  std::unordered_map<uint32_t, std::pair<int, int64_t>> first;   // key -> (member, line)
  for (size_t mi = 0; mi < m.size(); ++mi) {
    const JobState& s = c.J[(size_t)m[mi]];
    std::vector<uint64_t> kept((size_t)(s.n_data + 63) / 64 + 1), tpm(kept.size());
    rc = qm_batch_get_masks(c.batch, s.batch_v, kept.data(), tpm.data());
    if (rc != QM_OK) return c.lib(rc, err);
    int64_t rec = 0;
    for (int64_t i = 0; i < s.info.n_lines; ++i) {
      if (is_header(s.line_kind[(size_t)i])) continue;
      const int64_t r = rec++;
      if (!((kept[(size_t)r >> 6] >> (r & 63)) & 1ull) || (s.flags[r] & QM_F_NOKEY) || (uint32_t)(s.ref[r] | s.alt[r]) >= 4u) continue;
      first.emplace(((uint32_t)s.pos[r] << 4) | ((uint32_t)s.ref[r] << 2) | (uint32_t)s.alt[r], std::make_pair((int)mi, i));
    }
  }
  std::string out;
  auto put = [&](const JobState& s, int64_t i) {
    const int64_t a = s.line_off[(size_t)i], b = (i + 1 < s.info.n_lines) ? s.line_off[(size_t)i + 1] : (int64_t)s.vcf.n;
    out.append((const char*)s.vcf.p + a, (size_t)(b - a));
    if (out.empty() || out.back() != '\n') out.push_back('\n');
  };
  const JobState& s0 = c.J[(size_t)m[0]];
  for (int64_t i = 0; i < s0.info.n_lines; ++i) if (is_header(s0.line_kind[(size_t)i])) put(s0, i);
  for (int64_t i = 0; i < s0.info.n_lines; ++i)   // '#' lines the filter keeps stand among the kept lines of the filtered file once more
    if (s0.line_kind[(size_t)i] == QM_LINE_HEADER_KEPT || s0.line_kind[(size_t)i] == QM_LINE_HEADER_KEPT_TP) put(s0, i);
  for (uint32_t key : want) {
    const auto it = first.find(key);
    if (it == first.end()) { err = std::string(path) + ": key " + std::to_string(key) + " has votes and no kept line"; return QM_E_STATE; }
    put(c.J[(size_t)m[(size_t)it->second.first]], it->second.second);
  }
  rc = write_all_atomic(path, out);
  if (rc != QM_OK) err = std::string("cannot write ") + path;
  return rc;
}

// the vote tables of every group, and the consensus VCF of the groups that name a level
int votes_pass(const PassCtx& c, const qm_votes_args* va, std::string& err) {
  if (!va || va->n_groups <= 0) return QM_OK;
  for (int j = 0; j < c.n_jobs; ++j)
    if (va->group[j] >= 0 && c.J[(size_t)j].info.n_nokey_kept) return refuse_nokey(c.jobs[j].vcf_path, c.J[(size_t)j], "the vote pass", err);
  const GroupTables G = group_tables(c, va->group, va->n_groups);
  int rc = qm_batch_truth_hits(c.batch, nullptr);
  if (rc == QM_OK) rc = qm_batch_votes(c.batch, va->n_groups, G.goff.data(), G.gids.data(), nullptr);
  if (rc == QM_OK) rc = qm_batch_get_votes(c.batch, va->tp_votes, va->fp_votes, va->private_tp, va->private_fp, nullptr);
  if (rc != QM_OK) return c.lib(rc, err);
  for (int g = 0; g < va->n_groups && rc == QM_OK; ++g) {
    const int k = va->consensus_k ? va->consensus_k[g] : 0;
    if (k > 0) rc = write_consensus(c, g, G.members[(size_t)g], k, va->consensus_out[g], err);
  }
  return rc;
}

// ---- why a line is FP and a truth key FN ----
// `#line POS REF ALT QUAL class`, then one row per FP line of the job in file order: the 1-based line number, the line's own
// text of the four columns, the class of its record (rcls: one byte per record)
int write_fp_why_file(const char* path, const JobState& s, const uint8_t* rcls) {
  std::string out = "#line\tPOS\tREF\tALT\tQUAL\tclass\n";
  const uint8_t* text = s.vcf.p;
  const size_t len = s.vcf.n;
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    const int64_t r = rec++;
    if (rcls[r] >= QM_NM_R_CLASSES) continue;
    size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], len);
    if (e > b && text[e - 1] == '\n') --e;
    const uint8_t* f[6]; size_t fl[6]; int nf = 0;
    const uint8_t* q = text + b;
    while (nf < 6) {
      const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(text + e - q));
      f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(text + e - q); ++nf;
      if (!tb) break;
      q = tb + 1;
    }
    out.append(std::to_string(i + 1));
    for (int k : {1, 3, 4, 5}) { out.push_back('\t'); if (k < nf) out.append((const char*)f[k], fl[k]); }
    out.push_back('\t');
    out.append(NM_R_NAMES[rcls[r]]);
    out.push_back('\n');
  }
  return write_all_atomic(path, out);
}

// the class counts of every wanted job, and the why-files of the jobs that name them
int nearmiss_pass(const PassCtx& c, const qm_nearmiss_args* nm, std::string& err) {
  auto want = [&](int j) { return !c.jobs[j].pure && nm->want[j] != 0; };
  if (!nm || !c.any(want)) return QM_OK;
  auto fp_path = [&](int j) { return want(j) && nm->fp_why_out ? nm->fp_why_out[j] : nullptr; };
  auto fn_path = [&](int j) { return want(j) && nm->fn_why_out ? nm->fn_why_out[j] : nullptr; };
  for (int j = 0; j < c.n_jobs; ++j)
    if (fn_path(j) && c.J[(size_t)j].info.n_nokey_kept) return refuse_nokey(c.jobs[j].vcf_path, c.J[(size_t)j], "the explanation of the missed keys", err);
  std::vector<uint64_t> rec(c.nv * QM_NM_R_CLASSES), tru(c.nv * QM_NM_T_CLASSES);
  int rc = qm_batch_truth_hits(c.batch, nullptr);
  if (rc == QM_OK) rc = qm_batch_nearmiss(c.batch, nm->radius, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_nearmiss(c.batch, rec.data(), tru.data());
  if (rc == QM_OK) { c.scatter_rows(nm->rec, rec, QM_NM_R_CLASSES, want); c.scatter_rows(nm->tru, tru, QM_NM_T_CLASSES, want); }
  struct WhyTask { int j; bool fn; std::vector<uint8_t> cls; std::vector<uint32_t> bits; };
  std::vector<WhyTask> W;
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    const JobState& s = c.J[(size_t)j];
    if (fp_path(j)) {
      W.push_back({j, false, std::vector<uint8_t>((size_t)s.n_data + 1, (uint8_t)QM_NM_NONE), {}});
      rc = qm_batch_get_nearmiss_cls(c.batch, s.batch_v, W.back().cls.data());
    }
    if (fn_path(j) && rc == QM_OK) {
      const size_t tn = c.truth_of(j).keys.size();
      W.push_back({j, true, std::vector<uint8_t>(tn + 1, (uint8_t)QM_NM_NONE), std::vector<uint32_t>((tn + 31) / 32 + 1, 0u)});
      rc = qm_batch_get_nearmiss_truth(c.batch, s.batch_v, W.back().cls.data());
      if (rc == QM_OK) rc = qm_batch_get_truth_hits(c.batch, s.batch_v, W.back().bits.data(), (int64_t)((tn + 31) / 32));
    }
  }
  if (rc != QM_OK) return c.lib(rc, err);
  std::vector<int> wrc(W.size(), QM_OK);
  parallel_for((int)W.size(), c.nthr, [&](int k) {
    const WhyTask& w = W[(size_t)k];
    wrc[(size_t)k] = w.fn ? write_fn_why_file(nm->fn_why_out[w.j], c.truth_of(w.j), w.bits.data(), w.cls.data())
                          : write_fp_why_file(nm->fp_why_out[w.j], c.J[(size_t)w.j], w.cls.data());
  });
  for (size_t k = 0; k < W.size(); ++k)
    if (wrc[k] != QM_OK) { err = std::string("cannot write ") + (W[k].fn ? nm->fn_why_out : nm->fp_why_out)[W[k].j]; return wrc[k]; }
  return QM_OK;
}

// ---- indels and MNPs matched by normal form ----
// the spelling of an inline allele code (include/qmvt.h), `.` for any other code
std::string nz_spell(int32_t c) {
  const uint32_t u = (uint32_t)c;
  if (!(u < 4u || (u >= (2u << 26) && u < (14u << 26)))) return ".";
  const uint32_t n = u < 4u ? 1u : u >> 26;
  std::string out;
  for (uint32_t k = 0; k < n; ++k) out.push_back("ACGT"[(u >> (2 * k)) & 3u]);
  return out;
}
struct NzColumns { std::vector<int32_t> pos, ref, alt, row; std::vector<uint8_t> cls; };
struct NzEntries { std::vector<int32_t> pos, ref, alt; };
// `#line POS REF ALT NORM_POS NORM_REF NORM_ALT TRUTH_POS TRUTH_REF TRUTH_ALT`, then one row per rescued line of the job in file
// order: the 1-based line number, the line's own text of the three columns, the record's normal form, the truth entry of the
// smallest index with that form
int write_rescued_file(const char* path, const JobState& s, const NzColumns& c, const NzEntries& t) {
  std::string out = "#line\tPOS\tREF\tALT\tNORM_POS\tNORM_REF\tNORM_ALT\tTRUTH_POS\tTRUTH_REF\tTRUTH_ALT\n";
  const uint8_t* text = s.vcf.p;
  const size_t len = s.vcf.n;
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    const int64_t r = rec++;
    if (c.cls[(size_t)r] != QM_NORM_C_RESCUED) continue;
    size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], len);
    if (e > b && text[e - 1] == '\n') --e;
    const uint8_t* f[6]; size_t fl[6]; int nf = 0;
    const uint8_t* q = text + b;
    while (nf < 6) {
      const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(text + e - q));
      f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(text + e - q); ++nf;
      if (!tb) break;
      q = tb + 1;
    }
    out.append(std::to_string(i + 1));
    for (int k : {1, 3, 4}) { out.push_back('\t'); if (k < nf) out.append((const char*)f[k], fl[k]); }
    out += "\t" + std::to_string(c.pos[(size_t)r]) + "\t" + nz_spell(c.ref[(size_t)r]) + "\t" + nz_spell(c.alt[(size_t)r]);
    const int64_t k = c.row[(size_t)r];
    if (k >= 0 && (size_t)k < t.pos.size()) out += "\t" + std::to_string(t.pos[(size_t)k]) + "\t" + nz_spell(t.ref[(size_t)k]) + "\t" + nz_spell(t.alt[(size_t)k]);
    else out += "\t.\t.\t.";   // (a line the text side made a TP line: no truth entry carries its form)
    out.push_back('\n');
  }
  return write_all_atomic(path, out);
}

// the counts of every wanted job, and the rescued-lines files of the jobs that name one
int normalize_pass(const PassCtx& c, const Passes& P, std::string& err) {
  const qm_normalize_args* na = P.nz;
  auto want = [&](int j) { return !c.jobs[j].pure && na->genome_id[j] >= 0; };
  if (!na || !c.any(want)) return QM_OK;
  auto path = [&](int j) { return want(j) && na->rescued_out ? na->rescued_out[j] : nullptr; };
  std::vector<int32_t> gid(c.nv, -1);
  bool files = false;
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) { gid[(size_t)c.J[(size_t)j].batch_v] = na->genome_id[j]; files = files || path(j); }
  std::vector<uint64_t> rec(c.nv * QM_NORM_R_COLS), tru(c.nv * QM_NORM_T_COLS);
  int rc = qm_batch_normalize(c.batch, gid.data(), files ? QM_NORM_COLUMNS : 0u, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_normalize(c.batch, rec.data(), tru.data());
  if (rc == QM_OK) { c.scatter_rows(na->rec, rec, QM_NORM_R_COLS, want); c.scatter_rows(na->tru, tru, QM_NORM_T_COLS, want); }
  struct Task { int j; NzColumns cols; };
  std::vector<Task> W;
  std::vector<NzEntries> ent(c.T.size());
  std::vector<uint8_t> have(c.T.size(), 0);
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    if (!path(j)) continue;
    const JobState& s = c.J[(size_t)j];
    const size_t n = (size_t)s.n_data + 1;
    W.push_back({j, NzColumns{std::vector<int32_t>(n), std::vector<int32_t>(n), std::vector<int32_t>(n), std::vector<int32_t>(n, -1), std::vector<uint8_t>(n, 0)}});
    NzColumns& k = W.back().cols;
    rc = qm_batch_get_normalized(c.batch, s.batch_v, k.pos.data(), k.ref.data(), k.alt.data(), k.cls.data(), k.row.data());
    if (rc == QM_OK && !have[(size_t)s.truth]) {
      NzEntries& e = ent[(size_t)s.truth];
      int64_t tn = 0;
      (void)qm_truth_entries(c.ctx, c.truth_of(j).tid, nullptr, nullptr, nullptr, 0, &tn);   // (how many)
      e.pos.resize((size_t)tn + 1); e.ref.resize((size_t)tn + 1); e.alt.resize((size_t)tn + 1);
      rc = qm_truth_entries(c.ctx, c.truth_of(j).tid, e.pos.data(), e.ref.data(), e.alt.data(), tn, &tn);
      e.pos.resize((size_t)tn); e.ref.resize((size_t)tn); e.alt.resize((size_t)tn);
      have[(size_t)s.truth] = 1;
    }
  }
  if (rc != QM_OK) return c.lib(rc, err);
  std::vector<int> wrc(W.size(), QM_OK);
  parallel_for((int)W.size(), c.nthr, [&](int k) {
    const Task& w = W[(size_t)k];
    wrc[(size_t)k] = write_rescued_file(na->rescued_out[w.j], c.J[(size_t)w.j], w.cols, ent[(size_t)c.J[(size_t)w.j].truth]);
  });
  for (size_t k = 0; k < W.size(); ++k)
    if (wrc[k] != QM_OK) { err = std::string("cannot write ") + na->rescued_out[W[k].j]; return wrc[k]; }
  return QM_OK;
}

// ---- MNPs matched against adjacent SNVs ----
struct AtColumns { std::vector<uint8_t> cls, na; std::vector<uint16_t> hm; std::vector<uint64_t> kept; };
// `#line POS REF ALT N_ATOMS N_HIT HIT_MASK CLASS`, then one row per kept atomisable line of the job with at least 2 atoms in file
// order: the 1-based line number, the line's own text of the three columns, the atom and hit counts, the hit mask in hexadecimal
// and the class name
int write_atoms_file(const char* path, const JobState& s, const AtColumns& c) {
  static const char* const names[] = {"full", "partial", "none", "rescued", "long", "nokey", "novar", "unequal", "range"};
  std::string out = "#line\tPOS\tREF\tALT\tN_ATOMS\tN_HIT\tHIT_MASK\tCLASS\n";
  const uint8_t* text = s.vcf.p;
  const size_t len = s.vcf.n;
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    const int64_t r = rec++;
    if (c.na[(size_t)r] < 2 || !((c.kept[(size_t)r >> 6] >> (r & 63)) & 1ull)) continue;
    size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], len);
    if (e > b && text[e - 1] == '\n') --e;
    const uint8_t* f[6]; size_t fl[6]; int nf = 0;
    const uint8_t* q = text + b;
    while (nf < 6) {
      const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(text + e - q));
      f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(text + e - q); ++nf;
      if (!tb) break;
      q = tb + 1;
    }
    out.append(std::to_string(i + 1));
    for (int k : {1, 3, 4}) { out.push_back('\t'); if (k < nf) out.append((const char*)f[k], fl[k]); }
    char hex[16];
    snprintf(hex, sizeof hex, "0x%04x", (unsigned)c.hm[(size_t)r]);
    out += "\t" + std::to_string((int)c.na[(size_t)r]) + "\t" + std::to_string(__builtin_popcount((unsigned)c.hm[(size_t)r])) + "\t" + hex + "\t" +
           names[std::min<size_t>(c.cls[(size_t)r], 8)];
    out.push_back('\n');
  }
  return write_all_atomic(path, out);
}

// the counts of every wanted job, and the atoms files of the jobs that name one
int atomize_pass(const PassCtx& c, const Passes& P, std::string& err) {
  const qm_atomize_args* at = P.at;
  auto want = [&](int j) { return P.wants_atomize(j); };
  if (!at || !c.any(want)) return QM_OK;
  auto path = [&](int j) { return want(j) && at->atoms_out ? at->atoms_out[j] : nullptr; };
  bool files = false;
  for (int j = 0; j < c.n_jobs; ++j) files = files || path(j);
  std::vector<uint64_t> rec(c.nv * QM_ATOM_R_COLS), tru(c.nv * QM_ATOM_T_COLS);
  int rc = qm_batch_atomize(c.batch, files ? QM_ATOM_COLUMNS : 0u, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_atomize(c.batch, rec.data(), tru.data());
  if (rc == QM_OK) { c.scatter_rows(at->rec, rec, QM_ATOM_R_COLS, want); c.scatter_rows(at->tru, tru, QM_ATOM_T_COLS, want); }
  struct Task { int j; AtColumns cols; };
  std::vector<Task> W;
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    if (!path(j)) continue;
    const JobState& s = c.J[(size_t)j];
    const size_t n = (size_t)s.n_data + 1;
    W.push_back({j, AtColumns{std::vector<uint8_t>(n, 0), std::vector<uint8_t>(n, 0), std::vector<uint16_t>(n, 0), std::vector<uint64_t>(n / 64 + 2, 0)}});
    AtColumns& k = W.back().cols;
    std::vector<uint64_t> tpm(k.kept.size());
    rc = qm_batch_get_atomized(c.batch, s.batch_v, k.cls.data(), k.na.data(), k.hm.data());
    if (rc == QM_OK) rc = qm_batch_get_masks(c.batch, s.batch_v, k.kept.data(), tpm.data());
  }
  if (rc != QM_OK) return c.lib(rc, err);
  std::vector<int> wrc(W.size(), QM_OK);
  parallel_for((int)W.size(), c.nthr, [&](int k) {
    const Task& w = W[(size_t)k];
    wrc[(size_t)k] = write_atoms_file(at->atoms_out[w.j], c.J[(size_t)w.j], w.cols);
  });
  for (size_t k = 0; k < W.size(); ++k)
    if (wrc[k] != QM_OK) { err = std::string("cannot write ") + at->atoms_out[W[k].j]; return wrc[k]; }
  return QM_OK;
}

// TP, FP and FN by variant type and size: the shape table from the call's dictionary, the rows of every wanted
// mixed-sample job (a pure-strain job has no truth set to be measured against: its rows stay zero)
int types_pass(const PassCtx& c, const qm_types_args* ty, std::string& err) {
  if (!ty) return QM_OK;
  auto want = [&](int j) { return ty->want[j] != 0 && !c.jobs[j].pure; };
  if (!c.any(want)) return QM_OK;
  const int64_t ns = c.dict ? qm_dict_size(c.dict) : 0;
  std::vector<int32_t> len((size_t)ns);
  std::vector<uint32_t> head((size_t)ns), tail((size_t)ns);
  const int64_t got = ns ? qm_dict_shapes(c.dict, 0, ns, len.data(), head.data(), tail.data()) : 0;
  const size_t w = 2 * (size_t)(5 * ty->n_bins + 4);
  std::vector<uint64_t> rec(c.nv * w), tru(c.nv * w);
  int rc = qm_batch_types(c.batch, ty->edges, ty->n_bins, len.data(), head.data(), tail.data(), got, 0u, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_types(c.batch, rec.data(), tru.data());
  if (rc != QM_OK) return c.lib(rc, err);
  c.scatter_rows(ty->rec, rec, w, want);
  c.scatter_rows(ty->tru, tru, w, want);
  return QM_OK;
}

// The QUAL ROC under normal-form and atom matching: the two producer passes with their columns, run here as the
// batch calls they are -- none of their rows or files is handed out --, then the sweep; the rows of every wanted mixed-sample job
// (a pure-strain job has no truth set to be measured against: its rows stay zero)
int rroc_pass(const PassCtx& c, const qm_rescue_roc_args* rr, int n_bins, std::string& err) {
  if (!rr) return QM_OK;
  auto want = [&](int j) { return rr->want[j] != 0 && !c.jobs[j].pure; };
  if (!c.any(want)) return QM_OK;
  std::vector<int32_t> gid(c.nv, -1);
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) gid[(size_t)c.J[(size_t)j].batch_v] = rr->genome_id[j];
  const size_t w = 3 * (size_t)n_bins;
  std::vector<uint64_t> rn(c.nv * w), ra(c.nv * w), base(c.nv * 2);
  int rc = qm_batch_normalize(c.batch, gid.data(), QM_NORM_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_atomize(c.batch, QM_ATOM_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_rescue_roc(c.batch, QM_RROC_NORM | QM_RROC_ATOM, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_rescue_roc(c.batch, rn.data(), ra.data(), base.data());
  if (rc != QM_OK) return c.lib(rc, err);
  c.scatter_rows(rr->roc_n, rn, w, want);
  c.scatter_rows(rr->roc_a, ra, w, want);
  c.scatter_rows(rr->base, base, 2, want);
  return QM_OK;
}

// ---- the four rescues combined ----
struct LdColumns { std::vector<uint8_t> mask, emask; };
std::string ld_set_name(unsigned m) {
  std::string out;
  for (int k = 0; k < 4; ++k)
    if ((m >> k) & 1u) { if (!out.empty()) out.push_back('+'); out.push_back("NAHB"[k]); }
  return out.empty() ? "none" : out;
}
const char* ld_tier(unsigned m) {
  static const char* const names[] = {"normalized", "atomized", "haplotype", "subset"};
  for (int k = 0; k < 4; ++k)
    if ((m >> k) & 1u) return names[k];
  return "none";
}
// `#kind line POS REF ALT METHODS TIER`: every kept line of the job that is no TP line, in file order, then every truth entry no
// kept record spells, in table order (quasimodo_amd.ladder.job_rows)
int write_ladder_file(const char* path, const JobState& s, const LdColumns& c, const NzEntries& t) {
  std::string out = "#kind\tline\tPOS\tREF\tALT\tMETHODS\tTIER\n";
  const uint8_t* text = s.vcf.p;
  const size_t len = s.vcf.n;
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    const int64_t r = rec++;
    const unsigned m = c.mask[(size_t)r];
    if (!(m & QM_LADDER_M_K) || (m & QM_LADDER_M_S)) continue;
    size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], len);
    if (e > b && text[e - 1] == '\n') --e;
    const uint8_t* f[6]; size_t fl[6]; int nf = 0;
    const uint8_t* q = text + b;
    while (nf < 6) {
      const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(text + e - q));
      f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(text + e - q); ++nf;
      if (!tb) break;
      q = tb + 1;
    }
    out += "line\t" + std::to_string(i + 1);
    for (int k : {1, 3, 4}) { out.push_back('\t'); if (k < nf) out.append((const char*)f[k], fl[k]); }
    out += "\t" + ld_set_name(m & 15u) + "\t" + ld_tier(m & 15u) + "\n";
  }
  for (size_t j = 0; j < t.pos.size() && j < c.emask.size(); ++j) {
    const unsigned m = c.emask[j];
    if (m & QM_LADDER_M_S) continue;
    out += "entry\t.\t" + std::to_string(t.pos[j]) + "\t" + nz_spell(t.ref[j]) + "\t" + nz_spell(t.alt[j]) + "\t" + ld_set_name(m & 15u) + "\t" +
           ld_tier(m & 15u) + "\n";
  }
  return write_all_atomic(path, out);
}

// The four producer passes with their columns, run here as the batch calls they are -- none of their rows or files is handed out
// --, then the ladder; the rows of every wanted mixed-sample job (a pure-strain job has no truth set to be measured against: its
// rows stay zero) and the ladder files of the jobs that name one
int ladder_pass(const PassCtx& c, const qm_ladder_args* la, std::string& err) {
  if (!la) return QM_OK;
  auto want = [&](int j) { return la->want[j] != 0 && !c.jobs[j].pure; };
  if (!c.any(want)) return QM_OK;
  auto path = [&](int j) { return want(j) && la->ladder_out ? la->ladder_out[j] : nullptr; };
  std::vector<int32_t> gid(c.nv, -1);
  bool files = false;
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) { gid[(size_t)c.J[(size_t)j].batch_v] = la->genome_id[j]; files = files || path(j); }
  const unsigned what = (la->subsets ? QM_LADDER_SUBSETS : 0u) | (files ? QM_LADDER_COLUMNS : 0u);
  std::vector<uint64_t> rec(c.nv * QM_LADDER_COLS), tru(c.nv * QM_LADDER_COLS);
  int rc = qm_batch_normalize(c.batch, gid.data(), QM_NORM_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_atomize(c.batch, QM_ATOM_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_haplotypes(c.batch, gid.data(), la->gap, QM_HAP_COLUMNS, nullptr);
  if (rc == QM_OK && la->subsets) rc = qm_batch_hapsubsets(c.batch, QM_HAPSUB_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_ladder(c.batch, what, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_ladder(c.batch, rec.data(), tru.data());
  if (rc != QM_OK) return c.lib(rc, err);
  c.scatter_rows(la->rec, rec, QM_LADDER_COLS, want);
  c.scatter_rows(la->tru, tru, QM_LADDER_COLS, want);
  struct Task { int j; LdColumns cols; };
  std::vector<Task> W;
  std::vector<NzEntries> ent(c.T.size());
  std::vector<uint8_t> have(c.T.size(), 0);
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    if (!path(j)) continue;
    const JobState& s = c.J[(size_t)j];
    if (!have[(size_t)s.truth]) {
      NzEntries& e = ent[(size_t)s.truth];
      int64_t tn = 0;
      (void)qm_truth_entries(c.ctx, c.truth_of(j).tid, nullptr, nullptr, nullptr, 0, &tn);   // (how many)
      e.pos.resize((size_t)tn + 1); e.ref.resize((size_t)tn + 1); e.alt.resize((size_t)tn + 1);
      rc = qm_truth_entries(c.ctx, c.truth_of(j).tid, e.pos.data(), e.ref.data(), e.alt.data(), tn, &tn);
      e.pos.resize((size_t)tn); e.ref.resize((size_t)tn); e.alt.resize((size_t)tn);
      have[(size_t)s.truth] = 1;
    }
    if (rc != QM_OK) break;
    W.push_back({j, LdColumns{std::vector<uint8_t>((size_t)s.n_data + 1, 0), std::vector<uint8_t>(ent[(size_t)s.truth].pos.size() + 1, 0)}});
    rc = qm_batch_get_laddered(c.batch, s.batch_v, W.back().cols.mask.data(), W.back().cols.emask.data());
    W.back().cols.emask.resize(ent[(size_t)s.truth].pos.size());
  }
  if (rc != QM_OK) return c.lib(rc, err);
  std::vector<int> wrc(W.size(), QM_OK);
  parallel_for((int)W.size(), c.nthr, [&](int k) {
    const Task& w = W[(size_t)k];
    wrc[(size_t)k] = write_ladder_file(la->ladder_out[w.j], c.J[(size_t)w.j], w.cols, ent[(size_t)c.J[(size_t)w.j].truth]);
  });
  for (size_t k = 0; k < W.size(); ++k)
    if (wrc[k] != QM_OK) { err = std::string("cannot write ") + la->ladder_out[W[k].j]; return wrc[k]; }
  return QM_OK;
}

// The match ladder per variant type and size: the four rescues with their columns, the type pass with its row
// bytes (the shape table from the call's dictionary, so no long allele is without a row) and the ladder with its mask bytes, run
// here as the batch calls they are -- none of their rows or files is handed out --, then the cross; the blocks of every wanted
// mixed-sample job (a pure-strain job has no truth set to be measured against: its rows stay zero)
int ltypes_pass(const PassCtx& c, const qm_ladder_types_args* lt, std::string& err) {
  if (!lt) return QM_OK;
  auto want = [&](int j) { return lt->want[j] != 0 && !c.jobs[j].pure; };
  if (!c.any(want)) return QM_OK;
  std::vector<int32_t> gid(c.nv, -1);
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) gid[(size_t)c.J[(size_t)j].batch_v] = lt->genome_id[j];
  const int64_t ns = c.dict ? qm_dict_size(c.dict) : 0;
  std::vector<int32_t> len((size_t)ns);
  std::vector<uint32_t> head((size_t)ns), tail((size_t)ns);
  const int64_t got = ns ? qm_dict_shapes(c.dict, 0, ns, len.data(), head.data(), tail.data()) : 0;
  const size_t w = (size_t)(5 * lt->n_bins + 4) * QM_LADDER_COLS;
  std::vector<uint64_t> rec(c.nv * w), tru(c.nv * w);
  int rc = qm_batch_normalize(c.batch, gid.data(), QM_NORM_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_atomize(c.batch, QM_ATOM_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_haplotypes(c.batch, gid.data(), lt->gap, QM_HAP_COLUMNS, nullptr);
  if (rc == QM_OK && lt->subsets) rc = qm_batch_hapsubsets(c.batch, QM_HAPSUB_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_types(c.batch, lt->edges, lt->n_bins, len.data(), head.data(), tail.data(), got, QM_TYPE_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_ladder(c.batch, (lt->subsets ? QM_LADDER_SUBSETS : 0u) | QM_LADDER_COLUMNS, nullptr);
  if (rc == QM_OK) rc = qm_batch_ladder_types(c.batch, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_ladder_types(c.batch, rec.data(), tru.data(), nullptr);
  if (rc != QM_OK) return c.lib(rc, err);
  c.scatter_rows(lt->rec, rec, w, want);
  c.scatter_rows(lt->tru, tru, w, want);
  return QM_OK;
}

// ---- clusters of records matched by replayed haplotype ----
struct HpColumns { std::vector<uint8_t> cls, ecls; std::vector<int32_t> site; };
struct HpSites { std::vector<int32_t> first, lo, hi; };
// the trimmed form of two different strings over ACGT: the common prefix goes first, then the common suffix of what is left
struct HpForm { int64_t q; std::string r, a; };
HpForm hp_trim(int64_t p, const std::string& R, const std::string& A) {
  const size_t m = std::min(R.size(), A.size());
  size_t cp = 0, cs = 0;
  while (cp < m && R[cp] == A[cp]) ++cp;
  while (cs < m - cp && R[R.size() - 1 - cs] == A[A.size() - 1 - cs]) ++cs;
  return HpForm{p + (int64_t)cp, R.substr(cp, R.size() - cp - cs), A.substr(cp, A.size() - cp - cs)};
}
// the window [ws, we] of the genome with the variants of one side substituted (identical spellings collapsed, sorted by (q, |r|):
// the site is a MATCH one, so they do not conflict)
std::string hp_replay(const uint8_t* seq, int64_t len, int64_t ws, int64_t we, std::vector<HpForm> v) {
  std::sort(v.begin(), v.end(), [](const HpForm& x, const HpForm& y) { return x.q != y.q ? x.q < y.q : x.r.size() != y.r.size() ? x.r.size() < y.r.size() : x.a < y.a; });
  v.erase(std::unique(v.begin(), v.end(), [](const HpForm& x, const HpForm& y) { return x.q == y.q && x.r == y.r && x.a == y.a; }), v.end());
  std::string out;
  auto genome = [&](int64_t from, int64_t to) {   // G[from .. to]
    for (int64_t q = std::max<int64_t>(from, 1); q <= std::min(to, len); ++q) {
      const char ch = (char)(seq[q - 1] & ~0x20);
      out.push_back(ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' ? ch : 'N');
    }
  };
  int64_t cur = ws;
  for (const HpForm& f : v) { genome(cur, f.q - 1); out += f.a; cur = f.q + (int64_t)f.r.size(); }
  genome(cur, we);
  return out;
}
// `#site WIN_LO WIN_HI LINES ENTRIES REPLAY_LINES REPLAY_TRUTH`, one row per MATCH site of the job in site order
int write_sites_file(const char* path, const JobState& s, const HpColumns& c, const NzEntries& t, const HpSites& st, const uint8_t* seq, int64_t len) {
  std::string out = "#site\tWIN_LO\tWIN_HI\tLINES\tENTRIES\tREPLAY_LINES\tREPLAY_TRUTH\n";
  const uint8_t* text = s.vcf.p;
  const size_t tlen = s.vcf.n;
  const size_t ns = st.first.size();
  std::vector<std::string> lines(ns);
  std::vector<std::vector<HpForm>> side(ns);
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    const int64_t r = rec++;
    if (c.cls[(size_t)r] != QM_HAP_C_RESCUED) continue;
    const int32_t k = c.site[(size_t)r];
    if (k < 0 || (size_t)k >= ns) continue;
    size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], tlen);
    if (e > b && text[e - 1] == '\n') --e;
    const uint8_t* f[6]; size_t fl[6]; int nf = 0;
    const uint8_t* q = text + b;
    while (nf < 6) {
      const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(text + e - q));
      f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(text + e - q); ++nf;
      if (!tb) break;
      q = tb + 1;
    }
    if (nf < 5) continue;
    std::string& L = lines[(size_t)k];
    if (!L.empty()) L.push_back(';');
    L += std::to_string(i + 1);
    for (int x : {1, 3, 4}) { L.push_back(':'); L.append((const char*)f[x], fl[x]); }
    side[(size_t)k].push_back(hp_trim(s.pos[r], nz_spell(s.ref[r]), nz_spell(s.alt[r])));
  }
  for (size_t k = 0; k < ns; ++k) {
    if (lines[k].empty()) continue;
    const size_t e0 = (size_t)st.first[k], e1 = k + 1 < ns ? (size_t)st.first[k + 1] : t.pos.size();
    std::string ents;
    std::vector<HpForm> tside;
    for (size_t j = e0; j < e1; ++j) {
      if (c.ecls[j] != QM_HAP_C_RESCUED) continue;
      if (!ents.empty()) ents.push_back(';');
      ents += std::to_string(t.pos[j]) + ":" + nz_spell(t.ref[j]) + ":" + nz_spell(t.alt[j]);
      tside.push_back(hp_trim(t.pos[j], nz_spell(t.ref[j]), nz_spell(t.alt[j])));
    }
    out += std::to_string(k) + "\t" + std::to_string(st.lo[k]) + "\t" + std::to_string(st.hi[k]) + "\t" + lines[k] + "\t" + ents + "\t" +
           hp_replay(seq, len, st.lo[k], st.hi[k], side[k]) + "\t" + hp_replay(seq, len, st.lo[k], st.hi[k], tside) + "\n";
  }
  return write_all_atomic(path, out);
}

// the counts of every wanted job, and the sites files of the jobs that name one
int haplo_pass(const PassCtx& c, const qm_haplotypes_args* ha, std::string& err, bool columns = false) {
  if (!ha) return QM_OK;
  auto want = [&](int j) { return !c.jobs[j].pure && ha->genome_id[j] >= 0; };
  if (!c.any(want)) return QM_OK;
  auto path = [&](int j) { return want(j) && ha->sites_out ? ha->sites_out[j] : nullptr; };
  std::vector<int32_t> gid(c.nv, -1);
  bool files = columns;   // (the subset search behind this pass asks for the columns too)
  for (int j = 0; j < c.n_jobs; ++j) if (want(j)) { gid[(size_t)c.J[(size_t)j].batch_v] = ha->genome_id[j]; files = files || path(j); }
  std::vector<uint64_t> rec(c.nv * QM_HAP_R_COLS), tru(c.nv * QM_HAP_T_COLS);
  int rc = qm_batch_haplotypes(c.batch, gid.data(), ha->gap, files ? QM_HAP_COLUMNS : 0u, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_haplotypes(c.batch, rec.data(), tru.data());
  if (rc == QM_OK) { c.scatter_rows(ha->rec, rec, QM_HAP_R_COLS, want); c.scatter_rows(ha->tru, tru, QM_HAP_T_COLS, want); }
  struct Task { int j; HpColumns cols; };
  std::vector<Task> W;
  std::vector<NzEntries> ent(c.T.size());
  std::vector<HpSites> sites(c.T.size());
  std::vector<uint8_t> have(c.T.size(), 0);
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    if (!path(j)) continue;
    const JobState& s = c.J[(size_t)j];
    const size_t n = (size_t)s.n_data + 1;
    if (!have[(size_t)s.truth]) {
      NzEntries& e = ent[(size_t)s.truth];
      HpSites& st = sites[(size_t)s.truth];
      int64_t tn = 0, sn = 0;
      (void)qm_truth_entries(c.ctx, c.truth_of(j).tid, nullptr, nullptr, nullptr, 0, &tn);   // (how many)
      e.pos.resize((size_t)tn + 1); e.ref.resize((size_t)tn + 1); e.alt.resize((size_t)tn + 1);
      rc = qm_truth_entries(c.ctx, c.truth_of(j).tid, e.pos.data(), e.ref.data(), e.alt.data(), tn, &tn);
      e.pos.resize((size_t)tn); e.ref.resize((size_t)tn); e.alt.resize((size_t)tn);
      st.first.resize((size_t)tn + 1); st.lo.resize((size_t)tn + 1); st.hi.resize((size_t)tn + 1);
      if (rc == QM_OK) rc = qm_truth_sites(c.ctx, c.truth_of(j).tid, ha->genome_id[j], ha->gap, st.first.data(), st.lo.data(), st.hi.data(), tn + 1, &sn);
      st.first.resize((size_t)sn); st.lo.resize((size_t)sn); st.hi.resize((size_t)sn);
      have[(size_t)s.truth] = 1;
    }
    if (rc != QM_OK) break;
    W.push_back({j, HpColumns{std::vector<uint8_t>(n, 0), std::vector<uint8_t>(ent[(size_t)s.truth].pos.size() + 1, 0), std::vector<int32_t>(n, -1)}});
    HpColumns& k = W.back().cols;
    rc = qm_batch_get_haplotyped(c.batch, s.batch_v, k.cls.data(), k.site.data(), k.ecls.data());
  }
  if (rc != QM_OK) return c.lib(rc, err);
  std::vector<int> wrc(W.size(), QM_OK);
  parallel_for((int)W.size(), c.nthr, [&](int k) {
    const Task& w = W[(size_t)k];
    const size_t t = (size_t)c.J[(size_t)w.j].truth;
    wrc[(size_t)k] = write_sites_file(ha->sites_out[w.j], c.J[(size_t)w.j], w.cols, ent[t], sites[t], ha->genome_seq[w.j], ha->genome_len[w.j]);
  });
  for (size_t k = 0; k < W.size(); ++k)
    if (wrc[k] != QM_OK) { err = std::string("cannot write ") + ha->sites_out[W[k].j]; return wrc[k]; }
  return QM_OK;
}

// ---- a subset search inside the mismatched sites of the haplotype pass ----
// `line:POS:REF:ALT` of data line i (1-based line number, the line's own text of the three columns) appended to L; false: no such columns
bool hs_line_text(const JobState& s, int64_t i, std::string& L) {
  const uint8_t* text = s.vcf.p;
  const size_t tlen = s.vcf.n;
  size_t b = (size_t)s.line_off[(size_t)i], e = std::min((size_t)s.line_off[(size_t)i + 1], tlen);
  if (e > b && text[e - 1] == '\n') --e;
  const uint8_t* f[6]; size_t fl[6]; int nf = 0;
  const uint8_t* q = text + b;
  while (nf < 6) {
    const uint8_t* tb = (const uint8_t*)memchr(q, '\t', (size_t)(text + e - q));
    f[nf] = q; fl[nf] = tb ? (size_t)(tb - q) : (size_t)(text + e - q); ++nf;
    if (!tb) break;
    q = tb + 1;
  }
  if (nf < 5) return false;
  if (!L.empty()) L.push_back(';');
  L += std::to_string(i + 1);
  for (int x : {1, 3, 4}) { L.push_back(':'); L.append((const char*)f[x], fl[x]); }
  return true;
}
// `#site WIN_LO WIN_HI RESCUED LEFT_LINES FOUND LEFT_ENTRIES REPLAY_LINES REPLAY_TRUTH`, one row per PARTIAL site of the job in
// site order; an empty list prints as `.`; the two strings replay the CHOSEN forms on the host, as for sites.tsv
int write_subsets_file(const char* path, const JobState& s, const std::vector<uint8_t>& cls_s, const std::vector<int32_t>& site,
                       const std::vector<uint8_t>& ecls_s, const NzEntries& t, const HpSites& st, const uint8_t* seq, int64_t len) {
  std::string out = "#site\tWIN_LO\tWIN_HI\tRESCUED\tLEFT_LINES\tFOUND\tLEFT_ENTRIES\tREPLAY_LINES\tREPLAY_TRUTH\n";
  const size_t ns = st.first.size();
  std::vector<std::string> got(ns), left(ns);
  std::vector<std::vector<HpForm>> side(ns);
  int64_t rec = 0;
  for (int64_t i = 0; i < s.info.n_lines; ++i) {
    if (is_header(s.line_kind[(size_t)i])) continue;
    const int64_t r = rec++;
    const uint8_t c = cls_s[(size_t)r];
    if (c != QM_HAP_C_SUBSET && c != QM_HAP_C_LEFT) continue;
    const int32_t k = site[(size_t)r];
    if (k < 0 || (size_t)k >= ns) continue;
    if (!hs_line_text(s, i, c == QM_HAP_C_SUBSET ? got[(size_t)k] : left[(size_t)k])) continue;
    if (c == QM_HAP_C_SUBSET) side[(size_t)k].push_back(hp_trim(s.pos[r], nz_spell(s.ref[r]), nz_spell(s.alt[r])));
  }
  auto dot = [](const std::string& x) { return x.empty() ? std::string(".") : x; };
  for (size_t k = 0; k < ns; ++k) {
    if (got[k].empty()) continue;
    const size_t e0 = (size_t)st.first[k], e1 = k + 1 < ns ? (size_t)st.first[k + 1] : t.pos.size();
    std::string found, eleft;
    std::vector<HpForm> tside;
    for (size_t j = e0; j < e1; ++j) {
      if (ecls_s[j] != QM_HAP_C_SUBSET && ecls_s[j] != QM_HAP_C_LEFT) continue;
      std::string& E = ecls_s[j] == QM_HAP_C_SUBSET ? found : eleft;
      if (!E.empty()) E.push_back(';');
      E += std::to_string(t.pos[j]) + ":" + nz_spell(t.ref[j]) + ":" + nz_spell(t.alt[j]);
      if (ecls_s[j] == QM_HAP_C_SUBSET) tside.push_back(hp_trim(t.pos[j], nz_spell(t.ref[j]), nz_spell(t.alt[j])));
    }
    out += std::to_string(k) + "\t" + std::to_string(st.lo[k]) + "\t" + std::to_string(st.hi[k]) + "\t" + got[k] + "\t" + dot(left[k]) + "\t" +
           dot(found) + "\t" + dot(eleft) + "\t" + hp_replay(seq, len, st.lo[k], st.hi[k], side[k]) + "\t" +
           hp_replay(seq, len, st.lo[k], st.hi[k], tside) + "\n";
  }
  return write_all_atomic(path, out);
}

// the haplotype pass (its rows and its sites files, as haplo_pass alone leaves them), then the search: its rows, and the subsets
// files of the jobs that name one
int hapsub_pass(const PassCtx& c, const qm_hapsub_args* hs, std::string& err) {
  if (!hs) return QM_OK;
  auto want = [&](int j) { return !c.jobs[j].pure && hs->genome_id[j] >= 0; };
  if (!c.any(want)) return QM_OK;
  auto path = [&](int j) { return want(j) && hs->subsets_out ? hs->subsets_out[j] : nullptr; };
  bool files = false;
  for (int j = 0; j < c.n_jobs; ++j) files = files || path(j);
  qm_haplotypes_args ha;
  memset(&ha, 0, sizeof ha);
  ha.genome_id = hs->genome_id; ha.gap = hs->gap; ha.rec = hs->rec; ha.tru = hs->tru;
  ha.sites_out = hs->sites_out; ha.genome_seq = hs->genome_seq; ha.genome_len = hs->genome_len;
  int rc = haplo_pass(c, &ha, err, files);
  if (rc != QM_OK) return rc;
  std::vector<uint64_t> sub(c.nv * QM_HAPSUB_COLS);
  rc = qm_batch_hapsubsets(c.batch, files ? QM_HAPSUB_COLUMNS : 0u, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_hapsubsets(c.batch, sub.data());
  if (rc == QM_OK) c.scatter_rows(hs->sub, sub, QM_HAPSUB_COLS, want);
  struct Task { int j; std::vector<uint8_t> cls_s, ecls_s, cls, ecls; std::vector<int32_t> site; };
  std::vector<Task> W;
  std::vector<NzEntries> ent(c.T.size());
  std::vector<HpSites> sites(c.T.size());
  std::vector<uint8_t> have(c.T.size(), 0);
  for (int j = 0; j < c.n_jobs && rc == QM_OK; ++j) {
    if (!path(j)) continue;
    const JobState& s = c.J[(size_t)j];
    const size_t n = (size_t)s.n_data + 1;
    if (!have[(size_t)s.truth]) {
      NzEntries& e = ent[(size_t)s.truth];
      HpSites& st = sites[(size_t)s.truth];
      int64_t tn = 0, sn = 0;
      (void)qm_truth_entries(c.ctx, c.truth_of(j).tid, nullptr, nullptr, nullptr, 0, &tn);   // (how many)
      e.pos.resize((size_t)tn + 1); e.ref.resize((size_t)tn + 1); e.alt.resize((size_t)tn + 1);
      rc = qm_truth_entries(c.ctx, c.truth_of(j).tid, e.pos.data(), e.ref.data(), e.alt.data(), tn, &tn);
      e.pos.resize((size_t)tn); e.ref.resize((size_t)tn); e.alt.resize((size_t)tn);
      st.first.resize((size_t)tn + 1); st.lo.resize((size_t)tn + 1); st.hi.resize((size_t)tn + 1);
      if (rc == QM_OK) rc = qm_truth_sites(c.ctx, c.truth_of(j).tid, hs->genome_id[j], hs->gap, st.first.data(), st.lo.data(), st.hi.data(), tn + 1, &sn);
      st.first.resize((size_t)sn); st.lo.resize((size_t)sn); st.hi.resize((size_t)sn);
      have[(size_t)s.truth] = 1;
    }
    if (rc != QM_OK) break;
    const size_t ne = ent[(size_t)s.truth].pos.size() + 1;
    W.push_back({j, std::vector<uint8_t>(n, 0), std::vector<uint8_t>(ne, 0), std::vector<uint8_t>(n, 0), std::vector<uint8_t>(ne, 0), std::vector<int32_t>(n, -1)});
    Task& k = W.back();
    rc = qm_batch_get_haplotyped(c.batch, s.batch_v, k.cls.data(), k.site.data(), k.ecls.data());
    int64_t m = 0;
    if (rc == QM_OK) rc = qm_batch_get_hapsubsetted(c.batch, s.batch_v, k.cls_s.data(), k.ecls_s.data(), nullptr, nullptr, nullptr, 0, &m);
  }
  if (rc != QM_OK) return c.lib(rc, err);
  std::vector<int> wrc(W.size(), QM_OK);
  parallel_for((int)W.size(), c.nthr, [&](int k) {
    const Task& w = W[(size_t)k];
    const size_t t = (size_t)c.J[(size_t)w.j].truth;
    wrc[(size_t)k] = write_subsets_file(hs->subsets_out[w.j], c.J[(size_t)w.j], w.cls_s, w.site, w.ecls_s, ent[t], sites[t], hs->genome_seq[w.j], hs->genome_len[w.j]);
  });
  for (size_t k = 0; k < W.size(); ++k)
    if (wrc[k] != QM_OK) { err = std::string("cannot write ") + hs->subsets_out[W[k].j]; return wrc[k]; }
  return QM_OK;
}

// the filter surface: S and extra of every wanted job
int surface_pass(const PassCtx& c, const qm_surface_args* sf, std::string& err) {
  auto want = [&](int j) { return sf->want[j] != 0; };
  if (!sf || !c.any(want)) return QM_OK;
  const size_t gw = 3 * (size_t)sf->nq * (size_t)sf->na;
  std::vector<uint64_t> S(c.nv * gw), ex(c.nv * QM_SF_EXTRA);
  int rc = qm_batch_surface(c.batch, sf->q_step, sf->nq, sf->na, nullptr);
  if (rc == QM_OK) rc = qm_batch_get_surface(c.batch, S.data(), ex.data());
  if (rc == QM_OK) { c.scatter_rows(sf->S, S, gw, want); c.scatter_rows(sf->extra, ex, QM_SF_EXTRA, want); }
  return c.lib(rc, err);
}

}  // namespace

extern "C" int qm_extract_files(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds) {
  return qm_extract_files_ex(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, nullptr, 0, nullptr);
}

static int extract_files(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict, qm_file_stats* stats,
                         uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot, int n_slots, void* global_dev, const Passes& P);

// The entry points of the passes: validate, zero the outputs, fill the pass's fields of Passes, call.
extern "C" int qm_extract_files_ex(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                   qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                   int n_slots, void* global_dev) {
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, Passes());
}

// rule mutationcontext behind the worker: the motif pass runs on the batch the classification leaves in HBM
extern "C" int qm_extract_files_motifs(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                       qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                       int n_slots, void* global_dev, const int32_t* genome_id, uint64_t* motifs_out) {
  if (n_jobs > 0 && (!genome_id || !motifs_out)) return fail(QM_E_INVAL, "qm_extract_files_motifs: NULL genome ids or output");
  if (motifs_out) memset(motifs_out, 0, sizeof(uint64_t) * 3 * QM_MOTIF_COLS * (size_t)n_jobs);
  Passes P; P.genome_id = genome_id; P.motifs_out = motifs_out;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// both halves of rule mutationcontext behind the worker: the spectra (optional) and the allele-frequency profile
extern "C" int qm_extract_files_profile(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                        qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                        int n_slots, void* global_dev, const int32_t* genome_id, uint64_t* motifs_out,
                                        const qm_profile_args* profile) {
  if (!profile || (n_jobs > 0 && (!profile->want || !profile->grid || !profile->extra))) return fail(QM_E_INVAL, "qm_extract_files_profile: NULL arguments");
  if ((genome_id == nullptr) != (motifs_out == nullptr)) return fail(QM_E_INVAL, "qm_extract_files_profile: genome ids and the motif output come together");
  if (profile->window < 1 || profile->window >= QM_POS_LIMIT || profile->n_pos_bins < 1 || profile->n_af_bins < 1 ||
      (int64_t)profile->n_pos_bins * profile->n_af_bins > QM_AFP_MAX_CELLS)
    return fail(QM_E_INVAL, "qm_extract_files_profile: window " + std::to_string(profile->window) + ", " + std::to_string(profile->n_af_bins) + " x " +
                                std::to_string(profile->n_pos_bins) + " bins (1 <= window < 2^28, at most " + std::to_string(QM_AFP_MAX_CELLS) + " cells)");
  const size_t cells = (size_t)profile->n_pos_bins * (size_t)profile->n_af_bins;
  if (n_jobs > 0) {
    memset(profile->grid, 0, sizeof(uint64_t) * 2 * cells * (size_t)n_jobs);
    memset(profile->extra, 0, sizeof(uint64_t) * 2 * QM_AFP_EXTRA * (size_t)n_jobs);
  }
  if (motifs_out) memset(motifs_out, 0, sizeof(uint64_t) * 3 * QM_MOTIF_COLS * (size_t)n_jobs);
  Passes P; P.genome_id = genome_id; P.motifs_out = motifs_out; P.pa = profile;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the two group passes: every job names no group or one of the call's, none of them pure-strain, 1 to max_members jobs per group
static int check_groups(const std::string& who, int n_jobs, const qm_file_job* jobs, const int32_t* group, int n_groups, int max_members) {
  for (int j = 0; j < n_jobs; ++j) {
    if (group[j] < -1 || group[j] >= n_groups) return fail(QM_E_INVAL, who + ": job " + std::to_string(j) + " names group " + std::to_string(group[j]));
    if (jobs[j].pure && group[j] >= 0) return fail(QM_E_INVAL, who + ": pure-strain job " + std::to_string(j) + " cannot be in a group (its truth is never read)");
  }
  for (int g = 0; g < n_groups; ++g) {
    const int members = (int)std::count(group, group + n_jobs, g);
    if (members < 1 || members > max_members)
      return fail(QM_E_INVAL, who + ": group " + std::to_string(g) + " has " + std::to_string(members) + " jobs (1 to " + std::to_string(max_members) + ")");
  }
  return QM_OK;
}

// the truth-side view behind the worker: missed-variant lists and the caller Venn regions of groups of jobs
extern "C" int qm_extract_files_truthside(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                          qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                          int n_slots, void* global_dev, const qm_truthside_args* ts) {
  if (!ts || ts->n_groups < 0 || (n_jobs > 0 && (!ts->fn_out || !ts->group)) || (ts->n_groups > 0 && !ts->regions))
    return fail(QM_E_INVAL, "qm_extract_files_truthside: NULL arguments");
  if (mode & QM_BATCH_ALLELES) return fail(QM_E_STATE, "qm_extract_files_truthside: allele-extended batches have no truth-side view (single-base batches only)");
  const int rc = check_groups("qm_extract_files_truthside", n_jobs, jobs, ts->group, ts->n_groups, QM_TRUTH_GROUP_MAX);
  if (rc != QM_OK) return rc;
  memset(ts->regions, 0, sizeof(uint64_t) * QM_TRUTH_REGIONS * (size_t)ts->n_groups);
  if (ts->fp_regions) memset(ts->fp_regions, 0, sizeof(int64_t) * QM_TRUTH_REGIONS * (size_t)ts->n_groups);
  Passes P; P.ts = ts;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the counts per stratum behind the worker
extern "C" int qm_extract_files_strata(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                       qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                       int n_slots, void* global_dev, const qm_strata_args* strata) {
  if (!strata || (n_jobs > 0 && (!strata->want || !strata->rec || !strata->tru))) return fail(QM_E_INVAL, "qm_extract_files_strata: NULL arguments");
  int64_t info[2] = {0, 0};
  const int rc = qm_strata_info(ctx, strata->strata_id, info);
  if (rc != QM_OK) return rc;
  if (n_jobs > 0) {
    memset(strata->rec, 0, sizeof(uint64_t) * 3 * (size_t)(info[0] + 2) * (size_t)n_jobs);
    memset(strata->tru, 0, sizeof(uint64_t) * 2 * (size_t)(info[0] + 1) * (size_t)n_jobs);
  }
  Passes P; P.sa = strata;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the counts per sequence-context cell behind the worker
extern "C" int qm_extract_files_context(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                        qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                        int n_slots, void* global_dev, const qm_context_args* context) {
  const qm_context_args* cx = context;
  if (!cx || (n_jobs > 0 && (!cx->genome_id || !cx->rec || !cx->tru || !cx->gen))) return fail(QM_E_INVAL, "qm_extract_files_context: NULL arguments");
  if (cx->w < 0 || cx->w > QM_CX_MAX_HALF_WINDOW)
    return fail(QM_E_INVAL, "qm_extract_files_context: half window " + std::to_string(cx->w) + " (0 to " + std::to_string(QM_CX_MAX_HALF_WINDOW) + ")");
  if (cx->ng < 1 || cx->ng > QM_CX_MAX_GC_BINS)
    return fail(QM_E_INVAL, "qm_extract_files_context: " + std::to_string(cx->ng) + " GC bins (1 to " + std::to_string(QM_CX_MAX_GC_BINS) + ")");
  if (n_jobs > 0) {
    const size_t nc = (size_t)(16 * cx->ng + 1);
    memset(cx->rec, 0, sizeof(uint64_t) * 3 * (nc + 1) * (size_t)n_jobs);
    memset(cx->tru, 0, sizeof(uint64_t) * 2 * nc * (size_t)n_jobs);
    memset(cx->gen, 0, sizeof(uint64_t) * nc * (size_t)n_jobs);
  }
  Passes P; P.cx = cx;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// indels and MNPs matched by normal form behind the worker
extern "C" int qm_extract_files_normalize(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                          qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                          int n_slots, void* global_dev, const qm_normalize_args* normalize) {
  const qm_normalize_args* na = normalize;
  if (!na || (n_jobs > 0 && (!na->genome_id || !na->rec || !na->tru))) return fail(QM_E_INVAL, "qm_extract_files_normalize: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_normalize: the normal form is taken of indels and MNPs, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (n_jobs > 0) {
    memset(na->rec, 0, sizeof(uint64_t) * QM_NORM_R_COLS * (size_t)n_jobs);
    memset(na->tru, 0, sizeof(uint64_t) * QM_NORM_T_COLS * (size_t)n_jobs);
  }
  Passes P; P.nz = na;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// MNPs matched against adjacent SNVs behind the worker
extern "C" int qm_extract_files_atomize(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                        qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                        int n_slots, void* global_dev, const qm_atomize_args* atomize) {
  const qm_atomize_args* at = atomize;
  if (!at || (n_jobs > 0 && (!at->want || !at->rec || !at->tru))) return fail(QM_E_INVAL, "qm_extract_files_atomize: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_atomize: atoms are taken of MNPs, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (n_jobs > 0) {
    memset(at->rec, 0, sizeof(uint64_t) * QM_ATOM_R_COLS * (size_t)n_jobs);
    memset(at->tru, 0, sizeof(uint64_t) * QM_ATOM_T_COLS * (size_t)n_jobs);
  }
  Passes P; P.at = at;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// TP, FP and FN by variant type and size behind the worker
extern "C" int qm_extract_files_types(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                      qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                      int n_slots, void* global_dev, const qm_types_args* types) {
  const qm_types_args* ty = types;
  if (!ty || !ty->edges || (n_jobs > 0 && (!ty->want || !ty->rec || !ty->tru))) return fail(QM_E_INVAL, "qm_extract_files_types: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_types: variants are typed by their alleles, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (ty->n_bins < 1 || ty->n_bins > QM_TYPE_MAX_BINS)
    return fail(QM_E_INVAL, "qm_extract_files_types: " + std::to_string(ty->n_bins) + " size bins (1 to " + std::to_string(QM_TYPE_MAX_BINS) + ")");
  for (int i = 0; i < ty->n_bins; ++i)
    if (i == 0 ? ty->edges[0] != 1 : ty->edges[i] <= ty->edges[i - 1])
      return fail(QM_E_INVAL, "qm_extract_files_types: the size edges ascend from 1 (edge " + std::to_string(i) + " is " + std::to_string(ty->edges[i]) + ")");
  if (n_jobs > 0) {
    const size_t w = 2 * (size_t)(5 * ty->n_bins + 4);
    memset(ty->rec, 0, sizeof(uint64_t) * w * (size_t)n_jobs);
    memset(ty->tru, 0, sizeof(uint64_t) * w * (size_t)n_jobs);
  }
  Passes P; P.ty = ty;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// clusters of records matched by replayed haplotype behind the worker
extern "C" int qm_extract_files_haplotypes(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                           qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                           int n_slots, void* global_dev, const qm_haplotypes_args* haplotypes) {
  const qm_haplotypes_args* ha = haplotypes;
  if (!ha || (n_jobs > 0 && (!ha->genome_id || !ha->rec || !ha->tru))) return fail(QM_E_INVAL, "qm_extract_files_haplotypes: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_haplotypes: haplotypes are replayed from indels, MNPs and complex records, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (ha->gap < 0 || ha->gap > QM_HAP_MAX_GAP)
    return fail(QM_E_INVAL, "qm_extract_files_haplotypes: gap " + std::to_string(ha->gap) + " (0 to " + std::to_string(QM_HAP_MAX_GAP) + ")");
  for (int j = 0; j < n_jobs; ++j)
    if (ha->sites_out && ha->sites_out[j] && ha->genome_id[j] >= 0 && (!ha->genome_seq || !ha->genome_len || !ha->genome_seq[j] || ha->genome_len[j] < 1))
      return fail(QM_E_INVAL, "qm_extract_files_haplotypes: job " + std::to_string(j) + " names a sites file and not the bytes of its genome");
  if (n_jobs > 0) {
    memset(ha->rec, 0, sizeof(uint64_t) * QM_HAP_R_COLS * (size_t)n_jobs);
    memset(ha->tru, 0, sizeof(uint64_t) * QM_HAP_T_COLS * (size_t)n_jobs);
  }
  Passes P; P.hp = ha;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the subset search behind the haplotype pass behind the worker
extern "C" int qm_extract_files_hapsubsets(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                           qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                           int n_slots, void* global_dev, const qm_hapsub_args* hapsubsets) {
  const qm_hapsub_args* hs = hapsubsets;
  if (!hs || (n_jobs > 0 && (!hs->genome_id || !hs->rec || !hs->tru || !hs->sub))) return fail(QM_E_INVAL, "qm_extract_files_hapsubsets: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_hapsubsets: haplotypes are replayed from indels, MNPs and complex records, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (hs->gap < 0 || hs->gap > QM_HAP_MAX_GAP)
    return fail(QM_E_INVAL, "qm_extract_files_hapsubsets: gap " + std::to_string(hs->gap) + " (0 to " + std::to_string(QM_HAP_MAX_GAP) + ")");
  for (int j = 0; j < n_jobs; ++j) {
    const bool file = (hs->sites_out && hs->sites_out[j]) || (hs->subsets_out && hs->subsets_out[j]);
    if (file && hs->genome_id[j] >= 0 && (!hs->genome_seq || !hs->genome_len || !hs->genome_seq[j] || hs->genome_len[j] < 1))
      return fail(QM_E_INVAL, "qm_extract_files_hapsubsets: job " + std::to_string(j) + " names a sites or subsets file and not the bytes of its genome");
  }
  if (n_jobs > 0) {
    memset(hs->rec, 0, sizeof(uint64_t) * QM_HAP_R_COLS * (size_t)n_jobs);
    memset(hs->tru, 0, sizeof(uint64_t) * QM_HAP_T_COLS * (size_t)n_jobs);
    memset(hs->sub, 0, sizeof(uint64_t) * QM_HAPSUB_COLS * (size_t)n_jobs);
  }
  Passes P; P.hs = hs;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the QUAL ROC under normal-form and atom matching behind the worker
extern "C" int qm_extract_files_rescue_roc(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                           qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                           int n_slots, void* global_dev, const qm_rescue_roc_args* rescue_roc) {
  const qm_rescue_roc_args* rr = rescue_roc;
  if (!rr || (n_jobs > 0 && (!rr->genome_id || !rr->want || !rr->roc_n || !rr->roc_a || !rr->base)))
    return fail(QM_E_INVAL, "qm_extract_files_rescue_roc: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_rescue_roc: the rescue passes it sweeps match indels and MNPs, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (n_bins < 1 || n_bins > 256) return fail(QM_E_INVAL, "qm_extract_files_rescue_roc: n_bins = " + std::to_string(n_bins) + " (1 to 256)");
  if (n_jobs > 0) {
    memset(rr->roc_n, 0, sizeof(uint64_t) * 3 * (size_t)n_bins * (size_t)n_jobs);
    memset(rr->roc_a, 0, sizeof(uint64_t) * 3 * (size_t)n_bins * (size_t)n_jobs);
    memset(rr->base, 0, sizeof(uint64_t) * 2 * (size_t)n_jobs);
  }
  Passes P; P.rr = rr;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the four rescues combined behind the worker
extern "C" int qm_extract_files_ladder(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                       qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                       int n_slots, void* global_dev, const qm_ladder_args* ladder) {
  const qm_ladder_args* la = ladder;
  if (!la || (n_jobs > 0 && (!la->genome_id || !la->want || !la->rec || !la->tru)))
    return fail(QM_E_INVAL, "qm_extract_files_ladder: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_ladder: the rescue passes it combines match indels and MNPs, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (la->gap < 0 || la->gap > QM_HAP_MAX_GAP)
    return fail(QM_E_INVAL, "qm_extract_files_ladder: gap " + std::to_string(la->gap) + " (0 to " + std::to_string(QM_HAP_MAX_GAP) + ")");
  if (n_jobs > 0) {
    memset(la->rec, 0, sizeof(uint64_t) * QM_LADDER_COLS * (size_t)n_jobs);
    memset(la->tru, 0, sizeof(uint64_t) * QM_LADDER_COLS * (size_t)n_jobs);
  }
  Passes P; P.ld = la;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the match ladder per variant type and size behind the worker
extern "C" int qm_extract_files_ladder_types(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                             qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                             int n_slots, void* global_dev, const qm_ladder_types_args* ladder_types) {
  const qm_ladder_types_args* lt = ladder_types;
  if (!lt || !lt->edges || (n_jobs > 0 && (!lt->genome_id || !lt->want || !lt->rec || !lt->tru)))
    return fail(QM_E_INVAL, "qm_extract_files_ladder_types: NULL arguments");
  if (!(mode & QM_BATCH_ALLELES))
    return fail(QM_E_STATE, "qm_extract_files_ladder_types: the types and the rescue passes it crosses read indels and MNPs, which only the allele-extended mode (QM_BATCH_ALLELES) reads");
  if (lt->gap < 0 || lt->gap > QM_HAP_MAX_GAP)
    return fail(QM_E_INVAL, "qm_extract_files_ladder_types: gap " + std::to_string(lt->gap) + " (0 to " + std::to_string(QM_HAP_MAX_GAP) + ")");
  if (lt->n_bins < 1 || lt->n_bins > QM_TYPE_MAX_BINS)
    return fail(QM_E_INVAL, "qm_extract_files_ladder_types: " + std::to_string(lt->n_bins) + " size bins (1 to " + std::to_string(QM_TYPE_MAX_BINS) + ")");
  for (int i = 0; i < lt->n_bins; ++i)
    if (i == 0 ? lt->edges[0] != 1 : lt->edges[i] <= lt->edges[i - 1])
      return fail(QM_E_INVAL, "qm_extract_files_ladder_types: the size edges ascend from 1 (edge " + std::to_string(i) + " is " + std::to_string(lt->edges[i]) + ")");
  if (n_jobs > 0) {
    const size_t w = (size_t)(5 * lt->n_bins + 4) * QM_LADDER_COLS;
    memset(lt->rec, 0, sizeof(uint64_t) * w * (size_t)n_jobs);
    memset(lt->tru, 0, sizeof(uint64_t) * w * (size_t)n_jobs);
  }
  Passes P; P.lt = lt;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the bootstrap pass behind the worker
extern "C" int qm_extract_files_boot(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                     qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                     int n_slots, void* global_dev, const qm_boot_args* boot) {
  if (!boot || (n_jobs > 0 && (!boot->want || !boot->cnt || (boot->n_rep > 0 && !boot->rep)))) return fail(QM_E_INVAL, "qm_extract_files_boot: NULL arguments");
  if (boot->window < 1 || boot->n_win < 1 || boot->n_win > QM_BOOT_MAX_WINDOWS || boot->n_rep < 0 || boot->n_rep > QM_BOOT_MAX_REP)
    return fail(QM_E_INVAL, "qm_extract_files_boot: window = " + std::to_string(boot->window) + " (at least 1), n_win = " + std::to_string(boot->n_win) +
                                " (1 to " + std::to_string(QM_BOOT_MAX_WINDOWS) + "), n_rep = " + std::to_string(boot->n_rep) + " (0 to " + std::to_string(QM_BOOT_MAX_REP) + ")");
  if (n_jobs > 0) {
    memset(boot->cnt, 0, sizeof(uint64_t) * 4 * (size_t)(boot->n_win + 2) * (size_t)n_jobs);
    if (boot->n_rep) memset(boot->rep, 0, sizeof(uint64_t) * 4 * (size_t)boot->n_rep * (size_t)n_jobs);
  }
  Passes P; P.ba = boot;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// k-of-n caller consensus behind the worker: vote tables of groups of jobs, and a group's consensus VCF
extern "C" int qm_extract_files_votes(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                      qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                      int n_slots, void* global_dev, const qm_votes_args* votes) {
  const qm_votes_args* va = votes;
  if (!va || va->n_groups < 0 || (n_jobs > 0 && !va->group) || (va->n_groups > 0 && (!va->tp_votes || !va->fp_votes || !va->private_tp || !va->private_fp)))
    return fail(QM_E_INVAL, "qm_extract_files_votes: NULL arguments");
  if (mode & QM_BATCH_ALLELES) return fail(QM_E_STATE, "qm_extract_files_votes: allele-extended batches have no vote pass (single-base batches only)");
  const int rc = check_groups("qm_extract_files_votes", n_jobs, jobs, va->group, va->n_groups, QM_VOTE_GROUP_MAX);
  if (rc != QM_OK) return rc;
  for (int g = 0; g < va->n_groups; ++g) {
    const int members = (int)std::count(va->group, va->group + n_jobs, g);
    const int k = va->consensus_k ? va->consensus_k[g] : 0;
    if (k < 0 || k > members) return fail(QM_E_INVAL, "qm_extract_files_votes: group " + std::to_string(g) + ": consensus level " + std::to_string(k) + " with " + std::to_string(members) + " members");
    if (k > 0 && (!va->consensus_out || !va->consensus_out[g])) return fail(QM_E_INVAL, "qm_extract_files_votes: group " + std::to_string(g) + " names a consensus level and no file");
  }
  if (va->n_groups > 0) {
    memset(va->tp_votes, 0, sizeof(uint64_t) * QM_VOTE_SLOTS * (size_t)va->n_groups);
    memset(va->fp_votes, 0, sizeof(uint64_t) * QM_VOTE_SLOTS * (size_t)va->n_groups);
    memset(va->private_tp, 0, sizeof(uint64_t) * QM_VOTE_GROUP_MAX * (size_t)va->n_groups);
    memset(va->private_fp, 0, sizeof(uint64_t) * QM_VOTE_GROUP_MAX * (size_t)va->n_groups);
  }
  Passes P; P.va = va;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the near-miss classes behind the worker: why the FP lines are FP and the missed truth keys missed
extern "C" int qm_extract_files_nearmiss(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                         qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                         int n_slots, void* global_dev, const qm_nearmiss_args* nearmiss) {
  const qm_nearmiss_args* nm = nearmiss;
  if (!nm || (n_jobs > 0 && (!nm->want || !nm->rec || !nm->tru))) return fail(QM_E_INVAL, "qm_extract_files_nearmiss: NULL arguments");
  if (nm->radius < 0 || nm->radius > QM_NM_MAX_RADIUS)
    return fail(QM_E_INVAL, "qm_extract_files_nearmiss: radius " + std::to_string(nm->radius) + " (0 to " + std::to_string(QM_NM_MAX_RADIUS) + ")");
  if (mode & QM_BATCH_ALLELES) return fail(QM_E_STATE, "qm_extract_files_nearmiss: allele-extended batches have no near-miss pass (single-base batches only)");
  if (n_jobs > 0) {
    memset(nm->rec, 0, sizeof(uint64_t) * QM_NM_R_CLASSES * (size_t)n_jobs);
    memset(nm->tru, 0, sizeof(uint64_t) * QM_NM_T_CLASSES * (size_t)n_jobs);
  }
  Passes P; P.nm = nm;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

// the filter surface behind the worker: TP, FP and found truth keys at every QUAL x AF threshold
extern "C" int qm_extract_files_surface(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict,
                                        qm_file_stats* stats, uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot,
                                        int n_slots, void* global_dev, const qm_surface_args* surface) {
  const qm_surface_args* sf = surface;
  if (!sf || (n_jobs > 0 && (!sf->want || !sf->S || !sf->extra))) return fail(QM_E_INVAL, "qm_extract_files_surface: NULL arguments");
  if (sf->q_step < 1 || sf->q_step > QM_SF_MAX_QUAL_STEP)
    return fail(QM_E_INVAL, "qm_extract_files_surface: q_step " + std::to_string(sf->q_step) + " (1 to " + std::to_string(QM_SF_MAX_QUAL_STEP) + ")");
  if (sf->nq < 1 || sf->nq > QM_SF_MAX_QUAL_BINS)
    return fail(QM_E_INVAL, "qm_extract_files_surface: nq " + std::to_string(sf->nq) + " (1 to " + std::to_string(QM_SF_MAX_QUAL_BINS) + ")");
  if (sf->na < 1 || sf->na > QM_SF_MAX_AF_BINS)
    return fail(QM_E_INVAL, "qm_extract_files_surface: na " + std::to_string(sf->na) + " (1 to " + std::to_string(QM_SF_MAX_AF_BINS) + ")");
  if (sf->nq * sf->na > QM_SF_MAX_CELLS)
    return fail(QM_E_INVAL, "qm_extract_files_surface: nq * na = " + std::to_string(sf->nq * sf->na) + " cells (at most " + std::to_string(QM_SF_MAX_CELLS) + ")");
  if (mode & QM_BATCH_ALLELES) return fail(QM_E_STATE, "qm_extract_files_surface: allele-extended batches have no filter surface (single-base batches only)");
  for (int j = 0; j < n_jobs; ++j)
    if (sf->want[j] && jobs && jobs[j].pure)
      return fail(QM_E_INVAL, std::string("qm_extract_files_surface: ") + jobs[j].vcf_path + " is a pure-strain job: it has no truth set and no filter surface");
  if (n_jobs > 0) {
    memset(sf->S, 0, sizeof(uint64_t) * 3 * (size_t)sf->nq * (size_t)sf->na * (size_t)n_jobs);
    memset(sf->extra, 0, sizeof(uint64_t) * QM_SF_EXTRA * (size_t)n_jobs);
  }
  Passes P; P.sf = sf;
  return extract_files(ctx, n_jobs, jobs, n_bins, mode, strict, stats, roc_out, phase_seconds, truth_slot, n_slots, global_dev, P);
}

static int extract_files(qm_ctx* ctx, int n_jobs, const qm_file_job* jobs, int n_bins, unsigned mode, int strict, qm_file_stats* stats,
                         uint64_t* roc_out, double* phase_seconds, const int32_t* truth_slot, int n_slots, void* global_dev, const Passes& P) {
  if (!ctx || n_jobs < 0 || (n_jobs && !jobs) || n_bins < 1 || n_bins > QM_MAX_BINS || (mode & ~(unsigned)QM_BATCH_ALLELES))
    return fail(QM_E_INVAL, "qm_extract_files: bad arguments");
  if (global_dev && (n_slots < 1 || (n_jobs && !truth_slot))) return fail(QM_E_INVAL, "qm_extract_files_ex: global_dev needs truth_slot and n_slots >= 1");
  const size_t gbytes = global_dev ? (size_t)n_slots * 3 * (size_t)n_bins * sizeof(uint64_t) : 0;
  if (global_dev) { const int rc0 = qm_device_zero(ctx, global_dev, gbytes); if (rc0 != QM_OK) return rc0; }   // (on the context's device, whatever the caller's thread had current)
  if (n_jobs == 0) {   // nothing to do is not an error (a rank of a sharded run may hold no VCF)
    if (phase_seconds) memset(phase_seconds, 0, 8 * sizeof(double));
    return QM_OK;
  }
  const bool ext = (mode & QM_BATCH_ALLELES) != 0;
  // map + count, truth sets (beside the former), batch layout, tokenise + host path (+ uploads beside it), engine, masks back,
  // write, release (the truth sets overlap the first phases, so the sum of the phases exceeds the wall time of the call)
  double ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, phc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::mutex ph_mu;
  const bool trace = getenv("QM_FILES_TRACE") != nullptr;
  auto add_ph = [&](int k, double dt, double dc = 0.0) { std::lock_guard<std::mutex> g(ph_mu); ph[k] += dt; phc[k] += dc; };
  const int nthr = qm_host_threads();
  std::vector<JobState> J((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    const qm_file_job& q = jobs[j];
    if (!q.vcf_path || !q.filtered_out || !q.fp_out || (!q.pure && (!q.truth_path || !q.tp_out)) || (q.mode != 0 && q.mode != 1))
      return fail(QM_E_INVAL, "qm_extract_files: job " + std::to_string(j) + " is incomplete");
    if (ext && !q.pure && q.mode != 0) return fail(QM_E_INVAL, "qm_extract_files: the allele-extended mode needs VCF truth sets (mode 0)");
  }
  qm_dict* dict = ext ? qm_dict_create() : nullptr;
  std::vector<TruthState> T;
  int empty_tid = -1;

  // ---- the VCFs go through as ONE batch: stage one (map, count, tokenise, upload) of every VCF, then stage two (engine,
  //      masks, files).  A pipeline of groups -- stage two of group g on a thread of its own beside stage one of group g + 1 --
  //      was slower: 83 ms in one group, 86 / 108 / 142 ms in 2 / 4 / 6 (round 3, 16 VCFs of 10^6 lines; LABNOTES.md): every
  //      stage parallelises over files, so smaller groups only idle threads.
  qm_batch* batch = nullptr;        // the VCFs with a truth set, in job order
  std::vector<int64_t> nrec;
  std::vector<int32_t> tids;
  hipStream_t copy_stream = nullptr;
  std::thread truth_thread;   // ends with the patterns of the truth files
  auto cleanup = [&]() {
    if (truth_thread.joinable()) truth_thread.join();
    if (batch) { qm_batch_destroy(batch); batch = nullptr; }
    if (copy_stream) { (void)hipStreamDestroy(copy_stream); copy_stream = nullptr; }
    if (empty_tid >= 0) { (void)qm_truth_release(ctx, empty_tid); empty_tid = -1; }
    for (auto& t : T) { if (t.pats) qm_patterns_destroy(t.pats); if (t.tid >= 0) (void)qm_truth_release(ctx, t.tid); }
    if (dict) qm_dict_destroy(dict);
  };

  // ---- 1. the distinct truth files (keys for the device, patterns as text for the host path), on a thread of their own ...
  {
    std::map<std::pair<std::string, int>, int> seen;
    for (int j = 0; j < n_jobs; ++j) {
      if (jobs[j].pure) continue;
      const auto key = std::make_pair(std::string(jobs[j].truth_path), (int)jobs[j].mode);
      auto it = seen.find(key);
      if (it == seen.end()) { it = seen.emplace(key, (int)T.size()).first; T.emplace_back(); T.back().path = key.first; T.back().mode = key.second; }
      J[(size_t)j].truth = it->second;
    }
  }
  std::vector<int32_t> slot_of_truth(T.size(), -1);
  if (global_dev) {
    for (int j = 0; j < n_jobs; ++j) {
      if (jobs[j].pure) continue;
      const int32_t sl = truth_slot[j];
      int32_t& have = slot_of_truth[(size_t)J[(size_t)j].truth];
      if (sl < 0 || sl >= n_slots || (have >= 0 && have != sl)) {
        if (dict) qm_dict_destroy(dict);
        return fail(QM_E_INVAL, "qm_extract_files_ex: job " + std::to_string(j) + " names row " + std::to_string(sl) + " for a truth file that another job puts elsewhere (or outside [0, n_slots))");
      }
      have = sl;
    }
  }
  int truth_rc = QM_OK;
  std::string truth_msg;
  // The keys go first (the batch layout needs the truth ids as soon as the VCFs are counted); the patterns as text -- a hash
  // set of every row, wanted only by the host path and by the decision whether a VCF needs it -- are built on a thread of
  // their own and waited for by the first VCF that has been tokenised.
  std::mutex pats_mu;
  std::condition_variable pats_cv;
  bool pats_ready = false, keys_ready = false;
  truth_thread = std::thread([&]() {
    const double tt0 = now(), tc0 = trace ? cpu_now() : 0.0;
    parallel_for((int)T.size(), std::max(1, nthr / 4), [&](int k) {
      TruthState& t = T[(size_t)k];
      t.file.open_file(t.path.c_str());
      if (!t.file.ok) t.rc = QM_E_IO;
    });
    std::thread pats_thread([&]() {
      parallel_for((int)T.size(), std::max(1, nthr / 4), [&](int k) {
        TruthState& t = T[(size_t)k];
        if (t.rc != QM_OK) return;
        t.pats = qm_patterns_create(t.file.p, t.file.n, t.mode, ext ? 1 : 0);
        if (!t.pats) { t.rc = QM_E_INVAL; return; }
        (void)qm_patterns_info(t.pats, t.info);
      });
      { std::lock_guard<std::mutex> g(pats_mu); pats_ready = true; }
      pats_cv.notify_all();
    });
    for (auto& t : T) {
      if (truth_rc != QM_OK) break;
      if (t.rc == QM_E_IO) { truth_rc = t.rc; truth_msg = "cannot read truth file " + t.path; break; }
      const int64_t cap = qm_vcf_count_lines(t.file.p, t.file.n) + 1;
      std::vector<int32_t> tp((size_t)cap), tr((size_t)cap), ta((size_t)cap);
      const int64_t k = qm_truth_scan_ext(t.file.p, t.file.n, t.mode, cap, tp.data(), tr.data(), ta.data(), t.counts, dict);
      if (k < 0) { truth_rc = (int)k; truth_msg = "qm_truth_scan failed for " + t.path; break; }
      const int rc = qm_truth_load(ctx, tp.data(), tr.data(), ta.data(), k, &t.tid);
      if (rc != QM_OK) { truth_rc = rc; truth_msg = qm_last_error(ctx); break; }
      if (P.ts || P.va || P.nm) {
        for (int64_t i = 0; i < k; ++i)
          if ((uint32_t)(tr[(size_t)i] | ta[(size_t)i]) < 4u) t.keys.push_back(((uint32_t)tp[(size_t)i] << 4) | ((uint32_t)tr[(size_t)i] << 2) | (uint32_t)ta[(size_t)i]);
        std::sort(t.keys.begin(), t.keys.end());
        t.keys.erase(std::unique(t.keys.begin(), t.keys.end()), t.keys.end());
      }
    }
    add_ph(1, now() - tt0, trace ? cpu_now() - tc0 : 0.0);
    { std::lock_guard<std::mutex> g(pats_mu); keys_ready = true; }
    pats_cv.notify_all();
    pats_thread.join();   // (the VCFs do not wait for this thread but for pats_ready)
  });
  auto wait_patterns = [&]() { std::unique_lock<std::mutex> g(pats_mu); pats_cv.wait(g, [&] { return pats_ready; }); };

  CtxArena* const ca = arena_of(ctx);
  std::unique_lock<std::mutex> arena_lock(ca->mu);   // one call at a time per context uses its page-locked arena

  // ---- stage 1: map + count, batch layout, tokenise + host path + uploads ----
  auto stage_one = [&]() -> int {
    double t0 = now(), c0 = trace ? cpu_now() : 0.0;
    parallel_for(n_jobs, nthr, [&](int j) {
      JobState& s = J[(size_t)j];
      s.vcf.open_file(jobs[j].vcf_path);
      if (!s.vcf.ok) { s.rc = QM_E_IO; return; }
      int64_t nl = 0, nd = 0;
      qm_host_count_lines(s.vcf.p, s.vcf.n, &nl, &nd);
      s.n_lines = nl; s.n_data = nd;
    });
    add_ph(0, now() - t0, trace ? cpu_now() - c0 : 0.0);
    { std::unique_lock<std::mutex> g(pats_mu); pats_cv.wait(g, [&] { return keys_ready; }); }   // the thread itself ends with the patterns
    for (int j = 0; j < n_jobs; ++j)
      if (J[(size_t)j].rc != QM_OK) return fail(QM_E_IO, std::string("cannot read ") + jobs[j].vcf_path);
    if (truth_rc != QM_OK) return fail(truth_rc, truth_msg);
    t0 = now(); c0 = trace ? cpu_now() : 0.0;
    // the batch holds every mixed-sample job, and the pure-strain jobs a pass wants (against an empty truth set)
    for (int j = 0; j < n_jobs; ++j) {
      if (jobs[j].pure && !P.any_batch_only(j)) continue;
      if (jobs[j].pure && empty_tid < 0) {
        const int rc = qm_truth_load(ctx, nullptr, nullptr, nullptr, 0, &empty_tid);
        if (rc != QM_OK) return rc;
      }
      J[(size_t)j].batch_v = (int)nrec.size(); nrec.push_back(J[(size_t)j].n_data);
      tids.push_back(jobs[j].pure ? empty_tid : T[(size_t)J[(size_t)j].truth].tid);
    }
    if (!nrec.empty()) {
      const int rc = qm_batch_create_ext(ctx, (int)nrec.size(), nrec.data(), tids.data(), n_bins, mode, &batch);
      if (rc != QM_OK) return rc;
    }
    size_t need = 0;
    std::vector<size_t> aoff((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
      aoff[(size_t)j] = need;
      const size_t cap = (size_t)J[(size_t)j].n_lines + 1;
      need += ((cap * 17 + 255) & ~(size_t)255) + ((((cap + 63) / 64) * 16 + 255) & ~(size_t)255);
    }
    uint8_t* arena = ca->arena.get(need);
    if (!arena) return fail(QM_E_NOMEM, "qm_extract_files: no memory for the column buffers");
    if (hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) != hipSuccess) return fail(QM_E_HIP, "hipStreamCreate failed");
    add_ph(2, now() - t0, trace ? cpu_now() - c0 : 0.0);
    t0 = now(); c0 = trace ? cpu_now() : 0.0;
    const int per_file_threads = std::max(1, nthr / std::max(1, std::min(n_jobs, nthr)));
    parallel_for(n_jobs, nthr, [&](int j) {
      JobState& s = J[(size_t)j];
      const size_t cap = (size_t)s.n_lines + 1;
      uint8_t* a = arena + aoff[(size_t)j];
      s.pos = (int32_t*)a; s.ref = s.pos + cap; s.alt = s.ref + cap; s.qual = (float*)(s.alt + cap); s.flags = (uint8_t*)(s.qual + cap);
      s.kept = (uint64_t*)(a + ((cap * 17 + 255) & ~(size_t)255)); s.tp = s.kept + (cap + 63) / 64;
      s.line_off.resize(cap + 1);
      s.line_kind.resize(cap);
      s.rc = qm_host_scan_threads(s.vcf.p, s.vcf.n, (int64_t)cap, s.line_off.data(), s.line_kind.data(), s.pos, s.ref, s.alt, s.qual, s.flags,
                                  &s.info, dict, per_file_threads > 1 ? per_file_threads : -1);   // -1: one thread, lines counted above
      if (s.rc != QM_OK || s.info.n_data != s.n_data) {
        // (the file changed between the count and the scan: the scan stops at the room it was given)
        s.err = s.rc == QM_OK || s.rc == QM_E_INVAL ? "the file changed while it was being read" : "tokenising failed";
        if (s.rc == QM_OK) s.rc = QM_E_INVAL;
        return;
      }
      if (P.wants_af(j)) {   // the INFO column, by a scanner of its own
        int64_t ai[2];
        s.af.resize((size_t)s.n_data + 1);
        s.rc = qm_vcf_scan_af(s.vcf.p, s.vcf.n, s.info.n_lines, s.line_off.data(), s.line_kind.data(), s.af.data(), ai);
        if (s.rc != QM_OK) { s.err = "scanning the INFO column failed"; return; }
      }
      // the frequencies follow the columns (whose upload clears the VCF's mark); a blocking copy of this VCF's floats
      auto upload_af = [&]() {
        if (s.rc != QM_OK || !P.wants_af(j)) return;
        s.rc = qm_batch_upload_af(batch, s.batch_v, s.af.data());
        if (s.rc != QM_OK) s.err = qm_last_error(ctx);
      };
      if (jobs[j].pure) {
        if (s.batch_v >= 0 && !(strict && s.info.n_refused)) {
          s.rc = qm_batch_upload_async(batch, s.batch_v, s.pos, s.ref, s.alt, s.qual, s.flags, copy_stream);
          if (s.rc != QM_OK) s.err = qm_last_error(ctx);
          upload_af();
        }
        return;
      }
      wait_patterns();
      const TruthState& t = T[(size_t)s.truth];
      if (t.rc != QM_OK) { s.rc = t.rc; return; }
      if (s.info.n_host || s.info.n_nokey_kept || t.info[1] > 0 || t.info[2] > 0) {
        s.rc = qm_vcf_hostpath(t.pats, s.vcf.p, s.vcf.n, s.info.n_lines, s.line_off.data(), s.line_kind.data(), s.pos, s.ref, s.alt, s.flags, s.ex);
        if (s.rc != QM_OK) s.err = "the host path (fgrep -w on the text) failed";
      }
      if (s.rc == QM_OK && !(strict && s.info.n_refused)) {
        s.rc = qm_batch_upload_async(batch, s.batch_v, s.pos, s.ref, s.alt, s.qual, s.flags, copy_stream);
        if (s.rc != QM_OK) s.err = qm_last_error(ctx);   // this thread's message: the caller's thread would not see it
        upload_af();
      }
    });
    int rc = QM_OK;
    wait_patterns();
    for (const auto& t : T) {
      if (rc != QM_OK) break;
      if (t.rc != QM_OK) rc = fail(t.rc, "cannot take the patterns of truth file " + t.path);
      else if (strict && t.info[3] > 0) rc = fail(QM_E_NONCANON, t.path + ": " + std::to_string(t.info[3]) + " truth rows hold NUL or non-ASCII bytes");
    }
    for (int j = 0; j < n_jobs && rc == QM_OK; ++j) {
      const JobState& s = J[(size_t)j];
      if (s.rc != QM_OK) rc = fail(s.rc, std::string("tokenising / uploading failed for ") + jobs[j].vcf_path + (s.err.empty() ? "" : ": " + s.err));
      else if (strict && s.info.n_refused)
        rc = fail(QM_E_NONCANON, std::string(jobs[j].vcf_path) + " line " + std::to_string(s.info.first_refused_line) +
                                     ": a kept line holds NUL or non-ASCII bytes -- the reference's answer for it depends on the locale "
                                     "Python exports to grep; set QM_LENIENT=1 to classify it by its columns");
    }
    if (hipStreamSynchronize(copy_stream) != hipSuccess && rc == QM_OK) rc = fail(QM_E_HIP, "upload failed");
    add_ph(3, now() - t0, trace ? cpu_now() - c0 : 0.0);
    return rc;
  };

  // ---- stage 2: the engine, the class masks back, the three files of every VCF, the rows ----
  auto stage_two = [&](std::string& err) -> int {
    int rc = QM_OK;
    double t0 = now(), c0 = trace ? cpu_now() : 0.0;
    std::vector<int64_t> scal(nrec.size() * QM_N_SCALARS);
    std::vector<uint64_t> roc(nrec.size() * 3 * (size_t)n_bins);
    if (batch) {
      rc = qm_batch_run(batch, nullptr, nullptr);
      if (rc == QM_OK) rc = qm_batch_finish(batch, nullptr);
      if (rc == QM_OK) rc = qm_batch_get_scalars(batch, scal.data());
      if (rc == QM_OK) rc = qm_batch_get_roc(batch, roc.data());
      if (rc == QM_OK && global_dev) {
        // the per-truth-set sums as the engine left them in HBM, row by row ADDED into the caller's layout: what a multi-GPU
        // caller all-reduces (device to device: the counters never visit the host)
        void* src = nullptr;
        rc = qm_batch_global_device(batch, &src);
        const size_t roww = 3 * (size_t)n_bins;
        for (size_t k = 0; k < T.size() && rc == QM_OK; ++k) {
          if (slot_of_truth[k] < 0 || T[k].tid < 0) continue;
          rc = qm_device_add_u64(ctx, (uint64_t*)global_dev + (size_t)slot_of_truth[k] * roww, (const uint64_t*)src + (size_t)T[k].tid * roww, (int64_t)roww);
        }
      }
      if (rc != QM_OK) err = qm_last_error(ctx);
      // the passes, on the columns, masks and truth keys the classification leaves in HBM; the one that fails sets err
      const PassCtx pc{ctx, batch, n_jobs, jobs, J, T, nrec.size(), ext, nthr, dict};
      if (rc == QM_OK) rc = motifs_pass(pc, P, err);
      if (rc == QM_OK) rc = profile_pass(pc, P.pa, err);
      if (rc == QM_OK) rc = strata_pass(pc, P.sa, err);
      if (rc == QM_OK) rc = boot_pass(pc, P.ba, err);
      if (rc == QM_OK) rc = truthside_pass(pc, P.ts, err);
      if (rc == QM_OK) rc = votes_pass(pc, P.va, err);
      if (rc == QM_OK) rc = nearmiss_pass(pc, P.nm, err);
      if (rc == QM_OK) rc = context_pass(pc, P, err);
      if (rc == QM_OK) rc = normalize_pass(pc, P, err);
      if (rc == QM_OK) rc = atomize_pass(pc, P, err);
      if (rc == QM_OK) rc = types_pass(pc, P.ty, err);
      if (rc == QM_OK) rc = haplo_pass(pc, P.hp, err);
      if (rc == QM_OK) rc = hapsub_pass(pc, P.hs, err);
      if (rc == QM_OK) rc = rroc_pass(pc, P.rr, n_bins, err);
      if (rc == QM_OK) rc = ladder_pass(pc, P.ld, err);
      if (rc == QM_OK) rc = ltypes_pass(pc, P.lt, err);
      if (rc == QM_OK) rc = surface_pass(pc, P.sf, err);
    }
    add_ph(4, now() - t0, trace ? cpu_now() - c0 : 0.0);
    t0 = now(); c0 = trace ? cpu_now() : 0.0;
    for (int j = 0; j < n_jobs && rc == QM_OK; ++j) {
      JobState& s = J[(size_t)j];
      if (jobs[j].pure && !(P.wants_profile(j) && P.pa->points_out && P.pa->points_out[j])) continue;   // (a pure-strain job's masks: for its points file only)
      rc = qm_batch_get_masks(batch, s.batch_v, s.kept, s.tp);
      if (rc != QM_OK) err = qm_last_error(ctx);
    }
    add_ph(5, now() - t0, trace ? cpu_now() - c0 : 0.0);
    if (copy_stream) { (void)hipStreamDestroy(copy_stream); copy_stream = nullptr; }
    if (rc != QM_OK) return rc;
    t0 = now(); c0 = trace ? cpu_now() : 0.0;
    struct WTask { int j, select; const char* path; bool pure; };
    std::vector<WTask> W;
    for (int j = 0; j < n_jobs; ++j) {
      if (jobs[j].pure) { W.push_back({j, 0, jobs[j].filtered_out, true}); W.push_back({j, 0, jobs[j].fp_out, true}); }   // cp filtered fp (:33-36)
      else { W.push_back({j, 0, jobs[j].filtered_out, false}); W.push_back({j, 1, jobs[j].tp_out, false}); W.push_back({j, 2, jobs[j].fp_out, false}); }
    }
    if (P.pa && P.pa->points_out) {   // the data frames R plots
      const qm_profile_args* pa = P.pa;
      std::vector<int> pj;
      for (int j = 0; j < n_jobs; ++j) if (P.wants_profile(j) && pa->points_out[j]) pj.push_back(j);
      std::vector<int> prc(pj.size(), QM_OK);
      parallel_for((int)pj.size(), nthr, [&](int k) { prc[(size_t)k] = write_points_file(pa->points_out[pj[(size_t)k]], J[(size_t)pj[(size_t)k]]); });
      for (size_t k = 0; k < pj.size(); ++k)
        if (prc[k] != QM_OK) { err = std::string("cannot write ") + pa->points_out[pj[k]]; return prc[k]; }
    }
    std::vector<int> wrc(W.size(), QM_OK);
    parallel_for((int)W.size(), nthr, [&](int k) {
      const WTask& w = W[(size_t)k];
      const JobState& s = J[(size_t)w.j];
      // pure-strain samples never reach the device: kept = the A2 filter's verdict, which the tokenizer left in the flags
      wrc[(size_t)k] = qm_host_write_masks(w.path, s.vcf.p, s.vcf.n, s.info.n_lines, s.line_off.data(), s.line_kind.data(),
                                           w.pure ? nullptr : s.kept, w.pure ? nullptr : s.tp, s.flags, w.select);
    });
    for (size_t k = 0; k < W.size(); ++k)
      if (wrc[k] != QM_OK) { err = std::string("cannot write ") + W[k].path; return wrc[k]; }
    add_ph(6, now() - t0, trace ? cpu_now() - c0 : 0.0);
    // per-VCF rows
    for (int j = 0; j < n_jobs; ++j) {
      const JobState& s = J[(size_t)j];
      int64_t hk = 0, hk_tp = 0;
      for (int64_t i = 0; i < s.info.n_lines; ++i) { hk += s.line_kind[(size_t)i] == QM_LINE_HEADER_KEPT || s.line_kind[(size_t)i] == QM_LINE_HEADER_KEPT_TP; hk_tp += s.line_kind[(size_t)i] == QM_LINE_HEADER_KEPT_TP; }
      if (stats) {
        qm_file_stats& o = stats[j];
        memset(&o, 0, sizeof o);
        o.n_lines = s.info.n_lines; o.n_refused = s.info.n_refused; o.header_kept = hk; o.header_kept_tp = hk_tp; o.host_decided = s.ex[0]; o.r_hostile = s.info.n_r_hostile;
        if (jobs[j].pure) {
          int64_t np = 0;
          for (int64_t r = 0; r < s.n_data; ++r) np += s.flags[r] & QM_F_PASS;
          o.scalars[QM_S_NPASS] = np; o.scalars[QM_S_FP_LINES] = np; o.scalars[QM_S_SORTED] = 1; o.scalars[QM_S_NREC] = s.n_data;
        } else {
          memcpy(o.scalars, &scal[(size_t)s.batch_v * QM_N_SCALARS], sizeof o.scalars);
          // R keys a line by the TEXT of POS / REF / ALT; for lines without a comparable key the device counted distinct
          // (carried pos, ref, alt) instead: swap those for the text keys (qm_vcf_hostpath)
          o.scalars[QM_S_FP_R] += s.ex[4] - s.ex[2];
          o.scalars[QM_S_TP_R] += s.ex[3];
          o.genomediff = T[(size_t)s.truth].counts[0];
        }
      }
      if (roc_out) {
        uint64_t* dst = roc_out + (size_t)j * 3 * (size_t)n_bins;
        if (jobs[j].pure) memset(dst, 0, sizeof(uint64_t) * 3 * (size_t)n_bins);
        else memcpy(dst, &roc[(size_t)s.batch_v * 3 * (size_t)n_bins], sizeof(uint64_t) * 3 * (size_t)n_bins);
      }
    }
    // done: the batch, the mappings and the line tables go
    t0 = now(); c0 = trace ? cpu_now() : 0.0;
    if (batch) { qm_batch_destroy(batch); batch = nullptr; }
    const double t1 = now();
    parallel_for(n_jobs, nthr, [&](int j) { JobState tmp = std::move(J[(size_t)j]); (void)tmp; });   // unmap / free in parallel
    if (getenv("QM_FILES_TRACE")) fprintf(stderr, "release: batch destroy %.2f ms, unmap + free %.2f ms\n", (t1 - t0) * 1e3, (now() - t1) * 1e3);
    add_ph(7, now() - t0, trace ? cpu_now() - c0 : 0.0);
    return QM_OK;
  };

  std::string msg;
  int rc = stage_one();
  if (rc != QM_OK) msg = qm_last_error(ctx);
  else rc = stage_two(msg);
  cleanup();
  if (rc != QM_OK) return fail(rc, msg);
  if (phase_seconds) memcpy(phase_seconds, ph, sizeof ph);
  if (trace)   // (process-wide CPU time between a phase's two clock readings: phases that run beside each other share it)
    fprintf(stderr, "cpu seconds: map_count %.3f truth_beside %.3f batch_layout %.3f tokenise_upload %.3f engine %.3f masks_back %.3f write %.3f release %.3f\n",
            phc[0], phc[1], phc[2], phc[3], phc[4], phc[5], phc[6], phc[7]);
  return QM_OK;
}
