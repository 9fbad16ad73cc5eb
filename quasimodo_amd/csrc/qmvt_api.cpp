// qmvt_api.cpp -- C ABI of libqmvt.so (include/qmvt.h): the error message and the ids of the binary, contexts, truth sets,
// genomes, strata sets, resident batches up to qm_batch_run, the getters, the passes over a finished batch, the one-shot entry
// points, FP overlap.  Host side of the HIP engine; the text tokenizer/writers live in qmvt_host.cpp, VCFs found out of order
// and qm_batch_finish in qmvt_finish.cpp, the collective in qmvt_comm.cpp.
//
// There is deliberately no CPU implementation of the classification here: every
// compute entry point needs a HIP device and fails loudly without one.
#include "qmvt_batch.h"

static thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

void qm_set_error(const char* msg) { g_err = msg ? msg : ""; }   // for the other translation units of the library

extern "C" int qm_abi_version(void) { return QM_ABI_VERSION; }
#ifndef QM_KERNELS_ID
#define QM_KERNELS_ID "unknown"
#endif
#ifndef QM_BUILD_ID
#define QM_BUILD_ID "unknown"
#endif
// also findable in the file without loading it (quasimodo_amd/_lib.py: embedded_ids)
extern "C" const char qm_build_marker[] = "@(#)qmvt-ids kernels=" QM_KERNELS_ID " build=" QM_BUILD_ID ";";
extern "C" const char* qm_kernels_id(void) { return QM_KERNELS_ID; }
extern "C" const char* qm_build_id(void) { return QM_BUILD_ID; }
extern "C" const char* qm_last_error(qm_ctx*) { return g_err.c_str(); }

extern "C" int qm_init(int device_id, qm_ctx** out) {
  if (!out) return fail(QM_E_INVAL, "qm_init: out is NULL");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(QM_E_NODEVICE, "qm_init: no HIP device (%s); the engine has no CPU fallback", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
  if (device_id < 0 || device_id >= n) return fail(QM_E_INVAL, "qm_init: device %d out of range (have %d)", device_id, n);
  e = hipSetDevice(device_id);
  if (e != hipSuccess) return fail(QM_E_NODEVICE, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
  qm_ctx* c = new qm_ctx();
  c->dev = device_id;
  e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking);
  if (e != hipSuccess) { if (c->stream) (void)hipStreamDestroy(c->stream); delete c; return fail(QM_E_NODEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
  *out = c;
  return QM_OK;
}

void qm_pipeline_ctx_destroyed(qm_ctx* ctx);   // qmvt_pipeline.cpp: the context's page-locked buffers

extern "C" void qm_destroy(qm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->dev);
  qm_pipeline_ctx_destroyed(c);
  for (auto& t : c->truths) {
    (void)hipFree(t.d_keys); (void)hipFree(t.d_tidx);
    (void)hipFree(t.d_xkeys); (void)hipFree(t.d_xref); (void)hipFree(t.d_xalt); (void)hipFree(t.d_xtidx);
  }
  (void)hipFree(c->d_truths);
  for (auto& g : c->genomes) { (void)hipFree(g.d_words); (void)hipFree(g.d_ctab); (void)hipFree(g.d_cgen); }
  for (auto& t : c->strata) { (void)hipFree(t.d_bp); (void)hipFree(t.d_masks); (void)hipFree(t.d_cidx); }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  if (c->aux) (void)hipStreamDestroy(c->aux);
  delete c;
}

// ---------------------------------------------------------------------------
// truth sets
// ---------------------------------------------------------------------------
static int upload_truth_table(qm_ctx* c) {
  const int n = (int)c->truths.size();
  if (n > c->d_truths_cap) {
    (void)hipFree(c->d_truths);
    c->d_truths_cap = std::max(16, n * 2);
    DALLOC(c->d_truths, (size_t)c->d_truths_cap);
  }
  std::vector<TruthDev> h((size_t)n);
  for (int i = 0; i < n; ++i) {
    h[i].keys = c->truths[i].d_keys; h[i].tidx = c->truths[i].d_tidx;
    h[i].shift = c->truths[i].shift; h[i].nb = c->truths[i].nb; h[i].n = c->truths[i].n;
    h[i].xkeys = c->truths[i].d_xkeys; h[i].xref = c->truths[i].d_xref; h[i].xalt = c->truths[i].d_xalt;
    h[i].xtidx = c->truths[i].d_xtidx; h[i].xshift = c->truths[i].xshift; h[i].xnb = c->truths[i].xnb; h[i].xn = c->truths[i].xn;
  }
  HIPCHK(hipMemcpy(c->d_truths, h.data(), sizeof(TruthDev) * (size_t)n, hipMemcpyHostToDevice));
  return QM_OK;
}

// coarse position index over sorted keys (pos << 4 | nibble): tidx[b] = first key with pos >= b << shift
static void coarse_index(const std::vector<uint32_t>& keys, int32_t* shift_out, int32_t* nb_out, std::vector<int32_t>& tidx) {
  const uint32_t maxpos = keys.empty() ? 0u : (keys.back() >> 4);
  int shift = 0;
  while ((maxpos >> shift) >= (1u << 16)) ++shift;  // <= 65536 buckets
  const int32_t nb = (int32_t)(maxpos >> shift);
  tidx.assign((size_t)nb + 2, 0);
  size_t j = 0;
  for (int32_t b = 0; b <= nb + 1; ++b) {
    const uint64_t lim = ((uint64_t)b << shift) << 4;
    while (j < keys.size() && (uint64_t)keys[j] < lim) ++j;
    tidx[(size_t)b] = (int32_t)j;
  }
  tidx[(size_t)nb + 1] = (int32_t)keys.size();
  *shift_out = shift;
  *nb_out = nb;
}

struct XEntry { uint32_t key; int32_t ref, alt; };

// keys: single-base entries; xe: every valid entry (allele-extended batches join against these)
static void truth_free(Truth& t) {
  (void)hipFree(t.d_keys); (void)hipFree(t.d_tidx);
  (void)hipFree(t.d_xkeys); (void)hipFree(t.d_xref); (void)hipFree(t.d_xalt); (void)hipFree(t.d_xtidx);
  t = Truth();
}

static int truth_build(std::vector<uint32_t>& keys, std::vector<XEntry>& xe, Truth& t) {
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  t.n = (int64_t)keys.size();
  std::vector<int32_t> tidx;
  coarse_index(keys, &t.shift, &t.nb, tidx);
  DALLOC(t.d_keys, keys.size());
  DALLOC(t.d_tidx, tidx.size());
  if (!keys.empty()) HIPCHK(hipMemcpy(t.d_keys, keys.data(), keys.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(t.d_tidx, tidx.data(), tidx.size() * 4, hipMemcpyHostToDevice));
  {
    auto lt = [](const XEntry& a, const XEntry& b) {
      if (a.key != b.key) return a.key < b.key;
      if (a.ref != b.ref) return a.ref < b.ref;
      return a.alt < b.alt;
    };
    auto eq = [](const XEntry& a, const XEntry& b) { return a.key == b.key && a.ref == b.ref && a.alt == b.alt; };
    std::sort(xe.begin(), xe.end(), lt);
    xe.erase(std::unique(xe.begin(), xe.end(), eq), xe.end());
    t.xn = (int64_t)xe.size();
    std::vector<uint32_t> xk(xe.size());
    std::vector<int32_t> xr(xe.size()), xa(xe.size()), xtidx;
    for (size_t i = 0; i < xe.size(); ++i) { xk[i] = xe[i].key; xr[i] = xe[i].ref; xa[i] = xe[i].alt; }
    coarse_index(xk, &t.xshift, &t.xnb, xtidx);
    DALLOC(t.d_xkeys, xk.size());
    DALLOC(t.d_xref, xk.size());
    DALLOC(t.d_xalt, xk.size());
    DALLOC(t.d_xtidx, xtidx.size());
    if (!xk.empty()) {
      HIPCHK(hipMemcpy(t.d_xkeys, xk.data(), xk.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(t.d_xref, xr.data(), xr.size() * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(t.d_xalt, xa.data(), xa.size() * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(t.d_xtidx, xtidx.data(), xtidx.size() * 4, hipMemcpyHostToDevice));
  }
  return QM_OK;
}

static int truth_from_keys(qm_ctx* c, std::vector<uint32_t>& keys, std::vector<XEntry>& xe, int* truth_id) {
  Truth t;
  int rc = truth_build(keys, xe, t);
  if (rc != QM_OK) { truth_free(t); return rc; }   // nothing half-built stays behind
  int slot = -1;
  for (size_t i = 0; i < c->truths.size(); ++i) if (c->truths[i].released) { slot = (int)i; break; }
  if (slot >= 0) {   // a released slot is reused: long-lived contexts do not grow without bound
    t.gen = c->truths[(size_t)slot].gen + 1;
    c->truths[(size_t)slot] = t;
  } else {
    c->truths.push_back(t);
    slot = (int)c->truths.size() - 1;
  }
  rc = upload_truth_table(c);
  if (rc != QM_OK) {
    const uint32_t g = c->truths[(size_t)slot].gen;
    truth_free(c->truths[(size_t)slot]);
    if (slot == (int)c->truths.size() - 1 && g == 0) c->truths.pop_back();
    else { c->truths[(size_t)slot].released = true; c->truths[(size_t)slot].gen = g; }
    return rc;
  }
  if (truth_id) *truth_id = slot;
  return QM_OK;
}

extern "C" int qm_truth_release(qm_ctx* c, int truth_id) {
  if (!c || truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released)
    return fail(QM_E_INVAL, "qm_truth_release: no live truth set %d", truth_id);
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipStreamSynchronize(c->stream));   // nothing of this context still reads it
  const uint32_t g = c->truths[(size_t)truth_id].gen;
  truth_free(c->truths[(size_t)truth_id]);
  c->truths[(size_t)truth_id].released = true;
  c->truths[(size_t)truth_id].gen = g;
  return upload_truth_table(c);
}

// ---------------------------------------------------------------------------
// genomes
// ---------------------------------------------------------------------------
extern "C" int qm_genome_load(qm_ctx* c, const uint8_t* seq, int64_t len, int* genome_id) {
  if (!c || !seq || !genome_id || len < 1) return fail(QM_E_INVAL, "qm_genome_load: bad arguments");
  if (len > (int64_t)QM_POS_LIMIT) return fail(QM_E_RANGE, "qm_genome_load: %lld bases, more than 2^28", (long long)len);
  HIPCHK(hipSetDevice(c->dev));
  uint8_t code[256];
  memset(code, (int)GENOME_NOBASE, sizeof code);
  code['A'] = code['a'] = 0; code['C'] = code['c'] = 1; code['G'] = code['g'] = 2; code['T'] = code['t'] = 3;
  const size_t nw = (size_t)(len / 8 + 2);
  std::vector<uint32_t> w(nw, 0xffffffffu);   // no base past the end
  for (int64_t i = 0; i < len; i += 8) {
    uint32_t x = 0xffffffffu;
    for (int64_t k = 0; k < 8 && i + k < len; ++k) x = (x & ~(15u << (4 * k))) | ((uint32_t)code[seq[i + k]] << (4 * k));
    w[(size_t)(i / 8)] = x;
  }
  Genome g;
  g.len = len;
  DALLOC(g.d_words, nw);
  hipError_t e = hipMemcpy(g.d_words, w.data(), nw * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(g.d_words); return fail(QM_E_HIP, "qm_genome_load: hipMemcpy: %s", hipGetErrorString(e)); }
  int slot = -1;
  for (size_t i = 0; i < c->genomes.size(); ++i) if (c->genomes[i].released) { slot = (int)i; break; }
  if (slot >= 0) c->genomes[(size_t)slot] = g;
  else { c->genomes.push_back(g); slot = (int)c->genomes.size() - 1; }
  *genome_id = slot;
  return QM_OK;
}

extern "C" int qm_genome_release(qm_ctx* c, int genome_id) {
  if (!c || genome_id < 0 || genome_id >= (int)c->genomes.size() || c->genomes[(size_t)genome_id].released)
    return fail(QM_E_INVAL, "qm_genome_release: no live genome %d", genome_id);
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipDeviceSynchronize());   // a motif pass may still read it on a stream of the caller's
  Genome& g = c->genomes[(size_t)genome_id];
  (void)hipFree(g.d_words);
  (void)hipFree(g.d_ctab);
  (void)hipFree(g.d_cgen);
  g = Genome();
  g.released = true;
  return QM_OK;
}

// the sequence-context table of a genome
static int context_params(const char* who, int32_t w, int32_t ng) {
  if (w < 0 || w > QM_CX_MAX_HALF_WINDOW) return fail(QM_E_INVAL, "%s: half window %d (0 to %d)", who, w, QM_CX_MAX_HALF_WINDOW);
  if (ng < 1 || ng > QM_CX_MAX_GC_BINS) return fail(QM_E_INVAL, "%s: %d GC bins (1 to %d)", who, ng, QM_CX_MAX_GC_BINS);
  return QM_OK;
}
// The table of live genome `gid` for (w, ng): the cached one, or built on `st` and waited for, so that every later stream may read
// it.  A rebuild first drains the device: a pass on another stream may still read the table it replaces.  *built: a kernel ran.
static int context_table(qm_ctx* c, int gid, int32_t w, int32_t ng, hipStream_t st, bool* built) {
  Genome& g = c->genomes[(size_t)gid];
  if (g.cx_w == w && g.cx_ng == ng) return QM_OK;
  if (g.cx_w >= 0) HIPCHK(hipDeviceSynchronize());
  g.cx_w = g.cx_ng = -1;
  if (!g.d_ctab) DALLOC(g.d_ctab, (size_t)((g.len + 15) / 16 * 16));
  if (!g.d_cgen) DALLOC(g.d_cgen, (size_t)CX_MAX_CELLS);
  HIPCHK(hipMemsetAsync(g.d_cgen, 0, CX_MAX_CELLS * 8, st));
  ContextBuildParams P;
  P.words = g.d_words; P.tab = g.d_ctab; P.gen = g.d_cgen;
  P.len = (int32_t)g.len; P.w = w; P.ng = ng; P.pad = 0;
  launch_context_build(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  g.cx_w = w; g.cx_ng = ng;
  *built = true;
  return QM_OK;
}
extern "C" int qm_genome_context(qm_ctx* c, int genome_id, int32_t w, int32_t ng, uint8_t* cells, uint64_t* gen) {
  if (!c || genome_id < 0 || genome_id >= (int)c->genomes.size() || c->genomes[(size_t)genome_id].released)
    return fail(QM_E_INVAL, "qm_genome_context: no live genome %d", genome_id);
  int rc = context_params("qm_genome_context", w, ng);
  if (rc != QM_OK) return rc;
  HIPCHK(hipSetDevice(c->dev));
  bool built = false;
  rc = context_table(c, genome_id, w, ng, c->stream, &built);
  if (rc != QM_OK) return rc;
  const Genome& g = c->genomes[(size_t)genome_id];
  if (cells) HIPCHK(hipMemcpy(cells, g.d_ctab, (size_t)g.len, hipMemcpyDeviceToHost));
  if (gen) HIPCHK(hipMemcpy(gen, g.d_cgen, (size_t)(16 * ng + 1) * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}

// ---------------------------------------------------------------------------
// strata sets
// ---------------------------------------------------------------------------
extern "C" int qm_strata_load(qm_ctx* c, int n_strata, const int64_t* offsets, const int32_t* start, const int32_t* end, int* strata_id) {
  if (!c || !offsets || !strata_id) return fail(QM_E_INVAL, "qm_strata_load: bad arguments");
  if (n_strata < 1 || n_strata > QM_STRATA_MAX) return fail(QM_E_INVAL, "qm_strata_load: %d strata (1 to %d)", n_strata, QM_STRATA_MAX);
  if (offsets[0] != 0) return fail(QM_E_INVAL, "qm_strata_load: offsets[0] must be 0");
  for (int s = 0; s < n_strata; ++s)
    if (offsets[s + 1] < offsets[s]) return fail(QM_E_INVAL, "qm_strata_load: offsets step backwards at stratum %d", s);
  if (offsets[n_strata] > 0 && (!start || !end)) return fail(QM_E_INVAL, "qm_strata_load: NULL intervals");
  // per stratum: the union of its intervals as closed 1-based runs [start + 1, end]; every run toggles its bit at its first
  // position and behind its last (a run that ends at INT32_MAX is never closed)
  std::vector<std::pair<int64_t, uint32_t>> tog;
  std::vector<std::pair<int32_t, int32_t>> iv;
  for (int s = 0; s < n_strata; ++s) {
    iv.clear();
    for (int64_t i = offsets[s]; i < offsets[s + 1]; ++i) {
      if (start[i] < 0 || end[i] <= start[i])
        return fail(QM_E_INVAL, "qm_strata_load: stratum %d, interval %lld: (%d, %d) (need 0 <= start < end)", s, (long long)(i - offsets[s]), start[i], end[i]);
      iv.emplace_back(start[i], end[i]);
    }
    std::sort(iv.begin(), iv.end());
    for (size_t i = 0; i < iv.size();) {
      const int32_t a = iv[i].first;
      int32_t e = iv[i].second;
      size_t k = i + 1;
      while (k < iv.size() && iv[k].first <= e) { e = std::max(e, iv[k].second); ++k; }   // overlapping or touching
      tog.emplace_back((int64_t)a + 1, 1u << s);
      tog.emplace_back((int64_t)e + 1, 1u << s);
      i = k;
    }
  }
  std::sort(tog.begin(), tog.end());
  Strata t;
  t.n_strata = n_strata;
  t.bp.push_back(INT32_MIN);
  t.masks.push_back(0u);
  uint32_t cur = 0u;
  for (size_t i = 0; i < tog.size();) {
    const int64_t p = tog[i].first;
    for (; i < tog.size() && tog[i].first == p; ++i) cur ^= tog[i].second;
    if (p > (int64_t)INT32_MAX) break;
    if (cur == t.masks.back()) continue;
    if ((int64_t)t.bp.size() >= (int64_t)QM_STRATA_MAX_SEGMENTS)
      return fail(QM_E_LIMIT, "qm_strata_load: more than %d segments", QM_STRATA_MAX_SEGMENTS);
    t.bp.push_back((int32_t)p);
    t.masks.push_back(cur);
  }
  const size_t m = t.bp.size();
  HIPCHK(hipSetDevice(c->dev));
  std::vector<int32_t> cidx;
  if (m > (size_t)QM_STRATA_LDS_SEGMENTS) {
    // cells of 1 << shift positions from INT32_MIN: about 16 per segment (the positions of a genome fill 1/16 of int32), 2^16 .. 2^22
    int lg = 0;
    while (((size_t)1 << lg) < m) ++lg;
    lg = std::min(22, std::max(16, lg + 4));
    t.shift = 32 - lg;
    const int64_t ncell = (int64_t)1 << lg;
    cidx.resize((size_t)ncell + 1);
    size_t i = 0;
    for (int64_t cell = 0; cell < ncell; ++cell) {
      const int64_t first = (int64_t)INT32_MIN + (cell << t.shift);
      while (i + 1 < m && (int64_t)t.bp[i + 1] <= first) ++i;
      cidx[(size_t)cell] = (int32_t)i;
    }
    cidx[(size_t)ncell] = (int32_t)(m - 1);
  }
  int rc = dalloc(&t.d_bp, m);
  if (rc == QM_OK) rc = dalloc(&t.d_masks, m);
  if (rc == QM_OK && !cidx.empty()) rc = dalloc(&t.d_cidx, cidx.size());
  hipError_t e = hipSuccess;
  if (rc == QM_OK) {
    e = hipMemcpy(t.d_bp, t.bp.data(), m * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t.d_masks, t.masks.data(), m * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !cidx.empty()) e = hipMemcpy(t.d_cidx, cidx.data(), cidx.size() * 4, hipMemcpyHostToDevice);
  }
  if (rc != QM_OK || e != hipSuccess) {
    (void)hipFree(t.d_bp); (void)hipFree(t.d_masks); (void)hipFree(t.d_cidx);
    return rc != QM_OK ? rc : fail(QM_E_HIP, "qm_strata_load: hipMemcpy: %s", hipGetErrorString(e));
  }
  int slot = -1;
  for (size_t i = 0; i < c->strata.size(); ++i) if (c->strata[i].released) { slot = (int)i; break; }
  if (slot >= 0) c->strata[(size_t)slot] = std::move(t);
  else { c->strata.push_back(std::move(t)); slot = (int)c->strata.size() - 1; }
  *strata_id = slot;
  return QM_OK;
}

static const Strata* strata_live(qm_ctx* c, int id) {
  return (c && id >= 0 && id < (int)c->strata.size() && !c->strata[(size_t)id].released) ? &c->strata[(size_t)id] : nullptr;
}

extern "C" int qm_strata_info(qm_ctx* c, int strata_id, int64_t* info) {
  const Strata* t = strata_live(c, strata_id);
  if (!t || !info) return fail(QM_E_INVAL, "qm_strata_info: no live strata set %d", strata_id);
  info[0] = t->n_strata;
  info[1] = (int64_t)t->bp.size();
  return QM_OK;
}

extern "C" int qm_strata_segments(qm_ctx* c, int strata_id, int32_t* breakpoints, uint32_t* masks) {
  const Strata* t = strata_live(c, strata_id);
  if (!t || !breakpoints || !masks) return fail(QM_E_INVAL, "qm_strata_segments: no live strata set %d", strata_id);
  memcpy(breakpoints, t->bp.data(), t->bp.size() * 4);
  memcpy(masks, t->masks.data(), t->masks.size() * 4);
  return QM_OK;
}

extern "C" int qm_strata_release(qm_ctx* c, int strata_id) {
  if (!strata_live(c, strata_id)) return fail(QM_E_INVAL, "qm_strata_release: no live strata set %d", strata_id);
  HIPCHK(hipSetDevice(c->dev));
  HIPCHK(hipDeviceSynchronize());   // a pass may still read it on a stream of the caller's
  Strata& t = c->strata[(size_t)strata_id];
  (void)hipFree(t.d_bp); (void)hipFree(t.d_masks); (void)hipFree(t.d_cidx);
  t = Strata();
  t.released = true;
  return QM_OK;
}

extern "C" int qm_truth_load(qm_ctx* c, const int32_t* pos, const int32_t* ref, const int32_t* alt, int64_t n, int* truth_id) {
  if (!c) return fail(QM_E_INVAL, "qm_truth_load: ctx is NULL");
  if (n < 0 || (n > 0 && (!pos || !ref || !alt))) return fail(QM_E_INVAL, "qm_truth_load: bad arguments");
  HIPCHK(hipSetDevice(c->dev));
  std::vector<uint32_t> keys;
  std::vector<XEntry> xe;
  keys.reserve((size_t)n);
  xe.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    if (!allele_valid(ref[i]) || !allele_valid(alt[i])) continue;  // can never match a kept line
    if ((uint32_t)pos[i] >= (uint32_t)QM_POS_LIMIT)
      return fail(QM_E_RANGE, "qm_truth_load: position %d of row %lld outside [0, 2^28)", pos[i], (long long)i);
    const uint32_t key = ((uint32_t)pos[i] << 4) | allele_nib(ref[i], alt[i]);
    xe.push_back(XEntry{key, ref[i], alt[i]});
    if ((uint32_t)(ref[i] | alt[i]) < 4u) keys.push_back(key);   // single-base: what the reference's pattern list holds
  }
  return truth_from_keys(c, keys, xe, truth_id);
}

extern "C" int qm_truth_synth_ext(qm_ctx* c, int64_t L, int64_t T, uint64_t tseed, int indel_pct, int* truth_id) {
  if (!c) return fail(QM_E_INVAL, "qm_truth_synth: ctx is NULL");
  if (T <= 0 || L <= 0 || L % T != 0 || L >= QM_POS_LIMIT) return fail(QM_E_INVAL, "qm_truth_synth: need T | L and L < 2^28");
  if (indel_pct < 0 || indel_pct > 100) return fail(QM_E_INVAL, "qm_truth_synth: indel_pct must be 0..100");
  HIPCHK(hipSetDevice(c->dev));
  std::vector<uint32_t> keys;
  std::vector<XEntry> xe((size_t)T);
  keys.reserve((size_t)T);
  for (int64_t j = 0; j < T; ++j) {
    int32_t p, r, a;
    synth_truth(L, T, tseed, j, &p, &r, &a, indel_pct);
    const uint32_t key = ((uint32_t)p << 4) | allele_nib(r, a);
    xe[(size_t)j] = XEntry{key, r, a};
    if ((uint32_t)(r | a) < 4u) keys.push_back(key);
  }
  int tid = -1;
  int rc = truth_from_keys(c, keys, xe, &tid);
  if (rc != QM_OK) return rc;
  Truth& t = c->truths[(size_t)tid];
  t.synthetic = true; t.syn_L = L; t.syn_T = T; t.syn_seed = tseed; t.syn_pct = indel_pct;
  if (truth_id) *truth_id = tid;
  return QM_OK;
}
extern "C" int qm_truth_synth(qm_ctx* c, int64_t L, int64_t T, uint64_t tseed, int* truth_id) {
  return qm_truth_synth_ext(c, L, T, tseed, 0, truth_id);
}

extern "C" int qm_truth_size(qm_ctx* c, int truth_id, int64_t* n_unique) {
  if (!c || truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released || !n_unique) return fail(QM_E_INVAL, "qm_truth_size: bad arguments");
  *n_unique = c->truths[(size_t)truth_id].n;
  return QM_OK;
}
extern "C" int qm_truth_size_ext(qm_ctx* c, int truth_id, int64_t* n_unique) {
  if (!c || truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released || !n_unique) return fail(QM_E_INVAL, "qm_truth_size_ext: bad arguments");
  *n_unique = c->truths[(size_t)truth_id].xn;
  return QM_OK;
}
extern "C" int qm_truth_count(qm_ctx* c) { return c ? (int)c->truths.size() : 0; }

// ---------------------------------------------------------------------------
// batches
// ---------------------------------------------------------------------------
void build_layout(const int64_t* n_records, const int32_t* truth_ids, int n_vcf, Layout& L) {
  L.vcfs.assign((size_t)n_vcf, VcfDesc());
  L.spans.clear();
  L.tile_vcf.clear();
  int64_t off = 0;
  L.n_total = 0;
  L.max_n = 0;
  for (int v = 0; v < n_vcf; ++v) {
    VcfDesc& d = L.vcfs[(size_t)v];
    d.off = off;
    d.n = n_records[v];
    d.truth = truth_ids[v];
    d.tile0 = (int32_t)L.tile_vcf.size();
    d.ntiles = (int32_t)((d.n + K1_TILE - 1) / K1_TILE);
    d.span0 = (int32_t)L.spans.size();
    d.nspans = (d.ntiles + SPAN_TILES - 1) / SPAN_TILES;
    d.pad = 0;
    for (int t = 0; t < d.ntiles; ++t) L.tile_vcf.push_back(v);
    for (int s = 0; s < d.nspans; ++s) {
      SpanDesc sd;
      sd.vcf = v;
      sd.tile0 = d.tile0 + s * SPAN_TILES;
      sd.begin = d.off + (int64_t)s * SPAN_TILES * K1_TILE;
      sd.end = std::min(d.off + d.n, sd.begin + (int64_t)SPAN_TILES * K1_TILE);
      sd.voff = d.off; sd.vn = (int32_t)d.n; sd.truth = d.truth;
      L.spans.push_back(sd);
    }
    off += (d.n + VCF_ALIGN - 1) / VCF_ALIGN * VCF_ALIGN;
    L.n_total += d.n;
    L.max_n = std::max(L.max_n, d.n);
  }
  L.n_pad = off + K1_TILE;  // the last tile's vector loads may run past its VCF
}

bool memo_on() {   // read at every run / finish: bench.py times a batch with and without its memory in one process
  const char* e = getenv("QM_MEMO");
  return !e || atoi(e) != 0;
}
void forget_known(qm_batch* b, int v) {   // v < 0: every VCF
  if (!b->posor_seen.empty()) { if (v < 0) std::fill(b->posor_seen.begin(), b->posor_seen.end(), 0u); else b->posor_seen[(size_t)v] = 0u; }
  if (!b->known_nbk.empty()) { if (v < 0) std::fill(b->known_nbk.begin(), b->known_nbk.end(), 0u); else b->known_nbk[(size_t)v] = 0u; }
  if (b->known.empty() || b->n_known == 0) return;
  if (v < 0) { std::fill(b->known.begin(), b->known.end(), (uint8_t)0); b->n_known = 0; b->known_dirty = true; return; }
  if (b->known[(size_t)v]) { b->known[(size_t)v] = 0; --b->n_known; b->known_dirty = true; }
}

void batch_free(qm_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->ctx->dev);
  if (b->sub) { batch_free(b->sub); b->sub = nullptr; }
  if (b->h_summary) (void)hipHostFree(b->h_summary);
  if (b->h_mgen) (void)hipHostFree(b->h_mgen);
  for (PassState& p : b->pass) {
    if (p.done) (void)hipEventDestroy(p.done);
    for (auto& e : p.mark) if (e) (void)hipEventDestroy(e);
  }
  for (auto& r : b->ev) for (auto& e : r) if (e) (void)hipEventDestroy(e);
  for (auto& e : b->ev_sync) if (e) (void)hipEventDestroy(e);
  if (b->ev_join) (void)hipEventDestroy(b->ev_join);
  if (b->ev_flags) (void)hipEventDestroy(b->ev_flags);
  delete b;   // the device arrays go with it
}

// ---- the passes of a batch still in flight (include/qmvt.h at qm_batch_run) ----
// Orders what follows behind every pass of the batch still in flight, on whatever stream it was enqueued: `st` waits for the passes'
// done events (wait_host: the host does).  hit_readers: only the passes that read the hit bitmaps (READS: the readers of P_TRUTH).
// The wait list of everything that rewrites what passes read is the table of passes itself: no pass can be missing from it.  A
// done event exists once its pass has been called: a batch that never ran a pass makes no HIP call here.
static int wait_passes(qm_batch* b, hipStream_t st, bool wait_host, bool hit_readers = false) {
  for (int id = 0; id < N_PASSES; ++id) {
    const hipEvent_t e = b->pass[id].done;
    if (!e || (hit_readers && read_row(id, P_TRUTH) < 0)) continue;
    if (wait_host) HIPCHK(hipEventSynchronize(e));
    else HIPCHK(hipStreamWaitEvent(st, e, 0));
  }
  return QM_OK;
}

int upload_layout(qm_batch* b) {
  const Layout& L = b->L;
  HIPCHK(hipMemcpy(b->d_vcfs, L.vcfs.data(), sizeof(VcfDesc) * L.vcfs.size(), hipMemcpyHostToDevice));
  if (!L.spans.empty()) HIPCHK(hipMemcpy(b->d_spans, L.spans.data(), sizeof(SpanDesc) * L.spans.size(), hipMemcpyHostToDevice));
  if (!L.tile_vcf.empty()) HIPCHK(hipMemcpy(b->d_tile_vcf, L.tile_vcf.data(), 4 * L.tile_vcf.size(), hipMemcpyHostToDevice));
  return QM_OK;
}

int batch_alloc(qm_ctx* c, int n_vcf, const int64_t* n_records, const int32_t* truth_ids, int n_bins, qm_batch** out,
                bool packed, bool packed_alleles, bool alleles) {
  qm_batch* b = new qm_batch();
  b->ctx = c;
  b->n_vcf = n_vcf;
  b->n_bins = n_bins;
  b->h_afmark.assign((size_t)n_vcf, (uint8_t)0);
  build_layout(n_records, truth_ids, n_vcf, b->L);
  const Layout& L = b->L;
  const size_t nspans = L.spans.size(), ntiles = L.tile_vcf.size();
  const size_t np = (size_t)L.n_pad;
  const size_t nt = std::max<size_t>(1, (size_t)c->truths.size());
  b->n_truth = (int)nt;
  for (int v = 0; v < n_vcf; ++v) {
    const std::pair<int, uint32_t> tg(truth_ids[v], c->truths[(size_t)truth_ids[v]].gen);
    if (std::find(b->truth_gens.begin(), b->truth_gens.end(), tg) == b->truth_gens.end()) b->truth_gens.push_back(tg);
  }
  int rc = QM_OK;
  auto A = [&](auto& buf, size_t n) { if (rc == QM_OK) rc = buf.grow((int64_t)n, &b->dev_bytes); };
  if (packed) {
    A(b->pkey, np); A(b->pinf, np);
    if (packed_alleles) { A(b->ref, np); A(b->alt, np); }   // sorted copies of the allele codes
  } else {
    A(b->pos, np); A(b->ref, np); A(b->alt, np); A(b->qual, np); A(b->flags, np);
    if (!alleles) A(b->anib, np);
  }
  A(b->mask_pass, np / 64 + 64); A(b->mask_tp, np / 64 + 64); A(b->idx, np);
  A(b->tile_tp, ntiles); A(b->tile_fp, ntiles); A(b->tile_tp_off, ntiles + SPAN_TILES); A(b->tile_fp_off, ntiles + SPAN_TILES); A(b->vcf_tot, (size_t)n_vcf * 2);
  A(b->span_hist, nspans * SPAN_HIST_WORDS); A(b->span_scal, nspans * 8); A(b->vcf_flags, (size_t)n_vcf); A(b->vcf_posor, (size_t)n_vcf);
  A(b->roc, (size_t)n_vcf * 3 * (size_t)n_bins); A(b->global_acc, nt * 3 * (size_t)n_bins); A(b->scalars, (size_t)n_vcf * 8);
  A(b->d_vcfs, (size_t)n_vcf); A(b->d_spans, nspans); A(b->d_tile_vcf, ntiles); A(b->cls_scratch, (size_t)L.max_n);
  if (rc == QM_OK) rc = upload_layout(b);
  auto create_event = [&](hipEvent_t& e) {
    if (rc == QM_OK && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) rc = fail(QM_E_HIP, "hipEventCreate failed");
  };
  for (auto& e : b->ev_sync) create_event(e);
  create_event(b->ev_join);
  create_event(b->ev_flags);
  if (rc == QM_OK && !packed) {
    // padding lanes are masked in the kernels, but keep the columns defined.  On the context's
    // stream (hipMemset on the null stream would not be ordered before work on a non-blocking stream).
    hipError_t e = hipMemsetAsync(b->flags, 0, np, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->pos, 0, np * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->ref, 0, np * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->alt, 0, np * 4, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(b->qual, 0, np * 4, c->stream);
    if (e == hipSuccess && b->anib) e = hipMemsetAsync(b->anib, 0, np, c->stream);   // = allele_byte(0, 0)
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(QM_E_HIP, "hipMemset: %s", hipGetErrorString(e));
  }
  if (rc == QM_OK && !packed) {   // (the scratch batches of the sort path are finalized without it)
    void* h = nullptr;
    void* d = nullptr;
    // (QM_NO_MIRRORS=1, tests: as if the mapping had failed -- the flags come back by copies, every chunk is looked at before its last kernels)
    if (!getenv("QM_NO_MIRRORS") && hipHostMalloc(&h, 64 + 16 * (size_t)std::max(n_vcf, 1), hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&d, h, 0) == hipSuccess) {
      b->h_summary = static_cast<uint32_t*>(h);
      b->d_summary = static_cast<uint32_t*>(d);
      memset(h, 0, 64 + 16 * (size_t)std::max(n_vcf, 1));   // [16 words: the summary][n_vcf flags][n_vcf position bits][n_vcf bucket-row flags][n_vcf highest buckets]: k_finalize's host-mapped mirrors
    } else {   // not fatal: qm_batch_finish then reads the flags back every time
      if (h) (void)hipHostFree(h);
      (void)hipGetLastError();
    }
  }
  if (rc != QM_OK) { batch_free(b); return rc; }
  *out = b;
  return QM_OK;
}

extern "C" int qm_batch_create_ext(qm_ctx* c, int n_vcf, const int64_t* n_records, const int32_t* truth_id_per_vcf, int n_bins,
                                   unsigned mode, qm_batch** out) {
  if (!c || !out || n_vcf <= 0 || !n_records || !truth_id_per_vcf) return fail(QM_E_INVAL, "qm_batch_create: bad arguments");
  if (mode & ~(unsigned)QM_BATCH_ALLELES) return fail(QM_E_INVAL, "qm_batch_create_ext: unknown mode bits 0x%x", mode);
  if (n_bins < 1 || n_bins > QM_MAX_BINS) return fail(QM_E_INVAL, "qm_batch_create: n_bins must be 1..256");
  *out = nullptr;
  for (int v = 0; v < n_vcf; ++v) {
    if (n_records[v] < 0 || n_records[v] > 0x7fffff00ll) return fail(QM_E_INVAL, "qm_batch_create: VCF %d has %lld records", v, (long long)n_records[v]);
    if (truth_id_per_vcf[v] < 0 || truth_id_per_vcf[v] >= (int)c->truths.size() || c->truths[(size_t)truth_id_per_vcf[v]].released)
      return fail(QM_E_INVAL, "qm_batch_create: VCF %d names truth set %d (have %zu)", v, truth_id_per_vcf[v], c->truths.size());
  }
  HIPCHK(hipSetDevice(c->dev));
  int rc = batch_alloc(c, n_vcf, n_records, truth_id_per_vcf, n_bins, out, false, false, (mode & QM_BATCH_ALLELES) != 0);
  if (rc == QM_OK) (*out)->ext = (mode & QM_BATCH_ALLELES) != 0;
  return rc;
}
extern "C" int qm_batch_create(qm_ctx* c, int n_vcf, const int64_t* n_records, const int32_t* truth_id_per_vcf, int n_bins,
                               qm_batch** out) {
  return qm_batch_create_ext(c, n_vcf, n_records, truth_id_per_vcf, n_bins, 0u, out);
}

extern "C" void qm_batch_destroy(qm_batch* b) { batch_free(b); }
extern "C" int64_t qm_batch_device_bytes(qm_batch* b) { return b ? b->dev_bytes : 0; }
extern "C" int qm_batch_n_truth(qm_batch* b) { return b ? b->n_truth : 0; }

extern "C" int qm_batch_upload(qm_batch* b, int v, const int32_t* pos, const int32_t* ref, const int32_t* alt, const float* qual,
                               const uint8_t* flags) {
  if (!b || v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_upload: bad arguments");
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n == 0) return QM_OK;
  if (!pos || !ref || !alt || !qual || !flags) return fail(QM_E_INVAL, "qm_batch_upload: NULL column");
  HIPCHK(hipSetDevice(b->ctx->dev));
  const int rcw = wait_passes(b, nullptr, true);   // a pass still in flight reads the columns
  if (rcw != QM_OK) return rcw;
  const size_t n = (size_t)d.n;
  HIPCHK(hipMemcpy(b->pos + d.off, pos, n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->ref + d.off, ref, n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->alt + d.off, alt, n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->qual + d.off, qual, n * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->flags + d.off, flags, n, hipMemcpyHostToDevice));
  if (b->anib) {   // the allele bytes from the codes just copied, complete when this returns (as the copies are)
    launch_allele_byte(b->ref + d.off, b->alt + d.off, b->anib + d.off, d.n, b->ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
  }
  b->ran = b->finished = false;
  b->h_afmark[(size_t)v] = 0;   // the frequencies belonged to the records just replaced
  forget_known(b, v);
  return QM_OK;
}

// The same from page-locked host memory (hipHostMalloc / hipHostRegister), asynchronous on `stream` (NULL = the
// context's own stream): the copies of one VCF overlap the tokenising of the next.
extern "C" int qm_batch_upload_async(qm_batch* b, int v, const int32_t* pos, const int32_t* ref, const int32_t* alt, const float* qual,
                                     const uint8_t* flags, void* stream) {
  if (!b || v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_upload_async: bad arguments");
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n == 0) return QM_OK;
  if (!pos || !ref || !alt || !qual || !flags) return fail(QM_E_INVAL, "qm_batch_upload_async: NULL column");
  HIPCHK(hipSetDevice(b->ctx->dev));
  hipStream_t st = stream ? (hipStream_t)stream : b->ctx->stream;
  const int rcw = wait_passes(b, st, false);   // a pass still in flight reads the columns
  if (rcw != QM_OK) return rcw;
  const size_t n = (size_t)d.n;
  HIPCHK(hipMemcpyAsync(b->pos + d.off, pos, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->ref + d.off, ref, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->alt + d.off, alt, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->qual + d.off, qual, n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(b->flags + d.off, flags, n, hipMemcpyHostToDevice, st));
  if (b->anib) {   // the allele bytes, queued behind the copies on the same stream
    launch_allele_byte(b->ref + d.off, b->alt + d.off, b->anib + d.off, d.n, st);
    HIPCHK(hipGetLastError());
  }
  b->ran = b->finished = false;
  b->h_afmark[(size_t)v] = 0;   // the frequencies belonged to the records just replaced
  forget_known(b, v);
  return QM_OK;
}

static uint64_t gcd64(uint64_t a, uint64_t b) { while (b) { uint64_t t = a % b; a = b; b = t; } return a; }

extern "C" int qm_batch_synth(qm_batch* b, const qm_synth_cfg* cfg) {
  if (!b || !cfg) return fail(QM_E_INVAL, "qm_batch_synth: bad arguments");
  const Layout& L = b->L;
  for (const VcfDesc& d : L.vcfs) {
    if (d.n <= 0 || cfg->genome_len % d.n != 0) return fail(QM_E_INVAL, "qm_batch_synth: records per VCF must divide genome_len");
    if ((cfg->genome_len / cfg->truth_n) % (cfg->genome_len / d.n) != 0)
      return fail(QM_E_INVAL, "qm_batch_synth: VCF stratum width must divide the truth stratum width");
  }
  if (cfg->truth_n <= 0 || cfg->genome_len % cfg->truth_n != 0 || cfg->genome_len >= QM_POS_LIMIT)
    return fail(QM_E_INVAL, "qm_batch_synth: need truth_n | genome_len < 2^28");
  HIPCHK(hipSetDevice(b->ctx->dev));
  SynthParams S;
  S.vcfs = b->d_vcfs; S.pos = b->pos; S.ref = b->ref; S.alt = b->alt; S.qual = b->qual; S.flags = b->flags; S.anib = b->anib;
  S.genome_len = cfg->genome_len; S.truth_n = cfg->truth_n; S.truth_seed = cfg->truth_seed; S.seed = cfg->seed;
  S.per_vcf_truth = 0;
  if (cfg->truth_seed == QM_SYNTH_TRUTH_PER_VCF) {
    // every VCF against the synthetic truth set it was assigned at qm_batch_create (configs[4]: VCF v uses truth v mod 3)
    for (const VcfDesc& d : L.vcfs) {
      const Truth& t = b->ctx->truths[(size_t)d.truth];
      if (!t.synthetic || t.syn_L != cfg->genome_len || t.syn_T != cfg->truth_n || t.syn_pct != cfg->indel_pct || t.syn_seed > 0x7fffffffull)
        return fail(QM_E_INVAL, "qm_batch_synth: truth set %d was not made by qm_truth_synth_ext with this genome_len / truth_n / indel_pct", d.truth);
    }
    for (VcfDesc& d : b->L.vcfs) d.pad = (int32_t)b->ctx->truths[(size_t)d.truth].syn_seed;
    int rc = upload_layout(b);
    if (rc != QM_OK) return rc;
    S.per_vcf_truth = 1;
  }
  S.shuffled = cfg->shuffled;
  if (cfg->shuffled < 0) return fail(QM_E_INVAL, "qm_batch_synth: shuffled must be 0, 1 or a number of runs");
  if (cfg->shuffled > 1)
    for (const VcfDesc& d : L.vcfs) if (d.n > 0 && d.n < cfg->shuffled) return fail(QM_E_INVAL, "qm_batch_synth: %d runs need at least as many records per VCF", cfg->shuffled);
  S.indel_pct = cfg->indel_pct;
  if (cfg->indel_pct < 0 || cfg->indel_pct > 100) return fail(QM_E_INVAL, "qm_batch_synth: indel_pct must be 0..100");
  if (cfg->indel_pct > 0 && !b->ext) return fail(QM_E_INVAL, "qm_batch_synth: indel_pct > 0 needs an allele-extended batch");
  // slot i holds generated record (i * a + b) mod n, a coprime to every n in the batch
  uint64_t a = 2654435761ull;
  for (;;) {
    bool ok = true;
    for (const VcfDesc& d : L.vcfs) if (gcd64(a, (uint64_t)d.n) != 1) { ok = false; break; }
    if (ok) break;
    a += 2;
  }
  S.perm_a = a; S.perm_b = 12345;
  const int rcw = wait_passes(b, b->ctx->stream, false);   // a pass still in flight reads the columns
  if (rcw != QM_OK) return rcw;
  launch_synth(S, b->n_vcf, L.max_n, b->ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  b->ran = b->finished = false;
  std::fill(b->h_afmark.begin(), b->h_afmark.end(), (uint8_t)0);
  forget_known(b, -1);
  return QM_OK;
}

ClassifyParams classify_params(qm_batch* b) {
  ClassifyParams P;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.qual = b->qual; P.flags = b->flags; P.anib = b->anib;
  P.pkey = b->pkey; P.pinf = b->pinf;
  P.spans = b->d_spans; P.vcfs = b->d_vcfs; P.truths = b->ctx->d_truths;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp; P.tile_tp = b->tile_tp; P.tile_fp = b->tile_fp;
  P.span_hist = b->span_hist; P.span_scal = b->span_scal; P.n_bins = b->n_bins;
  P.ext = b->ext ? 1 : 0;
  P.span_base = 0;
  P.zero_acc = nullptr; P.zero_words = 0;
  P.known = nullptr;
  return P;
}
FinalizeParams finalize_params(qm_batch* b, uint64_t* global) {
  FinalizeParams F;
  F.vcfs = b->d_vcfs; F.truths = b->ctx->d_truths; F.span_hist = b->span_hist; F.span_scal = b->span_scal;
  F.tile_tp = b->tile_tp; F.tile_fp = b->tile_fp; F.tile_tp_off = b->tile_tp_off; F.tile_fp_off = b->tile_fp_off; F.vcf_tot = b->vcf_tot;
  F.roc = b->roc; F.scalars = b->scalars; F.vcf_flags = b->vcf_flags; F.vcf_posor = b->vcf_posor; F.global_acc = global; F.n_bins = b->n_bins; F.ext = b->ext ? 1 : 0;
  F.vcf_base = 0;
  F.parts = 3;
  F.known = nullptr;
  F.all_hist = nullptr;
  F.row_cap = nullptr;
  F.host_flags = nullptr; F.host_aux = nullptr;
  F.chunk_bad = nullptr; F.row_cap_limit = 0u; F.lazy_unsorted = 0;
  return F;
}
CompactParams compact_params(qm_batch* b) {
  CompactParams C;
  C.vcfs = b->d_vcfs; C.spans = b->d_spans; C.mask_pass = b->mask_pass; C.mask_tp = b->mask_tp;
  C.tile_fp = b->tile_fp; C.tile_tp_off = b->tile_tp_off; C.tile_fp_off = b->tile_fp_off; C.vcf_tot = b->vcf_tot; C.idx = b->idx;
  C.vcf_flags = b->vcf_flags; C.skip_unsorted = 1; C.span_base = 0; C.span_scal = b->span_scal;
  return C;
}

extern "C" int qm_batch_set_timing(qm_batch* b, int on) {
  if (!b) return fail(QM_E_INVAL, "qm_batch_set_timing: NULL batch");
  HIPCHK(hipSetDevice(b->ctx->dev));
  b->timing = on != 0;
  b->timed_runs = 0;   // averages restart
  if (b->timing && !b->ev[0][0]) for (auto& r : b->ev) for (auto& e : r) HIPCHK(hipEventCreate(&e));
  return QM_OK;
}

extern "C" int qm_batch_run(qm_batch* b, void* stream, void* global_dev) {
  if (!b) return fail(QM_E_INVAL, "qm_batch_run: NULL batch");
  qm_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  uint64_t* g = global_dev ? (uint64_t*)global_dev : b->global_acc;
  for (const auto& tg : b->truth_gens)
    if (tg.first >= (int)c->truths.size() || c->truths[(size_t)tg.first].released || c->truths[(size_t)tg.first].gen != tg.second)
      return fail(QM_E_STATE, "qm_batch_run: truth set %d was released after the batch was created", tg.first);
  const size_t gbytes = (size_t)b->n_truth * 3 * (size_t)b->n_bins * 8;   // as allocated at batch creation
  // a pass still in flight, on whatever stream, reads the masks and rows this run rewrites (include/qmvt.h)
  const int rcw = wait_passes(b, st, false);
  if (rcw != QM_OK) return rcw;
  hipEvent_t* ev = b->ev[b->timed_runs % qm_batch::EV_RING];
  const bool T = b->timing;
  if (T) HIPCHK(hipEventRecord(ev[0], st));
  // VCFs an earlier finish found out of order, columns unchanged since: their spans return at once (qm_batch: known)
  const bool use_known = memo_on() && b->n_known > 0;
  if (use_known && (b->known_dirty || !b->d_known)) {
    const int rc = b->d_known.grow(b->n_vcf, &b->dev_bytes);
    if (rc != QM_OK) return rc;
    HIPCHK(hipMemcpy(b->d_known, b->known.data(), (size_t)b->n_vcf, hipMemcpyHostToDevice));
    b->known_dirty = false;
  }
  b->run_used_known = use_known;
  b->flags_recorded = false;
  const int ns = (int)b->L.spans.size();
  if (use_known && b->n_known == b->n_vcf) {
    // every VCF known to be out of order: the optimistic pass, its k_finalize and its compaction would find and write what the
    // earlier run left (flags, position bits, rows nobody reads) -- only the per-truth sums are cleared
    HIPCHK(hipMemsetAsync(g, 0, gbytes, st));
    if (T) for (int q = 2; q < 7; ++q) HIPCHK(hipEventRecord(ev[q], st));
  } else {
    ClassifyParams P = classify_params(b);
    // k_finalize, behind this launch, adds to the per-truth sums: the first wave of the launch clears them
    if (ns > 0) { P.zero_acc = g; P.zero_words = (int32_t)(gbytes / 8); }
    else HIPCHK(hipMemsetAsync(g, 0, gbytes, st));   // a batch of empty VCFs launches nothing
    if (use_known) P.known = b->d_known;
    if (T) HIPCHK(hipEventRecord(ev[2], st));
    launch_classify_any(P, ns, st);
    if (T) HIPCHK(hipEventRecord(ev[3], st));
    FinalizeParams F = finalize_params(b, g);
    // (no summary word: with the mirrors, qm_batch_finish looks through the VCFs' flag words itself -- and every workgroup of a
    // batch of shuffled VCFs storing to that ONE word of host memory made this kernel 50 us instead of 15: same-address stores
    // to system memory queue up.)
    if (b->d_summary) { F.host_flags = b->d_summary + 16; F.host_aux = b->d_summary + 16 + b->n_vcf; }
    if (use_known) F.known = b->d_known;
    F.lazy_unsorted = 1;
    // The compaction waits only for what it needs of k_finalize -- per-VCF flags and tile offsets -- and the rows (ROC, scalars,
    // per-truth sums: 96 MB of span histograms to sum) go to the second stream beside it.  (Host order: what the compaction --
    // and a first-seen step's look at the flags -- waits for is queued first, the rows' part behind it; it starts beside the
    // compaction either way.)
    F.parts = 1;
    launch_finalize(F, b->n_vcf, st);
    HIPCHK(hipEventRecord(b->ev_flags, st));   // every VCF's flags are written
    b->flags_recorded = true;
    HIPCHK(hipEventRecord(b->ev_sync[0], st));
    if (T) { HIPCHK(hipEventRecord(ev[4], st)); HIPCHK(hipEventRecord(ev[5], st)); }
    launch_compact(compact_params(b), ns, st);
    HIPCHK(hipStreamWaitEvent(c->aux, b->ev_sync[0], 0));
    F.parts = 2;
    launch_finalize(F, b->n_vcf, c->aux);
    HIPCHK(hipEventRecord(b->ev_sync[1], c->aux));
    if (T) HIPCHK(hipEventRecord(ev[6], st));
    HIPCHK(hipStreamWaitEvent(st, b->ev_sync[1], 0));   // the rows of k_finalize
  }
  if (T) { HIPCHK(hipEventRecord(ev[1], st)); b->timed_runs++; }
  HIPCHK(hipGetLastError());
  b->ran = true;
  b->finished = false;
  for (PassState& p : b->pass) p.made = 0;   // every pass's result belongs to the run before
  b->last_global = g;
  return QM_OK;
}

extern "C" int qm_batch_timings(qm_batch* b, float* ms4) {
  if (!b || !ms4 || !b->timing || b->timed_runs == 0) return fail(QM_E_STATE, "qm_batch_timings: timing is off or nothing ran");
  HIPCHK(hipSetDevice(b->ctx->dev));
  const int n = (int)std::min<int64_t>(b->timed_runs, qm_batch::EV_RING);
  double acc[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {   // averages over the latest runs since qm_batch_set_timing(1)
    const int slot = (int)((b->timed_runs - 1 - i) % qm_batch::EV_RING);
    hipEvent_t* ev = b->ev[slot];
    HIPCHK(hipEventSynchronize(ev[1]));
    float t;
    HIPCHK(hipEventElapsedTime(&t, ev[2], ev[3])); acc[0] += t;   // classify
    HIPCHK(hipEventElapsedTime(&t, ev[3], ev[4])); acc[1] += t;   // finalize (the flags' part)
    HIPCHK(hipEventElapsedTime(&t, ev[5], ev[6])); acc[2] += t;   // compact
    HIPCHK(hipEventElapsedTime(&t, ev[0], ev[1])); acc[3] += t;
  }
  for (int k = 0; k < 4; ++k) ms4[k] = (float)(acc[k] / n);
  return QM_OK;
}

// ---- getters ------------------------------------------------------------------
// ---- what the passes over a finished batch share ----
// The truth sets of the batch are the ones it was created with: asked by every pass that reads their keys or the hit bitmaps.
static int truths_live(const qm_batch* b, const char* who) {
  const qm_ctx* c = b->ctx;
  for (const auto& tg : b->truth_gens)
    if (tg.first >= (int)c->truths.size() || c->truths[(size_t)tg.first].released || c->truths[(size_t)tg.first].gen != tg.second)
      return fail(QM_E_STATE, "%s: truth set %d was released after the batch was created", who, tg.first);
  return QM_OK;
}
// Every genome a VCF names (ids[v] >= 0; -1: none) is in range and live.
static int genomes_named(const qm_ctx* c, const char* who, const int32_t* ids, int nv) {
  for (int v = 0; v < nv; ++v) {
    const int gid = ids[v];
    if (gid < -1 || gid >= (int)c->genomes.size()) return fail(QM_E_INVAL, "%s: VCF %d names genome %d (have %zu)", who, v, gid, c->genomes.size());
    if (gid >= 0 && c->genomes[(size_t)gid].released) return fail(QM_E_STATE, "%s: VCF %d names released genome %d", who, v, gid);
  }
  return QM_OK;
}
// One pooled table per truth set that a VCF with a genome names (qm_batch_normalize, qm_batch_haplotypes): tabs[k] is the table of
// truth set tabs[k].truth over genome tabs[k].genome and starts at word tabs[k].off of the pool, words(truth set) long; tab_of[v]
// is the table of VCF v, -1 for a VCF that names no genome.  The VCFs that share a truth set must name one genome (`why`).
struct TruthTab { int truth, genome; size_t first_vcf, off; };
template <typename F>
static int tabs_by_truth(const qm_batch* b, const char* who, const char* why, const int32_t* genome_ids, F&& words, std::vector<TruthTab>* tabs,
                         std::vector<int>* tab_of, size_t* pool_words) {
  tab_of->assign((size_t)b->n_vcf, -1);
  for (size_t v = 0; v < (size_t)b->n_vcf; ++v) {
    const int gid = genome_ids[v], tid = b->L.vcfs[v].truth;
    if (gid < 0) continue;
    size_t k = 0;
    while (k < tabs->size() && (*tabs)[k].truth != tid) ++k;
    if (k == tabs->size()) {
      tabs->push_back(TruthTab{tid, gid, v, *pool_words});
      *pool_words += words(b->ctx->truths[(size_t)tid]);
    } else if ((*tabs)[k].genome != gid) {
      return fail(QM_E_INVAL, "%s: VCF %zu and VCF %zu share truth set %d and name genomes %d and %d (%s)", who, (*tabs)[k].first_vcf, v, tid,
                  (*tabs)[k].genome, gid, why);
    }
    (*tab_of)[v] = (int)k;
  }
  return QM_OK;
}
// A table built once in a pool of its own and read back (qm_truth_normalized, qm_truth_atoms, qm_truth_sites): build(pool, &src)
// lays the table out in the pool, enqueues its build on the context's stream and says where the `bytes` for `out` start.
template <typename F>
static int build_and_read(qm_ctx* c, const char* who, size_t pool_words, void* out, size_t bytes, F&& build) {
  uint32_t* pool = nullptr;
  DALLOC(pool, pool_words);
  const void* src = pool;
  const int rc = build(pool, &src);
  hipError_t e = rc == QM_OK ? hipStreamSynchronize(c->stream) : hipSuccess;
  if (rc == QM_OK && e == hipSuccess) e = hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost);
  (void)hipFree(pool);
  if (rc != QM_OK) return rc;
  if (e != hipSuccess) return fail(QM_E_HIP, "%s: %s", who, hipGetErrorString(e));
  return QM_OK;
}
// `rows` device rows of (kept, TP) lines as the caller's rows of (kept, TP, FP = kept - TP)
static int widen_kept_tp(const uint64_t* d_kt, size_t rows, uint64_t* out) {
  std::vector<uint64_t> kt(rows * 2);
  HIPCHK(hipMemcpy(kt.data(), d_kt, kt.size() * 8, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < rows; ++i) {
    out[3 * i] = kt[2 * i];
    out[3 * i + 1] = kt[2 * i + 1];
    out[3 * i + 2] = kt[2 * i] - kt[2 * i + 1];
  }
  return QM_OK;
}

// ---- the state of a pass (PassState, PASSES): how it opens, marks its kernels and closes; how its getters open ----
// How a pass opens: the context's device, the caller's stream or the context's, and the pass's done event -- created at first use,
// waited for on the host afterwards (the previous call of the pass has read its tables and left its outputs).  Then its readers
// (READS): one behind the previous call, maybe on another stream, reads what this call rewrites and may regrow, so it is waited
// for on the host, not only on the stream, and its result belongs to the call before.  OPEN_PASS declares `st` and returns a failure.
static int pass_open(qm_batch* b, PassId id, void* stream, hipStream_t* st) {
  hipEvent_t* ev = &b->pass[id].done;
  HIPCHK(hipSetDevice(b->ctx->dev));
  *st = stream ? (hipStream_t)stream : b->ctx->stream;
  if (!*ev) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(*ev));
  for (const PassRead& r : READS)
    if (r.producer == id && r.forget) {
      if (b->pass[r.reader].done) HIPCHK(hipEventSynchronize(b->pass[r.reader].done));
      b->pass[r.reader].made &= ~r.forget;
    }
  return QM_OK;
}
#define OPEN_PASS(b, id, stream, st) \
  hipStream_t st;                    \
  if (const int rc_ = pass_open(b, id, stream, &st); rc_ != QM_OK) return rc_
// What a reader asks of a pass it reads (READS), in front of its own opening: refused unless the producer made what it needs;
// `flag`: the reader's own flag that asks for this edge, if one does ...
template <PassId READER, PassId PRODUCER>
static int pass_needs(const qm_batch* b, const char* flag = "") {
  constexpr int row = read_row(READER, PRODUCER);
  static_assert(row >= 0, "READS has no such edge");
  if (b->pass[PRODUCER].made & READS[row].need) return QM_OK;
  return fail(QM_E_STATE, "%s: %s%sneeds %s behind the latest %s", PASSES[READER].name, flag, *flag ? " " : "", READS[row].call, PASSES[PRODUCER].since);
}
// ... and, in front of its first kernel that reads it: `st` waits for the producer, on whatever stream it was enqueued.
template <PassId READER, PassId PRODUCER>
static hipError_t pass_wait(qm_batch* b, hipStream_t st) {
  static_assert(read_row(READER, PRODUCER) >= 0, "READS has no such edge");
  return hipStreamWaitEvent(st, b->pass[PRODUCER].done, 0);
}
// In front of the first mark of a call: with qm_batch_set_timing on, the marks of the pass exist from here on (they need timing;
// the done events do without); the call has recorded none yet.
static hipError_t pass_marks(qm_batch* b, PassId id) {
  PassState& p = b->pass[id];
  for (int i = 0; b->timing && i < PASSES[id].marks; ++i)
    if (!p.mark[i]) { const hipError_t e = hipEventCreate(&p.mark[i]); if (e != hipSuccess) return e; }
  p.timed = false;
  return hipSuccess;
}
// Mark i of the pass on `st`, with timing on; the last mark of a pass says that the call recorded them all.
static hipError_t pass_mark(qm_batch* b, PassId id, int i, hipStream_t st) {
  if (!b->timing) return hipSuccess;
  const hipError_t e = hipEventRecord(b->pass[id].mark[i], st);
  if (e == hipSuccess && i == PASSES[id].marks - 1) b->pass[id].timed = true;
  return e;
}
// How a pass closes: its done event behind its last kernel, and what it made.
static hipError_t pass_done(qm_batch* b, PassId id, hipStream_t st, unsigned made) {
  const hipError_t e = hipEventRecord(b->pass[id].done, st);
  if (e == hipSuccess) b->pass[id].made = made;
  return e;
}
// How the getters of a pass open: refused while the pass made nothing behind the latest run, or what else it counts since ...
static int pass_ran(const qm_batch* b, PassId id, const char* who) {
  if (b->pass[id].made) return QM_OK;
  return fail(QM_E_STATE, "%s: no %s behind the latest %s", who, PASSES[id].name, PASSES[id].since);
}
#define NEED_PASS(b, id, who) \
  if (!(b)) return fail(QM_E_INVAL, who ": NULL batch"); \
  if (pass_ran(b, id, who) != QM_OK) return QM_E_STATE
// ... then, behind the checks of their own arguments, the context's device and a wait on the host for the pass.
static hipError_t pass_result(qm_batch* b, PassId id) {
  const hipError_t e = hipSetDevice(b->ctx->dev);
  return e != hipSuccess ? e : hipEventSynchronize(b->pass[id].done);
}
// The qm_batch_*_timings of a pass: the milliseconds between its marks, one value fewer than there are marks.
static int pass_timings(qm_batch* b, PassId id, const char* who, float* ms) {
  if (!b || !ms) return fail(QM_E_INVAL, "%s: NULL", who);
  const int rc = pass_ran(b, id, who);
  if (rc != QM_OK) return rc;
  const PassState& p = b->pass[id];
  if (!p.timed) return fail(QM_E_STATE, "%s: timing is off", who);
  const int n = PASSES[id].marks - 1;
  HIPCHK(hipSetDevice(b->ctx->dev));
  HIPCHK(hipEventSynchronize(p.mark[n]));
  for (int i = 0; i < n; ++i) HIPCHK(hipEventElapsedTime(ms + i, p.mark[i], p.mark[i + 1]));
  return QM_OK;
}
// One group of a pass over the hit bitmaps (G: TruthGroup, VoteGroup): VCFs vcf_ids[group_offsets[g] .. group_offsets[g + 1]), 1 to
// `max` of them, all of one truth set.  Fills t's bitmaps, words, T' and n; per_member(i, v) is the caller's own check of member i.
template <typename G, typename F>
static int walk_hit_group(const qm_batch* b, const char* who, int g, const int32_t* group_offsets, const int32_t* vcf_ids, int max, G& t, F&& per_member) {
  const int32_t o0 = group_offsets[g], o1 = group_offsets[g + 1];
  if (o0 < 0 || o1 - o0 < 1 || o1 - o0 > max) return fail(QM_E_INVAL, "%s: group %d has %d VCFs (1 to %d)", who, g, o1 - o0, max);
  memset(&t, 0, sizeof t);
  t.n = o1 - o0;
  int truth = -1;
  for (int i = 0; i < t.n; ++i) {
    const int v = vcf_ids[o0 + i];
    if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "%s: group %d names VCF %d (the batch has %d)", who, g, v, b->n_vcf);
    const int rc = per_member(i, v);
    if (rc != QM_OK) return rc;
    const int tv = b->L.vcfs[(size_t)v].truth;
    if (i == 0) truth = tv;
    else if (tv != truth) return fail(QM_E_INVAL, "%s: group %d mixes truth sets %d and %d", who, g, truth, tv);
    t.bits[i] = b->d_hits + b->h_hit_off[(size_t)v];
    t.words = b->h_hit_off[(size_t)v + 1] - b->h_hit_off[(size_t)v];
  }
  t.tn = b->h_hit_tn[(size_t)vcf_ids[o0]];   // T' as it was when the bitmaps were sized (qm_batch_truth_hits checked the generations)
  return QM_OK;
}

extern "C" int qm_batch_get_cls(qm_batch* b, int v, uint8_t* out) {
  NEED_FINISHED(b, "qm_batch_get_cls");
  if (v < 0 || v >= b->n_vcf || !out) return fail(QM_E_INVAL, "qm_batch_get_cls: bad arguments");
  HIPCHK(hipSetDevice(b->ctx->dev));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n == 0) return QM_OK;
  launch_masks_to_cls(b->mask_pass, b->mask_tp, d.off, d.n, b->cls_scratch, b->ctx->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, b->cls_scratch, (size_t)d.n, hipMemcpyDeviceToHost, b->ctx->stream));
  HIPCHK(hipStreamSynchronize(b->ctx->stream));
  return QM_OK;
}
// class masks of one VCF as they sit in HBM: bit r of word r / 64 = record r (1 bit per record and mask instead of the
// byte per record of qm_batch_get_cls).  (n + 63) / 64 words each.
extern "C" int qm_batch_get_masks(qm_batch* b, int v, uint64_t* kept, uint64_t* tp) {
  NEED_FINISHED(b, "qm_batch_get_masks");
  if (v < 0 || v >= b->n_vcf || !kept || !tp) return fail(QM_E_INVAL, "qm_batch_get_masks: bad arguments");
  HIPCHK(hipSetDevice(b->ctx->dev));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  const size_t nw = (size_t)((d.n + 63) / 64);
  if (nw) {
    HIPCHK(hipMemcpyAsync(kept, b->mask_pass + (d.off >> 6), nw * 8, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipMemcpyAsync(tp, b->mask_tp + (d.off >> 6), nw * 8, hipMemcpyDeviceToHost, b->ctx->stream));
    HIPCHK(hipStreamSynchronize(b->ctx->stream));
    if (d.n & 63) {   // bits beyond the VCF's last record are not defined on the device
      const uint64_t m = (1ull << (d.n & 63)) - 1ull;
      kept[nw - 1] &= m; tp[nw - 1] &= m;
    }
  }
  return QM_OK;
}
extern "C" int qm_batch_get_idx(qm_batch* b, int v, int32_t* out) {
  NEED_FINISHED(b, "qm_batch_get_idx");
  if (v < 0 || v >= b->n_vcf || !out) return fail(QM_E_INVAL, "qm_batch_get_idx: bad arguments");
  HIPCHK(hipSetDevice(b->ctx->dev));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n) HIPCHK(hipMemcpy(out, b->idx + d.off, (size_t)d.n * 4, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_roc(qm_batch* b, uint64_t* out) {
  NEED_FINISHED(b, "qm_batch_get_roc");
  HIPCHK(hipSetDevice(b->ctx->dev));
  HIPCHK(hipMemcpy(out, b->roc, (size_t)b->n_vcf * 3 * (size_t)b->n_bins * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_scalars(qm_batch* b, int64_t* out) {
  NEED_FINISHED(b, "qm_batch_get_scalars");
  HIPCHK(hipSetDevice(b->ctx->dev));
  HIPCHK(hipMemcpy(out, b->scalars, (size_t)b->n_vcf * 8 * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_global(qm_batch* b, uint64_t* out) {
  NEED_FINISHED(b, "qm_batch_get_global");
  HIPCHK(hipSetDevice(b->ctx->dev));
  HIPCHK(hipMemcpy(out, b->last_global, (size_t)b->n_truth * 3 * (size_t)b->n_bins * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
// the mutation-context spectra of the finished batch
extern "C" int qm_batch_motifs(qm_batch* b, const int32_t* genome_id_per_vcf, void* stream) {
  NEED_FINISHED(b, "qm_batch_motifs");
  if (!genome_id_per_vcf) return fail(QM_E_INVAL, "qm_batch_motifs: NULL genome ids");
  qm_ctx* c = b->ctx;
  int rc = genomes_named(c, "qm_batch_motifs", genome_id_per_vcf, b->n_vcf);
  if (rc != QM_OK) return rc;
  OPEN_PASS(b, P_MOTIFS, stream, st);   // (the previous call's copy has read the page-locked descriptors)
  const size_t nv = (size_t)b->n_vcf;
  // first use: every piece on its own, so that a call that failed half way is completed by the next
  rc = b->d_motifs.grow((int64_t)(nv * MOTIF_ROW_WORDS), &b->dev_bytes);
  if (rc == QM_OK) rc = b->d_mgen.grow((int64_t)nv, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  if (!b->h_mgen) HIPCHK(hipHostMalloc((void**)&b->h_mgen, nv * sizeof(GenomeRef), hipHostMallocDefault));
  for (size_t v = 0; v < nv; ++v) {
    const int gid = genome_id_per_vcf[v];
    b->h_mgen[v] = gid < 0 ? GenomeRef{nullptr, 0} : GenomeRef{c->genomes[(size_t)gid].d_words, c->genomes[(size_t)gid].len};
  }
  HIPCHK(hipMemcpyAsync(b->d_mgen, b->h_mgen, nv * sizeof(GenomeRef), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(b->d_motifs, 0, nv * MOTIF_ROW_WORDS * 8, st));
  MotifParams P;
  P.spans = b->d_spans; P.genomes = b->d_mgen;
  P.pos = b->pos; P.anib = b->anib; P.ref = b->ref; P.alt = b->alt; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  P.out = b->d_motifs;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_motif(P, b->ext, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_done(b, P_MOTIFS, st, 1));
  return QM_OK;
}
extern "C" int qm_batch_get_motifs(qm_batch* b, uint64_t* out) {
  if (!b || !out) return fail(QM_E_INVAL, "qm_batch_get_motifs: bad arguments");
  NEED_PASS(b, P_MOTIFS, "qm_batch_get_motifs");
  HIPCHK(pass_result(b, P_MOTIFS));
  HIPCHK(hipMemcpy(out, b->d_motifs, (size_t)b->n_vcf * MOTIF_ROW_WORDS * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
// the allele-frequency profiles of the finished batch
extern "C" int qm_batch_upload_af(qm_batch* b, int v, const float* af) {
  if (!b || v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_upload_af: bad arguments");
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n > 0 && !af) return fail(QM_E_INVAL, "qm_batch_upload_af: NULL column");
  HIPCHK(hipSetDevice(b->ctx->dev));
  {
    std::lock_guard<std::mutex> g(b->af_mu);
    if (!b->d_af) {   // first use: the column, defined everywhere (lanes past a VCF's last record are loaded and masked)
      const int rc = b->d_af.grow(b->L.n_pad, &b->dev_bytes);
      if (rc != QM_OK) return rc;
      HIPCHK(hipMemsetAsync(b->d_af, 0, (size_t)b->L.n_pad * sizeof(float), b->ctx->stream));   // (on the context's stream, as at create)
      HIPCHK(hipStreamSynchronize(b->ctx->stream));
    }
  }
  if (d.n > 0) {
    const int rcw = wait_passes(b, nullptr, true);   // a pass still in flight reads the frequencies
    if (rcw != QM_OK) return rcw;
    HIPCHK(hipMemcpy(b->d_af + d.off, af, (size_t)d.n * sizeof(float), hipMemcpyHostToDevice));
  }
  b->h_afmark[(size_t)v] = 1;
  return QM_OK;
}
extern "C" int qm_batch_af_profile(qm_batch* b, int32_t window, int32_t n_pos_bins, int32_t n_af_bins, void* stream) {
  NEED_FINISHED(b, "qm_batch_af_profile");
  if (window < 1 || window >= QM_POS_LIMIT || n_pos_bins < 1 || n_af_bins < 1 || (int64_t)n_pos_bins * n_af_bins > QM_AFP_MAX_CELLS)
    return fail(QM_E_INVAL, "qm_batch_af_profile: window %d, %d x %d bins (1 <= window < 2^28, at most %d cells)", window, n_af_bins, n_pos_bins, QM_AFP_MAX_CELLS);
  OPEN_PASS(b, P_AFP, stream, st);   // (the previous pass has read the marks and left the outputs)
  const size_t nv = (size_t)b->n_vcf, cells = (size_t)n_pos_bins * (size_t)n_af_bins;
  int rc = b->d_afgrid.grow((int64_t)(nv * 2 * cells), &b->dev_bytes);
  if (rc == QM_OK) rc = b->d_afextra.grow((int64_t)(nv * 2 * AFP_EXTRA), &b->dev_bytes);
  if (rc == QM_OK) rc = b->d_afmark.grow((int64_t)nv, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  bool any = false;
  for (size_t v = 0; v < nv; ++v) any = any || b->h_afmark[v];
  HIPCHK(hipMemcpy(b->d_afmark, b->h_afmark.data(), nv, hipMemcpyHostToDevice));   // blocking: the marks may change behind the call
  HIPCHK(hipMemsetAsync(b->d_afgrid, 0, nv * 2 * cells * 8, st));
  HIPCHK(hipMemsetAsync(b->d_afextra, 0, nv * 2 * AFP_EXTRA * 8, st));
  if (any) {   // (no mark anywhere: there may be no column at all, and every row is zero)
    AfProfileParams P;
    P.spans = b->d_spans; P.has_af = b->d_afmark;
    P.pos = b->pos; P.af = b->d_af; P.anib = b->anib; P.ref = b->ref; P.alt = b->alt;
    P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
    P.grid = b->d_afgrid; P.extra = b->d_afextra;
    P.n_spans = (int32_t)b->L.spans.size();
    P.window = window; P.n_pos = n_pos_bins; P.n_af = n_af_bins;
    P.div = afp_div((uint32_t)window);
    launch_af_profile(P, b->ext, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_done(b, P_AFP, st, 1));
  b->afp_cells = (int32_t)cells;
  return QM_OK;
}
extern "C" int qm_batch_get_af_profile(qm_batch* b, uint64_t* grid, uint64_t* extra) {
  if (!b || !grid) return fail(QM_E_INVAL, "qm_batch_get_af_profile: bad arguments");
  NEED_PASS(b, P_AFP, "qm_batch_get_af_profile");
  HIPCHK(pass_result(b, P_AFP));
  HIPCHK(hipMemcpy(grid, b->d_afgrid, (size_t)b->n_vcf * 2 * (size_t)b->afp_cells * 8, hipMemcpyDeviceToHost));
  if (extra) HIPCHK(hipMemcpy(extra, b->d_afextra, (size_t)b->n_vcf * 2 * AFP_EXTRA * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
// the counts per stratum of the finished batch
extern "C" int qm_batch_strata(qm_batch* b, int strata_id, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_strata");
  qm_ctx* c = b->ctx;
  const Strata* t = strata_live(c, strata_id);
  if (!t) return fail(QM_E_INVAL, "qm_batch_strata: no live strata set %d", strata_id);
  if (!what || (what & ~(QM_STRATA_RECORDS | QM_STRATA_TRUTH))) return fail(QM_E_INVAL, "qm_batch_strata: what = %u", what);
  if (what & QM_STRATA_TRUTH) {
    if (b->ext) return fail(QM_E_STATE, "qm_batch_strata: allele-extended batches have no truth-side bitmaps (QM_STRATA_RECORDS only)");
    if (pass_needs<P_STRATA, P_TRUTH>(b, "QM_STRATA_TRUTH") != QM_OK) return QM_E_STATE;
    const int rc = truths_live(b, "qm_batch_strata");
    if (rc != QM_OK) return rc;
  }
  OPEN_PASS(b, P_STRATA, stream, st);
  const size_t nv = (size_t)b->n_vcf;
  const int S = t->n_strata;
  b->pass[P_STRATA].made = 0;
  StrataTable tab;
  tab.bp = t->d_bp; tab.masks = t->d_masks; tab.cidx = t->d_cidx;
  tab.m = (int32_t)t->bp.size(); tab.shift = t->shift; tab.n_strata = S; tab.pad = 0;
  if (what & QM_STRATA_RECORDS) {
    const size_t words = nv * (size_t)(S + 2) * 2;
    const int rc = b->d_srec.grow((int64_t)std::max<size_t>(words, 1), &b->dev_bytes);
    if (rc != QM_OK) return rc;
    HIPCHK(hipMemsetAsync(b->d_srec, 0, words * 8, st));
    StrataRecParams P;
    P.spans = b->d_spans; P.pos = b->pos; P.flags = b->flags;
    P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
    P.out = b->d_srec; P.tab = tab;
    P.n_spans = (int32_t)b->L.spans.size();
    launch_strata_records(P, st);
    HIPCHK(hipGetLastError());
  }
  if (what & QM_STRATA_TRUTH) {
    // the planes of every distinct truth set of the batch, one behind the other (T' as the hit bitmaps were sized)
    std::vector<int64_t> plane_off(c->truths.size(), -1);
    int64_t total = 0, max_words = 0;
    for (size_t v = 0; v < nv; ++v) {
      const size_t tid = (size_t)b->L.vcfs[v].truth;
      if (plane_off[tid] >= 0) continue;
      const int64_t w = (b->h_hit_tn[v] + 31) / 32;
      plane_off[tid] = total;
      total += (int64_t)(S + 1) * w;
      max_words = std::max(max_words, w);
    }
    const size_t words = nv * (size_t)(S + 1) * 2;
    int rc = b->d_splanes.grow(std::max<int64_t>(total, 1), &b->dev_bytes);
    if (rc == QM_OK) rc = b->d_srows.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
    if (rc == QM_OK) rc = b->d_stru.grow((int64_t)std::max<size_t>(words, 1), &b->dev_bytes);
    if (rc != QM_OK) return rc;
    std::vector<StrataTruthRow> rows(nv);
    std::vector<uint8_t> done(c->truths.size(), 0);
    HIPCHK(pass_wait<P_STRATA, P_TRUTH>(b, st));   // the hit bitmaps, on whatever stream they were made
    for (size_t v = 0; v < nv; ++v) {
      const size_t tid = (size_t)b->L.vcfs[v].truth;
      const int64_t tn = b->h_hit_tn[v];
      rows[v].planes = b->d_splanes + plane_off[tid];
      rows[v].hits = b->d_hits + b->h_hit_off[v];
      rows[v].words = (tn + 31) / 32;
      if (!done[tid]) {
        done[tid] = 1;
        launch_strata_planes(tab, c->truths[tid].d_keys, tn, b->d_splanes + plane_off[tid], st);
      }
    }
    HIPCHK(hipGetLastError());
    if (nv) HIPCHK(hipMemcpy(b->d_srows, rows.data(), nv * sizeof(StrataTruthRow), hipMemcpyHostToDevice));   // blocking: rows dies here
    HIPCHK(hipMemsetAsync(b->d_stru, 0, words * 8, st));
    launch_strata_truth(b->d_srows, (int)nv, max_words, S, reinterpret_cast<unsigned long long*>(b->d_stru.p), st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_done(b, P_STRATA, st, what));
  b->strata_S = S;
  return QM_OK;
}
extern "C" int qm_batch_get_strata(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_STRATA, "qm_batch_get_strata");
  if ((rec && !(b->pass[P_STRATA].made & QM_STRATA_RECORDS)) || (tru && !(b->pass[P_STRATA].made & QM_STRATA_TRUTH)))
    return fail(QM_E_STATE, "qm_batch_get_strata: the latest qm_batch_strata did not make the %s side", rec && !(b->pass[P_STRATA].made & QM_STRATA_RECORDS) ? "record" : "truth");
  HIPCHK(pass_result(b, P_STRATA));
  const size_t nv = (size_t)b->n_vcf, S = (size_t)b->strata_S;
  if (rec && nv) {
    const int rc = widen_kept_tp(b->d_srec, nv * (S + 2), rec);
    if (rc != QM_OK) return rc;
  }
  if (tru && nv) HIPCHK(hipMemcpy(tru, b->d_stru, nv * (S + 1) * 2 * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
// the counts per sequence-context cell of the finished batch
extern "C" int qm_batch_context(qm_batch* b, const int32_t* genome_id_per_vcf, int32_t w, int32_t ng, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_context");
  if (!genome_id_per_vcf) return fail(QM_E_INVAL, "qm_batch_context: NULL genome ids");
  int rc = context_params("qm_batch_context", w, ng);
  if (rc != QM_OK) return rc;
  if (!what || (what & ~(QM_CX_RECORDS | QM_CX_TRUTH))) return fail(QM_E_INVAL, "qm_batch_context: what = %u", what);
  qm_ctx* c = b->ctx;
  rc = genomes_named(c, "qm_batch_context", genome_id_per_vcf, b->n_vcf);
  if (rc != QM_OK) return rc;
  if (what & QM_CX_TRUTH) {
    if (b->ext) return fail(QM_E_STATE, "qm_batch_context: allele-extended batches have no truth-side bitmaps (QM_CX_RECORDS only)");
    if (pass_needs<P_CONTEXT, P_TRUTH>(b, "QM_CX_TRUTH") != QM_OK) return QM_E_STATE;
    rc = truths_live(b, "qm_batch_context");
    if (rc != QM_OK) return rc;
  }
  OPEN_PASS(b, P_CONTEXT, stream, st);
  const size_t nv = (size_t)b->n_vcf, n_cells = (size_t)(16 * ng + 1);
  b->pass[P_CONTEXT].made = 0;   // from here on the outputs are rewritten
  rc = b->cx_gen.grow((int64_t)std::max<size_t>(nv * n_cells, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->cx_tabs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_CONTEXT));
  b->cx_built = false;
  HIPCHK(pass_mark(b, P_CONTEXT, 0, st));
  std::vector<ContextTab> tabs(nv, ContextTab{nullptr, 0});
  HIPCHK(hipMemsetAsync(b->cx_gen, 0, std::max<size_t>(nv * n_cells, 1) * 8, st));
  for (size_t v = 0; v < nv; ++v) {
    const int gid = genome_id_per_vcf[v];
    if (gid < 0) continue;
    rc = context_table(c, gid, w, ng, st, &b->cx_built);
    if (rc != QM_OK) return rc;
    const Genome& g = c->genomes[(size_t)gid];
    tabs[v] = ContextTab{g.d_ctab, g.len};
    HIPCHK(hipMemcpyAsync(b->cx_gen + v * n_cells, g.d_cgen, n_cells * 8, hipMemcpyDeviceToDevice, st));
  }
  if (nv) HIPCHK(hipMemcpy(b->cx_tabs, tabs.data(), nv * sizeof(ContextTab), hipMemcpyHostToDevice));   // blocking: tabs dies here
  HIPCHK(pass_mark(b, P_CONTEXT, 1, st));
  if (what & QM_CX_RECORDS) {
    const size_t words = nv * (n_cells + 1) * 2;
    rc = b->cx_rec.grow((int64_t)std::max<size_t>(words, 1), &b->dev_bytes);
    if (rc != QM_OK) return rc;
    HIPCHK(hipMemsetAsync(b->cx_rec, 0, words * 8, st));
    ContextRecParams P;
    P.spans = b->d_spans; P.tabs = b->cx_tabs; P.pos = b->pos; P.flags = b->flags;
    P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
    P.out = b->cx_rec;
    P.n_spans = (int32_t)b->L.spans.size(); P.ng = ng;
    launch_context_records(P, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_mark(b, P_CONTEXT, 2, st));
  if (what & QM_CX_TRUTH) {
    const size_t words = nv * n_cells * 2;
    rc = b->cx_tru.grow((int64_t)std::max<size_t>(words, 1), &b->dev_bytes);
    if (rc == QM_OK) rc = b->cx_rows.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
    if (rc != QM_OK) return rc;
    std::vector<ContextTruthRow> rows(nv);
    int64_t max_n = 0;
    for (size_t v = 0; v < nv; ++v) {
      rows[v].keys = c->truths[(size_t)b->L.vcfs[v].truth].d_keys;
      rows[v].hits = b->d_hits + b->h_hit_off[v];
      rows[v].tab = tabs[v].tab;
      rows[v].n = b->h_hit_tn[v];   // T' as the hit bitmaps were sized
      rows[v].len = tabs[v].len;
      max_n = std::max(max_n, rows[v].n);
    }
    HIPCHK(pass_wait<P_CONTEXT, P_TRUTH>(b, st));   // the hit bitmaps, on whatever stream they were made
    if (nv) HIPCHK(hipMemcpy(b->cx_rows, rows.data(), nv * sizeof(ContextTruthRow), hipMemcpyHostToDevice));   // blocking: rows dies here
    HIPCHK(hipMemsetAsync(b->cx_tru, 0, words * 8, st));
    launch_context_truth(b->cx_rows, (int)nv, max_n, ng, reinterpret_cast<unsigned long long*>(b->cx_tru.p), st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_mark(b, P_CONTEXT, 3, st));
  HIPCHK(pass_done(b, P_CONTEXT, st, what));
  b->cx_ng = ng;
  return QM_OK;
}
extern "C" int qm_batch_get_context(qm_batch* b, uint64_t* rec, uint64_t* tru, uint64_t* gen_per_vcf) {
  NEED_PASS(b, P_CONTEXT, "qm_batch_get_context");
  if ((rec && !(b->pass[P_CONTEXT].made & QM_CX_RECORDS)) || (tru && !(b->pass[P_CONTEXT].made & QM_CX_TRUTH)))
    return fail(QM_E_STATE, "qm_batch_get_context: the latest qm_batch_context did not make the %s side", rec && !(b->pass[P_CONTEXT].made & QM_CX_RECORDS) ? "record" : "truth");
  HIPCHK(pass_result(b, P_CONTEXT));
  const size_t nv = (size_t)b->n_vcf, n_cells = (size_t)(16 * b->cx_ng + 1);
  if (rec && nv) {
    const int rc = widen_kept_tp(b->cx_rec, nv * (n_cells + 1), rec);
    if (rc != QM_OK) return rc;
  }
  if (tru && nv) HIPCHK(hipMemcpy(tru, b->cx_tru, nv * n_cells * 2 * 8, hipMemcpyDeviceToHost));
  if (gen_per_vcf && nv) HIPCHK(hipMemcpy(gen_per_vcf, b->cx_gen, nv * n_cells * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_context_timings(qm_batch* b, float* ms3) {
  const int rc = pass_timings(b, P_CONTEXT, "qm_batch_context_timings", ms3);
  if (rc == QM_OK && !b->cx_built) ms3[0] = 0.0f;   // every table was cached
  return rc;
}
// ---- indels and MNPs matched by normal form ----
// The pool words of one table: [claim | spos | sref | salt | sresp][slots], [fpos | fref | falt][xn], stats[2] (8-byte aligned)
static size_t norm_pool_words(int64_t xn, uint32_t slots) {
  return 5 * (size_t)slots + ((3 * (size_t)xn + 1) & ~(size_t)1) + 4;
}
static NormTable norm_table(const Truth& t, const Genome& g, uint32_t* pool, uint32_t slots) {
  NormTable T;
  memset(&T, 0, sizeof T);
  T.words = g.d_words; T.len = g.len;
  T.xkeys = t.d_xkeys; T.xref = t.d_xref; T.xalt = t.d_xalt; T.xn = t.xn;
  T.slots = slots;
  T.claim = pool;
  T.spos = reinterpret_cast<int32_t*>(pool + (size_t)slots);
  T.sref = reinterpret_cast<int32_t*>(pool + 2 * (size_t)slots);
  T.salt = reinterpret_cast<int32_t*>(pool + 3 * (size_t)slots);
  T.sresp = pool + 4 * (size_t)slots;
  uint32_t* e = pool + 5 * (size_t)slots;
  T.fpos = reinterpret_cast<int32_t*>(e);
  T.fref = reinterpret_cast<int32_t*>(e + (size_t)t.xn);
  T.falt = reinterpret_cast<int32_t*>(e + 2 * (size_t)t.xn);
  T.stats = reinterpret_cast<unsigned long long*>(e + ((3 * (size_t)t.xn + 1) & ~(size_t)1));
  return T;
}
// Builds the table on `st` (the pool words start at a multiple of 8 bytes).
static int norm_build(const NormTable& T, hipStream_t st) {
  HIPCHK(hipMemsetAsync(T.claim, 0, (size_t)T.slots * 4, st));
  HIPCHK(hipMemsetAsync(T.sresp, 0, (size_t)T.slots * 4, st));
  HIPCHK(hipMemsetAsync(T.stats, 0, 16, st));
  launch_norm_truth(T, st);
  HIPCHK(hipGetLastError());
  return QM_OK;
}
extern "C" int qm_batch_normalize(qm_batch* b, const int32_t* genome_id_per_vcf, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_normalize");
  if (!genome_id_per_vcf) return fail(QM_E_INVAL, "qm_batch_normalize: NULL genome ids");
  if (what & ~QM_NORM_COLUMNS) return fail(QM_E_INVAL, "qm_batch_normalize: what = %u", what);
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_normalize: a single-base batch holds no indels or MNPs to normalise (create the batch with QM_BATCH_ALLELES)");
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  int rc = genomes_named(c, "qm_batch_normalize", genome_id_per_vcf, b->n_vcf);
  if (rc == QM_OK) rc = truths_live(b, "qm_batch_normalize");
  if (rc != QM_OK) return rc;
  // one table per truth set: the VCFs that share one must name one genome
  std::vector<TruthTab> pairs;
  std::vector<int> pair_of;
  size_t pool_words = 0, bit_words = 0;
  rc = tabs_by_truth(b, "qm_batch_normalize", "a normalised truth set belongs to one genome", genome_id_per_vcf,
                     [](const Truth& t) { return norm_pool_words(t.xn, norm_slots(t.xn)); }, &pairs, &pair_of, &pool_words);
  if (rc != QM_OK) return rc;
  for (size_t v = 0; v < nv; ++v)
    if (pair_of[v] >= 0) bit_words += 2 * (size_t)(norm_slots(c->truths[(size_t)b->L.vcfs[v].truth].xn) / 32u);
  OPEN_PASS(b, P_NORM, stream, st);
  b->pass[P_NORM].made = 0;   // from here on the outputs are rewritten (pass_open: the sweep and the ladder are done and forgotten)
  const size_t np = (size_t)b->L.n_pad;
  rc = b->nz_pool.grow((int64_t)std::max<size_t>(pool_words, 2), &b->dev_bytes);
  if (rc == QM_OK) rc = b->nz_bits.grow((int64_t)std::max<size_t>(bit_words, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->nz_vcfs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->nz_rec.grow((int64_t)std::max<size_t>(nv * NORM_R_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->nz_tru.grow((int64_t)std::max<size_t>(nv * NORM_T_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->nz_cls.grow((int64_t)np, &b->dev_bytes);
  if (rc == QM_OK && (what & QM_NORM_COLUMNS)) rc = b->nz_cols.grow((int64_t)(4 * np), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_NORM));
  HIPCHK(pass_mark(b, P_NORM, 0, st));
  std::vector<NormTable> tabs(pairs.size());
  for (size_t k = 0; k < pairs.size(); ++k) {
    const Truth& t = c->truths[(size_t)pairs[k].truth];
    tabs[k] = norm_table(t, c->genomes[(size_t)pairs[k].genome], b->nz_pool + pairs[k].off, norm_slots(t.xn));
    rc = norm_build(tabs[k], st);
    if (rc != QM_OK) return rc;
  }
  std::vector<NormVcf> vcfs(std::max<size_t>(nv, 1));
  memset(vcfs.data(), 0, vcfs.size() * sizeof(NormVcf));
  b->nz_has.assign(nv, 0);
  size_t bo = 0;
  for (size_t v = 0; v < nv; ++v) {
    if (pair_of[v] < 0) continue;
    const size_t w = tabs[(size_t)pair_of[v]].slots / 32u;
    vcfs[v].t = tabs[(size_t)pair_of[v]];
    vcfs[v].found = b->nz_bits + bo;
    vcfs[v].found_eq = b->nz_bits + bo + w;
    bo += 2 * w;
    b->nz_has[v] = 1;
  }
  if (nv) HIPCHK(hipMemcpy(b->nz_vcfs, vcfs.data(), nv * sizeof(NormVcf), hipMemcpyHostToDevice));   // blocking: vcfs dies here
  HIPCHK(hipMemsetAsync(b->nz_bits, 0, std::max<size_t>(bit_words, 1) * 4, st));
  HIPCHK(hipMemsetAsync(b->nz_rec, 0, std::max<size_t>(nv * NORM_R_COLS, 1) * 8, st));
  HIPCHK(hipMemsetAsync(b->nz_tru, 0, std::max<size_t>(nv * NORM_T_COLS, 1) * 8, st));
  HIPCHK(hipMemsetAsync(b->nz_cls, 0, np, st));
  HIPCHK(pass_mark(b, P_NORM, 1, st));
  NormRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.vcfs = b->nz_vcfs;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  P.cls = b->nz_cls;
  if (what & QM_NORM_COLUMNS) { P.npos = b->nz_cols; P.nref = b->nz_cols + np; P.nalt = b->nz_cols + 2 * np; P.nrow = b->nz_cols + 3 * np; }
  P.rec = b->nz_rec;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_norm_records(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_NORM, 2, st));
  launch_norm_found(b->nz_vcfs, (int)nv, b->nz_tru, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_NORM, 3, st));
  HIPCHK(pass_done(b, P_NORM, st, 1u | what));
  return QM_OK;
}
extern "C" int qm_batch_get_normalize(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_NORM, "qm_batch_get_normalize");
  HIPCHK(pass_result(b, P_NORM));
  const size_t nv = (size_t)b->n_vcf;
  if (rec && nv) HIPCHK(hipMemcpy(rec, b->nz_rec, nv * NORM_R_COLS * 8, hipMemcpyDeviceToHost));
  if (tru && nv) HIPCHK(hipMemcpy(tru, b->nz_tru, nv * NORM_T_COLS * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_normalized(qm_batch* b, int v, int32_t* pos, int32_t* ref, int32_t* alt, uint8_t* cls, int32_t* truth_row) {
  NEED_PASS(b, P_NORM, "qm_batch_get_normalized");
  if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_normalized: VCF %d (the batch has %d)", v, b->n_vcf);
  if (!b->nz_has[(size_t)v]) return fail(QM_E_STATE, "qm_batch_get_normalized: VCF %d named no genome in the latest qm_batch_normalize", v);
  if ((pos || ref || alt || truth_row) && !(b->pass[P_NORM].made & QM_NORM_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_get_normalized: the latest qm_batch_normalize did not keep the columns (QM_NORM_COLUMNS)");
  HIPCHK(pass_result(b, P_NORM));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n == 0) return QM_OK;
  const size_t np = (size_t)b->L.n_pad, n = (size_t)d.n;
  if (cls) HIPCHK(hipMemcpy(cls, b->nz_cls + d.off, n, hipMemcpyDeviceToHost));
  int32_t* const outs[4] = {pos, ref, alt, truth_row};
  for (size_t k = 0; k < 4; ++k)
    if (outs[k]) HIPCHK(hipMemcpy(outs[k], b->nz_cols + k * np + d.off, n * 4, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_normalize_timings(qm_batch* b, float* ms3) {
  return pass_timings(b, P_NORM, "qm_batch_normalize_timings", ms3);
}
extern "C" int qm_truth_entries(qm_ctx* c, int truth_id, int32_t* pos, int32_t* ref, int32_t* alt, int64_t capacity, int64_t* n_out) {
  if (!c || !n_out || capacity < 0) return fail(QM_E_INVAL, "qm_truth_entries: bad arguments");
  if (truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released)
    return fail(QM_E_INVAL, "qm_truth_entries: no live truth set %d", truth_id);
  HIPCHK(hipSetDevice(c->dev));
  const Truth& t = c->truths[(size_t)truth_id];
  *n_out = t.xn;
  if (t.xn > capacity) return fail(QM_E_RANGE, "qm_truth_entries: %lld entries, room for %lld", (long long)t.xn, (long long)capacity);
  const size_t n = (size_t)t.xn;
  if (!n) return QM_OK;
  if (pos) {
    HIPCHK(hipMemcpy(pos, t.d_xkeys, n * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) pos[i] = (int32_t)((uint32_t)pos[i] >> 4);
  }
  if (ref) HIPCHK(hipMemcpy(ref, t.d_xref, n * 4, hipMemcpyDeviceToHost));
  if (alt) HIPCHK(hipMemcpy(alt, t.d_xalt, n * 4, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_truth_normalized(qm_ctx* c, int truth_id, int genome_id, int32_t* pos, int32_t* ref, int32_t* alt, int64_t capacity, int64_t* n_out) {
  if (!c || !n_out || capacity < 0) return fail(QM_E_INVAL, "qm_truth_normalized: bad arguments");
  if (truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released)
    return fail(QM_E_INVAL, "qm_truth_normalized: no live truth set %d", truth_id);
  if (genome_id < 0 || genome_id >= (int)c->genomes.size() || c->genomes[(size_t)genome_id].released)
    return fail(QM_E_INVAL, "qm_truth_normalized: no live genome %d", genome_id);
  HIPCHK(hipSetDevice(c->dev));
  const Truth& t = c->truths[(size_t)truth_id];
  const uint32_t slots = norm_slots(t.xn);
  std::vector<uint32_t> h(4 * (size_t)slots);   // claim | spos | sref | salt: the head of the pool
  const int rc = build_and_read(c, "qm_truth_normalized", norm_pool_words(t.xn, slots), h.data(), h.size() * 4, [&](uint32_t* pool, const void**) {
    return norm_build(norm_table(t, c->genomes[(size_t)genome_id], pool, slots), c->stream);
  });
  if (rc != QM_OK) return rc;
  struct F { int32_t p, r, a; };
  std::vector<F> forms;
  for (size_t s = 0; s < slots; ++s)
    if (h[s]) forms.push_back(F{(int32_t)h[slots + s], (int32_t)h[2 * (size_t)slots + s], (int32_t)h[3 * (size_t)slots + s]});
  std::sort(forms.begin(), forms.end(), [](const F& x, const F& y) { return x.p != y.p ? x.p < y.p : x.r != y.r ? x.r < y.r : x.a < y.a; });
  *n_out = (int64_t)forms.size();
  if ((int64_t)forms.size() > capacity) return fail(QM_E_RANGE, "qm_truth_normalized: %zu forms, room for %lld", forms.size(), (long long)capacity);
  for (size_t i = 0; i < forms.size(); ++i) {
    if (pos) pos[i] = forms[i].p;
    if (ref) ref[i] = forms[i].r;
    if (alt) alt[i] = forms[i].a;
  }
  return QM_OK;
}
// ---- MNPs matched against adjacent SNVs ----
// The pool words of one set: set[slots], stats[2] (8-byte aligned: slots is even)
static size_t atom_pool_words(uint32_t slots) { return (size_t)slots + 4; }
static AtomTable atom_table(const Truth& t, uint32_t* pool, uint32_t slots) {
  AtomTable T;
  memset(&T, 0, sizeof T);
  T.xkeys = t.d_xkeys; T.xref = t.d_xref; T.xalt = t.d_xalt; T.xn = t.xn;
  T.slots = slots;
  T.set = pool;
  T.stats = reinterpret_cast<unsigned long long*>(pool + (size_t)slots);
  return T;
}
// Builds the set on `st` (the pool words start at a multiple of 8 bytes).
static int atom_build(const AtomTable& T, hipStream_t st) {
  HIPCHK(hipMemsetAsync(T.set, 0xff, (size_t)T.slots * 4, st));
  HIPCHK(hipMemsetAsync(T.stats, 0, 16, st));
  launch_atom_truth(T, st);
  HIPCHK(hipGetLastError());
  return QM_OK;
}
// How many atoms the atomisable entries of a truth set have together (what sizes its set): counted on the device at the first
// call that meets the truth set, one blocking 8-byte copy, and kept with it.
static int atom_total(qm_ctx* c, Truth& t, int64_t* out) {
  if (t.atom_total < 0) {
    unsigned long long* d = nullptr;
    unsigned long long h = 0;
    DALLOC(d, 1);
    hipError_t e = hipMemsetAsync(d, 0, 8, c->stream);
    if (e == hipSuccess) {
      launch_atom_count(atom_table(t, nullptr, ATOM_MIN_SLOTS), d, c->stream);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(&h, d, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(QM_E_HIP, "qm_batch_atomize: counting the atoms of a truth set: %s", hipGetErrorString(e));
    t.atom_total = (int64_t)h;
  }
  *out = t.atom_total;
  return QM_OK;
}
extern "C" int qm_batch_atomize(qm_batch* b, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_atomize");
  if (what & ~QM_ATOM_COLUMNS) return fail(QM_E_INVAL, "qm_batch_atomize: what = %u", what);
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_atomize: a single-base batch holds no MNPs to split into atoms (create the batch with QM_BATCH_ALLELES)");
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  int rc = truths_live(b, "qm_batch_atomize");
  if (rc != QM_OK) return rc;
  HIPCHK(hipSetDevice(c->dev));
  // one set per truth set
  struct Set { int truth; size_t off; uint32_t slots; };
  std::vector<Set> sets;
  std::vector<size_t> set_of(nv, 0);
  size_t pool_words = 0, bit_words = 0;
  int64_t max_lanes = 1;
  for (size_t v = 0; v < nv; ++v) {
    const int tid = b->L.vcfs[v].truth;
    size_t k = 0;
    while (k < sets.size() && sets[k].truth != tid) ++k;
    if (k == sets.size()) {
      int64_t total = 0;
      rc = atom_total(c, c->truths[(size_t)tid], &total);
      if (rc != QM_OK) return rc;
      const uint32_t slots = atom_slots(total);
      sets.push_back(Set{tid, pool_words, slots});
      pool_words += atom_pool_words(slots);
    }
    set_of[v] = k;
    const int64_t xn = c->truths[(size_t)tid].xn;
    bit_words += (size_t)(sets[k].slots / 32u) + (size_t)(xn / 32 + 1);
    max_lanes = std::max<int64_t>(max_lanes, std::max<int64_t>(xn, (int64_t)(sets[k].slots / 32u)));
  }
  OPEN_PASS(b, P_ATOM, stream, st);
  b->pass[P_ATOM].made = 0;   // from here on the outputs are rewritten (as in qm_batch_normalize)
  const size_t np = (size_t)b->L.n_pad;
  rc = b->at_pool.grow((int64_t)std::max<size_t>(pool_words, 2), &b->dev_bytes);
  if (rc == QM_OK) rc = b->at_bits.grow((int64_t)std::max<size_t>(bit_words, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->at_vcfs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->at_rec.grow((int64_t)std::max<size_t>(nv * ATOM_R_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->at_tru.grow((int64_t)std::max<size_t>(nv * ATOM_T_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK && (what & QM_ATOM_COLUMNS)) rc = b->at_cls.grow((int64_t)std::max<size_t>(2 * np, 1), &b->dev_bytes);
  if (rc == QM_OK && (what & QM_ATOM_COLUMNS)) rc = b->at_hm.grow((int64_t)std::max<size_t>(np, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_ATOM));
  HIPCHK(pass_mark(b, P_ATOM, 0, st));
  std::vector<AtomTable> tabs(sets.size());
  for (size_t k = 0; k < sets.size(); ++k) {
    tabs[k] = atom_table(c->truths[(size_t)sets[k].truth], b->at_pool + sets[k].off, sets[k].slots);
    rc = atom_build(tabs[k], st);
    if (rc != QM_OK) return rc;
  }
  std::vector<AtomVcf> vcfs(std::max<size_t>(nv, 1));
  memset(vcfs.data(), 0, vcfs.size() * sizeof(AtomVcf));
  size_t bo = 0;
  for (size_t v = 0; v < nv; ++v) {
    vcfs[v].t = tabs[set_of[v]];
    vcfs[v].abits = b->at_bits + bo;
    bo += (size_t)(vcfs[v].t.slots / 32u);
    vcfs[v].ebits = b->at_bits + bo;
    bo += (size_t)(vcfs[v].t.xn / 32 + 1);
  }
  if (nv) HIPCHK(hipMemcpy(b->at_vcfs, vcfs.data(), nv * sizeof(AtomVcf), hipMemcpyHostToDevice));   // blocking: vcfs dies here
  HIPCHK(hipMemsetAsync(b->at_bits, 0, std::max<size_t>(bit_words, 1) * 4, st));
  HIPCHK(hipMemsetAsync(b->at_rec, 0, std::max<size_t>(nv * ATOM_R_COLS, 1) * 8, st));
  HIPCHK(hipMemsetAsync(b->at_tru, 0, std::max<size_t>(nv * ATOM_T_COLS, 1) * 8, st));
  if (what & QM_ATOM_COLUMNS) {
    HIPCHK(hipMemsetAsync(b->at_cls, 0, std::max<size_t>(2 * np, 1), st));
    HIPCHK(hipMemsetAsync(b->at_hm, 0, std::max<size_t>(np, 1) * 2, st));
  }
  HIPCHK(pass_mark(b, P_ATOM, 1, st));
  AtomRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.vcfs = b->at_vcfs;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  if (what & QM_ATOM_COLUMNS) { P.cls = b->at_cls; P.n_atoms = b->at_cls + np; P.hit_mask = b->at_hm; }
  P.rec = b->at_rec;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_atom_records(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_ATOM, 2, st));
  launch_atom_found(b->at_vcfs, (int)nv, max_lanes, b->at_tru, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_ATOM, 3, st));
  HIPCHK(pass_done(b, P_ATOM, st, 1u | what));
  return QM_OK;
}
extern "C" int qm_batch_get_atomize(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_ATOM, "qm_batch_get_atomize");
  HIPCHK(pass_result(b, P_ATOM));
  const size_t nv = (size_t)b->n_vcf;
  if (rec && nv) HIPCHK(hipMemcpy(rec, b->at_rec, nv * ATOM_R_COLS * 8, hipMemcpyDeviceToHost));
  if (tru && nv) HIPCHK(hipMemcpy(tru, b->at_tru, nv * ATOM_T_COLS * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_atomized(qm_batch* b, int v, uint8_t* cls, uint8_t* n_atoms, uint16_t* hit_mask) {
  NEED_PASS(b, P_ATOM, "qm_batch_get_atomized");
  if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_atomized: VCF %d (the batch has %d)", v, b->n_vcf);
  if (!(b->pass[P_ATOM].made & QM_ATOM_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_get_atomized: the latest qm_batch_atomize did not keep the columns (QM_ATOM_COLUMNS)");
  HIPCHK(pass_result(b, P_ATOM));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n == 0) return QM_OK;
  const size_t np = (size_t)b->L.n_pad, n = (size_t)d.n;
  if (cls) HIPCHK(hipMemcpy(cls, b->at_cls + d.off, n, hipMemcpyDeviceToHost));
  if (n_atoms) HIPCHK(hipMemcpy(n_atoms, b->at_cls + np + d.off, n, hipMemcpyDeviceToHost));
  if (hit_mask) HIPCHK(hipMemcpy(hit_mask, b->at_hm + d.off, n * 2, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_atomize_timings(qm_batch* b, float* ms3) {
  return pass_timings(b, P_ATOM, "qm_batch_atomize_timings", ms3);
}
extern "C" int qm_truth_atoms(qm_ctx* c, int truth_id, uint32_t* keys, int64_t capacity, int64_t* n_out) {
  if (!c || !n_out || capacity < 0) return fail(QM_E_INVAL, "qm_truth_atoms: bad arguments");
  if (truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released)
    return fail(QM_E_INVAL, "qm_truth_atoms: no live truth set %d", truth_id);
  HIPCHK(hipSetDevice(c->dev));
  Truth& t = c->truths[(size_t)truth_id];
  int64_t total = 0;
  int rc = atom_total(c, t, &total);
  if (rc != QM_OK) return rc;
  const uint32_t slots = atom_slots(total);
  std::vector<uint32_t> h((size_t)slots);   // the set: the head of the pool
  rc = build_and_read(c, "qm_truth_atoms", atom_pool_words(slots), h.data(), h.size() * 4, [&](uint32_t* pool, const void**) {
    return atom_build(atom_table(t, pool, slots), c->stream);
  });
  if (rc != QM_OK) return rc;
  h.erase(std::remove(h.begin(), h.end(), ATOM_EMPTY), h.end());
  std::sort(h.begin(), h.end());
  *n_out = (int64_t)h.size();
  if ((int64_t)h.size() > capacity) return fail(QM_E_RANGE, "qm_truth_atoms: %zu atoms, room for %lld", h.size(), (long long)capacity);
  if (keys && !h.empty()) memcpy(keys, h.data(), h.size() * 4);
  return QM_OK;
}
// ---- the QUAL ROC under normal-form and atom matching ----
extern "C" int qm_batch_rescue_roc(qm_batch* b, unsigned which, void* stream) {
  NEED_FINISHED(b, "qm_batch_rescue_roc");
  if (which == 0 || (which & ~(QM_RROC_NORM | QM_RROC_ATOM))) return fail(QM_E_INVAL, "qm_batch_rescue_roc: which = %u", which);
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_rescue_roc: a single-base batch has no rescue passes to sweep (create the batch with QM_BATCH_ALLELES)");
  const bool wn = (which & QM_RROC_NORM) != 0, wa = (which & QM_RROC_ATOM) != 0;
  if (wn && pass_needs<P_RROC, P_NORM>(b, "QM_RROC_NORM") != QM_OK) return QM_E_STATE;
  if (wa && pass_needs<P_RROC, P_ATOM>(b, "QM_RROC_ATOM") != QM_OK) return QM_E_STATE;
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf, nb = (size_t)b->n_bins;
  int rc = truths_live(b, "qm_batch_rescue_roc");
  if (rc != QM_OK) return rc;
  // the cells of every VCF, one behind the other (a VCF's own: what one VCF carries is nothing to the next on the same truth set)
  std::vector<RrocVcf> vcfs(std::max<size_t>(nv, 1));
  memset(vcfs.data(), 0, vcfs.size() * sizeof(RrocVcf));
  std::vector<size_t> off_n(nv, 0), off_a(nv, 0), off_e(nv, 0);
  size_t words = 0;
  for (size_t v = 0; v < nv; ++v) {
    Truth& t = c->truths[(size_t)b->L.vcfs[v].truth];
    vcfs[v].xn = t.xn;
    if (wn && b->nz_has[v]) { off_n[v] = words; words += rroc_cell_words(t.xn) + 1; }
    if (wa) {
      int64_t total = 0;
      rc = atom_total(c, t, &total);   // (kept with the truth set since qm_batch_atomize met it: the slots of its set)
      if (rc != QM_OK) return rc;
      off_a[v] = words; words += (size_t)(atom_slots(total) / 2u);
      off_e[v] = words; words += rroc_cell_words(t.xn) + 1;
    }
  }
  OPEN_PASS(b, P_RROC, stream, st);
  b->pass[P_RROC].made = 0;   // from here on the outputs are rewritten
  const size_t rows = nv * 3 * nb, out_words = std::max<size_t>(2 * rows + 2 * nv, 1);
  rc = b->rr_best.grow((int64_t)std::max<size_t>(words, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->rr_vcfs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->rr_out.grow((int64_t)out_words, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  for (size_t v = 0; v < nv; ++v) {
    if (wn && b->nz_has[v]) vcfs[v].best_n = b->rr_best + off_n[v];
    if (wa) { vcfs[v].best_atom = b->rr_best + off_a[v]; vcfs[v].best_entry = b->rr_best + off_e[v]; }
  }
  HIPCHK(pass_marks(b, P_RROC));
  if (wn) HIPCHK(pass_wait<P_RROC, P_NORM>(b, st));   // the producers may have run on other streams
  if (wa) HIPCHK(pass_wait<P_RROC, P_ATOM>(b, st));
  if (nv) HIPCHK(hipMemcpy(b->rr_vcfs, vcfs.data(), nv * sizeof(RrocVcf), hipMemcpyHostToDevice));   // blocking: vcfs dies here
  HIPCHK(hipMemsetAsync(b->rr_best, 0, std::max<size_t>(words, 1) * 4, st));
  HIPCHK(hipMemsetAsync(b->rr_out, 0, out_words * 8, st));
  const size_t np = (size_t)b->L.n_pad;
  uint64_t* const base = b->rr_out + 2 * rows;
  RrocRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.vcfs = b->rr_vcfs;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.qual = b->qual; P.flags = b->flags;
  P.n_spans = (int32_t)b->L.spans.size(); P.n_bins = b->n_bins;
  HIPCHK(pass_mark(b, P_RROC, 0, st));
  if (wn) {
    P.nrow = b->nz_cols + 3 * np; P.hist = b->rr_out;
    launch_rroc_records(RROC_N, P, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_mark(b, P_RROC, 1, st));
  if (wn) {
    launch_rroc_units(RROC_N, b->rr_vcfs, nullptr, (int)nv, b->rr_out, b->n_bins, base, b->nz_tru, NORM_T_COLS, QM_NORM_T_FORMS, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_mark(b, P_RROC, 2, st));
  if (wa) {
    P.nrow = nullptr; P.avcfs = b->at_vcfs; P.hit_mask = b->at_hm; P.hist = b->rr_out + rows;
    launch_rroc_records(RROC_A, P, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_mark(b, P_RROC, 3, st));
  if (wa) {
    launch_rroc_units(RROC_A, b->rr_vcfs, b->at_vcfs, (int)nv, b->rr_out + rows, b->n_bins, base, b->at_tru, ATOM_T_COLS, QM_ATOM_T_ENTRIES, st);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(pass_mark(b, P_RROC, 4, st));
  HIPCHK(pass_done(b, P_RROC, st, which));
  return QM_OK;
}
extern "C" int qm_batch_get_rescue_roc(qm_batch* b, uint64_t* roc_n, uint64_t* roc_a, uint64_t* base) {
  NEED_PASS(b, P_RROC, "qm_batch_get_rescue_roc");
  if ((roc_n && !(b->pass[P_RROC].made & QM_RROC_NORM)) || (roc_a && !(b->pass[P_RROC].made & QM_RROC_ATOM)))
    return fail(QM_E_STATE, "qm_batch_get_rescue_roc: the latest qm_batch_rescue_roc did not sweep by %s", roc_n && !(b->pass[P_RROC].made & QM_RROC_NORM) ? "normal form" : "atoms");
  HIPCHK(pass_result(b, P_RROC));
  const size_t nv = (size_t)b->n_vcf, rows = nv * 3 * (size_t)b->n_bins;
  if (roc_n && nv) HIPCHK(hipMemcpy(roc_n, b->rr_out, rows * 8, hipMemcpyDeviceToHost));
  if (roc_a && nv) HIPCHK(hipMemcpy(roc_a, b->rr_out + rows, rows * 8, hipMemcpyDeviceToHost));
  if (base && nv) HIPCHK(hipMemcpy(base, b->rr_out + 2 * rows, nv * 2 * 8, hipMemcpyDeviceToHost));   // (0 for a matching not swept)
  return QM_OK;
}
extern "C" int qm_batch_rescue_roc_timings(qm_batch* b, float* ms4) {
  return pass_timings(b, P_RROC, "qm_batch_rescue_roc_timings", ms4);
}
// ---- the four rescues combined: final TP, FP and FN and the Venn of methods ----
extern "C" int qm_batch_ladder(qm_batch* b, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_ladder");
  if (what & ~(QM_LADDER_SUBSETS | QM_LADDER_COLUMNS)) return fail(QM_E_INVAL, "qm_batch_ladder: what = %u", what);
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_ladder: a single-base batch has no rescue passes to combine (create the batch with QM_BATCH_ALLELES)");
  const bool subsets = (what & QM_LADDER_SUBSETS) != 0, cols = (what & QM_LADDER_COLUMNS) != 0;
  if (pass_needs<P_LADDER, P_NORM>(b) != QM_OK) return QM_E_STATE;
  if (pass_needs<P_LADDER, P_ATOM>(b) != QM_OK) return QM_E_STATE;
  if (pass_needs<P_LADDER, P_HAPLO>(b) != QM_OK) return QM_E_STATE;
  if (subsets && pass_needs<P_LADDER, P_HAPSUB>(b, "QM_LADDER_SUBSETS") != QM_OK) return QM_E_STATE;
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  int rc = truths_live(b, "qm_batch_ladder");
  if (rc != QM_OK) return rc;
  std::vector<LadderVcf> vcfs(std::max<size_t>(nv, 1));
  memset(vcfs.data(), 0, vcfs.size() * sizeof(LadderVcf));
  std::vector<int64_t> eoff(nv + 1, 0);
  int64_t max_entries = 0;
  for (size_t v = 0; v < nv; ++v) {
    const int64_t xn = c->truths[(size_t)b->L.vcfs[v].truth].xn;
    eoff[v + 1] = eoff[v] + xn;
    max_entries = std::max(max_entries, xn);
    vcfs[v].eoff = eoff[v];
    vcfs[v].heoff = b->hp_eoff[v];
    vcfs[v].has = (b->nz_has[v] ? LADDER_HAS_NORM : 0u) | (b->hp_has[v] ? LADDER_HAS_HAP : 0u);
  }
  OPEN_PASS(b, P_LADDER, stream, st);
  b->pass[P_LADDER].made = 0;   // from here on the outputs are rewritten
  const size_t np = (size_t)b->L.n_pad, rows = nv * LADDER_COLS, out_words = std::max<size_t>(2 * rows, 1);
  rc = b->ld_vcfs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->ld_out.grow((int64_t)out_words, &b->dev_bytes);
  if (rc == QM_OK && cols) rc = b->ld_mask.grow((int64_t)std::max<size_t>(np, 1), &b->dev_bytes);
  if (rc == QM_OK && cols) rc = b->ld_emask.grow(std::max<int64_t>(eoff[nv], 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  b->ld_eoff = eoff;
  HIPCHK(pass_marks(b, P_LADDER));
  HIPCHK(pass_wait<P_LADDER, P_NORM>(b, st));   // the producers may have run on other streams
  HIPCHK(pass_wait<P_LADDER, P_ATOM>(b, st));
  HIPCHK(pass_wait<P_LADDER, P_HAPLO>(b, st));
  if (subsets) HIPCHK(pass_wait<P_LADDER, P_HAPSUB>(b, st));
  if (nv) HIPCHK(hipMemcpy(b->ld_vcfs, vcfs.data(), nv * sizeof(LadderVcf), hipMemcpyHostToDevice));   // blocking: vcfs dies here
  HIPCHK(hipMemsetAsync(b->ld_out, 0, out_words * 8, st));
  HIPCHK(pass_mark(b, P_LADDER, 0, st));
  LadderRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.vcfs = b->ld_vcfs;
  P.flags = b->flags; P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  P.cls_n = b->nz_cls; P.cls_a = b->at_cls; P.cls_h = b->hp_cls;
  P.cls_b = subsets ? (const uint8_t*)b->hs_cls : nullptr;
  P.mask = cols ? (uint8_t*)b->ld_mask : nullptr;
  P.rec = b->ld_out;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_ladder_records(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_LADDER, 1, st));
  LadderTruthParams Q;
  memset(&Q, 0, sizeof Q);
  Q.vcfs = b->ld_vcfs; Q.nvcfs = b->nz_vcfs; Q.avcfs = b->at_vcfs; Q.hvcfs = b->hp_vcfs;
  Q.ecls_b = subsets ? (const uint8_t*)b->hs_ecls : nullptr;
  Q.emask = cols ? (uint8_t*)b->ld_emask : nullptr;
  Q.tru = b->ld_out + rows;
  Q.n_vcf = (int32_t)nv;
  launch_ladder_truth(Q, max_entries, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_LADDER, 2, st));
  HIPCHK(pass_done(b, P_LADDER, st, 4u | what));
  return QM_OK;
}
extern "C" int qm_batch_get_ladder(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_LADDER, "qm_batch_get_ladder");
  HIPCHK(pass_result(b, P_LADDER));
  const size_t nv = (size_t)b->n_vcf, rows = nv * LADDER_COLS;
  if (rec && nv) HIPCHK(hipMemcpy(rec, b->ld_out, rows * 8, hipMemcpyDeviceToHost));
  if (tru && nv) HIPCHK(hipMemcpy(tru, b->ld_out + rows, rows * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_laddered(qm_batch* b, int v, uint8_t* mask, uint8_t* entry_mask) {
  NEED_PASS(b, P_LADDER, "qm_batch_get_laddered");
  if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_laddered: VCF %d (the batch has %d)", v, b->n_vcf);
  if (!(b->pass[P_LADDER].made & QM_LADDER_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_get_laddered: the latest qm_batch_ladder did not keep the columns (QM_LADDER_COLUMNS)");
  HIPCHK(pass_result(b, P_LADDER));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  const size_t n = (size_t)d.n, ne = (size_t)(b->ld_eoff[(size_t)v + 1] - b->ld_eoff[(size_t)v]);
  if (mask && n) HIPCHK(hipMemcpy(mask, b->ld_mask + d.off, n, hipMemcpyDeviceToHost));
  if (entry_mask && ne) HIPCHK(hipMemcpy(entry_mask, b->ld_emask + b->ld_eoff[(size_t)v], ne, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_ladder_timings(qm_batch* b, float* ms2) {
  return pass_timings(b, P_LADDER, "qm_batch_ladder_timings", ms2);
}
// ---- the match ladder per variant type and size ----
extern "C" int qm_batch_ladder_types(qm_batch* b, void* stream) {
  NEED_FINISHED(b, "qm_batch_ladder_types");
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_ladder_types: a single-base batch has neither types nor rescue passes to cross (create the batch with QM_BATCH_ALLELES)");
  if (pass_needs<P_LTYPES, P_TYPES>(b) != QM_OK) return QM_E_STATE;
  if (pass_needs<P_LTYPES, P_LADDER>(b) != QM_OK) return QM_E_STATE;
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  int rc = truths_live(b, "qm_batch_ladder_types");
  if (rc != QM_OK) return rc;
  int64_t max_entries = 0;
  for (size_t v = 0; v < nv; ++v) max_entries = std::max(max_entries, c->truths[(size_t)b->L.vcfs[v].truth].xn);
  OPEN_PASS(b, P_LTYPES, stream, st);
  b->pass[P_LTYPES].made = 0;   // from here on the outputs are rewritten
  const TypeBins& B = b->ty_bins;
  const size_t block = nv * (size_t)B.n_rows * LADDER_COLS, out_words = std::max<size_t>(2 * block, 1);
  rc = b->lt_out.grow((int64_t)out_words, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_LTYPES));
  HIPCHK(pass_wait<P_LTYPES, P_TYPES>(b, st));   // the producers may have run on other streams
  HIPCHK(pass_wait<P_LTYPES, P_LADDER>(b, st));
  HIPCHK(hipMemsetAsync(b->lt_out, 0, out_words * 8, st));
  HIPCHK(pass_mark(b, P_LTYPES, 0, st));
  LtypeRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.row = b->ty_row; P.mask = b->ld_mask;
  P.rec = b->lt_out;
  P.n_spans = (int32_t)b->L.spans.size();
  P.n_rows = B.n_rows;
  launch_ltype_records(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_LTYPES, 1, st));
  LtypeTruthParams Q;
  memset(&Q, 0, sizeof Q);
  Q.tvcfs = b->ty_vcfs; Q.lvcfs = b->ld_vcfs; Q.emask = b->ld_emask;
  Q.tru = b->lt_out + block;
  Q.bins = B;
  if (b->ty_nshapes) {
    const uint32_t* d = b->ty_shapes;
    const size_t ns = (size_t)b->ty_nshapes;
    Q.shapes.len = reinterpret_cast<const int32_t*>(d); Q.shapes.head = d + ns; Q.shapes.tail = d + 2 * ns; Q.shapes.n = b->ty_nshapes;
  }
  launch_ltype_truth(Q, (int)nv, max_entries, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_LTYPES, 2, st));
  HIPCHK(pass_done(b, P_LTYPES, st, 1u));
  b->lt_rows = B.n_rows;
  return QM_OK;
}
extern "C" int qm_batch_get_ladder_types(qm_batch* b, uint64_t* rec, uint64_t* tru, int* n_rows_out) {
  NEED_PASS(b, P_LTYPES, "qm_batch_get_ladder_types");
  HIPCHK(pass_result(b, P_LTYPES));
  const size_t block = (size_t)b->n_vcf * (size_t)b->lt_rows * LADDER_COLS;
  if (rec && block) HIPCHK(hipMemcpy(rec, b->lt_out, block * 8, hipMemcpyDeviceToHost));
  if (tru && block) HIPCHK(hipMemcpy(tru, b->lt_out + block, block * 8, hipMemcpyDeviceToHost));
  if (n_rows_out) *n_rows_out = b->lt_rows;
  return QM_OK;
}
extern "C" int qm_batch_ladder_types_timings(qm_batch* b, float* ms2) {
  return pass_timings(b, P_LTYPES, "qm_batch_ladder_types_timings", ms2);
}
// ---- TP, FP and FN by variant type and size ----
extern "C" int qm_batch_types(qm_batch* b, const int32_t* edges, int n_bins, const int32_t* len, const uint32_t* head, const uint32_t* tail,
                              int64_t n_shapes, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_types");
  if (what & ~QM_TYPE_COLUMNS) return fail(QM_E_INVAL, "qm_batch_types: what = %u", what);
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_types: a single-base batch holds SNVs only, there is nothing to type (create the batch with QM_BATCH_ALLELES)");
  if (!edges || n_bins < 1 || n_bins > QM_TYPE_MAX_BINS) return fail(QM_E_INVAL, "qm_batch_types: %d size bins (1 to %d)", n_bins, QM_TYPE_MAX_BINS);
  if (edges[0] != 1) return fail(QM_E_INVAL, "qm_batch_types: the first size edge is %d (it must be 1)", edges[0]);
  for (int i = 1; i < n_bins; ++i)
    if (edges[i] <= edges[i - 1]) return fail(QM_E_INVAL, "qm_batch_types: size edge %d is %d behind %d (the edges ascend)", i, edges[i], edges[i - 1]);
  if (n_shapes < 0 || n_shapes > 0x40000000ll || (n_shapes > 0 && (!len || !head || !tail))) return fail(QM_E_INVAL, "qm_batch_types: %lld shape rows (NULL arrays?)", (long long)n_shapes);
  for (int64_t i = 0; i < n_shapes; ++i)
    if (len[i] <= QM_ALLELE_INLINE_MAX)
      return fail(QM_E_INVAL, "qm_batch_types: shape row %lld has len %d (a dictionary id names an allele of at least %d bases)", (long long)i, len[i], QM_ALLELE_INLINE_MAX + 1);
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  int rc = truths_live(b, "qm_batch_types");
  if (rc != QM_OK) return rc;
  OPEN_PASS(b, P_TYPES, stream, st);
  b->pass[P_TYPES].made = 0;   // from here on the outputs are rewritten
  TypeBins B;
  memset(&B, 0, sizeof B);
  for (int i = 0; i < n_bins; ++i) B.edges[i] = edges[i];
  B.n_bins = n_bins;
  B.n_rows = TYPE_KINDS * n_bins + TYPE_OFFGRID;
  const size_t cells = 2 * (size_t)B.n_rows, np = (size_t)b->L.n_pad, ns = (size_t)n_shapes;
  size_t bit_words = 0;
  int64_t max_entries = 0;
  for (size_t v = 0; v < nv; ++v) {
    const int64_t xn = c->truths[(size_t)b->L.vcfs[v].truth].xn;
    bit_words += (size_t)(xn / 32 + 1);
    max_entries = std::max(max_entries, xn);
  }
  rc = b->ty_bits.grow((int64_t)std::max<size_t>(bit_words, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->ty_vcfs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->ty_rec.grow((int64_t)std::max<size_t>(nv * 2 * TYPE_MAX_ROWS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->ty_tru.grow((int64_t)std::max<size_t>(nv * 2 * TYPE_MAX_ROWS, 1), &b->dev_bytes);
  if (rc == QM_OK && ns) rc = b->ty_shapes.grow((int64_t)(3 * ns), &b->dev_bytes);
  if (rc == QM_OK && (what & QM_TYPE_COLUMNS)) rc = b->ty_row.grow((int64_t)std::max<size_t>(np, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_TYPES));
  std::vector<TypeVcf> vcfs(std::max<size_t>(nv, 1));
  memset(vcfs.data(), 0, vcfs.size() * sizeof(TypeVcf));
  size_t bo = 0;
  for (size_t v = 0; v < nv; ++v) {
    const Truth& t = c->truths[(size_t)b->L.vcfs[v].truth];
    vcfs[v].xkeys = t.d_xkeys; vcfs[v].xref = t.d_xref; vcfs[v].xalt = t.d_xalt; vcfs[v].xn = t.xn;
    vcfs[v].ebits = b->ty_bits + bo;
    bo += (size_t)(t.xn / 32 + 1);
  }
  // blocking copies: vcfs dies here, and the caller's shape arrays are read during the call only (the previous call of the pass
  // is done: pass_open waited for it)
  if (nv) HIPCHK(hipMemcpy(b->ty_vcfs, vcfs.data(), nv * sizeof(TypeVcf), hipMemcpyHostToDevice));
  TypeShapes S;
  memset(&S, 0, sizeof S);
  if (ns) {
    uint32_t* d = b->ty_shapes;
    HIPCHK(hipMemcpy(d, len, ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + ns, head, ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d + 2 * ns, tail, ns * 4, hipMemcpyHostToDevice));
    S.len = reinterpret_cast<const int32_t*>(d); S.head = d + ns; S.tail = d + 2 * ns; S.n = n_shapes;
  }
  HIPCHK(hipMemsetAsync(b->ty_bits, 0, std::max<size_t>(bit_words, 1) * 4, st));
  HIPCHK(hipMemsetAsync(b->ty_rec, 0, std::max<size_t>(nv * cells, 1) * 8, st));
  HIPCHK(hipMemsetAsync(b->ty_tru, 0, std::max<size_t>(nv * cells, 1) * 8, st));
  if (what & QM_TYPE_COLUMNS) HIPCHK(hipMemsetAsync(b->ty_row, 0, std::max<size_t>(np, 1), st));
  HIPCHK(pass_mark(b, P_TYPES, 0, st));
  TypeRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.vcfs = b->ty_vcfs;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  if (what & QM_TYPE_COLUMNS) P.row = b->ty_row;
  P.rec = b->ty_rec;
  P.shapes = S; P.bins = B;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_type_records(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_TYPES, 1, st));
  TypeTruthParams Q;
  memset(&Q, 0, sizeof Q);
  Q.vcfs = b->ty_vcfs; Q.tru = b->ty_tru; Q.shapes = S; Q.bins = B;
  launch_type_truth(Q, (int)nv, max_entries, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_TYPES, 2, st));
  HIPCHK(pass_done(b, P_TYPES, st, 1u | what));
  b->ty_rows = B.n_rows;
  b->ty_bins = B;
  b->ty_nshapes = n_shapes;
  return QM_OK;
}
extern "C" int qm_batch_get_types(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_TYPES, "qm_batch_get_types");
  HIPCHK(pass_result(b, P_TYPES));
  const size_t bytes = (size_t)b->n_vcf * 2 * (size_t)b->ty_rows * 8;
  if (rec && bytes) HIPCHK(hipMemcpy(rec, b->ty_rec, bytes, hipMemcpyDeviceToHost));
  if (tru && bytes) HIPCHK(hipMemcpy(tru, b->ty_tru, bytes, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_typed(qm_batch* b, int v, uint8_t* row) {
  NEED_PASS(b, P_TYPES, "qm_batch_get_typed");
  if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_typed: VCF %d (the batch has %d)", v, b->n_vcf);
  if (!(b->pass[P_TYPES].made & QM_TYPE_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_get_typed: the latest qm_batch_types did not keep the row bytes (QM_TYPE_COLUMNS)");
  HIPCHK(pass_result(b, P_TYPES));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n && row) HIPCHK(hipMemcpy(row, b->ty_row + d.off, (size_t)d.n, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_types_timings(qm_batch* b, float* ms2) {
  return pass_timings(b, P_TYPES, "qm_batch_types_timings", ms2);
}
// ---- clusters of records matched by replayed haplotype ----
// The pool words of one site table: [elo | ehi | esite | slo | shi][xn], sfirst[xn + 1], n_sites[2], ewhy[xn] as bytes
static size_t hap_pool_words(int64_t xn) { return 6 * (size_t)xn + 3 + ((size_t)xn + 3) / 4; }
static HapSites hap_sites(const Truth& t, const Genome& g, int gap, uint32_t* pool) {
  HapSites S;
  memset(&S, 0, sizeof S);
  const size_t xn = (size_t)t.xn;
  S.words = g.d_words; S.len = g.len;
  S.xkeys = t.d_xkeys; S.xref = t.d_xref; S.xalt = t.d_xalt; S.xn = t.xn;
  int32_t* w = reinterpret_cast<int32_t*>(pool);
  S.elo = w; S.ehi = w + xn; S.esite = w + 2 * xn; S.slo = w + 3 * xn; S.shi = w + 4 * xn;
  S.sfirst = w + 5 * xn;
  S.n_sites = w + 6 * xn + 1;
  S.ewhy = reinterpret_cast<uint8_t*>(w + 6 * xn + 3);
  S.gap = gap;
  return S;
}
static int hap_build(const HapSites& S, hipStream_t st) {
  launch_hap_sites(S, st);
  HIPCHK(hipGetLastError());
  return QM_OK;
}
extern "C" int qm_batch_haplotypes(qm_batch* b, const int32_t* genome_id_per_vcf, int gap, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_haplotypes");
  if (!genome_id_per_vcf) return fail(QM_E_INVAL, "qm_batch_haplotypes: NULL genome ids");
  if (what & ~QM_HAP_COLUMNS) return fail(QM_E_INVAL, "qm_batch_haplotypes: what = %u", what);
  if (gap < 0 || gap > QM_HAP_MAX_GAP) return fail(QM_E_INVAL, "qm_batch_haplotypes: gap %d (0 to %d)", gap, QM_HAP_MAX_GAP);
  if (!b->ext) return fail(QM_E_STATE, "qm_batch_haplotypes: a single-base batch holds no indels, MNPs or complex records to replay (create the batch with QM_BATCH_ALLELES)");
  if (b->n_vcf > 65535) return fail(QM_E_RANGE, "qm_batch_haplotypes: %d VCFs (at most 65535 in one batch)", b->n_vcf);
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  int rc = genomes_named(c, "qm_batch_haplotypes", genome_id_per_vcf, b->n_vcf);
  if (rc == QM_OK) rc = truths_live(b, "qm_batch_haplotypes");
  if (rc != QM_OK) return rc;
  // one site table per truth set: the VCFs that share one must name one genome
  std::vector<TruthTab> pairs;
  std::vector<int> pair_of;
  size_t pool_words = 0, bit_words = 0;
  rc = tabs_by_truth(b, "qm_batch_haplotypes", "the sites of a truth set belong to one genome", genome_id_per_vcf,
                     [](const Truth& t) { return hap_pool_words(t.xn); }, &pairs, &pair_of, &pool_words);
  if (rc != QM_OK) return rc;
  int64_t max_entries = 0;
  std::vector<int64_t> eoff(nv + 1, 0);   // (committed with what the pass made: a call refused below leaves the previous call's offsets)
  for (size_t v = 0; v < nv; ++v) {
    eoff[v + 1] = eoff[v];
    if (pair_of[v] < 0) continue;
    const int64_t xn = c->truths[(size_t)b->L.vcfs[v].truth].xn;
    bit_words += 3 * (size_t)(xn / 32 + 1);
    max_entries = std::max(max_entries, xn);
    eoff[v + 1] += xn;
  }
  OPEN_PASS(b, P_HAPLO, stream, st);
  b->pass[P_HAPLO].made = 0;   // from here on the outputs are rewritten (pass_open: the search and the ladder are done and forgotten)
  const size_t np = (size_t)b->L.n_pad;
  const bool cols = (what & QM_HAP_COLUMNS) != 0;
  rc = b->hp_pool.grow((int64_t)std::max<size_t>(pool_words, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_bits.grow((int64_t)std::max<size_t>(bit_words, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_vcfs.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_rec.grow((int64_t)std::max<size_t>(nv * HAP_R_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_tru.grow((int64_t)std::max<size_t>(nv * HAP_T_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_total.grow(1, &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_cls.grow((int64_t)std::max<size_t>(np, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hp_site.grow((int64_t)std::max<size_t>(np, 1), &b->dev_bytes);
  if (rc == QM_OK && cols) rc = b->hp_ecls.grow(std::max<int64_t>(eoff[nv], 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_HAPLO));
  HIPCHK(pass_mark(b, P_HAPLO, 0, st));
  std::vector<HapSites> tabs(pairs.size());
  for (size_t k = 0; k < pairs.size(); ++k) {
    tabs[k] = hap_sites(c->truths[(size_t)pairs[k].truth], c->genomes[(size_t)pairs[k].genome], gap, b->hp_pool + pairs[k].off);
    rc = hap_build(tabs[k], st);
    if (rc != QM_OK) return rc;
  }
  std::vector<HapVcf> vcfs(std::max<size_t>(nv, 1));
  memset(vcfs.data(), 0, vcfs.size() * sizeof(HapVcf));
  b->hp_has.assign(nv, 0);
  size_t bo = 0;
  for (size_t v = 0; v < nv; ++v) {
    if (pair_of[v] < 0) continue;
    const size_t w = (size_t)(tabs[(size_t)pair_of[v]].xn / 32 + 1);
    vcfs[v].s = tabs[(size_t)pair_of[v]];
    vcfs[v].off = b->L.vcfs[v].off;
    vcfs[v].ebits = b->hp_bits + bo;
    vcfs[v].sbits = b->hp_bits + bo + w;
    vcfs[v].srank = b->hp_bits + bo + 2 * w;
    if (cols) vcfs[v].ecls = b->hp_ecls + eoff[v];
    bo += 3 * w;
    b->hp_has[v] = 1;
  }
  if (nv) HIPCHK(hipMemcpy(b->hp_vcfs, vcfs.data(), nv * sizeof(HapVcf), hipMemcpyHostToDevice));   // blocking: vcfs dies here
  HIPCHK(hipMemsetAsync(b->hp_bits, 0, std::max<size_t>(bit_words, 1) * 4, st));
  HIPCHK(hipMemsetAsync(b->hp_rec, 0, std::max<size_t>(nv * HAP_R_COLS, 1) * 8, st));
  HIPCHK(hipMemsetAsync(b->hp_tru, 0, std::max<size_t>(nv * HAP_T_COLS, 1) * 8, st));
  HIPCHK(hipMemsetAsync(b->hp_total, 0, 8, st));
  HIPCHK(hipMemsetAsync(b->hp_cls, 0, std::max<size_t>(np, 1), st));
  HIPCHK(hipMemsetAsync(b->hp_site, 0xff, std::max<size_t>(np, 1) * 4, st));
  HIPCHK(pass_mark(b, P_HAPLO, 1, st));
  HapRecParams P;
  memset(&P, 0, sizeof P);
  P.spans = b->d_spans; P.vcfs = b->hp_vcfs;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  P.cls = b->hp_cls; P.site = b->hp_site; P.rec = b->hp_rec;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_hap_records(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_HAPLO, 2, st));
  launch_hap_truth(b->hp_vcfs, (int)nv, max_entries, b->hp_tru, b->hp_total, st);
  HIPCHK(hipGetLastError());
  // the one blocking readback of the pass: how many (VCF, open site) pairs there are sizes their lists
  unsigned long long n_pairs = 0;
  HIPCHK(hipMemcpyAsync(&n_pairs, b->hp_total, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (n_pairs > (unsigned long long)(0x7fffffff / HAP_PAIR_WORDS)) return fail(QM_E_RANGE, "qm_batch_haplotypes: %llu (VCF, open site) pairs", n_pairs);
  rc = b->hp_pairs.grow((int64_t)std::max<size_t>((size_t)n_pairs * HAP_PAIR_WORDS, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_mark(b, P_HAPLO, 3, st));
  P.pairs = b->hp_pairs;
  // (also without a pair: the pending lines of sites whose entries are all found become LONE there; no list is touched then)
  launch_hap_claim(P, (int)nv, max_entries, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_HAPLO, 4, st));
  HapReplayParams Q;
  memset(&Q, 0, sizeof Q);
  Q.vcfs = b->hp_vcfs;
  Q.pos = b->pos; Q.ref = b->ref; Q.alt = b->alt; Q.flags = b->flags; Q.mask_tp = b->mask_tp;
  Q.cls = b->hp_cls; Q.rec = b->hp_rec; Q.tru = b->hp_tru;
  Q.pairs = b->hp_pairs; Q.n_pairs = (int64_t)n_pairs;
  launch_hap_replay(Q, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_HAPLO, 5, st));
  HIPCHK(pass_done(b, P_HAPLO, st, 1u | what));
  b->hp_eoff = eoff;
  b->hp_gids.assign(genome_id_per_vcf, genome_id_per_vcf + nv);
  b->hp_npairs = (int64_t)n_pairs;
  return QM_OK;
}
extern "C" int qm_batch_get_haplotypes(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_HAPLO, "qm_batch_get_haplotypes");
  HIPCHK(pass_result(b, P_HAPLO));
  const size_t nv = (size_t)b->n_vcf;
  if (rec && nv) HIPCHK(hipMemcpy(rec, b->hp_rec, nv * HAP_R_COLS * 8, hipMemcpyDeviceToHost));
  if (tru && nv) HIPCHK(hipMemcpy(tru, b->hp_tru, nv * HAP_T_COLS * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_haplotyped(qm_batch* b, int v, uint8_t* cls, int32_t* site, uint8_t* entry_cls) {
  NEED_PASS(b, P_HAPLO, "qm_batch_get_haplotyped");
  if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_haplotyped: VCF %d (the batch has %d)", v, b->n_vcf);
  if (!b->hp_has[(size_t)v]) return fail(QM_E_STATE, "qm_batch_get_haplotyped: VCF %d named no genome in the latest qm_batch_haplotypes", v);
  if (!(b->pass[P_HAPLO].made & QM_HAP_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_get_haplotyped: the latest qm_batch_haplotypes did not keep the columns (QM_HAP_COLUMNS)");
  HIPCHK(pass_result(b, P_HAPLO));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  const size_t n = (size_t)d.n, ne = (size_t)(b->hp_eoff[(size_t)v + 1] - b->hp_eoff[(size_t)v]);
  if (cls && n) HIPCHK(hipMemcpy(cls, b->hp_cls + d.off, n, hipMemcpyDeviceToHost));
  if (site && n) HIPCHK(hipMemcpy(site, b->hp_site + d.off, n * 4, hipMemcpyDeviceToHost));
  if (entry_cls && ne) HIPCHK(hipMemcpy(entry_cls, b->hp_ecls + b->hp_eoff[(size_t)v], ne, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_haplotype_timings(qm_batch* b, float* ms5) {
  return pass_timings(b, P_HAPLO, "qm_batch_haplotype_timings", ms5);
}
// ---- a subset search inside the mismatched sites of the haplotype pass ----
extern "C" int qm_batch_hapsubsets(qm_batch* b, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_hapsubsets");
  if (what & ~(QM_HAPSUB_COLUMNS | QM_HAPSUB_NARROW_HASH)) return fail(QM_E_INVAL, "qm_batch_hapsubsets: what = %u", what);
  if (pass_ran(b, P_HAPLO, "qm_batch_hapsubsets") != QM_OK) return QM_E_STATE;
  const bool cols = (what & QM_HAPSUB_COLUMNS) != 0;
  if (cols && !(b->pass[P_HAPLO].made & QM_HAP_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_hapsubsets: QM_HAPSUB_COLUMNS needs the columns of the latest qm_batch_haplotypes (QM_HAP_COLUMNS)");
  qm_ctx* c = b->ctx;
  const size_t nv = (size_t)b->n_vcf;
  for (size_t v = 0; v < nv; ++v) {
    const int gid = b->hp_gids[v];
    if (gid >= 0 && (gid >= (int)c->genomes.size() || c->genomes[(size_t)gid].released))
      return fail(QM_E_STATE, "qm_batch_hapsubsets: VCF %zu names released genome %d", v, gid);
  }
  int rc = truths_live(b, "qm_batch_hapsubsets");
  if (rc != QM_OK) return rc;
  OPEN_PASS(b, P_HAPSUB, stream, st);
  b->pass[P_HAPSUB].made = 0;   // from here on the outputs are rewritten (as in qm_batch_normalize: the ladder reads the second classes)
  b->hs_listed = false;
  const size_t np = (size_t)b->L.n_pad, npairs = (size_t)b->hp_npairs, ne = (size_t)b->hp_eoff[nv];
  rc = b->hs_sub.grow((int64_t)std::max<size_t>(nv * HAPSUB_COLS, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->hs_res.grow((int64_t)std::max<size_t>(npairs, 1), &b->dev_bytes);
  if (rc == QM_OK && cols) rc = b->hs_cls.grow((int64_t)std::max<size_t>(np, 1), &b->dev_bytes);
  if (rc == QM_OK && cols) rc = b->hs_ecls.grow((int64_t)std::max<size_t>(ne, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(pass_marks(b, P_HAPSUB));
  HIPCHK(pass_wait<P_HAPSUB, P_HAPLO>(b, st));   // the pass may have run on another stream
  HIPCHK(pass_mark(b, P_HAPSUB, 0, st));
  HIPCHK(hipMemsetAsync(b->hs_res, 0, std::max<size_t>(npairs, 1) * 4, st));
  if (cols) {
    HIPCHK(hipMemcpyAsync(b->hs_cls, b->hp_cls, std::max<size_t>(np, 1), hipMemcpyDeviceToDevice, st));
    if (ne) HIPCHK(hipMemcpyAsync(b->hs_ecls, b->hp_ecls, ne, hipMemcpyDeviceToDevice, st));
  }
  HapSubParams P;
  memset(&P, 0, sizeof P);
  P.vcfs = b->hp_vcfs;
  P.pos = b->pos; P.ref = b->ref; P.alt = b->alt; P.flags = b->flags; P.mask_tp = b->mask_tp;
  P.cls = b->hp_cls; P.ecls = cols ? (const uint8_t*)b->hp_ecls : nullptr;
  P.rec = b->hp_rec; P.tru = b->hp_tru;
  P.pairs = b->hp_pairs; P.n_pairs = b->hp_npairs;
  P.sub = b->hs_sub; P.res = b->hs_res;
  P.cls_s = cols ? (uint8_t*)b->hs_cls : nullptr; P.ecls_s = cols ? (uint8_t*)b->hs_ecls : nullptr;
  P.n_vcf = (int32_t)nv; P.narrow = (what & QM_HAPSUB_NARROW_HASH) ? 1 : 0;
  launch_hap_subsets(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_mark(b, P_HAPSUB, 1, st));
  HIPCHK(pass_done(b, P_HAPSUB, st, 1u | what));
  return QM_OK;
}
extern "C" int qm_batch_get_hapsubsets(qm_batch* b, uint64_t* sub) {
  NEED_PASS(b, P_HAPLO, "qm_batch_get_hapsubsets");
  if (pass_ran(b, P_HAPSUB, "qm_batch_get_hapsubsets") != QM_OK) return QM_E_STATE;
  HIPCHK(pass_result(b, P_HAPSUB));
  const size_t nv = (size_t)b->n_vcf;
  if (sub && nv) HIPCHK(hipMemcpy(sub, b->hs_sub, nv * HAPSUB_COLS * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_hapsubsetted(qm_batch* b, int v, uint8_t* cls_s, uint8_t* entry_cls_s, int32_t* site_s, uint8_t* smask, uint8_t* tmask,
                                         int64_t capacity, int64_t* n_out) {
  NEED_PASS(b, P_HAPLO, "qm_batch_get_hapsubsetted");
  if (pass_ran(b, P_HAPSUB, "qm_batch_get_hapsubsetted") != QM_OK) return QM_E_STATE;
  if (v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_hapsubsetted: VCF %d (the batch has %d)", v, b->n_vcf);
  if (capacity < 0) return fail(QM_E_INVAL, "qm_batch_get_hapsubsetted: capacity %lld", (long long)capacity);
  if (!b->hp_has[(size_t)v]) return fail(QM_E_STATE, "qm_batch_get_hapsubsetted: VCF %d named no genome in the latest qm_batch_haplotypes", v);
  if ((cls_s || entry_cls_s) && !(b->pass[P_HAPSUB].made & QM_HAPSUB_COLUMNS))
    return fail(QM_E_STATE, "qm_batch_get_hapsubsetted: the latest qm_batch_hapsubsets did not keep the columns (QM_HAPSUB_COLUMNS)");
  HIPCHK(pass_result(b, P_HAPSUB));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  const size_t n = (size_t)d.n, ne = (size_t)(b->hp_eoff[(size_t)v + 1] - b->hp_eoff[(size_t)v]);
  if (cls_s && n) HIPCHK(hipMemcpy(cls_s, b->hs_cls + d.off, n, hipMemcpyDeviceToHost));
  if (entry_cls_s && ne) HIPCHK(hipMemcpy(entry_cls_s, b->hs_ecls + b->hp_eoff[(size_t)v], ne, hipMemcpyDeviceToHost));
  if (!b->hs_listed) {   // the PARTIAL pairs, once per search: the pairs are numbered VCF after VCF, sites ascending
    const size_t npairs = (size_t)b->hp_npairs;
    std::vector<uint32_t> res(npairs);
    std::vector<int32_t> vs(2 * npairs);
    if (npairs) {
      HIPCHK(hipMemcpy(res.data(), b->hs_res, npairs * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy2D(vs.data(), 8, b->hp_pairs, (size_t)HAP_PAIR_WORDS * 4, 8, npairs, hipMemcpyDeviceToHost));
    }
    b->hs_list.clear();
    for (size_t k = 0; k < npairs; ++k)
      if (res[k] & HAPSUB_RES_PARTIAL) {
        b->hs_list.push_back(vs[2 * k]); b->hs_list.push_back(vs[2 * k + 1]);
        b->hs_list.push_back((int32_t)((res[k] >> 8) & 255u)); b->hs_list.push_back((int32_t)(res[k] & 255u));
      }
    b->hs_listed = true;
  }
  int64_t m = 0;
  for (size_t k = 0; k + 3 < b->hs_list.size(); k += 4) {
    if (b->hs_list[k] != v) continue;
    if (m < capacity) {
      if (site_s) site_s[m] = b->hs_list[k + 1];
      if (smask) smask[m] = (uint8_t)b->hs_list[k + 2];
      if (tmask) tmask[m] = (uint8_t)b->hs_list[k + 3];
    }
    ++m;
  }
  if (n_out) *n_out = m;
  if (m > capacity && (site_s || smask || tmask))
    return fail(QM_E_RANGE, "qm_batch_get_hapsubsetted: %lld PARTIAL sites, room for %lld", (long long)m, (long long)capacity);
  return QM_OK;
}
extern "C" int qm_batch_hapsubset_timings(qm_batch* b, float* ms1) {
  if (!b || !ms1) return fail(QM_E_INVAL, "qm_batch_hapsubset_timings: NULL");
  if (pass_ran(b, P_HAPLO, "qm_batch_hapsubset_timings") != QM_OK) return QM_E_STATE;
  return pass_timings(b, P_HAPSUB, "qm_batch_hapsubset_timings", ms1);
}
extern "C" int qm_truth_sites(qm_ctx* c, int truth_id, int genome_id, int gap, int32_t* first_entry, int32_t* lo, int32_t* hi, int64_t capacity,
                              int64_t* n_out) {
  if (!c || !n_out || capacity < 0) return fail(QM_E_INVAL, "qm_truth_sites: bad arguments");
  if (gap < 0 || gap > QM_HAP_MAX_GAP) return fail(QM_E_INVAL, "qm_truth_sites: gap %d (0 to %d)", gap, QM_HAP_MAX_GAP);
  if (truth_id < 0 || truth_id >= (int)c->truths.size() || c->truths[(size_t)truth_id].released)
    return fail(QM_E_INVAL, "qm_truth_sites: no live truth set %d", truth_id);
  if (genome_id < 0 || genome_id >= (int)c->genomes.size() || c->genomes[(size_t)genome_id].released)
    return fail(QM_E_INVAL, "qm_truth_sites: no live genome %d", genome_id);
  HIPCHK(hipSetDevice(c->dev));
  const Truth& t = c->truths[(size_t)truth_id];
  const size_t xn = (size_t)t.xn;
  std::vector<int32_t> h(3 * xn + 3);   // slo | shi | sfirst[xn + 1] | n_sites
  const int rc = build_and_read(c, "qm_truth_sites", hap_pool_words(t.xn), h.data(), h.size() * 4, [&](uint32_t* pool, const void** src) {
    const HapSites S = hap_sites(t, c->genomes[(size_t)genome_id], gap, pool);
    *src = S.slo;
    return hap_build(S, c->stream);
  });
  if (rc != QM_OK) return rc;
  const int64_t ns = h[3 * xn + 1];
  *n_out = ns;
  if (ns > capacity) return fail(QM_E_RANGE, "qm_truth_sites: %lld sites, room for %lld", (long long)ns, (long long)capacity);
  for (int64_t s = 0; s < ns; ++s) {
    if (first_entry) first_entry[s] = h[2 * xn + (size_t)s];
    if (lo) lo[s] = h[(size_t)s];
    if (hi) hi[s] = h[xn + (size_t)s];
  }
  return QM_OK;
}
// paired block-bootstrap replicates of the finished batch's counts
extern "C" int qm_boot_draws(uint64_t seed, int32_t n_win, int32_t n_rep, uint16_t* mult) {
  if (n_win < 1 || n_win > QM_BOOT_MAX_WINDOWS || n_rep < 0 || n_rep > QM_BOOT_MAX_REP || (n_rep > 0 && !mult))
    return fail(QM_E_INVAL, "qm_boot_draws: n_win = %d (1 to %d), n_rep = %d (0 to %d)", n_win, QM_BOOT_MAX_WINDOWS, n_rep, QM_BOOT_MAX_REP);
  if (n_rep) memset(mult, 0, sizeof(uint16_t) * (size_t)n_rep * (size_t)n_win);
  for (int32_t r = 0; r < n_rep; ++r)
    for (int32_t j = 0; j < n_win; ++j) ++mult[(size_t)r * (size_t)n_win + boot_draw(seed, (uint32_t)r, (uint32_t)j, (uint32_t)n_win)];
  return QM_OK;
}
extern "C" int qm_batch_boot(qm_batch* b, int32_t window, int32_t n_win, int32_t n_rep, uint64_t seed, unsigned what, void* stream) {
  NEED_FINISHED(b, "qm_batch_boot");
  qm_ctx* c = b->ctx;
  if (window < 1) return fail(QM_E_INVAL, "qm_batch_boot: window = %d (at least 1)", window);
  if (n_win < 1 || n_win > QM_BOOT_MAX_WINDOWS) return fail(QM_E_INVAL, "qm_batch_boot: n_win = %d (1 to %d)", n_win, QM_BOOT_MAX_WINDOWS);
  if (n_rep < 0 || n_rep > QM_BOOT_MAX_REP) return fail(QM_E_INVAL, "qm_batch_boot: n_rep = %d (0 to %d)", n_rep, QM_BOOT_MAX_REP);
  if (!what || (what & ~(QM_BOOT_RECORDS | QM_BOOT_TRUTH))) return fail(QM_E_INVAL, "qm_batch_boot: what = %u", what);
  if (what & QM_BOOT_TRUTH) {
    if (b->ext) return fail(QM_E_STATE, "qm_batch_boot: allele-extended batches have no truth-side bitmaps (QM_BOOT_RECORDS only)");
    if (pass_needs<P_BOOT, P_TRUTH>(b, "QM_BOOT_TRUTH") != QM_OK) return QM_E_STATE;
    const int rc = truths_live(b, "qm_batch_boot");
    if (rc != QM_OK) return rc;
  }
  OPEN_PASS(b, P_BOOT, stream, st);
  const size_t nv = (size_t)b->n_vcf;
  b->pass[P_BOOT].made = 0;
  const size_t cw = nv * (size_t)(n_win + 2) * BOOT_COLS, rw = nv * (size_t)n_rep * BOOT_COLS;
  int rc = b->d_bcnt.grow((int64_t)std::max<size_t>(cw, 1), &b->dev_bytes);
  if (rc == QM_OK && n_rep) rc = b->d_brep.grow((int64_t)std::max<size_t>(rw, 1), &b->dev_bytes);
  if (rc == QM_OK && (what & QM_BOOT_TRUTH)) rc = b->d_brows.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(hipMemsetAsync(b->d_bcnt, 0, cw * 8, st));
  if (what & QM_BOOT_RECORDS) {
    BootRecParams P;
    P.spans = b->d_spans; P.pos = b->pos; P.flags = b->flags;
    P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
    P.cnt = b->d_bcnt;
    P.n_spans = (int32_t)b->L.spans.size();
    P.window = window; P.n_win = n_win; P.div = boot_div(window);
    launch_boot_records(P, st);
    HIPCHK(hipGetLastError());
  }
  if ((what & QM_BOOT_TRUTH) && nv) {
    std::vector<BootTruthRow> rows(nv);
    for (size_t v = 0; v < nv; ++v) {
      rows[v].keys = c->truths[(size_t)b->L.vcfs[v].truth].d_keys;
      rows[v].hits = b->d_hits + b->h_hit_off[v];
      rows[v].n = b->h_hit_tn[v];   // T' as the hit bitmaps were sized
    }
    HIPCHK(pass_wait<P_BOOT, P_TRUTH>(b, st));   // the hit bitmaps, on whatever stream they were made
    HIPCHK(hipMemcpy(b->d_brows, rows.data(), nv * sizeof(BootTruthRow), hipMemcpyHostToDevice));   // blocking: rows dies here
    launch_boot_truth(b->d_brows, (int)nv, window, n_win, b->d_bcnt, st);
    HIPCHK(hipGetLastError());
  }
  launch_boot_resample(b->d_bcnt, (int)nv, n_win, n_rep, seed, b->d_brep, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_done(b, P_BOOT, st, what));
  b->boot_nwin = n_win;
  b->boot_nrep = n_rep;
  return QM_OK;
}
extern "C" int qm_batch_get_boot(qm_batch* b, uint64_t* cnt, uint64_t* rep) {
  NEED_PASS(b, P_BOOT, "qm_batch_get_boot");
  HIPCHK(pass_result(b, P_BOOT));
  const size_t nv = (size_t)b->n_vcf;
  if (cnt && nv) HIPCHK(hipMemcpy(cnt, b->d_bcnt, nv * (size_t)(b->boot_nwin + 2) * BOOT_COLS * 8, hipMemcpyDeviceToHost));
  if (rep && nv && b->boot_nrep) HIPCHK(hipMemcpy(rep, b->d_brep, nv * (size_t)b->boot_nrep * BOOT_COLS * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
// the truth-side view of the finished batch
extern "C" int qm_batch_truth_hits(qm_batch* b, void* stream) {
  NEED_FINISHED(b, "qm_batch_truth_hits");
  qm_ctx* c = b->ctx;
  if (b->ext) return fail(QM_E_STATE, "qm_batch_truth_hits: allele-extended batches have no truth-side bitmaps (single-base batches only)");
  int rc = truths_live(b, "qm_batch_truth_hits");
  if (rc != QM_OK) return rc;
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  const size_t nv = (size_t)b->n_vcf;
  const size_t mask_words = (size_t)b->L.n_pad / 64 + 64;   // as mask_pass
  // first use: every buffer guarded on its own (a call that failed half way leaks nothing when it is repeated); the sizes follow
  // from the truth sets' T', which cannot change while the generations above hold
  if (b->h_hit_tn.empty()) {
    b->h_hit_off.assign(nv + 1, 0);
    b->h_hit_tn.assign(nv, 0);
    for (size_t v = 0; v < nv; ++v) {
      b->h_hit_tn[v] = c->truths[(size_t)b->L.vcfs[v].truth].n;
      b->h_hit_off[v + 1] = b->h_hit_off[v] + (b->h_hit_tn[v] + 31) / 32;
    }
  }
  const size_t hw = std::max<size_t>((size_t)b->h_hit_off[nv], 1);
  if (!b->pass[P_TRUTH].done) HIPCHK(hipEventCreateWithFlags(&b->pass[P_TRUTH].done, hipEventDisableTiming));
  else if (b->hits_enqueued) HIPCHK(hipStreamWaitEvent(st, b->pass[P_TRUTH].done, 0));   // an earlier pass, on whatever stream, still writes the same buffers
  rc = wait_passes(b, st, false, true);   // and the passes that read the hit bitmaps, on whatever stream (READS)
  if (rc != QM_OK) return rc;
  // (the one pass that does not open with pass_open: a stream wait, not a host wait -- the host reads nothing the pass leaves here)
  rc = b->d_hit_off.grow((int64_t)nv + 1, &b->dev_bytes);
  if (rc == QM_OK) rc = b->d_intruth.grow((int64_t)mask_words, &b->dev_bytes);
  if (rc == QM_OK) rc = b->d_hits.grow((int64_t)hw, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  if (!b->hit_off_uploaded) {
    HIPCHK(hipMemcpy(b->d_hit_off, b->h_hit_off.data(), (nv + 1) * 8, hipMemcpyHostToDevice));
    b->hit_off_uploaded = true;
  }
  if (!b->intruth_cleared) {
    HIPCHK(hipMemsetAsync(b->d_intruth, 0, mask_words * 8, st));   // the bytes between the VCFs are never written again
    b->intruth_cleared = true;
  }
  HIPCHK(hipMemsetAsync(b->d_hits, 0, hw * 4, st));
  TruthHitsParams P;
  P.spans = b->d_spans; P.truths = c->d_truths; P.hit_off = b->d_hit_off;
  P.pos = b->pos; P.anib = b->anib; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  P.hits = b->d_hits; P.mask_intruth = reinterpret_cast<uint8_t*>(b->d_intruth.p);
  P.n_spans = (int32_t)b->L.spans.size();
  launch_truth_hits(P, st);
  HIPCHK(hipGetLastError());
  HIPCHK(pass_done(b, P_TRUTH, st, 1));
  b->hits_enqueued = true;
  return QM_OK;
}
extern "C" int qm_batch_get_truth_hits(qm_batch* b, int v, uint32_t* bits, int64_t n_words) {
  NEED_PASS(b, P_TRUTH, "qm_batch_get_truth_hits");
  if (v < 0 || v >= b->n_vcf || (!bits && n_words)) return fail(QM_E_INVAL, "qm_batch_get_truth_hits: bad arguments");
  const int64_t have = b->h_hit_off[(size_t)v + 1] - b->h_hit_off[(size_t)v];
  if (n_words != have) return fail(QM_E_INVAL, "qm_batch_get_truth_hits: VCF %d has %lld words, not %lld", v, (long long)have, (long long)n_words);
  HIPCHK(pass_result(b, P_TRUTH));
  if (have) HIPCHK(hipMemcpy(bits, b->d_hits + b->h_hit_off[(size_t)v], (size_t)have * 4, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_intruth_mask(qm_batch* b, int v, uint64_t* mask) {
  NEED_PASS(b, P_TRUTH, "qm_batch_get_intruth_mask");
  if (v < 0 || v >= b->n_vcf || !mask) return fail(QM_E_INVAL, "qm_batch_get_intruth_mask: bad arguments");
  HIPCHK(pass_result(b, P_TRUTH));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  const size_t nw = (size_t)((d.n + 63) / 64);
  if (nw) {
    HIPCHK(hipMemcpy(mask, b->d_intruth + (d.off >> 6), nw * 8, hipMemcpyDeviceToHost));
    if (d.n & 63) mask[nw - 1] &= (1ull << (d.n & 63)) - 1ull;
  }
  return QM_OK;
}
extern "C" int qm_batch_truth_regions(qm_batch* b, int n_groups, const int32_t* group_offsets, const int32_t* vcf_ids, uint64_t* regions,
                                      uint32_t* union_bits) {
  NEED_PASS(b, P_TRUTH, "qm_batch_truth_regions");
  if (n_groups < 0 || (n_groups && (!group_offsets || !vcf_ids || !regions))) return fail(QM_E_INVAL, "qm_batch_truth_regions: bad arguments");
  if (n_groups == 0) return QM_OK;
  std::vector<TruthGroup> G((size_t)n_groups);
  std::vector<int64_t> uoff((size_t)n_groups + 1, 0);
  int64_t max_words = 0;
  for (int g = 0; g < n_groups; ++g) {
    TruthGroup& t = G[(size_t)g];
    const int32_t* ids = vcf_ids + group_offsets[g];
    const int rc = walk_hit_group(b, "qm_batch_truth_regions", g, group_offsets, vcf_ids, TS_MAX_GROUP, t, [&](int i, int v) {
      return std::find(ids, ids + i, v) == ids + i ? QM_OK : fail(QM_E_INVAL, "qm_batch_truth_regions: group %d names VCF %d twice", g, v);
    });
    if (rc != QM_OK) return rc;
    uoff[(size_t)g + 1] = uoff[(size_t)g] + t.words;
    max_words = std::max(max_words, t.words);
  }
  qm_ctx* c = b->ctx;
  HIPCHK(pass_result(b, P_TRUTH));
  TruthGroup* d_groups = nullptr;
  unsigned long long* d_reg = nullptr;
  uint32_t* d_uni = nullptr;
  int rc = dalloc(&d_groups, (size_t)n_groups);
  if (rc == QM_OK) rc = dalloc(&d_reg, (size_t)n_groups * TS_REGIONS);
  if (rc == QM_OK && union_bits) rc = dalloc(&d_uni, (size_t)uoff[(size_t)n_groups]);
  hipError_t e = hipSuccess;
  if (rc == QM_OK) {
    if (d_uni) for (int g = 0; g < n_groups; ++g) G[(size_t)g].uni = d_uni + uoff[(size_t)g];
    e = hipMemcpyAsync(d_groups, G.data(), sizeof(TruthGroup) * (size_t)n_groups, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_reg, 0, (size_t)n_groups * TS_REGIONS * 8, c->stream);
    if (e == hipSuccess) { launch_truth_regions(d_groups, n_groups, max_words, d_reg, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(regions, d_reg, (size_t)n_groups * TS_REGIONS * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && d_uni && uoff[(size_t)n_groups])
      e = hipMemcpyAsync(union_bits, d_uni, (size_t)uoff[(size_t)n_groups] * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (G stays alive until here)
  }
  (void)hipFree(d_groups); (void)hipFree(d_reg); (void)hipFree(d_uni);
  if (rc != QM_OK) return rc;
  if (e != hipSuccess) return fail(QM_E_HIP, "qm_batch_truth_regions: %s", hipGetErrorString(e));
  return QM_OK;
}
// k-of-n consensus over groups of the finished batch's VCFs
extern "C" int qm_batch_votes(qm_batch* b, int n_groups, const int32_t* group_offsets, const int32_t* vcf_ids, void* stream) {
  NEED_FINISHED(b, "qm_batch_votes");
  if (b->ext) return fail(QM_E_STATE, "qm_batch_votes: allele-extended batches have no truth-side bitmaps (single-base batches only)");
  if (pass_needs<P_VOTES, P_TRUTH>(b) != QM_OK) return QM_E_STATE;
  int rc = truths_live(b, "qm_batch_votes");
  if (rc != QM_OK) return rc;
  if (n_groups < 0 || (n_groups && (!group_offsets || !vcf_ids))) return fail(QM_E_INVAL, "qm_batch_votes: bad arguments");
  if (n_groups >= (1 << 23)) return fail(QM_E_LIMIT, "qm_batch_votes: %d groups", n_groups);
  const size_t nv = (size_t)b->n_vcf, ng = (size_t)n_groups;
  std::vector<int32_t> slot(std::max<size_t>(nv, 1), -1);
  std::vector<VoteGroup> G(std::max<size_t>(ng, 1));
  int64_t max_words = 0;
  for (int g = 0; g < n_groups; ++g) {
    VoteGroup& t = G[(size_t)g];
    rc = walk_hit_group(b, "qm_batch_votes", g, group_offsets, vcf_ids, VT_MAX_GROUP, t, [&](int i, int v) {
      if (slot[(size_t)v] >= 0) return fail(QM_E_INVAL, "qm_batch_votes: VCF %d sits in groups %d and %d (at most one)", v, slot[(size_t)v] >> 8, g);
      slot[(size_t)v] = (int32_t)(((uint32_t)g << 8) | (uint32_t)i);
      return (int)QM_OK;
    });
    if (rc != QM_OK) return rc;
    max_words = std::max(max_words, t.words);
  }
  OPEN_PASS(b, P_VOTES, stream, st);
  // a group's segment of the pair buffers holds its members' kept lines: the finished n_pass scalars bound the pairs from above
  std::vector<int64_t> sc(std::max<size_t>(nv, 1) * QM_N_SCALARS, 0);
  if (nv) HIPCHK(hipMemcpy(sc.data(), b->scalars, nv * QM_N_SCALARS * 8, hipMemcpyDeviceToHost));
  std::vector<SortSeg> segs(std::max<size_t>(ng, 1));
  std::vector<int32_t> tile_seg;
  int64_t koff = 0;
  for (int g = 0; g < n_groups; ++g) {
    SortSeg& s = segs[(size_t)g];
    memset(&s, 0, sizeof s);
    for (int32_t o = group_offsets[g]; o < group_offsets[g + 1]; ++o) s.n += std::max<int64_t>(sc[(size_t)vcf_ids[o] * QM_N_SCALARS + QM_S_NPASS], 0);
    s.koff = koff;
    s.tile0 = (int32_t)tile_seg.size();
    s.hoff = (int64_t)s.tile0 * 256;
    s.ntiles = (int32_t)((s.n + SORT_TILE - 1) / SORT_TILE);
    koff += (s.n + 63) & ~(int64_t)63;
    if (koff > 0x7fff0000ll) return fail(QM_E_LIMIT, "qm_batch_votes: the groups' members hold more than 2^31 kept lines");
    tile_seg.insert(tile_seg.end(), (size_t)s.ntiles, (int32_t)g);
  }
  const int64_t nst = (int64_t)tile_seg.size();
  const size_t out_words = ng * (2 * VT_SLOTS + 2 * VT_MAX_GROUP + 1);
  for (int i = 0; i < 2 && rc == QM_OK; ++i) {   // the sort kernels read whole 16-byte pieces
    rc = b->vt_k[i].grow(koff + 64, &b->dev_bytes);
    if (rc == QM_OK) rc = b->vt_v[i].grow(koff + 64, &b->dev_bytes);
  }
  if (rc == QM_OK) rc = b->vt_hist.grow(std::max<int64_t>(nst * 256, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_thd.grow(std::max<int64_t>(nst * VT_RUN_PER_SORT, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_cursor.grow((int64_t)std::max<size_t>(2 * ng, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_segs.grow((int64_t)std::max<size_t>(ng, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_tile_seg.grow(std::max<int64_t>(nst, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_slot.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_groups.grow((int64_t)std::max<size_t>(ng, 1), &b->dev_bytes);
  if (rc == QM_OK) rc = b->vt_out.grow((int64_t)std::max<size_t>(out_words, 1), &b->dev_bytes);
  // (growing keeps what fits: a call refused up to here leaves the previous pass and its outputs as they were, unless an
  //  array had to be replaced and then could not be)
  if (rc != QM_OK) { b->pass[P_VOTES].made = 0; return rc; }
  b->pass[P_VOTES].made = 0;   // from here on the outputs are rewritten
  b->vt_koff.assign(ng + 1, 0);
  for (size_t g = 0; g < ng; ++g) b->vt_koff[g] = segs[g].koff;
  b->vt_koff[ng] = koff;
  b->votes_groups = n_groups;
  if (n_groups == 0) {
    HIPCHK(pass_done(b, P_VOTES, st, 1));
    return QM_OK;
  }
  // blocking copies: the tables die here
  HIPCHK(hipMemcpy(b->vt_segs, segs.data(), ng * sizeof(SortSeg), hipMemcpyHostToDevice));
  if (nst) HIPCHK(hipMemcpy(b->vt_tile_seg, tile_seg.data(), (size_t)nst * 4, hipMemcpyHostToDevice));
  if (nv) HIPCHK(hipMemcpy(b->vt_slot, slot.data(), nv * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->vt_groups, G.data(), ng * sizeof(VoteGroup), hipMemcpyHostToDevice));
  HIPCHK(pass_wait<P_VOTES, P_TRUTH>(b, st));   // the hit bitmaps and the record mask, on whatever stream they were made
  HIPCHK(hipMemsetAsync(b->vt_out, 0, out_words * 8, st));
  HIPCHK(hipMemsetAsync(b->vt_cursor, 0, 2 * ng * 4, st));
  VoteOut O;
  O.tp = reinterpret_cast<unsigned long long*>(b->vt_out.p);
  O.fp = O.tp + ng * VT_SLOTS;
  O.ptp = O.fp + ng * VT_SLOTS;
  O.pfp = O.ptp + ng * VT_MAX_GROUP;
  O.nokey = O.pfp + ng * VT_MAX_GROUP;
  HIPCHK(pass_marks(b, P_VOTES));
  HIPCHK(pass_mark(b, P_VOTES, 0, st));
  launch_vote_truth(b->vt_groups, n_groups, max_words, O, st);
  HIPCHK(pass_mark(b, P_VOTES, 1, st));
  VoteKeysParams P;
  P.spans = b->d_spans; P.vcf_slot = b->vt_slot; P.segs = b->vt_segs;
  P.pos = b->pos; P.anib = b->anib; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_intruth = b->d_intruth;
  P.cursor = b->vt_cursor; P.keys = b->vt_k[0]; P.vals = b->vt_v[0]; P.nokey = O.nokey;
  P.n_spans = (int32_t)b->L.spans.size();
  launch_vote_keys(P, st);
  launch_vote_segs(b->vt_segs, b->vt_cursor, n_groups, st);
  HIPCHK(pass_mark(b, P_VOTES, 2, st));
  int cur = 0;
  for (int shift = 0; shift < 32; shift += 8) {
    launch_sort_pass(b->vt_segs, b->vt_tile_seg, n_groups, (int)nst, b->vt_k[cur], nullptr, b->vt_v[cur], shift, b->vt_hist, b->vt_k[cur ^ 1], nullptr,
                     b->vt_v[cur ^ 1], 0, st);
    cur ^= 1;
  }
  HIPCHK(pass_mark(b, P_VOTES, 3, st));
  // (four passes: the sorted pairs are back in the first pair of buffers, the second takes the distinct keys and masks)
  launch_vote_runs(b->vt_segs, b->vt_tile_seg, n_groups, (int)nst, b->vt_k[0], b->vt_v[0], b->vt_thd, b->vt_k[1], b->vt_v[1], b->vt_cursor + ng, O, st);
  HIPCHK(pass_mark(b, P_VOTES, 4, st));
  HIPCHK(hipGetLastError());
  HIPCHK(pass_done(b, P_VOTES, st, 1));
  return QM_OK;
}
extern "C" int qm_batch_vote_timings(qm_batch* b, float* ms4) {
  if (!b || !ms4) return fail(QM_E_INVAL, "qm_batch_vote_timings: NULL");
  if (!b->pass[P_VOTES].made || !b->pass[P_VOTES].timed)   // (one message for both)
    return fail(QM_E_STATE, "qm_batch_vote_timings: timing is off or no qm_batch_votes behind the latest run");
  return pass_timings(b, P_VOTES, "qm_batch_vote_timings", ms4);
}
extern "C" int qm_batch_get_votes(qm_batch* b, uint64_t* tp_votes, uint64_t* fp_votes, uint64_t* private_tp, uint64_t* private_fp, int64_t* nokey) {
  NEED_PASS(b, P_VOTES, "qm_batch_get_votes");
  HIPCHK(pass_result(b, P_VOTES));
  const size_t ng = (size_t)b->votes_groups;
  if (!ng) return QM_OK;
  const uint64_t* o = b->vt_out;
  if (tp_votes) HIPCHK(hipMemcpy(tp_votes, o, ng * VT_SLOTS * 8, hipMemcpyDeviceToHost));
  o += ng * VT_SLOTS;
  if (fp_votes) HIPCHK(hipMemcpy(fp_votes, o, ng * VT_SLOTS * 8, hipMemcpyDeviceToHost));
  o += ng * VT_SLOTS;
  if (private_tp) HIPCHK(hipMemcpy(private_tp, o, ng * VT_MAX_GROUP * 8, hipMemcpyDeviceToHost));
  o += ng * VT_MAX_GROUP;
  if (private_fp) HIPCHK(hipMemcpy(private_fp, o, ng * VT_MAX_GROUP * 8, hipMemcpyDeviceToHost));
  o += ng * VT_MAX_GROUP;
  if (nokey) HIPCHK(hipMemcpy(nokey, o, ng * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_vote_groups(qm_batch* b) {
  NEED_PASS(b, P_VOTES, "qm_batch_vote_groups");
  return b->votes_groups;
}
extern "C" int qm_batch_get_vote_keys(qm_batch* b, int group, uint32_t* keys, uint32_t* masks, int64_t capacity, int64_t* n_out) {
  NEED_PASS(b, P_VOTES, "qm_batch_get_vote_keys");
  if (group < 0 || group >= b->votes_groups || capacity < 0) return fail(QM_E_INVAL, "qm_batch_get_vote_keys: group %d (the pass had %d)", group, b->votes_groups);
  HIPCHK(pass_result(b, P_VOTES));
  uint32_t n = 0;
  HIPCHK(hipMemcpy(&n, b->vt_cursor + (size_t)b->votes_groups + (size_t)group, 4, hipMemcpyDeviceToHost));
  if (n_out) *n_out = (int64_t)n;
  if (!keys && !masks) return QM_OK;   // (the count alone)
  if ((int64_t)n > capacity) return fail(QM_E_INVAL, "qm_batch_get_vote_keys: group %d has %u distinct keys, capacity %lld", group, n, (long long)capacity);
  const int64_t off = b->vt_koff[(size_t)group];
  if (n && keys) HIPCHK(hipMemcpy(keys, b->vt_k[1] + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (n && masks) HIPCHK(hipMemcpy(masks, b->vt_v[1] + off, (size_t)n * 4, hipMemcpyDeviceToHost));
  return QM_OK;
}
// why a line is FP and a truth key FN: the near-miss classes of the finished batch
extern "C" int qm_batch_nearmiss(qm_batch* b, int32_t radius, void* stream) {
  NEED_FINISHED(b, "qm_batch_nearmiss");
  if (b->ext) return fail(QM_E_STATE, "qm_batch_nearmiss: allele-extended batches have no truth-side bitmaps (single-base batches only)");
  if (pass_needs<P_NEARMISS, P_TRUTH>(b) != QM_OK) return QM_E_STATE;
  if (radius < 0 || radius > QM_NM_MAX_RADIUS) return fail(QM_E_INVAL, "qm_batch_nearmiss: radius %d (0 to %d)", radius, QM_NM_MAX_RADIUS);
  qm_ctx* c = b->ctx;
  int rc = truths_live(b, "qm_batch_nearmiss");
  if (rc != QM_OK) return rc;
  OPEN_PASS(b, P_NEARMISS, stream, st);
  const size_t nv = (size_t)b->n_vcf;
  const size_t hw = std::max<size_t>((size_t)b->h_hit_off[nv], 1);   // as d_hits
  const size_t out_words = std::max<size_t>(nv, 1) * (NM_R_CLASSES + NM_T_CLASSES);
  rc = b->nm_planes.grow((int64_t)(NM_PLANES * hw), &b->dev_bytes);
  if (rc == QM_OK) rc = b->nm_rcls.grow(b->L.n_pad, &b->dev_bytes);
  if (rc == QM_OK) rc = b->nm_out.grow((int64_t)out_words, &b->dev_bytes);
  if (rc == QM_OK) rc = b->nm_tn.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc != QM_OK) { b->pass[P_NEARMISS].made = 0; return rc; }
  b->pass[P_NEARMISS].made = 0;   // from here on the outputs are rewritten
  if (!b->nm_tn_uploaded && nv) {
    HIPCHK(hipMemcpy(b->nm_tn, b->h_hit_tn.data(), nv * 8, hipMemcpyHostToDevice));
    b->nm_tn_uploaded = true;
  }
  HIPCHK(pass_wait<P_NEARMISS, P_TRUTH>(b, st));   // the hit bitmaps, on whatever stream they were made
  HIPCHK(hipMemsetAsync(b->nm_planes, 0, NM_PLANES * hw * 4, st));
  HIPCHK(hipMemsetAsync(b->nm_out, 0, out_words * 8, st));
  NearmissParams P;
  P.spans = b->d_spans; P.truths = c->d_truths; P.hit_off = b->d_hit_off;
  P.pos = b->pos; P.anib = b->anib; P.flags = b->flags;
  P.mask_pass = b->mask_pass; P.mask_tp = b->mask_tp;
  P.planes = b->nm_planes; P.plane_words = (int64_t)hw; P.rcls = b->nm_rcls;
  P.rec = reinterpret_cast<unsigned long long*>(b->nm_out.p);
  P.n_spans = (int32_t)b->L.spans.size(); P.radius = radius;
  HIPCHK(pass_marks(b, P_NEARMISS));
  HIPCHK(pass_mark(b, P_NEARMISS, 0, st));
  launch_nearmiss_records(P, st);
  HIPCHK(pass_mark(b, P_NEARMISS, 1, st));
  NearmissTruthParams Q;
  Q.hit_off = b->d_hit_off; Q.hit_tn = b->nm_tn; Q.hits = b->d_hits; Q.planes = b->nm_planes; Q.plane_words = (int64_t)hw;
  Q.tru = P.rec + std::max<size_t>(nv, 1) * NM_R_CLASSES;
  int64_t max_words = 0;
  for (size_t v = 0; v < nv; ++v) max_words = std::max<int64_t>(max_words, b->h_hit_off[v + 1] - b->h_hit_off[v]);
  launch_nearmiss_truth(Q, b->n_vcf, max_words, st);
  HIPCHK(pass_mark(b, P_NEARMISS, 2, st));
  HIPCHK(hipGetLastError());
  HIPCHK(pass_done(b, P_NEARMISS, st, 1));
  return QM_OK;
}
extern "C" int qm_batch_nearmiss_timings(qm_batch* b, float* ms2) {
  NEED_PASS(b, P_NEARMISS, "qm_batch_nearmiss_timings");
  return pass_timings(b, P_NEARMISS, "qm_batch_nearmiss_timings", ms2);
}
extern "C" int qm_batch_get_nearmiss(qm_batch* b, uint64_t* rec, uint64_t* tru) {
  NEED_PASS(b, P_NEARMISS, "qm_batch_get_nearmiss");
  HIPCHK(pass_result(b, P_NEARMISS));
  const size_t nv = (size_t)b->n_vcf;
  if (!nv) return QM_OK;
  if (rec) HIPCHK(hipMemcpy(rec, b->nm_out, nv * NM_R_CLASSES * 8, hipMemcpyDeviceToHost));
  if (tru) HIPCHK(hipMemcpy(tru, b->nm_out + nv * NM_R_CLASSES, nv * NM_T_CLASSES * 8, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_nearmiss_cls(qm_batch* b, int v, uint8_t* out) {
  NEED_PASS(b, P_NEARMISS, "qm_batch_get_nearmiss_cls");
  if (v < 0 || v >= b->n_vcf || !out) return fail(QM_E_INVAL, "qm_batch_get_nearmiss_cls: bad arguments");
  HIPCHK(pass_result(b, P_NEARMISS));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  if (d.n) HIPCHK(hipMemcpy(out, b->nm_rcls + d.off, (size_t)d.n, hipMemcpyDeviceToHost));
  return QM_OK;
}
extern "C" int qm_batch_get_nearmiss_truth(qm_batch* b, int v, uint8_t* out) {
  NEED_PASS(b, P_NEARMISS, "qm_batch_get_nearmiss_truth");
  if (v < 0 || v >= b->n_vcf || !out) return fail(QM_E_INVAL, "qm_batch_get_nearmiss_truth: bad arguments");
  HIPCHK(pass_result(b, P_NEARMISS));
  const int64_t off = b->h_hit_off[(size_t)v], words = b->h_hit_off[(size_t)v + 1] - off, tn = b->h_hit_tn[(size_t)v];
  if (!words) return QM_OK;
  const size_t hw = std::max<size_t>((size_t)b->h_hit_off[(size_t)b->n_vcf], 1);
  std::vector<uint32_t> w((size_t)words * (NM_PLANES + 1));   // the hit words, then the four planes' (no per-key array on the device)
  HIPCHK(hipMemcpy(w.data(), b->d_hits + off, (size_t)words * 4, hipMemcpyDeviceToHost));
  for (int p = 0; p < NM_PLANES; ++p)
    HIPCHK(hipMemcpy(w.data() + (size_t)(p + 1) * (size_t)words, b->nm_planes + (size_t)p * hw + (size_t)off, (size_t)words * 4, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < words; ++i) {
    uint32_t x[NM_T_CLASSES];
    nearmiss_truth_word(~w[(size_t)i], w[(size_t)(words + i)], w[(size_t)(2 * words + i)], w[(size_t)(3 * words + i)], w[(size_t)(4 * words + i)], x);
    for (int64_t k = 32 * i; k < std::min<int64_t>(32 * i + 32, tn); ++k) {
      uint8_t cls = (uint8_t)NM_NONE;
      for (int t = 0; t < NM_T_CLASSES; ++t) if ((x[t] >> (k & 31)) & 1u) cls = (uint8_t)t;
      out[k] = cls;
    }
  }
  return QM_OK;
}
// the filter surface of the finished batch: TP, FP and found truth keys at every QUAL x AF threshold
extern "C" int qm_batch_surface(qm_batch* b, int32_t q_step, int32_t nq, int32_t na, void* stream) {
  NEED_FINISHED(b, "qm_batch_surface");
  if (b->ext) return fail(QM_E_STATE, "qm_batch_surface: allele-extended batches have no filter surface (single-base batches only)");
  if (q_step < 1 || q_step > QM_SF_MAX_QUAL_STEP) return fail(QM_E_INVAL, "qm_batch_surface: q_step %d (1 to %d)", q_step, QM_SF_MAX_QUAL_STEP);
  if (nq < 1 || nq > QM_SF_MAX_QUAL_BINS) return fail(QM_E_INVAL, "qm_batch_surface: nq %d (1 to %d)", nq, QM_SF_MAX_QUAL_BINS);
  if (na < 1 || na > QM_SF_MAX_AF_BINS) return fail(QM_E_INVAL, "qm_batch_surface: na %d (1 to %d)", na, QM_SF_MAX_AF_BINS);
  if (nq * na > QM_SF_MAX_CELLS) return fail(QM_E_INVAL, "qm_batch_surface: nq * na = %d cells (at most %d)", nq * na, QM_SF_MAX_CELLS);
  qm_ctx* c = b->ctx;
  int rc = truths_live(b, "qm_batch_surface");
  if (rc != QM_OK) return rc;
  OPEN_PASS(b, P_SURFACE, stream, st);
  const size_t nv = (size_t)b->n_vcf, cells = (size_t)nq * (size_t)na;
  if (b->h_sf_off.empty()) {   // (T' cannot change while the generations truths_live checks hold)
    b->h_sf_off.assign(nv + 1, 0);
    for (size_t v = 0; v < nv; ++v) b->h_sf_off[v + 1] = b->h_sf_off[v] + c->truths[(size_t)b->L.vcfs[v].truth].n;
  }
  const size_t nbest = std::max<size_t>((size_t)b->h_sf_off[nv], 1);
  const size_t out_words = std::max<size_t>(nv, 1) * (SF_GRIDS * cells + SF_EXTRA);
  b->pass[P_SURFACE].made = 0;   // from here on the outputs are rewritten
  rc = b->sf_best.grow((int64_t)nbest, &b->dev_bytes);
  if (rc == QM_OK) rc = b->sf_off.grow((int64_t)nv + 1, &b->dev_bytes);
  if (rc == QM_OK) rc = b->sf_out.grow((int64_t)out_words, &b->dev_bytes);
  if (rc == QM_OK) rc = b->sf_mark.grow((int64_t)std::max<size_t>(nv, 1), &b->dev_bytes);
  if (rc != QM_OK) return rc;
  if (!b->sf_off_uploaded) {
    HIPCHK(hipMemcpy(b->sf_off, b->h_sf_off.data(), (nv + 1) * 8, hipMemcpyHostToDevice));
    b->sf_off_uploaded = true;
  }
  bool any_af = false;
  for (size_t v = 0; v < nv; ++v) any_af = any_af || b->h_afmark[v];
  if (nv) HIPCHK(hipMemcpy(b->sf_mark, b->h_afmark.data(), nv, hipMemcpyHostToDevice));   // blocking: the marks may change behind the call
  HIPCHK(hipMemsetAsync(b->sf_best, 0, nbest * 4, st));
  HIPCHK(hipMemsetAsync(b->sf_out, 0, out_words * 8, st));
  SurfaceParams P;
  P.spans = b->d_spans; P.truths = c->d_truths; P.has_af = b->sf_mark; P.best_off = b->sf_off;
  P.pos = b->pos; P.anib = b->anib; P.flags = b->flags; P.qual = b->qual;
  P.af = any_af ? b->d_af.p : nullptr;   // (no mark anywhere: there may be no column at all)
  P.best = b->sf_best;
  P.grid = reinterpret_cast<unsigned long long*>(b->sf_out.p);
  P.extra = P.grid + std::max<size_t>(nv, 1) * SF_GRIDS * cells;
  P.n_spans = (int32_t)b->L.spans.size();
  P.q_step = q_step; P.nq = nq; P.na = na;
  int64_t max_tn = 0;
  for (size_t v = 0; v < nv; ++v) max_tn = std::max<int64_t>(max_tn, b->h_sf_off[v + 1] - b->h_sf_off[v]);
  HIPCHK(pass_marks(b, P_SURFACE));
  HIPCHK(pass_mark(b, P_SURFACE, 0, st));
  launch_surface_records(P, st);
  HIPCHK(pass_mark(b, P_SURFACE, 1, st));
  launch_surface_truth(P, b->n_vcf, max_tn, st);
  HIPCHK(pass_mark(b, P_SURFACE, 2, st));
  launch_surface_sums(P, b->n_vcf, st);
  HIPCHK(pass_mark(b, P_SURFACE, 3, st));
  HIPCHK(hipGetLastError());
  HIPCHK(pass_done(b, P_SURFACE, st, 1));
  b->sf_cells = (int32_t)cells;
  return QM_OK;
}
extern "C" int qm_batch_surface_timings(qm_batch* b, float* ms3) {
  NEED_PASS(b, P_SURFACE, "qm_batch_surface_timings");
  return pass_timings(b, P_SURFACE, "qm_batch_surface_timings", ms3);
}
extern "C" int qm_batch_get_surface(qm_batch* b, uint64_t* S, uint64_t* extra) {
  NEED_PASS(b, P_SURFACE, "qm_batch_get_surface");
  HIPCHK(pass_result(b, P_SURFACE));
  const size_t nv = (size_t)b->n_vcf, gw = (size_t)SF_GRIDS * (size_t)b->sf_cells;
  if (!nv) return QM_OK;
  if (S) HIPCHK(hipMemcpy(S, b->sf_out, nv * gw * 8, hipMemcpyDeviceToHost));
  if (extra) {
    HIPCHK(hipMemcpy(extra, b->sf_out + nv * gw, nv * SF_EXTRA * 8, hipMemcpyDeviceToHost));
    for (size_t v = 0; v < nv; ++v) extra[v * SF_EXTRA + QM_SF_TRUTH] = (uint64_t)(b->h_sf_off[v + 1] - b->h_sf_off[v]);   // T', as the rows of `best` were sized
  }
  return QM_OK;
}
// dst[i] += src[i] for device arrays (qm_extract_files_ex adds the per-truth sums of its batch into the caller's buffer)
int qm_device_add_u64(qm_ctx* c, uint64_t* dst, const uint64_t* src, int64_t n) {
  if (!c || !dst || !src || n < 0) return fail(QM_E_INVAL, "qm_device_add_u64: bad arguments");
  HIPCHK(hipSetDevice(c->dev));
  launch_add_u64(dst, src, n, c->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return QM_OK;
}
// bytes of a device buffer cleared on the context's device (qm_extract_files_ex: the caller's per-truth-file sums)
int qm_device_zero(qm_ctx* c, void* dst, size_t bytes) {
  if (!c || (!dst && bytes)) return fail(QM_E_INVAL, "qm_device_zero: bad arguments");
  HIPCHK(hipSetDevice(c->dev));
  if (bytes) HIPCHK(hipMemsetAsync(dst, 0, bytes, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return QM_OK;
}
extern "C" int qm_path_stats_total(qm_ctx* c, int64_t* out) {
  if (!c || !out) return fail(QM_E_INVAL, "qm_path_stats_total: NULL");
  memcpy(out, c->path_total, sizeof c->path_total);
  return QM_OK;
}

extern "C" int qm_batch_path_stats(qm_batch* b, int64_t* out) {
  NEED_FINISHED(b, "qm_batch_path_stats");
  if (!out) return fail(QM_E_INVAL, "qm_batch_path_stats: NULL");
  memcpy(out, b->path_stats, sizeof b->path_stats);
  return QM_OK;
}
extern "C" int qm_batch_global_device(qm_batch* b, void** dev) {
  NEED_FINISHED(b, "qm_batch_global_device");
  if (!dev) return fail(QM_E_INVAL, "qm_batch_global_device: NULL");
  *dev = b->last_global;
  return QM_OK;
}
extern "C" int qm_batch_get_columns(qm_batch* b, int v, int32_t* pos, int32_t* ref, int32_t* alt, float* qual, uint8_t* flags) {
  if (!b || v < 0 || v >= b->n_vcf) return fail(QM_E_INVAL, "qm_batch_get_columns: bad arguments");
  HIPCHK(hipSetDevice(b->ctx->dev));
  const VcfDesc& d = b->L.vcfs[(size_t)v];
  const size_t n = (size_t)d.n;
  if (!n) return QM_OK;
  if (pos) HIPCHK(hipMemcpy(pos, b->pos + d.off, n * 4, hipMemcpyDeviceToHost));
  if (ref) HIPCHK(hipMemcpy(ref, b->ref + d.off, n * 4, hipMemcpyDeviceToHost));
  if (alt) HIPCHK(hipMemcpy(alt, b->alt + d.off, n * 4, hipMemcpyDeviceToHost));
  if (qual) HIPCHK(hipMemcpy(qual, b->qual + d.off, n * 4, hipMemcpyDeviceToHost));
  if (flags) HIPCHK(hipMemcpy(flags, b->flags + d.off, n, hipMemcpyDeviceToHost));
  return QM_OK;
}

// ---------------------------------------------------------------------------
// one-shot host-buffer entry point
// ---------------------------------------------------------------------------
extern "C" int qm_classify_batch(qm_ctx* c, int n_vcf, const int64_t* rec_offsets, const int32_t* pos, const int32_t* ref,
                                 const int32_t* alt, const float* qual, const uint8_t* flags, const int32_t* truth_id_per_vcf,
                                 int n_bins, uint8_t* out_cls, uint64_t* out_roc, int64_t* out_scalars, int32_t* out_idx,
                                 uint64_t* out_global) {
  return qm_classify_batch_ext(c, n_vcf, rec_offsets, pos, ref, alt, qual, flags, truth_id_per_vcf, n_bins, 0u, out_cls, out_roc,
                               out_scalars, out_idx, out_global);
}

extern "C" int qm_classify_batch_ext(qm_ctx* c, int n_vcf, const int64_t* rec_offsets, const int32_t* pos, const int32_t* ref,
                                     const int32_t* alt, const float* qual, const uint8_t* flags, const int32_t* truth_id_per_vcf,
                                     int n_bins, unsigned mode, uint8_t* out_cls, uint64_t* out_roc, int64_t* out_scalars,
                                     int32_t* out_idx, uint64_t* out_global) {
  if (!c || n_vcf <= 0 || !rec_offsets || !truth_id_per_vcf) return fail(QM_E_INVAL, "qm_classify_batch: bad arguments");
  std::vector<int64_t> n((size_t)n_vcf);
  for (int v = 0; v < n_vcf; ++v) {
    n[(size_t)v] = rec_offsets[v + 1] - rec_offsets[v];
    if (n[(size_t)v] < 0) return fail(QM_E_INVAL, "qm_classify_batch: rec_offsets must be non-decreasing");
  }
  qm_batch* b = nullptr;
  int rc = qm_batch_create_ext(c, n_vcf, n.data(), truth_id_per_vcf, n_bins, mode, &b);
  if (rc != QM_OK) return rc;
  for (int v = 0; v < n_vcf && rc == QM_OK; ++v) {
    const int64_t o = rec_offsets[v];
    rc = qm_batch_upload(b, v, pos + o, ref + o, alt + o, qual + o, flags + o);
  }
  if (rc == QM_OK) rc = qm_batch_run(b, nullptr, nullptr);
  if (rc == QM_OK) rc = qm_batch_finish(b, nullptr);
  for (int v = 0; v < n_vcf && rc == QM_OK; ++v) {
    if (out_cls) rc = qm_batch_get_cls(b, v, out_cls + rec_offsets[v]);
    if (rc == QM_OK && out_idx) rc = qm_batch_get_idx(b, v, out_idx + rec_offsets[v]);
  }
  if (rc == QM_OK && out_roc) rc = qm_batch_get_roc(b, out_roc);
  if (rc == QM_OK && out_scalars) rc = qm_batch_get_scalars(b, out_scalars);
  if (rc == QM_OK && out_global) rc = qm_batch_get_global(b, out_global);
  std::string keep = g_err;
  qm_batch_destroy(b);
  g_err = keep;
  return rc;
}

// ---------------------------------------------------------------------------
// self-contained synthetic run (for harnesses that are not Python)
// ---------------------------------------------------------------------------
extern "C" int qm_bench_synth(qm_ctx* c, const qm_synth_cfg* cfg, int n_vcf, int64_t records_per_vcf, int n_bins, int steps,
                              qm_bench_result* out) {
  if (!c || !cfg || !out || n_vcf <= 0 || records_per_vcf <= 0 || steps <= 0) return fail(QM_E_INVAL, "qm_bench_synth: bad arguments");
  int tid = -1;
  int rc = qm_truth_synth_ext(c, cfg->genome_len, cfg->truth_n, cfg->truth_seed, cfg->indel_pct, &tid);
  if (rc != QM_OK) return rc;
  std::vector<int64_t> n((size_t)n_vcf, records_per_vcf);
  std::vector<int32_t> tids((size_t)n_vcf, tid);
  qm_batch* b = nullptr;
  rc = qm_batch_create_ext(c, n_vcf, n.data(), tids.data(), n_bins, cfg->indel_pct > 0 ? QM_BATCH_ALLELES : 0u, &b);
  if (rc != QM_OK) { std::string keep = g_err; (void)qm_truth_release(c, tid); g_err = keep; return rc; }
  rc = qm_batch_synth(b, cfg);
  if (rc == QM_OK) rc = qm_batch_run(b, nullptr, nullptr);      // warm-up, also sorts what needs sorting once
  if (rc == QM_OK) rc = qm_batch_finish(b, nullptr);
  if (rc == QM_OK) rc = qm_batch_set_timing(b, 1);
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < steps && rc == QM_OK; ++i) {
    rc = qm_batch_run(b, nullptr, nullptr);
    if (rc == QM_OK && cfg->shuffled) rc = qm_batch_finish(b, nullptr);
  }
  if (rc == QM_OK) rc = qm_batch_finish(b, nullptr);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  float ms[4] = {0, 0, 0, 0};
  if (rc == QM_OK) rc = qm_batch_timings(b, ms);
  if (rc == QM_OK) {
    std::vector<int64_t> sc((size_t)n_vcf * QM_N_SCALARS);
    rc = qm_batch_get_scalars(b, sc.data());
    memset(out, 0, sizeof *out);
    out->records = (int64_t)n_vcf * records_per_vcf;
    out->seconds_per_step = sec / steps;
    out->classifications_per_s = (double)out->records * steps / sec;
    out->classify_ms = ms[0]; out->finalize_ms = ms[1]; out->compact_ms = ms[2];
    for (int v = 0; v < n_vcf; ++v) {
      out->kept += sc[(size_t)v * QM_N_SCALARS + QM_S_NPASS];
      out->tp_lines += sc[(size_t)v * QM_N_SCALARS + QM_S_TP_LINES];
      out->fp_lines += sc[(size_t)v * QM_N_SCALARS + QM_S_FP_LINES];
    }
    out->device_bytes = qm_batch_device_bytes(b);
  }
  std::string keep = g_err;
  qm_batch_destroy(b);
  (void)qm_truth_release(c, tid);   // the synthetic truth set belonged to this run only
  g_err = keep;
  return rc;
}

// ---------------------------------------------------------------------------
// what this GPU streams: the measured denominators beside the 8 TB/s of the data sheet
// ---------------------------------------------------------------------------
extern "C" int qm_bw_probe(qm_ctx* c, int64_t bytes, int reps, double* gbps3) {
  if (!c || !gbps3 || bytes < (1 << 20) || reps < 1) return fail(QM_E_INVAL, "qm_bw_probe: bad arguments");
  HIPCHK(hipSetDevice(c->dev));
  bytes &= ~(int64_t)4095;
  uint8_t *a = nullptr, *d = nullptr;
  uint32_t* sink = nullptr;
  int rc = dalloc(&a, (size_t)bytes);
  if (rc == QM_OK) rc = dalloc(&d, (size_t)bytes);
  if (rc == QM_OK) rc = dalloc(&sink, 1);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  auto done = [&](int r) { (void)hipFree(a); (void)hipFree(d); (void)hipFree(sink); if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); return r; };
  if (rc != QM_OK) return done(rc);
  hipError_t e = hipMemsetAsync(a, 1, (size_t)bytes, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(d, 2, (size_t)bytes, c->stream);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  if (e != hipSuccess) return done(fail(QM_E_HIP, "qm_bw_probe: %s", hipGetErrorString(e)));
  for (int mode = 0; mode < 3; ++mode) {   // 0 read only, 1 copy (bytes read + bytes written), 2 write only
    launch_bw_probe(mode, a, d, bytes, sink, c->stream);   // warm-up
    (void)hipEventRecord(e0, c->stream);
    for (int r = 0; r < reps; ++r) launch_bw_probe(mode, a, d, bytes, sink, c->stream);
    (void)hipEventRecord(e1, c->stream);
    e = hipEventSynchronize(e1);
    float ms = 0;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return done(fail(QM_E_HIP, "qm_bw_probe: %s", hipGetErrorString(e)));
    gbps3[mode] = (mode == 1 ? 2.0 : 1.0) * (double)bytes * reps / ((double)ms * 1e-3) / 1e9;
  }
  return done(QM_OK);
}

// ---------------------------------------------------------------------------
// FP overlap (A7)
// ---------------------------------------------------------------------------
extern "C" int qm_fp_overlap(qm_ctx* c, int n_sets, const int64_t* set_offsets, const int32_t* pos, const int32_t* ref,
                             const int32_t* alt, int64_t* regions) {
  if (!c || n_sets < 1 || n_sets > 5 || !set_offsets || !regions) return fail(QM_E_INVAL, "qm_fp_overlap: bad arguments");
  HIPCHK(hipSetDevice(c->dev));
  const int64_t n = set_offsets[n_sets] - set_offsets[0];
  const int nreg = 1 << n_sets;
  for (int i = 0; i < nreg; ++i) regions[i] = 0;
  if (n <= 0) return QM_OK;
  if (n > 0x7fffff00ll) return fail(QM_E_INVAL, "qm_fp_overlap: too many keys");
  std::vector<int32_t> set_of((size_t)n);
  for (int s = 0; s < n_sets; ++s)
    for (int64_t i = set_offsets[s]; i < set_offsets[s + 1]; ++i) set_of[(size_t)(i - set_offsets[0])] = s;
  const int64_t o = set_offsets[0];
  int32_t *dp = nullptr, *dr = nullptr, *da = nullptr, *ds = nullptr;
  uint32_t *k[2] = {nullptr, nullptr}, *v[2] = {nullptr, nullptr}, *hist = nullptr, *bad = nullptr;
  unsigned long long* dreg = nullptr;
  SortSeg* dseg = nullptr;
  int32_t* dts = nullptr;
  int rc = QM_OK;
  auto cleanup = [&]() {
    void* ps[] = {dp, dr, da, ds, k[0], k[1], v[0], v[1], hist, bad, dreg, dseg, dts};
    for (void* p : ps) (void)hipFree(p);
  };
#define A_(p, cnt) if (rc == QM_OK) rc = dalloc(&(p), (size_t)(cnt));
  A_(dp, n) A_(dr, n) A_(da, n) A_(ds, n) A_(k[0], n + 64) A_(k[1], n + 64) A_(v[0], n + 64) A_(v[1], n + 64)   /* the sort kernels read whole 16-byte pieces */
  A_(hist, (size_t)((n + SORT_TILE - 1) / SORT_TILE) * 256) A_(bad, 1) A_(dreg, nreg) A_(dseg, 1)
  A_(dts, (n + SORT_TILE - 1) / SORT_TILE)
#undef A_
  if (rc != QM_OK) { cleanup(); return rc; }
  hipStream_t st = c->stream;
  hipError_t e = hipMemcpy(dp, pos + o, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dr, ref + o, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(da, alt + o, (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ds, set_of.data(), (size_t)n * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 4, st);
  if (e == hipSuccess) e = hipMemsetAsync(dreg, 0, sizeof(unsigned long long) * (size_t)nreg, st);
  if (e != hipSuccess) { cleanup(); return fail(QM_E_HIP, "qm_fp_overlap: %s", hipGetErrorString(e)); }
  launch_overlap_pack(dp, dr, da, ds, n, k[0], v[0], bad, st);
  {
    SortSeg g;
    memset(&g, 0, sizeof g);
    g.n = n; g.ntiles = (int32_t)((n + SORT_TILE - 1) / SORT_TILE);
    std::vector<int32_t> ts((size_t)g.ntiles, 0);
    e = hipMemcpy(dseg, &g, sizeof g, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dts, ts.data(), 4 * ts.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { cleanup(); return fail(QM_E_HIP, "qm_fp_overlap: %s", hipGetErrorString(e)); }
  }
  int cur = 0;
  for (int shift = 0; shift < 32; shift += 8) {
    launch_sort_pass(dseg, dts, 1, (int)((n + SORT_TILE - 1) / SORT_TILE), k[cur], nullptr, v[cur], shift, hist, k[cur ^ 1], nullptr, v[cur ^ 1], 0, st);
    cur ^= 1;
  }
  launch_overlap_count(k[cur], v[cur], n, dreg, st);
  std::vector<unsigned long long> hreg((size_t)nreg);
  uint32_t hbad = 0;
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipMemcpy(hreg.data(), dreg, sizeof(unsigned long long) * (size_t)nreg, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&hbad, bad, 4, hipMemcpyDeviceToHost);
  cleanup();
  if (e != hipSuccess) return fail(QM_E_HIP, "qm_fp_overlap: %s", hipGetErrorString(e));
  if (hbad) return fail(QM_E_INVAL, "qm_fp_overlap: a key is not a single-base variant with 0 <= pos < 2^28");
  for (int i = 0; i < nreg; ++i) regions[i] = (int64_t)hreg[(size_t)i];
  return QM_OK;
}
