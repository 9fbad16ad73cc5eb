// qmvt_finish.cpp -- VCFs found out of order and qm_batch_finish: the routing, the chunk tables, the four chunk
// paths with their fallback, and the rescan behind them.  Part of libqmvt.so's host side (qmvt_batch.h).
#include "qmvt_batch.h"

// ---- VCFs found out of order: redone in chunks of <= 2^28 records, every step of a chunk one launch ----
constexpr int64_t SORT_CHUNK_RECORDS = 1ll << 28;
static int64_t sort_chunk_records() {   // QM_SORT_CHUNK_RECORDS (tests, tools/gpu_fuzz.py): small chunks, several of them per finish
  if (const char* e = getenv("QM_SORT_CHUNK_RECORDS")) { const long long v = atoll(e); if (v > 0) return std::min<int64_t>(v, SORT_CHUNK_RECORDS); }
  return SORT_CHUNK_RECORDS;
}

// --- which path a VCF takes.  Plain values in, no batch: the routing compiles on its own.
constexpr int N_PATHS = 5;
constexpr int PX_MAX_PARTS = 4;              // partitions of 2^27 keys a VCF of the partitions path may span
constexpr int PW_SHIFT = DJ_BIG_SHIFT + 8;   // 29: a partition of wide buckets
// The knobs of the routing, read from the environment ONCE per qm_batch_finish: route() runs once per VCF, and ten getenv calls per
// VCF were 22 us of a first-seen step's host time (256 VCFs) -- between the flags' arrival and the first launch, with the device waiting.
struct PathEnv {
  int forced = -1;                       // QM_UNSORTED_PATH (tests, fuzz): a Path every unsorted VCF it holds takes first, or -1
  bool join_hash = false;                // QM_JOIN=hash: the hashed bucket join; the paths that have only k_join_lean are off
  bool speculate = true;                 // QM_SPECULATE=0: every one-level chunk is looked at before its results are handed over
  int64_t bucket_min = HB_MIN_RECORDS;   // QM_BUCKET_MIN: tests and tools/gpu_fuzz.py send their small VCFs through the buckets too
};
// partitions of 2^pshift keys a VCF's position bits reach into (key = pos << 4 | nibble)
static int parts_of(uint32_t posor, int pshift = P2_SHIFT) { return (int)((((uint64_t)posor << 4) | 15u) >> pshift) + 1; }
// the one-level path's bucket shift: the top eight key bits in use are the bucket number
static int onelevel_shift(uint32_t posor) {
  const uint32_t kor = (posor << 4) | 15u;
  int msb = 31;
  while (msb > 0 && !((kor >> msb) & 1u)) --msb;
  return std::max(4, msb - 7);
}
// Capacity: what a path's tables and entries can hold at all.  One level: 256 buckets x 8 sub-regions x 1 024 entries at five eighths
// full, 21 index bits.  Two levels: 26 index bits (runs of 2^24).  Partitions: <= 4 of 2^27 keys, 21 (allele-extended: the second
// stream's entries) or 26 index bits.  Wide: <= 2 partitions of 2^29 keys.  The bucket joins of the last three are k_join_lean's.
static bool onelevel_holds(int64_t n, const PathEnv& env) {
  return n >= env.bucket_min && n <= (int64_t)HB_BUCKETS * HB_MAX_RECORDS * 5 / 8 && n <= ((int64_t)1 << HB_INDEX_BITS);
}
static bool wide_fits(bool ext, int64_t n, uint32_t posor, const PathEnv& env) {
  return !ext && !env.join_hash && n <= ((int64_t)1 << 26) && parts_of(posor, PW_SHIFT) <= 2;
}
static bool path_holds(Path p, bool ext, int64_t n, uint32_t posor, const PathEnv& env) {
  switch (p) {
    case Path::Radix: return true;
    case Path::OneLevel: return onelevel_holds(n, env);
    case Path::TwoLevel: return !ext && !env.join_hash && n > 0 && n <= ((int64_t)P2_MAX_HALVES << P2_INDEX_BITS);
    case Path::Partitions:
      return !env.join_hash && n >= HB_MIN_RECORDS && n <= ((int64_t)1 << (ext ? HB_INDEX_BITS : 26)) && parts_of(posor) <= PX_MAX_PARTS;
    case Path::Wide: return wide_fits(ext, n, posor, env) && n >= env.bucket_min;
  }
  return false;
}
// The path of one unsorted VCF of n records whose position bits are posor, against a truth set of truth_n keys.  The first row of
// DESIGN.md §4.4's table that takes it.
static Path route(bool ext, int64_t n, uint32_t posor, int64_t truth_n, const PathEnv& env) {
  if (env.forced >= 0 && path_holds((Path)env.forced, ext, n, posor, env)) return (Path)env.forced;
  const int parts = parts_of(posor);
  const int64_t kor = ((int64_t)posor << 4) | 15;
  // More records than the narrow buckets of its reference hold (8 192 per 2^15 positions, the sub-regions 13/16 full on average: 0.2
  // records per position) overflow the partitions and the two levels alike: such a VCF goes to the radix sort alone instead of taking
  // its chunk with it.  (The position bits are an upper bound of up to twice the highest position: this errs towards the buckets.)
  const bool dense = !ext && n > ((kor >> DJ_MAX_SHIFT) + 1) * (HB_MAX_RECORDS * 13 / 16);
  // row "allele-extended batches; default-mode VCFs on 8.4-16.8 M positions": partitions.  Default mode: a reference of 8.4 ... 16.8 M
  // positions is ONE pair of partitions = one pass of the 512-digit scatter and the bit-map join, where the one-level path would need
  // the hashed join and larger VCFs two levels (eight partitions per pass lost to the two levels by 2.6x: the pieces a tile leaves per
  // bucket fall below an L2 line, profiles/r06_pmc_scatter2048_not_kept.json).  Allele-extended: whatever the one-level path does not
  // take on a single partition.
  if (!dense && path_holds(Path::Partitions, ext, n, posor, env) && (ext ? parts > 1 || !onelevel_holds(n, env) : parts == 2)) return Path::Partitions;
  // row "default mode, 16.8-67 M positions": wide buckets, one pass of the 512-digit scatter over the columns where the two levels move
  // every record twice.  Not fuller than eight sub-regions of 4 096 take; a bucket stages 4 096 truth keys (three quarters of that on
  // average: the rest is room for an uneven truth set).
  if (wide_fits(ext, n, posor, env) && n >= HB_MIN_RECORDS && parts >= 3) {
    const int64_t buckets = (kor >> DJ_BIG_SHIFT) + 1;
    if (n <= buckets * (4 * HB_MAX_RECORDS * 13 / 16) && truth_n <= buckets * (4 * DJ_TRUTH_MAX * 3 / 4)) {
      // above the one-level path's 1.31 M records (50 Mb, 1.6e8 records per step: 2 M-record VCFs 4.3e10 /s against the two levels'
      // 2.8e10, 5 M 6.7e10 against 3.6e10)
      if (!onelevel_holds(n, env)) return Path::Wide;
      // below it, the one-level path's hashed join (7.5e10 /s where it fits, the wide buckets 3.9e10) -- unless the truth set is
      // too dense for the 1 024 truth keys it stages per bucket of 2^18+ positions (the chunk would overflow: radix sort, 1.3-1.7e10 /s;
      // wide buckets 2.7-3.4e10)
      if (truth_n > ((kor >> onelevel_shift(posor)) + 1) * (HB_TRUTH_SLOTS / 2 * 5 / 8)) return Path::Wide;
    }
  }
  // rows "16 384 ... 1.31 M records" (k_join_lean) and "wider references" (k_classify_hash): one level, a VCF's 256 workgroups
  // and rows whatever it holds (smaller VCFs are sorted in no time)
  if (path_holds(Path::OneLevel, ext, n, posor, env)) return Path::OneLevel;
  // row "1.31 M ... 67 M records on references beyond that": two levels
  if (!dense && n >= HB_MIN_RECORDS && path_holds(Path::TwoLevel, ext, n, posor, env)) return Path::TwoLevel;
  // last row: the radix sort
  return Path::Radix;
}

// What a path does with a chunk: how many VCFs it takes (rows of 1.5 KB and >= 1 MB of bucket regions per VCF; wide buckets 2 x 67 MB),
// whether a VCF weighs its records once per pass over its columns (partitions: a PAIR of them per pass), how often a chunk and the
// VCFs of it that fitted run before what is left without a result goes to the next path.
struct PathInfo { int max_vcfs; bool per_pass; int runs; Path next; };
static const PathInfo PATHS[N_PATHS] = {
    /* Radix      */ {INT32_MAX, false, 1, Path::Radix},
    /* OneLevel   */ {4096, false, INT32_MAX, Path::Radix},
    /* TwoLevel   */ {4096, false, 3, Path::Radix},   // (a partition too dense names one VCF at a time)
    /* Partitions */ {4096 / PX_MAX_PARTS, true, 2, Path::Radix},
    /* Wide       */ {64, false, 2, Path::TwoLevel},
};

static thread_local PathEnv g_penv;
static int read_path_env() {
  PathEnv e;
  if (const char* v = getenv("QM_UNSORTED_PATH")) {
    static const char* const names[N_PATHS] = {"radix", nullptr, "two_level", "partitions", "wide"};
    for (int p = 0; p < N_PATHS; ++p) if (names[p] && strcmp(v, names[p]) == 0) e.forced = p;
    if (e.forced < 0 && *v) return fail(QM_E_INVAL, "QM_UNSORTED_PATH=%s: radix, two_level, partitions or wide", v);
  }
  if (const char* v = getenv("QM_JOIN")) e.join_hash = strcmp(v, "hash") == 0;
  if (const char* v = getenv("QM_SPECULATE")) e.speculate = atoi(v) != 0;
  if (const char* v = getenv("QM_BUCKET_MIN")) e.bucket_min = atoll(v);
  g_penv = e;
  return QM_OK;
}

// --- the device arrays of a chunk

// the scratch batch of a radix chunk: the sorted copies of its VCFs and their rows; rebuilt only when the chunk's shape changes
static int ensure_sub(qm_batch* b, const std::vector<int>& vs) {
  const int nseg = (int)vs.size();
  std::vector<int64_t> sig((size_t)nseg);
  std::vector<int32_t> tids((size_t)nseg);
  for (int i = 0; i < nseg; ++i) { sig[(size_t)i] = b->L.vcfs[(size_t)vs[(size_t)i]].n; tids[(size_t)i] = b->L.vcfs[(size_t)vs[(size_t)i]].truth; }
  if (!b->sub || b->sub_sig != sig) {
    if (b->sub) { b->dev_bytes -= b->sub->dev_bytes; batch_free(b->sub); b->sub = nullptr; }
    int rc = batch_alloc(b->ctx, nseg, sig.data(), tids.data(), b->n_bins, &b->sub, true, b->ext);
    if (rc != QM_OK) return rc;
    b->sub->ext = b->ext;
    b->dev_bytes += b->sub->dev_bytes;
    b->sub_sig = sig;
    b->sub_tids = tids;
  } else if (b->sub_tids != tids) {
    b->sub_tids = tids;
    for (int i = 0; i < nseg; ++i) b->sub->L.vcfs[(size_t)i].truth = tids[(size_t)i];
    for (SpanDesc& sd : b->sub->L.spans) sd.truth = b->sub->L.vcfs[(size_t)sd.vcf].truth;
    int rc = upload_layout(b->sub);
    if (rc != QM_OK) return rc;
  }
  return QM_OK;
}

// behind a bucket chunk's cursors ([nseg][256][8], then one flag word per segment): 32 + 16 * 65 phase clocks of a profiling build, the
// scatter's per-segment histograms, seg_maxd, the chunk's "bad" word -- all of it cleared in front of the scatter
static int64_t cursor_words(int64_t nseg) { return nseg * HB_BUCKETS * HB_SUBS + nseg + 32 + 16 * 65 + nseg * (SEG_HIST_WORDS + 1) + 1; }
struct CursorRegion { uint32_t *seg_hist, *seg_maxd, *chunk_bad; uint32_t words; };
static CursorRegion cursor_region(const qm_batch* b, int nseg) {
  CursorRegion C;
  C.seg_hist = b->bk_cursor + (size_t)nseg * HB_BUCKETS * HB_SUBS + (size_t)nseg + 32 + 16 * 65;
  C.seg_maxd = C.seg_hist + (size_t)nseg * SEG_HIST_WORDS;
  C.chunk_bad = C.seg_maxd + nseg;
  C.words = (uint32_t)cursor_words(nseg);
  return C;
}

// The arrays every bucket path fills for nseg segments: bucket regions (xs: the second entry stream's too), cursors, row descriptors,
// the rows, the scatter's tile map, the row descriptors of k_finalize, and the rows (ROC, scalars, flags) of the VCFs before
// k_sort_copy_rows takes them home -- small arrays of their own, so that a bucket chunk needs no scratch batch
static int ensure_bucket_arrays(qm_batch* b, int64_t nseg, int64_t bk_ents, int64_t nbt, bool xs) {
  const int64_t rows = nseg * HB_BUCKETS, orows = nseg * (xs ? 2 * HB_BUCKETS : HB_BUCKETS);
  int64_t* by = &b->dev_bytes;
  int rc = b->bk_hist.grow(orows * SPAN_HIST_WORDS, by);
  if (rc == QM_OK) rc = b->bk_scal.grow(orows * 8, by);
  if (rc == QM_OK && xs) rc = b->bk_xent.grow(2 * bk_ents, by);
  if (rc == QM_OK && xs) rc = b->bk_xcursor.grow(rows * HB_SUBS, by);
  if (rc == QM_OK && xs) rc = b->bk_xrows.grow(rows, by);
  if (rc == QM_OK) rc = b->d_bk_vcfs.grow(nseg, by);
  if (rc == QM_OK) rc = b->bk_ent.grow(bk_ents, by);
  if (rc == QM_OK) rc = b->bk_rows.grow(rows, by);
  if (rc == QM_OK) rc = b->bk_cursor.grow(cursor_words(nseg), by);
  if (rc == QM_OK) rc = b->d_bk_tile_seg.grow(nbt, by);
  if (rc == QM_OK) rc = b->bk_roc.grow(nseg * 3 * b->n_bins, by);
  if (rc == QM_OK) rc = b->bk_rscal.grow(nseg * 8, by);
  if (rc == QM_OK) rc = b->bk_vflags.grow(nseg, by);
  return rc;
}

// --- the tables of a chunk on the device.  d_segs, the tile maps, d_bk_vcfs, d_vsegs, d_vparts and the two levels' p_* hold ONE chunk's
// tables at a time: b->tables says which path built them for which VCFs, and what else they follow from.  A path rebuilds them when
// its chunk's record differs -- a batch run again with the same VCFs out of order uploads nothing.
static bool owns(const qm_batch* b, Path path, const std::vector<int>& vs, const std::vector<uint32_t>& key) {
  return b->tables.path == path && b->tables.vcfs == vs && b->tables.key == key;
}
static std::vector<uint32_t> posor_of(const std::vector<int>& vs, const std::vector<uint32_t>& posor) {
  std::vector<uint32_t> k(vs.size());
  for (size_t i = 0; i < vs.size(); ++i) k[i] = posor[(size_t)vs[i]];
  return k;
}

// One chunk's tables on the host, built by its path segment by segment (add_bucket_seg, add_vcf_row, ktile_maps) and put on the device
// in one go (upload_tables).
struct ChunkTables {
  bool maps = true;                              // false: the tables are on the device already, only the geometry is wanted -- no per-tile entries
  std::vector<SortSeg> segs, vsegs;              // the segments; where a VCF has several, one row per VCF for the hand-over
  std::vector<int32_t> vparts;                   // segments per VCF (beside vsegs)
  std::vector<VcfDesc> fake;                     // the rows of a segment's buckets as the "spans" of a VCF, for k_finalize
  std::vector<int32_t> tile_seg, bk_tile_seg;    // the segment of every sort tile (radix) / scatter tile (buckets)
  std::vector<int32_t> ktile_seg, ktile_local;   // k_tile_counts' map: the VCF (index into the chunk) and the tile inside it of every K1 tile
  std::vector<int> seg_vcf;                      // the VCF of every segment
  int64_t bk_ents = 0, nbt = 0, nst = 0, nkt = 0, koff = 0, hoff = 0;   // bucket entries, scatter / sort / K1 tiles, keys, histogram words so far
};
// Entries per sub-region of a segment of n records: between 128 and 256 buckets are in use, a sub-region takes every eighth tile; half
// as much again on top, a power of two up to sub_max
static int64_t sub_cap(int64_t n, int64_t sub_max) {
  const int64_t want = n / (128 * HB_SUBS) * 3 / 2 + 16;
  int64_t cap = 16;
  while (cap < want && cap < sub_max) cap *= 2;
  return cap;
}
// One more segment of the bucket scatter.  g: who it is (records, VCF, shift, buckets, key range); tiles: the scatter tiles it owns.
// Its regions, its place in the tile map, its `rows` bucket rows as the "spans" of a VCF of `truth` for k_finalize (the rows of a
// segment lie 256 apart; xs, two entry streams: 512).
static void add_bucket_seg(ChunkTables* T, SortSeg g, int64_t tiles, int64_t sub_max, int32_t truth, bool xs, int rows) {
  const int32_t i = (int32_t)T->segs.size();
  g.bk_cap = (int32_t)sub_cap(g.n, sub_max); g.bk_off = T->bk_ents; g.bk_tile0 = (int32_t)T->nbt;
  T->bk_ents += (int64_t)HB_BUCKETS * HB_SUBS * g.bk_cap;
  T->nbt += tiles;
  if (T->maps) T->bk_tile_seg.insert(T->bk_tile_seg.end(), (size_t)tiles, i);
  VcfDesc f = VcfDesc();
  f.off = 0; f.n = g.n; f.truth = truth; f.tile0 = 0; f.ntiles = 0; f.span0 = i * (xs ? 2 * HB_BUCKETS : HB_BUCKETS); f.nspans = rows; f.pad = 0;
  T->fake.push_back(f);
  T->seg_vcf.push_back(g.main_vcf);
  T->segs.push_back(g);
}
// the row of VCF v (descriptor d) whose segments begin at seg0 and end here: what hand_over adds up per VCF
static void add_vcf_row(ChunkTables* T, const VcfDesc& d, int v, int seg0) {
  SortSeg vg;
  memset(&vg, 0, sizeof vg);
  vg.src_off = d.off; vg.n = d.n; vg.main_vcf = v; vg.sub_vcf = seg0; vg.main_tile0 = d.tile0;
  T->vsegs.push_back(vg);
  T->vparts.push_back((int32_t)T->segs.size() - seg0);
}
static void ktile_maps(const qm_batch* b, const std::vector<int>& vs, ChunkTables* T) {
  for (size_t i = 0; i < vs.size(); ++i) {
    const int nt = b->L.vcfs[(size_t)vs[i]].ntiles;
    T->nkt += nt;
    if (T->maps) for (int t = 0; t < nt; ++t) { T->ktile_seg.push_back((int32_t)i); T->ktile_local.push_back(t); }
  }
}

// One segment per VCF (the radix sort, the one-level buckets): where its records are, its sort tiles, its digit histograms, its buckets
static void vcf_segs(const qm_batch* b, const std::vector<int>& vs, const std::vector<uint32_t>& posor, ChunkTables* T) {
  const bool xs = b->ext;
  int64_t dst_off = 0;
  for (size_t i = 0; i < vs.size(); ++i) {
    const VcfDesc& d = b->L.vcfs[(size_t)vs[i]];
    SortSeg g;
    memset(&g, 0, sizeof g);
    g.src_off = d.off; g.dst_off = dst_off; g.koff = T->koff; g.hoff = T->hoff; g.n = d.n;   // dst_off: as build_layout lays the scratch batch out
    dst_off += (d.n + VCF_ALIGN - 1) / VCF_ALIGN * VCF_ALIGN;
    g.tile0 = (int32_t)T->nst; g.ntiles = (int32_t)((d.n + SORT_TILE - 1) / SORT_TILE);
    g.main_vcf = vs[i]; g.sub_vcf = (int32_t)i; g.main_tile0 = d.tile0;
    g.pad = onelevel_shift(posor[(size_t)vs[i]]);
    // buckets above the VCF's highest position are empty by construction: <= 256
    g.nbk = std::min((int)(((posor[(size_t)vs[i]] << 4) | 15u) >> g.pad) + 1, (int)HB_BUCKETS); g.key_base = 0u;
    if (T->maps) T->tile_seg.insert(T->tile_seg.end(), (size_t)g.ntiles, (int32_t)i);
    T->nst += g.ntiles;
    T->koff += (d.n + 63) / 64 * 64;
    T->hoff += (int64_t)g.ntiles * 256;
    add_bucket_seg(T, g, (d.n + BK_TILE - 1) / BK_TILE, HB_SUB_MAX, d.truth, xs, xs ? 2 * HB_BUCKETS : g.nbk);
  }
  ktile_maps(b, vs, T);
}

// A chunk's tables onto the device: the arrays grown to hold them (bucket paths: the chunk's regions, cursors and rows with them), the
// copies, one wait -- the host tables may go when this returns -- and the record of what the shared arrays hold now.  key: what the
// tables follow from besides the chunk's VCFs.
static int upload_tables(qm_batch* b, Path path, const std::vector<int>& vs, const std::vector<uint32_t>& key, const ChunkTables& T, hipStream_t st) {
  b->tables = qm_batch::Tables();
  const bool radix = path == Path::Radix;
  if (T.nst > INT32_MAX || T.nkt > INT32_MAX || T.nbt > INT32_MAX)
    return fail(QM_E_LIMIT, "%s: too many tiles", path == Path::Radix || path == Path::OneLevel ? "sort chunk" : "bucket path");
  const int64_t nseg = (int64_t)T.segs.size(), nv = (int64_t)T.vsegs.size();
  int64_t* by = &b->dev_bytes;
  int rc = b->d_segs.grow(nseg, by);
  if (rc == QM_OK) rc = b->d_ktile_seg.grow(T.nkt, by);
  if (rc == QM_OK) rc = b->d_ktile_local.grow(T.nkt, by);
  if (rc == QM_OK && radix) rc = b->d_tile_seg.grow(T.nst, by);
  if (rc == QM_OK && nv) rc = b->d_vsegs.grow(nv, by);
  if (rc == QM_OK && nv) rc = b->d_vparts.grow(nv, by);
  if (rc == QM_OK && !radix) rc = ensure_bucket_arrays(b, nseg, T.bk_ents, T.nbt, b->ext);
  if (rc != QM_OK) return rc;
  auto put = [st](void* dst, const auto& v) {
    return v.empty() ? hipSuccess : hipMemcpyAsync(dst, v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice, st);
  };
  HIPCHK(put(b->d_segs, T.segs));
  HIPCHK(put(b->d_vsegs, T.vsegs));
  HIPCHK(radix ? put(b->d_tile_seg, T.tile_seg) : put(b->d_bk_tile_seg, T.bk_tile_seg));
  HIPCHK(put(b->d_ktile_seg, T.ktile_seg));
  HIPCHK(put(b->d_ktile_local, T.ktile_local));
  if (!radix) HIPCHK(put(b->d_bk_vcfs, T.fake));
  HIPCHK(put(b->d_vparts, T.vparts));
  HIPCHK(hipStreamSynchronize(st));
  b->tables = qm_batch::Tables{path, vs, key, (int)nseg, T.nbt, T.nkt, T.seg_vcf};
  return QM_OK;
}

// --- what the bucket paths share

// The launch parameters of every bucket path, for the segment table in d_segs: cursors, entries, rows.  What differs is set by the
// path itself: l1_ent / l1_half (two levels), pairs (partitions), seg_maxd (one level), H.zero.
static void bucket_params(qm_batch* b, int nseg, bool xs, uint32_t* seg_hist, BucketScatterParams* S, HashParams* H) {
  S->segs = b->d_segs; S->tile_seg = b->d_bk_tile_seg; S->pos = b->pos; S->ref = b->ref; S->alt = b->alt; S->qual = b->qual; S->flags = b->flags; S->anib = b->anib;
  S->cursor = b->bk_cursor; S->ent = b->bk_ent; S->mask_pass = reinterpret_cast<uint32_t*>(b->mask_pass.p); S->mask_tp = reinterpret_cast<uint32_t*>(b->mask_tp.p);
  S->n_seg = nseg; S->n_bins = b->n_bins; S->tile_base = 0;
  S->xent = xs ? b->bk_xent.p : nullptr; S->xcursor = xs ? b->bk_xcursor.p : nullptr; S->ext = xs ? 1 : 0;
  S->seg_hist = seg_hist;   // k_join_lean follows: the scatter counts every record by bin
  S->l1_ent = nullptr; S->l1_half = nullptr; S->pairs = 0; S->seg_maxd = nullptr;
  H->segs = b->d_segs; H->rows = b->bk_rows; H->rows_out = b->bk_rows; H->ent = b->bk_ent; H->cursor = b->bk_cursor; H->truths = b->ctx->d_truths; H->vcfs = b->d_vcfs;
  H->mask_tp = b->mask_tp; H->row_hist = b->bk_hist; H->row_scal = b->bk_scal; H->n_seg = nseg; H->n_bins = b->n_bins; H->seg_base = 0;
  H->xrows = xs ? b->bk_xrows.p : nullptr; H->xent = xs ? b->bk_xent.p : nullptr; H->xcursor = xs ? b->bk_xcursor.p : nullptr;
  H->out_stride = xs ? 2 * HB_BUCKETS : HB_BUCKETS; H->ext = xs ? 1 : 0;
  H->scatter_hist = seg_hist ? 1 : 0;
  H->seg_maxd = nullptr;
  H->zero = nullptr; H->n_zero = 0u;
}
static FinalizeParams bucket_rows_finalize(qm_batch* b, const uint32_t* all_hist) {
  FinalizeParams F = finalize_params(b, nullptr);   // the rows join the per-truth sums only once no bucket is known to have overflowed
  F.all_hist = all_hist;
  F.vcfs = b->d_bk_vcfs; F.span_hist = b->bk_hist; F.span_scal = b->bk_scal; F.vcf_posor = nullptr;
  F.roc = b->bk_roc; F.scalars = b->bk_rscal; F.vcf_flags = b->bk_vflags;
  F.vcf_tot = nullptr;   // (these "VCFs" are rows of buckets: no tiles, no lists -- and not the main batch's numbering)
  return F;
}

// what the flag word of VCF v says went wrong with it: a position out of range, the de-duplication limit; QM_OK for neither
static int flag_failure(uint32_t fl, int v) {
  if (fl & SPANF_BADPOS) return fail(QM_E_RANGE, "VCF %d holds a position outside [0, 2^28)", v);
  if (fl & SPANF_RUNLIMIT)
    return fail(QM_E_LIMIT, "VCF %d repeats one position more than %d times between equal alleles (allele-extended de-duplication limit)", v, 1 << 14);
  return QM_OK;
}

// The verdict on a bucket chunk whose rows' flags are on the host: per segment its flag word and (maxd, or null) the highest bucket its
// records reached, against the nbk launched.  A bad position fails the finish; *named gets the VCFs with an overflowing bucket (a VCF's
// segments lie one behind the other) -- nothing of such a chunk may be handed over.
static int bucket_verdict(qm_batch* b, const uint32_t* fl, const uint32_t* maxd, uint32_t nbk, const std::vector<int>& seg_vcf, std::vector<int>* named) {
  named->clear();
  for (size_t i = 0; i < seg_vcf.size(); ++i) {
    const int v = seg_vcf[i];
    const int rc = flag_failure(fl[i] & SPANF_BADPOS, v);
    if (rc != QM_OK) return rc;
    // (maxd above nbk: a remembered bound that no longer holds -- cannot happen while the columns stay the same)
    const bool over = (fl[i] & SPANF_OVERFLOW) || (maxd && maxd[i] > nbk);
    if (over && (named->empty() || named->back() != v)) named->push_back(v);
  }
  if (!named->empty()) b->path_stats[QM_PATH_OVERFLOW_CHUNKS] += 1;
  return QM_OK;
}

// A bucket chunk's results home: its rows under the original VCFs and into the per-truth sums (k_sort_copy_rows; nparts: segments per
// VCF to add up, or null), the tile counts from its masks.  segs: one per VCF.  gate (a speculative chunk): the chunk's "bad" word --
// k_sort_copy_rows leaves everything alone if it says the chunk overflowed; such a chunk is counted when it is settled (stat < 0).
static int hand_over(qm_batch* b, const SortSeg* segs, int nv, const int32_t* nparts, int64_t nkt, const uint32_t* gate, int stat, hipStream_t st) {
  launch_sort_copy_rows(segs, nv, b->bk_roc, b->bk_rscal, b->roc, b->scalars, b->n_bins, st, b->last_global, b->d_vcfs, nparts, gate);
  launch_tile_counts(segs, b->d_ktile_seg, b->d_ktile_local, (int)nkt, b->mask_pass, b->mask_tp, b->tile_tp, b->tile_fp, st);
  HIPCHK(hipGetLastError());
  if (stat >= 0) b->path_stats[stat] += nv;
  return QM_OK;   // no wait: the rescan that follows is on the same stream and ends with one
}

// QM_FINISH_TRACE: the host's clock (us), and its readings inside the latest chunk (entered, tables ready, scatter queued)
static double ftrace_now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec * 1e6 + t.tv_nsec * 1e-3; }
static thread_local double g_ftrace[4];

// --- the radix sort: stable LSD passes by position over the digits in use, k_classify<PACKED> on the sorted copies, results home.
// stat: the counter its VCFs go to (QM_PATH_RADIX, or QM_PATH_RADIX_AFTER_OVERFLOW behind a bucket path).
static int radix_chunk(qm_batch* b, const std::vector<int>& vs, hipStream_t st, const std::vector<uint32_t>& posor, int stat) {
  g_ftrace[0] = ftrace_now();
  const int nseg = (int)vs.size();
  int rc = ensure_sub(b, vs);
  if (rc != QM_OK) return rc;
  const std::vector<uint32_t> key = posor_of(vs, posor);
  ChunkTables T;
  T.maps = !owns(b, Path::Radix, vs, key);
  vcf_segs(b, vs, posor, &T);
  if (T.maps) rc = upload_tables(b, Path::Radix, vs, key, T, st);
  if (rc != QM_OK) return rc;
  const int nst = (int)T.nst, nkt = (int)T.nkt;
  b->path_stats[stat] += nseg;
  b->path_stats[QM_PATH_RADIX_CHUNKS] += 1;
  qm_batch* s = b->sub;
  // --- 1. + 2. stable LSD radix sort by position (key bits 4..31), only the digits in use.  The first pass packs the
  //        records to (key, info, original index) on the fly; the last pass drops keys and infos straight into the
  //        scratch batch.  (Its ping-pong arrays exist only once a chunk has come this way.)
  for (int i = 0; i < 2 && rc == QM_OK; ++i) {
    rc = b->sk[i].grow(T.koff, &b->dev_bytes);
    if (rc == QM_OK) rc = b->sv[i].grow(T.koff, &b->dev_bytes);
    if (rc == QM_OK) rc = b->si[i].grow(T.koff, &b->dev_bytes);
  }
  if (rc == QM_OK) rc = b->shist.grow(T.hoff, &b->dev_bytes);
  if (rc == QM_OK) rc = b->sorbits.grow(1, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  HIPCHK(hipMemsetAsync(b->sorbits, 0, 4, st));
  launch_sort_first_hist(b->d_segs, b->d_tile_seg, nst, b->pos, b->shist, b->sorbits, st);
  uint32_t orbits = 0;
  HIPCHK(hipMemcpyAsync(&orbits, b->sorbits, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (memo_on()) {   // every position bit in use in this chunk: corrects an under-estimate the VCFs were (or will be) remembered with
    if (b->posor_seen.empty()) b->posor_seen.assign((size_t)b->n_vcf, 0u);
    for (int v : vs) {
      b->posor_seen[(size_t)v] |= orbits >> 4;
      if (!b->known_posor.empty() && b->known[(size_t)v]) b->known_posor[(size_t)v] |= orbits >> 4;
    }
  }
  int npass = 1;
  while (4 + 8 * npass < 32 && (orbits >> (4 + 8 * npass)) != 0) ++npass;
  int cur = 0;
  const SortCols src = {b->pos, b->ref, b->alt, b->qual, b->flags, b->anib};
  {
    const bool last = npass == 1;
    launch_sort_first_scatter(b->d_segs, b->d_tile_seg, nseg, nst, src, b->n_bins, b->ext ? 1 : 0, b->shist, last ? s->pkey : b->sk[0],
                              last ? s->pinf : b->si[0], b->sv[0], last ? 1 : 0, b->mask_pass, b->mask_tp, st);
  }
  for (int ps = 1; ps < npass; ++ps) {
    const bool last = ps == npass - 1;
    launch_sort_pass(b->d_segs, b->d_tile_seg, nseg, nst, b->sk[cur], b->si[cur], b->sv[cur], 4 + 8 * ps, b->shist,
                     last ? s->pkey : b->sk[cur ^ 1], last ? s->pinf : b->si[cur ^ 1], b->sv[cur ^ 1], last ? 1 : 0, st);
    cur ^= 1;
  }
  const uint32_t* perm = b->sv[cur];
  if (b->ext) launch_sort_gather_alleles(b->d_segs, b->d_tile_seg, nst, perm, b->ref, b->alt, s->ref, s->alt, st);
  // --- 3. the normal path on the sorted copies (their ROC rows go into the caller's per-truth sums)
  launch_classify_any(classify_params(s), (int)s->L.spans.size(), st);
  launch_finalize(finalize_params(s, b->last_global), nseg, st);
  // --- 4. results back under the original VCFs: ROC + scalar rows, class bits in input order
  launch_sort_copy_rows(b->d_segs, nseg, s->roc, s->scalars, b->roc, b->scalars, b->n_bins, st);
  launch_sort_scatter_tp(b->d_segs, b->d_tile_seg, nst, s->mask_tp, perm, b->mask_tp, st);
  launch_tile_counts(b->d_segs, b->d_ktile_seg, b->d_ktile_local, nkt, b->mask_pass, b->mask_tp, b->tile_tp, b->tile_fp, st);
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> sfl((size_t)nseg);
  HIPCHK(hipMemcpyAsync(sfl.data(), s->vcf_flags, 4 * sfl.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int i = 0; i < nseg; ++i) {
    if (sfl[(size_t)i] & SPANF_UNSORTED) return fail(QM_E_HIP, "internal: VCF %d still unsorted after the radix sort", vs[(size_t)i]);
    // the optimistic pass stops streaming at the first out-of-order tile: a bad position behind it shows up only here
    rc = flag_failure(sfl[(size_t)i], vs[(size_t)i]);
    if (rc != QM_OK) return rc;
  }
  return QM_OK;
}

// --- one level: ONE scatter of each VCF's records on its top eight key bits into fixed-size bucket regions, the join per bucket.
// *named: the VCFs whose buckets overflowed (nothing of the chunk was handed over); empty when the chunk is done -- or queued
// (may_speculate: its results are handed over without a look at its flags, settle_pending looks at them behind the finish's last wait).
static int onelevel_chunk(qm_batch* b, const std::vector<int>& vs, hipStream_t st, const std::vector<uint32_t>& posor, bool may_speculate,
                          std::vector<int>* named) {
  named->clear();
  g_ftrace[0] = ftrace_now();
  const int nseg = (int)vs.size();
  const std::vector<uint32_t> key = posor_of(vs, posor);
  ChunkTables T;
  T.maps = !owns(b, Path::OneLevel, vs, key);
  vcf_segs(b, vs, posor, &T);
  const std::vector<SortSeg>& segs = T.segs;
  int lb_all = 0, nbk_all = 1;
  for (const SortSeg& g : segs) { lb_all = std::max(lb_all, (int)g.pad); nbk_all = std::max(nbk_all, (int)g.nbk); }
  // the join: one bit per key of the bucket in LDS where a bucket's key range allows it (k_join_lean: two bits per position), the hashed
  // tables of k_classify_hash otherwise (QM_JOIN=hash: always)
  const bool direct = lb_all <= DJ_MAX_SHIFT && !g_penv.join_hash;
  // allele-extended batches: two entry streams and two joins per bucket (k_join_lean for the single-base records, k_join_ext for the
  // others), both of which need the bucket's key range to fit the bit maps; wider key ranges take the radix sort
  const bool xs = b->ext;
  if (xs && !direct) return radix_chunk(b, vs, st, posor, QM_PATH_RADIX);
  if (xs) nbk_all = HB_BUCKETS;   // every row of a segment is written (the rows of the second stream follow at a fixed distance)
  int rc = T.maps ? upload_tables(b, Path::OneLevel, vs, key, T, st) : QM_OK;
  if (rc != QM_OK) return rc;
  const int nbt = (int)T.nbt, nkt = (int)T.nkt;
  const CursorRegion C = cursor_region(b, nseg);
  BucketScatterParams S;
  HashParams H;
  bucket_params(b, nseg, xs, direct ? C.seg_hist : nullptr, &S, &H);
  S.seg_maxd = C.seg_maxd;
  if (xs) HIPCHK(hipMemsetAsync(b->bk_xcursor, 0, (size_t)nseg * HB_BUCKETS * HB_SUBS * 4, st));
  H.zero = b->bk_cursor; H.n_zero = C.words;   // the scatter's cursors, flags, counts: cleared by the kernel that writes the rows
  g_ftrace[1] = ftrace_now();
  launch_bucket_rows(H, nseg, st);
  H.zero = nullptr; H.n_zero = 0u;
  // k_classify_hash issues instructions where the scatter waits for memory: a few segment ranges, the join of one on the second
  // stream beside the scatter of the next, fill each other's gaps (- 7 %).  The bit-map join was bound by the latency of a
  // workgroup's serial steps and wants every LDS slot of the chip: beside a scatter it only loses (3.06 ms in one piece
  // against 3.11 - 3.22 in 2 - 8 ranges, same box)
  int nbk_launch = nbk_all;
  const int parts = nseg >= 8 && !direct ? qm_batch::JOIN_PARTS : 1;
  // The buckets above a VCF's highest position hold nothing, and a workgroup that finds its bucket empty has still held a slot of its
  // CU for a memory round trip: 40 % of the grid on a 5 Mb genome, whose position BITS (all the optimistic pass hands over) bound the
  // buckets in use only by 256 -- 0.09 of the step's 2.65 ms (same box).  The scatter notes the highest bucket it filled per segment
  // (seg_maxd): the join's workgroups above it leave at once and k_finalize sums no row of theirs -- no round trip through the host.
  const bool tight_nbk = direct && parts == 1;
  if (tight_nbk) H.seg_maxd = C.seg_maxd;
  hipStream_t aux = parts > 1 ? b->ctx->aux : st;
  int i0 = 0;
  for (int p = 0; p < parts; ++p) {
    // ranges of about equal record counts
    int i1 = p + 1 == parts ? nseg : i0;
    if (p + 1 < parts) {
      const int64_t want = (int64_t)nbt * (p + 1) / parts;
      while (i1 < nseg && segs[(size_t)i1].bk_tile0 < want) ++i1;
      i1 = std::max(i1, i0);
    }
    if (i1 > i0) {
      const int t0 = segs[(size_t)i0].bk_tile0, t1 = i1 < nseg ? segs[(size_t)i1].bk_tile0 : nbt;
      S.tile_base = t0;
      launch_bucket_scatter(S, t1 - t0, st);
      g_ftrace[2] = ftrace_now();
      if (parts > 1) {
        HIPCHK(hipEventRecord(b->ev_sync[p], st));
        HIPCHK(hipStreamWaitEvent(aux, b->ev_sync[p], 0));
      }
      H.seg_base = i0;
      if (tight_nbk) {   // a batch that ran before remembers the highest bucket of every VCF: nothing is launched above
        bool have = memo_on() && !b->known_nbk.empty();
        uint32_t m = 0;
        if (have) for (int i = 0; i < nseg && have; ++i) { const uint32_t k = b->known_nbk[(size_t)vs[(size_t)i]]; have = k != 0u; m = std::max(m, k); }
        if (have && !xs) nbk_launch = (int)std::min<uint32_t>(std::max(m, 1u), (uint32_t)nbk_all);   // (two streams: every bucket is launched, the rows of the second follow at a fixed distance)
      }
      if (direct) launch_join_lean(H, i1 - i0, lb_all, nbk_launch, aux);
      else launch_classify_hash(H, i1 - i0, aux);
      if (xs) launch_join_ext(H, i1 - i0, nbk_all, aux);
    }
    i0 = i1;
  }
  if (parts > 1) {
    HIPCHK(hipEventRecord(b->ev_join, aux));
    HIPCHK(hipStreamWaitEvent(st, b->ev_join, 0));
  }
  const bool mirrors = b->d_summary != nullptr && nseg <= b->n_vcf;   // (one segment per VCF on this path)
  // No round trip through the host between the rows' k_finalize and the kernels that hand the chunk's results over: they are queued
  // at once, k_sort_copy_rows looks at the chunk's "bad" word on the device, and qm_batch_finish reads the mirrors behind its last
  // wait (settle_pending) -- 15-25 us per chunk of 2.5 ms.  Every chunk of a finish has mirror words of its own (b->pend_segs).
  const bool speculate = may_speculate && mirrors && b->pend_segs + nseg <= b->n_vcf && g_penv.speculate;
  const int moff = speculate ? b->pend_segs : 0;
  {
    FinalizeParams F = bucket_rows_finalize(b, S.seg_hist);
    if (tight_nbk) F.row_cap = C.seg_maxd;   // (the rows above were not written by this run)
    if (mirrors) { F.host_flags = b->d_summary + 16 + 2 * b->n_vcf + moff; F.host_aux = b->d_summary + 16 + 3 * b->n_vcf + moff; }   // (a place of their own: the run's flags may still be unread)
    if (speculate) { F.chunk_bad = C.chunk_bad; F.row_cap_limit = (uint32_t)nbk_launch; }
    launch_finalize(F, nseg, st);
  }
  b->path_stats[QM_PATH_BUCKET_CHUNKS] += 1;
  if (speculate) {
    rc = hand_over(b, b->d_segs, nseg, nullptr, nkt, C.chunk_bad, -1, st);
    if (rc != QM_OK) return rc;
    b->pend.push_back(qm_batch::Pending{vs, moff, nbk_launch, tight_nbk, direct});
    b->pend_segs += nseg;
    return QM_OK;
  }
  HIPCHK(hipGetLastError());
  std::vector<uint32_t> hfl((size_t)nseg), hmd((size_t)nseg, 0u);
  if (!mirrors) {
    HIPCHK(hipMemcpyAsync(hfl.data(), b->bk_vflags, 4 * hfl.size(), hipMemcpyDeviceToHost, st));
    if (tight_nbk) HIPCHK(hipMemcpyAsync(hmd.data(), C.seg_maxd, 4 * hmd.size(), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  if (mirrors) {   // k_finalize's host-mapped mirrors: the flags and (row_cap) the highest buckets, no copy
    memcpy(hfl.data(), b->h_summary + 16 + 2 * b->n_vcf, 4 * hfl.size());
    if (tight_nbk) memcpy(hmd.data(), b->h_summary + 16 + 3 * b->n_vcf, 4 * hmd.size());
  }
  if (tight_nbk && memo_on()) {
    if (b->known_nbk.empty()) b->known_nbk.assign((size_t)b->n_vcf, 0u);
    for (int i = 0; i < nseg; ++i) b->known_nbk[(size_t)vs[(size_t)i]] = std::max(hmd[(size_t)i], 1u);
  }
  rc = bucket_verdict(b, hfl.data(), tight_nbk ? hmd.data() : nullptr, (uint32_t)nbk_launch, vs, named);
  if (rc != QM_OK || !named->empty()) return rc;
  return hand_over(b, b->d_segs, nseg, nullptr, nkt, nullptr, direct ? QM_PATH_DIRECT : QM_PATH_HASHED, st);
}

// The flags of a bucket chunk with one segment per (VCF, partition), copied back; the verdict; the hand-over of a chunk that fitted
static int look_and_hand_over(qm_batch* b, int nv, int stat, hipStream_t st, std::vector<int>* named) {
  HIPCHK(hipGetLastError());
  const int nseg = b->tables.nseg;
  std::vector<uint32_t> hfl((size_t)nseg);
  HIPCHK(hipMemcpyAsync(hfl.data(), b->bk_vflags, 4 * hfl.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const int rc = bucket_verdict(b, hfl.data(), nullptr, 0u, b->tables.seg_vcf, named);
  if (rc != QM_OK || !named->empty()) return rc;
  return hand_over(b, b->d_vsegs, nv, b->d_vparts, b->tables.nkt, nullptr, stat, st);
}

// --- two levels (qmvt_dev.h): VCFs too large for 256 buckets of 8 192 records.  k_part_hist + k_part_scatter deal the records to
// partitions of 2^27 keys in exactly sized regions; every (VCF, partition in use) is then a segment of the one-level scatter, read from
// those entries.  *named: a VCF with a partition too dense for its buckets (named before anything is scattered), or the VCFs whose
// buckets overflowed.
static int two_level_chunk(qm_batch* b, const std::vector<int>& vs, hipStream_t st, std::vector<int>* named) {
  named->clear();
  const int nv = (int)vs.size();
  // --- level 1: descriptors, tile map, counting pass.  A level-1 entry has 24 index bits: a VCF above 2^24 records is dealt out in
  //     HALVES -- runs of 2^24 records, each a level-1 segment of its own (own counts, own regions, indices relative to its first
  //     record) -- whose regions lie one behind the other inside every partition of the VCF, so that a partition still is ONE run of
  //     entries for the second level, which adds the half's base back (BucketScatterParams.l1_half).
  constexpr int64_t HALF = (int64_t)1 << P2_INDEX_BITS;
  std::vector<PartSeg> ps;
  std::vector<int> half_vcf, vcf_half0((size_t)nv + 1, 0);   // VCF (index into vs) of every half; first half of every VCF
  std::vector<int32_t> ptile;
  int64_t ent_total = 0, nt1 = 0;
  const bool same_vs = b->tables.path == Path::TwoLevel && b->tables.vcfs == vs;   // the level-1 tables depend on the chunk's VCFs only
  bool any_halves = false;
  for (int i = 0; i < nv; ++i) {
    const VcfDesc& d = b->L.vcfs[(size_t)vs[(size_t)i]];
    vcf_half0[(size_t)i] = (int)ps.size();
    const int nh = (int)std::max<int64_t>(1, (d.n + HALF - 1) / HALF);
    any_halves = any_halves || nh > 1;
    for (int h = 0; h < nh; ++h) {
      PartSeg g;
      g.src_off = d.off + (int64_t)h * HALF; g.n = std::min<int64_t>(HALF, d.n - (int64_t)h * HALF); g.ent_off = ent_total; g.tile0 = (int32_t)nt1; g.main_vcf = vs[(size_t)i];
      const int64_t t = (g.n + BK_TILE - 1) / BK_TILE;
      if (!same_vs) ptile.insert(ptile.end(), (size_t)t, (int32_t)ps.size());
      nt1 += t;
      ps.push_back(g);
      half_vcf.push_back(i);
    }
    ent_total += d.n + 2 * P2_PARTS;   // every partition starts on a 16-byte boundary: at most one entry of padding each
  }
  vcf_half0[(size_t)nv] = (int)ps.size();
  const int nh_all = (int)ps.size();
  if (nt1 > INT32_MAX) return fail(QM_E_LIMIT, "bucket path: too many tiles");
  constexpr int NC = P2_PARTS * P2_SUBS;
  int64_t* by = &b->dev_bytes;
  int rc = b->p_segs.grow((int64_t)nh_all, by);
  if (rc == QM_OK) rc = b->p_tile_seg.grow(nt1, by);
  if (rc == QM_OK) rc = b->p_cnt.grow((int64_t)nh_all * NC, by);
  if (rc == QM_OK) rc = b->p_off.grow((int64_t)nh_all * (NC + 1), by);
  if (rc == QM_OK) rc = b->p_cursor.grow((int64_t)nh_all * NC, by);
  if (rc == QM_OK) rc = b->p_flags.grow((int64_t)nh_all, by);
  if (rc == QM_OK) rc = b->p_ent.grow(ent_total + 64, by);
  if (rc != QM_OK) return rc;
  if (!same_vs) {
    HIPCHK(hipMemcpyAsync(b->p_segs, ps.data(), sizeof(PartSeg) * ps.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->p_tile_seg, ptile.data(), 4 * ptile.size(), hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemsetAsync(b->p_cnt, 0, (size_t)nh_all * NC * 4, st));
  HIPCHK(hipMemsetAsync(b->p_cursor, 0, (size_t)nh_all * NC * 4, st));
  HIPCHK(hipMemsetAsync(b->p_flags, 0, (size_t)nh_all * 4, st));
  PartParams PP;
  PP.segs = b->p_segs; PP.tile_seg = b->p_tile_seg; PP.pos = b->pos; PP.ref = b->ref; PP.alt = b->alt; PP.qual = b->qual; PP.flags = b->flags; PP.anib = b->anib;
  PP.cnt = b->p_cnt; PP.off = b->p_off; PP.cursor = b->p_cursor; PP.segflags = b->p_flags; PP.ent = b->p_ent;
  PP.mask_pass = reinterpret_cast<uint32_t*>(b->mask_pass.p); PP.mask_tp = reinterpret_cast<uint32_t*>(b->mask_tp.p); PP.n_seg = nh_all; PP.n_bins = b->n_bins;
  launch_part_hist(PP, (int)nt1, st);
  std::vector<uint32_t> cnt((size_t)nh_all * NC), pfl((size_t)nh_all);
  HIPCHK(hipMemcpyAsync(cnt.data(), b->p_cnt, 4 * cnt.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(pfl.data(), b->p_flags, 4 * pfl.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));   // (also: the host tables above may go)
  for (int hh = 0; hh < nh_all; ++hh) {
    rc = flag_failure(pfl[(size_t)hh] & SPANF_BADPOS, vs[(size_t)half_vcf[(size_t)hh]]);
    if (rc != QM_OK) return rc;
  }
  // --- exact regions; one level-2 segment per (VCF, partition in use).  The same VCFs with the same counts as last time (a batch
  //     run again): every table below is still on the device
  if (!(same_vs && b->tables.key == cnt)) {
    b->tables = qm_batch::Tables();
    std::vector<uint32_t> off((size_t)nh_all * (NC + 1));
    std::vector<uint32_t> half_off;   // [segment][4]: where the entries of the VCF's 2nd, 3rd, 4th half begin inside the segment's run
    ChunkTables T;
    for (int i = 0; i < nv; ++i) {
      const VcfDesc& d = b->L.vcfs[(size_t)vs[(size_t)i]];
      uint32_t run = 0;
      const int seg0 = (int)T.segs.size();
      const int h0 = vcf_half0[(size_t)i], h1 = vcf_half0[(size_t)i + 1];
      for (int p = 0; p < P2_PARTS; ++p) {
        run = (run + 1u) & ~1u;
        const uint32_t start = run;
        uint32_t hb[4] = {0u, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        for (int hh = h0; hh < h1; ++hh) {   // the halves' regions of the partition one behind the other
          hb[hh - h0] = run - start;
          for (int k = 0; k < P2_SUBS; ++k) { off[(size_t)hh * (NC + 1) + (size_t)p * P2_SUBS + k] = run; run += cnt[(size_t)hh * NC + (size_t)p * P2_SUBS + k]; }
        }
        const int64_t np = (int64_t)run - start;
        if (np == 0) continue;
        half_off.insert(half_off.end(), hb, hb + 4);
        // all 256 buckets of a partition are in use: more than 6 656 records per bucket on average will not fit 8 x 1 024
        if (np > (int64_t)HB_BUCKETS * HB_MAX_RECORDS * 13 / 16) { named->push_back(vs[(size_t)i]); return QM_OK; }
        SortSeg g;
        memset(&g, 0, sizeof g);
        g.src_off = d.off; g.koff = ps[(size_t)h0].ent_off + start; g.n = np;   // (the halves of a VCF share its level-1 region)
        g.main_vcf = vs[(size_t)i]; g.sub_vcf = i; g.main_tile0 = d.tile0;
        g.pad = DJ_MAX_SHIFT; g.nbk = HB_BUCKETS; g.key_base = (uint32_t)p << P2_SHIFT;
        // the buckets of a PARTITION as the "spans" of a VCF for k_finalize: one workgroup per partition (one per VCF summed
        // 1 536 rows by itself); k_sort_copy_rows adds a VCF's partitions up when the rows go home
        add_bucket_seg(&T, g, (np + BK_TILE - 1) / BK_TILE, HB_SUB_MAX, d.truth, false, HB_BUCKETS);
      }
      for (int hh = h0; hh < h1; ++hh) off[(size_t)hh * (NC + 1) + NC] = run;
      add_vcf_row(&T, d, vs[(size_t)i], seg0);
    }
    ktile_maps(b, vs, &T);
    rc = b->p_half.grow((int64_t)T.segs.size() * 4, by);
    if (rc != QM_OK) return rc;
    HIPCHK(hipMemcpyAsync(b->p_half, half_off.data(), 4 * half_off.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->p_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice, st));
    rc = upload_tables(b, Path::TwoLevel, vs, cnt, T, st);   // (its wait: the two tables above may go as well)
    if (rc != QM_OK) return rc;
  }
  const int nseg = b->tables.nseg;
  const CursorRegion C = cursor_region(b, nseg);
  HIPCHK(hipMemsetAsync(b->bk_cursor, 0, (size_t)C.words * 4, st));
  // --- level 1 scatter, then the one-level path over the partitions: rows, scatter from the level-1 entries, join, rows summed per VCF
  launch_part_scatter(PP, (int)nt1, st);
  BucketScatterParams S;
  HashParams H;
  bucket_params(b, nseg, false, C.seg_hist, &S, &H);
  S.l1_ent = b->p_ent; S.l1_half = any_halves ? b->p_half.p : nullptr;
  // (no look at the highest filled bucket, seg_maxd: every partition but a VCF's last fills its 256 buckets, and the look costs the
  // scatter more than the few empty workgroups cost the join -- 2.81 against 2.71 ms per 16 x 10 M records)
  launch_bucket_rows(H, nseg, st);
  launch_bucket_scatter(S, (int)b->tables.nbt, st);
  launch_join_lean(H, nseg, DJ_MAX_SHIFT, HB_BUCKETS, st);
  launch_finalize(bucket_rows_finalize(b, C.seg_hist), nseg, st);
  b->path_stats[QM_PATH_BUCKET_CHUNKS] += 1;
  return look_and_hand_over(b, nv, QM_PATH_DIRECT2, st, named);
}

// --- partitions of the key space, read from the columns: VCFs too large or too wide for 256 buckets (allele-extended ones;
// default-mode ones on references of 8.4 ... 16.8 M positions), and (wide) the wide buckets.
// The one-level path needs <= 8 192 records and <= 2^19 keys per bucket: configs[4]'s VCFs (2 M records on a 10 Mb genome) have
// neither.  The two-level path's first scatter packs level-1 entries that have no room for allele codes, so for these batches
// every PARTITION of 2^27 keys (256 buckets of 2^19) is a segment of the one-level scatter that reads ALL of its VCF's columns
// and keeps the records of its own key range (SortSeg.part).  Two neighbouring partitions share one pass (the 512-digit
// instantiation of the scatter: the first one's tiles fill both), so a 10 Mb genome costs ONE read of the columns, four partitions
// two; nothing else is new -- bucket rows, the two joins, the rows per segment and their sum per VCF are the one-level and
// two-level paths'.
// WIDE buckets: 2^17 positions and up to 32 768 records per bucket, 256 of them per partition of 2^29 keys.  A shuffled
// default-mode VCF of 1.3 ... 67 M records on a reference of up to 67 M positions -- configs[3]'s 10 M records on 50 Mb -- is then
// TWO partitions = ONE pass of the 512-digit scatter over its columns (pieces of 64 bytes and more: whole sectors) and
// k_join_lean<.., BIG> per bucket, where the two-level path moves every record twice.
// *named: the VCFs whose buckets overflowed.
static int partitions_chunk(qm_batch* b, const std::vector<int>& vs, hipStream_t st, const std::vector<uint32_t>& posor, bool wide,
                            std::vector<int>* named) {
  named->clear();
  const int nv = (int)vs.size();
  const Path path = wide ? Path::Wide : Path::Partitions;
  const int pshift = wide ? PW_SHIFT : P2_SHIFT, bshift = wide ? DJ_BIG_SHIFT : DJ_MAX_SHIFT;
  const int64_t sub_max = wide ? 4 * HB_SUB_MAX : HB_SUB_MAX;
  const bool xs = b->ext;                                  // two entry streams (allele-extended batches)
  constexpr int G = 2;                                     // partitions per pass over the columns
  const std::vector<uint32_t> key = posor_of(vs, posor);
  if (!owns(b, path, vs, key)) {
    ChunkTables T;
    for (int i = 0; i < nv; ++i) {
      const VcfDesc& d = b->L.vcfs[(size_t)vs[(size_t)i]];
      const uint32_t kor = (key[(size_t)i] << 4) | 15u;
      const int parts = parts_of(key[(size_t)i], pshift);
      const int seg0 = (int)T.segs.size();
      for (int p = 0; p < parts; ++p) {
        SortSeg g;
        memset(&g, 0, sizeof g);
        g.src_off = d.off; g.n = d.n; g.main_vcf = vs[(size_t)i]; g.sub_vcf = i; g.main_tile0 = d.tile0;
        g.pad = bshift; g.key_base = (uint32_t)p << pshift;
        // two neighbouring partitions share ONE pass over the columns: the tiles belong to the first of the pair, whose digits (512
        // of them) reach into the second's cursors, regions and rows (same capacity, laid out one behind the other)
        const int gfirst = p / G * G, gsize = std::min(G, parts - gfirst);
        const bool lead = p == gfirst && gsize > 1, follow = p != gfirst;
        const bool pair_last = gfirst + gsize == parts;
        g.part = (pair_last ? 2 : 1) | (lead ? 4 | (gsize << 4) : 0);
        g.nbk = p + 1 == parts ? std::min<int>(HB_BUCKETS, (int)((kor - g.key_base) >> bshift) + 1) : HB_BUCKETS;
        // (how the records spread over the partitions is not known: room as for all of them; the second of a pair has no tiles of
        // its own; the two streams' rows of a partition)
        add_bucket_seg(&T, g, follow ? 0 : (d.n + BK_TILE - 1) / BK_TILE, sub_max, d.truth, xs, xs ? 2 * HB_BUCKETS : HB_BUCKETS);
      }
      add_vcf_row(&T, d, vs[(size_t)i], seg0);
    }
    ktile_maps(b, vs, &T);
    const int rc = upload_tables(b, path, vs, key, T, st);
    if (rc != QM_OK) return rc;
  }
  const int nseg = b->tables.nseg;
  const CursorRegion C = cursor_region(b, nseg);
  if (xs) HIPCHK(hipMemsetAsync(b->bk_xcursor, 0, (size_t)nseg * HB_BUCKETS * HB_SUBS * 4, st));
  BucketScatterParams S;
  HashParams H;
  bucket_params(b, nseg, xs, C.seg_hist, &S, &H);
  S.pairs = 1;   // (tiles of single partitions run through the 512-digit instantiation as well)
  // (no look at the highest filled bucket, seg_maxd: measured on this path and lost, 2.08 against 2.02 ms per 64 x 2 M)
  H.zero = b->bk_cursor; H.n_zero = C.words;   // the scatter's cursors, flags and counts: cleared by the kernel that writes the rows (one dispatch instead of a memset's two)
  launch_bucket_rows(H, nseg, st);
  H.zero = nullptr; H.n_zero = 0u;
  launch_bucket_scatter(S, (int)b->tables.nbt, st);
  if (wide) launch_join_big(H, nseg, HB_BUCKETS, st);
  else launch_join_lean(H, nseg, DJ_MAX_SHIFT, HB_BUCKETS, st);
  if (xs) launch_join_ext(H, nseg, HB_BUCKETS, st);
  launch_finalize(bucket_rows_finalize(b, C.seg_hist), nseg, st);
  b->path_stats[QM_PATH_BUCKET_CHUNKS] += 1;
  return look_and_hand_over(b, nv, QM_PATH_PARTITIONS, st, named);
}

// --- one chunk on its path, and what an overflow leaves.  A run that overflows hands nothing over: the VCFs it names are held back
// and the others run again among themselves, up to PATHS[path].runs runs; every VCF then still without a result goes to the next path
// (the radix sort counts it as QM_PATH_RADIX_AFTER_OVERFLOW).  named: VCFs a run of this chunk has named already (settle_pending:
// the speculative run of a one-level chunk).
static int run_chunk_with_fallback(qm_batch* b, Path path, const std::vector<int>& chunk, hipStream_t st, const std::vector<uint32_t>& posor,
                                   std::vector<int> named = {}) {
  if (path == Path::Radix) return radix_chunk(b, chunk, st, posor, QM_PATH_RADIX);
  auto without = [](const std::vector<int>& a, const std::vector<int>& drop) {
    std::vector<int> r;
    for (int v : a) if (std::find(drop.begin(), drop.end(), v) == drop.end()) r.push_back(v);
    return r;
  };
  std::vector<int> vs = without(chunk, named);   // the VCFs of the next run
  bool done = false;
  for (int k = named.empty() ? 0 : 1; k < PATHS[(int)path].runs && !vs.empty(); ++k) {
    std::vector<int> more;
    int rc = QM_OK;
    switch (path) {
      case Path::OneLevel: rc = onelevel_chunk(b, vs, st, posor, k == 0, &more); break;
      case Path::TwoLevel: rc = two_level_chunk(b, vs, st, &more); break;
      default: rc = partitions_chunk(b, vs, st, posor, path == Path::Wide, &more); break;
    }
    if (rc != QM_OK) return rc;
    if (more.empty()) { done = true; break; }
    if (more.size() >= vs.size()) break;
    named.insert(named.end(), more.begin(), more.end());
    vs = without(vs, more);
  }
  const std::vector<int>& left = done ? named : chunk;
  if (left.empty()) return QM_OK;
  const Path next = PATHS[(int)path].next;
  if (next == Path::Radix) return radix_chunk(b, left, st, posor, QM_PATH_RADIX_AFTER_OVERFLOW);
  return run_chunk_with_fallback(b, next, left, st, posor);
}

// re-derive tile offsets + compaction for every VCF (cheap: masks only)
static int rescan_and_compact(qm_batch* b, hipStream_t st);

// The VCFs found out of order, redone: each on the path route() gives it, in chunks of that path.  posor[v]: the position bits the
// optimistic pass saw in VCF v.
static int redo_unsorted(qm_batch* b, const std::vector<int>& todo, const std::vector<uint32_t>& posor, hipStream_t st) {
  std::vector<int> by_path[N_PATHS];
  for (int v : todo) {
    const VcfDesc& d = b->L.vcfs[(size_t)v];
    by_path[(int)route(b->ext, d.n, posor[(size_t)v], b->ctx->truths[(size_t)d.truth].n, g_penv)].push_back(v);
  }
  const int64_t budget = sort_chunk_records();
  for (int p = N_PATHS - 1; p >= 0; --p) {   // (the wide buckets first, the radix sort last)
    const PathInfo& P = PATHS[p];
    std::vector<int> chunk;
    int64_t chunk_n = 0;
    for (size_t i = 0; i <= by_path[p].size(); ++i) {
      const bool end = i == by_path[p].size();
      const int v = end ? -1 : by_path[p][i];
      const int64_t w = end ? 0 : b->L.vcfs[(size_t)v].n * (P.per_pass ? (parts_of(posor[(size_t)v]) + 1) / 2 : 1);
      if (!chunk.empty() && (end || chunk_n + w > budget || (int)chunk.size() >= P.max_vcfs)) {
        const int rc = run_chunk_with_fallback(b, (Path)p, chunk, st, posor);
        if (rc != QM_OK) return rc;
        chunk.clear();
        chunk_n = 0;
      }
      if (!end) { chunk.push_back(v); chunk_n += w; }
    }
  }
  return QM_OK;
}

// The one-level chunks queued without a look at their flags (onelevel_chunk: speculate), behind the wait that ended the step: the
// mirrors of their rows' k_finalize say whether a chunk fitted.  One that did not was left alone by k_sort_copy_rows (nothing of it
// joined the per-truth sums) and takes run_chunk_with_fallback now, followed by another rescan.
static int settle_pending(qm_batch* b, const std::vector<uint32_t>& posor, hipStream_t st) {
  std::vector<qm_batch::Pending> pend;
  pend.swap(b->pend);
  b->pend_segs = 0;
  // every chunk's verdict first: a re-run below writes its own mirror words over theirs
  std::vector<std::vector<int>> named(pend.size());
  for (size_t k = 0; k < pend.size(); ++k) {
    const qm_batch::Pending& p = pend[k];
    const uint32_t* fl = b->h_summary + 16 + 2 * (size_t)b->n_vcf + (size_t)p.off;
    const uint32_t* md = b->h_summary + 16 + 3 * (size_t)b->n_vcf + (size_t)p.off;
    if (p.tight && memo_on()) {
      if (b->known_nbk.empty()) b->known_nbk.assign((size_t)b->n_vcf, 0u);
      for (size_t i = 0; i < p.vs.size(); ++i) if (md[i] <= (uint32_t)p.nbk_launch) b->known_nbk[(size_t)p.vs[i]] = std::max(md[i], 1u);
    }
    const int rc = bucket_verdict(b, fl, p.tight ? md : nullptr, (uint32_t)p.nbk_launch, p.vs, &named[k]);
    if (rc != QM_OK) return rc;
  }
  bool again = false;
  for (size_t k = 0; k < pend.size(); ++k) {
    const qm_batch::Pending& p = pend[k];
    if (named[k].empty()) { b->path_stats[p.direct ? QM_PATH_DIRECT : QM_PATH_HASHED] += (int64_t)p.vs.size(); continue; }
    if (p.tight && !b->known_nbk.empty()) for (int v : p.vs) b->known_nbk[(size_t)v] = 0u;
    // (what the radix sort learns about its chunk's positions corrects the estimate such a VCF is remembered with: posor_seen)
    const int rc = run_chunk_with_fallback(b, Path::OneLevel, p.vs, st, posor, named[k]);
    if (rc != QM_OK) return rc;
    again = true;
  }
  return again ? rescan_and_compact(b, st) : QM_OK;
}

extern "C" int qm_batch_finish(qm_batch* b, void* stream) {
  if (!b || !b->ran) return fail(QM_E_STATE, "qm_batch_finish: nothing was run");
  qm_ctx* c = b->ctx;
  HIPCHK(hipSetDevice(c->dev));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (b->finished) { HIPCHK(hipStreamSynchronize(st)); return QM_OK; }
  if (read_path_env() != QM_OK) { (void)hipStreamSynchronize(st); return QM_E_INVAL; }
  for (auto& x : b->path_stats) x = 0;
  b->pend.clear(); b->pend_segs = 0;
  // QM_FINISH_TRACE=1: the host's clock at the stations of this call, in us since it was entered (stderr)
  static const bool ftrace = getenv("QM_FINISH_TRACE") != nullptr;
  double ft[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (ftrace) ft[0] = ftrace_now();
  // an error exit: nothing of this run is left in flight behind it, no chunk waits to be settled; what the batch remembers goes where
  // the error may have come from what it remembered (forget: all of it)
  auto abandon = [&](int rc, bool forget) {
    (void)hipStreamSynchronize(st);
    b->pend.clear(); b->pend_segs = 0;
    if (forget) forget_known(b, -1);
    return rc;
  };
  std::vector<uint32_t> posor((size_t)b->n_vcf, 0u);
  bool redone = false;
  if (b->run_used_known) {
    // the VCFs known to be out of order: their bucket path goes onto the stream behind the run, before anything is waited for
    std::vector<int> kn;
    for (int v = 0; v < b->n_vcf; ++v) if (b->known[(size_t)v]) { kn.push_back(v); posor[(size_t)v] = b->known_posor[(size_t)v]; }
    b->path_stats[QM_PATH_UNSORTED] += (int64_t)kn.size();
    const int rc = redo_unsorted(b, kn, posor, st);
    if (rc != QM_OK) return abandon(rc, true);
    redone = !kn.empty();
  }
  // every VCF known to be out of order: the run launched no optimistic pass, nothing can have raised a flag, and the rescan below
  // goes onto the stream behind the bucket path without a round trip through the host in between
  const bool nothing_ran = b->run_used_known && b->n_known == b->n_vcf && b->h_summary != nullptr;
  // the flags (and their mirrors) are complete behind the k_finalize part that writes them: the wait is for that kernel, while the
  // run's compaction and row sums go on -- the bucket path of what is found out of order is built and queued beside them.
  // Without the mirrors the flags are copied back: the wait is for the whole stream.
  bool idle = nothing_ran;   // has the stream been waited for?
  if (!nothing_ran) {
    if (b->flags_recorded && b->h_summary) HIPCHK(hipEventSynchronize(b->ev_flags));
    else { HIPCHK(hipStreamSynchronize(st)); idle = true; }
  }
  if (ftrace) ft[1] = ftrace_now();
  std::vector<int> todo;
  if (!nothing_ran) {
    std::vector<uint32_t> fl((size_t)b->n_vcf);
    if (b->h_summary) memcpy(fl.data(), b->h_summary + 16, 4 * fl.size());   // k_finalize's host-mapped mirror: complete behind the wait above
    else HIPCHK(hipMemcpy(fl.data(), b->vcf_flags, 4 * fl.size(), hipMemcpyDeviceToHost));
    for (int v = 0; v < b->n_vcf; ++v) {
      if (fl[(size_t)v] & (SPANF_BADPOS | SPANF_RUNLIMIT)) return abandon(flag_failure(fl[(size_t)v], v), false);
      if ((fl[(size_t)v] & SPANF_UNSORTED) && !(b->run_used_known && b->known[(size_t)v])) todo.push_back(v);
    }
    if (!todo.empty()) {
      std::vector<uint32_t> po((size_t)b->n_vcf);
      if (b->h_summary) memcpy(po.data(), b->h_summary + 16 + b->n_vcf, 4 * po.size());
      else HIPCHK(hipMemcpy(po.data(), b->vcf_posor, 4 * po.size(), hipMemcpyDeviceToHost));
      for (int v : todo) posor[(size_t)v] = po[(size_t)v];
      b->path_stats[QM_PATH_UNSORTED] += (int64_t)todo.size();
      if (ftrace) ft[2] = ftrace_now();
      const int rc = redo_unsorted(b, todo, posor, st);
      if (rc != QM_OK) return abandon(rc, false);
      if (ftrace) ft[3] = ftrace_now();
      redone = true;
    }
  }
  if (redone) {
    int rc = rescan_and_compact(b, st);
    if (rc == QM_OK && !b->pend.empty()) rc = settle_pending(b, posor, st);
    if (rc != QM_OK) return abandon(rc, memo_on());
  } else if (nothing_ran || !idle) {
    HIPCHK(hipStreamSynchronize(st));
  }
  if (memo_on() && !todo.empty()) {
    if (b->known.empty()) { b->known.assign((size_t)b->n_vcf, (uint8_t)0); b->known_posor.assign((size_t)b->n_vcf, 0u); }
    for (int v : todo) if (!b->known[(size_t)v]) {
      b->known[(size_t)v] = 1; b->known_posor[(size_t)v] = posor[(size_t)v] | (b->posor_seen.empty() ? 0u : b->posor_seen[(size_t)v]);
      ++b->n_known; b->known_dirty = true;
    }
  }
  for (int k = 0; k < QM_N_PATH_STATS; ++k) c->path_total[k] += b->path_stats[k];
  b->finished = true;
  if (ftrace) {
    ft[4] = ftrace_now();
    fprintf(stderr, "finish trace: flags waited for %.1f us, read %.1f, bucket path queued %.1f, everything done %.1f (the latest chunk: entered %.1f, tables %.1f, scatter queued %.1f)\n", ft[1] - ft[0],
            ft[2] ? ft[2] - ft[0] : 0.0, ft[3] ? ft[3] - ft[0] : 0.0, ft[4] - ft[0], g_ftrace[0] - ft[0], g_ftrace[1] - ft[0], g_ftrace[2] - ft[0]);
  }
  return QM_OK;
}

// k_finalize recomputes the offsets of every tile; to keep ROC rows and per-truth
// sums untouched it runs on a throw-away output set.
static int rescan_and_compact(qm_batch* b, hipStream_t st) {
  int rc = b->rs_roc.grow((int64_t)b->n_vcf * 3 * b->n_bins, &b->dev_bytes);
  if (rc == QM_OK) rc = b->rs_scal.grow((int64_t)b->n_vcf * 8, &b->dev_bytes);
  if (rc == QM_OK) rc = b->rs_flags.grow(b->n_vcf, &b->dev_bytes);
  if (rc != QM_OK) return rc;
  FinalizeParams F = finalize_params(b, nullptr);
  F.roc = b->rs_roc; F.scalars = b->rs_scal; F.vcf_flags = b->rs_flags; F.vcf_posor = nullptr;
  F.parts = 1;   // the tile offsets only: the rows it would sum are thrown away (611 span rows per 10 M-record VCF: 0.3 ms for sixteen of them)
  launch_finalize(F, b->n_vcf, st);
  CompactParams CP = compact_params(b);
  CP.skip_unsorted = 0;   // the flags still say 'unsorted' for the VCFs just redone: compact them too
  launch_compact(CP, (int)b->L.spans.size(), st);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(QM_E_HIP, "rescan/compact: %s", hipGetErrorString(e));
  return QM_OK;
}
