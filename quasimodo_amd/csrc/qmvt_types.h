// qmvt_types.h -- the variant-type pass (qmvt_types.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_types, qm_dict_shapes).  Kept apart from qmvt_dev.h so that the kernels id stays what the profiles of
// the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int TYPE_MAX_BINS = 16;            // include/qmvt.h QM_TYPE_MAX_BINS
constexpr int TYPE_KINDS = 5;                // SNV, MNP, INS, DEL, CPX: the grid is [TYPE_KINDS][n_bins]
constexpr int TYPE_OFFGRID = 4;              // the rows behind the grid
constexpr int TYPE_MAX_ROWS = TYPE_KINDS * TYPE_MAX_BINS + TYPE_OFFGRID;   // QM_TYPE_MAX_ROWS
constexpr uint32_t TYPE_SNV = 0u, TYPE_MNP = 1u, TYPE_INS = 2u, TYPE_DEL = 3u, TYPE_CPX = 4u;   // QM_TYPE_*
constexpr uint32_t TYPE_NOKEY = 0u, TYPE_NOVAR = 1u, TYPE_LONGPAIR = 2u, TYPE_NOSHAPE = 3u;     // + TYPE_KINDS * n_bins
constexpr uint32_t TYPE_LONG_HEAD = 13u;     // bases of a long allele the shape table keeps at either end (QM_ALLELE_INLINE_MAX)

// One row per dictionary id: the length of the interned allele (at least 14) and its first and last 13 bases, 2 bits per base,
// base k at bits 2 k -- the layout of an inline code.  n = 0 (and null pointers) without a table.
struct TypeShapes {
  const int32_t* len;
  const uint32_t* head;
  const uint32_t* tail;
  int64_t n;
};

// the size bins: edges[0] == 1 < edges[1] < ...; bin b holds edges[b] <= size < edges[b + 1], the last one is open
struct TypeBins {
  int32_t edges[TYPE_MAX_BINS];
  int32_t n_bins;
  int32_t n_rows;            // TYPE_KINDS * n_bins + TYPE_OFFGRID
};

// the truth set of one VCF and the pass's own bitmap of its entries
struct TypeVcf {
  const uint32_t* xkeys;     // the truth set's allele-extended table, sorted by (key, ref, alt)
  const int32_t* xref;
  const int32_t* xalt;
  int64_t xn;
  uint32_t* ebits;           // [xn / 32 + 1] the entry is spelled like a kept record with valid codes and no QMF_NOKEY
};

// ---- how a variant is typed: shared by the pass (qmvt_types.hip) and by the pass that crosses its rows with the ladder's mask
// bytes (qmvt_ltypes.hip), so that a truth entry lands in the same row in both ----
// inline codes (include/qmvt.h): 0 .. 3 one base, len << 26 | bases for 2 .. 13 bases
__device__ inline bool vt_inline(int32_t c) {
  const uint32_t u = (uint32_t)c;
  return u < 4u || (u - (2u << 26)) < (12u << 26);
}

// bit 2 k: field k of the two words differs
__device__ inline uint32_t vt_diff(uint32_t x, uint32_t y) {
  const uint32_t d = x ^ y;
  return (d | d >> 1) & 0x1555555u;
}

// The row of the variant (r, a): TYPE_KINDS * n_bins + the first off-grid reason that applies, else type * n_bins + bin.
// What the trimming reads of an allele: its length, the word of its first bases and the word of its last `e` ones (base k at bits
// 2 k in both).  An inline code is both words itself; a long allele takes them from its row of the shape table.
__device__ inline uint32_t vt_row(int32_t r, int32_t a, bool nokey, const TypeShapes& S, const TypeBins& B) {
  const uint32_t off = (uint32_t)(TYPE_KINDS * B.n_bins);
  if (nokey || !allele_valid(r) || !allele_valid(a)) return off + TYPE_NOKEY;
  if (r == a) return off + TYPE_NOVAR;
  const bool long_r = !vt_inline(r), long_a = !vt_inline(a);
  if (long_r && long_a) return off + TYPE_LONGPAIR;
  const uint32_t ur = (uint32_t)r, ua = (uint32_t)a;
  uint32_t len_r = ur < 4u ? 1u : ur >> 26, len_a = ua < 4u ? 1u : ua >> 26;   // (of the inline ones)
  uint32_t head_r = ur & 0x03ffffffu, head_a = ua & 0x03ffffffu;
  uint32_t tail_r = head_r, tail_a = head_a, e_r = len_r, e_a = len_a;
  if (long_r || long_a) {
    // (a valid code under the dictionary's base is no inline code and no id: it has no row either)
    const uint32_t u = long_r ? ur : ua;
    const int64_t id = u >= 0x40000000u ? (int64_t)(u & 0x3fffffffu) : S.n;
    if (id >= S.n) return off + TYPE_NOSHAPE;
    const uint32_t len = (uint32_t)S.len[id], head = S.head[id] & 0x03ffffffu, tail = S.tail[id] & 0x03ffffffu;
    len_r = long_r ? len : len_r; head_r = long_r ? head : head_r; tail_r = long_r ? tail : tail_r; e_r = long_r ? TYPE_LONG_HEAD : e_r;
    len_a = long_a ? len : len_a; head_a = long_a ? head : head_a; tail_a = long_a ? tail : tail_a; e_a = long_a ? TYPE_LONG_HEAD : e_a;
  }
  // at most one allele is long, so m <= 13: neither count looks past the 13 bases a word holds
  const uint32_t m = min(len_r, len_a);
  const uint32_t fields = (1u << (2u * m)) - 1u;
  const uint32_t cp = (uint32_t)__builtin_ctz((vt_diff(head_r, head_a) & fields) | (1u << (2u * m))) >> 1;
  // the last m bases of either allele, base k of them at bits 2 k: equal fields are counted from the top
  const uint32_t ds = vt_diff(tail_r >> (2u * (e_r - m)), tail_a >> (2u * (e_a - m))) & fields;
  const uint32_t cs = min(ds ? (uint32_t)__builtin_clz(ds << (32u - 2u * m)) >> 1 : m, m - cp);   // the prefix went first
  const uint32_t tr = len_r - cp - cs, ta = len_a - cp - cs;
  const uint32_t type = tr == 0u ? TYPE_INS : ta == 0u ? TYPE_DEL : tr != ta ? TYPE_CPX : tr == 1u ? TYPE_SNV : TYPE_MNP;
  const uint32_t size = max(tr, ta);
  uint32_t bin = 0u;
#pragma unroll
  for (int i = 1; i < TYPE_MAX_BINS; ++i) bin += (i < B.n_bins && size >= (uint32_t)B.edges[i]) ? 1u : 0u;
  return type * (uint32_t)B.n_bins + bin;
}

struct TypeRecParams {
  const SpanDesc* spans;
  const TypeVcf* vcfs;       // [n_vcf]
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint8_t* row;              // [n_pad] the row of every record, or null
  uint64_t* rec;             // [n_vcf][n_rows][2], cleared on the same stream before the launch
  TypeShapes shapes;
  TypeBins bins;
  int32_t n_spans;
  int32_t pad;
};

struct TypeTruthParams {
  const TypeVcf* vcfs;       // [n_vcf]
  uint64_t* tru;             // [n_vcf][n_rows][2], cleared on the same stream before the launch
  TypeShapes shapes;
  TypeBins bins;
};

void launch_type_records(const TypeRecParams& P, hipStream_t st);
void launch_type_truth(const TypeTruthParams& P, int n_vcf, int64_t max_entries, hipStream_t st);

}  // namespace qm
