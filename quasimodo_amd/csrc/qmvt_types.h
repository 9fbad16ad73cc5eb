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
