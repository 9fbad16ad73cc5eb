// qmvt_ltypes.h -- the match ladder per variant type and size (qmvt_ltypes.hip) and its host side (qmvt_api.cpp).  Internal; the
// public surface is include/qmvt.h (qm_batch_ladder_types).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_ladder.h"
#include "qmvt_types.h"

namespace qm {

// a row's cells in the LDS histogram are its 18 output columns: [0] (KEPT / ENTRIES) stays zero while records are counted and
// is formed from the other 17 in front of the flush
constexpr int LTYPE_LDS_WORDS = TYPE_MAX_ROWS * LADDER_COLS;

struct LtypeRecParams {
  const SpanDesc* spans;
  const uint8_t* row;        // [n_pad] the row bytes of qm_batch_types(.., QM_TYPE_COLUMNS)
  const uint8_t* mask;       // [n_pad] the mask bytes of qm_batch_ladder(.., QM_LADDER_COLUMNS)
  uint64_t* rec;             // [n_vcf][n_rows][LADDER_COLS], cleared on the same stream before the launch
  int32_t n_spans;
  int32_t n_rows;
};

struct LtypeTruthParams {
  const TypeVcf* tvcfs;      // [n_vcf] what the latest qm_batch_types left: the truth set's allele-extended table
  const LadderVcf* lvcfs;    // [n_vcf] what the latest qm_batch_ladder left: where the VCF's entry bytes start
  const uint8_t* emask;      // the entry bytes of qm_batch_ladder(.., QM_LADDER_COLUMNS)
  uint64_t* tru;             // [n_vcf][n_rows][LADDER_COLS], cleared on the same stream before the launch
  TypeShapes shapes;         // of the latest qm_batch_types
  TypeBins bins;
};

void launch_ltype_records(const LtypeRecParams& P, hipStream_t st);
// max_entries: the largest truth set among the VCFs
void launch_ltype_truth(const LtypeTruthParams& P, int n_vcf, int64_t max_entries, hipStream_t st);

}  // namespace qm
