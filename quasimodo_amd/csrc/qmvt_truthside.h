// qmvt_truthside.h -- the truth-side pass (qmvt_truthside.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_truth_hits, qm_batch_truth_regions).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int TS_LDS_WORDS = 4096;       // hit-bitmap words a workgroup collects in LDS (16 KB: truth sets up to 131 072 keys)
constexpr int TS_MAX_GROUP = 5;          // include/qmvt.h QM_TRUTH_GROUP_MAX: VCFs per group of k_truth_regions
constexpr int TS_REGIONS = 32;           // 1 << TS_MAX_GROUP slots per group
// The arms that lost the A/B of LABNOTES round 9 stay buildable, not shipped: -DQM_TS_VARIANT=1 one global atomic per hit instead
// of the LDS bitmap, 2 every kept record looked up (no IDDOT shortcut), 3 both.  The outputs are the same.
#ifndef QM_TS_VARIANT
#define QM_TS_VARIANT 0
#endif
constexpr bool TS_USE_LDS = !(QM_TS_VARIANT & 1);
constexpr bool TS_SHORTCUT = !(QM_TS_VARIANT & 2);

struct TruthHitsParams {
  const SpanDesc* spans;
  const TruthDev* truths;
  const int64_t* hit_off;     // [n_vcf + 1] first word of every VCF's hit bitmap
  const int32_t* pos;
  const uint8_t* anib;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint32_t* hits;             // cleared on the same stream before the launch
  uint8_t* mask_intruth;      // the record mask as bytes (bit r & 7 of byte r >> 3: the layout of mask_pass / mask_tp)
  int32_t n_spans;
};

// one group of k_truth_regions: n VCFs of one truth set
struct TruthGroup {
  const uint32_t* bits[TS_MAX_GROUP];
  uint32_t* uni;              // or null: the OR of the members' bitmaps, `words` words
  int64_t words;              // ceil(tn / 32)
  int64_t tn;                 // T'
  int32_t n;
  int32_t pad;
};

void launch_truth_hits(const TruthHitsParams& P, hipStream_t st);
void launch_truth_regions(const TruthGroup* groups, int n_groups, int64_t max_words, unsigned long long* regions, hipStream_t st);

}  // namespace qm
