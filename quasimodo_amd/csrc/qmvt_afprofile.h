// qmvt_afprofile.h -- the allele-frequency profile pass (qmvt_afprofile.hip) and its host side (qmvt_api.cpp).  Internal; the
// public surface is include/qmvt.h (qm_batch_upload_af, qm_batch_af_profile).  Kept apart from qmvt_dev.h so that the kernels id
// stays what the profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int AFP_NO_AF = 0;             // include/qmvt.h QM_AFP_*
constexpr int AFP_OUTSIDE = 1;
constexpr int AFP_N_GRID = 2;
constexpr int AFP_EXTRA = 3;
constexpr int AFP_MAX_CELLS = 8192;      // n_af * n_pos at most: 2 * 8192 u32 = 64 KiB of LDS
constexpr int AFP_POS_BITS = 28;         // the reciprocal divides every (pos - 1) < 2^28 exactly

// floor(n / d) for every n < 2^28 as (n * mul) >> shift: shift = 28 + ceil(log2 d), mul = floor(2^shift / d) + 1 < 2^29.
// (Granlund & Montgomery 1994, theorem 4.2: 2^shift < mul * d <= 2^shift + d <= 2^shift + 2^ceil(log2 d).)
struct AfpDiv {
  uint32_t mul;
  uint32_t shift;
};
inline AfpDiv afp_div(uint32_t d) {   // 1 <= d < 2^28
  uint32_t l = 0;
  while ((1u << l) < d) ++l;
  const uint32_t sh = AFP_POS_BITS + l;
  return AfpDiv{(uint32_t)((1ull << sh) / d) + 1u, sh};
}

struct AfProfileParams {
  const SpanDesc* spans;
  const uint8_t* has_af;      // [n_vcf]: 0 = the VCF's frequencies were not uploaded, its rows stay zero
  const int32_t* pos;
  const float* af;            // laid out like pos
  const uint8_t* anib;        // batches without QM_BATCH_ALLELES
  const int32_t* ref;         // allele-extended batches: the int32 codes
  const int32_t* alt;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint64_t* grid;             // [n_vcf][2][n_af][n_pos], cleared on the same stream before the launch
  uint64_t* extra;            // [n_vcf][2][AFP_EXTRA], likewise
  int32_t n_spans;
  int32_t window, n_pos, n_af;
  AfpDiv div;                 // afp_div(window)
};

void launch_af_profile(const AfProfileParams& P, bool ext, hipStream_t st);

}  // namespace qm
