// qmvt_surface.h -- the filter surface pass (qmvt_surface.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_surface, qm_batch_get_surface).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int SF_MAX_NQ = 256;           // include/qmvt.h QM_SF_MAX_QUAL_BINS
constexpr int SF_MAX_NA = 64;            // include/qmvt.h QM_SF_MAX_AF_BINS
constexpr int SF_MAX_CELLS = 4096;       // include/qmvt.h QM_SF_MAX_CELLS: nq * na at most (two u32 grids: 32 KiB of LDS)
constexpr int SF_GRIDS = 3;              // TP records, FP records, found truth keys (U)
constexpr int SF_EXTRA = 4;              // include/qmvt.h QM_SF_*: counted, counted without AF, left out (no bin), T'
constexpr int SF_REC_EXTRA = 3;          // ... of which k_surface_records counts the first three
constexpr int SF_STAGE = 4096;           // truth keys whose best codes a workgroup stages in LDS (16 KiB); larger sets go to HBM
constexpr int SF_TRUTH_CHUNK = 8192;     // truth keys per workgroup of k_surface_truth (at most 64 workgroups per VCF)
// dynamic LDS of k_surface_records, in u32 words: the two grids, the extras, the staged codes -- 49 168 bytes at the cell limit
inline size_t sf_records_lds_words(int cells) { return (size_t)2 * (size_t)cells + SF_EXTRA + SF_STAGE; }
static_assert(((size_t)2 * SF_MAX_CELLS + SF_EXTRA + SF_STAGE) * 4 <= 65536, "grids plus staging: what a launch gets without asking");

struct SurfaceParams {
  const SpanDesc* spans;
  const TruthDev* truths;
  const uint8_t* has_af;      // [n_vcf]: 0 = the VCF's frequencies were not uploaded, every record of it has no AF
  const int64_t* best_off;    // [n_vcf + 1] first code of every VCF's row of `best`
  const int32_t* pos;
  const uint8_t* anib;
  const uint8_t* flags;
  const float* qual;
  const float* af;            // laid out like pos; may be NULL when no VCF has the mark
  uint32_t* best;             // per (VCF, truth key): max(1 + qb * na + ab) over its counted '.'-ID records, 0 = never; cleared before the launch
  unsigned long long* grid;   // [n_vcf][SF_GRIDS][nq * na], cleared on the same stream before the launch
  unsigned long long* extra;  // [n_vcf][SF_EXTRA], likewise
  int32_t n_spans;
  int32_t q_step, nq, na;
};

void launch_surface_records(const SurfaceParams& P, hipStream_t st);
void launch_surface_truth(const SurfaceParams& P, int n_vcf, int64_t max_tn, hipStream_t st);
void launch_surface_sums(const SurfaceParams& P, int n_vcf, hipStream_t st);

}  // namespace qm
