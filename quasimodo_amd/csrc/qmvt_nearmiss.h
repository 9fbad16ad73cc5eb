// qmvt_nearmiss.h -- the near-miss pass (qmvt_nearmiss.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_nearmiss, qm_batch_get_nearmiss*).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int NM_PLANES = 4;             // FILTERED, ALLELE, POSITION, NEAR: one bit per truth key each, laid out like the hit bitmap
constexpr int NM_LDS_WORDS = 1024;       // words of every plane a workgroup collects in LDS (4 x 4 KB: truth sets up to 32 768 keys)
constexpr int NM_MAX_RADIUS = 64;        // include/qmvt.h QM_NM_MAX_RADIUS
constexpr int NM_R_CLASSES = 6;          // include/qmvt.h QM_NM_R_*
constexpr int NM_T_CLASSES = 5;          // include/qmvt.h QM_NM_T_*
constexpr uint32_t NM_NONE = 255u;       // include/qmvt.h QM_NM_NONE
enum { NM_P_FILTERED = 0, NM_P_ALLELE = 1, NM_P_POSITION = 2, NM_P_NEAR = 3 };
enum { NM_R_IDCOL = 0, NM_R_ALLELE = 1, NM_R_REFBASE = 2, NM_R_NEAR = 3, NM_R_ISOLATED = 4, NM_R_NOKEY = 5 };

struct NearmissParams {
  const SpanDesc* spans;
  const TruthDev* truths;
  const int64_t* hit_off;     // [n_vcf + 1] first word of every VCF's hit bitmap (and of its row in every plane)
  const int32_t* pos;
  const uint8_t* anib;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint32_t* planes;           // [NM_PLANES][plane_words], cleared on the same stream before the launch
  int64_t plane_words;        // hit_off[n_vcf]
  uint8_t* rcls;              // one class byte per record, laid out like pos
  unsigned long long* rec;    // [n_vcf][NM_R_CLASSES], cleared on the same stream before the launch
  int32_t n_spans;
  int32_t radius;
};

struct NearmissTruthParams {
  const int64_t* hit_off;
  const int64_t* hit_tn;      // [n_vcf] T' of every VCF's truth set
  const uint32_t* hits;
  const uint32_t* planes;
  int64_t plane_words;
  unsigned long long* tru;    // [n_vcf][NM_T_CLASSES], cleared on the same stream before the launch
};

// the truth-side class of the keys of one word, by precedence: c[k] = the missed keys (bits of `miss`) of class k
__host__ __device__ inline void nearmiss_truth_word(uint32_t miss, uint32_t f, uint32_t a, uint32_t p, uint32_t n, uint32_t c[NM_T_CLASSES]) {
  c[0] = miss & f; miss &= ~f;
  c[1] = miss & a; miss &= ~a;
  c[2] = miss & p; miss &= ~p;
  c[3] = miss & n;
  c[4] = miss & ~n;
}

void launch_nearmiss_records(const NearmissParams& P, hipStream_t st);
void launch_nearmiss_truth(const NearmissTruthParams& P, int n_vcf, int64_t max_words, hipStream_t st);

}  // namespace qm
