// qmvt_strata.h -- the stratification pass (qmvt_strata.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_strata_load, qm_batch_strata).  Kept apart from qmvt_dev.h so that the kernels id stays what the profiles
// of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int STRATA_MAX = 32;               // include/qmvt.h QM_STRATA_MAX
constexpr int STRATA_LDS_SEGMENTS = 4096;    // QM_STRATA_LDS_SEGMENTS: 16 KiB of breakpoints + 16 KiB of masks
constexpr int STRATA_REC_ROWS = STRATA_MAX + 2;   // the strata, outside, nokey
constexpr int STRATA_PLANE_KEYS = 4096;      // truth keys per workgroup of k_strata_planes (the staged table is paid for once)
// The reduction that lost the A/B of LABNOTES round 12 stays buildable, not shipped: -DQM_STRATA_VARIANT=1 one LDS atomic per
// record and stratum bit instead of the wave's ballots.  The outputs are the same.
#ifndef QM_STRATA_VARIANT
#define QM_STRATA_VARIANT 0
#endif
constexpr bool STRATA_BALLOT = !(QM_STRATA_VARIANT & 1);

// The flattened strata set: breakpoints bp[0] = INT32_MIN < bp[1] < ... < bp[m - 1], masks[i] valid on [bp[i], bp[i + 1]) (the
// last segment runs to INT32_MAX).  cidx (m > STRATA_LDS_SEGMENTS only, else null): cidx[c] = the segment that holds the first
// position of cell c, cells of 1 << shift positions counted from INT32_MIN; ncell + 1 entries, the last m - 1.
struct StrataTable {
  const int32_t* bp;
  const uint32_t* masks;
  const int32_t* cidx;
  int32_t m;
  int32_t shift;
  int32_t n_strata;
  int32_t pad;
};

struct StrataRecParams {
  const SpanDesc* spans;
  const int32_t* pos;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint64_t* out;              // [n_vcf][S + 2][2] (kept, TP), cleared on the same stream before the launch
  StrataTable tab;
  int32_t n_spans;
};

// one VCF of k_strata_truth: the planes of its truth set, its hit bitmap
struct StrataTruthRow {
  const uint32_t* planes;     // [S + 1][words]
  const uint32_t* hits;       // [words]
  int64_t words;              // ceil(T' / 32)
};

void launch_strata_records(const StrataRecParams& P, hipStream_t st);
// planes[s][w] bit k = key 32 w + k of `keys` (n sorted distinct truth keys) lies in stratum s; plane S = in no stratum
void launch_strata_planes(const StrataTable& tab, const uint32_t* keys, int64_t n, uint32_t* planes, hipStream_t st);
// out[v][S + 1][2] += (keys of the row, those of them hit); cleared on the same stream before the launch
void launch_strata_truth(const StrataTruthRow* rows, int n_vcf, int64_t max_words, int n_strata, unsigned long long* out, hipStream_t st);

}  // namespace qm
