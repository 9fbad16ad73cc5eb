// qmvt_boot.h -- the paired block-bootstrap pass (qmvt_boot.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_boot, qm_batch_get_boot, qm_boot_draws).  Kept apart from qmvt_dev.h so that the kernels id stays what
// the profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_afprofile.h"   // AfpDiv / afp_div: the exact reciprocal of (pos - 1) / window

namespace qm {

constexpr int BOOT_MAX_WINDOWS = 4096;     // include/qmvt.h QM_BOOT_MAX_WINDOWS: [4096 + 2][2] u32 counters = 32 784 B of LDS
constexpr int BOOT_MAX_REP = 16384;        // QM_BOOT_MAX_REP
constexpr int BOOT_COLS = 4;               // kept lines, TP lines, truth keys, hit keys
constexpr int BOOT_VCF_SPLIT = 64;         // at most this many workgroups share the VCFs of one replicate
// The reduction that the wave's ballot replaced stays buildable, not shipped: -DQM_BOOT_VARIANT=1 one LDS atomic per counted
// record.  The outputs are the same.
#ifndef QM_BOOT_VARIANT
#define QM_BOOT_VARIANT 0
#endif
constexpr bool BOOT_BALLOT = !(QM_BOOT_VARIANT & 1);

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QM_BOOT_HD __host__ __device__
#else
#define QM_BOOT_HD
#endif

// Draw j of replicate b: the splitmix64 finaliser over seed + golden * (b * n_win + j + 1), reduced to 0 .. n_win - 1 by a
// multiply-shift of its upper half (bias below n_win / 2^32).  All arithmetic is mod 2^64.  The one statement of the hash: the
// kernel and qm_boot_draws both compile this.
QM_BOOT_HD inline uint32_t boot_draw(uint64_t seed, uint32_t b, uint32_t j, uint32_t n_win) {
  const uint64_t x = seed + 0x9E3779B97F4A7C15ull * ((uint64_t)b * n_win + j + 1ull);
  uint64_t z = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (uint32_t)(((z >> 32) * (uint64_t)n_win) >> 32);
}

// The divisor of a window: windows of 2^28 positions or more hold every position the reciprocal is asked about in window 0
// (mul = 0), and afp_div is defined below that only.
inline AfpDiv boot_div(int32_t window) {
  return (uint32_t)window < (1u << AFP_POS_BITS) ? afp_div((uint32_t)window) : AfpDiv{0u, 0u};
}

struct BootRecParams {
  const SpanDesc* spans;
  const int32_t* pos;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint64_t* cnt;              // [n_vcf][n_win + 2][BOOT_COLS]; columns 0 and 1 are added to; cleared on the same stream before the launch
  int32_t n_spans;
  int32_t window, n_win;
  AfpDiv div;                 // boot_div(window)
};

// one VCF of k_boot_truth: the sorted distinct keys of its truth set, its hit bitmap
struct BootTruthRow {
  const uint32_t* keys;       // [n]
  const uint32_t* hits;       // [ceil(n / 32)]
  int64_t n;
};

void launch_boot_records(const BootRecParams& P, hipStream_t st);
// cnt[v][.][2], cnt[v][.][3] = (truth keys of the row, those of them hit); cnt cleared on the same stream before the launch
void launch_boot_truth(const BootTruthRow* rows, int n_vcf, int32_t window, int32_t n_win, uint64_t* cnt, hipStream_t st);
// rep[v][b][c] = sum_w mult[b][w] * cnt[v][w][c] + cnt[v][n_win][c] + cnt[v][n_win + 1][c]; every word of rep is stored
void launch_boot_resample(const uint64_t* cnt, int n_vcf, int32_t n_win, int32_t n_rep, uint64_t seed, uint64_t* rep, hipStream_t st);

}  // namespace qm
