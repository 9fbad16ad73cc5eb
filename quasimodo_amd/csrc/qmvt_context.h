// qmvt_context.h -- the sequence-context pass (qmvt_context.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_genome_context, qm_batch_context).  Kept apart from qmvt_dev.h so that the kernels id stays what the profiles
// of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int CX_MAX_HALF_WINDOW = 1024;     // include/qmvt.h QM_CX_MAX_HALF_WINDOW
constexpr int CX_MAX_GC_BINS = 15;           // QM_CX_MAX_GC_BINS
constexpr int CX_HP_ROWS = 16;               // homopolymer rows 0 .. 15 (15 = 15 and longer)
constexpr int CX_MAX_CELLS = CX_HP_ROWS * CX_MAX_GC_BINS + 1;   // the grid and NONE
constexpr uint32_t CX_NONE = 255u;           // the table's byte of a position without a cell
constexpr int CX_TILE = 4096;                // positions per workgroup of k_context_build: 16 per lane, one 16-byte store
constexpr int CX_STAGE = CX_TILE + 2 * CX_MAX_HALF_WINDOW;   // the tile and its halo: 24 staged positions per lane
// The reduction that lost the A/B of LABNOTES round 17 stays buildable, not shipped: -DQM_CX_VARIANT=1 a wave's records of one cell
// are added once (ballot / match on the cell) instead of one LDS atomic per record.  The outputs are the same.
#ifndef QM_CX_VARIANT
#define QM_CX_VARIANT 0
#endif
constexpr bool CX_AGGREGATE = (QM_CX_VARIANT & 1) != 0;

// k_context_build: the 4-bit packed genome of qm_genome_load (words = len / 8 + 2, no base past the end) -> tab[p - 1] = cell(p),
// gen[cell] += 1 for p = 1 .. len.  tab holds len rounded up to 16 bytes; gen is cleared on the same stream before the launch.
struct ContextBuildParams {
  const uint32_t* words;
  uint8_t* tab;
  unsigned long long* gen;   // [16 ng + 1]
  int32_t len;
  int32_t w;
  int32_t ng;
  int32_t pad;
};

// the table of one VCF's genome (tab null: the VCF names no genome, its rows stay zero)
struct ContextTab {
  const uint8_t* tab;
  int64_t len;
};

struct ContextRecParams {
  const SpanDesc* spans;
  const ContextTab* tabs;     // [n_vcf]
  const int32_t* pos;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint64_t* out;              // [n_vcf][16 ng + 2][2] (kept, TP), cleared on the same stream before the launch
  int32_t n_spans;
  int32_t ng;
};

// one VCF of k_context_truth: the sorted distinct keys of its truth set, its hit bitmap, its genome's table
struct ContextTruthRow {
  const uint32_t* keys;
  const uint32_t* hits;
  const uint8_t* tab;         // null: zero rows
  int64_t n;                  // T' as the hit bitmaps were sized
  int64_t len;
};

void launch_context_build(const ContextBuildParams& P, hipStream_t st);
void launch_context_records(const ContextRecParams& P, hipStream_t st);
// out[v][16 ng + 1][2] += (keys of the cell, those of them hit); cleared on the same stream before the launch
void launch_context_truth(const ContextTruthRow* rows, int n_vcf, int64_t max_n, int ng, unsigned long long* out, hipStream_t st);

}  // namespace qm
