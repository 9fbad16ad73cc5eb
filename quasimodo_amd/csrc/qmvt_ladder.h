// qmvt_ladder.h -- the four rescues combined (qmvt_ladder.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_ladder).  Kept apart from qmvt_dev.h so that the kernels id stays what the profiles of the
// classification pass are keyed on.
#pragma once
#include "qmvt_atom.h"
#include "qmvt_haplo.h"
#include "qmvt_norm.h"

namespace qm {

constexpr int LADDER_COLS = 18;              // include/qmvt.h QM_LADDER_COLS: two totals, then the 16 cells of the four method bits
// the bits of a mask byte (QM_LADDER_M_*)
constexpr uint32_t LADDER_N = 1u, LADDER_A = 2u, LADDER_H = 4u, LADDER_B = 8u, LADDER_K = 64u, LADDER_S = 128u;
// LadderVcf::has
constexpr uint32_t LADDER_HAS_NORM = 1u, LADDER_HAS_HAP = 2u;

// what the latest producer calls left of one VCF beyond their own descriptors
struct LadderVcf {
  int64_t eoff;              // the VCF's first byte in the entry masks (every VCF has its truth set's entries there)
  int64_t heoff;             // ... in the search's second entry classes (laid out as the haplotype pass's: VCFs with a genome only)
  uint32_t has;              // LADDER_HAS_NORM: the VCF named a genome in qm_batch_normalize; LADDER_HAS_HAP: in qm_batch_haplotypes
  uint32_t pad;
};

struct LadderRecParams {
  const SpanDesc* spans;
  const LadderVcf* vcfs;     // [n_vcf]
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  const uint8_t* cls_n;      // [n_pad] the class bytes of qm_batch_normalize
  const uint8_t* cls_a;      // ... of qm_batch_atomize
  const uint8_t* cls_h;      // ... of qm_batch_haplotypes
  const uint8_t* cls_b;      // the second class bytes of qm_batch_hapsubsets, or null: the bit stays 0
  uint8_t* mask;             // [n_pad] a mask byte per record, or null
  uint64_t* rec;             // [n_vcf][LADDER_COLS], cleared on the same stream before the launch
  int32_t n_spans;
  int32_t pad;
};

struct LadderTruthParams {
  const LadderVcf* vcfs;     // [n_vcf]
  const NormVcf* nvcfs;      // [n_vcf] what the three producers left
  const AtomVcf* avcfs;
  const HapVcf* hvcfs;
  const uint8_t* ecls_b;     // the search's second entry classes, or null: the bit stays 0
  uint8_t* emask;            // a mask byte per (VCF, entry), or null
  uint64_t* tru;             // [n_vcf][LADDER_COLS], cleared on the same stream before the launch
  int32_t n_vcf;
  int32_t pad;
};

void launch_ladder_records(const LadderRecParams& P, hipStream_t st);
// max_entries: the largest truth set among the VCFs
void launch_ladder_truth(const LadderTruthParams& P, int64_t max_entries, hipStream_t st);

}  // namespace qm
