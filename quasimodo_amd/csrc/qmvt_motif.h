// qmvt_motif.h -- the mutation-context pass (qmvt_motif.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_genome_load, qm_batch_motifs).  Kept apart from qmvt_dev.h so that the kernels id stays what the profiles
// of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int MOTIF_COLS = 98;           // include/qmvt.h QM_MOTIF_COLS: 96 motifs, outside, REF mismatch
constexpr int MOTIF_OTHER = 96;
constexpr int MOTIF_REF_MISMATCH = 97;
constexpr int MOTIF_ROW_WORDS = 3 * MOTIF_COLS;   // kept, TP, FP
constexpr uint32_t GENOME_NOBASE = 15u;  // 4-bit genome code of a byte that is not ACGTacgt

// One genome as the device holds it: base i in bits 4 (i % 8) .. + 3 of word i / 8 (A=0 C=1 G=2 T=3, GENOME_NOBASE
// otherwise), words len / 8 + 2 (a window that starts in the last word still loads two).
struct GenomeRef {
  const uint32_t* words;   // null: the VCF has no genome, its rows stay zero
  int64_t len;
};

struct MotifParams {
  const SpanDesc* spans;
  const GenomeRef* genomes;   // [n_vcf]
  const int32_t* pos;
  const uint8_t* anib;        // batches without QM_BATCH_ALLELES
  const int32_t* ref;         // allele-extended batches: the int32 codes
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint64_t* out;              // [n_vcf][3][MOTIF_COLS], cleared on the same stream before the launch
  int32_t n_spans;
};

void launch_motif(const MotifParams& P, bool ext, hipStream_t st);

}  // namespace qm
