// qmvt_rroc.h -- the QUAL sweep of the two per-record rescue passes (qmvt_rroc.hip) and its host side (qmvt_api.cpp).  Internal; the
// public surface is include/qmvt.h (qm_batch_rescue_roc).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_atom.h"

namespace qm {

constexpr int RROC_N = 0, RROC_A = 1;        // the two matchings (QM_RROC_NORM, QM_RROC_ATOM are 1 << these)
constexpr int RROC_MAX_BINS = 256;           // a batch has 1 .. 256 QUAL bins: b + 1 fits a 16-bit best cell

// 32-bit words that hold n 16-bit best cells
inline size_t rroc_cell_words(int64_t n) { return (size_t)((n + 1) / 2); }

// The best cells of one VCF: 16 bits per unit, two to a word, 0 = no carrier, else 1 + the highest QUAL bin of the unit's carriers.
// By normal form the unit is the form, named by the smallest entry index of its members (the nrow column of k_norm_records); by
// atoms there is a cell per slot of the truth set's atom set and a cell per allele-extended entry.
struct RrocVcf {
  uint32_t* best_n;          // [rroc_cell_words(xn)], null: the VCF named no genome, its rows by normal form stay zero
  uint32_t* best_atom;       // [slots / 2], null: the atoms were not asked for
  uint32_t* best_entry;      // [rroc_cell_words(xn)]
  int64_t xn;                // entries of the VCF's truth set
};

struct RrocRecParams {
  const SpanDesc* spans;
  const RrocVcf* vcfs;       // [n_vcf]
  const AtomVcf* avcfs;      // [n_vcf] the sets qm_batch_atomize left (atoms only)
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const float* qual;
  const uint8_t* flags;
  const int32_t* nrow;       // [n_pad] the truth row of every record's form, -1: none (normal form only)
  const uint16_t* hit_mask;  // [n_pad] which atoms of an atomisable record the set holds (atoms only)
  uint64_t* hist;            // [n_vcf][3][n_bins]: rows 0 (TP) and 1 (FP) are added to; cleared on the same stream first
  int32_t n_spans;
  int32_t n_bins;
};

// hist[v][0 .. 1] += the TP / FP histograms of VCF v, the best cells raised (mode: RROC_N or RROC_A)
void launch_rroc_records(int mode, const RrocRecParams& P, hipStream_t st);
// hist[v][2] = the histogram of the bests of VCF v's units, then all three rows become suffix sums; base[v][mode] = the baseline
// read from the producer's truth-side row (tru[v * tru_cols + tru_col], 0 where the VCF has no cells)
void launch_rroc_units(int mode, const RrocVcf* vcfs, const AtomVcf* avcfs, int n_vcf, uint64_t* hist, int n_bins, uint64_t* base,
                       const uint64_t* tru, int tru_cols, int tru_col, hipStream_t st);

}  // namespace qm
