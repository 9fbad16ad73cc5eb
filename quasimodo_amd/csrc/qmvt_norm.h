// qmvt_norm.h -- the normalisation pass (qmvt_norm.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_normalize, qm_truth_normalized).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int NORM_R_COLS = 12;              // include/qmvt.h QM_NORM_R_COLS
constexpr int NORM_T_COLS = 5;               // QM_NORM_T_COLS
constexpr uint32_t NORM_MIN_SLOTS = 64u;     // the smallest table: two words of every bitmap
// class bytes (QM_NORM_C_*)
constexpr uint32_t NORM_UNCHANGED = 0u, NORM_RESPELLED = 1u, NORM_RESCUED = 2u, NORM_LONG = 3u, NORM_NOKEY = 4u, NORM_NOVAR = 5u,
                   NORM_RANGE = 6u, NORM_REFMISMATCH = 7u, NORM_NOBASE = 8u;

// slots of the table of a truth set with xn entries: a power of two, at least 2 xn
inline uint32_t norm_slots(int64_t xn) {
  uint32_t s = NORM_MIN_SLOTS;
  while ((int64_t)s < 2 * xn) s <<= 1;
  return s;
}

// The normalised truth set of one (truth set, genome): an open-addressing table over the 96-bit forms, linear probing.
// claim[s] = 0: empty, else 1 + the smallest entry index among the entries of the slot's form.  The per-entry arrays hold every
// entry's form (k_norm_truth); k_norm_insert claims slots by entry index, so a lane that meets a claimed slot reads the claimer's
// form from arrays an EARLIER launch wrote and never waits for another lane's stores; k_norm_fill copies the payload to the slots.
struct NormTable {
  const uint32_t* words;     // the genome, 4-bit packed (len / 8 + 2 words, no base past the end)
  int64_t len;
  const uint32_t* xkeys;     // the truth set's allele-extended table, sorted by (key, ref, alt)
  const int32_t* xref;
  const int32_t* xalt;
  int64_t xn;
  int32_t* fpos;             // [xn] the form of every entry
  int32_t* fref;
  int32_t* falt;
  uint32_t* claim;           // [slots]
  int32_t* spos;             // [slots] payload of the claimed slots
  int32_t* sref;
  int32_t* salt;
  uint32_t* sresp;           // [slots] != 0: some entry of the form was respelled
  unsigned long long* stats; // [2] distinct forms, entries that are not normalisable
  uint32_t slots;
  uint32_t pad;
};

// the table of one VCF and its two bitmaps over the slots (words null: the VCF names no genome, its rows stay zero)
struct NormVcf {
  NormTable t;
  uint32_t* found;           // [slots / 32] the form was found by a kept record
  uint32_t* found_eq;        // [slots / 32] ... by one spelled like an entry of the truth set
};

struct NormRecParams {
  const SpanDesc* spans;
  const NormVcf* vcfs;       // [n_vcf]
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint8_t* cls;              // [n_pad] class bytes
  int32_t* npos;             // [n_pad] normalised columns and the truth row of the form (-1: none), or all four null
  int32_t* nref;
  int32_t* nalt;
  int32_t* nrow;
  uint64_t* rec;             // [n_vcf][NORM_R_COLS], cleared on the same stream before the launch
  int32_t n_spans;
  int32_t pad;
};

// builds T on `st`: claim / sresp / stats are cleared on the same stream first
void launch_norm_truth(const NormTable& T, hipStream_t st);
void launch_norm_records(const NormRecParams& P, hipStream_t st);
// tru[v][NORM_T_COLS] of every VCF with a table
void launch_norm_found(const NormVcf* vcfs, int n_vcf, uint64_t* tru, hipStream_t st);

}  // namespace qm
