// qmvt_atom.h -- the atomisation pass (qmvt_atom.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_atomize, qm_truth_atoms).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int ATOM_R_COLS = 13;              // include/qmvt.h QM_ATOM_R_COLS
constexpr int ATOM_T_COLS = 6;               // QM_ATOM_T_COLS
constexpr uint32_t ATOM_MIN_SLOTS = 64u;     // the smallest set: two words of the atom bitmap
constexpr uint32_t ATOM_EMPTY = 0xffffffffu; // no atom: an atom's REF and ALT differ, so its low nibble is never 15
// class bytes (QM_ATOM_C_*)
constexpr uint32_t ATOM_FULL = 0u, ATOM_PARTIAL = 1u, ATOM_NONE = 2u, ATOM_RESCUED = 3u, ATOM_LONG = 4u, ATOM_NOKEY = 5u, ATOM_NOVAR = 6u,
                   ATOM_UNEQUAL = 7u, ATOM_RANGE = 8u;
// columns of rec (QM_ATOM_R_*)
constexpr int ATOM_R_KEPT = 0, ATOM_R_TP = 1, ATOM_R_TP_A = 2, ATOM_R_RESCUED = 3, ATOM_R_MULTI = 4, ATOM_R_PARTIAL = 5, ATOM_R_ATOMS = 6,
              ATOM_R_ATOMS_HIT = 7, ATOM_R_LONG = 8;

// slots of the set of a truth set whose atomisable entries have n_atoms atoms together: a power of two, at least 2 n_atoms
inline uint32_t atom_slots(int64_t n_atoms) {
  uint32_t s = ATOM_MIN_SLOTS;
  while ((int64_t)s < 2 * n_atoms) s <<= 1;
  return s;
}

// The atom set of one truth set: open addressing over the 32-bit atoms (pos << 4 | ref << 2 | alt), linear probing.  The key is
// the whole payload: a slot is claimed by one atomicCAS on the key word, and a lane that meets a claimed slot compares the word.
struct AtomTable {
  const uint32_t* xkeys;     // the truth set's allele-extended table, sorted by (key, ref, alt)
  const int32_t* xref;
  const int32_t* xalt;
  int64_t xn;
  uint32_t* set;             // [slots], ATOM_EMPTY where unclaimed
  unsigned long long* stats; // [2] distinct atoms, atomisable entries
  uint32_t slots;
  uint32_t pad;
};

// the set of one VCF and its two bitmaps
struct AtomVcf {
  AtomTable t;
  uint32_t* abits;           // [slots / 32] the atom of the slot is carried by a kept atomisable record
  uint32_t* ebits;           // [xn / 32 + 1] the entry is spelled like a kept record with valid codes and no QMF_NOKEY
};

struct AtomRecParams {
  const SpanDesc* spans;
  const AtomVcf* vcfs;       // [n_vcf]
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint8_t* cls;              // [n_pad] class bytes, atom counts and hit masks, or all three null
  uint8_t* n_atoms;
  uint16_t* hit_mask;
  uint64_t* rec;             // [n_vcf][ATOM_R_COLS], cleared on the same stream before the launch
  int32_t n_spans;
  int32_t pad;
};

// the atoms of the atomisable entries of a truth set, repeats included, added to *total (for atom_slots)
void launch_atom_count(const AtomTable& T, unsigned long long* total, hipStream_t st);
// builds T on `st`: set is filled with ATOM_EMPTY and stats cleared on the same stream first
void launch_atom_truth(const AtomTable& T, hipStream_t st);
void launch_atom_records(const AtomRecParams& P, hipStream_t st);
// tru[v][ATOM_T_COLS] of every VCF, cleared on the same stream before the launch
void launch_atom_found(const AtomVcf* vcfs, int n_vcf, int64_t max_lanes, uint64_t* tru, hipStream_t st);

}  // namespace qm
