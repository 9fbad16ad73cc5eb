// qmvt_haplo.h -- the haplotype pass (qmvt_haplo.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_haplotypes, qm_truth_sites).  Kept apart from qmvt_dev.h so that the kernels id stays what the
// profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int HAP_R_COLS = 16;               // include/qmvt.h QM_HAP_R_COLS
constexpr int HAP_T_COLS = 8;                // QM_HAP_T_COLS
constexpr int HAP_MAX_GAP = 32;              // QM_HAP_MAX_GAP
constexpr int HAP_MAX_WINDOW = 256;          // QM_HAP_MAX_WINDOW
constexpr int HAP_MAX_ITEMS = 8;             // QM_HAP_MAX_ITEMS
constexpr int HAP_PAIR_WORDS = HAP_MAX_ITEMS + 3;   // a (VCF, open site) pair: VCF, site, count of open lines, their record indices
// class bytes (QM_HAP_C_*); HAP_PENDING lives between k_hap_records and k_hap_claim / k_hap_replay only
constexpr uint32_t HAP_MATCHED = 0u, HAP_RESCUED = 1u, HAP_OUTSIDE = 2u, HAP_LONE = 3u, HAP_MISMATCH = 4u, HAP_CONFLICT = 5u,
                   HAP_TOOMANY = 6u, HAP_TOOLONG = 7u, HAP_LONG = 8u, HAP_NOKEY = 9u, HAP_NOVAR = 10u, HAP_RANGE = 11u,
                   HAP_REFMISMATCH = 12u, HAP_NOTKEPT = 13u, HAP_PENDING = 14u;
// columns (QM_HAP_R_* / QM_HAP_T_*): the column of class c >= HAP_OUTSIDE is c + 3
constexpr int HAP_R_KEPT = 0, HAP_R_TP = 1, HAP_R_TP_H = 2, HAP_R_RESCUED = 3, HAP_R_OPEN = 4, HAP_R_CLASS0 = 3;
constexpr int HAP_T_ENTRIES = 0, HAP_T_FOUND = 1, HAP_T_FOUND_H = 2, HAP_T_OPEN = 3, HAP_T_UNUSABLE = 4, HAP_T_SITES = 5,
              HAP_T_TRIED = 6, HAP_T_MATCHED = 7;

// The sites of one (truth set, genome, gap).  Per entry: 0 for a usable one, else the reason (HAP_LONG ...), its footprint and
// its site (-1 for the others); per site: the first entry and the window.  n_sites[0] is written by k_hap_sites.
struct HapSites {
  const uint32_t* words;     // the genome, 4-bit packed (len / 8 + 2 words, no base past the end)
  int64_t len;
  const uint32_t* xkeys;     // the truth set's allele-extended table, sorted by (key, ref, alt)
  const int32_t* xref;
  const int32_t* xalt;
  int64_t xn;
  int32_t* elo;              // [xn]
  int32_t* ehi;              // [xn]
  int32_t* esite;            // [xn]
  int32_t* sfirst;           // [xn + 1]
  int32_t* slo;              // [xn] window of every site
  int32_t* shi;              // [xn]
  int32_t* n_sites;          // [2]
  uint8_t* ewhy;             // [xn]
  int32_t gap;
  int32_t pad;
};

// the sites of one VCF and what the pass keeps of it (s.words null: the VCF names no genome, its rows stay zero)
struct HapVcf {
  HapSites s;
  int64_t off;               // the VCF's first record in the batch
  uint32_t* ebits;           // [xn / 32 + 1] the entry is spelled like a kept record with valid codes and no QMF_NOKEY
  uint32_t* sbits;           // [xn / 32 + 1] the site is no TOOLONG one and has an open entry
  uint32_t* srank;           // [xn / 32 + 1] the pairs before the word's first site, over all VCFs (k_hap_rank)
  uint8_t* ecls;             // [xn] class byte per entry, or null
};

struct HapRecParams {
  const SpanDesc* spans;
  const HapVcf* vcfs;        // [n_vcf]
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_tp;
  uint8_t* cls;              // [n_pad] class bytes
  int32_t* site;             // [n_pad] the site of every usable record, -1 for none
  uint64_t* rec;             // [n_vcf][HAP_R_COLS], cleared on the same stream before the first launch
  int32_t* pairs;            // [n_pairs][HAP_PAIR_WORDS] (k_hap_claim)
  int32_t n_spans;
  int32_t pad;
};

struct HapReplayParams {
  const HapVcf* vcfs;
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_tp;
  uint8_t* cls;
  uint64_t* rec;
  uint64_t* tru;             // [n_vcf][HAP_T_COLS]
  const int32_t* pairs;
  int64_t n_pairs;
};

// ---- the subset search behind the pass (k_hap_subsets) ----
constexpr int HAPSUB_COLS = 8;               // include/qmvt.h QM_HAPSUB_COLS
constexpr uint32_t HAP_SUBSET = 14u, HAP_LEFT = 15u;   // QM_HAP_C_SUBSET / _LEFT: in the search's own class arrays only (14 is HAP_PENDING inside the pass)
constexpr int HAPSUB_SEARCHED = 0, HAPSUB_PARTIAL = 1, HAPSUB_NOSUBSET = 2, HAPSUB_TP_S = 3, HAPSUB_RESCUED_S = 4, HAPSUB_FOUND_S = 5,
              HAPSUB_LEFT_LINES = 6, HAPSUB_LEFT_ENTRIES = 7;
// the word of a pair in HapSubParams::res: 0 not searched, HAPSUB_RES_NOSUBSET, or HAPSUB_RES_PARTIAL | S mask << 8 | T mask
constexpr uint32_t HAPSUB_RES_PARTIAL = 1u << 16, HAPSUB_RES_NOSUBSET = 1u << 17;

// What qm_batch_haplotypes left in the batch, read only, and the search's own outputs.
struct HapSubParams {
  const HapVcf* vcfs;
  const int32_t* pos;
  const int32_t* ref;
  const int32_t* alt;
  const uint8_t* flags;
  const uint64_t* mask_tp;
  const uint8_t* cls;        // the pass's class bytes
  const uint8_t* ecls;       // the pass's entry classes (the base every HapVcf::ecls points into), or null
  const uint64_t* rec;       // [n_vcf][HAP_R_COLS]
  const uint64_t* tru;       // [n_vcf][HAP_T_COLS]
  const int32_t* pairs;
  int64_t n_pairs;
  uint64_t* sub;             // [n_vcf][HAPSUB_COLS]
  uint32_t* res;             // [n_pairs], cleared on the same stream before the launch
  uint8_t* cls_s;            // [n_pad] a copy of cls made on the same stream before the launch, or null
  uint8_t* ecls_s;           // as ecls, or null
  int32_t n_vcf;
  int32_t narrow;            // QM_HAPSUB_NARROW_HASH: hashes of 4 bits, the answer rests on the verification alone
};

// k_hap_subsets_init + k_hap_subsets: sub starts from TP_H and FOUND_H, then one wave per pair
void launch_hap_subsets(const HapSubParams& P, hipStream_t st);

// builds S on `st`: per-entry arrays, site indices, windows
void launch_hap_sites(const HapSites& S, hipStream_t st);
// k_hap_records: classes, sites, the counts that need no replay, the found bitmaps
void launch_hap_records(const HapRecParams& P, hipStream_t st);
// k_hap_truth + k_hap_rank: the truth-side counts, the open-site bitmaps, their ranks, and total[0] = the number of pairs
void launch_hap_truth(const HapVcf* vcfs, int n_vcf, int64_t max_entries, uint64_t* tru, unsigned long long* total, hipStream_t st);
// k_hap_pairs: names every pair (VCF, site, count 0); k_hap_claim: LONE lines, and the open lines of every pair
void launch_hap_claim(const HapRecParams& P, int n_vcf, int64_t max_entries, hipStream_t st);
void launch_hap_replay(const HapReplayParams& P, hipStream_t st);

}  // namespace qm
