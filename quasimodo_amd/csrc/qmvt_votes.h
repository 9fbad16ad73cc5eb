// qmvt_votes.h -- the k-of-n consensus pass (qmvt_votes.hip) and its host side (qmvt_api.cpp).  Internal; the public surface is
// include/qmvt.h (qm_batch_votes, qm_batch_get_votes, qm_batch_get_vote_keys).  Kept apart from qmvt_dev.h so that the kernels id
// stays what the profiles of the classification pass are keyed on.
#pragma once
#include "qmvt_dev.h"

namespace qm {

constexpr int VT_MAX_GROUP = 32;         // include/qmvt.h QM_VOTE_GROUP_MAX: VCFs per group
constexpr int VT_SLOTS = VT_MAX_GROUP + 1;   // vote counts 0 .. 32
constexpr int VT_PLANES = 6;             // bit planes of the carry-save counter: 0 .. 63 >= 32
constexpr int VT_RUN_TILE = 1024;        // sorted pairs per workgroup of k_vote_heads / k_vote_runs (4 consecutive per lane)
static_assert(SORT_TILE % VT_RUN_TILE == 0, "a run tile lies inside one sort tile (the sort's tile table names its group)");
constexpr int VT_RUN_PER_SORT = SORT_TILE / VT_RUN_TILE;

// one group of k_vote_truth: n VCFs of one truth set
struct VoteGroup {
  const uint32_t* bits[VT_MAX_GROUP];   // the members' hit bitmaps (qm_batch_truth_hits)
  int64_t words;                        // ceil(tn / 32)
  int64_t tn;                           // T'
  int32_t n;
  int32_t pad;
};

// The per-group outputs, one array each, all u64: tp[g][VT_SLOTS], fp[g][VT_SLOTS], ptp[g][VT_MAX_GROUP], pfp[g][VT_MAX_GROUP],
// nokey[g].  Cleared on the same stream before the launches.
struct VoteOut {
  unsigned long long* tp;
  unsigned long long* fp;
  unsigned long long* ptp;
  unsigned long long* pfp;
  unsigned long long* nokey;
};

struct VoteKeysParams {
  const SpanDesc* spans;
  const int32_t* vcf_slot;      // [n_vcf] group << 8 | member index, or -1: the VCF sits in no group
  const SortSeg* segs;          // [n_groups] the group's segment of the pair buffers: koff = first pair, n = its capacity
  const int32_t* pos;
  const uint8_t* anib;
  const uint8_t* flags;
  const uint64_t* mask_pass;
  const uint64_t* mask_intruth;
  uint32_t* cursor;             // [n_groups] pairs written so far; cleared before the launch
  uint32_t* keys;               // the pair buffers
  uint32_t* vals;
  unsigned long long* nokey;    // [n_groups]
  int32_t n_spans;
};

void launch_vote_truth(const VoteGroup* groups, int n_groups, int64_t max_words, const VoteOut& out, hipStream_t st);
void launch_vote_keys(const VoteKeysParams& P, hipStream_t st);
// segs[g].n = cursor[g] (never above the capacity it held): the sort and the run kernels then see the pairs that were written
void launch_vote_segs(SortSeg* segs, const uint32_t* cursor, int n_groups, hipStream_t st);
// The sorted pairs of every group (keys / vals + segs[g].koff, segs[g].n of them) -> the ascending distinct keys and the OR of
// their member bits at ukeys / umasks + segs[g].koff, ucount[g] of them; fp / pfp of `out` accumulated.  tile_seg: the sort's
// table (group of every sort tile), n_sort_tiles of them; thd: n_sort_tiles * VT_RUN_PER_SORT words of scratch.
void launch_vote_runs(const SortSeg* segs, const int32_t* tile_seg, int n_groups, int n_sort_tiles, const uint32_t* keys, const uint32_t* vals,
                      uint32_t* thd, uint32_t* ukeys, uint32_t* umasks, uint32_t* ucount, const VoteOut& out, hipStream_t st);

}  // namespace qm
