// qmvt_votes.hip -- k-of-n caller consensus over a finished batch: for groups of up to 32 VCFs of one truth set,
// how many members call every key.  k_vote_truth counts the votes of the truth keys from the hit bitmaps of qm_batch_truth_hits
// (a bit-sliced carry-save counter over 32 keys per word); k_vote_keys compacts the members' kept records outside the truth set
// into (key, member) pairs, the radix passes of qmvt_kernels.hip sort every group's pairs, and k_vote_heads / k_vote_scan /
// k_vote_runs turn the sorted pairs into the ascending distinct keys, their member masks and the vote histogram.  Its own
// translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's profiles are keyed on.
#include "qmvt_votes.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

__device__ __forceinline__ uint32_t vt_lanes_below(uint64_t b) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}

// Adds the workgroup's LDS counters to the group's rows: one 64-bit atomic per non-zero slot.  hist: VT_SLOTS counters, priv:
// VT_MAX_GROUP counters; lanes 0 .. 32 take the histogram, lanes 64 .. 95 the private counts.  Called behind a barrier.
__device__ inline void vote_flush(const uint32_t* hist, const uint32_t* priv, unsigned long long* out_hist, unsigned long long* out_priv) {
  const int t = (int)threadIdx.x;
  if (t < VT_SLOTS) {
    if (hist[t]) atomicAdd(out_hist + t, (unsigned long long)hist[t]);
  } else if (t >= 64 && t < 64 + VT_MAX_GROUP) {
    if (priv[t - 64]) atomicAdd(out_priv + (t - 64), (unsigned long long)priv[t - 64]);
  }
}

// grid (x, group): tp[group][c] += truth keys with exactly c votes, ptp[group][i] += keys only member i hit; 32 keys per word.
// The votes of a word's 32 keys are six bit planes (plane j = bit j of every key's count); a member's word is added with a
// ripple of half adders, and the keys with exactly c votes are the AND of the planes or their complements.
__global__ __launch_bounds__(256) void k_vote_truth(const VoteGroup* groups, VoteOut out) {
  __shared__ uint32_t s_hist[VT_SLOTS];
  __shared__ uint32_t s_priv[VT_MAX_GROUP];
  if (threadIdx.x < VT_SLOTS) s_hist[threadIdx.x] = 0u;
  if (threadIdx.x < VT_MAX_GROUP) s_priv[threadIdx.x] = 0u;
  __syncthreads();
  const VoteGroup& G = groups[blockIdx.y];
  const int n = G.n;
  const int64_t words = G.words, tn = G.tn;
  uint32_t acc[VT_SLOTS];
#pragma unroll
  for (int c = 0; c < VT_SLOTS; ++c) acc[c] = 0u;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t p[VT_PLANES];
#pragma unroll
    for (int j = 0; j < VT_PLANES; ++j) p[j] = 0u;
    for (int i = 0; i < n; ++i) {
      uint32_t carry = G.bits[i][w];
#pragma unroll
      for (int j = 0; j < VT_PLANES; ++j) {
        const uint32_t t = p[j] & carry;
        p[j] ^= carry;
        carry = t;
      }
    }
    const uint32_t valid = (w == words - 1 && (tn & 31)) ? (1u << (uint32_t)(tn & 31)) - 1u : 0xffffffffu;
#pragma unroll
    for (int c = 0; c < VT_SLOTS; ++c) {
      if (c <= n) {   // (uniform)
        uint32_t a = valid;
#pragma unroll
        for (int j = 0; j < VT_PLANES; ++j) a &= ((c >> j) & 1) ? p[j] : ~p[j];
        acc[c] += (uint32_t)__popc(a);
      }
    }
    const uint32_t one = valid & p[0] & ~(p[1] | p[2] | p[3] | p[4] | p[5]);
    if (one) {
      for (int i = 0; i < n; ++i) {
        const uint32_t x = G.bits[i][w] & one;
        if (x) atomicAdd(s_priv + i, (uint32_t)__popc(x));
      }
    }
  }
#pragma unroll
  for (int c = 0; c < VT_SLOTS; ++c)
    if (acc[c]) atomicAdd(s_hist + c, acc[c]);
  __syncthreads();
  vote_flush(s_hist, s_priv, out.tp + (int64_t)blockIdx.y * VT_SLOTS, out.ptp + (int64_t)blockIdx.y * VT_MAX_GROUP);
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads, one nibble of the
// masks per lane).  The records with kept, not in the truth set and a comparable key leave as (key, member) pairs: four ballots
// say where a lane's pairs go inside the wave's piece, and lane 0 reserves the piece with one atomic on the group's cursor.
__global__ __launch_bounds__(256) void k_vote_keys(VoteKeysParams P) {
  const int lane = (int)(threadIdx.x & 63u);
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    const int32_t slot = P.vcf_slot[sd.vcf];
    if (slot < 0) continue;   // (uniform over the workgroup)
    const int grp = slot >> 8;
    const uint32_t member = (uint32_t)(slot & 255);
    const int64_t koff = P.segs[grp].koff;
    const uint32_t cap = (uint32_t)P.segs[grp].n;
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 4 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 4 * (int64_t)threadIdx.x;
      uint32_t kb = 0u;
      if (g < sd.end) {
        kb = (uint32_t)(P.mask_pass[g >> 6] >> (int)(g & 63)) & 15u;
        if (sd.end - g < 4) kb &= (1u << (uint32_t)(sd.end - g)) - 1u;   // bits past the VCF's last record are not defined
      }
      if (!__ballot(kb != 0u)) continue;   // (uniform over the wave; no workgroup barrier inside this loop)
      uint32_t sel = 0u, nk = 0u, key[4] = {0u, 0u, 0u, 0u};
      if (kb) {
        const uint32_t it = (uint32_t)(P.mask_intruth[g >> 6] >> (int)(g & 63)) & 15u;
        const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
        const uint32_t a4 = *reinterpret_cast<const uint32_t*>(P.anib + g);
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((kb >> k) & 1u)) continue;
          const uint32_t ab = (a4 >> (8 * k)) & 0xffu;
          if ((f4 >> (8 * k)) & QMF_NOKEY) { nk |= 1u << k; continue; }
          if (((it >> k) & 1u) || (ab & ANIB_NONE)) continue;
          sel |= 1u << k;
          key[k] = ((uint32_t)p4[k] << 4) | ab;
        }
      }
      uint64_t b[4];
      uint32_t before[4], total = 0u, nnk = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        b[k] = __ballot(((sel >> k) & 1u) != 0u);
        before[k] = total;
        total += (uint32_t)__popcll(b[k]);
        nnk += (uint32_t)__popcll(__ballot(((nk >> k) & 1u) != 0u));
      }
      if (nnk && lane == 0) atomicAdd(P.nokey + grp, (unsigned long long)nnk);
      if (!total) continue;
      uint32_t base = 0u;
      if (lane == 0) base = atomicAdd(P.cursor + grp, total);
      base = (uint32_t)__shfl((int)base, 0);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!((sel >> k) & 1u)) continue;
        const uint32_t at = base + before[k] + vt_lanes_below(b[k]);
        if (at < cap) {   // the host sized the segment by the members' kept lines: always
          P.keys[koff + at] = key[k];
          P.vals[koff + at] = member;
        }
      }
    }
  }
}

__global__ void k_vote_segs(SortSeg* segs, const uint32_t* cursor, int n_groups) {
  const int g = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (g >= n_groups) return;
  const int64_t c = (int64_t)cursor[g];
  if (c < segs[g].n) segs[g].n = c;
}

// A lane's four consecutive sorted pairs of run tile `t` of its group.  head[k]: pair k starts a run of equal keys.
struct VoteLane {
  uint32_t key[4], bit[4];
  bool valid[4], head[4];
};
__device__ inline VoteLane vote_load(const uint32_t* keys, const uint32_t* vals, int64_t koff, int64_t n, int64_t i, bool want_bits) {
  VoteLane L;
#pragma unroll
  for (int k = 0; k < 4; ++k) { L.key[k] = 0u; L.bit[k] = 0u; L.valid[k] = false; L.head[k] = false; }
  if (i >= n) return L;
  // koff is a multiple of 64 and i of 4, the buffers are padded: whole 16-byte loads, the tail masked
  const qm_uint4 k4 = *reinterpret_cast<const qm_uint4*>(keys + koff + i);
  qm_uint4 v4 = {0u, 0u, 0u, 0u};
  if (want_bits) v4 = *reinterpret_cast<const qm_uint4*>(vals + koff + i);
  uint32_t prev = i > 0 ? keys[koff + i - 1] : 0u;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    L.valid[k] = i + k < n;
    L.key[k] = k4[k];
    L.bit[k] = L.valid[k] ? 1u << (v4[k] & 31u) : 0u;
    L.head[k] = L.valid[k] && (i + k == 0 || k4[k] != prev);
    prev = k4[k];
  }
  return L;
}

// The group and the place of run tile `t` (numbered over all groups, VT_RUN_PER_SORT per sort tile)
__device__ inline SortSeg vote_tile(const SortSeg* segs, const int32_t* tile_seg, int t, int* grp, int64_t* base) {
  *grp = tile_seg[t / VT_RUN_PER_SORT];
  const SortSeg sg = segs[*grp];
  *base = ((int64_t)t - (int64_t)sg.tile0 * VT_RUN_PER_SORT) * VT_RUN_TILE;
  return sg;
}

// thd[t] = runs that start in run tile t
__global__ __launch_bounds__(256) void k_vote_heads(const SortSeg* segs, const int32_t* tile_seg, const uint32_t* keys, uint32_t* thd) {
  __shared__ uint32_t s_n;
  int grp;
  int64_t base;
  const SortSeg sg = vote_tile(segs, tile_seg, (int)blockIdx.x, &grp, &base);
  if (threadIdx.x == 0) s_n = 0u;
  __syncthreads();
  const VoteLane L = vote_load(keys, nullptr, sg.koff, sg.n, base + 4 * (int64_t)threadIdx.x, false);
  uint32_t c = (uint32_t)L.head[0] + (uint32_t)L.head[1] + (uint32_t)L.head[2] + (uint32_t)L.head[3];
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  if ((threadIdx.x & 63u) == 0u && c) atomicAdd(&s_n, c);
  __syncthreads();
  if (threadIdx.x == 0) thd[blockIdx.x] = s_n;
}

// One workgroup per group: thd of the group's run tiles -> exclusive prefix sums; ucount[group] = the sum, its distinct keys
__global__ __launch_bounds__(256) void k_vote_scan(const SortSeg* segs, uint32_t* thd, uint32_t* ucount) {
  __shared__ uint32_t s_wave[4];
  const SortSeg sg = segs[blockIdx.x];
  uint32_t* h = thd + (int64_t)sg.tile0 * VT_RUN_PER_SORT;
  const int64_t total = (int64_t)sg.ntiles * VT_RUN_PER_SORT;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  uint32_t carry = 0u;
  for (int64_t b0 = 0; b0 < total; b0 += 256) {   // (uniform over the workgroup)
    const int64_t i = b0 + threadIdx.x;
    const uint32_t x = i < total ? h[i] : 0u;
    uint32_t incl = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, o);
      if (lane >= o) incl += y;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t woff = 0u, btot = 0u;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const uint32_t t = s_wave[w]; woff += w < wave ? t : 0u; btot += t; }
    if (i < total) h[i] = carry + woff + incl - x;
    carry += btot;
    __syncthreads();
  }
  if (threadIdx.x == 0) ucount[blockIdx.x] = carry;
}

// One workgroup per run tile.  A run belongs to the tile its head lies in.  Inside the tile a segmented OR-scan (four pairs per
// lane in registers, shuffles inside the wave, one LDS hop across the four waves) gives every pair the OR of its run's member
// bits up to itself and the rank of its run among the tile's heads; the pair that ends a run writes it.  Pairs in front of the
// tile's first head continue a run of an earlier tile and are left to that tile.  Hand-over: a run that is still open at the
// tile's last pair is finished by the whole workgroup, which reads on past the tile 256 pairs at a time until the key changes or
// the group's pairs end.  Only ORs and integer adds: the result does not depend on the order of equal keys.
__global__ __launch_bounds__(256) void k_vote_runs(const SortSeg* segs, const int32_t* tile_seg, const uint32_t* keys, const uint32_t* vals,
                                                   const uint32_t* thd, uint32_t* ukeys, uint32_t* umasks, VoteOut out) {
  __shared__ uint32_t s_hist[VT_SLOTS];
  __shared__ uint32_t s_priv[VT_MAX_GROUP];
  __shared__ uint32_t s_wf[4], s_wv[4], s_wc[4];
  __shared__ uint32_t s_open[4];   // the open run: flag, key, rank, mask
  int grp;
  int64_t base;
  const SortSeg sg = vote_tile(segs, tile_seg, (int)blockIdx.x, &grp, &base);
  if (base >= sg.n) return;   // (uniform) a tile past the pairs that were written
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < VT_SLOTS) s_hist[tid] = 0u;
  if (tid < VT_MAX_GROUP) s_priv[tid] = 0u;
  if (tid < 4) s_open[tid] = 0u;
  const int64_t n = sg.n, koff = sg.koff;
  const int64_t i = base + 4 * (int64_t)tid;
  const VoteLane L = vote_load(keys, vals, koff, n, i, true);
  // inside the lane: the OR since the lane's latest head (or since its first pair), heads so far
  uint32_t loc[4], hc[4];
  loc[0] = L.bit[0];
  hc[0] = (uint32_t)L.head[0];
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    loc[k] = L.head[k] ? L.bit[k] : loc[k - 1] | L.bit[k];
    hc[k] = hc[k - 1] + (uint32_t)L.head[k];
  }
  // across the lanes of the wave: inclusive scan of (has a head, OR since the latest head), and of the head counts
  uint32_t f = hc[3] ? 1u : 0u, v = loc[3], cnt = hc[3];
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t fa = (uint32_t)__shfl_up((int)f, o), va = (uint32_t)__shfl_up((int)v, o), ca = (uint32_t)__shfl_up((int)cnt, o);
    if (lane >= o) {
      if (!f) v |= va;
      f |= fa;
      cnt += ca;
    }
  }
  if (lane == 63) { s_wf[wave] = f; s_wv[wave] = v; s_wc[wave] = cnt; }
  // what the lanes in front of this one in its wave leave open
  uint32_t ef = (uint32_t)__shfl_up((int)f, 1), ev = (uint32_t)__shfl_up((int)v, 1), ec = (uint32_t)__shfl_up((int)cnt, 1);
  if (lane == 0) { ef = 0u; ev = 0u; ec = 0u; }
  __syncthreads();
  uint32_t cf = 0u, cv = 0u, cc = 0u;   // ... and the waves in front of this one
  for (int w = 0; w < wave; ++w) {
    cv = s_wf[w] ? s_wv[w] : cv | s_wv[w];
    cf |= s_wf[w];
    cc += s_wc[w];
  }
  const uint32_t carry = ef ? ev : cv | ev;   // OR of the open run in front of this lane (inside the tile)
  const bool head_before = (cf | ef) != 0u;    // some head of the tile lies in front of this lane
  const uint32_t rank0 = cc + ec;              // heads of the tile in front of this lane
  const uint32_t next = (i + 4 < n) ? keys[koff + i + 4] : 0u;
  const uint32_t uoff = thd[blockIdx.x];       // distinct keys of the group in front of this tile
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!L.valid[k]) continue;
    const bool owned = head_before || hc[k] != 0u;     // the run's head lies in this tile
    if (!owned) continue;
    const uint32_t m = hc[k] ? loc[k] : loc[k] | carry;
    const uint32_t rank = rank0 + hc[k] - 1u;
    const bool last_pair = i + k == n - 1;
    const uint32_t nk = k < 3 ? L.key[k + 1] : next;
    const bool tail = last_pair || ((k < 3 ? L.valid[k + 1] : true) && nk != L.key[k]);
    if (tail) {
      ukeys[koff + uoff + rank] = L.key[k];
      umasks[koff + uoff + rank] = m;
      const int c = __popc(m);
      atomicAdd(s_hist + c, 1u);
      if (c == 1) atomicAdd(s_priv + (__ffs((int)m) - 1), 1u);
    } else if (tid == 255 && k == 3) {   // the tile's last pair, and its run goes on behind the tile
      s_open[0] = 1u; s_open[1] = L.key[k]; s_open[2] = rank; s_open[3] = m;
    }
  }
  __syncthreads();
  if (s_open[0]) {   // (uniform)
    const uint32_t K = s_open[1];
    uint32_t acc = 0u;
    for (int64_t j = base + VT_RUN_TILE + tid;; j += 256) {
      const bool mt = j < n && keys[koff + j] == K;
      if (mt) acc |= 1u << (vals[koff + j] & 31u);
      if (__syncthreads_or(!mt)) break;   // sorted: the pairs with the run's key are a prefix of what lies behind the tile
    }
    for (int o = 32; o > 0; o >>= 1) acc |= (uint32_t)__shfl_xor((int)acc, o);
    if (lane == 0 && acc) atomicOr(&s_open[3], acc);
    __syncthreads();
    if (tid == 0) {
      const uint32_t m = s_open[3];
      ukeys[koff + uoff + s_open[2]] = K;
      umasks[koff + uoff + s_open[2]] = m;
      const int c = __popc(m);
      s_hist[c] += 1u;
      if (c == 1) s_priv[__ffs((int)m) - 1] += 1u;
    }
    __syncthreads();
  }
  vote_flush(s_hist, s_priv, out.fp + (int64_t)grp * VT_SLOTS, out.pfp + (int64_t)grp * VT_MAX_GROUP);
}

void launch_vote_truth(const VoteGroup* groups, int n_groups, int64_t max_words, const VoteOut& out, hipStream_t st) {
  if (n_groups <= 0 || max_words <= 0) return;
  const int64_t bx = std::min<int64_t>(64, std::max<int64_t>(1, (max_words + 255) / 256));
  for (int g0 = 0; g0 < n_groups; g0 += 65535) {   // (the grid's y extent)
    VoteOut o = out;
    o.tp += (int64_t)g0 * VT_SLOTS;
    o.ptp += (int64_t)g0 * VT_MAX_GROUP;
    hipLaunchKernelGGL(k_vote_truth, dim3((unsigned)bx, (unsigned)std::min(65535, n_groups - g0)), dim3(256), 0, st, groups + g0, o);
  }
}

void launch_vote_keys(const VoteKeysParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_vote_keys, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_vote_segs(SortSeg* segs, const uint32_t* cursor, int n_groups, hipStream_t st) {
  if (n_groups <= 0) return;
  hipLaunchKernelGGL(k_vote_segs, dim3((unsigned)((n_groups + 255) / 256)), dim3(256), 0, st, segs, cursor, n_groups);
}

void launch_vote_runs(const SortSeg* segs, const int32_t* tile_seg, int n_groups, int n_sort_tiles, const uint32_t* keys, const uint32_t* vals,
                      uint32_t* thd, uint32_t* ukeys, uint32_t* umasks, uint32_t* ucount, const VoteOut& out, hipStream_t st) {
  if (n_groups <= 0) return;
  const unsigned nt = (unsigned)n_sort_tiles * VT_RUN_PER_SORT;
  if (nt) hipLaunchKernelGGL(k_vote_heads, dim3(nt), dim3(256), 0, st, segs, tile_seg, keys, thd);
  hipLaunchKernelGGL(k_vote_scan, dim3((unsigned)n_groups), dim3(256), 0, st, segs, thd, ucount);
  if (nt) hipLaunchKernelGGL(k_vote_runs, dim3(nt), dim3(256), 0, st, segs, tile_seg, keys, vals, thd, ukeys, umasks, out);
}

}  // namespace qm
