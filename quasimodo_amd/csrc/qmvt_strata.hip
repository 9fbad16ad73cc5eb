// qmvt_strata.hip -- TP, FP and FN counts of a finished batch per genome region (BED strata).  k_strata_records
// streams the class masks and, under the kept bits, pos and flags in input order and counts the kept and the TP lines of every
// VCF per stratum; k_strata_planes turns the stratum masks of a truth set's keys into bit planes over the key index, and
// k_strata_truth counts them against the hit bitmaps of qm_batch_truth_hits.  Its own translation unit: qm_kernels_id
// (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's profiles are keyed on.
#include "qmvt_strata.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// Index of the segment that holds p: upper_bound(bp, p) - 1, for every int32 p (bp[0] = INT32_MIN).  `prev` is the segment the
// lane's previous lookup ended in and is tried first: in a sorted VCF consecutive records almost always share it.  STAGED: bp is
// the workgroup's LDS copy of the whole table; otherwise the coarse index names the cell's segments in global memory.
template <bool STAGED>
__device__ inline int32_t strata_find(const StrataTable& T, const int32_t* bp, int32_t p, int32_t prev) {
  if (bp[prev] <= p && (prev + 1 >= T.m || p < bp[prev + 1])) return prev;
  int32_t lo = 0, hi = T.m;   // the answer lies in [lo, hi), and bp[lo] <= p
  if constexpr (!STAGED) {
    const uint32_t c = ((uint32_t)p ^ 0x80000000u) >> (uint32_t)T.shift;   // (p - INT32_MIN) >> shift
    lo = T.cidx[c];
    hi = T.cidx[c + 1] + 1;
  }
  while (hi - lo > 1) {
    const int32_t mid = (lo + hi) >> 1;
    if (bp[mid] <= p) lo = mid; else hi = mid;
  }
  return lo;
}

template <bool STAGED>
__device__ inline void strata_stage(const StrataTable& T, int32_t* s_bp, uint32_t* s_mask) {
  if constexpr (STAGED) {
    for (int i = threadIdx.x; i < T.m; i += blockDim.x) { s_bp[i] = T.bp[i]; s_mask[i] = T.masks[i]; }
    __syncthreads();
  }
}

// Adds the workgroup's counters to the VCF's rows and clears them.  cnt: [rows][2] u32 in LDS (kept, TP), laid out like the rows.
__device__ inline void strata_flush(uint32_t* cnt, int words, uint64_t* out) {
  __syncthreads();
  if ((int)threadIdx.x < words) {
    const uint32_t v = cnt[threadIdx.x];
    if (v) {
      atomicAdd(reinterpret_cast<unsigned long long*>(out + threadIdx.x), (unsigned long long)v);
      cnt[threadIdx.x] = 0u;
    }
  }
  __syncthreads();
}

// One wave's records of one step, one per lane: `in` = the lane has a counted record, `tp` = it is a TP line, `row` = its rows as
// bits (0 .. 31 the strata, 32 outside, 33 nokey).  Integer adds only, in any order: a ballot and two popcounts per row bit that
// some lane of the wave carries, one lane adds to LDS.  Called by every lane of the wave (uniform control flow).
__device__ inline void strata_count(uint32_t* cnt, bool in, bool tp, uint64_t row, bool first) {
  if constexpr (STRATA_BALLOT) {
    const uint64_t tpb = __ballot(in && tp);
    uint64_t rem = in ? row : 0ull;
    uint64_t any;
    while ((any = __ballot(rem != 0ull)) != 0ull) {
      const int leader = __ffsll((unsigned long long)any) - 1;
      // the leader's rows, known to every lane (two 32-bit broadcasts)
      const uint64_t lead = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(rem >> 32), leader) << 32) | (uint32_t)__shfl((int)(uint32_t)rem, leader);
      uint64_t todo = lead;
      while (todo) {
        const int s = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1ull;
        const uint64_t b = __ballot(((rem >> s) & 1ull) != 0ull);
        if (first) {
          atomicAdd(cnt + 2 * s, (uint32_t)__popcll(b));
          const uint32_t t = (uint32_t)__popcll(b & tpb);
          if (t) atomicAdd(cnt + 2 * s + 1, t);
        }
      }
      rem &= ~lead;
    }
  } else {
    uint64_t todo = in ? row : 0ull;
    while (todo) {
      const int s = __ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1ull;
      atomicAdd(cnt + 2 * s, 1u);
      if (tp) atomicAdd(cnt + 2 * s + 1, 1u);
    }
  }
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads).  Every lane stays
// in the loop for all of a span's steps: the wave's ballots need them together.
template <bool STAGED>
__global__ __launch_bounds__(256) void k_strata_records(StrataRecParams P) {
  __shared__ int32_t s_bp[STAGED ? STRATA_LDS_SEGMENTS : 1];
  __shared__ uint32_t s_mask[STAGED ? STRATA_LDS_SEGMENTS : 1];
  __shared__ uint32_t cnt[2 * STRATA_REC_ROWS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE = 65 536 records: u32 suffices
  const StrataTable T = P.tab;
  const int S = T.n_strata;
  const int words = 2 * (S + 2);
  if ((int)threadIdx.x < 2 * STRATA_REC_ROWS) cnt[threadIdx.x] = 0u;
  strata_stage<STAGED>(T, s_bp, s_mask);
  __syncthreads();
  const int32_t* bp = STAGED ? s_bp : T.bp;
  const uint32_t* masks = STAGED ? s_mask : T.masks;
  const bool first = (threadIdx.x & 63u) == 0u;
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  int32_t seg = 0;
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (cur >= 0) strata_flush(cnt, words, P.out + (int64_t)cur * words);
      cur = sd.vcf;
    }
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 4 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 4 * (int64_t)threadIdx.x;
      uint32_t kb = 0u, tb = 0u;
      if (g < sd.end) {
        const int sh = (int)(g & 63);
        kb = (uint32_t)(P.mask_pass[g >> 6] >> sh) & 15u;
        if (sd.end - g < 4) kb &= (1u << (uint32_t)(sd.end - g)) - 1u;   // bits past the VCF's last record are not defined
      }
      if (!__ballot(kb != 0u)) continue;   // (uniform over the wave)
      uint64_t row[4] = {0ull, 0ull, 0ull, 0ull};
      if (kb) {
        tb = (uint32_t)(P.mask_tp[g >> 6] >> (int)(g & 63)) & 15u;
        const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((kb >> k) & 1u)) continue;
          if ((f4 >> (8 * k)) & QMF_NOKEY) { row[k] = 1ull << (S + 1); continue; }   // its pos column is not consulted
          seg = strata_find<STAGED>(T, bp, p4[k], seg);
          const uint32_t m = masks[seg];
          row[k] = m ? (uint64_t)m : 1ull << S;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) strata_count(cnt, (kb >> k) & 1u, (tb >> k) & 1u, row[k], first);
    }
  }
  if (cur >= 0) strata_flush(cnt, words, P.out + (int64_t)cur * words);
}

// A lane per key, STRATA_PLANE_KEYS keys per workgroup; a wave's 64 keys are two words of every plane, written by two lanes.
template <bool STAGED>
__global__ __launch_bounds__(256) void k_strata_planes(StrataTable T, const uint32_t* keys, int64_t n, uint32_t* planes) {
  __shared__ int32_t s_bp[STAGED ? STRATA_LDS_SEGMENTS : 1];
  __shared__ uint32_t s_mask[STAGED ? STRATA_LDS_SEGMENTS : 1];
  strata_stage<STAGED>(T, s_bp, s_mask);
  const int32_t* bp = STAGED ? s_bp : T.bp;
  const uint32_t* masks = STAGED ? s_mask : T.masks;
  const int S = T.n_strata;
  const int64_t words = (n + 31) >> 5;
  const int lane = (int)(threadIdx.x & 63u);
  int32_t seg = 0;
  const int64_t j0 = (int64_t)blockIdx.x * STRATA_PLANE_KEYS;
  for (int64_t jb = j0; jb < min(j0 + (int64_t)STRATA_PLANE_KEYS, n); jb += blockDim.x) {   // (uniform over the workgroup)
    const int64_t j = jb + threadIdx.x;
    uint32_t m = 0u;
    const bool have = j < n;
    if (have) {
      seg = strata_find<STAGED>(T, bp, (int32_t)(keys[j] >> 4), seg);
      m = masks[seg];
    }
    const int64_t w = (j - lane) >> 5;   // the wave's first word
    for (int s = 0; s <= S; ++s) {
      const uint64_t b = __ballot(have && (s < S ? ((m >> s) & 1u) != 0u : m == 0u));
      if (lane < 2 && w + lane < words) planes[(int64_t)s * words + w + lane] = (uint32_t)(b >> (32 * lane));
    }
  }
}

// grid (x, vcf): out[vcf][s] += (truth keys in row s, those of them the VCF hit), 32 keys per word
__global__ __launch_bounds__(256) void k_strata_truth(const StrataTruthRow* rows, int n_strata, unsigned long long* out) {
  __shared__ uint32_t cnt[2 * (STRATA_MAX + 1)];
  if ((int)threadIdx.x < 2 * (STRATA_MAX + 1)) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const StrataTruthRow R = rows[blockIdx.y];
  for (int s = 0; s <= n_strata; ++s) {
    const uint32_t* plane = R.planes + (int64_t)s * R.words;
    uint32_t c0 = 0u, c1 = 0u;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < R.words; w += (int64_t)gridDim.x * blockDim.x) {
      const uint32_t x = plane[w];
      c0 += (uint32_t)__popc(x);
      c1 += (uint32_t)__popc(x & R.hits[w]);
    }
    if (c0) atomicAdd(cnt + 2 * s, c0);
    if (c1) atomicAdd(cnt + 2 * s + 1, c1);
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 * (n_strata + 1) && cnt[threadIdx.x])
    atomicAdd(out + (int64_t)blockIdx.y * 2 * (n_strata + 1) + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

void launch_strata_records(const StrataRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  if (P.tab.m <= STRATA_LDS_SEGMENTS) hipLaunchKernelGGL(k_strata_records<true>, grid, dim3(256), 0, st, P);
  else hipLaunchKernelGGL(k_strata_records<false>, grid, dim3(256), 0, st, P);
}

void launch_strata_planes(const StrataTable& tab, const uint32_t* keys, int64_t n, uint32_t* planes, hipStream_t st) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + STRATA_PLANE_KEYS - 1) / STRATA_PLANE_KEYS));
  if (tab.m <= STRATA_LDS_SEGMENTS) hipLaunchKernelGGL(k_strata_planes<true>, grid, dim3(256), 0, st, tab, keys, n, planes);
  else hipLaunchKernelGGL(k_strata_planes<false>, grid, dim3(256), 0, st, tab, keys, n, planes);
}

void launch_strata_truth(const StrataTruthRow* rows, int n_vcf, int64_t max_words, int n_strata, unsigned long long* out, hipStream_t st) {
  if (n_vcf <= 0 || max_words <= 0) return;
  const int64_t bx = std::min<int64_t>(64, std::max<int64_t>(1, (max_words + 255) / 256));
  for (int v0 = 0; v0 < n_vcf; v0 += 65535)   // (the grid's y extent)
    hipLaunchKernelGGL(k_strata_truth, dim3((unsigned)bx, (unsigned)std::min(65535, n_vcf - v0)), dim3(256), 0, st, rows + v0, n_strata,
                       out + (int64_t)v0 * 2 * (n_strata + 1));
}

}  // namespace qm
