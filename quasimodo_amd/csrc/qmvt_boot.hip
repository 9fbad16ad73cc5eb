// qmvt_boot.hip -- paired block-bootstrap replicates of a finished batch's counts.  k_boot_records streams the
// class masks and, under the kept bits, pos and flags in input order and counts the kept and the TP lines of every VCF per genome
// window; k_boot_truth places the sorted keys of a truth set and the hit ones into the same windows; k_boot_resample draws the
// window multiplicities of a replicate from a counter-based hash (the same draws for every VCF) and forms the replicate's four
// sums per VCF.  Integers only.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the
// classification pass's profiles are keyed on.
#include "qmvt_boot.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

typedef unsigned long long bt_u64x2 __attribute__((ext_vector_type(2)));

// Adds the workgroup's counters to the VCF's rows and clears them.  c: [n_win + 2][2] u32 in LDS (kept, TP); out: the VCF's
// [n_win + 2][BOOT_COLS] rows.  Non-zero cells only.
__device__ inline void boot_flush(uint32_t* c, int words, uint64_t* out) {
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += blockDim.x) {
    const uint32_t v = c[i];
    if (v) {
      atomicAdd(reinterpret_cast<unsigned long long*>(out + (int64_t)(i >> 1) * BOOT_COLS + (i & 1)), (unsigned long long)v);
      c[i] = 0u;
    }
  }
  __syncthreads();
}

// One wave's records of one step, one per lane: `in` = the lane has a counted record, `tp` = it is a TP line, `row` = its row.
// A sorted VCF puts the whole wave on one row: the lanes that share the first pending lane's row are balloted and added as two
// popcounts by one lane; what is left (a window edge inside the wave, a shuffled VCF) goes to LDS one atomic each, to rows that
// mostly differ.  Called by every lane of the wave (uniform control flow).
__device__ inline void boot_count(uint32_t* c, bool in, bool tp, int32_t row, bool first) {
  if constexpr (BOOT_BALLOT) {
    const uint64_t act = __ballot(in);
    if (!act) return;   // (uniform over the wave)
    const int32_t lead = __shfl(row, __ffsll((unsigned long long)act) - 1);
    const bool same = in && row == lead;
    const uint64_t b = __ballot(same);
    const uint64_t tb = __ballot(same && tp);
    if (first) {
      atomicAdd(c + 2 * lead, (uint32_t)__popcll(b));
      if (tb) atomicAdd(c + 2 * lead + 1, (uint32_t)__popcll(tb));
    }
    in = in && !same;
  }
  if (in) {
    atomicAdd(c + 2 * row, 1u);
    if (tp) atomicAdd(c + 2 * row + 1, 1u);
  }
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads).  Every lane stays
// in the loop for all of a span's steps: the wave's ballots need them together.
__global__ __launch_bounds__(256) void k_boot_records(BootRecParams P) {
  extern __shared__ uint32_t boot_c[];   // [n_win + 2][2]: at most PASS_SPANS * SPAN_TILES * K1_TILE = 65 536 records, u32 suffices
  const int32_t nw = P.n_win;
  const int words = 2 * (nw + 2);
  for (int i = threadIdx.x; i < words; i += blockDim.x) boot_c[i] = 0u;
  __syncthreads();
  const bool first = (threadIdx.x & 63u) == 0u;
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (cur >= 0) boot_flush(boot_c, words, P.cnt + (int64_t)cur * (nw + 2) * BOOT_COLS);
      cur = sd.vcf;
    }
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 4 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 4 * (int64_t)threadIdx.x;
      uint32_t kb = 0u, tb = 0u;
      if (g < sd.end) {
        kb = (uint32_t)(P.mask_pass[g >> 6] >> (int)(g & 63)) & 15u;
        if (sd.end - g < 4) kb &= (1u << (uint32_t)(sd.end - g)) - 1u;   // bits past the VCF's last record are not defined
      }
      if (!__ballot(kb != 0u)) continue;   // (uniform over the wave)
      int32_t row[4] = {0, 0, 0, 0};
      if (kb) {
        tb = (uint32_t)(P.mask_tp[g >> 6] >> (int)(g & 63)) & 15u;
        const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if ((f4 >> (8 * k)) & QMF_NOKEY) { row[k] = nw + 1; continue; }   // its pos column is not consulted
          const uint32_t n = (uint32_t)p4[k] - 1u;
          // (pos - 1) / window: the reciprocal is exact below 2^28 (qmvt_afprofile.h); a position beyond is divided the long way
          const uint32_t w = n < (1u << AFP_POS_BITS) ? (uint32_t)(((uint64_t)n * P.div.mul) >> P.div.shift) : n / (uint32_t)P.window;
          row[k] = (p4[k] >= 1 && w < (uint32_t)nw) ? (int32_t)w : nw;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) boot_count(boot_c, (kb >> k) & 1u, (tb >> k) & 1u, row[k], first);
    }
  }
  if (cur >= 0) boot_flush(boot_c, words, P.cnt + (int64_t)cur * (nw + 2) * BOOT_COLS);
}

// The first index whose key lies at position p or beyond: lower_bound(keys, p << 4).  Keys hold positions below 2^28.
__device__ inline int64_t boot_edge(const BootTruthRow& R, int64_t p) {
  if (p >= ((int64_t)1 << AFP_POS_BITS)) return R.n;
  const uint32_t k = (uint32_t)p << 4;
  int64_t lo = 0, hi = R.n;   // the answer lies in [lo, hi]
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (R.keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the set bits of hits[lo .. hi), lo < hi
__device__ inline uint64_t boot_popc(const uint32_t* hits, int64_t lo, int64_t hi) {
  const int64_t wl = lo >> 5, wh = (hi - 1) >> 5;
  uint64_t c = 0ull;
  for (int64_t w = wl; w <= wh; ++w) {
    uint32_t x = hits[w];
    if (w == wl) x &= ~0u << (uint32_t)(lo & 31);
    if (w == wh && (hi & 31)) x &= (1u << (uint32_t)(hi & 31)) - 1u;
    c += (uint64_t)__popc(x);
  }
  return c;
}

// grid (ceil(n_win / 256), vcf), a lane per window: the keys are sorted, so a window's keys are the index range between the
// bisected edges of the window, and the hit ones are the popcount of that range of the bitmap.  Every (VCF, window) cell has one
// writer: plain stores.  `outside` is the keys at position 0 and those behind the last window, added by two lanes of block x = 0.
__global__ __launch_bounds__(256) void k_boot_truth(const BootTruthRow* rows, int32_t window, int32_t n_win, uint64_t* cnt) {
  __shared__ int64_t s_edge[257];
  const BootTruthRow R = rows[blockIdx.y];
  const int w0 = (int)blockIdx.x * 256;
  for (int i = threadIdx.x; i < 257; i += blockDim.x) s_edge[i] = boot_edge(R, (int64_t)min(w0 + i, n_win) * window + 1);
  __syncthreads();
  uint64_t* out = cnt + (int64_t)blockIdx.y * (n_win + 2) * BOOT_COLS;
  const int w = w0 + (int)threadIdx.x;
  if (w < n_win) {
    const int64_t lo = s_edge[threadIdx.x], hi = s_edge[threadIdx.x + 1];
    if (hi > lo) {
      out[(int64_t)w * BOOT_COLS + 2] = (uint64_t)(hi - lo);
      out[(int64_t)w * BOOT_COLS + 3] = boot_popc(R.hits, lo, hi);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 2) {
    const int64_t lo = threadIdx.x == 0 ? 0 : boot_edge(R, (int64_t)n_win * window + 1);
    const int64_t hi = threadIdx.x == 0 ? s_edge[0] : R.n;
    if (hi > lo) {
      atomicAdd(reinterpret_cast<unsigned long long*>(out + (int64_t)n_win * BOOT_COLS + 2), (unsigned long long)(hi - lo));
      atomicAdd(reinterpret_cast<unsigned long long*>(out + (int64_t)n_win * BOOT_COLS + 3), (unsigned long long)boot_popc(R.hits, lo, hi));
    }
  }
}

// grid (replicate, VCF share): the workgroup builds the replicate's multiplicities in LDS from the hash, then each wave takes
// VCFs: lanes stride over the windows, four 64-bit sums per lane, reduced across the wave; lane 0 adds the two rows that are not
// resampled and stores.  cnt is read once per replicate with plain loads, so that the caches keep what they can of it: it fits
// the L2 only for small batches (n_vcf * (n_win + 2) * 32 B: 0.8 GB at 6 250 VCFs x 4096 windows, beyond the L2 and only partly
// inside the Infinity Cache).
__global__ __launch_bounds__(256) void k_boot_resample(const uint64_t* cnt, int n_vcf, int32_t n_win, uint64_t seed, uint64_t* rep) {
  extern __shared__ uint32_t boot_m[];   // [n_win]
  const uint32_t b = blockIdx.x;
  const int64_t n_rep = gridDim.x;
  for (int i = threadIdx.x; i < n_win; i += blockDim.x) boot_m[i] = 0u;
  __syncthreads();
  for (int j = threadIdx.x; j < n_win; j += blockDim.x) atomicAdd(boot_m + boot_draw(seed, b, (uint32_t)j, (uint32_t)n_win), 1u);
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  const int waves = (int)(blockDim.x >> 6);
  for (int v = (int)blockIdx.y * waves + (int)(threadIdx.x >> 6); v < n_vcf; v += (int)gridDim.y * waves) {   // (uniform over the wave)
    const uint64_t* C = cnt + (int64_t)v * (n_win + 2) * BOOT_COLS;
    unsigned long long a0 = 0ull, a1 = 0ull, a2 = 0ull, a3 = 0ull;
    for (int w = lane; w < n_win; w += 64) {
      const unsigned long long m = boot_m[w];
      const bt_u64x2 x = *reinterpret_cast<const bt_u64x2*>(C + (int64_t)w * BOOT_COLS);
      const bt_u64x2 y = *reinterpret_cast<const bt_u64x2*>(C + (int64_t)w * BOOT_COLS + 2);
      a0 += m * x[0]; a1 += m * x[1]; a2 += m * y[0]; a3 += m * y[1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      a0 += __shfl_xor(a0, off); a1 += __shfl_xor(a1, off); a2 += __shfl_xor(a2, off); a3 += __shfl_xor(a3, off);
    }
    if (lane == 0) {
      const uint64_t* F = C + (int64_t)n_win * BOOT_COLS;   // outside, nokey: in every replicate once
      uint64_t* out = rep + ((int64_t)v * n_rep + b) * BOOT_COLS;
      out[0] = a0 + F[0] + F[4]; out[1] = a1 + F[1] + F[5]; out[2] = a2 + F[2] + F[6]; out[3] = a3 + F[3] + F[7];
    }
  }
}

void launch_boot_records(const BootRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  hipLaunchKernelGGL(k_boot_records, grid, dim3(256), (size_t)2 * (size_t)(P.n_win + 2) * sizeof(uint32_t), st, P);
}

void launch_boot_truth(const BootTruthRow* rows, int n_vcf, int32_t window, int32_t n_win, uint64_t* cnt, hipStream_t st) {
  const unsigned bx = (unsigned)((n_win + 255) / 256);
  for (int v0 = 0; v0 < n_vcf; v0 += 65535)   // (the grid's y extent)
    hipLaunchKernelGGL(k_boot_truth, dim3(bx, (unsigned)std::min(65535, n_vcf - v0)), dim3(256), 0, st, rows + v0, window, n_win,
                       cnt + (int64_t)v0 * (n_win + 2) * BOOT_COLS);
}

void launch_boot_resample(const uint64_t* cnt, int n_vcf, int32_t n_win, int32_t n_rep, uint64_t seed, uint64_t* rep, hipStream_t st) {
  if (n_vcf <= 0 || n_rep <= 0) return;
  const unsigned by = (unsigned)std::min(BOOT_VCF_SPLIT, (n_vcf + 3) / 4);
  hipLaunchKernelGGL(k_boot_resample, dim3((unsigned)n_rep, by), dim3(256), (size_t)n_win * sizeof(uint32_t), st, cnt, n_vcf, n_win, seed, rep);
}

}  // namespace qm
