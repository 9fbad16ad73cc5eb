// qmvt_context.hip -- TP, FP and FN counts of a finished batch per sequence-context cell: homopolymer row x local GC bin
// (DESIGN.md 4.16).  k_context_build turns the 4-bit packed genome of qm_genome_load into one cell byte per position and the
// number of positions per cell; k_context_records streams the class masks and, under the kept bits, pos and flags in input order
// and counts the kept and the TP lines of every VCF per cell through one byte gather from that table; k_context_truth places
// the distinct keys of every VCF's truth set and counts them against the hit bitmaps of qm_batch_truth_hits.  Integer adds
// only.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's
// profiles are keyed on.
#include "qmvt_context.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

static_assert(CX_TILE == 16 * 256 && CX_STAGE == 24 * 256, "k_context_build: 16 positions and 24 staged positions per lane");
static_assert(CX_MAX_HALF_WINDOW % 8 == 0 && CX_TILE % 16 == 0, "a lane's staged positions are whole genome words");

// word wi of the packed genome; no base before the genome and behind its nw words
__device__ inline uint32_t cx_word(const uint32_t* words, int32_t nw, int32_t wi) {
  return (wi >= 0 && wi < nw) ? words[wi] : 0xffffffffu;
}

// base indicator << 16 | C-or-G indicator of a 4-bit code
__device__ inline uint32_t cx_ind(uint32_t c) {
  return c < 4u ? 0x10000u | ((c ^ (c >> 1)) & 1u) : 0u;   // C = 1, G = 2
}

// One workgroup per CX_TILE positions.  The base and GC indicators of the tile and a halo of CX_MAX_HALF_WINDOW positions to
// either side go to LDS as exclusive prefix sums (both counts in one word: at most CX_STAGE each), so a window costs two
// reads; min(15, run) is exact from the 14 positions to either side, six packed words per lane, without LDS.
__global__ __launch_bounds__(256) void k_context_build(ContextBuildParams P) {
  __shared__ uint32_t s_pre[CX_STAGE + 1];
  __shared__ uint32_t s_wave[4];
  __shared__ uint32_t s_gen[CX_MAX_CELLS];
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  const int32_t nw = P.len / 8 + 2;
  const int32_t t0 = (int32_t)blockIdx.x * CX_TILE;   // the tile's first position, 0-based
  const int n_cells = CX_HP_ROWS * P.ng + 1;
  for (int i = t; i < CX_MAX_CELLS; i += 256) s_gen[i] = 0u;

  // staged position k of the workgroup = genome position t0 - CX_MAX_HALF_WINDOW + k; lane t takes 24 t .. 24 t + 23: three words
  const int32_t wi0 = (t0 - CX_MAX_HALF_WINDOW) / 8 + 3 * t;   // (exact: both are multiples of 8)
  uint32_t x[3];
  uint32_t tot = 0u;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    x[q] = cx_word(P.words, nw, wi0 + q);
#pragma unroll
    for (int e = 0; e < 8; ++e) tot += cx_ind((x[q] >> (4 * e)) & 15u);
  }
  uint32_t inc = tot;   // inclusive scan over the wave, then over the four waves
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)inc, d);
    if (lane >= d) inc += y;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t run_sum = inc - tot;
  for (int q = 0; q < wave; ++q) run_sum += s_wave[q];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s_pre[24 * t + 8 * q + e] = run_sum;
      run_sum += cx_ind((x[q] >> (4 * e)) & 15u);
    }
  }
  if (t == 255) s_pre[CX_STAGE] = run_sum;
  __syncthreads();

  // lane t takes positions i0 .. i0 + 15; bit b of V / E is position i0 - 16 + b: it holds a base / the base of the one before
  const int32_t i0 = t0 + 16 * t;
  if (i0 < P.len) {
    uint64_t V = 0ull, E = 0ull;
    uint32_t prev = 15u;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const uint32_t y = cx_word(P.words, nw, i0 / 8 - 2 + q);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t c = (y >> (4 * e)) & 15u;
        if (c < 4u) {
          V |= 1ull << (8 * q + e);
          if (c == prev) E |= 1ull << (8 * q + e);
        }
        prev = c;
      }
    }
    // run of bit b, b = 15 .. 32: 1 + the E bits from b down + the E bits from b + 1 up (bits 1 .. 47 are known: 14 to either side)
    uint32_t run[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) {
      const int b = 15 + k;
      const int l = __clzll((long long)~(E << (63 - b)));
      const int r = __ffsll((unsigned long long)~(E >> (b + 1))) - 1;
      run[k] = ((V >> b) & 1ull) ? (uint32_t)min(15, 1 + l + r) : 0u;
    }
    uint32_t cells[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      uint32_t cell = CX_NONE;
      if (i0 + k < P.len) {
        const uint32_t hp = max(run[k], max(run[k + 1], run[k + 2]));
        const int li = 16 * t + k + CX_MAX_HALF_WINDOW;   // the position's staged index
        const uint32_t d = s_pre[li + P.w + 1] - s_pre[li - P.w];   // (no borrow: both halves are non-negative)
        const uint32_t nb = d >> 16, gc = d & 0xffffu;
        if (nb) cell = hp * (uint32_t)P.ng + min((uint32_t)P.ng - 1u, gc * (uint32_t)P.ng / nb);
        atomicAdd(s_gen + (nb ? (int)cell : n_cells - 1), 1u);
      }
      cells[k >> 2] |= cell << (8 * (k & 3));
    }
    qm_uint4 v4;
    v4.x = cells[0]; v4.y = cells[1]; v4.z = cells[2]; v4.w = cells[3];
    *reinterpret_cast<qm_uint4*>(P.tab + i0) = v4;
  }
  __syncthreads();
  for (int i = t; i < n_cells; i += 256)
    if (s_gen[i]) atomicAdd(P.gen + i, (unsigned long long)s_gen[i]);
}

// the row of a position under a VCF's table: its cell, NONE (row 16 ng) outside the genome and where the table says so
__device__ inline uint32_t cx_row(const uint8_t* tab, uint32_t len, int32_t p, uint32_t none) {
  if ((uint32_t)p - 1u >= len) return none;   // p < 1 or p > len
  const uint32_t c = tab[(uint32_t)p - 1u];
  return c == CX_NONE ? none : c;
}

// Adds the workgroup's counters to the VCF's rows and clears them.  cnt: [rows][2] u32 in LDS (kept, TP), laid out like the rows.
__device__ inline void cx_flush(uint32_t* cnt, int words, uint64_t* out) {
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += blockDim.x) {
    const uint32_t v = cnt[i];
    if (v) {
      atomicAdd(reinterpret_cast<unsigned long long*>(out + i), (unsigned long long)v);
      cnt[i] = 0u;
    }
  }
  __syncthreads();
}

// One wave's records of one step, one per lane: `in` = the lane has a counted record, `tp` = it is a TP line, `row` = its row.
// AGG: one add per distinct row of the wave (the first lane that still holds a record names the row, a ballot finds its
// peers); called by every lane of the wave (uniform control flow).  Otherwise one LDS atomic per record.
template <bool AGG>
__device__ inline void cx_count(uint32_t* cnt, bool in, bool tp, uint32_t row, int lane) {
  if constexpr (AGG) {
    const uint64_t tpb = __ballot(in && tp);
    uint64_t left;
    while ((left = __ballot(in)) != 0ull) {
      const int leader = __ffsll((unsigned long long)left) - 1;
      const uint32_t r = (uint32_t)__shfl((int)row, leader);
      const uint64_t peers = __ballot(in && row == r);
      if (lane == leader) {
        atomicAdd(cnt + 2 * r, (uint32_t)__popcll(peers));
        const uint32_t n_tp = (uint32_t)__popcll(peers & tpb);
        if (n_tp) atomicAdd(cnt + 2 * r + 1, n_tp);
      }
      if (row == r) in = false;
    }
  } else {
    if (in) {
      atomicAdd(cnt + 2 * row, 1u);
      if (tp) atomicAdd(cnt + 2 * row + 1, 1u);
    }
  }
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads).  Every lane stays
// in the loop for all of a span's steps: the wave's ballots need them together.
template <bool AGG>
__global__ __launch_bounds__(256) void k_context_records(ContextRecParams P) {
  __shared__ uint32_t cnt[2 * (CX_MAX_CELLS + 1)];   // at most PASS_SPANS * SPAN_TILES * K1_TILE = 65 536 records: u32 suffices
  const uint32_t none = (uint32_t)(CX_HP_ROWS * P.ng);
  const int words = 2 * ((int)none + 2);   // the grid, NONE, nokey
  for (int i = threadIdx.x; i < 2 * (CX_MAX_CELLS + 1); i += blockDim.x) cnt[i] = 0u;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  ContextTab T{nullptr, 0};
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (T.tab) cx_flush(cnt, words, P.out + (int64_t)cur * words);
      cur = sd.vcf;
      T = P.tabs[cur];
    }
    if (!T.tab) continue;   // (uniform over the workgroup)
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 4 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 4 * (int64_t)threadIdx.x;
      uint32_t kb = 0u, tb = 0u;
      if (g < sd.end) {
        kb = (uint32_t)(P.mask_pass[g >> 6] >> (int)(g & 63)) & 15u;
        if (sd.end - g < 4) kb &= (1u << (uint32_t)(sd.end - g)) - 1u;   // bits past the VCF's last record are not defined
      }
      if (!__ballot(kb != 0u)) continue;   // (uniform over the wave)
      uint32_t row[4] = {0u, 0u, 0u, 0u};
      if (kb) {
        tb = (uint32_t)(P.mask_tp[g >> 6] >> (int)(g & 63)) & 15u;
        const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((kb >> k) & 1u)) continue;
          row[k] = ((f4 >> (8 * k)) & QMF_NOKEY) ? none + 1u   // its pos column is not consulted
                                                 : cx_row(T.tab, (uint32_t)T.len, p4[k], none);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) cx_count<AGG>(cnt, (kb >> k) & 1u, (tb >> k) & 1u, row[k], lane);
    }
  }
  if (T.tab) cx_flush(cnt, words, P.out + (int64_t)cur * words);
}

// grid (x, vcf), a lane per distinct truth key: out[vcf][cell(key >> 4)] += (1, the key's bit in the VCF's hit bitmap)
__global__ __launch_bounds__(256) void k_context_truth(const ContextTruthRow* rows, int ng, unsigned long long* out) {
  __shared__ uint32_t cnt[2 * CX_MAX_CELLS];
  const ContextTruthRow R = rows[blockIdx.y];
  if (!R.tab) return;   // (uniform over the workgroup)
  const uint32_t none = (uint32_t)(CX_HP_ROWS * ng);
  const int words = 2 * ((int)none + 1);
  for (int i = threadIdx.x; i < words; i += blockDim.x) cnt[i] = 0u;
  __syncthreads();
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < R.n; j += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t row = cx_row(R.tab, (uint32_t)R.len, (int32_t)(R.keys[j] >> 4), none);
    atomicAdd(cnt + 2 * row, 1u);
    if ((R.hits[j >> 5] >> (uint32_t)(j & 31)) & 1u) atomicAdd(cnt + 2 * row + 1, 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += blockDim.x)
    if (cnt[i]) atomicAdd(out + (int64_t)blockIdx.y * words + i, (unsigned long long)cnt[i]);
}

void launch_context_build(const ContextBuildParams& P, hipStream_t st) {
  if (P.len <= 0) return;
  hipLaunchKernelGGL(k_context_build, dim3((unsigned)((P.len + CX_TILE - 1) / CX_TILE)), dim3(256), 0, st, P);
}

void launch_context_records(const ContextRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  hipLaunchKernelGGL(k_context_records<CX_AGGREGATE>, grid, dim3(256), 0, st, P);
}

void launch_context_truth(const ContextTruthRow* rows, int n_vcf, int64_t max_n, int ng, unsigned long long* out, hipStream_t st) {
  if (n_vcf <= 0 || max_n <= 0) return;
  const int64_t bx = std::min<int64_t>(64, std::max<int64_t>(1, (max_n + 255) / 256));
  for (int v0 = 0; v0 < n_vcf; v0 += 65535)   // (the grid's y extent)
    hipLaunchKernelGGL(k_context_truth, dim3((unsigned)bx, (unsigned)std::min(65535, n_vcf - v0)), dim3(256), 0, st, rows + v0, ng,
                       out + (int64_t)v0 * 2 * (CX_HP_ROWS * ng + 1));
}

}  // namespace qm
