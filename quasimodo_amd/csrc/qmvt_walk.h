// qmvt_walk.h -- the walk over a finished batch's spans that every pass's record kernel makes, and what goes
// with it: the grid of such a kernel, the mask of a lane's records at a VCF's ragged end, the flush of LDS counts.  Device side
// only: included by the pass units (qmvt_*.hip), never by the host code.
#pragma once
#include "qmvt_dev.h"

namespace qm {

typedef int qm_int4 __attribute__((ext_vector_type(4)));
typedef unsigned qm_uint4 __attribute__((ext_vector_type(4)));
typedef float qm_float4 __attribute__((ext_vector_type(4)));
typedef unsigned qm_uint2 __attribute__((ext_vector_type(2)));

constexpr int PASS_SPANS = 4;   // batch spans (SPAN_TILES tiles of one VCF each) per workgroup of a record kernel
static_assert((int64_t)PASS_SPANS * SPAN_TILES * K1_TILE < (1ll << 32), "a workgroup's counts of its records fit u32 cells");

inline unsigned pass_grid(int n_spans) { return (unsigned)((n_spans + PASS_SPANS - 1) / PASS_SPANS); }

// One workgroup (256 lanes) takes PASS_SPANS consecutive spans of the batch layout; a span never crosses a VCF and starts at a
// multiple of 256 records.  Lane t takes records g .. g + PER - 1, g = g0 + PER t, of every step g0 = begin, begin + 256 PER, ...
//   enter(vcf, sd) -> bool   when the VCF changes: load the per-VCF state, say whether the VCF is walked at all
//   step(vcf, sd, g)         every step of a walked span
//   leave(vcf)               once per walked VCF, before the next enter and at the end: flush what the steps counted
// All three are uniform over the workgroup, so each may hold barriers.  The loop is the uniform one, for every kernel: step is
// called for the lanes with g >= sd.end too, every lane stays for all of a span's steps, and a body may use ballots and
// barriers.  A body that has none starts with `if (g >= sd.end) return;`.  A loop in which each lane leaves on its own is not
// offered: it is correct only until the body gains its first wave-wide operation.
template <int PER, typename Enter, typename Step, typename Leave>
__device__ __forceinline__ void walk_spans(const SpanDesc* spans, int n_spans, Enter&& enter, Step&& step, Leave&& leave) {
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, n_spans);
  int cur = -1;
  bool walked = false;
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = spans[s];
    if (sd.vcf != cur) {
      if (walked) leave(cur);
      cur = sd.vcf;
      walked = enter(cur, sd);
    }
    if (!walked) continue;   // (uniform over the workgroup)
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += PER * (int64_t)blockDim.x)
      step(cur, sd, g0 + PER * (int64_t)threadIdx.x);
  }
  if (walked) leave(cur);
}

// bit k: record g + k exists (bits and columns past the VCF's last record are not defined); 0 for a lane behind the end
template <int PER>
__device__ __forceinline__ uint32_t rec_live(int64_t g, int64_t end) {
  static_assert(PER == 4 || PER == 8 || PER == 16, "a lane's records are a nibble, a byte or a half word of the masks");
  const int64_t n = end - g;
  return n >= PER ? (1u << PER) - 1u : n > 0 ? (1u << (uint32_t)n) - 1u : 0u;
}

// the PER bits of a record mask at g: g is a multiple of PER and PER divides 64, so they sit in one word
template <int PER>
__device__ __forceinline__ uint32_t mask_bits(const uint64_t* mask, int64_t g) {
  static_assert(PER == 4 || PER == 8 || PER == 16, "the bits of a lane's records never straddle a 64-bit word");
  return (uint32_t)(mask[g >> 6] >> (int)(g & 63)) & ((1u << PER) - 1u);
}

// Adds the workgroup's n LDS counts to a VCF's 64-bit row, non-zero cells only, and leaves them zero.  Uniform over the workgroup.
__device__ inline void flush_counts(uint32_t* lds, int n, unsigned long long* row) {
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const uint32_t v = lds[i];
    if (v) {
      atomicAdd(row + i, (unsigned long long)v);
      lds[i] = 0u;
    }
  }
  __syncthreads();
}

}  // namespace qm
