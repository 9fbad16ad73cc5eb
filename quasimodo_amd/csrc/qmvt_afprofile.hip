// qmvt_afprofile.hip -- k_af_profile: genome position against allele frequency of the TP and FP SNVs of every VCF of a finished
// batch, as a grid of counts (the reference's rule mutationcontext: filterVCF + varPlot of scripts/mutation_context_profile.R,
// DESIGN.md 4.9).  One streaming pass over the class masks and, under the kept bits, pos, the optional af column and the allele
// byte, in input order.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the
// classification pass's profiles are keyed on.
#include "qmvt_afprofile.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// Adds the workgroup's grids and the lanes' extras to the VCF's rows and clears both.  h: [2][cells] u32 in LDS (at least
// 2 * AFP_EXTRA words), laid out like the VCF's rows of the output; c: this lane's extras, summed through the first words of h
// once the grid has left them zero (64 KiB of grid leave no room for a second array).
__device__ inline void afp_flush(uint32_t* h, uint32_t (&c)[2 * AFP_EXTRA], int cells, uint64_t* grid, uint64_t* extra) {
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x) {
    const uint32_t v = h[i];
    if (v) {
      atomicAdd(reinterpret_cast<unsigned long long*>(grid + i), (unsigned long long)v);
      h[i] = 0u;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 2 * AFP_EXTRA; ++k) {
    if (c[k]) atomicAdd(h + k, c[k]);
    c[k] = 0u;
  }
  __syncthreads();
  if (threadIdx.x < 2 * AFP_EXTRA) {
    const uint32_t v = h[threadIdx.x];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(extra + threadIdx.x), (unsigned long long)v);
    h[threadIdx.x] = 0u;
  }
  __syncthreads();
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads).
template <bool EXT>
__global__ __launch_bounds__(256) void k_af_profile(AfProfileParams P) {
  extern __shared__ uint32_t afp_h[];   // [TP, FP][n_af][n_pos]: at most PASS_SPANS * SPAN_TILES * K1_TILE records, u32 suffices
  const int cells = P.n_af * P.n_pos;
  for (int i = threadIdx.x; i < max(2 * cells, 2 * AFP_EXTRA); i += blockDim.x) afp_h[i] = 0u;
  __syncthreads();
  uint32_t c[2 * AFP_EXTRA] = {0u, 0u, 0u, 0u, 0u, 0u};
  const float fa = (float)P.n_af;
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  bool on = false;
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (on) afp_flush(afp_h, c, cells, P.grid + (int64_t)cur * 2 * cells, P.extra + (int64_t)cur * 2 * AFP_EXTRA);
      cur = sd.vcf;
      on = P.has_af[cur] != 0;
    }
    if (!on) continue;
    for (int64_t g = sd.begin + 4 * (int64_t)threadIdx.x; g < sd.end; g += 4 * (int64_t)blockDim.x) {
      const int sh = (int)(g & 63);
      uint32_t kb = (uint32_t)(P.mask_pass[g >> 6] >> sh) & 15u;
      if (sd.end - g < 4) kb &= (1u << (uint32_t)(sd.end - g)) - 1u;   // bits past the VCF's last record are not defined
      if (!kb) continue;
      const uint32_t tb = (uint32_t)(P.mask_tp[g >> 6] >> sh) & 15u;
      const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));      // read once
      const qm_float4 f4 = __builtin_nontemporal_load(reinterpret_cast<const qm_float4*>(P.af + g));
      uint32_t ab4 = 0u;   // four allele bytes: ref << 2 | alt, ANIB_NONE when either is not a single base
      if constexpr (EXT) {
        const int4 r4 = *reinterpret_cast<const int4*>(P.ref + g);
        const int4 a4 = *reinterpret_cast<const int4*>(P.alt + g);
        ab4 = (uint32_t)allele_byte(r4.x, a4.x) | ((uint32_t)allele_byte(r4.y, a4.y) << 8) | ((uint32_t)allele_byte(r4.z, a4.z) << 16) |
              ((uint32_t)allele_byte(r4.w, a4.w) << 24);
      } else {
        ab4 = *reinterpret_cast<const uint32_t*>(P.anib + g);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!((kb >> k) & 1u) || ((ab4 >> (8 * k)) & ANIB_NONE)) continue;   // not kept, or not an SNV: counted nowhere
        const uint32_t fp = ((tb >> k) & 1u) ^ 1u;                             // class 0 = TP, 1 = FP
        const float f = f4[k];
        const uint32_t n = (uint32_t)p4[k] - 1u;                               // pos < 1 wraps beyond every bin
        if (f != f) { c[AFP_NO_AF] += fp ^ 1u; c[AFP_EXTRA + AFP_NO_AF] += fp; continue; }
        // (pos - 1) / window: the reciprocal is exact below 2^28 (qmvt_afprofile.h); a position beyond, which no scanner
        // makes, is divided the long way
        const uint32_t pb = n < (1u << AFP_POS_BITS) ? (uint32_t)(((uint64_t)n * P.div.mul) >> P.div.shift) : n / (uint32_t)P.window;
        if (!(f >= 0.0f) || f > 1.0f || p4[k] < 1 || pb >= (uint32_t)P.n_pos) {
          c[AFP_OUTSIDE] += fp ^ 1u; c[AFP_EXTRA + AFP_OUTSIDE] += fp;
          continue;
        }
        const int a = min(P.n_af - 1, (int)__fmul_rn(f, fa));                  // one float multiply, contracted with nothing
        c[AFP_N_GRID] += fp ^ 1u; c[AFP_EXTRA + AFP_N_GRID] += fp;
        atomicAdd(afp_h + ((int)fp * P.n_af + a) * P.n_pos + (int)pb, 1u);
      }
    }
  }
  if (on) afp_flush(afp_h, c, cells, P.grid + (int64_t)cur * 2 * cells, P.extra + (int64_t)cur * 2 * AFP_EXTRA);
}

void launch_af_profile(const AfProfileParams& P, bool ext, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  const size_t lds = std::max((size_t)2 * (size_t)P.n_af * (size_t)P.n_pos, (size_t)2 * AFP_EXTRA) * sizeof(uint32_t);
  if (ext) hipLaunchKernelGGL(k_af_profile<true>, grid, dim3(256), lds, st, P);
  else hipLaunchKernelGGL(k_af_profile<false>, grid, dim3(256), lds, st, P);
}

}  // namespace qm
