// qmvt_motif.hip -- k_motif: the 96-motif mutation-context spectra of the kept, TP and FP SNVs of every VCF of a finished batch
// (the reference's rule mutationcontext: SomaticSignatures mutationContext + motifMatrix).  One streaming pass over
// pos, the allele byte, the two class masks and (under the kept bit) flags, in input order, with a gather of a 3-base window from
// a 4-bit packed genome that sits in L2.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id
// the classification pass's profiles are keyed on.
#include "qmvt_motif.h"
#include "qmvt_walk.h"

namespace qm {

// Adds the workgroup's TP / FP histograms to the VCF's [3][MOTIF_COLS] rows (kept = TP + FP) and clears them.
__device__ inline void motif_flush(uint32_t* h, uint64_t* out) {
  __syncthreads();
  for (int c = threadIdx.x; c < MOTIF_COLS; c += blockDim.x) {
    const uint32_t t = h[c], f = h[MOTIF_COLS + c];
    if (t + f) atomicAdd(reinterpret_cast<unsigned long long*>(out + c), (unsigned long long)(t + f));
    if (t) atomicAdd(reinterpret_cast<unsigned long long*>(out + MOTIF_COLS + c), (unsigned long long)t);
    if (f) atomicAdd(reinterpret_cast<unsigned long long*>(out + 2 * MOTIF_COLS + c), (unsigned long long)f);
    h[c] = 0u;
    h[MOTIF_COLS + c] = 0u;
  }
  __syncthreads();
}

// The span walk written out, in the form in which every lane leaves on its own: the body holds no wave-wide operation and must
// not gain one (through walk_spans k_motif<true> needs 82 registers for 72 and loses two waves per SIMD).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads).
template <bool EXT>
__global__ __launch_bounds__(256) void k_motif(MotifParams P) {
  __shared__ uint32_t h[2 * MOTIF_COLS];   // [TP, FP][MOTIF_COLS]: at most PASS_SPANS * SPAN_TILES * K1_TILE records, u32 suffices
  for (int i = threadIdx.x; i < 2 * MOTIF_COLS; i += blockDim.x) h[i] = 0u;
  __syncthreads();
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  GenomeRef G{nullptr, 0};
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (G.words) motif_flush(h, P.out + (int64_t)cur * MOTIF_ROW_WORDS);
      cur = sd.vcf;
      G = P.genomes[cur];
    }
    if (!G.words) continue;
    const uint32_t lenm2 = G.len > 2 ? (uint32_t)(G.len - 2) : 0u;   // p - 2 < lenm2  <=>  2 <= p < len: G[p-2] .. G[p] exist
    for (int64_t g = sd.begin + 4 * (int64_t)threadIdx.x; g < sd.end; g += 4 * (int64_t)blockDim.x) {
      const int sh = (int)(g & 63);
      uint32_t kb = (uint32_t)(P.mask_pass[g >> 6] >> sh) & 15u;
      if (sd.end - g < 4) kb &= (1u << (uint32_t)(sd.end - g)) - 1u;   // bits past the VCF's last record are not defined
      if (!kb) continue;
      const uint32_t tb = (uint32_t)(P.mask_tp[g >> 6] >> sh) & 15u;
      const int4 p4 = *reinterpret_cast<const int4*>(P.pos + g);
      const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
      uint32_t ab4 = 0u;   // four allele bytes: ref << 2 | alt, ANIB_NONE when either is not a single base
      if constexpr (EXT) {
        const int4 r4 = *reinterpret_cast<const int4*>(P.ref + g);
        const int4 a4 = *reinterpret_cast<const int4*>(P.alt + g);
        ab4 = (uint32_t)allele_byte(r4.x, a4.x) | ((uint32_t)allele_byte(r4.y, a4.y) << 8) | ((uint32_t)allele_byte(r4.z, a4.z) << 16) |
              ((uint32_t)allele_byte(r4.w, a4.w) << 24);
      } else {
        ab4 = *reinterpret_cast<const uint32_t*>(P.anib + g);
      }
      const int32_t pp[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t ab = (ab4 >> (8 * k)) & 0xffu;
        if (!((kb >> k) & 1u) || (ab & ANIB_NONE)) continue;   // not kept, or not an SNV: counted nowhere
        uint32_t a = ab >> 2, b = ab & 3u;
        uint32_t col = MOTIF_OTHER;
        bool mism = false;
        const uint32_t i0 = (uint32_t)pp[k] - 2u;
        if (!(((f4 >> (8 * k)) & QMF_NOKEY)) && a != b && i0 < lenm2) {
          const uint64_t w = ((uint64_t)G.words[(i0 >> 3) + 1] << 32) | G.words[i0 >> 3];
          const uint32_t win = (uint32_t)(w >> (4 * (i0 & 7u)));
          uint32_t l = win & 15u, r = (win >> 8) & 15u;
          if (l < 4u && r < 4u) {
            mism = ((win >> 4) & 15u) != a;   // G[p-1] against the VCF's REF (check = FALSE: the motif keeps the VCF's REF)
            if (!(a & 1u)) {                  // A or G: the reverse complement of the context
              const uint32_t t = 3u - r;
              r = 3u - l; l = t; a = 3u - a; b = 3u - b;
            }
            const uint32_t kk = a == 1u ? (b == 0u ? 0u : b - 1u) : 3u + b;   // CA CG CT TA TC TG
            col = 16u * kk + 4u * l + r;
          }
        }
        uint32_t* row = h + (((tb >> k) & 1u) ? 0 : MOTIF_COLS);
        atomicAdd(row + col, 1u);
        if (mism) atomicAdd(row + MOTIF_REF_MISMATCH, 1u);
      }
    }
  }
  if (G.words) motif_flush(h, P.out + (int64_t)cur * MOTIF_ROW_WORDS);
}

void launch_motif(const MotifParams& P, bool ext, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  if (ext) hipLaunchKernelGGL(k_motif<true>, grid, dim3(256), 0, st, P);
  else hipLaunchKernelGGL(k_motif<false>, grid, dim3(256), 0, st, P);
}

}  // namespace qm
