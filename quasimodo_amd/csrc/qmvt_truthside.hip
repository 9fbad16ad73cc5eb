// qmvt_truthside.hip -- the truth-side view of a finished batch: k_truth_hits marks, per VCF, which keys of its
// truth set some kept record carries (a bitmap over the sorted distinct keys: the set behind QM_S_TP_R) and which records carry a
// key of the truth set (a record mask: its complement under the kept mask is the key multiset behind QM_S_FP_R); k_truth_regions
// counts, for groups of up to five VCFs of one truth set, the truth keys per membership mask -- the `Genome` half of the caller
// Venn diagram of scripts/caller_performance_compare.R:110-119,510-549 -- and writes the OR of the group's bitmaps.  Its own
// translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's profiles are keyed on.
#include "qmvt_truthside.h"
#include "qmvt_walk.h"

namespace qm {

// index of `key` among the truth set's sorted distinct keys, or -1: the coarse position index, then a bisection of its cell
__device__ inline int32_t truth_find(const TruthDev& T, uint32_t pos, uint32_t key) {
  const uint32_t b = pos >> T.shift;
  if (b > (uint32_t)T.nb) return -1;   // (tidx has nb + 2 entries)
  int32_t lo = T.tidx[b];
  const int32_t end = T.tidx[b + 1];
  int32_t hi = end;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (T.keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  return (lo < end && T.keys[lo] == key) ? lo : -1;
}

// ORs the words the workgroup touched into the VCF's bitmap (one atomic per touched word) and clears them
__device__ inline void hits_flush(uint32_t* lds, uint32_t* row, int32_t words) {
  __syncthreads();
  for (int32_t w = threadIdx.x; w < words; w += blockDim.x) {
    const uint32_t x = lds[w];
    if (x) { atomicOr(row + w, x); lds[w] = 0u; }
  }
  __syncthreads();
}

// The span walk of qmvt_walk.h, 8 records per lane (aligned loads, one whole mask byte per lane).
__global__ __launch_bounds__(256) void k_truth_hits(TruthHitsParams P) {
  __shared__ uint32_t lds[TS_LDS_WORDS];
  for (int i = threadIdx.x; i < TS_LDS_WORDS; i += blockDim.x) lds[i] = 0u;
  __syncthreads();
  TruthDev T{};
  uint32_t* row = nullptr;
  int32_t words = 0;
  bool in_lds = false;
  walk_spans<8>(
      P.spans, P.n_spans,
      [&](int vcf, const SpanDesc& sd) {
        T = P.truths[sd.truth];
        row = P.hits + P.hit_off[vcf];
        words = (int32_t)((T.n + 31) >> 5);
        in_lds = TS_USE_LDS && words <= TS_LDS_WORDS;
        return true;
      },
      [&](int, const SpanDesc& sd, int64_t g) {
        if (g >= sd.end) return;
        const uint32_t kb = mask_bits<8>(P.mask_pass, g) & rec_live<8>(g, sd.end);
        uint32_t out = 0u;
        if (kb) {
          const uint32_t tb = mask_bits<8>(P.mask_tp, g);
          const qm_int4 pa = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));
          const qm_int4 pb = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g + 4));
          const uint2 ab8 = *reinterpret_cast<const uint2*>(P.anib + g);
          const uint2 f8 = *reinterpret_cast<const uint2*>(P.flags + g);
          const int32_t pp[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const uint32_t ab = ((k < 4 ? ab8.x : ab8.y) >> (8 * (k & 3))) & 0xffu;
            const uint32_t fl = ((k < 4 ? f8.x : f8.y) >> (8 * (k & 3))) & 0xffu;
            if (!((kb >> k) & 1u) || (ab & ANIB_NONE) || (fl & QMF_NOKEY)) continue;   // not kept, or no comparable key
            // a kept '.'-ID line with a key that is no TP line: its key is not in the truth set (exact: DESIGN.md 4.8)
            if (TS_SHORTCUT && (fl & QMF_IDDOT) && !((tb >> k) & 1u)) continue;
            const uint32_t p = (uint32_t)pp[k];
            const int32_t j = truth_find(T, p, (p << 4) | ab);
            if (j < 0) continue;
            out |= 1u << k;
            if (in_lds) atomicOr(lds + (j >> 5), 1u << (j & 31));
            else atomicOr(row + (j >> 5), 1u << (j & 31));
          }
        }
        P.mask_intruth[g >> 3] = (uint8_t)out;
      },
      [&](int) {
        if (in_lds) hits_flush(lds, row, words);   // (uniform over the workgroup)
      });
}

// grid (x, group): regions[group][m] += truth keys whose membership mask over the group's VCFs is m, 32 keys per word
__global__ __launch_bounds__(256) void k_truth_regions(const TruthGroup* groups, unsigned long long* regions) {
  __shared__ uint32_t cnt[TS_REGIONS];
  if (threadIdx.x < TS_REGIONS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const TruthGroup G = groups[blockIdx.y];
  uint32_t c[TS_REGIONS];
#pragma unroll
  for (int m = 0; m < TS_REGIONS; ++m) c[m] = 0u;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < G.words; w += (int64_t)gridDim.x * blockDim.x) {
    uint32_t x[TS_MAX_GROUP];
#pragma unroll
    for (int i = 0; i < TS_MAX_GROUP; ++i) x[i] = i < G.n ? G.bits[i][w] : 0u;
    const uint32_t valid = (w == G.words - 1 && (G.tn & 31)) ? (1u << (uint32_t)(G.tn & 31)) - 1u : 0xffffffffu;
    if (G.uni) G.uni[w] = x[0] | x[1] | x[2] | x[3] | x[4];
#pragma unroll
    for (int m = 0; m < TS_REGIONS; ++m) {
      uint32_t a = valid;
#pragma unroll
      for (int i = 0; i < TS_MAX_GROUP; ++i) a &= ((m >> i) & 1) ? x[i] : ~x[i];
      c[m] += (uint32_t)__popc(a);
    }
  }
#pragma unroll
  for (int m = 0; m < TS_REGIONS; ++m)
    if (c[m]) atomicAdd(cnt + m, c[m]);
  __syncthreads();
  if (threadIdx.x < TS_REGIONS && cnt[threadIdx.x])
    atomicAdd(regions + (int64_t)blockIdx.y * TS_REGIONS + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

void launch_truth_hits(const TruthHitsParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_truth_hits, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_truth_regions(const TruthGroup* groups, int n_groups, int64_t max_words, unsigned long long* regions, hipStream_t st) {
  if (n_groups <= 0) return;
  const int64_t bx = std::min<int64_t>(64, std::max<int64_t>(1, (max_words + 255) / 256));
  hipLaunchKernelGGL(k_truth_regions, dim3((unsigned)bx, (unsigned)n_groups), dim3(256), 0, st, groups, regions);
}

}  // namespace qm
