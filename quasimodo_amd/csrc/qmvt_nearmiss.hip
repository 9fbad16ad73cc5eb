// qmvt_nearmiss.hip -- why a line is a false positive and a truth key a false negative.  k_nearmiss_records streams
// every record of a finished batch once, in input order, finds the truth keys within `radius` positions of it (the coarse index
// of its window's first cell, one bisection, a bounded walk forward), gives every FP line one class byte and marks, per VCF, in
// four bit planes laid out like the hit bitmap what the VCF's records say about every truth key (called and filtered; another
// alt; something else at the position; something nearby).  k_nearmiss_truth reduces the planes and the hit bitmap of
// k_truth_hits to the classes of the missed keys.  Its own translation unit: qm_kernels_id stays the id the classification
// pass's profiles are keyed on.
#include "qmvt_nearmiss.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// a lane's class counts between two flushes, 10 bits per class in one register pair: it sees at most 8 records per 2048 of
// PASS_SPANS spans
constexpr int NM_CNT_BITS = 10;
static_assert((int64_t)PASS_SPANS * SPAN_TILES * K1_TILE / 256 < (1 << NM_CNT_BITS), "packed per-lane class counts");
static_assert(NM_R_CLASSES * NM_CNT_BITS <= 64, "packed per-lane class counts");

// Behind the last record of a VCF inside the workgroup: the lanes' class counts meet in LDS and leave as one 64-bit atomic per
// class; the plane words the workgroup touched are ORed into the VCF's rows (one atomic per touched word) and cleared.
__device__ inline void nearmiss_flush(uint32_t* lds, uint32_t* rc, uint64_t& cnt, const NearmissParams& P, int vcf, int64_t off, int32_t words,
                                      bool in_lds) {
  if (cnt) {
#pragma unroll
    for (int k = 0; k < NM_R_CLASSES; ++k) {
      const uint32_t x = (uint32_t)(cnt >> (NM_CNT_BITS * k)) & ((1u << NM_CNT_BITS) - 1u);
      if (x) atomicAdd(rc + k, x);
    }
    cnt = 0;
  }
  __syncthreads();
  if (in_lds) {
    for (int32_t w = threadIdx.x; w < words; w += blockDim.x) {
#pragma unroll
      for (int p = 0; p < NM_PLANES; ++p) {
        const uint32_t x = lds[p * NM_LDS_WORDS + w];
        if (x) { atomicOr(P.planes + (int64_t)p * P.plane_words + off + w, x); lds[p * NM_LDS_WORDS + w] = 0u; }
      }
    }
  }
  if (threadIdx.x < NM_R_CLASSES && rc[threadIdx.x]) {
    atomicAdd(P.rec + (int64_t)vcf * NM_R_CLASSES + threadIdx.x, (unsigned long long)rc[threadIdx.x]);
    rc[threadIdx.x] = 0u;
  }
  __syncthreads();
}

// The span walk of qmvt_walk.h, 8 records per lane: one whole byte of every record mask, eight class bytes.
__global__ __launch_bounds__(256) void k_nearmiss_records(NearmissParams P) {
  __shared__ uint32_t lds[NM_PLANES * NM_LDS_WORDS];
  __shared__ uint32_t rc[8];
  for (int i = threadIdx.x; i < NM_PLANES * NM_LDS_WORDS; i += blockDim.x) lds[i] = 0u;
  if (threadIdx.x < 8) rc[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t radius = (uint32_t)P.radius;
  TruthDev T{};
  int64_t off = 0;
  int32_t words = 0;
  bool in_lds = false;
  uint64_t cnt = 0;
  walk_spans<8>(
      P.spans, P.n_spans,
      [&](int vcf, const SpanDesc& sd) {
        T = P.truths[sd.truth];
        off = P.hit_off[vcf];
        words = (int32_t)((T.n + 31) >> 5);
        in_lds = words <= NM_LDS_WORDS;
        return true;
      },
      [&](int, const SpanDesc& sd, int64_t g) {
        if (g >= sd.end) return;
        const uint32_t valid = rec_live<8>(g, sd.end);   // bits past the VCF's last record are not defined
        const uint32_t kb = mask_bits<8>(P.mask_pass, g) & valid;
        const uint32_t fb = kb & ~mask_bits<8>(P.mask_tp, g);   // the FP lines: kept, no TP line
        const qm_int4 pa = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));
        const qm_int4 pb = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g + 4));
        const uint2 ab8 = *reinterpret_cast<const uint2*>(P.anib + g);
        const uint2 f8 = *reinterpret_cast<const uint2*>(P.flags + g);
        const int32_t pp[8] = {pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w};
        uint64_t cls8 = ~0ull;   // NM_NONE in every byte
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (!((valid >> k) & 1u)) continue;
          const uint32_t ab = ((k < 4 ? ab8.x : ab8.y) >> (8 * (k & 3))) & 0xffu;
          const uint32_t fl = ((k < 4 ? f8.x : f8.y) >> (8 * (k & 3))) & 0xffu;
          const bool kept = (kb >> k) & 1u;
          const bool fpl = (fb >> k) & 1u;
          uint32_t c = NM_R_NOKEY;
          if (!(fl & QMF_NOKEY)) {   // a usable position: the truth keys of [pos - radius, pos + radius]
            const bool cmp = !(ab & ANIB_NONE);
            const uint32_t p = (uint32_t)pp[k];
            const uint32_t lo = p > radius ? p - radius : 0u;
            const uint64_t hi = (uint64_t)p + radius;
            const uint32_t b = lo >> T.shift;
            bool exact = false, sra = false, atpos = false, near = false;
            if (b <= (uint32_t)T.nb) {   // (tidx has nb + 2 entries)
              int32_t j = T.tidx[b];
              int32_t e = T.tidx[b + 1];
              const uint64_t lokey = (uint64_t)lo << 4;
              while (j < e) {   // the first key at or behind the window's first position; none in the cell: the next cell's first
                const int32_t mid = (j + e) >> 1;
                if ((uint64_t)T.keys[mid] < lokey) j = mid + 1; else e = mid;
              }
              for (; j < (int32_t)T.n; ++j) {   // at most 16 keys per position, 2 radius + 1 positions
                const uint32_t key = T.keys[j];
                const uint32_t kp = key >> 4;
                if ((uint64_t)kp > hi) break;
                int plane = NM_P_NEAR;
                if (kp != p) near = true;
                else {
                  atpos = true;
                  plane = NM_P_POSITION;
                  if (cmp) {
                    if ((key & 15u) == ab) { exact = true; plane = kept ? -1 : NM_P_FILTERED; }
                    else if (((key >> 2) & 3u) == (ab >> 2)) { sra = true; plane = NM_P_ALLELE; }
                  }
                }
                if (plane < 0) continue;
                const uint32_t bit = 1u << (j & 31);   // bits are only ever set: a plain look first spares the atomic where a neighbour was here
                if (in_lds) {
                  uint32_t* w = lds + plane * NM_LDS_WORDS + (j >> 5);
                  if (!(*(volatile uint32_t*)w & bit)) atomicOr(w, bit);
                } else {
                  uint32_t* w = P.planes + (int64_t)plane * P.plane_words + off + (j >> 5);
                  if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
                }
              }
            }
            if (cmp) c = exact ? NM_R_IDCOL : sra ? NM_R_ALLELE : atpos ? NM_R_REFBASE : near ? NM_R_NEAR : NM_R_ISOLATED;
          }
          if (fpl) {
            cls8 ^= (uint64_t)(c ^ NM_NONE) << (8 * k);
            cnt += 1ull << (NM_CNT_BITS * c);
          }
        }
        *reinterpret_cast<uint64_t*>(P.rcls + g) = cls8;
      },
      [&](int vcf) { nearmiss_flush(lds, rc, cnt, P, vcf, off, words, in_lds); });
}

// grid (x, VCF), strided over the VCF's words: the hit bitmap and the four planes, 32 keys per word, to the five counts of the missed keys.
__global__ __launch_bounds__(256) void k_nearmiss_truth(NearmissTruthParams P) {
  __shared__ uint32_t cnt[8];
  if (threadIdx.x < 8) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int v = blockIdx.y;
  const int64_t off = P.hit_off[v];
  const int64_t words = P.hit_off[v + 1] - off;
  const int64_t tn = P.hit_tn[v];
  uint32_t c[NM_T_CLASSES];
#pragma unroll
  for (int k = 0; k < NM_T_CLASSES; ++k) c[k] = 0u;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t valid = (w == words - 1 && (tn & 31)) ? (1u << (uint32_t)(tn & 31)) - 1u : 0xffffffffu;
    const uint32_t miss = ~P.hits[off + w] & valid;
    uint32_t x[NM_T_CLASSES];
    nearmiss_truth_word(miss, P.planes[off + w], P.planes[P.plane_words + off + w], P.planes[2 * P.plane_words + off + w],
                        P.planes[3 * P.plane_words + off + w], x);
#pragma unroll
    for (int k = 0; k < NM_T_CLASSES; ++k) c[k] += (uint32_t)__popc(x[k]);
  }
#pragma unroll
  for (int k = 0; k < NM_T_CLASSES; ++k)
    if (c[k]) atomicAdd(cnt + k, c[k]);
  __syncthreads();
  if (threadIdx.x < NM_T_CLASSES && cnt[threadIdx.x])
    atomicAdd(P.tru + (int64_t)v * NM_T_CLASSES + threadIdx.x, (unsigned long long)cnt[threadIdx.x]);
}

void launch_nearmiss_records(const NearmissParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_nearmiss_records, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_nearmiss_truth(const NearmissTruthParams& P, int n_vcf, int64_t max_words, hipStream_t st) {
  if (n_vcf <= 0) return;
  // as launch_truth_regions, but a workgroup per 2 048 words (65 536 keys): five words and five atomics per workgroup make a
  // workgroup per 256 words the slower launch at 40 000 keys (measured)
  const int64_t bx = std::min<int64_t>(64, std::max<int64_t>(1, (max_words + 2047) / 2048));
  for (int v0 = 0; v0 < n_vcf; v0 += 65535) {   // (grid y holds 65 535 VCFs)
    NearmissTruthParams Q = P;
    Q.hit_off += v0; Q.hit_tn += v0; Q.tru += (int64_t)v0 * NM_T_CLASSES;
    hipLaunchKernelGGL(k_nearmiss_truth, dim3((unsigned)bx, (unsigned)std::min(n_vcf - v0, 65535)), dim3(256), 0, st, Q);
  }
}

}  // namespace qm
