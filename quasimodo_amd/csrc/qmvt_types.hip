// qmvt_types.hip -- TP, FP and FN by variant type and size: every record of a finished allele-extended batch and
// every entry of its truth sets is typed SNV, MNP, INS, DEL or CPX from its two allele codes -- the common prefix, then the common
// suffix of what is left, are trimmed; what remains names the type and the size --, binned by size and counted per VCF.
// k_type_records streams the batch in input order, counts the kept records and the TP lines among them per row and marks the
// truth entries spelled like a kept record; k_type_truth counts the entries and the marked ones per row.  Alleles of more than 13
// bases are dictionary ids: a table of (length, first 13 bases, last 13 bases) per id decides every pair with ONE long allele.
// Integer work only: no output depends on the order the lanes run in.  Its own translation unit: qm_kernels_id
// (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's profiles are keyed on.
#include "qmvt_types.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// the index of the entry spelled (p, r, a) in the truth set's sorted table, or -1 (0 <= p < 2^28: the caller's duty)
__device__ inline int64_t vt_entry(const TypeVcf& V, int32_t p, int32_t r, int32_t a) {
  const uint32_t key = ((uint32_t)p << 4) | allele_nib(r, a);
  int64_t lo = 0, hi = V.xn;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const uint32_t k = V.xkeys[mid];
    bool less = k < key;
    if (k == key) {
      const int32_t rr = V.xref[mid];
      less = rr < r || (rr == r && V.xalt[mid] < a);
    }
    if (less) lo = mid + 1; else hi = mid;
  }
  return lo < V.xn && V.xkeys[lo] == key && V.xref[lo] == r && V.xalt[lo] == a ? lo : -1;
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte accesses).  Every kept
// record adds one to its row's cell of the workgroup's LDS histogram (a TP line one more to the cell beside it): one LDS atomic
// per count, no reduction over the wave (DESIGN.md 4.19 says why).  The histogram goes to the VCF's rows when the VCF changes.
__global__ __launch_bounds__(256) void k_type_records(TypeRecParams P) {
  __shared__ uint32_t hist[2 * TYPE_MAX_ROWS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records per workgroup: u32 suffices
  if (threadIdx.x < 2 * TYPE_MAX_ROWS) hist[threadIdx.x] = 0u;
  __syncthreads();
  const int cells = 2 * P.bins.n_rows;
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  auto flush = [&]() {   // (uniform over the workgroup)
    __syncthreads();
    if ((int)threadIdx.x < cells && hist[threadIdx.x]) {
      atomicAdd(reinterpret_cast<unsigned long long*>(P.rec + (int64_t)cur * cells + threadIdx.x), (unsigned long long)hist[threadIdx.x]);
      hist[threadIdx.x] = 0u;
    }
    __syncthreads();
  };
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (cur >= 0) flush();
      cur = sd.vcf;
    }
    const TypeVcf& V = P.vcfs[cur];
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 4 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 4 * (int64_t)threadIdx.x;
      if (g >= sd.end) continue;
      const uint32_t nrec = (uint32_t)min((int64_t)4, sd.end - g);   // (bits and columns past the VCF's last record are not defined)
      const uint32_t kb = (uint32_t)(P.mask_pass[g >> 6] >> (int)(g & 63)) & 15u;
      const uint32_t tb = (uint32_t)(P.mask_tp[g >> 6] >> (int)(g & 63)) & 15u;
      const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
      const qm_int4 r4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.ref + g));
      const qm_int4 a4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.alt + g));
      const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
      uint32_t row4 = 0u;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if ((uint32_t)k >= nrec) continue;
        const bool kept = (kb >> k) & 1u, tp = (tb >> k) & 1u, nokey = ((f4 >> (8 * k)) & QMF_NOKEY) != 0u;
        const int32_t p = p4[k], r = r4[k], a = a4[k];
        const uint32_t row = vt_row(r, a, nokey, P.shapes, P.bins);
        row4 |= row << (8 * k);
        if (!kept) continue;
        atomicAdd(hist + 2u * row, 1u);
        if (tp) atomicAdd(hist + 2u * row + 1u, 1u);
        if (!nokey && allele_valid(r) && allele_valid(a) && (uint32_t)p < (1u << 28)) {
          const int64_t e = vt_entry(V, p, r, a);
          if (e >= 0) {
            const uint32_t bit = 1u << ((uint32_t)e & 31u);
            if (!(V.ebits[e >> 5] & bit)) atomicOr(V.ebits + (e >> 5), bit);   // (a stale read only repeats the atomic)
          }
        }
      }
      if (P.row) *reinterpret_cast<uint32_t*>(P.row + g) = row4;
    }
  }
  if (cur >= 0) flush();
}

// grid (x, VCF), a lane per entry of the VCF's truth set: its row, and whether k_type_records marked it
__global__ __launch_bounds__(256) void k_type_truth(TypeTruthParams P) {
  __shared__ uint32_t hist[2 * TYPE_MAX_ROWS];
  if (threadIdx.x < 2 * TYPE_MAX_ROWS) hist[threadIdx.x] = 0u;
  __syncthreads();
  const TypeVcf& V = P.vcfs[blockIdx.y];
  const int cells = 2 * P.bins.n_rows;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < V.xn) {
    const uint32_t row = vt_row(V.xref[j], V.xalt[j], false, P.shapes, P.bins);
    atomicAdd(hist + 2u * row, 1u);
    if ((V.ebits[j >> 5] >> ((uint32_t)j & 31u)) & 1u) atomicAdd(hist + 2u * row + 1u, 1u);
  }
  __syncthreads();
  if ((int)threadIdx.x < cells && hist[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(P.tru + (int64_t)blockIdx.y * cells + threadIdx.x), (unsigned long long)hist[threadIdx.x]);
}

void launch_type_records(const TypeRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  hipLaunchKernelGGL(k_type_records, grid, dim3(256), 0, st, P);
}

void launch_type_truth(const TypeTruthParams& P, int n_vcf, int64_t max_entries, hipStream_t st) {
  if (max_entries <= 0) return;
  const unsigned gx = (unsigned)((max_entries + 255) / 256);
  for (int v0 = 0; v0 < n_vcf; v0 += 65535) {   // (the y dimension of a grid holds 65535 blocks)
    const int nv = std::min(n_vcf - v0, 65535);
    TypeTruthParams Q = P;
    Q.vcfs = P.vcfs + v0;
    Q.tru = P.tru + (int64_t)v0 * 2 * P.bins.n_rows;
    hipLaunchKernelGGL(k_type_truth, dim3(gx, (unsigned)nv), dim3(256), 0, st, Q);
  }
}

}  // namespace qm
