// qmvt_surface.hip -- the filter surface of a finished batch: TP records, FP records and found truth keys of every
// VCF in every cell of a QUAL x AF threshold grid.  k_surface_records streams every record once (pos, allele byte, flags, qual,
// af), looks its key up by exact equality (the coarse index, one bisection), bumps the TP / FP cell of its (QUAL bin, AF bin) and
// keeps, per truth key, the largest cell code among its '.'-ID records; k_surface_truth histograms those codes into the U grid;
// k_surface_sums turns the three grids into 2-D suffix sums ("filter at QUAL >= i * q_step and AF >= k / na").  Integer max and
// add only: the result does not depend on the order of the records.  Its own translation unit: qm_kernels_id stays the id the
// classification pass's profiles are keyed on.
#include "qmvt_surface.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// index of `key` among the truth set's sorted distinct keys, or -1 (k_truth_hits' lookup: equality only, no window)
__device__ inline int32_t sf_find(const TruthDev& T, uint32_t pos, uint32_t key) {
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

// qmo_qual_bin(q, limit): floor(q) clamped to limit - 1; NaN and floor(q) < 0 give -1
__device__ inline int sf_qual_bin(float q, int limit) {
  if (!(q >= 0.0f)) return -1;
  if (q >= (float)limit) return limit - 1;
  return (int)q;
}

// Behind the last record of a VCF inside the workgroup: the non-zero cells of the two grids leave as 64-bit atomics, the
// non-zero staged codes as atomicMax, the lanes' three extras meet in LDS and leave as one atomic each; everything is left zero.
__device__ inline void sf_flush(uint32_t* h, uint32_t (&c)[SF_REC_EXTRA], int cells, bool staged, int32_t tn, unsigned long long* grid,
                                unsigned long long* extra, uint32_t* best_row) {
  uint32_t* ex = h + 2 * cells;
  uint32_t* stage = ex + SF_EXTRA;
#pragma unroll
  for (int k = 0; k < SF_REC_EXTRA; ++k) {
    if (c[k]) atomicAdd(ex + k, c[k]);
    c[k] = 0u;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * cells; i += blockDim.x) {
    const uint32_t v = h[i];
    if (v) { atomicAdd(grid + i, (unsigned long long)v); h[i] = 0u; }
  }
  if (staged) {
    for (int32_t j = threadIdx.x; j < tn; j += blockDim.x) {
      const uint32_t v = stage[j];
      if (v) { atomicMax(best_row + j, v); stage[j] = 0u; }
    }
  }
  if (threadIdx.x < SF_REC_EXTRA) {
    const uint32_t v = ex[threadIdx.x];
    if (v) { atomicAdd(extra + threadIdx.x, (unsigned long long)v); ex[threadIdx.x] = 0u; }
  }
  __syncthreads();
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte loads).
__global__ __launch_bounds__(256) void k_surface_records(SurfaceParams P) {
  extern __shared__ uint32_t sf_h[];   // [TP, FP][nq][na], SF_EXTRA extras, SF_STAGE staged codes
  const int cells = P.nq * P.na;
  const int lds_words = 2 * cells + SF_EXTRA + SF_STAGE;
  for (int i = threadIdx.x; i < lds_words; i += blockDim.x) sf_h[i] = 0u;
  __syncthreads();
  uint32_t* stage = sf_h + 2 * cells + SF_EXTRA;
  uint32_t c[SF_REC_EXTRA] = {0u, 0u, 0u};
  const float fa = (float)P.na;
  const int limit = P.nq * P.q_step;
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  int cur = -1;
  TruthDev T{};
  bool on = false, staged = false;
  uint32_t* best_row = nullptr;
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (cur >= 0) sf_flush(sf_h, c, cells, staged, (int32_t)T.n, P.grid + (int64_t)cur * SF_GRIDS * cells, P.extra + (int64_t)cur * SF_EXTRA, best_row);
      cur = sd.vcf;
      T = P.truths[sd.truth];
      on = P.has_af[cur] != 0;
      staged = T.n <= SF_STAGE;
      best_row = P.best + P.best_off[cur];
    }
    for (int64_t g = sd.begin + 4 * (int64_t)threadIdx.x; g < sd.end; g += 4 * (int64_t)blockDim.x) {
      const uint32_t valid = sd.end - g < 4 ? (1u << (uint32_t)(sd.end - g)) - 1u : 15u;   // records past the VCF's last are not defined
      const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));      // read once
      const qm_float4 q4 = __builtin_nontemporal_load(reinterpret_cast<const qm_float4*>(P.qual + g));
      const uint32_t ab4 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(P.anib + g));
      const uint32_t fl4 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(P.flags + g));
      qm_float4 f4 = {0.0f, 0.0f, 0.0f, 0.0f};
      if (on) f4 = __builtin_nontemporal_load(reinterpret_cast<const qm_float4*>(P.af + g));
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t anib = (ab4 >> (8 * k)) & 0xffu;
        if (!((valid >> k) & 1u) || (anib & ANIB_NONE)) continue;   // no record, or not a single-base one: counted nowhere
        const uint32_t fl = (fl4 >> (8 * k)) & 0xffu;
        const int b = sf_qual_bin(q4[k], limit);
        if (b < 0) { c[2] += 1u; continue; }
        const int qb = b / P.q_step;
        const float f = f4[k];
        const bool noaf = !on || f != f;
        int ab = 0;
        // min(na - 1, (int)(af * na)) with one float multiply, contracted with nothing; af >= 1 (+inf too) is the last bin either way
        if (!noaf && f >= 0.0f) ab = f >= 1.0f ? P.na - 1 : min(P.na - 1, (int)__fmul_rn(f, fa));
        c[0] += 1u;
        c[1] += noaf ? 1u : 0u;
        int32_t j = -1;
        if (!(fl & QMF_NOKEY)) {
          const uint32_t p = (uint32_t)p4[k];
          j = sf_find(T, p, (p << 4) | anib);
        }
        const bool hit = j >= 0 && (fl & QMF_IDDOT);
        const bool is_tp = hit || (fl & QMF_TPLINE);
        const int cell = qb * P.na + ab;
        atomicAdd(sf_h + (is_tp ? 0 : cells) + cell, 1u);
        if (hit) {
          const uint32_t code = 1u + (uint32_t)cell;
          if (staged) atomicMax(stage + j, code);
          else if (__hip_atomic_load(best_row + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < code) atomicMax(best_row + j, code);   // codes only rise: a stale look costs one spare atomic
        }
      }
    }
  }
  if (cur >= 0) sf_flush(sf_h, c, cells, staged, (int32_t)T.n, P.grid + (int64_t)cur * SF_GRIDS * cells, P.extra + (int64_t)cur * SF_EXTRA, best_row);
}

// grid (key chunks, VCF): the best codes of SF_TRUTH_CHUNK-strided keys into an LDS U grid, the non-zero cells out
__global__ __launch_bounds__(256) void k_surface_truth(SurfaceParams P) {
  extern __shared__ uint32_t sf_u[];   // [nq][na]
  const int cells = P.nq * P.na;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) sf_u[i] = 0u;
  __syncthreads();
  const int v = blockIdx.y;
  const int64_t off = P.best_off[v];
  const int64_t tn = P.best_off[v + 1] - off;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < tn; j += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t code = P.best[off + j];
    if (code != 0u && code <= (uint32_t)cells) atomicAdd(sf_u + (code - 1u), 1u);
  }
  __syncthreads();
  unsigned long long* u = P.grid + ((int64_t)v * SF_GRIDS + 2) * cells;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) {
    const uint32_t x = sf_u[i];
    if (x) atomicAdd(u + i, (unsigned long long)x);
  }
}

// One workgroup per (VCF, grid): S[i][k] = sum of the grid over qb >= i and ab >= k, in place, in u64.  Along AF one lane per
// QUAL row (nq <= 256), then along QUAL one lane per AF column (na <= 64).
__global__ __launch_bounds__(256) void k_surface_sums(SurfaceParams P) {
  extern __shared__ unsigned long long sf_s[];   // [nq][na]
  const int cells = P.nq * P.na;
  unsigned long long* g = P.grid + (int64_t)blockIdx.x * cells;
  for (int i = threadIdx.x; i < cells; i += blockDim.x) sf_s[i] = g[i];
  __syncthreads();
  for (int i = threadIdx.x; i < P.nq; i += blockDim.x) {
    unsigned long long run = 0;
    for (int k = P.na - 1; k >= 0; --k) { run += sf_s[i * P.na + k]; sf_s[i * P.na + k] = run; }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < P.na; k += blockDim.x) {
    unsigned long long run = 0;
    for (int i = P.nq - 1; i >= 0; --i) { run += sf_s[i * P.na + k]; sf_s[i * P.na + k] = run; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < cells; i += blockDim.x) g[i] = sf_s[i];
}

void launch_surface_records(const SurfaceParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  const size_t lds = sf_records_lds_words(P.nq * P.na) * sizeof(uint32_t);
  hipLaunchKernelGGL(k_surface_records, grid, dim3(256), lds, st, P);
}

void launch_surface_truth(const SurfaceParams& P, int n_vcf, int64_t max_tn, hipStream_t st) {
  if (n_vcf <= 0 || max_tn <= 0) return;
  const int64_t bx = std::min<int64_t>(64, std::max<int64_t>(1, (max_tn + SF_TRUTH_CHUNK - 1) / SF_TRUTH_CHUNK));
  const size_t lds = (size_t)P.nq * (size_t)P.na * sizeof(uint32_t);
  for (int v0 = 0; v0 < n_vcf; v0 += 65535) {   // (grid y holds 65 535 VCFs)
    SurfaceParams Q = P;
    Q.best_off += v0; Q.grid += (int64_t)v0 * SF_GRIDS * P.nq * P.na;
    hipLaunchKernelGGL(k_surface_truth, dim3((unsigned)bx, (unsigned)std::min(n_vcf - v0, 65535)), dim3(256), lds, st, Q);
  }
}

void launch_surface_sums(const SurfaceParams& P, int n_vcf, hipStream_t st) {
  if (n_vcf <= 0) return;
  const size_t lds = (size_t)P.nq * (size_t)P.na * sizeof(unsigned long long);
  hipLaunchKernelGGL(k_surface_sums, dim3((unsigned)n_vcf * SF_GRIDS), dim3(256), lds, st, P);
}

}  // namespace qm
