// qmvt_ltypes.hip -- the match ladder per variant type and size: the rows of the type pass (4.19) crossed with
// the 18 columns of the ladder (4.23).  k_ltype_records streams the row byte the type pass and the mask byte the ladder left of
// every record -- two bytes per record, nothing else -- and counts the kept records per (row, column); k_ltype_truth types every
// entry of a VCF's truth set as k_type_truth does (vt_row, qmvt_types.h) and counts it under its entry byte.  Nothing is
// normalised, atomised, replayed or typed by new rules.  Integer work only: no output depends on the order the lanes run in.
// Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's profiles are
// keyed on.
#include "qmvt_ltypes.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// A lane adds a run of equal (row, column) pairs among its 16 records with one LDS atomic ("measured": 2.4 times
// faster than an atomic per kept record on the synthetic batch).  A/B switch: 0 = one LDS atomic per kept record
#ifndef QM_LTYPE_MERGE
#define QM_LTYPE_MERGE 1
#endif

// the column of a mask byte that is not zero, less one (KEPT / ENTRIES is formed at the flush): TP / FOUND, else the cell of its
// low four bits
__device__ __forceinline__ uint32_t lt_col(uint32_t byte) { return (byte & LADDER_S) ? 1u : 2u + (byte & 15u); }

// Column 0 of every row from its other 17 cells, then the rows to the VCF's block.  Uniform over the workgroup.
__device__ inline void lt_flush(uint32_t* hist, int n_rows, uint64_t* out) {
  __syncthreads();
  for (int r = threadIdx.x; r < n_rows; r += blockDim.x) {
    uint32_t sum = 0u;
    for (int c = 1; c < LADDER_COLS; ++c) sum += hist[r * LADDER_COLS + c];
    hist[r * LADDER_COLS] = sum;
  }
  flush_counts(hist, n_rows * LADDER_COLS, reinterpret_cast<unsigned long long*>(out));
}

// One workgroup per PASS_SPANS consecutive spans (walk_spans), lane t takes 16 records per step: one 16-byte load of their row
// bytes, one of their mask bytes.  A zero mask byte is a record that is not kept; what lies behind the VCF's last record is
// masked out (rec_live: the bytes there are not defined).  A kept record adds one to its (row, column) cell of the workgroup's
// LDS histogram -- MERGE: a run of records of one cell adds its length --; the histogram goes to the VCF's block when the VCF
// changes and at the end.
template <bool MERGE>
__global__ __launch_bounds__(256) void k_ltype_records(LtypeRecParams P) {
  __shared__ uint32_t hist[LTYPE_LDS_WORDS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records per workgroup: u32 suffices
  for (int i = threadIdx.x; i < LTYPE_LDS_WORDS; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  const uint32_t n_rows = (uint32_t)P.n_rows;
  walk_spans<16>(
      P.spans, P.n_spans, [&](int, const SpanDesc&) { return true; },
      [&](int, const SpanDesc& sd, int64_t g) {
        if (g >= sd.end) return;   // (no wave-wide operation below)
        const uint32_t live = rec_live<16>(g, sd.end);
        const qm_uint4 m16 = __builtin_nontemporal_load(reinterpret_cast<const qm_uint4*>(P.mask + g));   // read once
        if (live == 0xffffu && (m16[0] | m16[1] | m16[2] | m16[3]) == 0u) return;                         // none of the 16 is kept
        const qm_uint4 r16 = __builtin_nontemporal_load(reinterpret_cast<const qm_uint4*>(P.row + g));
        uint32_t prev = ~0u, run = 0u;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const uint32_t byte = (m16[k >> 2] >> (8 * (k & 3))) & 255u, row = (r16[k >> 2] >> (8 * (k & 3))) & 255u;
          if (!((live >> k) & 1u) || byte == 0u || row >= n_rows) continue;   // (a row byte is below n_rows: the guard keeps a stray one out of LDS)
          const uint32_t cell = row * LADDER_COLS + lt_col(byte);
          if (!MERGE) {
            atomicAdd(hist + cell, 1u);
          } else if (cell == prev) {
            ++run;
          } else {
            if (run) atomicAdd(hist + prev, run);
            prev = cell;
            run = 1u;
          }
        }
        if (MERGE && run) atomicAdd(hist + prev, run);
      },
      [&](int vcf) { lt_flush(hist, P.n_rows, P.rec + (int64_t)vcf * P.n_rows * LADDER_COLS); });
}

// grid (x, VCF), a lane per entry of the VCF's truth set: its row as k_type_truth finds it, its entry byte
__global__ __launch_bounds__(256) void k_ltype_truth(LtypeTruthParams P) {
  __shared__ uint32_t hist[LTYPE_LDS_WORDS];
  for (int i = threadIdx.x; i < LTYPE_LDS_WORDS; i += blockDim.x) hist[i] = 0u;
  __syncthreads();
  const TypeVcf& V = P.tvcfs[blockIdx.y];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < V.xn) {
    const uint32_t row = vt_row(V.xref[j], V.xalt[j], false, P.shapes, P.bins);
    const uint32_t byte = P.emask[P.lvcfs[blockIdx.y].eoff + j];
    atomicAdd(hist + row * LADDER_COLS + lt_col(byte), 1u);
  }
  lt_flush(hist, P.bins.n_rows, P.tru + (int64_t)blockIdx.y * P.bins.n_rows * LADDER_COLS);
}

void launch_ltype_records(const LtypeRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_ltype_records<QM_LTYPE_MERGE != 0>, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_ltype_truth(const LtypeTruthParams& P, int n_vcf, int64_t max_entries, hipStream_t st) {
  if (max_entries <= 0) return;
  const unsigned gx = (unsigned)((max_entries + 255) / 256);
  for (int v0 = 0; v0 < n_vcf; v0 += 65535) {   // (the y dimension of a grid holds 65535 blocks)
    const int nv = std::min(n_vcf - v0, 65535);
    LtypeTruthParams Q = P;
    Q.tvcfs = P.tvcfs + v0;
    Q.lvcfs = P.lvcfs + v0;
    Q.tru = P.tru + (int64_t)v0 * P.bins.n_rows * LADDER_COLS;
    hipLaunchKernelGGL(k_ltype_truth, dim3(gx, (unsigned)nv), dim3(256), 0, st, Q);
  }
}

}  // namespace qm
