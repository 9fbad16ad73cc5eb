// qmvt_rroc.hip -- the QUAL ROC of a finished allele-extended batch under the two per-record rescue passes: by
// normal form (4.17) and by atoms (4.18).  k_rroc_records<MODE> streams the batch in input order and reads what the finished
// pass left -- the truth row of every record's form, or the hit masks beside the atom sets and the truth table --, adds the
// record to the TP or the FP histogram of its QUAL bin and raises the best bin of the truth-side units it carries;
// k_rroc_units<MODE> takes the histogram of the bests per VCF (by atoms: the minimum over an atomisable entry's atoms first) and
// turns the three rows into suffix sums.  Nothing is normalised or atomised again.  Integer work only: no output depends on the
// order the lanes run in.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the
// classification pass's profiles are keyed on.
#include "qmvt_rroc.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// floor(q) clamped to n_bins - 1; NaN and q < 0 give -1: the bin of the batch's own ROC
__device__ inline int rr_qual_bin(float q, int n_bins) {
  if (!(q >= 0.0f)) return -1;
  if (q >= (float)n_bins) return n_bins - 1;
  return (int)q;
}

// ---- what qmvt_atom.hip defines for its own kernels, restated: the set and the table are the ones that pass built ----
__device__ inline bool rr_inline(int32_t c) {
  const uint32_t u = (uint32_t)c;
  return u < 4u || (u - (2u << 26)) < (12u << 26);
}
__device__ inline uint32_t rr_len(int32_t c) { return (uint32_t)c < 4u ? 1u : (uint32_t)c >> 26; }
__device__ inline uint32_t rr_bits(int32_t c) { return (uint32_t)c & 0x03ffffffu; }
// whether (p, r, a) is atomisable, with m = its mismatch mask (bit 2 k: base k differs)
__device__ inline bool rr_atomisable(int32_t p, int32_t r, int32_t a, bool nokey, uint32_t& m) {
  m = 0u;
  if (!rr_inline(r) || !rr_inline(a) || nokey || r == a) return false;
  const uint32_t len = rr_len(r);
  if (len != rr_len(a)) return false;
  if (p < 0 || (uint32_t)p + len - 1u >= (1u << 28)) return false;
  const uint32_t d = rr_bits(r) ^ rr_bits(a);
  m = (d | d >> 1) & 0x1555555u & ((1u << (2u * len)) - 1u);
  return true;
}
// the atom at base offset k
__device__ inline uint32_t rr_atom(int32_t p, int32_t r, int32_t a, uint32_t k) {
  return (((uint32_t)p + k) << 4) | (((rr_bits(r) >> (2u * k)) & 3u) << 2) | ((rr_bits(a) >> (2u * k)) & 3u);
}
__device__ inline uint32_t rr_hash(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// the slot of an atom, or -1
__device__ inline int32_t rr_probe(const AtomTable& T, uint32_t key) {
  const uint32_t mask = T.slots - 1u;
  uint32_t h = rr_hash(key) & mask;
  for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
    const uint32_t k = T.set[h];
    if (k == key) return (int32_t)h;
    if (k == ATOM_EMPTY) return -1;
  }
  return -1;
}
// the index of the entry spelled (p, r, a) in the truth set's sorted table, or -1 (0 <= p < 2^28: the caller's duty)
__device__ inline int64_t rr_entry(const AtomTable& T, int32_t p, int32_t r, int32_t a) {
  const uint32_t key = ((uint32_t)p << 4) | allele_nib(r, a);
  int64_t lo = 0, hi = T.xn;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const uint32_t k = T.xkeys[mid];
    bool less = k < key;
    if (k == key) {
      const int32_t rr = T.xref[mid];
      less = rr < r || (rr == r && T.xalt[mid] < a);
    }
    if (less) lo = mid + 1; else hi = mid;
  }
  return lo < T.xn && T.xkeys[lo] == key && T.xref[lo] == r && T.xalt[lo] == a ? lo : -1;
}

// ---- best cells: 16 bits, two to a word ----
__device__ inline uint32_t rr_cell(const uint32_t* cells, int64_t i) { return (cells[i >> 1] >> (16u * (uint32_t)(i & 1))) & 0xffffu; }
// An atomic max on one half of a word: tried only while the half reads smaller than v, and the other half goes back as it was
// read with it, so a neighbour raised in between makes the exchange fail and is read again.  (The cells only grow within a call:
// a stale first read costs a round, never a lost update.)
__device__ inline void rr_raise(uint32_t* cells, int64_t i, uint32_t v) {
  uint32_t* w = cells + (i >> 1);
  const uint32_t sh = 16u * (uint32_t)(i & 1);
  uint32_t old = *w;
  while (((old >> sh) & 0xffffu) < v) {
    const uint32_t got = atomicCAS(w, old, (old & ~(0xffffu << sh)) | (v << sh));
    if (got == old) break;
    old = got;
  }
}

// The span walk of qmvt_walk.h, 4 records per lane (aligned 16-byte / 8-byte / 4-byte accesses).  The two histograms of the
// workgroup's VCF live in LDS and leave for the VCF's 64-bit rows when the VCF changes and at the end.
template <int MODE>
__global__ __launch_bounds__(256) void k_rroc_records(RrocRecParams P) {
  __shared__ uint32_t h[2 * RROC_MAX_BINS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records per workgroup: u32 suffices
  const int nb = P.n_bins;
  for (int i = (int)threadIdx.x; i < 2 * nb; i += (int)blockDim.x) h[i] = 0u;
  __syncthreads();
  RrocVcf V{};
  walk_spans<4>(
      P.spans, P.n_spans,
      [&](int vcf, const SpanDesc&) {
        V = P.vcfs[vcf];
        return MODE != RROC_N || V.best_n != nullptr;
      },
      [&](int vcf, const SpanDesc& sd, int64_t g) {
        if (g >= sd.end) return;
        const uint32_t live = rec_live<4>(g, sd.end);   // (columns past the VCF's last record are not defined)
        const qm_float4 q4 = __builtin_nontemporal_load(reinterpret_cast<const qm_float4*>(P.qual + g));   // read once
        const qm_int4 r4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.ref + g));
        const qm_int4 a4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.alt + g));
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
        qm_int4 x4 = {0, 0, 0, 0};          // normal form: the truth rows; atoms: the positions
        qm_uint2 m2 = {0u, 0u};             // atoms: the hit masks
        if (MODE == RROC_N) {
          x4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.nrow + g));
        } else {
          x4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));
          m2 = __builtin_nontemporal_load(reinterpret_cast<const qm_uint2*>(P.hit_mask + g));
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((live >> k) & 1u)) continue;
          const int32_t r = r4[k], a = a4[k];
          const int b = rr_qual_bin(q4[k], nb);
          if (b < 0 || !allele_valid(r) || !allele_valid(a)) continue;   // the universe of the batch's own ROC
          const uint32_t fl = (f4 >> (8 * k)) & 255u;
          const bool iddot = (fl & QMF_IDDOT) != 0u;
          bool hit;
          if (MODE == RROC_N) {
            const int32_t row = x4[k];
            hit = row >= 0 && (int64_t)row < V.xn;
            if (hit && iddot && rr_cell(V.best_n, row) < (uint32_t)b + 1u) rr_raise(V.best_n, row, (uint32_t)b + 1u);
          } else {
            const AtomTable& T = P.avcfs[vcf].t;
            const int32_t p = x4[k];
            const bool nokey = (fl & QMF_NOKEY) != 0u;
            uint32_t mm;
            if (rr_atomisable(p, r, a, nokey, mm)) {
              uint32_t hm = (m2[k >> 1] >> (16 * (k & 1))) & 0xffffu;
              hit = (uint32_t)__popc(hm) == (uint32_t)__popc(mm);
              if (iddot) {   // a carrier: every atom it hits, a partial record's too
                while (hm) {
                  const uint32_t o = (uint32_t)__builtin_ctz(hm);
                  hm &= hm - 1u;
                  const int32_t slot = rr_probe(T, rr_atom(p, r, a, o));   // (the producer found it: the probe succeeds)
                  if (slot >= 0 && rr_cell(V.best_atom, slot) < (uint32_t)b + 1u) rr_raise(V.best_atom, slot, (uint32_t)b + 1u);
                }
              }
            } else {
              const int64_t e = (!nokey && (uint32_t)p < (1u << 28)) ? rr_entry(T, p, r, a) : -1;
              hit = e >= 0;
              if (hit && iddot && rr_cell(V.best_entry, e) < (uint32_t)b + 1u) rr_raise(V.best_entry, e, (uint32_t)b + 1u);
            }
          }
          const bool tp = (hit && iddot) || (fl & QMF_TPLINE);
          atomicAdd(h + (tp ? 0 : nb) + b, 1u);
        }
      },
      [&](int vcf) { flush_counts(h, 2 * nb, reinterpret_cast<unsigned long long*>(P.hist) + (int64_t)vcf * 3 * nb); });
}

// A workgroup per VCF: the histogram of the bests of its units in LDS, then the suffix sums of the three rows in place (one lane
// per row: at most 256 steps), and the baseline beside them.
template <int MODE>
__global__ __launch_bounds__(256) void k_rroc_units(const RrocVcf* vcfs, const AtomVcf* avcfs, unsigned long long* hist, int nb,
                                                    unsigned long long* base, const unsigned long long* tru, int tru_cols, int tru_col) {
  __shared__ uint32_t u[RROC_MAX_BINS];   // at most 2^28 entries per truth set: u32 suffices
  const int v = (int)blockIdx.x;
  const RrocVcf V = vcfs[v];
  for (int i = (int)threadIdx.x; i < nb; i += (int)blockDim.x) u[i] = 0u;
  __syncthreads();
  const bool has = MODE == RROC_N ? V.best_n != nullptr : true;
  if (has) {
    for (int64_t j = threadIdx.x; j < V.xn; j += blockDim.x) {
      uint32_t c;
      if (MODE == RROC_N) {
        c = rr_cell(V.best_n, j);   // (only the cell of a form's smallest entry index is ever raised)
      } else {
        const AtomTable& T = avcfs[v].t;
        const int32_t p = (int32_t)(T.xkeys[j] >> 4), r = T.xref[j], a = T.xalt[j];
        uint32_t mm;
        if (rr_atomisable(p, r, a, false, mm)) {
          c = 0xffffu;
          while (mm) {
            const uint32_t o = (uint32_t)__builtin_ctz(mm) >> 1;
            mm &= mm - 1u;
            const int32_t slot = rr_probe(T, rr_atom(p, r, a, o));
            c = min(c, slot >= 0 ? rr_cell(V.best_atom, slot) : 0u);
          }
          if (c == 0xffffu) c = 0u;   // (no atom: cannot happen, REF != ALT)
        } else {
          c = rr_cell(V.best_entry, j);
        }
      }
      if (c && c <= (uint32_t)nb) atomicAdd(u + (c - 1u), 1u);
    }
  }
  __syncthreads();
  unsigned long long* row = hist + (int64_t)v * 3 * nb;
  if (threadIdx.x < 3) {
    unsigned long long* o = row + (int64_t)threadIdx.x * nb;
    unsigned long long run = 0;
    for (int b = nb - 1; b >= 0; --b) {
      run += threadIdx.x == 2 ? (unsigned long long)u[b] : o[b];
      o[b] = run;
    }
  }
  if (threadIdx.x == 3) base[(int64_t)v * 2 + MODE] = has ? tru[(int64_t)v * tru_cols + tru_col] : 0ull;
}

void launch_rroc_records(int mode, const RrocRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  if (mode == RROC_N) hipLaunchKernelGGL(k_rroc_records<RROC_N>, grid, dim3(256), 0, st, P);
  else hipLaunchKernelGGL(k_rroc_records<RROC_A>, grid, dim3(256), 0, st, P);
}

void launch_rroc_units(int mode, const RrocVcf* vcfs, const AtomVcf* avcfs, int n_vcf, uint64_t* hist, int n_bins, uint64_t* base,
                       const uint64_t* tru, int tru_cols, int tru_col, hipStream_t st) {
  if (n_vcf <= 0) return;
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  unsigned long long* bs = reinterpret_cast<unsigned long long*>(base);
  const unsigned long long* t = reinterpret_cast<const unsigned long long*>(tru);
  if (mode == RROC_N) hipLaunchKernelGGL(k_rroc_units<RROC_N>, dim3((unsigned)n_vcf), dim3(256), 0, st, vcfs, avcfs, h, n_bins, bs, t, tru_cols, tru_col);
  else hipLaunchKernelGGL(k_rroc_units<RROC_A>, dim3((unsigned)n_vcf), dim3(256), 0, st, vcfs, avcfs, h, n_bins, bs, t, tru_cols, tru_col);
}

}  // namespace qm
