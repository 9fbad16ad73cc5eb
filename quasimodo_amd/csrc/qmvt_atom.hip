// qmvt_atom.hip -- MNPs matched against adjacent SNVs: every equal-length substitution with inline allele codes
// is split into its single-base atoms (pos << 4 | ref << 2 | alt, one 32-bit word), on both sides.  k_atom_truth puts the atoms
// of a truth set's allele-extended entries into an open-addressing set, k_atom_records streams the finished batch in input
// order, probes every record's atoms in its VCF's set and counts, k_atom_found asks per truth entry whether all its atoms were
// carried by kept records.  Integer work only: no output depends on the order the lanes run in.  Its own translation unit:
// qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's profiles are keyed on.
#include "qmvt_atom.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// inline codes (include/qmvt.h): 0 .. 3 one base, len << 26 | bases for 2 .. 13 bases
__device__ inline bool at_inline(int32_t c) {
  const uint32_t u = (uint32_t)c;
  return u < 4u || (u - (2u << 26)) < (12u << 26);
}
__device__ inline uint32_t at_len(int32_t c) { return (uint32_t)c < 4u ? 1u : (uint32_t)c >> 26; }
__device__ inline uint32_t at_bits(int32_t c) { return (uint32_t)c & 0x03ffffffu; }

// 0 for an atomisable variant, with m = its mismatch mask (bit 2 k: base k differs); else the first reason that applies
__device__ inline uint32_t at_reason(int32_t p, int32_t r, int32_t a, bool nokey, uint32_t& m) {
  m = 0u;
  if (!at_inline(r) || !at_inline(a)) return ATOM_LONG;
  if (nokey) return ATOM_NOKEY;
  if (r == a) return ATOM_NOVAR;
  const uint32_t len = at_len(r);
  if (len != at_len(a)) return ATOM_UNEQUAL;
  if (p < 0 || (uint32_t)p + len - 1u >= (1u << 28)) return ATOM_RANGE;
  const uint32_t d = at_bits(r) ^ at_bits(a);
  m = (d | d >> 1) & 0x1555555u & ((1u << (2u * len)) - 1u);
  return 0u;
}
// the atom at the lowest set bit of m, which is cleared; k = its offset
__device__ inline uint32_t at_next(uint32_t& m, int32_t p, int32_t r, int32_t a, uint32_t& k) {
  const uint32_t sh = (uint32_t)__builtin_ctz(m);
  m &= m - 1u;
  k = sh >> 1;
  return (((uint32_t)p + k) << 4) | (((at_bits(r) >> sh) & 3u) << 2) | ((at_bits(a) >> sh) & 3u);
}

__device__ inline uint32_t at_hash(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// the slot of an atom, or -1 (the set has empty slots: at most slots / 2 are claimed)
__device__ inline int32_t at_probe(const AtomTable& T, uint32_t key) {
  const uint32_t mask = T.slots - 1u;
  uint32_t h = at_hash(key) & mask;
  for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
    const uint32_t k = T.set[h];
    if (k == key) return (int32_t)h;
    if (k == ATOM_EMPTY) return -1;
  }
  return -1;
}

// the index of the entry spelled (p, r, a) in the truth set's sorted table, or -1 (0 <= p < 2^28: the caller's duty)
__device__ inline int64_t at_entry(const AtomTable& T, int32_t p, int32_t r, int32_t a) {
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

__device__ inline uint32_t at_wave_sum(uint32_t x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o);
  return x;   // (lane 0 holds the sum)
}

// a lane per entry: how many atoms the atomisable entries have together, repeats included
__global__ __launch_bounds__(256) void k_atom_count(AtomTable T, unsigned long long* total) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t m = 0u;
  if (j < T.xn) (void)at_reason((int32_t)(T.xkeys[j] >> 4), T.xref[j], T.xalt[j], false, m);
  const uint32_t n = at_wave_sum((uint32_t)__popc(m));
  if ((threadIdx.x & 63u) == 0u && n) atomicAdd(total, (unsigned long long)n);
}

// a lane per entry: every atom of an atomisable entry claims its slot, or finds it claimed by an equal atom.  The lanes of a
// wave walk their mismatch masks together, so that the claims are counted by ballots.
__global__ __launch_bounds__(256) void k_atom_truth(AtomTable T) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t p = 0, r = 0, a = 0;
  uint32_t m = 0u;
  bool ok = false;
  if (j < T.xn) {
    p = (int32_t)(T.xkeys[j] >> 4); r = T.xref[j]; a = T.xalt[j];
    ok = at_reason(p, r, a, false, m) == 0u;
  }
  const uint32_t mask = T.slots - 1u;
  uint32_t n_new = 0u;   // (uniform over the wave)
  while (__ballot(m != 0u)) {
    bool claimed = false;
    if (m) {
      uint32_t k;
      const uint32_t key = at_next(m, p, r, a, k);
      uint32_t h = at_hash(key) & mask;
      for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
        const uint32_t old = atomicCAS(T.set + h, ATOM_EMPTY, key);
        claimed = old == ATOM_EMPTY;
        if (claimed || old == key) break;
      }
    }
    n_new += (uint32_t)__popcll(__ballot(claimed));
  }
  const uint64_t mo = __ballot(ok);
  if ((threadIdx.x & 63u) == 0u) {
    if (n_new) atomicAdd(T.stats, (unsigned long long)n_new);
    if (mo) atomicAdd(T.stats + 1, (unsigned long long)__popcll(mo));
  }
}

// The span walk written out (through walk_spans this kernel measured slower than its own frame, LABNOTES round 29).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 4 t + 1024 i .. + 3 (every span starts at a multiple of 256 records: aligned 16-byte / 4-byte accesses).  Every lane stays
// in the loop for all of a span's steps: the wave's ballots need them together.  The counters are wave-uniform registers (the
// two atom sums: one register per lane, reduced over the wave at the flush), added to LDS and from there to the VCF's row when
// the VCF changes.
__global__ __launch_bounds__(256) void k_atom_records(AtomRecParams P) {
  __shared__ uint32_t cnt[ATOM_R_COLS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records of at most 13 atoms per workgroup: u32 suffices
  if (threadIdx.x < ATOM_R_COLS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  uint32_t acc[ATOM_R_COLS];
#pragma unroll
  for (int c = 0; c < ATOM_R_COLS; ++c) acc[c] = 0u;
  uint32_t sum_a = 0u, sum_h = 0u;   // this lane's atoms and hit atoms
  int cur = -1;
  auto flush = [&]() {   // (uniform over the workgroup)
    acc[ATOM_R_ATOMS] = at_wave_sum(sum_a);
    acc[ATOM_R_ATOMS_HIT] = at_wave_sum(sum_h);
    sum_a = sum_h = 0u;
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < ATOM_R_COLS; ++c)
        if (acc[c]) atomicAdd(cnt + c, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < ATOM_R_COLS; ++c) acc[c] = 0u;
    flush_counts(cnt, ATOM_R_COLS, reinterpret_cast<unsigned long long*>(P.rec + (int64_t)cur * ATOM_R_COLS));
  };
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (cur >= 0) flush();
      cur = sd.vcf;
    }
    const AtomVcf& V = P.vcfs[cur];
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 4 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 4 * (int64_t)threadIdx.x;
      uint32_t m[4] = {0u, 0u, 0u, 0u};   // bit c: the record counts in column c (but the two atom sums)
      if (g < sd.end) {
        const uint32_t nrec = (uint32_t)min((int64_t)4, sd.end - g);   // (bits and columns past the VCF's last record are not defined)
        const uint32_t kb = (uint32_t)(P.mask_pass[g >> 6] >> (int)(g & 63)) & 15u;
        const uint32_t tb = (uint32_t)(P.mask_tp[g >> 6] >> (int)(g & 63)) & 15u;
        const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
        const qm_int4 r4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.ref + g));
        const qm_int4 a4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.alt + g));
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
        uint32_t c4 = 0u, n4 = 0u;
        qm_uint2 h4 = {0u, 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if ((uint32_t)k >= nrec) continue;
          const uint32_t fl = (f4 >> (8 * k)) & 255u;
          const bool kept = (kb >> k) & 1u, tp = (tb >> k) & 1u, nokey = (fl & QMF_NOKEY) != 0u;
          const int32_t p = p4[k], r = r4[k], a = a4[k];
          uint32_t mm;
          const uint32_t why = at_reason(p, r, a, nokey, mm);
          const bool ok = why == 0u;
          const uint32_t na = (uint32_t)__popc(mm);
          uint32_t hm = 0u;
          while (mm) {
            uint32_t o;
            const uint32_t key = at_next(mm, p, r, a, o);
            const int32_t slot = at_probe(V.t, key);
            if (slot < 0) continue;
            hm |= 1u << o;
            const uint32_t w = (uint32_t)slot >> 5, bit = 1u << ((uint32_t)slot & 31u);
            if (kept && !(V.abits[w] & bit)) atomicOr(V.abits + w, bit);   // (a stale read only repeats the atomic)
          }
          const uint32_t nh = (uint32_t)__popc(hm);
          // an entry spelled like the record: an atomisable entry has all its atoms in the set
          if (kept && !nokey && (ok ? nh == na : (allele_valid(r) && allele_valid(a) && (uint32_t)p < (1u << 28)))) {
            const int64_t e = at_entry(V.t, p, r, a);
            if (e >= 0) {
              const uint32_t bit = 1u << ((uint32_t)e & 31u);
              if (!(V.ebits[e >> 5] & bit)) atomicOr(V.ebits + (e >> 5), bit);
            }
          }
          const bool tp_a = ok ? kept && ((nh == na && (fl & QMF_IDDOT)) || (fl & QMF_TPLINE)) : tp;
          const bool rescued = tp_a && !tp;
          const uint32_t c = rescued ? ATOM_RESCUED : !ok ? why : nh == na ? ATOM_FULL : nh ? ATOM_PARTIAL : ATOM_NONE;
          c4 |= c << (8 * k);
          n4 |= (ok ? na : 0u) << (8 * k);
          h4[k >> 1] |= hm << (16 * (k & 1));
          if (kept) {
            uint32_t mk = 1u | (tp ? 2u : 0u) | (tp_a ? 4u : 0u) | (rescued ? 8u : 0u);
            if (ok) {
              mk |= (na >= 2u ? 16u : 0u) | (nh > 0u && nh < na ? 32u : 0u);
              sum_a += na;
              sum_h += nh;
            } else {
              mk |= 1u << ((uint32_t)ATOM_R_LONG + why - ATOM_LONG);
            }
            m[k] = mk;
          }
        }
        if (P.cls) {
          *reinterpret_cast<uint32_t*>(P.cls + g) = c4;
          *reinterpret_cast<uint32_t*>(P.n_atoms + g) = n4;
          *reinterpret_cast<qm_uint2*>(P.hit_mask + g) = h4;
        }
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (!__ballot(m[k] != 0u)) continue;   // (uniform over the wave)
#pragma unroll
        for (int c = 0; c < ATOM_R_COLS; ++c)
          if (c != ATOM_R_ATOMS && c != ATOM_R_ATOMS_HIT) acc[c] += (uint32_t)__popcll(__ballot((m[k] >> c) & 1u));
      }
    }
  }
  if (cur >= 0) flush();
}

// grid (x, VCF), a lane per entry of the VCF's truth set and per word of its atom bitmap
__global__ __launch_bounds__(256) void k_atom_found(const AtomVcf* vcfs, unsigned long long* tru) {
  const AtomVcf& V = vcfs[blockIdx.y];
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool found = false, found_a = false;
  if (j < V.t.xn) {
    found = (V.ebits[j >> 5] >> ((uint32_t)j & 31u)) & 1u;
    const int32_t p = (int32_t)(V.t.xkeys[j] >> 4), r = V.t.xref[j], a = V.t.xalt[j];
    uint32_t mm;
    if (at_reason(p, r, a, false, mm) == 0u) {
      found_a = true;
      while (mm) {
        uint32_t o;
        const int32_t slot = at_probe(V.t, at_next(mm, p, r, a, o));
        found_a = found_a && slot >= 0 && ((V.abits[(uint32_t)slot >> 5] >> ((uint32_t)slot & 31u)) & 1u);
      }
    } else {
      found_a = found;
    }
  }
  const uint32_t n_bits = at_wave_sum(j < (int64_t)(V.t.slots / 32u) ? (uint32_t)__popc(V.abits[j]) : 0u);
  const uint64_t mf = __ballot(found), ma = __ballot(found_a);
  unsigned long long* o = tru + (int64_t)blockIdx.y * ATOM_T_COLS;
  if ((threadIdx.x & 63u) == 0u) {
    if (n_bits) atomicAdd(o + 3, (unsigned long long)n_bits);
    if (mf) atomicAdd(o + 4, (unsigned long long)__popcll(mf));
    if (ma) atomicAdd(o + 5, (unsigned long long)__popcll(ma));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    o[0] = (unsigned long long)V.t.xn;
    o[1] = V.t.stats[1];
    o[2] = V.t.stats[0];
  }
}

void launch_atom_count(const AtomTable& T, unsigned long long* total, hipStream_t st) {
  if (T.xn <= 0) return;
  hipLaunchKernelGGL(k_atom_count, dim3((unsigned)((T.xn + 255) / 256)), dim3(256), 0, st, T, total);
}

void launch_atom_truth(const AtomTable& T, hipStream_t st) {
  if (T.xn <= 0) return;
  hipLaunchKernelGGL(k_atom_truth, dim3((unsigned)((T.xn + 255) / 256)), dim3(256), 0, st, T);
}

void launch_atom_records(const AtomRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  const dim3 grid(pass_grid(P.n_spans));
  hipLaunchKernelGGL(k_atom_records, grid, dim3(256), 0, st, P);
}

void launch_atom_found(const AtomVcf* vcfs, int n_vcf, int64_t max_lanes, uint64_t* tru, hipStream_t st) {
  const unsigned gx = (unsigned)((std::max<int64_t>(max_lanes, 1) + 255) / 256);
  for (int v0 = 0; v0 < n_vcf; v0 += 65535) {   // (the y dimension of a grid holds 65535 blocks)
    const int nv = std::min(n_vcf - v0, 65535);
    hipLaunchKernelGGL(k_atom_found, dim3(gx, (unsigned)nv), dim3(256), 0, st, vcfs + v0, reinterpret_cast<unsigned long long*>(tru) + (int64_t)v0 * ATOM_T_COLS);
  }
}

}  // namespace qm
