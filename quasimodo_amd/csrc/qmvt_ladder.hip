// qmvt_ladder.hip -- the four rescues of a finished allele-extended batch combined: by normal form (4.17), by
// atoms (4.18), by replayed haplotype (4.20) and by a subset of a mismatched site (4.21).  k_ladder_records streams the class
// bytes the four passes left beside the flag bytes and the two record masks, gives every record one mask byte and counts the
// kept lines that are no TP by spelling in the 16 cells of the four method bits; k_ladder_truth does the same for every (VCF,
// truth entry) from the passes' found bitmaps and entry classes.  Nothing is normalised, atomised or replayed again.  Integer
// work only: no output depends on the order the lanes run in.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip +
// qmvt_dev.h) stays the id the classification pass's profiles are keyed on.
#include "qmvt_ladder.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// 16 bytes of a column; a lane at its VCF's tail reads the nrec < 16 bytes the VCF has, one by one
__device__ inline qm_uint4 ld_load16(const uint8_t* p, uint32_t nrec) {
  if (nrec >= 16u) return __builtin_nontemporal_load(reinterpret_cast<const qm_uint4*>(p));   // read once
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t k = 0; k < 16u; ++k)
    if (k < nrec) w[k >> 2] |= (uint32_t)p[k] << (8u * (k & 3u));
  qm_uint4 v = {w[0], w[1], w[2], w[3]};
  return v;
}

// ---- what qmvt_norm.hip and qmvt_atom.hip define for their own kernels, restated: the tables are the ones those passes built ----
__device__ inline uint32_t ld_form_hash(int32_t p, int32_t r, int32_t a) {
  uint32_t x = (uint32_t)p * 0x9e3779b1u ^ (uint32_t)r * 0x85ebca77u ^ (uint32_t)a * 0xc2b2ae3du;
  x ^= x >> 15; x *= 0x2c1b3c6du;
  x ^= x >> 12; x *= 0x297a2d39u;
  x ^= x >> 15;
  return x;
}
// the slot of form (p, r, a), or -1
__device__ inline int32_t ld_form_probe(const NormTable& T, int32_t p, int32_t r, int32_t a) {
  const uint32_t mask = T.slots - 1u;
  uint32_t h = ld_form_hash(p, r, a) & mask;
  for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
    if (T.claim[h] == 0u) return -1;
    if (T.spos[h] == p && T.sref[h] == r && T.salt[h] == a) return (int32_t)h;
  }
  return -1;
}
__device__ inline bool ld_inline(int32_t c) {
  const uint32_t u = (uint32_t)c;
  return u < 4u || (u - (2u << 26)) < (12u << 26);
}
__device__ inline uint32_t ld_len(int32_t c) { return (uint32_t)c < 4u ? 1u : (uint32_t)c >> 26; }
__device__ inline uint32_t ld_bits(int32_t c) { return (uint32_t)c & 0x03ffffffu; }
// whether the entry (p, r, a) is atomisable, with m = its mismatch mask (bit 2 k: base k differs)
__device__ inline bool ld_atomisable(int32_t p, int32_t r, int32_t a, uint32_t& m) {
  m = 0u;
  if (!ld_inline(r) || !ld_inline(a) || r == a) return false;
  const uint32_t len = ld_len(r);
  if (len != ld_len(a)) return false;
  if (p < 0 || (uint32_t)p + len - 1u >= (1u << 28)) return false;
  const uint32_t d = ld_bits(r) ^ ld_bits(a);
  m = (d | d >> 1) & 0x1555555u & ((1u << (2u * len)) - 1u);
  return true;
}
__device__ inline uint32_t ld_atom(int32_t p, int32_t r, int32_t a, uint32_t k) {
  return (((uint32_t)p + k) << 4) | (((ld_bits(r) >> (2u * k)) & 3u) << 2) | ((ld_bits(a) >> (2u * k)) & 3u);
}
__device__ inline uint32_t ld_atom_hash(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// the slot of an atom, or -1
__device__ inline int32_t ld_atom_probe(const AtomTable& T, uint32_t key) {
  const uint32_t mask = T.slots - 1u;
  uint32_t h = ld_atom_hash(key) & mask;
  for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
    const uint32_t k = T.set[h];
    if (k == key) return (int32_t)h;
    if (k == ATOM_EMPTY) return -1;
  }
  return -1;
}

// The span walk written out (through walk_spans the register counts of this kernel end up in scratch memory).
// One workgroup per PASS_SPANS consecutive spans of the batch layout (a span never crosses a VCF); lane t takes records
// begin + 16 t + 4096 i .. + 15 (every span starts at a multiple of 256 records: aligned 16-byte loads, and the 16 bits of either
// record mask sit in one word).  Every lane counts its own records by popcounts of 16-bit masks, in registers; the counts go to
// the LDS histogram and from there to the VCF's 64-bit row when the VCF changes and at the end.
__global__ __launch_bounds__(256) void k_ladder_records(LadderRecParams P) {
  __shared__ uint32_t cnt[LADDER_COLS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records per workgroup: u32 suffices
  if (threadIdx.x < LADDER_COLS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int s0 = blockIdx.x * PASS_SPANS;
  const int s1 = min(s0 + PASS_SPANS, P.n_spans);
  uint32_t acc[LADDER_COLS];
#pragma unroll
  for (int c = 0; c < LADDER_COLS; ++c) acc[c] = 0u;
  int cur = -1;
  auto flush = [&]() {   // (uniform over the workgroup)
#pragma unroll
    for (int c = 0; c < LADDER_COLS; ++c) {
      if (acc[c]) atomicAdd(cnt + c, acc[c]);
      acc[c] = 0u;
    }
    flush_counts(cnt, LADDER_COLS, reinterpret_cast<unsigned long long*>(P.rec + (int64_t)cur * LADDER_COLS));
  };
  for (int s = s0; s < s1; ++s) {
    const SpanDesc sd = P.spans[s];
    if (sd.vcf != cur) {
      if (cur >= 0) flush();
      cur = sd.vcf;
    }
    const uint32_t has = P.vcfs[cur].has;
    const bool sub = P.cls_b != nullptr;
    for (int64_t g0 = sd.begin; g0 < sd.end; g0 += 16 * (int64_t)blockDim.x) {
      const int64_t g = g0 + 16 * (int64_t)threadIdx.x;
      if (g >= sd.end) continue;
      const uint32_t nrec = (uint32_t)min((int64_t)16, sd.end - g);   // (bits and columns past the VCF's last record are not defined)
      const uint32_t live = (1u << nrec) - 1u;
      const uint32_t kb = (uint32_t)(P.mask_pass[g >> 6] >> (int)(g & 63)) & live;
      const uint32_t tb = (uint32_t)(P.mask_tp[g >> 6] >> (int)(g & 63)) & kb;
      const qm_uint4 f16 = ld_load16(P.flags + g, nrec);
      const qm_uint4 n16 = ld_load16(P.cls_n + g, nrec);
      const qm_uint4 a16 = ld_load16(P.cls_a + g, nrec);
      const qm_uint4 h16 = ld_load16(P.cls_h + g, nrec);
      qm_uint4 b16 = {0u, 0u, 0u, 0u};
      if (sub) b16 = ld_load16(P.cls_b + g, nrec);
      uint32_t mN = 0u, mA = 0u, mH = 0u, mB = 0u, mI = 0u;   // bit k: record k has the class, or QMF_IDDOT
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const int w = k >> 2, sh = 8 * (k & 3);
        mI |= (((f16[w] >> sh) & QMF_IDDOT) ? 1u : 0u) << k;
        mN |= ((((n16[w] >> sh) & 255u) == NORM_RESCUED) ? 1u : 0u) << k;
        mA |= ((((a16[w] >> sh) & 255u) == ATOM_RESCUED) ? 1u : 0u) << k;
        mH |= ((((h16[w] >> sh) & 255u) == HAP_RESCUED) ? 1u : 0u) << k;
        mB |= ((((b16[w] >> sh) & 255u) == HAP_SUBSET) ? 1u : 0u) << k;
      }
      const uint32_t open = kb & ~tb;   // the kept lines that are no TP by spelling
      mN &= (has & LADDER_HAS_NORM) ? kb : 0u;
      mA &= kb;
      mH &= (has & LADDER_HAS_HAP) ? (open & mI) : 0u;
      mB &= (sub && (has & LADDER_HAS_HAP)) ? (open & mI) : 0u;
      acc[0] += (uint32_t)__popc(kb);
      acc[1] += (uint32_t)__popc(tb);
      if (((mN | mA | mH | mB) & open) == 0u) {
        acc[2] += (uint32_t)__popc(open);
      } else {
#pragma unroll
        for (uint32_t m = 0; m < 16u; ++m)
          acc[2 + m] += (uint32_t)__popc(open & ((m & LADDER_N) ? mN : ~mN) & ((m & LADDER_A) ? mA : ~mA) & ((m & LADDER_H) ? mH : ~mH) &
                                         ((m & LADDER_B) ? mB : ~mB));
      }
      if (P.mask) {
        uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
          const uint32_t byte = ((kb >> k) & 1u) * LADDER_K | ((tb >> k) & 1u) * LADDER_S | ((mN >> k) & 1u) * LADDER_N | ((mA >> k) & 1u) * LADDER_A |
                                ((mH >> k) & 1u) * LADDER_H | ((mB >> k) & 1u) * LADDER_B;
          o[k >> 2] |= byte << (8 * (k & 3));
        }
        if (nrec >= 16u) {
          const qm_uint4 v = {o[0], o[1], o[2], o[3]};
          *reinterpret_cast<qm_uint4*>(P.mask + g) = v;
        } else {
#pragma unroll
          for (uint32_t k = 0; k < 16u; ++k)
            if (k < nrec) P.mask[g + k] = (uint8_t)(o[k >> 2] >> (8u * (k & 3u)));
        }
      }
    }
  }
  if (cur >= 0) flush();
}

// A lane per (VCF, truth entry), blockIdx.y = the VCF: the entry's five bits from what the passes left -- the spelled-alike
// bitmap, the found bit of its form's slot, the carried bits of its atoms' slots, the two entry classes --, counted per wave by
// ballots into the LDS histogram and from there into the VCF's 64-bit row.
__global__ __launch_bounds__(256) void k_ladder_truth(LadderTruthParams P) {
  __shared__ uint32_t cnt[LADDER_COLS];
  if (threadIdx.x < LADDER_COLS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int v = (int)blockIdx.y;
  const LadderVcf L = P.vcfs[v];
  const AtomVcf& A = P.avcfs[v];
  const NormVcf& N = P.nvcfs[v];
  const HapVcf& H = P.hvcfs[v];
  const int64_t xn = A.t.xn;
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if ((int64_t)blockIdx.x * blockDim.x >= xn) return;   // (uniform over the workgroup)
  const bool live = j < xn;
  uint32_t byte = 0u;
  if (live) {
    if ((A.ebits[j >> 5] >> (uint32_t)(j & 31)) & 1u) byte |= LADDER_S;
    if ((L.has & LADDER_HAS_NORM) && N.t.words) {
      const int32_t slot = ld_form_probe(N.t, N.t.fpos[j], N.t.fref[j], N.t.falt[j]);   // (the pass inserted it: the probe succeeds)
      if (slot >= 0 && ((N.found[(uint32_t)slot >> 5] >> ((uint32_t)slot & 31u)) & 1u)) byte |= LADDER_N;
    }
    const int32_t p = (int32_t)(A.t.xkeys[j] >> 4), r = A.t.xref[j], a = A.t.xalt[j];
    uint32_t mm;
    if (ld_atomisable(p, r, a, mm)) {
      bool all = mm != 0u;
      while (mm && all) {
        const uint32_t o = (uint32_t)__builtin_ctz(mm) >> 1;
        mm &= mm - 1u;
        const int32_t slot = ld_atom_probe(A.t, ld_atom(p, r, a, o));
        all = slot >= 0 && ((A.abits[(uint32_t)slot >> 5] >> ((uint32_t)slot & 31u)) & 1u);
      }
      if (all) byte |= LADDER_A;
    }
    if ((L.has & LADDER_HAS_HAP) && H.ecls) {
      if (H.ecls[j] == HAP_RESCUED) byte |= LADDER_H;
      if (P.ecls_b && P.ecls_b[L.heoff + j] == HAP_SUBSET) byte |= LADDER_B;
    }
    if (P.emask) P.emask[L.eoff + j] = (uint8_t)byte;
  }
  const bool lane0 = (threadIdx.x & 63u) == 0u;
  const bool found = live && (byte & LADDER_S);
  const bool open = live && !(byte & LADDER_S);
  const uint32_t n_live = (uint32_t)__popcll(__ballot(live)), n_found = (uint32_t)__popcll(__ballot(found));
  if (lane0) {
    atomicAdd(cnt + 0, n_live);
    if (n_found) atomicAdd(cnt + 1, n_found);
  }
  if (__ballot(open)) {   // (uniform over the wave)
#pragma unroll
    for (uint32_t m = 0; m < 16u; ++m) {
      const uint32_t c = (uint32_t)__popcll(__ballot(open && (byte & 15u) == m));
      if (lane0 && c) atomicAdd(cnt + 2 + m, c);
    }
  }
  __syncthreads();
  if (threadIdx.x < LADDER_COLS && cnt[threadIdx.x])
    atomicAdd(reinterpret_cast<unsigned long long*>(P.tru + (int64_t)v * LADDER_COLS + threadIdx.x), (unsigned long long)cnt[threadIdx.x]);
}

void launch_ladder_records(const LadderRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_ladder_records, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_ladder_truth(const LadderTruthParams& P, int64_t max_entries, hipStream_t st) {
  if (P.n_vcf <= 0 || max_entries <= 0) return;
  const dim3 grid((unsigned)((max_entries + 255) / 256), (unsigned)P.n_vcf);
  hipLaunchKernelGGL(k_ladder_truth, grid, dim3(256), 0, st, P);
}

}  // namespace qm
