// qmvt_norm.hip -- indels and MNPs matched by normal form: every variant is trimmed and left-aligned against
// the 4-bit packed genome of qm_genome_load, so that two spellings of one event carry one (pos, ref, alt).  k_norm_truth turns
// the allele-extended entries of a truth set into their forms, k_norm_insert / k_norm_fill build the open-addressing table of
// the distinct forms, k_norm_records streams the finished batch in input order, normalises every record, probes its VCF's table
// and counts, k_norm_found takes the popcounts of the per-VCF bitmaps.  Integer work only: no output depends on the order the
// lanes run in.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h) stays the id the classification pass's
// profiles are keyed on.
#include "qmvt_norm.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

// inline codes (include/qmvt.h): 0 .. 3 one base, len << 26 | bases for 2 .. 13 bases
__device__ inline bool nm_inline(int32_t c) {
  const uint32_t u = (uint32_t)c;
  return u < 4u || (u - (2u << 26)) < (12u << 26);
}
__device__ inline uint32_t nm_len(int32_t c) { return (uint32_t)c < 4u ? 1u : (uint32_t)c >> 26; }
__device__ inline uint32_t nm_bits(int32_t c) { return (uint32_t)c & 0x03ffffffu; }
__device__ inline int32_t nm_code(uint32_t len, uint32_t bits) { return (int32_t)(len == 1u ? bits : (len << 26) | bits); }

// The genome through the one packed word a lane holds: a walk reads memory once per eight bases.  The words stay where they are
// (L2): the trip count differs per lane, a staged window would be sized by the longest walk of the workgroup.
struct NmGenome {
  const uint32_t* words;
  int32_t wi;
  uint32_t x;
};
// G[q], 1 <= q <= len (the caller's duty): 0 .. 3, or a code that is no base
__device__ inline uint32_t nm_base(NmGenome& g, int32_t q) {
  const int32_t wi = (q - 1) >> 3;
  if (wi != g.wi) {
    g.wi = wi;
    g.x = g.words[wi];
  }
  return (g.x >> (4 * ((q - 1) & 7))) & 15u;
}

struct NmForm {
  int32_t p, r, a;
  uint32_t cls;   // NORM_UNCHANGED, NORM_RESPELLED or a reason (then p, r, a are the input)
};

__device__ inline NmForm nm_normalize(const uint32_t* words, int64_t len, int32_t p, int32_t r, int32_t a, bool nokey) {
  NmForm f{p, r, a, NORM_UNCHANGED};
  if (!nm_inline(r) || !nm_inline(a)) { f.cls = NORM_LONG; return f; }
  if (nokey) { f.cls = NORM_NOKEY; return f; }
  if (r == a) { f.cls = NORM_NOVAR; return f; }
  uint32_t lr = nm_len(r), la = nm_len(a), br = nm_bits(r), ba = nm_bits(a);
  if (p < 1 || (int64_t)p + (int64_t)lr - 1 > len) { f.cls = NORM_RANGE; return f; }
  NmGenome g{words, -1, 0u};
  for (uint32_t k = 0; k < lr; ++k)
    if (nm_base(g, p + (int32_t)k) != ((br >> (2 * k)) & 3u)) { f.cls = NORM_REFMISMATCH; return f; }   // (no base: a mismatch too)
  if (lr == 1u && la == 1u) return f;   // an SNV is its own normal form
  int32_t q = p;
  for (;;) {
    bool changed = false;
    if (((br >> (2 * (lr - 1u))) & 3u) == ((ba >> (2 * (la - 1u))) & 3u) && ((lr >= 2u && la >= 2u) || q > 1)) {
      --lr; --la;
      br &= (1u << (2 * lr)) - 1u;
      ba &= (1u << (2 * la)) - 1u;
      changed = true;
    }
    if (lr == 0u || la == 0u) {   // (only behind a drop at q > 1: q - 1 is inside the genome)
      const uint32_t c = nm_base(g, q - 1);
      if (c >= 4u) { f.cls = NORM_NOBASE; return f; }
      br = (br << 2) | c; ba = (ba << 2) | c;
      ++lr; ++la; --q;
      changed = true;
    }
    if (!changed) break;
  }
  while (lr >= 2u && la >= 2u && ((br ^ ba) & 3u) == 0u) {
    br >>= 2; ba >>= 2;
    --lr; --la; ++q;
  }
  f.p = q; f.r = nm_code(lr, br); f.a = nm_code(la, ba);
  if (f.p != p || f.r != r || f.a != a) f.cls = NORM_RESPELLED;
  return f;
}

__device__ inline uint32_t nm_hash(int32_t p, int32_t r, int32_t a) {
  uint32_t x = (uint32_t)p * 0x9e3779b1u ^ (uint32_t)r * 0x85ebca77u ^ (uint32_t)a * 0xc2b2ae3du;
  x ^= x >> 15; x *= 0x2c1b3c6du;
  x ^= x >> 12; x *= 0x297a2d39u;
  x ^= x >> 15;
  return x;
}

// the slot of form (p, r, a), or -1 (the table has empty slots: at most slots / 2 are claimed)
__device__ inline int32_t nm_probe(const NormTable& T, int32_t p, int32_t r, int32_t a) {
  const uint32_t mask = T.slots - 1u;
  uint32_t h = nm_hash(p, r, a) & mask;
  for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
    if (T.claim[h] == 0u) return -1;
    if (T.spos[h] == p && T.sref[h] == r && T.salt[h] == a) return (int32_t)h;
  }
  return -1;
}

// whether (p, r, a) is spelled like an entry of the truth set: a binary search of its sorted table
__device__ inline bool nm_is_entry(const NormTable& T, int32_t p, int32_t r, int32_t a) {
  if ((uint32_t)p >= (1u << 28)) return false;
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
  return lo < T.xn && T.xkeys[lo] == key && T.xref[lo] == r && T.xalt[lo] == a;
}

// a lane per entry: its form, and how many entries have no normal form
__global__ __launch_bounds__(256) void k_norm_truth(NormTable T) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (j < T.xn) {
    const NmForm f = nm_normalize(T.words, T.len, (int32_t)(T.xkeys[j] >> 4), T.xref[j], T.xalt[j], false);
    T.fpos[j] = f.p; T.fref[j] = f.r; T.falt[j] = f.a;
    bad = f.cls > NORM_RESCUED;
  }
  const uint64_t m = __ballot(bad);
  if (m && (threadIdx.x & 63u) == 0u) atomicAdd(T.stats + 1, (unsigned long long)__popcll(m));
}

// a lane per entry: claims the slot of its form with its index, or joins the entries that share it.  The claimer's form is read
// from the per-entry arrays of the launch before, so no lane waits for another lane's stores.
__global__ __launch_bounds__(256) void k_norm_insert(NormTable T) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= T.xn) return;
  const int32_t p = T.fpos[j], r = T.fref[j], a = T.falt[j];
  const bool respelled = p != (int32_t)(T.xkeys[j] >> 4) || r != T.xref[j] || a != T.xalt[j];
  const uint32_t mask = T.slots - 1u, me = (uint32_t)j + 1u;
  uint32_t h = nm_hash(p, r, a) & mask;
  for (uint32_t it = 0; it < T.slots; ++it, h = (h + 1u) & mask) {
    const uint32_t old = atomicCAS(T.claim + h, 0u, me);
    if (old == 0u) break;
    const uint32_t o = old - 1u;   // (whoever holds the slot by now has this entry's form or another's: one test)
    if (T.fpos[o] == p && T.fref[o] == r && T.falt[o] == a) {
      atomicMin(T.claim + h, me);
      break;
    }
  }
  if (respelled) atomicOr(T.sresp + h, 1u);
}

// a lane per slot: the payload of the claimed slots, and how many there are
__global__ __launch_bounds__(256) void k_norm_fill(NormTable T) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  bool used = false;
  if (s < T.slots) {
    const uint32_t c = T.claim[s];
    used = c != 0u;
    if (used) { T.spos[s] = T.fpos[c - 1u]; T.sref[s] = T.fref[c - 1u]; T.salt[s] = T.falt[c - 1u]; }
  }
  const uint64_t m = __ballot(used);
  if (m && (threadIdx.x & 63u) == 0u) atomicAdd(T.stats, (unsigned long long)__popcll(m));
}

// The span walk of qmvt_walk.h, 4 records per lane (aligned 16-byte / 4-byte accesses).  The counters are wave-uniform registers,
// taken by ballots over the whole wave, added to LDS and from there to the VCF's row when the VCF changes.
__global__ __launch_bounds__(256) void k_norm_records(NormRecParams P) {
  __shared__ uint32_t cnt[NORM_R_COLS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records per workgroup: u32 suffices
  if (threadIdx.x < NORM_R_COLS) cnt[threadIdx.x] = 0u;
  __syncthreads();
  const int lane = (int)(threadIdx.x & 63u);
  uint32_t acc[NORM_R_COLS];
#pragma unroll
  for (int c = 0; c < NORM_R_COLS; ++c) acc[c] = 0u;
  const NormVcf* vp = nullptr;
  walk_spans<4>(
      P.spans, P.n_spans,
      [&](int vcf, const SpanDesc&) {
        vp = P.vcfs + vcf;
        return vp->t.words != nullptr;
      },
      [&](int, const SpanDesc& sd, int64_t g) {
        const NormVcf& V = *vp;
        uint32_t m[4] = {0u, 0u, 0u, 0u};   // bit c: the record counts in column c
        if (g < sd.end) {
          const uint32_t live = rec_live<4>(g, sd.end);
          const uint32_t kb = mask_bits<4>(P.mask_pass, g);
          const uint32_t tb = mask_bits<4>(P.mask_tp, g);
          const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
          const qm_int4 r4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.ref + g));
          const qm_int4 a4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.alt + g));
          const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
          qm_int4 op = p4, orf = r4, oa = a4, orow = {-1, -1, -1, -1};
          uint32_t c4 = 0u;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (!((live >> k) & 1u)) continue;
            const uint32_t fl = (f4 >> (8 * k)) & 255u;
            const bool kept = (kb >> k) & 1u, tp = (tb >> k) & 1u, nokey = (fl & QMF_NOKEY) != 0u;
            const NmForm f = nm_normalize(V.t.words, V.t.len, p4[k], r4[k], a4[k], nokey);
            int32_t slot = -1;
            if (!nokey && allele_valid(r4[k]) && allele_valid(a4[k])) slot = nm_probe(V.t, f.p, f.r, f.a);
            const bool tp_n = kept && ((slot >= 0 && (fl & QMF_IDDOT)) || (fl & QMF_TPLINE));
            const bool rescued = tp_n && !tp;
            if (kept && slot >= 0) {
              const uint32_t w = (uint32_t)slot >> 5, bit = 1u << ((uint32_t)slot & 31u);
              if (!(V.found[w] & bit)) atomicOr(V.found + w, bit);   // (a stale read only repeats the atomic)
              if (!(V.found_eq[w] & bit) && nm_is_entry(V.t, p4[k], r4[k], a4[k])) atomicOr(V.found_eq + w, bit);
            }
            op[k] = f.p; orf[k] = f.r; oa[k] = f.a;
            if (slot >= 0) orow[k] = (int32_t)V.t.claim[slot] - 1;
            c4 |= (rescued ? NORM_RESCUED : f.cls) << (8 * k);
            if (kept) {
              uint32_t mk = 1u | (tp ? 2u : 0u) | (tp_n ? 4u : 0u) | (rescued ? 8u : 0u);
              if (f.cls == NORM_RESPELLED) mk |= 16u | (((uint32_t)(f.r | f.a) < 4u) ? 32u : 0u);
              if (f.cls > NORM_RESCUED) mk |= 1u << (6u + f.cls - NORM_LONG);
              m[k] = mk;
            }
          }
          *reinterpret_cast<uint32_t*>(P.cls + g) = c4;
          if (P.npos) {
            *reinterpret_cast<qm_int4*>(P.npos + g) = op;
            *reinterpret_cast<qm_int4*>(P.nref + g) = orf;
            *reinterpret_cast<qm_int4*>(P.nalt + g) = oa;
            *reinterpret_cast<qm_int4*>(P.nrow + g) = orow;
          }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!__ballot(m[k] != 0u)) continue;   // (uniform over the wave)
#pragma unroll
          for (int c = 0; c < NORM_R_COLS; ++c) acc[c] += (uint32_t)__popcll(__ballot((m[k] >> c) & 1u));
        }
      },
      [&](int vcf) {
        if (lane == 0) {
#pragma unroll
          for (int c = 0; c < NORM_R_COLS; ++c)
            if (acc[c]) atomicAdd(cnt + c, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < NORM_R_COLS; ++c) acc[c] = 0u;
        flush_counts(cnt, NORM_R_COLS, reinterpret_cast<unsigned long long*>(P.rec + (int64_t)vcf * NORM_R_COLS));
      });
}

// a workgroup per VCF: the popcounts of its bitmaps beside the numbers of its table
__global__ __launch_bounds__(256) void k_norm_found(const NormVcf* vcfs, unsigned long long* tru) {
  __shared__ uint32_t sum[2];
  const NormVcf& V = vcfs[blockIdx.x];
  if (!V.t.words) return;   // (uniform over the workgroup)
  if (threadIdx.x < 2) sum[threadIdx.x] = 0u;
  __syncthreads();
  uint32_t n_found = 0u, n_only = 0u;
  for (uint32_t w = threadIdx.x; w < V.t.slots / 32u; w += blockDim.x) {
    const uint32_t f = V.found[w];
    n_found += (uint32_t)__popc(f);
    n_only += (uint32_t)__popc(f & ~V.found_eq[w]);
  }
  if (n_found) atomicAdd(sum, n_found);
  if (n_only) atomicAdd(sum + 1, n_only);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long* o = tru + (int64_t)blockIdx.x * NORM_T_COLS;
    o[0] = (unsigned long long)V.t.xn;
    o[1] = V.t.stats[0];
    o[2] = sum[0];
    o[3] = sum[1];
    o[4] = V.t.stats[1];
  }
}

void launch_norm_truth(const NormTable& T, hipStream_t st) {
  if (T.xn > 0) {
    const dim3 grid((unsigned)((T.xn + 255) / 256));
    hipLaunchKernelGGL(k_norm_truth, grid, dim3(256), 0, st, T);
    hipLaunchKernelGGL(k_norm_insert, grid, dim3(256), 0, st, T);
  }
  hipLaunchKernelGGL(k_norm_fill, dim3((T.slots + 255u) / 256u), dim3(256), 0, st, T);
}

void launch_norm_records(const NormRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_norm_records, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_norm_found(const NormVcf* vcfs, int n_vcf, uint64_t* tru, hipStream_t st) {
  if (n_vcf <= 0) return;
  hipLaunchKernelGGL(k_norm_found, dim3((unsigned)n_vcf), dim3(256), 0, st, vcfs, reinterpret_cast<unsigned long long*>(tru));
}

}  // namespace qm
