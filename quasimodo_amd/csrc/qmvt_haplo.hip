// qmvt_haplo.hip -- clusters of records matched by replayed haplotype: the kept records of a finished
// allele-extended batch that no truth entry spells, and the truth entries no kept record spells, are grouped by the sites of the
// truth set -- chains of entries at most 2 g bases apart --, each side of a site is replayed onto the genome over the site's
// window, and both sides are rescued where the two sequences are equal.  k_hap_entries / k_hap_sites / k_hap_windows build the
// sites of a (truth set, genome, gap); k_hap_records streams the batch in input order, classes every record, finds its site and
// marks the entries it spells; k_hap_truth / k_hap_rank / k_hap_pairs count the truth side and number the (VCF, site) pairs
// with an open entry; k_hap_claim hands every open line to its pair; k_hap_replay decides one pair per wave.  Integer work only:
// no output depends on the order the lanes run in.  Its own translation unit: qm_kernels_id (qmvt_kernels.hip + qmvt_dev.h)
// stays the id the classification pass's profiles are keyed on.
#include "qmvt_haplo.h"
#include "qmvt_walk.h"

#include <algorithm>

namespace qm {

constexpr int32_t HP_NO_HI = -(1 << 30);   // the largest footprint end before the first usable entry

// inline codes (include/qmvt.h): 0 .. 3 one base, len << 26 | bases for 2 .. 13 bases
__device__ inline bool hp_inline(int32_t c) {
  const uint32_t u = (uint32_t)c;
  return u < 4u || (u - (2u << 26)) < (12u << 26);
}
__device__ inline uint32_t hp_len(int32_t c) { return (uint32_t)c < 4u ? 1u : (uint32_t)c >> 26; }
__device__ inline uint32_t hp_bits(int32_t c) { return (uint32_t)c & 0x03ffffffu; }
// G[q], 1 <= q <= len (the caller's duty): 0 .. 3, or the code that is no base
__device__ inline uint32_t hp_base(const uint32_t* words, int32_t q) { return (words[(q - 1) >> 3] >> (4 * ((q - 1) & 7))) & 15u; }
// bit 2 k: field k of the two words differs
__device__ inline uint32_t hp_diff(uint32_t x, uint32_t y) {
  const uint32_t d = x ^ y;
  return (d | d >> 1) & 0x1555555u;
}

// 0 for a usable variant, else the first reason that applies
__device__ inline uint32_t hp_why(const uint32_t* words, int64_t len, int32_t p, int32_t r, int32_t a, bool nokey) {
  if (!hp_inline(r) || !hp_inline(a)) return HAP_LONG;
  if (nokey) return HAP_NOKEY;
  if (r == a) return HAP_NOVAR;
  const uint32_t lr = hp_len(r), br = hp_bits(r);
  if (p < 1 || (int64_t)p + (int64_t)lr - 1 > len) return HAP_RANGE;
  for (uint32_t k = 0; k < lr; ++k)
    if (hp_base(words, p + (int32_t)k) != ((br >> (2 * k)) & 3u)) return HAP_REFMISMATCH;   // (no base: a mismatch too)
  return 0u;
}

// the trimmed form of two different inline codes: the common prefix goes first, then the common suffix of what is left
__device__ inline void hp_trim(int32_t p, int32_t r, int32_t a, int32_t& q, uint32_t& tr, uint32_t& ta, uint32_t& ab) {
  const uint32_t lr = hp_len(r), la = hp_len(a), br = hp_bits(r), ba = hp_bits(a);
  const uint32_t m = min(lr, la);
  const uint32_t fields = (1u << (2u * m)) - 1u;
  const uint32_t cp = (uint32_t)__builtin_ctz((hp_diff(br, ba) & fields) | (1u << (2u * m))) >> 1;
  const uint32_t ds = hp_diff(br >> (2u * (lr - m)), ba >> (2u * (la - m))) & fields;
  const uint32_t cs = min(ds ? (uint32_t)__builtin_clz(ds << (32u - 2u * m)) >> 1 : m, m - cp);
  q = p + (int32_t)cp;
  tr = lr - cp - cs;
  ta = la - cp - cs;
  ab = (ba >> (2u * cp)) & ((1u << (2u * ta)) - 1u);
}

// the index of the entry spelled (p, r, a) in the truth set's sorted table, or -1 (0 <= p < 2^28: the caller's duty)
__device__ inline int64_t hp_entry(const HapSites& S, int32_t p, int32_t r, int32_t a) {
  const uint32_t key = ((uint32_t)p << 4) | allele_nib(r, a);
  int64_t lo = 0, hi = S.xn;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const uint32_t k = S.xkeys[mid];
    bool less = k < key;
    if (k == key) {
      const int32_t rr = S.xref[mid];
      less = rr < r || (rr == r && S.xalt[mid] < a);
    }
    if (less) lo = mid + 1; else hi = mid;
  }
  return lo < S.xn && S.xkeys[lo] == key && S.xref[lo] == r && S.xalt[lo] == a ? lo : -1;
}

// The site whose window holds the footprint [lo, hi], or -1: the first site whose window ends at or behind hi, if it starts at
// or before lo.  (Window ends never descend: the largest footprint end of a site is larger than that of the site before.)
__device__ inline int32_t hp_site(const HapSites& S, int32_t ns, int32_t lo, int32_t hi) {
  int32_t x = 0, y = ns;
  while (x < y) {
    const int32_t mid = (x + y) >> 1;
    if (S.shi[mid] < hi) x = mid + 1; else y = mid;
  }
  return x < ns && S.slo[x] <= lo ? x : -1;
}

// ---- the sites of a (truth set, genome, gap) ----
// a lane per entry: usable or why not, and the footprint of its trimmed form
__global__ __launch_bounds__(256) void k_hap_entries(HapSites S) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= S.xn) return;
  const int32_t p = (int32_t)(S.xkeys[j] >> 4), r = S.xref[j], a = S.xalt[j];
  const uint32_t why = hp_why(S.words, S.len, p, r, a, false);
  int32_t q = 0;
  uint32_t tr = 0u, ta = 0u, ab = 0u;
  if (!why) hp_trim(p, r, a, q, tr, ta, ab);
  S.ewhy[j] = (uint8_t)why;
  S.elo[j] = q;
  S.ehi[j] = max(q, q + (int32_t)tr - 1);
}

// One workgroup walks the table in its order, 256 entries a step: the running maximum of the footprint ends decides whether a
// usable entry opens a site (its footprint starts more than 2 g behind every end before it), a running sum numbers the sites.
__global__ __launch_bounds__(256) void k_hap_sites(HapSites S) {
  __shared__ int32_t smax[256];
  __shared__ int32_t ssum[256];
  const int t = (int)threadIdx.x;
  int32_t cmax = HP_NO_HI, ccnt = 0;
  for (int64_t base = 0; base < S.xn; base += 256) {
    const int64_t j = base + t;
    const bool use = j < S.xn && S.ewhy[j] == 0;
    const int32_t lo = use ? S.elo[j] : 0, hi = use ? S.ehi[j] : HP_NO_HI;
    smax[t] = hi;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int32_t v = t >= d ? max(smax[t], smax[t - d]) : smax[t];
      __syncthreads();
      smax[t] = v;
      __syncthreads();
    }
    const int32_t before = max(cmax, t ? smax[t - 1] : HP_NO_HI);
    const bool opens = use && lo > before + 2 * S.gap;   // (the first usable entry: lo >= 1 > HP_NO_HI + 64)
    ssum[t] = opens ? 1 : 0;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
      const int32_t v = t >= d ? ssum[t] + ssum[t - d] : ssum[t];
      __syncthreads();
      ssum[t] = v;
      __syncthreads();
    }
    const int32_t idx = ccnt + ssum[t] - 1;
    if (j < S.xn) S.esite[j] = use ? idx : -1;
    if (opens) S.sfirst[idx] = (int32_t)j;
    cmax = max(cmax, smax[255]);
    ccnt += ssum[255];
    __syncthreads();
  }
  if (t == 0) {
    S.n_sites[0] = ccnt;
    S.sfirst[ccnt] = (int32_t)S.xn;
  }
}

// a lane per site: the window over the footprints of its usable entries
__global__ __launch_bounds__(256) void k_hap_windows(HapSites S) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= S.n_sites[0]) return;
  int32_t lo = 0x7fffffff, hi = HP_NO_HI;
  for (int32_t j = S.sfirst[s]; j < S.sfirst[s + 1]; ++j) {
    if (S.ewhy[j]) continue;
    lo = min(lo, S.elo[j]);
    hi = max(hi, S.ehi[j]);
  }
  S.slo[s] = max(1, lo - S.gap);
  S.shi[s] = (int32_t)min(S.len + 1, (int64_t)hi + S.gap);
}

// ---- the records ----
// The span walk of qmvt_walk.h, 4 records per lane (aligned 16-byte / 4-byte accesses).  Every kept record adds to its columns
// of the workgroup's LDS row, which goes to the VCF's row when the VCF changes.  A kept, usable, unmatched record inside the
// window of a site that is not TOOLONG stays HAP_PENDING for k_hap_claim.
__global__ __launch_bounds__(256) void k_hap_records(HapRecParams P) {
  __shared__ uint32_t hist[HAP_R_COLS];   // at most PASS_SPANS * SPAN_TILES * K1_TILE records per workgroup: u32 suffices
  if (threadIdx.x < HAP_R_COLS) hist[threadIdx.x] = 0u;
  __syncthreads();
  const HapVcf* vp = nullptr;
  int32_t ns = 0;
  walk_spans<4>(
      P.spans, P.n_spans,
      [&](int vcf, const SpanDesc&) {
        vp = P.vcfs + vcf;
        if (!vp->s.words) return false;
        ns = vp->s.n_sites[0];
        return true;
      },
      [&](int, const SpanDesc& sd, int64_t g) {
        if (g >= sd.end) return;
        const HapVcf& V = *vp;
        const uint32_t live = rec_live<4>(g, sd.end);
        const uint32_t kb = mask_bits<4>(P.mask_pass, g);
        const uint32_t tb = mask_bits<4>(P.mask_tp, g);
        const qm_int4 p4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.pos + g));   // read once
        const qm_int4 r4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.ref + g));
        const qm_int4 a4 = __builtin_nontemporal_load(reinterpret_cast<const qm_int4*>(P.alt + g));
        const uint32_t f4 = *reinterpret_cast<const uint32_t*>(P.flags + g);
        qm_int4 st4 = {-1, -1, -1, -1};
        uint32_t c4 = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((live >> k) & 1u)) continue;
          const bool kept = (kb >> k) & 1u, tp = (tb >> k) & 1u, nokey = ((f4 >> (8 * k)) & QMF_NOKEY) != 0u;
          const int32_t p = p4[k], r = r4[k], a = a4[k];
          int64_t e = -1;
          if (!nokey && allele_valid(r) && allele_valid(a) && (uint32_t)p < (1u << 28)) e = hp_entry(V.s, p, r, a);
          const uint32_t why = hp_why(V.s.words, V.s.len, p, r, a, nokey);
          int32_t st = -1;
          if (!why) {
            int32_t q;
            uint32_t tr, ta, ab;
            hp_trim(p, r, a, q, tr, ta, ab);
            st = hp_site(V.s, ns, q, max(q, q + (int32_t)tr - 1));
          }
          uint32_t c;
          if (e >= 0) c = HAP_MATCHED;
          else if (why) c = why;
          else if (!kept) c = HAP_NOTKEPT;
          else if (st < 0) c = HAP_OUTSIDE;
          else c = V.s.shi[st] - V.s.slo[st] + 1 > HAP_MAX_WINDOW ? HAP_TOOLONG : HAP_PENDING;
          st4[k] = st;
          c4 |= c << (8 * k);
          if (!kept) continue;
          atomicAdd(hist + HAP_R_KEPT, 1u);
          if (tp) {
            atomicAdd(hist + HAP_R_TP, 1u);
            atomicAdd(hist + HAP_R_TP_H, 1u);
          }
          if (e >= 0) {
            const uint32_t bit = 1u << ((uint32_t)e & 31u);
            if (!(V.ebits[e >> 5] & bit)) atomicOr(V.ebits + (e >> 5), bit);   // (a stale read only repeats the atomic)
          } else {
            if (c == HAP_PENDING || c == HAP_TOOLONG) atomicAdd(hist + HAP_R_OPEN, 1u);
            if (c != HAP_PENDING) atomicAdd(hist + HAP_R_CLASS0 + c, 1u);
          }
        }
        *reinterpret_cast<uint32_t*>(P.cls + g) = c4;
        *reinterpret_cast<qm_int4*>(P.site + g) = st4;
      },
      [&](int vcf) { flush_counts(hist, HAP_R_COLS, reinterpret_cast<unsigned long long*>(P.rec + (int64_t)vcf * HAP_R_COLS)); });
}

// ---- the truth side ----
// grid (x, VCF), a lane per entry of the VCF's truth set: found, unusable or open; an open entry marks its site unless the
// site is TOOLONG
__global__ __launch_bounds__(256) void k_hap_truth(const HapVcf* vcfs, unsigned long long* tru) {
  const HapVcf& V = vcfs[blockIdx.y];
  if (!V.s.words) return;   // (uniform over the workgroup)
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool found = false, bad = false, open = false;
  if (j < V.s.xn) {
    found = (V.ebits[j >> 5] >> ((uint32_t)j & 31u)) & 1u;
    const uint32_t why = V.s.ewhy[j];
    bad = why != 0u;
    open = !found && !bad;
    uint32_t c = found ? HAP_MATCHED : why;
    if (open) {
      const int32_t s = V.s.esite[j];
      const bool toolong = V.s.shi[s] - V.s.slo[s] + 1 > HAP_MAX_WINDOW;
      c = toolong ? HAP_TOOLONG : HAP_LONE;   // (LONE until k_hap_replay says what became of the site)
      const uint32_t bit = 1u << ((uint32_t)s & 31u);
      if (!toolong && !(V.sbits[s >> 5] & bit)) atomicOr(V.sbits + (s >> 5), bit);
    }
    if (V.ecls) V.ecls[j] = (uint8_t)c;
  }
  unsigned long long* o = tru + (int64_t)blockIdx.y * HAP_T_COLS;
  const uint64_t mf = __ballot(found), mb = __ballot(bad), mo = __ballot(open);
  if ((threadIdx.x & 63u) == 0u) {
    if (mf) {
      atomicAdd(o + HAP_T_FOUND, (unsigned long long)__popcll(mf));
      atomicAdd(o + HAP_T_FOUND_H, (unsigned long long)__popcll(mf));
    }
    if (mo) atomicAdd(o + HAP_T_OPEN, (unsigned long long)__popcll(mo));
    if (mb) atomicAdd(o + HAP_T_UNUSABLE, (unsigned long long)__popcll(mb));
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    o[HAP_T_ENTRIES] = (unsigned long long)V.s.xn;
    o[HAP_T_SITES] = (unsigned long long)V.s.n_sites[0];
  }
}

// One workgroup, VCF after VCF: the number of marked sites before every word of a VCF's bitmap, counted over all VCFs, so that
// the pair of (VCF, site) is one load and one popcount away; total[0] = the number of pairs.
__global__ __launch_bounds__(256) void k_hap_rank(const HapVcf* vcfs, int n_vcf, unsigned long long* total) {
  __shared__ uint32_t ssum[256];
  const int t = (int)threadIdx.x;
  uint32_t run = 0u;
  for (int v = 0; v < n_vcf; ++v) {
    const HapVcf& V = vcfs[v];
    if (!V.s.words) continue;
    const int64_t nw = ((int64_t)V.s.n_sites[0] + 31) / 32;
    for (int64_t base = 0; base < nw; base += 256) {
      const int64_t w = base + t;
      const uint32_t n = w < nw ? (uint32_t)__popc(V.sbits[w]) : 0u;
      ssum[t] = n;
      __syncthreads();
      for (int d = 1; d < 256; d <<= 1) {
        const uint32_t x = t >= d ? ssum[t] + ssum[t - d] : ssum[t];
        __syncthreads();
        ssum[t] = x;
        __syncthreads();
      }
      if (w < nw) V.srank[w] = run + ssum[t] - n;
      run += ssum[255];
      __syncthreads();
    }
  }
  if (t == 0) total[0] = run;
}

// grid (x, VCF), a lane per word of the VCF's bitmap: names the pairs of its marked sites, no open line yet
__global__ __launch_bounds__(256) void k_hap_pairs(const HapVcf* vcfs, int32_t* pairs) {
  const HapVcf& V = vcfs[blockIdx.y];
  if (!V.s.words) return;
  const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= ((int64_t)V.s.n_sites[0] + 31) / 32) return;
  uint32_t bits = V.sbits[w];
  int64_t pair = V.srank[w];
  while (bits) {
    const int b = __builtin_ctz(bits);
    bits &= bits - 1u;
    int32_t* pr = pairs + pair * HAP_PAIR_WORDS;
    pr[0] = (int32_t)blockIdx.y;
    pr[1] = (int32_t)(w * 32 + b);
    pr[2] = 0;
    ++pair;
  }
}

// The span walk again, over the class bytes alone: a pending line whose site has no open entry is LONE; every other one takes a
// slot of its pair with one atomic add -- past HAP_MAX_ITEMS it only marks the pair, and is TOOMANY itself.
__global__ __launch_bounds__(256) void k_hap_claim(HapRecParams P) {
  __shared__ uint32_t hist[2];
  if (threadIdx.x < 2) hist[threadIdx.x] = 0u;
  __syncthreads();
  const HapVcf* vp = nullptr;
  walk_spans<4>(
      P.spans, P.n_spans,
      [&](int vcf, const SpanDesc&) {
        vp = P.vcfs + vcf;
        return vp->s.words != nullptr;
      },
      [&](int, const SpanDesc& sd, int64_t g) {
        if (g >= sd.end) return;
        const HapVcf& V = *vp;
        const uint32_t live = rec_live<4>(g, sd.end);
        const uint32_t c4 = *reinterpret_cast<const uint32_t*>(P.cls + g);
        uint32_t o4 = c4;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (!((live >> k) & 1u) || ((c4 >> (8 * k)) & 255u) != HAP_PENDING) continue;
          const int32_t st = P.site[g + k];
          const uint32_t word = V.sbits[st >> 5], below = (1u << ((uint32_t)st & 31u)) - 1u;
          uint32_t c = HAP_LONE;
          if ((word >> ((uint32_t)st & 31u)) & 1u) {
            int32_t* pr = P.pairs + ((int64_t)V.srank[st >> 5] + __popc(word & below)) * HAP_PAIR_WORDS;
            const int32_t slot = atomicAdd(pr + 2, 1);
            c = HAP_PENDING;   // (k_hap_replay writes it)
            if (slot < HAP_MAX_ITEMS) pr[3 + slot] = (int32_t)(g + k - V.off);
            else c = HAP_TOOMANY;
          }
          if (c == HAP_LONE) atomicAdd(hist, 1u);
          if (c == HAP_TOOMANY) atomicAdd(hist + 1, 1u);
          o4 = (o4 & ~(255u << (8 * k))) | (c << (8 * k));
        }
        if (o4 != c4) *reinterpret_cast<uint32_t*>(P.cls + g) = o4;
      },
      [&](int vcf) {   // (the two cells are columns apart in the VCF's row: a flush of its own)
        __syncthreads();
        if (threadIdx.x < 2 && hist[threadIdx.x]) {
          const int col = HAP_R_CLASS0 + (int)(threadIdx.x ? HAP_TOOMANY : HAP_LONE);
          atomicAdd(reinterpret_cast<unsigned long long*>(P.rec + (int64_t)vcf * HAP_R_COLS + col), (unsigned long long)hist[threadIdx.x]);
          hist[threadIdx.x] = 0u;
        }
        __syncthreads();
      });
}

// ---- the replay ----
// One wave (a workgroup of its own) per pair.  Lanes 0 .. 7 hold the open lines, lanes 8 .. 15 the open entries; identical
// spellings of a side collapse, every remaining item takes its rank by (q, |r|, lane) among its side, neighbours in that order
// are tested for a conflict, and the output offset of every ALT piece is its window offset plus the length deltas before it.
// The two replays are never stored: lane t computes symbols t, t + 64, ... of both and compares them.
__global__ __launch_bounds__(64) void k_hap_replay(HapReplayParams P) {
  __shared__ int32_t ent[HAP_MAX_ITEMS];
  __shared__ int32_t it_p[16], it_r[16], it_a[16], it_q[16];
  __shared__ uint32_t it_lr[16], it_dup[16];
  __shared__ int32_t vq[2][HAP_MAX_ITEMS], vst[2][HAP_MAX_ITEMS];
  __shared__ uint32_t vlr[2][HAP_MAX_ITEMS], vla[2][HAP_MAX_ITEMS], vab[2][HAP_MAX_ITEMS];
  __shared__ int32_t tot[2], dlt[2];
  const int t = (int)threadIdx.x;
  const int32_t* pr = P.pairs + (int64_t)blockIdx.x * HAP_PAIR_WORDS;
  const int32_t v = pr[0], s = pr[1], cnt = pr[2];
  if (cnt <= 0) return;   // (uniform: no open line, the site is not tried)
  const HapVcf& V = P.vcfs[v];
  const HapSites& S = V.s;
  const int nrec = min(cnt, HAP_MAX_ITEMS);
  const int32_t e0 = S.sfirst[s], e1 = S.sfirst[s + 1];
  int nent = 0;
  for (int32_t b = e0; b < e1; b += 64) {
    const int32_t j = b + t;
    const bool open = j < e1 && S.ewhy[j] == 0 && !((V.ebits[j >> 5] >> ((uint32_t)j & 31u)) & 1u);
    const uint64_t m = __ballot(open);
    if (open) {
      const int r = nent + __popcll(m & ((1ull << t) - 1ull));
      if (r < HAP_MAX_ITEMS) ent[r] = j;
    }
    nent += __popcll(m);
  }
  __syncthreads();
  uint32_t outcome = HAP_TOOMANY;
  if (cnt <= HAP_MAX_ITEMS && nent <= HAP_MAX_ITEMS) {
    const int side = t >> 3, k = t & 7;
    const bool have = t < 16 && k < (side ? nent : nrec);
    int32_t p = 0, r = 0, a = 1, q = 0;
    uint32_t tr = 0u, ta = 0u, ab = 0u;
    if (have) {
      if (side) {
        const int32_t j = ent[k];
        p = (int32_t)(S.xkeys[j] >> 4); r = S.xref[j]; a = S.xalt[j];
      } else {
        const int64_t gi = V.off + pr[3 + k];
        p = P.pos[gi]; r = P.ref[gi]; a = P.alt[gi];
      }
      hp_trim(p, r, a, q, tr, ta, ab);
    }
    if (t < 16) { it_p[t] = p; it_r[t] = r; it_a[t] = a; it_q[t] = q; it_lr[t] = tr; }
    __syncthreads();
    bool dup = false;
    if (have)
      for (int i = side * 8; i < t; ++i) dup = dup || (it_p[i] == p && it_r[i] == r && it_a[i] == a);
    if (t < 16) it_dup[t] = (!have || dup) ? 1u : 0u;
    __syncthreads();
    if (have && !dup) {
      int rank = 0;
      for (int i = side * 8; i < side * 8 + 8; ++i) {
        if (it_dup[i] || i == t) continue;
        const bool less = it_q[i] != q ? it_q[i] < q : it_lr[i] != tr ? it_lr[i] < tr : i < t;
        rank += less ? 1 : 0;
      }
      vq[side][rank] = q; vlr[side][rank] = tr; vla[side][rank] = ta; vab[side][rank] = ab;
    }
    const uint64_t mk = __ballot(have && !dup);
    const int nv0 = __popcll(mk & 0xffull), nv1 = __popcll(mk & 0xff00ull);
    __syncthreads();
    const int nvs = side ? nv1 : nv0;
    bool bad = false;
    if (t < 16 && k + 1 < nvs) {
      const int32_t qa = vq[side][k], qb = vq[side][k + 1];
      bad = qb < qa + (int32_t)vlr[side][k] || (qb == qa && vlr[side][k + 1] == 0u);
    }
    if (__ballot(bad)) {
      outcome = HAP_CONFLICT;
    } else {
      const int32_t ws = S.slo[s], wend = (int32_t)min((int64_t)S.shi[s], S.len);
      if (t < 2) {   // (side t: at most eight pieces)
        int32_t d = 0;
        const int n = t ? nv1 : nv0;
        for (int i = 0; i < n; ++i) {
          vst[t][i] = vq[t][i] - ws + d;
          d += (int32_t)vla[t][i] - (int32_t)vlr[t][i];
        }
        dlt[t] = d;
        tot[t] = wend - ws + 1 + d;
      }
      __syncthreads();
      bool differ = tot[0] != tot[1];
      if (!differ) {
        for (int32_t o = t; o < tot[0]; o += 64) {
          uint32_t sym[2];
#pragma unroll
          for (int sd = 0; sd < 2; ++sd) {
            const int n = sd ? nv1 : nv0;
            int32_t gq = ws + o - dlt[sd];   // behind the last piece
            uint32_t c = 16u;
            for (int i = 0; i < n; ++i) {
              const int32_t b0 = vst[sd][i];
              if (o < b0) { gq = o - b0 + vq[sd][i]; break; }
              if (o < b0 + (int32_t)vla[sd][i]) { c = (vab[sd][i] >> (2 * (o - b0))) & 3u; break; }
            }
            sym[sd] = c < 16u ? c : hp_base(S.words, gq);
          }
          differ = differ || sym[0] != sym[1];
        }
      }
      outcome = __ballot(differ) ? HAP_MISMATCH : HAP_RESCUED;
    }
  }
  // what became of the site, to its lines and entries
  bool gained = false;
  if (t < nrec) {
    const int64_t gi = V.off + pr[3 + t];
    P.cls[gi] = (uint8_t)outcome;
    if (outcome == HAP_RESCUED) gained = (P.flags[gi] & QMF_IDDOT) && !((P.mask_tp[gi >> 6] >> (int)(gi & 63)) & 1ull);
  }
  const uint64_t mg = __ballot(gained);
  if (V.ecls)
    for (int32_t j = e0 + t; j < e1; j += 64)
      if (S.ewhy[j] == 0 && !((V.ebits[j >> 5] >> ((uint32_t)j & 31u)) & 1u)) V.ecls[j] = (uint8_t)outcome;
  if (t == 0) {
    unsigned long long* orec = reinterpret_cast<unsigned long long*>(P.rec) + (int64_t)v * HAP_R_COLS;
    unsigned long long* otru = reinterpret_cast<unsigned long long*>(P.tru) + (int64_t)v * HAP_T_COLS;
    atomicAdd(otru + HAP_T_TRIED, 1ull);
    if (outcome == HAP_RESCUED) {
      atomicAdd(otru + HAP_T_MATCHED, 1ull);
      atomicAdd(otru + HAP_T_FOUND_H, (unsigned long long)nent);
      if (mg) {
        atomicAdd(orec + HAP_R_TP_H, (unsigned long long)__popcll(mg));
        atomicAdd(orec + HAP_R_RESCUED, (unsigned long long)__popcll(mg));
      }
    } else {
      atomicAdd(orec + HAP_R_CLASS0 + outcome, (unsigned long long)nrec);
    }
  }
}

// ---- the subset search ----
// a < b in the total order of distinct trimmed forms: (q, |r|, |a|, a as a string over A<C<G<T -- base k of an allele sits in bits
// 2 k, so the lowest field that differs decides)
__device__ inline bool hs_less(int32_t q1, uint32_t r1, uint32_t a1, uint32_t b1, int32_t q2, uint32_t r2, uint32_t a2, uint32_t b2) {
  if (q1 != q2) return q1 < q2;
  if (r1 != r2) return r1 < r2;
  if (a1 != a2) return a1 < a2;
  const uint32_t d = b1 ^ b2;
  if (!d) return false;
  const uint32_t sh = (uint32_t)__builtin_ctz(d) & ~1u;
  return ((b1 >> sh) & 3u) < ((b2 >> sh) & 3u);
}

constexpr uint32_t HS_B1 = 0x9E3779B1u, HS_B2 = 0x85EBCA77u;   // the bases of the two polynomial hashes mod 2^32 (odd)
constexpr int32_t HS_NONE = (int32_t)0x80000000;               // the length delta of a subset that is not admissible
constexpr int HS_TAB = HAP_MAX_WINDOW + 4;                      // prefix tables: offsets 0 .. HAP_MAX_WINDOW

// a lane per VCF: TP_S and FOUND_S start from the pass's TP_H and FOUND_H
__global__ __launch_bounds__(256) void k_hap_subsets_init(HapSubParams P) {
  const int v = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (v >= P.n_vcf) return;
  uint64_t* o = P.sub + (int64_t)v * HAPSUB_COLS;
  for (int k = 0; k < HAPSUB_COLS; ++k) o[k] = 0ull;
  o[HAPSUB_TP_S] = P.rec[(int64_t)v * HAP_R_COLS + HAP_R_TP_H];
  o[HAPSUB_FOUND_S] = P.tru[(int64_t)v * HAP_T_COLS + HAP_T_FOUND_H];
}

// One wave (a workgroup of its own) per pair; a pair that was not tried, or whose site is neither MISMATCH nor CONFLICT, returns
// at once.  Lanes 0 .. 7 hold the open lines, lanes 8 .. 15 the open entries, gathered as k_hap_replay gathers them.  Spellings
// that trim to one form collapse; the forms of a side take their rank in the total order (no lane, no slot of the pair list takes
// part: the lists fill in the order the claims arrive).  Every non-empty subset of a side gets its admissibility (8 x 8 conflict
// bits), its length delta and two 32-bit polynomial hashes of its replay, composed in O(its forms) from prefix hashes of the
// window's genome symbols and the hashes of the ALT pieces.  The candidates -- pairs of subsets whose deltas and hashes agree -- are
// taken in the optimum's order (each lane keeps the least order key of its S masks over all T masks, a wave minimum picks one) and
// VERIFIED symbol by symbol as k_hap_replay compares, nothing stored; a candidate that fails is the floor of the next round.  The
// answer never rests on a hash: narrow hashes (4 bits) give the same result through more rounds.
__global__ __launch_bounds__(64) void k_hap_subsets(HapSubParams P) {
  __shared__ int32_t ent[HAP_MAX_ITEMS];
  __shared__ int32_t it_q[16];
  __shared__ uint32_t it_lr[16], it_la[16], it_ab[16], it_dup[16];
  __shared__ int32_t fq[2][HAP_MAX_ITEMS];
  __shared__ uint32_t flr[2][HAP_MAX_ITEMS], fla[2][HAP_MAX_ITEMS], fab[2][HAP_MAX_ITEMS], fcf[2][HAP_MAX_ITEMS];
  __shared__ uint32_t fh1[2][HAP_MAX_ITEMS], fh2[2][HAP_MAX_ITEMS];
  __shared__ uint32_t pw1[HS_TAB], pw2[HS_TAB], gh1[HS_TAB], gh2[HS_TAB];
  __shared__ uint32_t sc1[64], sc2[64];
  __shared__ uint32_t sh1[2][256], sh2[2][256];
  __shared__ int32_t sdl[2][256];
  __shared__ int32_t vq[2][HAP_MAX_ITEMS], vst[2][HAP_MAX_ITEMS];
  __shared__ uint32_t vla[2][HAP_MAX_ITEMS], vab[2][HAP_MAX_ITEMS];
  __shared__ int32_t vn[2], dlt[2], tot[2];
  const int t = (int)threadIdx.x;
  const int32_t* pr = P.pairs + (int64_t)blockIdx.x * HAP_PAIR_WORDS;
  const int32_t v = pr[0], s = pr[1], cnt = pr[2];
  if (cnt <= 0 || cnt > HAP_MAX_ITEMS) return;   // (uniform: not tried, or TOOMANY)
  const HapVcf& V = P.vcfs[v];
  const HapSites& S = V.s;
  const uint32_t c0 = P.cls[V.off + pr[3]];
  if (c0 != HAP_MISMATCH && c0 != HAP_CONFLICT) return;   // (uniform: every open line of a site carries the site's outcome)
  const int nrec = cnt;
  const int32_t e0 = S.sfirst[s], e1 = S.sfirst[s + 1];
  int nent = 0;
  for (int32_t b = e0; b < e1; b += 64) {
    const int32_t j = b + t;
    const bool open = j < e1 && S.ewhy[j] == 0 && !((V.ebits[j >> 5] >> ((uint32_t)j & 31u)) & 1u);
    const uint64_t m = __ballot(open);
    if (open) {
      const int r = nent + __popcll(m & ((1ull << t) - 1ull));
      if (r < HAP_MAX_ITEMS) ent[r] = j;
    }
    nent += __popcll(m);
  }
  if (nent <= 0 || nent > HAP_MAX_ITEMS) return;   // (uniform; a MISMATCH or CONFLICT site holds 1 .. 8 open entries)
  __syncthreads();
  // the items and their forms
  const int side = (t >> 3) & 1, k = t & 7;
  const bool have = t < 16 && k < (side ? nent : nrec);
  int32_t q = 0;
  uint32_t tr = 0u, ta = 0u, ab = 0u;
  if (have) {
    int32_t p, r, a;
    if (side) {
      const int32_t j = ent[k];
      p = (int32_t)(S.xkeys[j] >> 4); r = S.xref[j]; a = S.xalt[j];
    } else {
      const int64_t gi = V.off + pr[3 + k];
      p = P.pos[gi]; r = P.ref[gi]; a = P.alt[gi];
    }
    hp_trim(p, r, a, q, tr, ta, ab);
  }
  if (t < 16) { it_q[t] = q; it_lr[t] = tr; it_la[t] = ta; it_ab[t] = ab; }
  __syncthreads();
  bool dup = false;
  if (have)
    for (int i = side * 8; i < t; ++i) dup = dup || (it_q[i] == q && it_lr[i] == tr && it_la[i] == ta && it_ab[i] == ab);
  if (t < 16) it_dup[t] = (!have || dup) ? 1u : 0u;
  __syncthreads();
  int frank = 0;   // the bit of this item's form in its side's masks
  if (have) {
    for (int i = side * 8; i < side * 8 + 8; ++i)
      if (!it_dup[i] && hs_less(it_q[i], it_lr[i], it_la[i], it_ab[i], q, tr, ta, ab)) ++frank;
    if (!dup) {
      uint32_t h1 = 0u, h2 = 0u;
      for (uint32_t i = 0; i < ta; ++i) {
        const uint32_t c = ((ab >> (2u * i)) & 3u) + 1u;
        h1 = h1 * HS_B1 + c;
        h2 = h2 * HS_B2 + c;
      }
      fq[side][frank] = q; flr[side][frank] = tr; fla[side][frank] = ta; fab[side][frank] = ab;
      fh1[side][frank] = h1; fh2[side][frank] = h2;
    }
  }
  const uint64_t mk = __ballot(have && !dup);
  const int nf0 = __popcll(mk & 0xffull), nf1 = __popcll(mk & 0xff00ull);
  __syncthreads();
  // the conflict bits of every form against the others of its side, all pairs
  if (t < 16 && k < (side ? nf1 : nf0)) {
    const int n = side ? nf1 : nf0;
    uint32_t cf = 0u;
    for (int j = 0; j < n; ++j) {
      if (j == k) continue;
      const int x = min(j, k), y = max(j, k);
      const bool bad = fq[side][y] < fq[side][x] + (int32_t)flr[side][x] || (fq[side][y] == fq[side][x] && flr[side][y] == 0u);
      cf |= bad ? 1u << j : 0u;
    }
    fcf[side][k] = cf;
  }
  // powers of the bases and prefix hashes of the window's symbols: lane t owns offsets 4 t .. 4 t + 3 (symbols past the window
  // count as 0; no prefix that is used holds one)
  const int32_t ws = S.slo[s], wend = (int32_t)min((int64_t)S.shi[s], S.len);
  const int32_t W = min(max(wend - ws + 1, 0), HAP_MAX_WINDOW);
  {
    uint32_t p1 = 1u, p2 = 1u, x1 = HS_B1, x2 = HS_B2;
    for (uint32_t e = 4u * (uint32_t)t; e; e >>= 1) {
      if (e & 1u) { p1 *= x1; p2 *= x2; }
      x1 *= x1; x2 *= x2;
    }
    for (int i = 0; i < 4; ++i) {
      pw1[4 * t + i] = p1; pw2[4 * t + i] = p2;
      p1 *= HS_B1; p2 *= HS_B2;
    }
    if (t == 63) { pw1[256] = p1; pw2[256] = p2; }
  }
  uint32_t sy[4];
  uint32_t c1 = 0u, c2 = 0u;
  for (int i = 0; i < 4; ++i) {
    const int32_t o = 4 * t + i;
    sy[i] = o < W ? hp_base(S.words, ws + o) + 1u : 0u;
    c1 = c1 * HS_B1 + sy[i];
    c2 = c2 * HS_B2 + sy[i];
  }
  sc1[t] = c1; sc2[t] = c2;
  __syncthreads();
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y1 = t >= d ? sc1[t - d] * pw1[4 * d] + sc1[t] : sc1[t];
    const uint32_t y2 = t >= d ? sc2[t - d] * pw2[4 * d] + sc2[t] : sc2[t];
    __syncthreads();
    sc1[t] = y1; sc2[t] = y2;
    __syncthreads();
  }
  {
    uint32_t g1 = t ? sc1[t - 1] : 0u, g2 = t ? sc2[t - 1] : 0u;
    for (int i = 0; i < 4; ++i) {
      gh1[4 * t + i] = g1; gh2[4 * t + i] = g2;
      g1 = g1 * HS_B1 + sy[i];
      g2 = g2 * HS_B2 + sy[i];
    }
    if (t == 63) { gh1[256] = g1; gh2[256] = g2; }
  }
  __syncthreads();
  // every subset of a side: admissible or not, its length delta, the hashes of its replay
  for (int sd = 0; sd < 2; ++sd) {
    const int n = sd ? nf1 : nf0;
    for (uint32_t m = (uint32_t)t; m < (1u << n); m += 64u) {
      if (!m) continue;
      bool adm = true;
      int32_t cur = 0, d = 0;
      uint32_t h1 = 0u, h2 = 0u;
      for (int i = 0; i < n; ++i) {
        if (!((m >> i) & 1u)) continue;
        adm = adm && !(fcf[sd][i] & m);
        if (!adm) break;
        const int32_t qo = fq[sd][i] - ws, len = qo - cur;   // (admissible so far: 0 <= cur <= qo <= W)
        h1 = (h1 * pw1[len] + gh1[qo] - gh1[cur] * pw1[len]) * pw1[fla[sd][i]] + fh1[sd][i];
        h2 = (h2 * pw2[len] + gh2[qo] - gh2[cur] * pw2[len]) * pw2[fla[sd][i]] + fh2[sd][i];
        cur = qo + (int32_t)flr[sd][i];
        d += (int32_t)fla[sd][i] - (int32_t)flr[sd][i];
      }
      if (adm) {
        const int32_t len = W - cur;
        h1 = h1 * pw1[len] + gh1[W] - gh1[cur] * pw1[len];
        h2 = h2 * pw2[len] + gh2[W] - gh2[cur] * pw2[len];
      }
      sh1[sd][m] = P.narrow ? h1 >> 28 : h1;   // (the top bits: the low ones of a polynomial mod 2^32 mix nothing)
      sh2[sd][m] = P.narrow ? 0u : h2;
      sdl[sd][m] = adm ? d : HS_NONE;
    }
  }
  __syncthreads();
  // the candidates in the optimum's order: the largest |S| + |T|, then the larger |T|, then the smallest S mask, then the smallest
  // T mask -- one order key, smaller is better
  uint32_t floor = 0u, found = 0u;
  for (;;) {
    uint32_t best = 0xffffffffu;
    for (uint32_t ms = (uint32_t)t; ms < (1u << nf0); ms += 64u) {
      if (!ms) continue;
      const int32_t ds = sdl[0][ms];
      if (ds == HS_NONE) continue;
      const uint32_t a1 = sh1[0][ms], a2 = sh2[0][ms];
      const uint32_t ps = (uint32_t)__popc(ms);
      for (uint32_t mt = 1u; mt < (1u << nf1); ++mt) {
        if (sdl[1][mt] != ds || sh1[1][mt] != a1 || sh2[1][mt] != a2) continue;
        const uint32_t pt = (uint32_t)__popc(mt);
        const uint32_t key = ((16u - ps - pt) << 20) | ((8u - pt) << 16) | (ms << 8) | mt;
        if (key > floor && key < best) best = key;
      }
    }
    for (int off = 32; off; off >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, off));
    if (best == 0xffffffffu) break;   // (uniform) no candidate is left: NOSUBSET
    const uint32_t ms = (best >> 8) & 255u, mt = best & 255u;
    if (t < 2) {   // (side t: the pieces of its subset)
      const uint32_t m = t ? mt : ms;
      const int n = t ? nf1 : nf0;
      int32_t d = 0;
      int c = 0;
      for (int i = 0; i < n; ++i) {
        if (!((m >> i) & 1u)) continue;
        vq[t][c] = fq[t][i]; vla[t][c] = fla[t][i]; vab[t][c] = fab[t][i];
        vst[t][c] = fq[t][i] - ws + d;
        d += (int32_t)fla[t][i] - (int32_t)flr[t][i];
        ++c;
      }
      vn[t] = c;
      dlt[t] = d;
      tot[t] = W + d;
    }
    __syncthreads();
    bool differ = tot[0] != tot[1];
    if (!differ) {
      for (int32_t o = t; o < tot[0]; o += 64) {
        uint32_t sym[2];
#pragma unroll
        for (int sd = 0; sd < 2; ++sd) {
          const int n = vn[sd];
          int32_t gq = ws + o - dlt[sd];   // behind the last piece
          uint32_t c = 16u;
          for (int i = 0; i < n; ++i) {
            const int32_t b0 = vst[sd][i];
            if (o < b0) { gq = o - b0 + vq[sd][i]; break; }
            if (o < b0 + (int32_t)vla[sd][i]) { c = (vab[sd][i] >> (2 * (o - b0))) & 3u; break; }
          }
          sym[sd] = c < 16u ? c : hp_base(S.words, max(min(max(gq, ws), wend), 1));   // (ws <= gq <= wend as it is: the load stays inside the genome whatever the tables hold)
        }
        differ = differ || sym[0] != sym[1];
      }
    }
    const bool same = !__ballot(differ);
    __syncthreads();   // (the piece tables are rebuilt in the next round)
    if (same) { found = best; break; }
    floor = best;
  }
  // what became of the site
  const uint32_t ms = (found >> 8) & 255u, mt = found & 255u;
  const bool in = have && found && (((side ? mt : ms) >> frank) & 1u);
  bool gained = false;
  if (found && have) {
    if (!side) {
      const int64_t gi = V.off + pr[3 + k];
      gained = in && (P.flags[gi] & QMF_IDDOT) && !((P.mask_tp[gi >> 6] >> (int)(gi & 63)) & 1ull);
      if (P.cls_s) P.cls_s[gi] = (uint8_t)(in ? HAP_SUBSET : HAP_LEFT);
    } else if (P.ecls_s && V.ecls) {
      P.ecls_s[(V.ecls - P.ecls) + ent[k]] = (uint8_t)(in ? HAP_SUBSET : HAP_LEFT);
    }
  }
  const uint64_t mi = __ballot(in), mg = __ballot(gained);
  if (t == 0) {
    unsigned long long* o = reinterpret_cast<unsigned long long*>(P.sub) + (int64_t)v * HAPSUB_COLS;
    atomicAdd(o + HAPSUB_SEARCHED, 1ull);
    atomicAdd(o + (found ? HAPSUB_PARTIAL : HAPSUB_NOSUBSET), 1ull);
    if (found) {
      const int rl = __popcll(mi & 0xffull), fe = __popcll(mi & 0xff00ull);
      atomicAdd(o + HAPSUB_RESCUED_S, (unsigned long long)rl);
      atomicAdd(o + HAPSUB_FOUND_S, (unsigned long long)fe);
      if (mg) atomicAdd(o + HAPSUB_TP_S, (unsigned long long)__popcll(mg));
      if (nrec - rl) atomicAdd(o + HAPSUB_LEFT_LINES, (unsigned long long)(nrec - rl));
      if (nent - fe) atomicAdd(o + HAPSUB_LEFT_ENTRIES, (unsigned long long)(nent - fe));
    }
    P.res[blockIdx.x] = found ? (HAPSUB_RES_PARTIAL | (found & 0xffffu)) : HAPSUB_RES_NOSUBSET;
  }
}

// ---- launchers ----
void launch_hap_subsets(const HapSubParams& P, hipStream_t st) {
  if (P.n_vcf > 0) hipLaunchKernelGGL(k_hap_subsets_init, dim3((unsigned)((P.n_vcf + 255) / 256)), dim3(256), 0, st, P);
  if (P.n_pairs > 0) hipLaunchKernelGGL(k_hap_subsets, dim3((unsigned)P.n_pairs), dim3(64), 0, st, P);
}

void launch_hap_sites(const HapSites& S, hipStream_t st) {
  if (S.xn > 0) hipLaunchKernelGGL(k_hap_entries, dim3((unsigned)((S.xn + 255) / 256)), dim3(256), 0, st, S);
  hipLaunchKernelGGL(k_hap_sites, dim3(1), dim3(256), 0, st, S);
  if (S.xn > 0) hipLaunchKernelGGL(k_hap_windows, dim3((unsigned)((S.xn + 255) / 256)), dim3(256), 0, st, S);
}

void launch_hap_records(const HapRecParams& P, hipStream_t st) {
  if (P.n_spans <= 0) return;
  hipLaunchKernelGGL(k_hap_records, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

// (the y dimension of a grid holds 65535 blocks: qm_batch_haplotypes refuses a batch of more VCFs)
void launch_hap_truth(const HapVcf* vcfs, int n_vcf, int64_t max_entries, uint64_t* tru, unsigned long long* total, hipStream_t st) {
  if (n_vcf > 0 && max_entries > 0)
    hipLaunchKernelGGL(k_hap_truth, dim3((unsigned)((max_entries + 255) / 256), (unsigned)n_vcf), dim3(256), 0, st, vcfs,
                       reinterpret_cast<unsigned long long*>(tru));
  hipLaunchKernelGGL(k_hap_rank, dim3(1), dim3(256), 0, st, vcfs, n_vcf, total);
}

void launch_hap_claim(const HapRecParams& P, int n_vcf, int64_t max_entries, hipStream_t st) {
  if (n_vcf <= 0 || max_entries <= 0 || P.n_spans <= 0) return;
  const unsigned gx = (unsigned)((max_entries / 32 + 1 + 255) / 256);
  const HapVcf* vcfs = P.vcfs;
  int32_t* pairs = P.pairs;
  hipLaunchKernelGGL(k_hap_pairs, dim3(gx, (unsigned)n_vcf), dim3(256), 0, st, vcfs, pairs);
  hipLaunchKernelGGL(k_hap_claim, dim3(pass_grid(P.n_spans)), dim3(256), 0, st, P);
}

void launch_hap_replay(const HapReplayParams& P, hipStream_t st) {
  if (P.n_pairs <= 0) return;
  hipLaunchKernelGGL(k_hap_replay, dim3((unsigned)P.n_pairs), dim3(64), 0, st, P);
}

}  // namespace qm
