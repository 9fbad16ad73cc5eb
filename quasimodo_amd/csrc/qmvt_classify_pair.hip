// qmvt_classify_pair.hip -- k_classify_pair: the classification of sorted, single-base, column-input batches (the flagship
// shape), a translation unit of its own outside the kernels id.
//
// It is k_classify<false, false> of qmvt_kernels.hip -- one wave per span, no barriers, the same ClassifyParams, the same
// outputs bit for bit -- with ONE change of schedule: two consecutive rounds of 256 records are unpacked and staged side by
// side, and the truth keys of the pair's position range are joined against the 512 staged keys at once.  At the flagship's
// densities a round meets about 26 truth keys, so 26 of 64 lanes ran the bisect and the walk while all 64 paid for them, and
// the range count and the glue around it were paid per round whatever the number of keys; a pair puts about 51 keys on the
// 64 lanes for one bisect step more.  The per-record pass still runs per round (each half with its own hit nibbles, its own
// predecessor position and its own mask slot), and a tile whose truth slice is too large for LDS is still joined round by
// round, chunk by chunk, as before.
//
// Why the results are the same: whether a record is hit depends on its key and the tile's slice only; the per-truth-entry
// state (smax / srf) is accumulated over the tile, and the tile still owns it; histogram adds commute.  What depends on the
// ROUND -- which records are loaded, whose positions enter the position-OR, how many mask words of a ragged end are
// stored -- keeps the round as its unit here.
//
// A full pair whose 512 records are live and strictly ascending -- every pair of the flagship, most pairs of a real sorted
// VCF -- is "plain": one test on the raw loads sends it through specialisations of the unpack, the join and the per-record pass
// that carry no liveness select, no order test, no repeated-position ladder and no walk of a run (plain_pair below).
//
// The device helpers are this file's own copies (namespace qm::cpair): qmvt_kernels.hip and qmvt_dev.h do not change.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qmvt_classify_pair.h"

namespace qm {
namespace cpair {

template <typename T> __device__ __forceinline__ T ntl(const T* p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ uint64_t ballot64(bool p) { return __ballot(p); }
__device__ __forceinline__ int popc64(uint64_t x) { return __popcll(x); }

__device__ __forceinline__ int qual_bin(float q, int n_bins) {
  if (!(q >= 0.0f)) return -1;
  if (q >= (float)n_bins) return n_bins - 1;
  return (int)q;
}

// info of a record (the layout of qmvt_kernels.hip: k_compact and the sort path never see it, the rare paths below repack it)
constexpr uint32_t I_BIN1 = 0x1ffu;
constexpr uint32_t I_PASS = 1u << 9;
constexpr uint32_t I_IDDOT = 1u << 10;
constexpr uint32_t I_NOKEY = 1u << 11;
constexpr uint32_t I_LIVE = 1u << 12;
constexpr uint32_t I_BADPOS = 1u << 13;
constexpr uint32_t I_KEPT = 1u << 16;
constexpr uint32_t I_IDDOT4 = 1u << 20;
constexpr uint32_t I_TPLINE = 1u << 24;

// one record from its columns, any position (the rare paths: run continuation, repeated keys)
__device__ __forceinline__ void pack_record(int p, uint32_t d, float q, uint32_t fl, int nb, uint32_t& key, uint32_t& inf) {
  d &= 0xffu;
  const bool okpos = (uint32_t)p < (uint32_t)QM_POS_LIMIT_DEV;
  const bool live = okpos && d < 16u;
  key = ((uint32_t)p << 4) | (live ? d : 0u);
  inf = (live ? (uint32_t)(qual_bin(q, nb) + 1) : 0u) | ((fl & 7u) << 9) | (live ? I_LIVE : 0u) | (okpos ? 0u : I_BADPOS) |
        ((live && (fl & QMF_PASS)) ? I_KEPT : 0u) | ((fl & QMF_IDDOT) ? I_IDDOT4 : 0u) | ((live && (fl & QMF_TPLINE)) ? I_TPLINE : 0u);
}
__device__ __forceinline__ uint32_t flag_info(uint32_t f) {
  return ((f & 7u) << 9) | I_LIVE | ((f & QMF_PASS) ? I_KEPT : 0u) | ((f & QMF_IDDOT) ? I_IDDOT4 : 0u) | ((f & QMF_TPLINE) ? I_TPLINE : 0u);
}
// (int)floorf(c) in ONE vector instruction instead of two (c is a number in [-1, 255] here: no saturation, no NaN)
__device__ __forceinline__ int floor_to_int(float c) {
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(c));
  return r;
}
// the main loop's packer: one LDS read per record; a record out of range is caught by the round's position-OR
// (PLAIN: a record of a plain pair -- in range and single-base by the pair's test, so `live` is a constant)
template <bool PLAIN>
__device__ __forceinline__ void pack_record_fast(int p, uint32_t d, float q, uint32_t f4x4, float nbm1f, const uint32_t* flut,
                                                 uint32_t& key, uint32_t& inf) {
  const bool live = PLAIN || ((uint32_t)p | (d << 24)) < (uint32_t)QM_POS_LIMIT_DEV;
  key = ((uint32_t)p << 4) | (live ? d : 0u);
  const float c = fminf(fmaxf(q, -1.0f), nbm1f);   // NaN -> -1
  const uint32_t b1 = (uint32_t)(floor_to_int(c) + 1);
  const uint32_t g = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(flut) + f4x4);
  inf = live ? (b1 | g) : 0u;
}

struct Cols {
  const int32_t* pos;
  const float* qual;
  const uint8_t* flags;
  const uint8_t* anib;
};
struct Raw4 { int4 p; float4 q; uint32_t f, d; };   // one round's loads of a lane, still in flight
struct In4 { uint32_t key[4], inf[4], posor; };     // the lane's 4 records of a round, packed

__device__ __forceinline__ void load_raw(const Cols& C, int idx, Raw4& R) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  typedef float v4f __attribute__((ext_vector_type(4)));
  const v4i vp = __builtin_nontemporal_load(reinterpret_cast<const v4i*>(C.pos + idx));
  R.d = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(C.anib + idx));
  const v4f vq = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(C.qual + idx));
  R.p = make_int4(vp.x, vp.y, vp.z, vp.w);
  R.q = make_float4(vq.x, vq.y, vq.z, vq.w);
  R.f = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(C.flags + idx));
}
template <bool PLAIN>
__device__ __forceinline__ void unpack_raw(const Raw4& R, float nbm1f, In4& X, const uint32_t* flut) {
  pack_record_fast<PLAIN>(R.p.x, R.d & 0xffu, R.q.x, (R.f << 2) & 0x3cu, nbm1f, flut, X.key[0], X.inf[0]);
  pack_record_fast<PLAIN>(R.p.y, (R.d >> 8) & 0xffu, R.q.y, (R.f >> 6) & 0x3cu, nbm1f, flut, X.key[1], X.inf[1]);
  pack_record_fast<PLAIN>(R.p.z, (R.d >> 16) & 0xffu, R.q.z, (R.f >> 14) & 0x3cu, nbm1f, flut, X.key[2], X.inf[2]);
  pack_record_fast<PLAIN>(R.p.w, R.d >> 24, R.q.w, (R.f >> 22) & 0x3cu, nbm1f, flut, X.key[3], X.inf[3]);
  X.posor = (uint32_t)R.p.x | (uint32_t)R.p.y | (uint32_t)R.p.z | (uint32_t)R.p.w;
}

// wave-uniform single values go through the scalar cache (they count on lgkmcnt and never drain the vector prefetch)
typedef const __attribute__((address_space(4))) int32_t* ci32p;
__device__ __forceinline__ int uload(const int32_t* p, int i) { return ((ci32p)(uintptr_t)p)[i]; }
__device__ __forceinline__ void rec_packed(const Cols& C, int i, int nb, uint32_t& key, uint32_t& inf) {
  pack_record(C.pos[i], C.anib[i], C.qual[i], C.flags[i], nb, key, inf);
}

typedef const __attribute__((address_space(1))) uint32_t* gu32p;
typedef const __attribute__((address_space(1))) int32_t* gi32p;
struct TruthG { gu32p keys; gi32p tidx; int32_t shift, nb; };

// ---- LDS layout of the wave (dword offsets into one array) -----------------------------------------------------------------
// The histograms, the slice and its state, the flag table, the tile counts and the mask batch are k_classify's; the record
// staging holds a PAIR: 512 keys (16 blocks of 32 keys + 4 dwords of padding each: the bisect's probes of one step land on
// different banks), 512 u16 infos, 16 hit words.
constexpr int PAIR = 512;
constexpr int L_HTP = 0;   // (classify_half's histogram address relies on the 0)
constexpr int L_HFP = 130;
constexpr int L_HU = 260;
constexpr int L_KEYS = 388;
constexpr int L_SMAX = L_KEYS + K1_SLICE;
constexpr int L_SRF = L_SMAX + K1_SLICE;
constexpr int L_RKEY = (L_SRF + K1_SLICE / 32 + 3) & ~3;
constexpr int RKEY_PAD = PAIR + (PAIR / 32) * 4;   // 576
constexpr int L_RINF = L_RKEY + RKEY_PAD;
constexpr int L_HITS = L_RINF + PAIR / 2;
constexpr int L_FLUT = L_HITS + PAIR / 32;
constexpr int L_TCNT = L_FLUT + 16;
#ifndef QM_PAIR_MASK_TILES
#define QM_PAIR_MASK_TILES 8
#endif
constexpr int MASK_TILES = QM_PAIR_MASK_TILES;
constexpr int L_MASK = (L_TCNT + 2 * SPAN_TILES + 3) & ~3;
constexpr int L_TOTAL = L_MASK + 64 * MASK_TILES;
static_assert(L_RKEY % 4 == 0 && L_RINF % 2 == 0 && L_MASK % 4 == 0, "b128 / b64 LDS accesses need natural alignment");
static_assert(K1_ROUNDS == 4, "a tile is two pairs, 32 + 32 mask words");
static_assert(SPAN_TILES % MASK_TILES == 0, "mask batches tile the span");
static_assert(K1_SLICE % 64 == 0, "the next tile's slice waits in K1_SLICE / 64 registers per lane");

__device__ __forceinline__ void hist_add(uint32_t* lds, int table, uint32_t slot) {
  atomicAdd(&lds[table + (slot >> 1)], 1u << (16u * (slot & 1u)));
}
__device__ __forceinline__ uint32_t hist_get(const uint32_t* lds, int table, uint32_t slot) {
  return (lds[table + (slot >> 1)] >> (16u * (slot & 1u))) & 0xffffu;
}

// logical record index of the pair -> dword of its staged key
__host__ __device__ constexpr int rk(int i) { return L_RKEY + i + ((i >> 5) << 2); }
// padded -> logical: pp / 36 blocks of padding lie below padded index pp.  The bisect never stops on padding, and the
// multiply-shift below is the exact quotient for every padded index of a pair (checked here, index by index).
constexpr uint32_t DIV36_MUL = 7282u, DIV36_SHIFT = 18u;
__host__ __device__ constexpr int unpad(int pp) { return pp - 4 * (int)(((uint32_t)pp * DIV36_MUL) >> DIV36_SHIFT); }
constexpr bool unpad_exact() {
  for (int pp = 0; pp < RKEY_PAD; ++pp) {
    if ((int)(((uint32_t)pp * DIV36_MUL) >> DIV36_SHIFT) != pp / 36) return false;
    if (pp % 36 < 32 && rk(unpad(pp)) != L_RKEY + pp) return false;   // a key's dword maps back to its record
  }
  for (int i = 0; i < PAIR; ++i)
    if (unpad(rk(i) - L_RKEY) != i) return false;
  return true;
}
static_assert(unpad_exact(), "padded -> logical index of the staged keys must be exact up to the last padded dword");

struct Slice { int m; };   // keys staged at L_KEYS (state at L_SMAX / L_SRF)

__device__ __forceinline__ void stage_slice(uint32_t* lds, const TruthG& tr, int c0, const Slice& S, int lane) {
  for (int j = lane; j < S.m; j += 64) {
    lds[L_KEYS + j] = tr.keys[c0 + j];
    lds[L_SMAX + j] = 0;
  }
  if (lane < K1_SLICE / 32) lds[L_SRF + lane] = 0;
}
__device__ __forceinline__ void slice_range(const TruthG& tr, int a, int b, int& lo, int& hi) {
  uint32_t ba = (uint32_t)a >> tr.shift;
  uint32_t bb = ((uint32_t)b >> tr.shift) + 1u;
  const uint32_t lim = (uint32_t)tr.nb + 1u;
  ba = ba < lim ? ba : lim;
  bb = bb < lim ? bb : lim;
  lo = uload((const int32_t*)(uintptr_t)tr.tidx, (int)ba);
  hi = uload((const int32_t*)(uintptr_t)tr.tidx, (int)bb);
  if (hi < lo) hi = lo;   // only on unsorted input (results discarded)
}
struct SegBounds { int a, b, prevp, nextp; };
__device__ __forceinline__ SegBounds seg_bounds(const Cols& C, int sb, int se, int vn) {
  SegBounds t;
  t.a = uload(C.pos, sb);
  t.b = uload(C.pos, se - 1);
  t.prevp = (sb > 0) ? uload(C.pos, sb - 1) : INT32_MIN;
  t.nextp = (se < vn) ? uload(C.pos, se) : INT32_MIN;
  return t;
}

// ---- phase A: one round's keys and infos into its half of the pair's staging -------------------------------------------------
// records at or beyond `te` become key 0xffffffff (sorts last, matches nothing), info 0: a ragged end, or a whole second half
__device__ __forceinline__ void stage_half(uint32_t* lds, In4& X, int half, int i0, int te, int lane) {
  if (i0 - lane * 4 + 256 > te) {   // wave-uniform
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (i0 + k >= te) { X.key[k] = 0xffffffffu; X.inf[k] = 0u; }
  }
  uint4 kv;
  kv.x = X.key[0]; kv.y = X.key[1]; kv.z = X.key[2]; kv.w = X.key[3];
  uint2 iv;
  iv.x = (X.inf[0] & 0xffffu) | (X.inf[1] << 16); iv.y = (X.inf[2] & 0xffffu) | (X.inf[3] << 16);
  *reinterpret_cast<uint4*>(&lds[L_RKEY + half * (RKEY_PAD / 2) + lane * 4 + ((lane >> 3) << 2)]) = kv;
  *reinterpret_cast<uint2*>(&lds[L_RINF + half * (PAIR / 4) + lane * 2]) = iv;
}

// ---- phase B: the truth keys of a position range search the staged records ----------------------------------------------------
// NREC = 512: the whole pair (records 0 .. nrec - 1 of it); NREC = 256: the half that starts at record `r0` (0 or 256), for
// the round-by-round path of an oversize slice.  own_a: INT32_MIN when the segment owns the run at its first position, else
// that position (the run started in an earlier segment, which owns its truth entries).
// PLAIN (a plain pair: strictly ascending, every record live, own_a == INT32_MIN): a truth key's position holds at most one
// staged record, so the walk of the run is one straight-line trip.
template <int NREC, bool PLAIN>
__device__ __forceinline__ void join_staged(uint32_t* lds, const Slice& S, int r0, int nrec, int own_a, int lane) {
  if (S.m <= 0 || nrec <= 0) return;
  const int kb = L_RKEY + r0 + ((r0 >> 5) << 2);   // first staged key of the searched records
  const uint32_t first_pos = lds[kb] >> 4;
  const uint32_t last_pos = lds[rk(r0 + nrec - 1)] >> 4;
  int rlo = 0, rhi = 0;
  for (int base = 0; base < S.m; base += 64) {
    const int j = base + lane;
    const uint32_t kp = j < S.m ? lds[L_KEYS + j] >> 4 : 0xffffffffu;
    rlo += popc64(ballot64(kp < first_pos));
    rhi += popc64(ballot64(kp <= last_pos));
  }
  for (int base = rlo; base < rhi; base += 64) {
    const int j = base + lane;
    if (j < rhi) {
      const uint32_t kkey = lds[L_KEYS + j];
      const uint32_t kpos = kkey >> 4;
      const uint32_t kfloor = kkey & ~15u;
      // first staged record with position >= kpos: a branch-free lower bound in the PADDED index space (36 dwords per block
      // of 32 keys): the first steps pick the block, five the key inside it, none of them crosses padding
      int pp = 0;
#pragma unroll
      for (int st = (NREC / 64) * 36; st >= 36; st >>= 1)
        if (lds[kb + pp + st - 5] < kfloor) pp += st;   // last key of the block(s) below: logical 32 b - 1 = padded 36 b - 5
#pragma unroll
      for (int st = 16; st > 0; st >>= 1)
        if (lds[kb + pp + st - 1] < kfloor) pp += st;
      int s = unpad(pp);
      if (lds[kb + pp] < kfloor) s += 1;   // the last key of all still below
      s += r0;
      const int send = r0 + nrec;
      uint32_t mx = 0, rf = 0;
      if constexpr (PLAIN) {   // the one record that can carry this key (no LDS word behind the staged keys is read)
        if (s < send && lds[rk(s)] == kkey) {
          const uint32_t inf = (lds[L_RINF + (s >> 1)] >> (16 * (s & 1))) & 0xffffu;
          if ((inf & (I_LIVE | I_NOKEY)) == I_LIVE) {
            atomicOr(&lds[L_HITS + (s >> 5)], 1u << (s & 31));
            if (inf & I_IDDOT) mx = inf & I_BIN1;
            rf = (inf & I_PASS) ? 1u : 0u;
          }
        }
      } else {
        for (; s < send; ++s) {   // the run of records at this position
          const uint32_t rkey = lds[rk(s)];
          if ((rkey & ~15u) != kfloor) break;
          if (rkey != kkey) continue;
          const uint32_t inf = (lds[L_RINF + (s >> 1)] >> (16 * (s & 1))) & 0xffffu;
          if ((inf & (I_LIVE | I_NOKEY)) != I_LIVE) continue;
          atomicOr(&lds[L_HITS + (s >> 5)], 1u << (s & 31));
          if ((int)kpos != own_a) {
            const uint32_t b1 = inf & I_BIN1;
            if ((inf & I_IDDOT) && b1 > mx) mx = b1;
            rf |= (inf & I_PASS) ? 1u : 0u;
          }
        }
      }
      if (mx) atomicMax(&lds[L_SMAX + j], mx);
      if (rf) atomicOr(&lds[L_SRF + (j >> 5)], 1u << (j & 31));
    }
  }
}

__device__ __forceinline__ int slice_lower_bound(const uint32_t* lds, const Slice& S, uint32_t key) {
  int lo = 0, n = S.m;
  while (n > 0) {
    const int h = n >> 1;
    if (lds[L_KEYS + lo + h] < key) { lo += h + 1; n -= h + 1; } else n = h;
  }
  return lo;
}
// records after the segment that continue its last run of equal positions
__device__ __forceinline__ void continue_run(const Cols& C, uint32_t* lds, const Slice& S, int se, int vn, int bpos, int nb, int lane) {
  for (int base = se; base < vn; base += 64) {
    const int i = base + lane;
    bool cont = false;
    if (i < vn) {
      cont = (C.pos[i] == bpos);
      if (cont && S.m > 0) {
        uint32_t key, inf;
        rec_packed(C, i, nb, key, inf);
        if ((inf & (I_LIVE | I_NOKEY)) == I_LIVE) {
          const int j = slice_lower_bound(lds, S, key);
          if (j < S.m && lds[L_KEYS + j] == key) {
            if (inf & I_IDDOT) atomicMax(&lds[L_SMAX + j], inf & I_BIN1);
            if (inf & I_PASS) atomicOr(&lds[L_SRF + (j >> 5)], 1u << (j & 31));
          }
        }
      }
    }
    if (ballot64(cont) != ~0ull) break;
  }
}
__device__ __forceinline__ uint32_t flush_slice(uint32_t* lds, const Slice& S, int lane) {
  uint32_t tpr = 0;
  for (int j = lane; j < S.m; j += 64) {
    const uint32_t mx = lds[L_SMAX + j];
    if (mx) hist_add(lds, L_HU, mx - 1u);
    tpr += (lds[L_SRF + (j >> 5)] >> (j & 31)) & 1u;
  }
  return tpr;
}
// has a kept record with this key been seen earlier in the VCF?  (the predecessor has the same position: walk its run backwards)
__device__ __forceinline__ uint32_t repeated_key(const Cols& C, int i, uint32_t key, uint32_t nokey, int nb) {
  for (int j = i - 1; j >= 0; --j) {
    if (C.pos[j] != (int)(key >> 4)) break;
    uint32_t kj, ij;
    rec_packed(C, j, nb, kj, ij);
    if (kj == key && (ij & (I_LIVE | I_PASS)) == (I_LIVE | I_PASS) && (ij & I_NOKEY) == nokey) return 1u;
  }
  return 0u;
}

struct Acc {
  uint32_t bad;              // per lane: bit0 order violated, bit1 position out of range
  uint32_t fpr;              // per lane: distinct kept keys outside the truth set
  uint32_t n_pass, n_tp;     // per lane: kept / TP lines of the current tile
  uint32_t top_tp, top_fp;   // wave-uniform: records of the saturated top bin
  uint32_t posor;            // per lane: OR of the positions seen
};

__device__ __forceinline__ uint32_t or_reduce8(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
  return v;
}

// ---- phase C: per-record work on the packed registers of ONE round (a half of the pair) ---------------------------------------
// hword: the half's first hit word; prev_last: position of the record before the round; mslot: the round's first mask word
// PLAIN (a half of a plain pair): every position is in range and above its predecessor, so no order or range bit is set, no
// record repeats its predecessor's position (no `cand`, no repeated_key) and the predecessor is never fetched
template <bool PLAIN>
__device__ __forceinline__ void classify_half(uint32_t* lds, const Cols& C, const In4& X, int hword, int rbase, int prev_last, int nb,
                                              int mslot, Acc& A, int lane) {
  const uint32_t hit = (lds[hword + (lane >> 3)] >> (4 * (lane & 7))) & 15u;
  uint32_t nib = 0, anyinf = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    nib |= (X.inf[k] >> 16) << k;
    anyinf |= X.inf[k];
  }
  const uint32_t pass = nib & 15u, iddot = (nib >> 4) & 15u, tpline = (nib >> 8) & 15u;
  if (!PLAIN) A.bad |= ((anyinf & I_BADPOS) | (X.posor >> 28)) ? 2u : 0u;
  A.posor |= X.posor;
  const uint32_t tpkey = (hit & iddot) | tpline;
  const uint32_t tp = pass & tpkey;
  const uint32_t fpkey = pass & ~hit;
  A.n_pass += (uint32_t)__popc(pass);
  A.n_tp += (uint32_t)__popc(tp);
  A.fpr += (uint32_t)__popc(fpkey);
  {
    const uint32_t sh = 4u * (uint32_t)(lane & 7);
    const uint32_t wp = or_reduce8(pass << sh);
    const uint32_t wt = or_reduce8(tp << sh);
    if ((lane & 7) == 7) {
      lds[L_MASK + mslot + (lane >> 3)] = wp;
      lds[L_MASK + 32 * MASK_TILES + mslot + (lane >> 3)] = wt;
    }
  }
  int pp = 0;
  if (!PLAIN) {
    pp = __shfl_up((int)(X.key[3] >> 4), 1);
    if (lane == 0) pp = prev_last;
  }
  const int i0 = rbase + lane * 4;
  uint32_t cand = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = (int)(X.key[k] >> 4);
    if (!PLAIN) {
      A.bad |= (p < pp) ? 1u : 0u;
      cand |= ((p == pp) ? 1u : 0u) << k;
    }
    {
      const uint32_t b1 = X.inf[k] & I_BIN1;
      const uint32_t notp = ((~tpkey) >> k) & 1u;
      const bool top = b1 == (uint32_t)nb;
      const uint64_t mtop = ballot64(top);
      if (mtop) {   // wave-uniform: the saturated top bin is counted with ballots, its lanes sit out the LDS add
        const uint32_t ntp = (uint32_t)popc64(ballot64(top && !notp));
        A.top_tp += ntp;
        A.top_fp += (uint32_t)popc64(mtop) - ntp;
      }
      if (!top) atomicAdd(&lds[(b1 >> 1) + notp * (uint32_t)L_HFP], 1u << ((b1 << 4) & 31u));   // hist_add(notp ? L_HFP : L_HTP, b1), L_HTP == 0
    }
    pp = p;
  }
  cand &= fpkey;
  if (cand) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((cand >> k) & 1u) A.fpr -= repeated_key(C, i0 + k, X.key[k], X.inf[k] & I_NOKEY, nb);
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#define QM_DPP_ADD(ctrl, rmask) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rmask, 0xf, false)
  QM_DPP_ADD(0xb1, 0xf);
  QM_DPP_ADD(0x4e, 0xf);
  QM_DPP_ADD(0x141, 0xf);
  QM_DPP_ADD(0x140, 0xf);
  QM_DPP_ADD(0x142, 0xa);
  QM_DPP_ADD(0x143, 0xc);
#undef QM_DPP_ADD
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

// one round of an oversize tile (dense truth against a sparse VCF): the round is its own owner of truth state, its slice is
// walked in chunks staged on the spot -- or, out of order, flags the VCF (it is redone through the sort: nothing to join)
__device__ __forceinline__ void oversize_round(uint32_t* lds, const Cols& C, const TruthG& tr, const In4& X, Slice& S, int r0, int rbase,
                                               int rend, int vn, int nb, Acc& A, uint32_t& acc_tpr, int lane) {
  const int pl = __shfl_up((int)(X.key[3] >> 4), 1);
  const bool ooo = (lane > 0 && X.key[0] != 0xffffffffu && (int)(X.key[0] >> 4) < pl) ||
                   (X.key[1] < (X.key[0] & ~15u)) || (X.key[2] < (X.key[1] & ~15u)) || (X.key[3] < (X.key[2] & ~15u));
  if (ballot64(ooo) != 0ull) {
    A.bad |= 1u;
    return;
  }
  const SegBounds RB = seg_bounds(C, rbase, rend, vn);
  const bool r_started = (rbase > 0) && (RB.prevp == RB.a);
  const int r_own_a = r_started ? RB.a : INT32_MIN;
  int rlo, rhi;
  slice_range(tr, RB.a, RB.b, rlo, rhi);
  for (int c0 = rlo; c0 < rhi; c0 += K1_SLICE) {
    S.m = (rhi - c0) < K1_SLICE ? (rhi - c0) : K1_SLICE;
    stage_slice(lds, tr, c0, S, lane);
    __syncthreads();
    join_staged<256, false>(lds, S, r0, rend - rbase, r_own_a, lane);
    if (RB.nextp == RB.b && !(r_started && RB.a == RB.b)) continue_run(C, lds, S, rend, vn, RB.b, nb, lane);
    __syncthreads();
    acc_tpr += flush_slice(lds, S, lane);
    __syncthreads();
  }
  S.m = 0;
}

// ---- the plain pair ---------------------------------------------------------------------------------------------
// Decided once per FULL pair on the raw loads, one ballot: each of the 512 positions is above its predecessor (inside a lane
// the record in front of it, across lanes the previous lane's fourth record, for lane 0 the record before the half), no position
// has a bit at or above 28 (which also rejects a negative one), no allele byte is ANIB_NONE.  Such a pair holds none of what the
// general path tests per record -- a dead or out-of-range record, a descent, a repeated position -- and runs through the PLAIN
// specialisations of the unpack, the join and the per-record pass, in which those conditions are compile-time constants.
#ifndef QM_PAIR_PLAIN
#define QM_PAIR_PLAIN 1   // 0: the test is constant false and the kernel is the general path alone (the A/B arm)
#endif
__device__ __forceinline__ bool plain_pair(const Raw4& N0, const Raw4& N1, int prev_last, int lane) {
  int pp0 = __shfl_up(N0.p.w, 1), pp1 = __shfl_up(N1.p.w, 1);
  const int last0 = __builtin_amdgcn_readlane(N0.p.w, 63);
  if (lane == 0) { pp0 = prev_last; pp1 = last0; }
  const bool asc = (N0.p.x > pp0) & (N0.p.y > N0.p.x) & (N0.p.z > N0.p.y) & (N0.p.w > N0.p.z) &
                   (N1.p.x > pp1) & (N1.p.y > N1.p.x) & (N1.p.z > N1.p.y) & (N1.p.w > N1.p.z);
  const uint32_t por = (uint32_t)(N0.p.x | N0.p.y | N0.p.z | N0.p.w | N1.p.x | N1.p.y | N1.p.z | N1.p.w);
  const bool ok = asc & (((por & 0xf0000000u) | ((N0.d | N1.d) & 0xf0f0f0f0u)) == 0u);
  return ballot64(!ok) == 0ull;
}

#ifndef QM_PAIR_WAVES_PER_EU
#define QM_PAIR_WAVES_PER_EU 4   // 128 VGPRs: two rounds in flight and two unpacked across the join; LDS holds 17 waves per CU
#endif

__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(QM_PAIR_WAVES_PER_EU, 5))) void k_classify_pair(ClassifyParams P) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[L_TOTAL];

  const int lane = (int)threadIdx.x;
  const int span_id = (int)blockIdx.x + P.span_base;
  const SpanDesc sp = P.spans[span_id];
  TruthG tr;
  {
    const TruthDev& t = P.truths[sp.truth];
    tr.keys = (gu32p)t.keys; tr.tidx = (gi32p)t.tidx; tr.shift = t.shift; tr.nb = t.nb;
  }
  Cols C;
  C.pos = P.pos + sp.voff; C.qual = P.qual + sp.voff; C.flags = P.flags + sp.voff; C.anib = P.anib + sp.voff;
  uint32_t* const mpass32 = reinterpret_cast<uint32_t*>(P.mask_pass + (sp.voff >> 6));
  uint32_t* const mtp32 = reinterpret_cast<uint32_t*>(P.mask_tp + (sp.voff >> 6));
  const int vn = sp.vn;
  const int sp_end = (int)(sp.end - sp.voff);
  const int nb = P.n_bins;
  const float nbm1f = (float)(nb - 1);

  for (int i = lane; i < L_KEYS; i += 64) lds[i] = 0;   // histograms
  if (lane < 16) lds[L_FLUT + lane] = flag_info((uint32_t)lane);
  if (P.zero_acc && blockIdx.x == 0)
    for (int i = lane; i < P.zero_words; i += 64) P.zero_acc[i] = 0ull;
  if (P.known && P.known[sp.vcf]) return;   // found out of order by an earlier run of the same columns: the span's rows still say so
  Acc A = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  uint32_t acc_pass = 0, acc_tp = 0;  // wave-uniform
  uint32_t acc_tpr = 0;               // per lane, reduced at the end

  // ---- prologue: first pair in flight, first tile's bounds and slice ---------------------------------------------------------
  int tb = (int)(sp.begin - sp.voff);
  int te = (tb + K1_TILE < sp_end) ? tb + K1_TILE : sp_end;
  Raw4 N0, N1 = {};
  load_raw(C, tb + lane * 4, N0);
  if (tb + 256 < sp_end) load_raw(C, tb + 256 + lane * 4, N1);
  // sixty-four records spread evenly over the WHOLE VCF, one per lane: the same 64 lines for every span of the VCF
  int spos = 0;
  if (vn >= 4096) spos = C.pos[(int)(((int64_t)lane * vn) >> 6)];
  SegBounds B = seg_bounds(C, tb, te, vn);
  {
    // A span whose FIRST round is out of order, or whose VCF's sixty-four samples are, leaves here: what stays behind is the
    // flag and the position bits of the round (and of the samples).  Only positions in range count -- a round with a bad one
    // takes the long way and is flagged there.
    const int n0 = te - tb < 256 ? te - tb : 256;
    const int j = lane * 4;
    const int pl = __shfl_up(N0.p.w, 1);
    const bool ooo = (j + 1 < n0 && N0.p.y < N0.p.x) || (j + 2 < n0 && N0.p.z < N0.p.y) || (j + 3 < n0 && N0.p.w < N0.p.z) || (lane > 0 && j < n0 && N0.p.x < pl);
    uint32_t po = (j < n0 ? (uint32_t)N0.p.x : 0u) | (j + 1 < n0 ? (uint32_t)N0.p.y : 0u) | (j + 2 < n0 ? (uint32_t)N0.p.z : 0u) | (j + 3 < n0 ? (uint32_t)N0.p.w : 0u);
    const int spl = __shfl_up(spos, 1);
    const bool sooo = vn >= 4096 && lane > 0 && spos < spl;
    po |= vn >= 4096 ? (uint32_t)spos : 0u;
    if (ballot64(ooo || sooo) != 0ull && ballot64((po >> 28) != 0u) == 0ull) {
      for (int o = 32; o > 0; o >>= 1) po |= (uint32_t)__shfl_xor((int)po, o);
      if (lane < 8) P.span_scal[(size_t)span_id * 8 + lane] = lane == 5 ? (uint32_t)SPANF_UNSORTED : lane == 6 ? po : 0u;
      return;
    }
  }
  int lo, hi;
  slice_range(tr, B.a, B.b, lo, hi);
  Slice S;
  S.m = (hi - lo) <= K1_SLICE ? (hi - lo) : 0;   // an oversize slice is handled round by round
  stage_slice(lds, tr, lo, S, lane);
  __syncthreads();

  int tile = sp.tile0;
  for (;;) {
    const bool has_next_tile = te < sp_end;
    const int ntb = tb + K1_TILE;
    const int nte = (ntb + K1_TILE < sp_end) ? ntb + K1_TILE : sp_end;
    const bool oversize = (hi - lo) > K1_SLICE;
    const bool started_before = (tb > 0) && (B.prevp == B.a);
    const int own_a = started_before ? B.a : INT32_MIN;
    const bool owns_b = !(started_before && B.a == B.b);
    const int npairs = (te - tb + PAIR - 1) / PAIR;
    const int mtile = 32 * ((tile - sp.tile0) % MASK_TILES);

    SegBounds NB = B;
    int nlo = 0, nhi = 0;
    constexpr int NSL = K1_SLICE / 64;   // registers per lane that hold the next tile's slice
    uint32_t nkeys[NSL];
#pragma unroll
    for (int q = 0; q < NSL; ++q) nkeys[q] = 0u;
    int prev_last = B.prevp;
    if (has_next_tile) NB = seg_bounds(C, ntb, nte, vn);
    for (int pr = 0; pr < npairs; ++pr) {
      const int pbase = tb + pr * PAIR;
      const int hbase = pbase + 256;                           // the second half's first record
      const int pend = pbase + PAIR < te ? pbase + PAIR : te;
      const bool two = hbase < te;                             // the second half holds records (wave-uniform)
      // wave-uniform; a tile that starts inside a run of one position (own_a set) stays on the general path, which knows own_a
      const bool plain = QM_PAIR_PLAIN && !oversize && !started_before && pbase + PAIR <= te && plain_pair(N0, N1, prev_last, lane);
      In4 X0, X1;
      if (plain) {
        unpack_raw<true>(N0, nbm1f, X0, lds + L_FLUT);
        unpack_raw<true>(N1, nbm1f, X1, lds + L_FLUT);
      } else {
        unpack_raw<false>(N0, nbm1f, X0, lds + L_FLUT);
        unpack_raw<false>(N1, nbm1f, X1, lds + L_FLUT);        // (a half behind the tile's end: staged as padding, never classified)
      }
      // the next tile's slice is fetched as a side chain spread over this tile's pairs, so none of its three dependent
      // global round trips (bounds -> position index -> keys) is exposed: bounds in front of the loop, the index behind the first
      // pair's join, the keys here in the second pair
      if (has_next_tile && pr != 0) {
        const int nm = (nhi - nlo) <= K1_SLICE ? (nhi - nlo) : 0;
#pragma unroll
        for (int q = 0; q < NSL; ++q) nkeys[q] = q * 64 + lane < nm ? tr.keys[nlo + q * 64 + lane] : 0u;
      }
      // then the following pair's records into flight, round by round (rounds are contiguous across the span's tiles) -- behind
      // the unpack, not hoisted over it: the loads then land in the registers the unpack has just read, and the loop carries
      // no register copies for the double buffer (18 v_mov per pair otherwise)
      __builtin_amdgcn_sched_barrier(0);
      if (pbase + PAIR < sp_end) load_raw(C, pbase + PAIR + lane * 4, N0);
      if (hbase + PAIR < sp_end) load_raw(C, hbase + PAIR + lane * 4, N1);
      stage_half(lds, X0, 0, pbase + lane * 4, te, lane);
      stage_half(lds, X1, 1, hbase + lane * 4, te, lane);
      if (lane < PAIR / 32) lds[L_HITS + lane] = 0;
      __syncthreads();
      if (plain) {
        join_staged<PAIR, true>(lds, S, 0, PAIR, INT32_MIN, lane);
      } else if (!oversize) {
        join_staged<PAIR, false>(lds, S, 0, pend - pbase, own_a, lane);
      } else {
        oversize_round(lds, C, tr, X0, S, 0, pbase, two ? hbase : pend, vn, nb, A, acc_tpr, lane);
        if (two) oversize_round(lds, C, tr, X1, S, 256, hbase, pend, vn, nb, A, acc_tpr, lane);
      }
      if (has_next_tile && pr == 0) slice_range(tr, NB.a, NB.b, nlo, nhi);
      __syncthreads();
      if (plain) {   // both halves hold records; no predecessor is looked at
        classify_half<true>(lds, C, X0, L_HITS, pbase, 0, nb, mtile + 16 * pr, A, lane);
        classify_half<true>(lds, C, X1, L_HITS + 8, hbase, 0, nb, mtile + 16 * pr + 8, A, lane);
      } else {
        classify_half<false>(lds, C, X0, L_HITS, pbase, prev_last, nb, mtile + 16 * pr, A, lane);
        if (two) classify_half<false>(lds, C, X1, L_HITS + 8, hbase, (int)(lds[rk(255)] >> 4), nb, mtile + 16 * pr + 8, A, lane);
      }
      prev_last = (int)(lds[rk(PAIR - 1)] >> 4);
      __syncthreads();
    }

    // ---- tile epilogue: run continuation, per-truth-entry state -> histogram, counts ----
    if (!oversize) {
      if (B.nextp == B.b && owns_b) continue_run(C, lds, S, te, vn, B.b, nb, lane);
      __syncthreads();
      acc_tpr += flush_slice(lds, S, lane);
    }
    {
      const uint32_t tile_np = wave_sum(A.n_pass), tile_nt = wave_sum(A.n_tp);
      A.n_pass = 0; A.n_tp = 0;
      if (lane == 0) {   // the tile counts wait for the end of the span
        lds[L_TCNT + (tile - sp.tile0)] = tile_nt;
        lds[L_TCNT + SPAN_TILES + (tile - sp.tile0)] = tile_np - tile_nt;
      }
      acc_pass += tile_np;
      acc_tp += tile_nt;
    }
    const bool stop_unsorted = ballot64(A.bad & 1u) != 0ull;
    {
      // a full batch of mask words, or the span's last tiles: one 16-byte store per lane and mask (dword stores for a ragged end)
      constexpr int MT = MASK_TILES;
      const int tin = (tile - sp.tile0) % MT;
      if (tin == MT - 1 || !has_next_tile || stop_unsorted) {
        __syncthreads();
        const int b0 = tb - tin * K1_TILE;                    // first record of the batch (VCF-relative)
        const int nd = ((te - b0 + 255) >> 8) * 8;            // dwords of the ROUNDS that ran (every VCF owns its masks up to a multiple of 256 records); the rest of the LDS batch is stale
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          uint32_t* dst = (half ? mtp32 : mpass32) + (b0 >> 5);
          const int src = L_MASK + half * 32 * MT;
          for (int w = 4 * lane; w < 32 * MT; w += 256) {
            if (w + 3 < nd) {
              typedef unsigned v4u_ __attribute__((ext_vector_type(4)));
              __builtin_nontemporal_store(*reinterpret_cast<const v4u_*>(&lds[src + w]), reinterpret_cast<v4u_*>(dst + w));
            }
            else for (int k = 0; k < 4; ++k) if (w + k < nd) dst[w + k] = lds[src + w + k];
          }
        }
      }
    }

    if (!has_next_tile) break;
    if (stop_unsorted) break;   // the VCF is redone through the sort and nothing computed here is used: stop streaming it
    // ---- the next tile's slice leaves its registers (a full tile has two pairs: the side chain has run to its end) ----
    B = NB;
    tb = ntb;
    te = nte;
    ++tile;
    lo = nlo;
    hi = nhi;
    S.m = (hi - lo) <= K1_SLICE ? (hi - lo) : 0;
#pragma unroll
    for (int q = 0; q < NSL; ++q) {
      const int j = q * 64 + lane;
      if (j < S.m) { lds[L_KEYS + j] = nkeys[q]; lds[L_SMAX + j] = 0; }
    }
    if (lane < K1_SLICE / 32) lds[L_SRF + lane] = 0;
    __syncthreads();
  }

  // ---- span epilogue -------------------------------------------------------------------
  acc_tpr = wave_sum(acc_tpr);
  A.fpr = wave_sum(A.fpr);
  const uint64_t any_uns = ballot64(A.bad & 1u);
  const uint64_t any_bad = ballot64(A.bad & 2u);
  __syncthreads();
  const uint32_t top_tp = A.top_tp, top_fp = A.top_fp;
  uint32_t* oh = P.span_hist + (size_t)span_id * SPAN_HIST_WORDS;
  for (int i = lane; i < 128; i += 64) {
    const int b0 = 2 * i, b1 = 2 * i + 1;
    oh[i] = (hist_get(lds, L_HTP, 1 + b0) + (b0 == nb - 1 ? top_tp : 0u)) | ((hist_get(lds, L_HTP, 1 + b1) + (b1 == nb - 1 ? top_tp : 0u)) << 16);
    oh[128 + i] = (hist_get(lds, L_HFP, 1 + b0) + (b0 == nb - 1 ? top_fp : 0u)) | ((hist_get(lds, L_HFP, 1 + b1) + (b1 == nb - 1 ? top_fp : 0u)) << 16);
    oh[256 + i] = hist_get(lds, L_HU, b0) | (hist_get(lds, L_HU, b1) << 16);
  }
  {   // the span's tile counts: lanes 0..15 TP, 16..31 FP
    const int nt_span = (sp_end - (int)(sp.begin - sp.voff) + K1_TILE - 1) / K1_TILE;
    const int t = lane & (SPAN_TILES - 1);
    if (lane < 2 * SPAN_TILES && t < nt_span) (lane < SPAN_TILES ? P.tile_tp : P.tile_fp)[sp.tile0 + t] = lds[L_TCNT + lane];
  }
  if (lane == 0) {
    uint32_t* sc = P.span_scal + (size_t)span_id * 8;
    sc[0] = acc_pass; sc[1] = acc_tp; sc[2] = acc_pass - acc_tp; sc[3] = acc_tpr; sc[4] = A.fpr;
    sc[5] = (any_uns ? SPANF_UNSORTED : 0u) | (any_bad ? SPANF_BADPOS : 0u);
    sc[7] = 0;
  }
  {
    uint32_t po = A.posor;   // OR over the wave (once per span)
    for (int o = 32; o > 0; o >>= 1) po |= (uint32_t)__shfl_xor((int)po, o);
    if (lane == 0) P.span_scal[(size_t)span_id * 8 + 6] = po;
  }
}

}  // namespace cpair

void launch_classify_pair(const ClassifyParams& P, int n_spans, hipStream_t st) {   // spans P.span_base .. + n_spans
  if (n_spans <= 0) return;
  hipLaunchKernelGGL(cpair::k_classify_pair, dim3(n_spans), dim3(64), 0, st, P);
}

}  // namespace qm
