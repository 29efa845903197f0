// crp_lines.hpp — the lines of the split CRP's selects (crp_split.hip, its only includer): one
// wave holds one line (CRP row or column) of 16-bit key prefixes in registers and answers the
// threshold search's queries on it by SWAR arithmetic (packed lane fields inside 32-bit words).
//
//  Codes<NP, WIN>  a lane's 2 NP packed codes, the optional 7-bit window codes around a hint, and
//                  every word-level query on them, once.
//  Line<32>        lines up to 2,048 codes, 32 consecutive elements per lane.
//  LineS<8|16>     lines up to 512 / 1,024 codes, lane-strided.
//  Line2           lines up to 4,096 codes: two Line<32> halves.
// The three layouts add only where an element lives (lane, mask bit), how it is loaded and, for
// LineS, which of the core's flag bits are elements. What the selects see of a line: count_le,
// eq_mask, le_mask, min_max, min_greater, hist_rank, build_window, sample, ebase, elem, lane_of,
// bit_of, kHalves, kHist.
//
// Lane l holds its elements as packed words: one element in bits 0..15, another in bits 16..31.
// Real prefixes are <= 0x7f80 (keys are >= +0, the sign bit is 0), so 0x7fff marks "no element"
// and every field keeps a free guard bit for SWAR arithmetic.
#pragma once
#include "common.hpp"

// v_writelane_b32 through the LLVM intrinsic (hipcc has no builtin for it), so the compiler's
// hazard recognizer inserts the wait state between the ballot's SGPR write and the writelane
// (the inline-asm form of round 3 lacked it and produced wrong words)
__device__ int acoss_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

namespace acoss {

// 16-bit prefix of "no element": above every real prefix (finite keys >= +0 have prefixes <= 0x7f80)
constexpr unsigned kNone = 0x7fffu;

__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned pk_max_u16(unsigned a, unsigned b) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned pk_add_u16(unsigned a, unsigned b) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ unsigned pk_subsat_u16(unsigned a, unsigned b) {
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// Bits h and h + 16 of the result take the per-field flags (bits 15 and 31) of SWAR word h: the
// flag bits of a SWAR compare on word h become two mask bits with one shift and one and-or, so an
// element mask costs 3 VALU per word.
__device__ __forceinline__ uint32_t gather_flags(uint32_t acc, uint32_t s, int h) {
  return ((s >> (15 - h)) & (0x00010001u << h)) | acc;
}
// Bits h, h + 8, h + 16, h + 24 of the result take the flags (bits 7, 15, 23, 31) of word h.
__device__ __forceinline__ uint32_t gather_flags8(uint32_t acc, uint32_t s, int h) {
  return ((s >> (7 - h)) & (0x01010101u << h)) | acc;
}

// Smallest prefix > x (x < kNone) among a lane's packed words, or 0xffffffff: per field
// (k - x - 1) mod 2^16 (one wrapping packed add) puts every real k > x at k - x - 1 <= 0x7f80 - x - 1,
// kNone at 0x7fff - x - 1 and every k <= x at >= 0x10000 - x - 1, so a packed minimum and one
// compare find it (2 VALU per word; the per-element compare/select form took ~7 per element).
template <int NW>
__device__ __forceinline__ unsigned swar_min_greater(const unsigned (&pv)[NW], unsigned x) {
  const unsigned X = ((0x10000u - x - 1u) & 0xffffu) * 0x10001u;
  unsigned a = 0xffffffffu;
#pragma unroll
  for (int h = 0; h < NW; ++h) a = pk_min_u16(a, pk_add_u16(pv[h], X));
  const unsigned d = min(a & 0xffffu, a >> 16);
  return d < kNone - x - 1u ? d + x + 1u : 0xffffffffu;
}

// Unconditional histogram adds: an element outside the bins goes to this lane's own sink word
// (the 64 words after the 128 bins, WaveLds::sink; a lane-private address, no bank conflict), so
// every element issues the same ds_add instead of a compare, an exec-mask save / restore and a
// masked add. Used by the window-code histogram (hist_fill_w8); the 16-bit-prefix histogram keeps
// the masked add (hist_add below), where the sink measured 6 % slower at 500 frames.
typedef __attribute__((address_space(3))) unsigned lds_u32;
// 32-bit LDS addresses of a wave's histogram: the bins' base as an SGPR (bin address = c * 4 +
// base in one v_lshl_add) and this lane's sink word
struct HistAddr {
  unsigned hb, sk;
  __device__ __forceinline__ explicit HistAddr(unsigned* hist) {
    hb = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(lds_u32*)hist);
    sk = hb + 512u + 4u * (threadIdx.x & 63);
  }
};
__device__ __forceinline__ void hist_add(unsigned* hist, const HistAddr& A, unsigned c, bool in) {
  if (in) __hip_atomic_fetch_add(hist + c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void hist_clear(unsigned* hist) {
  reinterpret_cast<uint2*>(hist)[threadIdx.x & 63] = make_uint2(0u, 0u);
  __builtin_amdgcn_wave_barrier();
}

// The shared tail of the two histogram searches: the wave's 128 bins (bin c <-> prefix base + c,
// two per lane) are filled, below_tot elements lie under them; one wave scan places rank rho.
// False, deciding nothing, when the answer is outside the bins (wave-uniform), or in bin 0 when
// that bin is not one exact prefix. le / less: count(<= P) / count(< P), as prefix_of_rank.
__device__ __forceinline__ bool hist_place(const unsigned* hist, int rho, unsigned base, int below_tot, bool bin0_exact,
                                           unsigned* P, int* le, int* less) {
  __builtin_amdgcn_wave_barrier();
  const uint2 hv = reinterpret_cast<const uint2*>(hist)[threadIdx.x & 63];
  const int sl = (int)(hv.x + hv.y);
  const int S = wave_incl_scan(sl);
  const int tot = __builtin_amdgcn_readlane(S, 63);
  const int r = rho - below_tot;
  if (r < 0 || r >= tot) return false;
  const int E = S - sl;
  const int src = __builtin_ctzll(__ballot(E <= r && r < S));
  const int Es = __builtin_amdgcn_readlane(E, src);
  const int h0 = __builtin_amdgcn_readlane((int)hv.x, src), h1 = __builtin_amdgcn_readlane((int)hv.y, src);
  const bool second = r >= Es + h0;
  if (!bin0_exact && src == 0 && !second) return false;
  *P = base + 2u * (unsigned)src + (second ? 1u : 0u);
  *less = below_tot + Es + (second ? h0 : 0);
  *le = *less + (second ? h1 : h0);
  return true;
}

// A line's 7-bit window codes (w8: four codes per word; window base8 = hint - 63, code c <->
// prefix base8 + c exactly for c in 1..126, and for c = 0 too when base8 = 0; code 0 otherwise
// means "at or below base8", 127 "at or above base8 + 127") into the wave's bins: every code
// below 127 is counted into its LDS bin straight from its byte, code 0 included (bin 0 then holds
// the elements at or below base8, exact only when base8 == 0), so no separate count of the
// elements under the window; code 127 to this lane's sink; no exec masking.
// The sink select is done on a whole word at once (SWAR): byte k of wp = code + 1 (1..128, no
// carry between bytes); the bytes at 128 (code 127) get lane + 1 more, to 129 + lane; then bin
// index b - 1 for every byte b, so the sink of lane l is index 128 + l (A.sk). Per code one byte
// extract and one address, per word six ops (a per-code compare, hazard nop and select measured
// 0.8 % slower end to end).
template <int NW>
__device__ __forceinline__ void hist_fill_w8(const unsigned (&w8)[NW], unsigned* hist) {
  hist_clear(hist);
  const HistAddr A(hist);
  const unsigned lane1 = (unsigned)((threadIdx.x & 63) + 1) * 0x01010101u;  // lane + 1 (<= 64) in every byte
  const unsigned hbm = A.hb - 4u;
#pragma unroll
  for (int h = 0; h < NW; ++h) {
    const unsigned wp = w8[h] + 0x01010101u;
    const unsigned H = wp & 0x80808080u;
    const unsigned S = wp + ((H - (H >> 7)) & lane1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned a = hbm + 4u * ((S >> (8 * k)) & 0xffu);
      __hip_atomic_fetch_add((lds_u32*)(size_t)a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
  }
}

// A lane's 2 NP codes as NP packed words pv (which elements they are is the layout's business),
// and every query that is arithmetic on those words. The per-lane pieces (cnt*, eq*, le*,
// *_lane) are branch-free and return raw values: flags of word h's two fields on bits h and
// h + 16 (16-bit words) or of its four bytes on bits h + 8 k (window codes).
// WIN: an optional 7-bit window around a hint: w8 holds min(max(prefix - base8, 0), 127) for the
// lane's codes, four per word (byte k of word h = the code of pv[h + (k & 1) NP/2]'s field k >> 1).
// For thresholds in [base8, base8 + 126] it answers count / member / le queries exactly at half
// the VALU of the 16-bit words (codes 0 and 127 are the saturated "below" and "above" classes).
template <int NP, bool WIN>
struct Codes {
  unsigned pv[NP];
  unsigned w8[WIN ? NP / 2 : 1];
  unsigned base8;
  bool win;
  // a freshly loaded line has no window
  __device__ __forceinline__ void no_window() {
    if constexpr (WIN) {
      win = false;
      base8 = 0u;
    }
  }
  __device__ __forceinline__ void build_window(unsigned center) {
    static_assert(WIN, "window codes: 16 or 32 codes per lane only");
    base8 = center > 63u ? center - 63u : 0u;
    win = true;
    const unsigned B2 = base8 * 0x10001u;
    unsigned c[NP];
#pragma unroll
    for (int h = 0; h < NP; ++h) c[h] = pk_min_u16(pk_subsat_u16(pv[h], B2), 0x007f007fu);
#pragma unroll
    for (int h = 0; h < NP / 2; ++h) w8[h] = __builtin_amdgcn_perm(c[h + NP / 2], c[h], 0x06020400u);
  }
  // wave-uniform: the window codes answer a count / le query at x, a member query at P
  __device__ __forceinline__ bool in_win(unsigned x) const { return win && x >= base8 && x <= base8 + 126u; }
  __device__ __forceinline__ bool eq_in_win(unsigned P) const {
    return in_win(P) && (P > base8 || base8 == 0u);  // code 0 is exact only when base8 == 0
  }
  // #elements <= x (x <= 0x7fff): per field (x + 0x8000) - a keeps bit 15 iff a <= x, with no
  // borrow across fields; popcount on VALU, one DPP wave sum (no SGPR per compare, no SALU).
  __device__ __forceinline__ unsigned cnt8(unsigned x) const {
    const unsigned X4 = (x - base8 + 0x80u) * 0x01010101u;
    unsigned c = 0;
#pragma unroll
    for (int h = 0; h < NP / 2; ++h) c = __builtin_popcount((X4 - w8[h]) & 0x80808080u) + c;
    return c;
  }
  __device__ __forceinline__ unsigned cnt16(unsigned x) const {
    const unsigned X2 = (x + 0x8000u) * 0x10001u;
    unsigned c = 0;
#pragma unroll
    for (int h = 0; h < NP; ++h) c = __builtin_popcount((X2 - pv[h]) & 0x80008000u) + c;
    return c;
  }
  __device__ __forceinline__ int count_le(unsigned x) const {
    if constexpr (WIN) {
      if (in_win(x)) return wave_sum((int)cnt8(x));
    }
    return wave_sum((int)cnt16(x));
  }
  // Flag set iff the element's prefix == P (P <= kCodeMax). Per field, (a ^ P) + 0x7fff keeps bit
  // 15 iff a != P; fields are <= 0x7fff, so nothing carries across.
  __device__ __forceinline__ uint32_t eq8(unsigned P) const {
    const unsigned PP = (P - base8) * 0x01010101u;
    uint32_t ne8 = 0;
#pragma unroll
    for (int h = 0; h < NP / 2; ++h) ne8 = gather_flags8(ne8, (w8[h] ^ PP) + 0x7f7f7f7fu, h);
    return ~ne8;
  }
  __device__ __forceinline__ uint32_t eq16(unsigned P) const {
    const unsigned PP = P * 0x10001u;
    uint32_t ne = 0;
#pragma unroll
    for (int h = 0; h < NP; ++h) ne = gather_flags(ne, (pv[h] ^ PP) + 0x7fff7fffu, h);
    return ~ne;
  }
  // Flag set iff the element's prefix <= x (x <= 0x7fff; kNone is never <= a real x).
  __device__ __forceinline__ uint32_t le8(unsigned x) const {
    const unsigned X4 = (x - base8 + 0x80u) * 0x01010101u;
    uint32_t le8 = 0;
#pragma unroll
    for (int h = 0; h < NP / 2; ++h) le8 = gather_flags8(le8, X4 - w8[h], h);
    return le8;
  }
  __device__ __forceinline__ uint32_t le16(unsigned x) const {
    const unsigned X2 = (x + 0x8000u) * 0x10001u;
    uint32_t le = 0;
#pragma unroll
    for (int h = 0; h < NP; ++h) le = gather_flags(le, X2 - pv[h], h);
    return le;
  }
  // min over elements (kNone is above every real prefix) and max over real elements
  // (kNone + 1 wraps to 0x8000, masked to 0: below every real prefix + 1); lane shares first
  __device__ __forceinline__ void min_max_lane(unsigned* a_io, unsigned* b_io) const {
    unsigned a = *a_io, b = *b_io;
#pragma unroll
    for (int h = 0; h < NP; ++h) {
      a = pk_min_u16(a, pv[h]);
      b = pk_max_u16(b, pk_add_u16(pv[h], 0x00010001u) & 0x7fff7fffu);
    }
    *a_io = a;
    *b_io = b;
  }
  // the wave's finish of min_max_lane's packed pair (a, b)
  static __device__ __forceinline__ void min_max_wave(unsigned a, unsigned b, unsigned* mn, unsigned* mx) {
    a = min(a & 0xffffu, a >> 16);
    b = max(b & 0xffffu, b >> 16);
    *mn = wave_min_u32(a);
    const unsigned m = wave_max_u32(b);
    *mx = m ? m - 1 : 0u;
  }
  __device__ __forceinline__ void min_max(unsigned* mn, unsigned* mx) const {
    unsigned a = 0xffffffffu, b = 0u;
    min_max_lane(&a, &b);
    min_max_wave(a, b, mn, mx);
  }
  __device__ __forceinline__ unsigned min_greater_lane(unsigned x) const { return swar_min_greater(pv, x); }
  __device__ __forceinline__ unsigned min_greater(unsigned x) const { return wave_min_u32(min_greater_lane(x)); }
  // Prefix of rank rho (0-based: the least P with count(<= P) > rho) from ONE pass over the line:
  // every element inside the 128-prefix window [base, base + 128) around the hint (the previous
  // line's answer; adjacent lines share 8 of their 9 stacked frames, so the answer lies inside
  // the window for about 99 % of the lines) is counted into its LDS bin, the elements below the
  // window by one SWAR count; one wave scan of the bins then places rank rho. Two wave reductions
  // instead of the search's ~5 dependent count passes. Returns false, deciding nothing, when the
  // answer lies outside the window. *hbase: the bins' base, for hist_next.
  // Invariant: a windowed line's hist_rank runs only after build_window. line_plan calls it only
  // with a hint, and rows_body / cols_body build the window of every windowed line that has one
  // (the hint that the plan sees is never kNoHint: sample_hint supplies the first). So a windowed
  // line bins its window codes, whose base is the same hint's, and only the unwindowed LineS<8>
  // bins 16-bit prefixes.
  static constexpr bool kHist = true;
  __device__ __forceinline__ bool hist_rank(unsigned hint, int rho, unsigned* hist, unsigned* P, int* le,
                                            int* less, unsigned* hbase) const {
    if constexpr (WIN) {
      *hbase = base8;
      // code 0 is exact only when base8 == 0: a rank landing in bin 0 otherwise decides nothing
      const bool exact0 = base8 == 0u;
      hist_fill_w8(w8, hist);
      return hist_place(hist, rho, base8, 0, exact0, P, le, less);
    } else {
      const unsigned base = hint > 64u ? hint - 64u : 0u;
      *hbase = base;
      hist_clear(hist);
      const HistAddr HA(hist);
      // elements below the window (kNone never is): #(prefix <= base - 1)
      const unsigned below = base > 0u ? cnt16(base - 1u) : 0u;
#pragma unroll
      for (int h = 0; h < NP; ++h) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          // (wraps for p < base; kNone, 0x7fff, is never inside: base <= 0x7f80 - 64)
          const unsigned c = (half ? (pv[h] >> 16) : (pv[h] & 0xffffu)) - base;
          hist_add(hist, HA, c, c < 128u);
        }
      }
      return hist_place(hist, rho, base, wave_sum((int)below), true, P, le, less);
    }
  }
};

// Lane l holds its KPL = 32 elements (element q = line element 32 l + q) as 16 packed words in
// SPLIT order: word h = element h (bits 0..15) and element h + 16 (bits 16..31), so the core's
// flag bits are the elements' own numbers, from the 16-bit words (bits h, h + 16) and from the
// window codes (word h = elements h, h + 8, h + 16, h + 24) alike.
template <int KPL>
struct Line : Codes<KPL / 2, true> {
  static_assert(KPL == 32, "split word order assumes 32 elements per lane");
  static constexpr int kHalves = 1;
  // element of mask bit b: lane * KPL + b (ebase() opaque, so element indices are not hoisted
  // out of callers' loops)
  __device__ __forceinline__ int ebase() const {
    int e = (threadIdx.x & 63) * KPL;
    asm volatile("" : "+v"(e));
    return e;
  }
  __device__ __forceinline__ int elem(int eb, int b) const { return eb + b; }
  static __device__ __forceinline__ int lane_of(int e) { return e / KPL; }
  static __device__ __forceinline__ int bit_of(int e) { return e % KPL; }
  // sample for sample_hint: element KPL * lane (kNone past the line)
  __device__ __forceinline__ unsigned sample() const { return this->pv[0] & 0xffffu; }
  // Lane l's KPL elements start at col0 + l * lane_stride. STORED_SPLIT: the plane holds every
  // run in split order already (the strip-major column plane, written so by the sweep);
  // otherwise (row-major plane, natural order) the loaded pairs are repacked, one v_perm per word.
  template <bool STORED_SPLIT>
  __device__ __forceinline__ void load_lanes(const uint16_t* col0, size_t lane_stride, int n) {
    const int lane = threadIdx.x & 63;
    const int base = lane * KPL;
    // every lane loads a whole run: the lane holding the end of the line reads its run in full
    // (runs lie inside the plane: the row pitch and the strips are whole runs) and masks the
    // tail; lanes past the line re-read lane 0's run and mask all of it. No per-element
    // conditional loads: hipcc branches around each and waits vmcnt(0) after each (16-32
    // serial L2 round trips per line)
    // (lanes past the line reading a constant run of kNone instead of the fill below: -1 % at
    // 2,000 frames, profiles/r04/ab_q2000.txt)
    const uint16_t* src = col0 + (base < n ? (size_t)lane * lane_stride : (size_t)0);
    this->no_window();
    unsigned w[KPL / 2];
#pragma unroll
    for (int q = 0; q < KPL / 8; ++q) {
      const uint4 v = reinterpret_cast<const uint4*>(src)[q];
      w[4 * q + 0] = v.x;
      w[4 * q + 1] = v.y;
      w[4 * q + 2] = v.z;
      w[4 * q + 3] = v.w;
    }
    if (STORED_SPLIT) {
#pragma unroll
      for (int h = 0; h < KPL / 2; ++h) this->pv[h] = w[h];
    } else {
#pragma unroll
      for (int h = 0; h < KPL / 2; ++h)  // (element h, element h + 16) from natural pairs
        this->pv[h] = __builtin_amdgcn_perm(w[8 + (h >> 1)], w[h >> 1], (h & 1) ? 0x07060302u : 0x05040100u);
    }
    // the planes hold kNone past the line's end inside the last run (the sweep stores it), so
    // only lanes wholly past the line need filling
    if (base >= n) {
#pragma unroll
      for (int h = 0; h < KPL / 2; ++h) this->pv[h] = kNone * 0x10001u;
    }
  }
  // one wave-uniform branch over the core's pieces, as Line2 and LineS
  __device__ __forceinline__ uint32_t eq_mask(unsigned P) const {
    if (this->eq_in_win(P)) return this->eq8(P);
    return this->eq16(P);
  }
  __device__ __forceinline__ uint32_t le_mask(unsigned x) const {
    if (this->in_win(x)) return this->le8(x);
    return this->le16(x);
  }
};

// Short lines (up to 64 KQ elements): lane l holds elements l + 64 q, q < KQ,
// so a wave-wide ballot of one mask bit is two consecutive 32-element words of the line (the
// CRP's row and strip words) and every load is coalesced across the wave. KQ/2 packed words:
// word h = element q = h (bits 0..15) and q = h + KQ/2 (bits 16..31); mask bit h <-> q = h and
// bit h + 16 <-> q = h + KQ/2, the same flag gather as the long lines' split order. KQ = 16
// adds the long lines' 7-bit window codes (4 words: word h = elements q = h + 4k, k = 0..3, one
// per byte; its flag gather puts q = h + 4k on bit h + 8k, which wmask moves to the 16-bit
// layout's bits); KQ = 8 searches its 4 words directly.
template <int KQ>
struct LineS : Codes<KQ / 2, KQ == 16> {
  static_assert(KQ == 8 || KQ == 16, "short lines: 8 or 16 elements per lane");
  static constexpr bool kWin = KQ == 16;
  static constexpr int kHalves = 1;
  static constexpr uint32_t kMaskAll = ((1u << (KQ / 2)) - 1u) * 0x10001u;
  static constexpr uint32_t kWinLo = ((1u << (KQ / 4)) - 1u) * 0x10001u;
  static __device__ __forceinline__ uint32_t wmask(uint32_t m) {
    return (m & kWinLo) | ((m >> (8 - KQ / 4)) & (kWinLo << (KQ / 4)));
  }
  static __device__ __forceinline__ int q_of_bit(int b) { return b < 16 ? b : b - 16 + KQ / 2; }
  static __device__ __forceinline__ int bit_of_q(int q) { return q < KQ / 2 ? q : q - KQ / 2 + 16; }
  __device__ __forceinline__ int ebase() const {
    int e = threadIdx.x & 63;
    asm volatile("" : "+v"(e));
    return e;
  }
  __device__ __forceinline__ int elem(int eb, int b) const { return eb + 64 * q_of_bit(b); }
  static __device__ __forceinline__ int lane_of(int e) { return e & 63; }
  static __device__ __forceinline__ int bit_of(int e) { return bit_of_q(e >> 6); }
  // sample for sample_hint: element l + 64 (l mod KQ), spread over the line
  __device__ __forceinline__ unsigned sample() const {
    // a mux tree on the lane bits (an index compare chain becomes a scratch-array lookup)
    const int lane = threadIdx.x & 63;
    unsigned t[KQ / 2];
#pragma unroll
    for (int k = 0; k < KQ / 2; ++k) t[k] = this->pv[k];
#pragma unroll
    for (int bit = 1, n = KQ / 2; n > 1; bit <<= 1, n >>= 1) {
      const bool sel = (lane & bit) != 0;
#pragma unroll
      for (int k = 0; k < n / 2; ++k) t[k] = sel ? t[2 * k + 1] : t[2 * k];
    }
    return (lane & (KQ / 2)) ? (t[0] >> 16) : (t[0] & 0xffffu);
  }
  // the n codes of a line; addr(e): where element e's code is. Every lane loads (elements past
  // the line re-read element n - 1 and are replaced by kNone): no per-element branches.
  // FRESH: the lane's element offsets are computed here, not shared with the caller's other loads
  // (a rare reload then keeps none of them in registers meanwhile).
  template <bool FRESH = false, class AT>
  __device__ __forceinline__ void load(AT addr, int n) {
    int lane = threadIdx.x & 63;
    if (FRESH) asm volatile("" : "+v"(lane));
    this->no_window();
    unsigned v[KQ];
#pragma unroll
    for (int q = 0; q < KQ; ++q) v[q] = *addr(min(lane + 64 * q, n - 1));
#pragma unroll
    for (int q = 0; q < KQ; ++q) v[q] = lane + 64 * q < n ? v[q] : kNone;
#pragma unroll
    for (int h = 0; h < KQ / 2; ++h) this->pv[h] = v[h] | (v[h + KQ / 2] << 16);
  }
  // the core's raw flags, cut to this layout's elements (le16 needs no cut: kNone is never <= x)
  __device__ __forceinline__ uint32_t eq_mask(unsigned P) const {
    if constexpr (kWin) {
      // eq_in_win's condition, spelled out: through the call k_sweep_rows9<16> takes two more
      // SGPR spills (85 for 83, profiles/crp_lines/codegen.md)
      if (this->in_win(P) && (P > this->base8 || this->base8 == 0u)) return wmask(this->eq8(P));
    }
    return this->eq16(P) & kMaskAll;
  }
  __device__ __forceinline__ uint32_t le_mask(unsigned x) const {
    if constexpr (kWin) {
      if (this->in_win(x)) return wmask(this->le8(x));
    }
    return this->le16(x);
  }
};

// Lane t's 32-bit line word t (elements 32 t .. 32 t + 31) from a short line's per-lane mask:
// word 2q + half is the low / high half of the ballot of bit q. Lanes past 2 KQ get 0.
template <int KQ>
__device__ __forceinline__ uint32_t lane_words(uint32_t mask) {
  // each ballot half is wave-uniform (an SGPR): one v_writelane_b32 places it on its lane
  uint32_t out = 0;
#pragma unroll
  for (int q = 0; q < KQ; ++q) {
    const unsigned long long bal = __ballot((mask >> LineS<KQ>::bit_of_q(q)) & 1u);
    out = (uint32_t)acoss_writelane((int)(uint32_t)bal, 2 * q, (int)out);
    out = (uint32_t)acoss_writelane((int)(uint32_t)(bal >> 32), 2 * q + 1, (int)out);
  }
  return out;
}

// Lines of 2049..4096 codes: two long-line halves held by one wave, elements [0, 2048) in A
// and [2048, n) in B (lane l: elements 32 l.. and 2048 + 32 l..). One wave sum per count; masks
// are 64-bit (A in bits 0..31, B in 32..63); the le words of B live in W.words[64 + lane].
struct Line2 {
  Line<32> A, B;
  static constexpr int kHalves = 2;
  static constexpr bool kHist = false;
  __device__ __forceinline__ int ebase() const { return A.ebase(); }
  __device__ __forceinline__ int elem(int eb, int b) const { return b < 32 ? eb + b : 2048 + eb + (b - 32); }
  static __device__ __forceinline__ int lane_of(int e) { return e < 2048 ? (e >> 5) : 64 + ((e - 2048) >> 5); }
  static __device__ __forceinline__ int bit_of(int e) { return e & 31; }
  // sample: even lanes from A (element 32 l), odd lanes from B (element 2048 + 32 l)
  __device__ __forceinline__ unsigned sample() const {
    const unsigned a = A.sample(), b = B.sample();  // (selecting the half object would keep both in scratch)
    return (threadIdx.x & 1) ? b : a;
  }
  __device__ __forceinline__ void build_window(unsigned c) {
    A.build_window(c);
    B.build_window(c);
  }
  // (both halves share the window, so one wave-uniform branch serves both: branching per half
  // lets the compiler merge the two halves' paths into pointer phis, which keeps the line in scratch)
  __device__ __forceinline__ int count_le(unsigned x) const {
    if (A.in_win(x)) return wave_sum((int)(A.cnt8(x) + B.cnt8(x)));
    return wave_sum((int)(A.cnt16(x) + B.cnt16(x)));
  }
  __device__ __forceinline__ uint64_t eq_mask(unsigned P) const {
    if (A.eq_in_win(P)) return (uint64_t)A.eq8(P) | ((uint64_t)B.eq8(P) << 32);
    return (uint64_t)A.eq16(P) | ((uint64_t)B.eq16(P) << 32);
  }
  __device__ __forceinline__ uint64_t le_mask(unsigned x) const {
    if (A.in_win(x)) return (uint64_t)A.le8(x) | ((uint64_t)B.le8(x) << 32);
    return (uint64_t)A.le16(x) | ((uint64_t)B.le16(x) << 32);
  }
  __device__ __forceinline__ void min_max(unsigned* mn, unsigned* mx) const {
    unsigned a = 0xffffffffu, b = 0u;
    A.min_max_lane(&a, &b);
    B.min_max_lane(&a, &b);
    Line<32>::min_max_wave(a, b, mn, mx);
  }
  __device__ __forceinline__ unsigned min_greater(unsigned x) const {
    return wave_min_u32(min(A.min_greater_lane(x), B.min_greater_lane(x)));
  }
};

}  // namespace acoss
