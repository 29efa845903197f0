// ef_select.hpp — csm_to_binary's line select, once: the count(kappa, n) least cells of a line
// become 1, ties to the lowest index. The count, the keys and the three selects (knock64,
// wave_line_select, wave_line_select_stream) under every kernel of ef_binarize.hip, rows and columns,
// and k_binarize_rows (misc.hip). A kernel brings its own loads (keys into registers, or a key
// reader) and its own emit (bits into words). The selects take nn >= 1; kappa == 0 (all ones),
// nn <= 0 and a line that keeps everything stay with the callers.
#pragma once
#include "common.hpp"

namespace acoss {

// The count for a line of n: np.round (half to even) of kappa n, or kappa itself from 1 on. The host
// wrappers reject a count >= n as the reference's argpartition does; the clamp is for direct callers.
__host__ __device__ __forceinline__ int ef_count(double kappa, int n) {
  return min(kappa < 1.0 ? (int)rint(kappa * (double)n) : (int)kappa, n);
}

// Keys whose unsigned order is a select's order on values: float32 ascending (fkey_f32, common.hpp:
// -0 before +0), float64 descending for early SNF's largest (-0 counted as +0, as its row kernel).
template <typename T>
struct ColKey;
template <>
struct ColKey<float> {
  typedef unsigned K;
  static constexpr int kBits = 32;
  static __device__ __forceinline__ K key(float f) { return fkey_f32(f); }
};
template <>
struct ColKey<double> {
  typedef unsigned long long K;
  static constexpr int kBits = 64;
  static __device__ __forceinline__ K key(double d) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, d + 0.0);
    return (u >> 63) ? u : ~(u | 0x8000000000000000ull);
  }
};

// Lane-private: the nn least of key[0..n) in (key ascending, index ascending) as a 64-bit mask, by
// nn knock-out rounds (each takes the least key not yet taken, strict <, indices ascending: the
// lowest index among equal keys). n, nn wave-uniform, 1 <= nn <= n <= 64. No LDS, no cross-lane step.
__device__ __forceinline__ unsigned long long knock64(const unsigned (&key)[64], int n, int nn) {
  unsigned long long sel = 0ull;
#pragma unroll 1
  for (int t = 0; t < nn; ++t) {  // wave-uniform; nn <= n, so an untaken index always exists
    unsigned bk = 0xffffffffu;
    int bi = -1;
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      if (i < n) {  // wave-uniform
        const bool better = !((sel >> i) & 1ull) && (bi < 0 || key[i] < bk);
        bk = better ? key[i] : bk;
        bi = better ? i : bi;
      }
    }
    sel |= 1ull << bi;
  }
  return sel;
}

// The nn-th smallest (1-based) of the wave's keys kr (KB per lane) within [lo, hi], by radix
// select: from the highest bit where lo and hi differ, 8-bit digits, each digit from one LDS
// histogram of the candidates (keys matching the digits so far) and one wave scan of its 256
// bins; about 4 passes instead of the ~26 count passes of a bisection over [lo, hi]. Every key
// issues one unconditional ds_add: candidates to their digit's bin, the rest to a lane-private
// sink word (hist: 256 bins + 64 sink words, this wave's own). Same answer as the bisection:
// the least key v with #(keys <= v) >= nn.
template <int KB>
__device__ __forceinline__ unsigned radix_kth(const unsigned (&kr)[KB], unsigned lo, unsigned hi, int nn, int lane,
                                              unsigned* hist) {
  if (lo >= hi) return lo;
  typedef __attribute__((address_space(3))) unsigned lds_u32;
  const unsigned hb = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(size_t)(lds_u32*)hist);
  const unsigned sk = hb + 1024u + 4u * (unsigned)lane;
  int sh = 32 - __builtin_clz(lo ^ hi);  // bits [0, sh) differ inside [lo, hi]
  unsigned prefix = sh >= 32 ? 0u : (lo >> sh) << sh;
  int rank = nn - 1;
  while (sh > 0) {  // wave-uniform
    const int dsh = sh > 8 ? sh - 8 : 0;
    reinterpret_cast<uint4*>(hist)[lane] = make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_wave_barrier();
    const unsigned P = sh >= 32 ? 0u : prefix >> sh;
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      const unsigned k = kr[q];
      const bool cand = sh >= 32 || (k >> sh) == P;
      const unsigned d = (k >> dsh) & 0xffu;
      const unsigned a = cand ? hb + 4u * d : sk;
      __hip_atomic_fetch_add((lds_u32*)(size_t)a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    __builtin_amdgcn_wave_barrier();
    const uint4 hv = reinterpret_cast<const uint4*>(hist)[lane];  // bins 4 lane .. 4 lane + 3
    const int sl = (int)(hv.x + hv.y + hv.z + hv.w);
    const int S = wave_incl_scan(sl);
    const int E = S - sl;
    const int src = __builtin_ctzll(__ballot(E <= rank && rank < S));
    int r = rank - __builtin_amdgcn_readlane(E, src);
    const int h0 = __builtin_amdgcn_readlane((int)hv.x, src), h1 = __builtin_amdgcn_readlane((int)hv.y, src),
              h2 = __builtin_amdgcn_readlane((int)hv.z, src);
    unsigned b = 0;
    if (r >= h0) {
      r -= h0;
      b = 1;
      if (r >= h1) {
        r -= h1;
        b = 2;
        if (r >= h2) {
          r -= h2;
          b = 3;
        }
      }
    }
    prefix |= (4u * (unsigned)src + b) << dsh;
    rank = r;
    sh = dsh;
    __builtin_amdgcn_wave_barrier();
  }
  return prefix;
}

// Wave per line, the line's keys in registers: lane l holds kr[q] = key of index i0 + q for
// q < per, i0 + q < i1 (i0 = l per, i1 = min(n, i0 + per)) and 0xffffffff padding beyond (a NaN can
// have that key too, hence the guards). wave_line_kth: the nn-th key, by radix_kth within the wave's
// range of real keys. wave_line_keep: emit(q, keep) for q = 0 .. KB - 1, keep = the key is below
// kth, or equals it and fewer than nn - #below equal keys come before in index order.
// wave_line_select: both.
template <int KB>
__device__ __forceinline__ unsigned wave_line_kth(const unsigned (&kr)[KB], int per, int i0, int i1, int nn, int lane,
                                                  unsigned* hist) {
  unsigned mn = 0xffffffffu, mx = 0u;  // bound the search by the line's range
#pragma unroll
  for (int q = 0; q < KB; ++q) {
    mn = min(mn, kr[q]);
    if (q < per && i0 + q < i1) mx = max(mx, kr[q]);
  }
  return radix_kth(kr, wave_min_u32(mn), wave_max_u32(mx), nn, lane, hist);
}
template <int KB, class Emit>
__device__ __forceinline__ void wave_line_keep(const unsigned (&kr)[KB], unsigned kth, int per, int i0, int i1, int nn,
                                               Emit emit) {
  int less = 0, eq = 0;
#pragma unroll
  for (int q = 0; q < KB; ++q) {
    less += kr[q] < kth;
    eq += kr[q] == kth;
  }
  const int take_eq = nn - wave_sum(less);
  int seen = wave_incl_scan(eq) - eq;
#pragma unroll
  for (int q = 0; q < KB; ++q) {
    bool v = kr[q] < kth;
    if (kr[q] == kth && q < per && i0 + q < i1) {
      v = seen < take_eq;
      ++seen;
    }
    emit(q, v);
  }
}
template <int KB, class Emit>
__device__ __forceinline__ void wave_line_select(const unsigned (&kr)[KB], int per, int i0, int i1, int nn, int lane,
                                                 unsigned* hist, Emit emit) {
  wave_line_keep(kr, wave_line_kth(kr, per, i0, i1, nn, lane, hist), per, i0, i1, nn, emit);
}

// Wave per line of any length, nothing kept: lane l reads the keys at(k) of its indices [i0, i1)
// again in every pass. wave_stream_kth: the least key with #(keys <= kth) >= nn by bisection over
// [0, 0xffffffff]. wave_stream_keep: one pass for the less / equal counts, one that calls
// emit(k, keep) for every k. wave_line_select_stream: both.
template <class At>
__device__ __forceinline__ unsigned wave_stream_kth(At at, int i0, int i1, int nn) {
  unsigned lo = 0, hi = 0xffffffffu;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    int c = 0;
    for (int k = i0; k < i1; ++k) c += at(k) <= mid;
    if (wave_sum(c) >= nn)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}
template <class At, class Emit>
__device__ __forceinline__ void wave_stream_keep(At at, unsigned kth, int i0, int i1, int nn, Emit emit) {
  int less = 0, eq = 0;
  for (int k = i0; k < i1; ++k) {
    const unsigned kk = at(k);
    less += kk < kth;
    eq += kk == kth;
  }
  const int take_eq = nn - wave_sum(less);  // equal keys taken in index order
  int seen = wave_incl_scan(eq) - eq;
  for (int k = i0; k < i1; ++k) {
    const unsigned kk = at(k);
    bool v = kk < kth;
    if (kk == kth) {
      v = seen < take_eq;
      ++seen;
    }
    emit(k, v);
  }
}
template <class At, class Emit>
__device__ __forceinline__ void wave_line_select_stream(At at, int i0, int i1, int nn, Emit emit) {
  wave_stream_keep(at, wave_stream_kth(at, i0, i1, nn), i0, i1, nn, emit);
}

}  // namespace acoss
