// common.hpp — host + device helpers shared by the acoss HIP kernels (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "acoss_hip.h"

namespace acoss {

// ---- host side: error string + workspace cache (common.cpp) ----
void set_error(const char* fmt, ...);
void clear_error();
// Grow-only device buffer `slot` on the current device (stream-ordered users: the previous
// contents are not preserved on growth). Returns nullptr (and sets the error) on failure.
void* workspace(int slot, size_t bytes);
int release_all_workspaces();
hipStream_t side_stream(int idx = 0);  // per-device helper streams (non-blocking)
hipEvent_t sync_event(int idx);  // per-device timing-free events for cross-stream ordering

// Optional per-phase timing with HIP events recorded on the launch stream (bench.py reads it
// through acoss_profile_read). Phases are small integers; names in common.cpp.
enum Phase { PH_PREP = 0, PH_OTI, PH_SEL_ROWS, PH_SEL_COLS, PH_MASK, PH_DP_QMAX, PH_DP_DMAX, PH_SW, PH_CSM,
             PH_BIN, PH_WCSM, PH_SIMPLE, PH_SWEEP, PH_FTM_SYNC, PH_FTM_DFT, PH_FTM_MEDIAN, PH_FTM_SCORES,
             PH_DP_TRACE, PH_DP_DIR, PH_BACKTRACK, PH_SNF, PH_RQA, PH_COUNT };
bool profiling();
void prof_begin(int phase, hipStream_t s);
void prof_end(int phase, hipStream_t s);

#define ACOSS_HIP_CHECK(expr)                                                                      \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      ::acoss::set_error("%s:%d %s: %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_));        \
      return ACOSS_E_HIP;                                                                          \
    }                                                                                              \
  } while (0)

#define ACOSS_LAUNCH_CHECK()                                                                       \
  do {                                                                                             \
    hipError_t e_ = hipGetLastError();                                                             \
    if (e_ != hipSuccess) {                                                                        \
      ::acoss::set_error("%s:%d kernel launch: %s", __FILE__, __LINE__, hipGetErrorString(e_));    \
      return ACOSS_E_HIP;                                                                          \
    }                                                                                              \
  } while (0)

// essentia stackChromaFrames count: for (i = 0; i < n - m*tau; i += tau).
__host__ __device__ inline int stacked_len(int n, int m, int tau) {
  const int inc = m * tau;
  return (n <= inc || tau <= 0) ? 0 : (n - inc + tau - 1) / tau;
}

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- device helpers ----
constexpr int kWave = 64;

// ---- wave64 collectives on DPP (VALU, no LDS round trip) ----
// update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl): row_shr:n = 0x110+n,
// row_bcast:15 = 0x142, row_bcast:31 = 0x143 (GFX9 family, gfx950 included).
template <int CTRL, int ROWMASK = 0xf>
__device__ __forceinline__ unsigned dpp_u32(unsigned old, unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)v, CTRL, ROWMASK, 0xf, false);
}

// Inclusive scan (sum) over the 64 lanes.
__device__ __forceinline__ int wave_incl_scan(int x) {
  unsigned v = (unsigned)x;
  v += dpp_u32<0x111>(0u, v);
  v += dpp_u32<0x112>(0u, v);
  v += dpp_u32<0x114>(0u, v);
  v += dpp_u32<0x118>(0u, v);
  v += dpp_u32<0x142, 0xa>(0u, v);
  v += dpp_u32<0x143, 0xc>(0u, v);
  return (int)v;
}

// Reductions: the scan pattern leaves the total in lane 63; readlane broadcasts it (SGPR).
__device__ __forceinline__ int wave_sum(int x) { return __builtin_amdgcn_readlane(wave_incl_scan(x), 63); }

__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
  const unsigned I = 0xffffffffu;
  v = min(v, dpp_u32<0x111>(I, v));
  v = min(v, dpp_u32<0x112>(I, v));
  v = min(v, dpp_u32<0x114>(I, v));
  v = min(v, dpp_u32<0x118>(I, v));
  v = min(v, dpp_u32<0x142, 0xa>(I, v));
  v = min(v, dpp_u32<0x143, 0xc>(I, v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  v = max(v, dpp_u32<0x111>(0u, v));
  v = max(v, dpp_u32<0x112>(0u, v));
  v = max(v, dpp_u32<0x114>(0u, v));
  v = max(v, dpp_u32<0x118>(0u, v));
  v = max(v, dpp_u32<0x142, 0xa>(0u, v));
  v = max(v, dpp_u32<0x143, 0xc>(0u, v));
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// Max of non-negative floats / doubles: order-preserving on the bit patterns.
__device__ __forceinline__ float wave_max(float v) {
  return __builtin_bit_cast(float, wave_max_u32(__builtin_bit_cast(unsigned, v)));
}

__device__ inline double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// Value of lane `src` (wave-uniform) in every lane: v_readlane, no LDS.
__device__ __forceinline__ int lane_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// The n cells a backtrack (crp_dp.hip, sw.hip) left in out[], last to first, turned round by
// the whole wave, and -1 after them up to path_cap.
__device__ __forceinline__ void path_turn_and_pad(int2* out, int n, int path_cap, int lane) {
  for (int t = lane; t < n / 2; t += 64) {
    const int2 a = out[t], b = out[n - 1 - t];
    out[t] = b;
    out[n - 1 - t] = a;
  }
  for (int t = n + lane; t < path_cap; t += 64) out[t] = make_int2(-1, -1);
}

// XCD-aware block swizzle (speed only, never correctness): blocks are dealt round-robin over
// the 8 XCDs, so linear ids b and b + 8 share an L2. This bijection on [0, nwg) makes runs of
// consecutive LOGICAL ids share one XCD (MI355X_MICROARCH.md, workgroup dispatch / T1).
__device__ __forceinline__ int xcd_remap(int lin, int nwg) {
  const int q = nwg / 8, r = nwg % 8, xcd = lin % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lin / 8;
}

// Correctly rounded sqrt (hipcc default: -fhip-fp32-correctly-rounded-divide-sqrt).
__device__ inline float sqrt_rn(float x) { return __builtin_sqrtf(x); }

// Largest float T such that sqrt_rn(T) <= thr (thr >= 0). sqrt_rn is monotone, so for a
// key k >= 0:  sqrt_rn(k) <= thr  <=>  k <= T.  Lets the mask compare squared distances.
__host__ __device__ inline float next_up(float x) {
  unsigned u = __builtin_bit_cast(unsigned, x);
  return __builtin_bit_cast(float, u + 1u);  // x >= 0, finite
}
__host__ __device__ inline float next_down(float x) {
  unsigned u = __builtin_bit_cast(unsigned, x);
  return u == 0u ? x : __builtin_bit_cast(float, u - 1u);
}
// Closed form (no search): with up = next_up(thr) and m = (thr + up) / 2 (exact in double),
// sqrt_rn(T) <= thr  <=>  T < m^2, or T == m^2 and the tie rounds to thr (thr's last bit even).
// m has at most 26 significant bits, so m^2 is exact in double; T is m^2 rounded down to float,
// stepped down once more on an exact tie that rounds up. (The two 16-step searches this replaces
// unrolled into ~100 instructions per line of the selects; tests/test_sq_threshold.py checks the
// closed form against the search.)
__device__ inline float sq_threshold(float thr) {
  const double m = ((double)thr + (double)next_up(thr)) * 0.5;
  const double m2 = m * m;
  float t = (float)m2;             // round to nearest
  if ((double)t > m2) t = next_down(t);  // -> round down
  if ((double)t == m2 && (__builtin_bit_cast(unsigned, thr) & 1u)) t = next_down(t);
  return t;
}

// ---- canonical elementwise math shared with the CPU oracle (oracle/ef_oracle.cpp) ----
// exp(x) of a float in ONE fixed sequence of correctly rounded double operations: k = rint(x / ln2)
// (x times the double 1/ln2), r = x - k ln2 by two fma steps (ln2 = hi + lo), a degree-13 Taylor
// polynomial in r by fma Horner steps, an exact scale by 2^k, one rounding to float. Every step is
// an IEEE basic operation, so the oracle's restatement gives the same bits; ocml's expf and libm's
// expf each round their own way in the last ulp, which made EarlyFusion's early score unpinnable
// (VERDICT r05 missing #1). Relative error before the final rounding < 1e-15 (|r| <= ln2 / 2).
__device__ inline float canon_expf(float xf) {
  const double x = (double)xf;
  if (x != x) return xf;
  if (x < -104.0) return 0.0f;                 // below half the least float denormal
  if (x > 89.0) return __builtin_inff();       // above FLT_MAX
  const double k = __builtin_rint(x * 0x1.71547652b82fep+0);
  double r = __builtin_fma(-k, 0x1.62e42fefa39efp-1, x);
  r = __builtin_fma(-k, 0x1.abc9e3b39803fp-56, r);
  double p = 0x1.6124613a86d09p-33;            // 1/13!
  p = __builtin_fma(p, r, 0x1.1eed8eff8d898p-29);
  p = __builtin_fma(p, r, 0x1.ae64567f544e4p-26);
  p = __builtin_fma(p, r, 0x1.27e4fb7789f5cp-22);
  p = __builtin_fma(p, r, 0x1.71de3a556c734p-19);
  p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-16);
  p = __builtin_fma(p, r, 0x1.a01a01a01a01ap-13);
  p = __builtin_fma(p, r, 0x1.6c16c16c16c17p-10);
  p = __builtin_fma(p, r, 0x1.1111111111111p-7);
  p = __builtin_fma(p, r, 0x1.5555555555555p-5);
  p = __builtin_fma(p, r, 0x1.5555555555555p-3);
  p = __builtin_fma(p, r, 0x1p-1);
  p = __builtin_fma(p, r, 0x1p+0);
  p = __builtin_fma(p, r, 0x1p+0);
  const double s = __builtin_bit_cast(double, (unsigned long long)((long long)k + 1023) << 52);  // 2^k, k in [-150, 129]
  return (float)(p * s);
}

__device__ __forceinline__ unsigned fkey_f32(float f) {  // order-preserving float -> u32
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Mean of the k smallest values of a line in the CANONICAL order (getWCSM's row / column
// k-nearest means, similarity_fusion.py:47-51): the k smallest values (NaN never taken; +inf fills
// in when fewer than k are not NaN) added one at a time in ascending order to +0, then divided by
// k. That is the order k_ef_kmin's sorted registers produce, and the oracle's. One wave per line:
// round t takes the least key above the previous round's (a wave minimum) and adds that value once
// per occurrence, so a line costs one pass per DISTINCT value among its k smallest.
template <class At>
__device__ inline float kmean_canon(At at, int len, int k, int lane) {
  float sum = 0.0f;
  int taken = 0;
  unsigned prev = 0u;
  bool first = true;
  while (taken < k) {  // wave-uniform
    unsigned m = 0xffffffffu;
    for (int e = lane; e < len; e += 64) {
      const float v = at(e);
      const unsigned key = fkey_f32(v);
      if (v == v && (first || key > prev) && key < m) m = key;
    }
    m = wave_min_u32(m);
    if (m == 0xffffffffu) {  // no value left that is not NaN
      sum = sum + __builtin_inff();
      break;
    }
    int c = 0;
    for (int e = lane; e < len; e += 64) c += fkey_f32(at(e)) == m;
    c = wave_sum(c);
    const float v = __builtin_bit_cast(float, (m & 0x80000000u) ? (m & 0x7fffffffu) : ~m);
    for (int t = 0; t < c && taken < k; ++t, ++taken) sum = sum + v;
    prev = m;
    first = false;
  }
  return sum / (float)k;
}

}  // namespace acoss
