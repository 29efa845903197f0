// misc.hip — the acoss-side pairwise helpers used by EarlyFusionTraile (and exposed on their
// own through the C-ABI):
//   get_oti              acoss/algorithms/utils/cross_recurrence.py:75-103
//   get_csm / get_csm_cosine / get_ssm / get_csm_blocked_oti     cross_recurrence.py:10-134
//   csm_to_binary        cross_recurrence.py:136-161
//   getWCSM              acoss/algorithms/utils/similarity_fusion.py:38-54
//   exp(-x) elementwise (acoss_neg_exp), in the canonical arithmetic
// smith_waterman_constrained and where its alignment lies are in sw.hip.
#include <algorithm>
#include <cstdlib>

#include "common.hpp"
#include "ef_select.hpp"

namespace acoss {

namespace {

// ---------------------------------------------------------------------------------------
// get_oti: argmax_i sum(roll(C1, i) * C2), first max wins (np.argmax).
// ---------------------------------------------------------------------------------------
__global__ void k_get_oti(const float* __restrict__ C1, const float* __restrict__ C2, int n, int32_t* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  float a[12], b[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    a[c] = C1[k * 12 + c];
    b[c] = C2[k * 12 + c];
  }
  int best = 0;
  float bv = 0.0f;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    float s = 0.0f;  // np.sum of the 12 products (sequential; numpy pairwise == sequential below 8+)
#pragma unroll
    for (int c = 0; c < 12; ++c) s = s + a[(c - i + 12) % 12] * b[c];
    if (i == 0 || s > bv) {
      bv = s;
      best = i;
    }
  }
  out[k] = best;
}

// ---------------------------------------------------------------------------------------
// CSM: C = Xr . Yn^T on MFMA (v_mfma_f32_32x32x2_f32, exact f32), 64x64 tile per block of 4
// waves, K staged through LDS in chunks of 32; fused epilogue per kind:
//   0 euclid: sqrt(max(0, (|x|^2 + |y|^2) - 2 C))          (get_csm, :46-48)
//   1 cosine: 1 - C   on rows pre-normalised               (get_csm_cosine, :67-73)
//   2 ssm:    euclid of X with itself, diagonal forced 0    (get_ssm, :24-28)
// Xr = X with every 12-bin block rolled by `roll` (get_csm_blocked_oti, :131-133).
// ---------------------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kT = 64, kKC = 32;

__global__ void k_row_prep(const float* __restrict__ X, int M, int d, int roll, int normalise, float* __restrict__ Xo,
                           float* __restrict__ sq) {
  // one wave per row: rolled (and optionally L2-normalised) copy + squared norm
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* x = X + (size_t)row * d;
  float s = 0.0f;
  for (int c = lane; c < d; c += 64) s += x[c] * x[c];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const float nrm = sqrtf(s);
  const float inv_den = (normalise && nrm != 0.0f) ? nrm : 1.0f;  // XNorm[XNorm == 0] = 1
  float s2 = 0.0f;
  for (int c = lane; c < d; c += 64) {
    int src = c;
    if (roll > 0) {  // np.roll over the chroma axis of each 12-bin block
      const int blk = c / 12, cc = c - blk * 12;
      src = blk * 12 + (cc - roll + 12) % 12;
    }
    const float v = normalise ? x[src] / inv_den : x[src];
    Xo[(size_t)row * d + c] = v;
    s2 += v * v;
  }
  for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
  if (lane == 0) sq[row] = s2;
}

template <int KIND>
__global__ __launch_bounds__(256) void k_csm(const float* __restrict__ X, const float* __restrict__ Y, int M, int N,
                                             int d, const float* __restrict__ xsq, const float* __restrict__ ysq,
                                             float* __restrict__ out) {
  __shared__ float Xs[kT][kKC + 1];
  __shared__ float Ys[kT][kKC + 1];
  const int bi = blockIdx.y * kT, bj = blockIdx.x * kT;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  f32x16 acc = {};
  for (int k0 = 0; k0 < d; k0 += kKC) {
    __syncthreads();
    for (int e = t; e < kT * kKC; e += 256) {
      const int r = e / kKC, c = e - r * kKC;
      const int k = k0 + c;
      Xs[r][c] = (bi + r < M && k < d) ? X[(size_t)(bi + r) * d + k] : 0.0f;
      Ys[r][c] = (bj + r < N && k < d) ? Y[(size_t)(bj + r) * d + k] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kKC; kk += 2) {
      const float a = Xs[32 * wr + (lane & 31)][kk + (lane >> 5)];
      const float b = Ys[32 * wc + (lane & 31)][kk + (lane >> 5)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
    }
  }
  const int col = bj + 32 * wc + (lane & 31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = bi + 32 * wr + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (row < M && col < N) {
      float v;
      if (KIND == 1) {
        v = 1.0f - acc[reg];
      } else {
        float c2 = (xsq[row] + ysq[col]) - 2.0f * acc[reg];
        if (c2 < 0.0f) c2 = 0.0f;
        if (KIND == 2 && row == col) c2 = 0.0f;
        v = sqrtf(c2);
      }
      out[(size_t)row * N + col] = v;
    }
  }
}

// ---------------------------------------------------------------------------------------
// csm_to_binary: the nn smallest of every row -> 1 (ties: lowest column first).
// One wave per row, lane l columns [l * per, (l + 1) * per), the row read again in every
// pass (wave_line_select_stream, ef_select.hpp); a byte per column. nn <= 0: all ones.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_binarize_rows(const float* __restrict__ D, int M, int N, int nn,
                                                       uint8_t* __restrict__ B) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= M) return;
  const float* x = D + (size_t)row * N;
  uint8_t* o = B + (size_t)row * N;
  if (nn <= 0) {
    for (int c = lane; c < N; c += 64) o[c] = 1;
    return;
  }
  const int per = (N + 63) / 64;  // columns per lane (chunked)
  const int c0 = lane * per, c1 = min(N, c0 + per);
  wave_line_select_stream([&](int k) { return fkey_f32(x[k]); }, c0, c1, nn, [&](int k, bool v) { o[k] = v; });
}

// ---------------------------------------------------------------------------------------
// getWCSM: Eps = (mean of k2 smallest per row + mean of k1 smallest per column + CSM) / 3,
// W = exp(-CSM^2 / (2 (mu Eps)^2)).
// ---------------------------------------------------------------------------------------
template <bool COLS>
__global__ __launch_bounds__(256) void k_kmean(const float* __restrict__ C, int M, int N, int k, float* __restrict__ out) {
  // mean of the k smallest values of a row (COLS=false) or column, canonical order (kmean_canon)
  const int line = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nl = COLS ? N : M, len = COLS ? M : N;
  if (line >= nl) return;
  auto at = [&](int e) { return COLS ? C[(size_t)e * N + line] : C[(size_t)line * N + e]; };
  const float m = kmean_canon(at, len, k, lane);
  if (lane == 0) out[line] = m;
}

__global__ void k_wcsm_apply(const float* __restrict__ C, int M, int N, const float* __restrict__ r,
                             const float* __restrict__ c, float mu, float* __restrict__ W) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)M * N) return;
  const int i = (int)(e / N), j = (int)(e - (size_t)i * N);
  const float v = C[e];
  const float eps = ((r[i] + c[j]) + v) / 3.0f;
  const float me = mu * eps;
  W[e] = canon_expf(-(v * v) / (2.0f * (me * me)));
}

}  // namespace

}  // namespace acoss

using namespace acoss;

extern "C" int acoss_get_oti(const float* C1, const float* C2, int32_t n, int32_t* out, void* hip_stream) {
  clear_error();
  if (n < 0 || (n > 0 && (!C1 || !C2 || !out))) {
    set_error("acoss_get_oti: bad arguments");
    return ACOSS_E_ARG;
  }
  if (n == 0) return ACOSS_OK;
  hipLaunchKernelGGL(k_get_oti, dim3((n + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(hip_stream), C1, C2, n,
                     out);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

extern "C" int acoss_csm(const float* X, int32_t M, const float* Y, int32_t N, int32_t d, int32_t kind,
                         int32_t oti_shift, float* out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || d <= 0 || kind < 0 || kind > 2 || !X || !out || (kind != 2 && !Y)) {
    set_error("acoss_csm: bad arguments");
    return ACOSS_E_ARG;
  }
  if (oti_shift > 0 && d % 12 != 0) {
    set_error("acoss_csm: oti_shift needs d to be a multiple of 12");
    return ACOSS_E_ARG;
  }
  if (kind == 2) {
    Y = X;
    N = M;
  }
  if (M == 0 || N == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  prof_begin(PH_CSM, s);
  const size_t bytes = align_up((size_t)M * d * 4, 256) * 2 + align_up((size_t)(M + N) * 4, 256);
  char* ws = static_cast<char*>(workspace(4, bytes));
  if (!ws) return ACOSS_E_HIP;
  float* Xp = reinterpret_cast<float*>(ws);
  float* Yp = reinterpret_cast<float*>(ws + align_up((size_t)M * d * 4, 256));
  float* sq = reinterpret_cast<float*>(ws + 2 * align_up((size_t)M * d * 4, 256));
  const int roll = oti_shift > 0 ? oti_shift % 12 : 0;
  const int norm = kind == 1;
  // workspace slot 4 holds the prepared X; Y gets its own slot (may be larger than X)
  float* Yw = reinterpret_cast<float*>(workspace(5, align_up((size_t)N * d * 4, 256) + align_up((size_t)N * 4, 256)));
  if (!Yw) return ACOSS_E_HIP;
  float* ysq = Yw + align_up((size_t)N * d, 64);
  (void)Yp;
  hipLaunchKernelGGL(k_row_prep, dim3((M + 3) / 4), dim3(256), 0, s, X, M, d, roll, norm, Xp, sq);
  ACOSS_LAUNCH_CHECK();
  if (kind == 2) {
    hipLaunchKernelGGL(k_row_prep, dim3((N + 3) / 4), dim3(256), 0, s, X, N, d, 0, 0, Yw, ysq);
  } else {
    hipLaunchKernelGGL(k_row_prep, dim3((N + 3) / 4), dim3(256), 0, s, Y, N, d, 0, norm, Yw, ysq);
  }
  ACOSS_LAUNCH_CHECK();
  const dim3 grid((N + kT - 1) / kT, (M + kT - 1) / kT);
  if (kind == 0)
    hipLaunchKernelGGL(k_csm<0>, grid, dim3(256), 0, s, Xp, Yw, M, N, d, sq, ysq, out);
  else if (kind == 1)
    hipLaunchKernelGGL(k_csm<1>, grid, dim3(256), 0, s, Xp, Yw, M, N, d, sq, ysq, out);
  else
    hipLaunchKernelGGL(k_csm<2>, grid, dim3(256), 0, s, Xp, Yw, M, N, d, sq, ysq, out);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_CSM, s);
  return ACOSS_OK;
}

extern "C" int acoss_binarize_rows(const float* D, int32_t M, int32_t N, int32_t nneighbs, uint8_t* B,
                                   void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || (M > 0 && N > 0 && (!D || !B)) || nneighbs > N) {
    set_error("acoss_binarize_rows: bad arguments (nneighbs=%d, N=%d)", nneighbs, N);
    return ACOSS_E_ARG;
  }
  if (M == 0 || N == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  prof_begin(PH_BIN, s);
  hipLaunchKernelGGL(k_binarize_rows, dim3((M + 3) / 4), dim3(256), 0, s, D, M, N, nneighbs, B);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_BIN, s);
  return ACOSS_OK;
}

extern "C" int acoss_wcsm(const float* CSM, int32_t M, int32_t N, int32_t k1, int32_t k2, float mu, float* W,
                          void* hip_stream) {
  clear_error();
  if (M <= 0 || N <= 0 || !CSM || !W || k1 <= 0 || k2 <= 0 || k1 > M || k2 > N) {
    set_error("acoss_wcsm: bad arguments");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  prof_begin(PH_WCSM, s);
  float* ws = static_cast<float*>(workspace(6, ((size_t)M + N) * 4 + 256));
  if (!ws) return ACOSS_E_HIP;
  float* rmean = ws;
  float* cmean = ws + M;
  hipLaunchKernelGGL(k_kmean<false>, dim3((M + 3) / 4), dim3(256), 0, s, CSM, M, N, k2, rmean);
  ACOSS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_kmean<true>, dim3((N + 3) / 4), dim3(256), 0, s, CSM, M, N, k1, cmean);
  ACOSS_LAUNCH_CHECK();
  const size_t tot = (size_t)M * N;
  hipLaunchKernelGGL(k_wcsm_apply, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, CSM, M, N, rmean, cmean, mu,
                     W);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_WCSM, s);
  return ACOSS_OK;
}

__global__ void k_neg_exp(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = canon_expf(-x[e]);
}

extern "C" int acoss_neg_exp(const float* x, int64_t n, float* out, void* hip_stream) {
  clear_error();
  if (n < 0 || (n > 0 && (!x || !out))) {
    set_error("acoss_neg_exp: bad arguments");
    return ACOSS_E_ARG;
  }
  if (n == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(k_neg_exp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, out);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}
