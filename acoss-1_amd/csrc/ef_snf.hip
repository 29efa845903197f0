// ef_snf.hip — acoss_earlyfusion_snf: the per-pair similarity network fusion ("early SNF") of
// EarlyFusion for a batch of pairs (the definition: include/acoss_hip.h).
//
// Per pair (a, b), M and N blocks, n = M + N, for each feature f (mfccs, ssms, chromas):
//   CSM_f (M x N), SSMA_f (M x M), SSMB_f (N x N)     float32 distances (ef_launch_csms; the self
//                                                     distances once per track of a chunk)
//   W_f = getWCSMSSM(SSMA_f, SSMB_f, CSM_f, K, mu)    n x n, float32 values held in float64
//   P_f = getP(W_f), S_f = getS(W_f, K)               float64
//   niters rounds of P_f <- S_f ((P_g + P_h) / 2) S_f^T + reg_diag I   (g, h the other two)
//   cross = F[:M, M:] + F[M:, :M]^T, F the mean of the three; the nn largest of each row -> 1
//   early_snf = constrained Smith-Waterman of that matrix (launch_swb_batch)
// Stages over a workspace chunk of pairs (every n x n plane at pitch ldn = 2 ld):
//   k_efs_means    wave per line: the k-smallest means of the CSM's rows and columns and of the two
//                  symmetrised SSMs' rows (k1, k2 of the pair), canonical ascending order
//   k_efs_rows     wave per (row, pair, feature): the row of W (canon_expf), its sequential sum,
//                  the row of P, and the K largest of the row sorted by column (S)
//   the fusion     n <= kEfsLdsN: k_efs_fuse_lds, one workgroup per pair runs all 3 niters steps
//                  with A and B = A S^T in LDS (2 n^2 float64 <= 160 KB), the P planes through L2;
//                  longer pairs: k_efs_diffuse (B = A S^T, a row of A in LDS per block) and
//                  k_efs_left (S B + reg_diag I), one launch each per step over (row, pair)
//   k_efs_cross    F and the cross block (also to the caller's ragged cross_out)
//   binarize       ef_launch_rowbin_snf (k_efs_binarize, ef_binarize.hip): the nn largest of each row,
//                  ties to the lowest column, into the bit plane layout of the Smith-Waterman kernels
//                  (u16 words of 16 rows); acoss_earlyfusion_snf2 with ACOSS_EF_BIN_MUTUAL then runs
//                  ef_launch_colpass_snf over the plane, and copies the plane out as bytes when
//                  binary_out is given
// Both fusion regimes run the same float64 operations in the same order (each product sums over
// the K neighbours in ascending column order from +0, one rounded multiply and one rounded add
// per term), so a pair's bits do not depend on its regime, its chunk or its place in the list.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.hpp"
#include "ef_internal.hpp"
#include "sw_internal.hpp"

namespace acoss {
namespace {

constexpr int kEfsKmax = 64;     // neighbours per row (one per lane in k_efs_rows)
constexpr int kEfsRegs = 16;     // row values per lane kept in registers by k_efs_rows
constexpr int kEfsNmax = 64 * kEfsRegs;  // largest n = M + N
constexpr int kLdsBytes = 160 * 1024;    // LDS of a CU, all of which one workgroup may take
// the LDS regime keeps A and B, n^2 float64 each: 16 n^2 <= 163840 -> n <= 101
constexpr int efs_lds_n() {
  int n = 0;
  while (16 * (n + 1) * (n + 1) <= kLdsBytes) ++n;
  return n;
}
constexpr int kEfsLdsN = efs_lds_n();
static_assert(kEfsLdsN == 101, "2 n^2 float64 within 160 KB");

struct SnfPairs {
  EfPairs E;
  const int32_t *sa, *sb;  // per pair: its tracks' planes among the chunk's self distances
};

// cross_off against the pairs' own M N, before any write: the first bad pair goes to bad[0]
__global__ void k_efs_off_check(EfPairs E, int64_t n_pairs, const int64_t* __restrict__ cross_off, int64_t cross_total,
                                unsigned long long* __restrict__ bad) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int64_t need = (int64_t)E.nb[E.pairs[2 * p]] * E.nb[E.pairs[2 * p + 1]];
  const int64_t lo = cross_off[p], hi = cross_off[p + 1];
  if (lo < 0 || hi < lo || hi > cross_total || need > hi - lo) atomicMin(bad, (unsigned long long)p);
}

// mean[((f P + p) 4 + seg) ld + idx]: seg 0 the k2 smallest of CSM row idx, 1 the k1 smallest of CSM
// column idx, 2 / 3 getW's MeanDist of row idx of DSym(SSMA) with k1 / DSym(SSMB) with k2.
__global__ __launch_bounds__(256) void k_efs_means(const float* __restrict__ C, int64_t cstride,
                                                   const float* __restrict__ T, int64_t tstride, int ld, SnfPairs S,
                                                   int K, int P, float* __restrict__ mean) {
  const int p = blockIdx.y, f = blockIdx.z;
  int a, b, M, N, k1, k2;
  pair_dims(S.E, p, &a, &b, &M, &N);
  if (!snf_split(M, N, K, &k1, &k2)) return;
  const int L = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int seg = L / ld, idx = L - seg * ld;
  if (seg >= 4 || idx >= ((seg & 1) ? N : M)) return;
  const size_t mat = (size_t)ld * ld;
  float m;
  if (seg < 2) {
    const float* Cm = C + f * cstride + (size_t)p * mat;
    if (seg == 0)
      m = kmean_canon([&](int e) { return Cm[(size_t)idx * ld + e]; }, N, k2, lane);
    else
      m = kmean_canon([&](int e) { return Cm[(size_t)e * ld + idx]; }, M, k1, lane);
  } else {
    const float* D = T + f * tstride + (size_t)(seg == 2 ? S.sa[p] : S.sb[p]) * mat;
    const int len = seg == 2 ? M : N, k = seg == 2 ? k1 : k2;
    auto at = [&](int e) { return e == idx ? 0.0f : 0.5f * (D[(size_t)idx * ld + e] + D[(size_t)e * ld + idx]); };
    m = kmean_canon(at, len, k + 1, lane);
    m = m * (float)(k + 1) / (float)k;
  }
  if (lane == 0) mean[(((size_t)f * P + p) * 4 + seg) * ld + idx] = m;
}

// Row i of W_f (float32 values), of P_f = W / rowsum and of S_f for one (row, pair, feature) per
// wave. Lane l holds columns l, l + 64, ...; the row sum adds them one at a time in ascending
// column order (float64); the K largest are taken one per round (greatest value, lowest column
// among equals), ranked by column, summed in that order and divided by the sum.
// Jn / Vn: [(f P + p) K + k][ldn] (neighbour k of every row: rows consecutive).
__global__ __launch_bounds__(256) void k_efs_rows(const float* __restrict__ C, int64_t cstride,
                                                  const float* __restrict__ T, int64_t tstride, int ld, SnfPairs S,
                                                  int K, float mu, int P, const float* __restrict__ mean,
                                                  double* __restrict__ Pl, int32_t* __restrict__ Jn,
                                                  double* __restrict__ Vn) {
  __shared__ int32_t s_j[4][kEfsKmax];
  __shared__ float s_v[4][kEfsKmax];
  const int p = blockIdx.y, f = blockIdx.z;
  int a, b, M, N, k1, k2;
  pair_dims(S.E, p, &a, &b, &M, &N);
  if (!snf_split(M, N, K, &k1, &k2)) return;
  const int n = M + N, ldn = 2 * ld;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + w;
  if (i >= n) return;  // a whole wave; no block barrier below
  const size_t mat = (size_t)ld * ld;
  const float* Cm = C + f * cstride + (size_t)p * mat;
  const float* DA = T + f * tstride + (size_t)S.sa[p] * mat;
  const float* DB = T + f * tstride + (size_t)S.sb[p] * mat;
  const float* mn = mean + ((size_t)f * P + p) * 4 * ld;  // rmean | cmean | mA | mB
  auto w_ssm = [&](const float* D, const float* md, int r, int c) {
    const float d = r == c ? 0.0f : 0.5f * (D[(size_t)r * ld + c] + D[(size_t)c * ld + r]);
    const float eps = ((md[r] + md[c]) + d) / 3.0f;
    const float me = mu * eps;
    float den = 2.0f * (me * me);
    if (den == 0.0f) den = 1.0f;
    return canon_expf(-(d * d) / den);
  };
  auto w_csm = [&](int r, int c) {  // getWCSM at CSM[r, c]
    const float v = Cm[(size_t)r * ld + c];
    const float eps = ((mn[r] + mn[ld + c]) + v) / 3.0f;
    const float me = mu * eps;
    return canon_expf(-(v * v) / (2.0f * (me * me)));
  };
  float wv[kEfsRegs];
#pragma unroll
  for (int q = 0; q < kEfsRegs; ++q) {
    const int j = lane + 64 * q;
    float v = 0.0f;
    if (j < n) {
      if (i < M)
        v = j < M ? w_ssm(DA, mn + 2 * ld, i, j) : w_csm(i, j - M);
      else
        v = j < M ? w_csm(j, i - M) : w_ssm(DB, mn + 3 * ld, i - M, j - M);
    }
    wv[q] = v;
  }
  double rs = 0.0;
#pragma unroll
  for (int q = 0; q < kEfsRegs; ++q) {
    if (64 * q < n) {  // wave-uniform
      const int cnt = min(64, n - 64 * q);
      const int bits = __builtin_bit_cast(int, wv[q]);
      for (int t = 0; t < cnt; ++t) rs = rs + (double)__builtin_bit_cast(float, __builtin_amdgcn_readlane(bits, t));
    }
  }
  if (rs == 0.0) rs = 1.0;
  double* prow = Pl + ((size_t)f * P + p) * ldn * ldn + (size_t)i * ldn;
#pragma unroll
  for (int q = 0; q < kEfsRegs; ++q) {
    const int j = lane + 64 * q;
    if (j < n) prow[j] = (double)wv[q] / rs;
  }
  // the K largest (K < n): W >= 0 (or NaN, whose pattern orders above every number), so the bit
  // patterns order as the values; key + 1 leaves 0 for "no candidate"
  unsigned taken = 0u;
  int sel_j = 0;
  float sel_v = 0.0f;
  for (int t = 0; t < K; ++t) {  // wave-uniform
    unsigned bk = 0u;
    int bq = -1;
#pragma unroll
    for (int q = 0; q < kEfsRegs; ++q) {
      const unsigned key = __builtin_bit_cast(unsigned, wv[q]) + 1u;
      const bool better = lane + 64 * q < n && !((taken >> q) & 1u) && (bq < 0 || key > bk);
      bk = better ? key : bk;
      bq = better ? q : bq;
    }
    const unsigned m = wave_max_u32(bq >= 0 ? bk : 0u);
    const unsigned col = wave_min_u32(bq >= 0 && bk == m ? (unsigned)(lane + 64 * bq) : 0xffffffffu);
    if (lane == (int)(col & 63u)) taken |= 1u << (col >> 6);
    if (lane == t) {
      sel_j = (int)col;
      sel_v = __builtin_bit_cast(float, m - 1u);
    }
  }
  int rank = 0;
  for (int u = 0; u < K; ++u) rank += __builtin_amdgcn_readlane(sel_j, u) < sel_j ? 1 : 0;
  if (lane < K) {
    s_j[w][rank] = sel_j;
    s_v[w][rank] = sel_v;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double sn = 0.0;
  for (int k = 0; k < K; ++k) sn = sn + (double)s_v[w][k];
  if (sn == 0.0) sn = 1.0;
  if (lane < K) {
    const size_t o = (((size_t)f * P + p) * K + lane) * ldn + i;
    Jn[o] = s_j[w][lane];
    Vn[o] = (double)s_v[w][lane] / sn;
  }
}

// The planes of a chunk: X[0..2] the matrices a step reads (P, or the running Pts), Y the plane the
// step's feature writes.
struct FusePlanes {
  const double* in[3];
  double* out;
};

// B[a, j] = sum_k V[j, k] A[a, J[j, k]], A = (X_g + X_h) / 2 (g < h the features other than f), for
// one row a of one pair per block; the row of A sits in LDS.
__global__ __launch_bounds__(256) void k_efs_diffuse(FusePlanes X, int f, int ld, EfPairs E, int K, int P, int n_lo,
                                                     const int32_t* __restrict__ Jn, const double* __restrict__ Vn,
                                                     double* __restrict__ Bm) {
  extern __shared__ double s_row[];
  const int p = blockIdx.y, r = blockIdx.x;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  const int n = M + N, ldn = 2 * ld;
  if (!snf_split(M, N, K, &k1, &k2) || n <= n_lo || r >= n) return;  // the whole block
  const size_t base = (size_t)p * ldn * ldn + (size_t)r * ldn;
  const double* x0 = X.in[f == 0 ? 1 : 0] + base;
  const double* x1 = X.in[f == 2 ? 1 : 2] + base;
  for (int c = threadIdx.x; c < n; c += 256) s_row[c] = (x0[c] + x1[c]) / 2.0;
  __syncthreads();
  const int32_t* J = Jn + ((size_t)f * P + p) * K * ldn;
  const double* V = Vn + ((size_t)f * P + p) * K * ldn;
  for (int j = threadIdx.x; j < n; j += 256) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = acc + V[(size_t)k * ldn + j] * s_row[J[(size_t)k * ldn + j]];
    Bm[base + j] = acc;
  }
}

// out[i, c] = sum_k V[i, k] B[J[i, k], c] (+ reg_diag at c == i), one row i of one pair per block.
__global__ __launch_bounds__(256) void k_efs_left(const double* __restrict__ Bm, int f, int ld, EfPairs E, int K, int P,
                                                  int n_lo, const int32_t* __restrict__ Jn,
                                                  const double* __restrict__ Vn, double reg_diag,
                                                  double* __restrict__ out) {
  __shared__ int32_t s_j[kEfsKmax];
  __shared__ double s_v[kEfsKmax];
  const int p = blockIdx.y, i = blockIdx.x;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  const int n = M + N, ldn = 2 * ld;
  if (!snf_split(M, N, K, &k1, &k2) || n <= n_lo || i >= n) return;  // the whole block
  if ((int)threadIdx.x < K) {
    const size_t o = (((size_t)f * P + p) * K + threadIdx.x) * ldn + i;
    s_j[threadIdx.x] = Jn[o];
    s_v[threadIdx.x] = Vn[o];
  }
  __syncthreads();
  const double* B = Bm + (size_t)p * ldn * ldn;
  double* o = out + (size_t)p * ldn * ldn + (size_t)i * ldn;
  for (int c = threadIdx.x; c < n; c += 256) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = acc + s_v[k] * B[(size_t)s_j[k] * ldn + c];
    if (c == i && reg_diag > 0.0) acc = acc + reg_diag;
    o[c] = acc;
  }
}

// All 3 niters steps of one short pair (n <= kEfsLdsN) in one workgroup: A and B in LDS, the three
// running matrices in their global planes (L2). The first round reads Pl[0..2] and writes
// Pl[3..5]; every later round updates Pl[3..5] in place, feature by feature, as the reference's
// aliased lists do. Block barriers order the global writes of a step before the next step's reads
// (one workgroup, one CU). A launch takes the pairs with n_lo < n <= n_hi, with LDS for n_hi and
// THREADS sized to that class, so the short pairs of a chunk run several workgroups per CU.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_efs_fuse_lds(double* __restrict__ Pl, int ld, EfPairs E, int K, int P,
                                                          int n_lo, int n_hi, int niters,
                                                          const int32_t* __restrict__ Jn,
                                                          const double* __restrict__ Vn, double reg_diag) {
  extern __shared__ double s_ab[];
  const int p = blockIdx.x;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  const int n = M + N, ldn = 2 * ld;
  if (!snf_split(M, N, K, &k1, &k2) || n <= n_lo || n > n_hi) return;  // the whole block
  double* A = s_ab;
  double* B = s_ab + n * n;
  const size_t n2 = (size_t)ldn * ldn, fs = (size_t)P * n2;  // plane and feature strides
  const int tid = threadIdx.x, nn = n * n;
  for (int it = 0; it < niters; ++it) {
    for (int f = 0; f < 3; ++f) {
      const int g = f == 0 ? 1 : 0, h = f == 2 ? 1 : 2;
      const double* x0 = Pl + (it == 0 ? g : 3 + g) * fs + (size_t)p * n2;
      const double* x1 = Pl + (it == 0 ? h : 3 + h) * fs + (size_t)p * n2;
      double* out = Pl + (3 + f) * fs + (size_t)p * n2;
      const int32_t* J = Jn + ((size_t)f * P + p) * K * ldn;
      const double* V = Vn + ((size_t)f * P + p) * K * ldn;
      for (int e = tid; e < nn; e += THREADS) {
        const int r = e / n, c = e - r * n;
        A[e] = (x0[(size_t)r * ldn + c] + x1[(size_t)r * ldn + c]) / 2.0;
      }
      __syncthreads();
      for (int e = tid; e < nn; e += THREADS) {
        const int r = e / n, j = e - r * n;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc = acc + V[(size_t)k * ldn + j] * A[r * n + J[(size_t)k * ldn + j]];
        B[e] = acc;
      }
      __syncthreads();
      for (int e = tid; e < nn; e += THREADS) {
        const int i = e / n, c = e - i * n;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) acc = acc + V[(size_t)k * ldn + i] * B[J[(size_t)k * ldn + i] * n + c];
        if (c == i && reg_diag > 0.0) acc = acc + reg_diag;
        out[(size_t)i * ldn + c] = acc;
      }
      __syncthreads();
    }
  }
}

// F = (((0 + X_0) + X_1) + X_2) / 3; cross[i, j] = F[i, M + j] + F[M + j, i] into the chunk's
// cross planes (pitch ld) and, when asked for, the caller's ragged cross_out. A pair the reference
// cannot fuse writes NaN over its range of cross_out.
__global__ void k_efs_cross(const double* __restrict__ X, int ld, EfPairs E, int K, int P, double* __restrict__ cr,
                            const int64_t* __restrict__ cross_off, double* __restrict__ cross_out) {
  const int p = blockIdx.y;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (unsigned)(M * N)) return;
  const int i = (int)(e / (unsigned)N), j = (int)(e - (unsigned)i * (unsigned)N);
  double v = __builtin_nan("");
  if (snf_split(M, N, K, &k1, &k2)) {
    const int ldn = 2 * ld;
    const size_t n2 = (size_t)ldn * ldn, fs = (size_t)P * n2;
    const double* x = X + (size_t)p * n2;
    const size_t u = (size_t)i * ldn + M + j, l = (size_t)(M + j) * ldn + i;
    const double fu = (((0.0 + x[u]) + x[fs + u]) + x[2 * fs + u]) / 3.0;
    const double fl = (((0.0 + x[l]) + x[fs + l]) + x[2 * fs + l]) / 3.0;
    v = fu + fl;
    cr[(size_t)p * ld * ld + (size_t)i * ld + j] = v;
  }
  if (cross_out) cross_out[cross_off[p] + (int64_t)i * N + j] = v;
}

__global__ void k_efs_refused(EfPairs E, int P, int K, double* __restrict__ score) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  if (!snf_split(M, N, K, &k1, &k2)) score[p] = __builtin_nan("");
}

}  // namespace
}  // namespace acoss

using namespace acoss;

namespace {

// The one driver under acoss_earlyfusion_snf and acoss_earlyfusion_snf2.
int efs_batches(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks, int32_t max_blocks,
                int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs, int64_t n_pairs, double kappa,
                int32_t K, float mu, int32_t binarize, int32_t niters, double reg_diag, double* score_out,
                const int64_t* cross_off, int64_t cross_total, double* cross_out, uint8_t* binary_out,
                void* hip_stream) {
  clear_error();
  if (binarize != ACOSS_EF_BIN_ROWS && binarize != ACOSS_EF_BIN_MUTUAL) {
    set_error("acoss_earlyfusion_snf2: unknown binarize %d", binarize);
    return ACOSS_E_ARG;
  }
  const bool ragged = cross_out || binary_out;  // either output is laid out by cross_off
  const EfBank B{mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, d_mfcc, d_ssm, d_chroma};
  // K against the lane limit only, whatever max_blocks is: the reference needs K < M + N, k1 <= M - 2
  // and k2 <= N - 2 of each pair (snf_split), and a pair that breaks them scores NaN on its own
  if (int rc = ef_check_args("acoss_earlyfusion_snf", B, max_blocks, pairs, n_pairs, kappa, K, kEfsKmax, score_out,
                             niters < 0 || !(reg_diag >= 0.0) || (ragged && (!cross_off || cross_total < 0))))
    return rc;
  const int ld = (int)align_up((size_t)max_blocks, 4);
  if (2 * ld > kEfsNmax) {
    set_error("acoss_earlyfusion_snf: more than %d blocks in a track", kEfsNmax / 2);
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const EfPairs Eall{pairs, block_off, n_blocks};
  // the pair list on the host (the tracks of each chunk), cross_off checked on the device
  std::vector<int32_t> hp((size_t)2 * n_pairs);
  unsigned long long* d_bad = static_cast<unsigned long long*>(workspace(27, 256));
  if (!d_bad) return ACOSS_E_HIP;
  unsigned long long h_bad = ~0ull;
  if (ragged) {
    ACOSS_HIP_CHECK(hipMemsetAsync(d_bad, 0xff, 8, s));
    hipLaunchKernelGGL(k_efs_off_check, dim3((unsigned)((n_pairs + 255) / 256)), dim3(256), 0, s, Eall, n_pairs,
                       cross_off, cross_total, d_bad);
    ACOSS_LAUNCH_CHECK();
    ACOSS_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, 8, hipMemcpyDeviceToHost, s));
  }
  ACOSS_HIP_CHECK(hipMemcpyAsync(hp.data(), pairs, hp.size() * 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_bad != ~0ull) {
    set_error("acoss_earlyfusion_snf: cross_off of pair %lld is negative, leaves less than the pair's M * N or ends "
              "past cross_total=%lld", (long long)h_bad, (long long)cross_total);
    return ACOSS_E_ARG;
  }
  for (int32_t t : hp)
    if (t < 0 || t >= n_tracks) {
      set_error("acoss_earlyfusion_snf: a pair names a track outside [0, %d)", n_tracks);
      return ACOSS_E_ARG;
    }
  EfPrep R;
  if (int rc = ef_prepare(B, s, &R)) return rc;

  // chunk of pairs under the byte budget of acoss_earlyfusion (ACOSS_EF_BYTES): 3 CSMs, the self
  // distances of at most 2 tracks per pair, the means, 6 running planes and B, the neighbour
  // lists, the cross plane, the bit plane and the Smith-Waterman scratch
  const int ldn = 2 * ld;
  const size_t mat = (size_t)ld * ld, n2 = (size_t)ldn * ldn;
  const int64_t wplane = (int64_t)((ld + 15) / 16) * ld;
  const size_t sw_b = sw_bnd_bytes(ld, ld);
  const size_t per_pair = 3 * mat * 4 + 2 * 3 * mat * 4 + 3 * 4 * (size_t)ld * 4 + 7 * n2 * 8 +
                          3 * (size_t)K * ldn * 12 + mat * 8 + (size_t)wplane * 2 + sw_b + 64;
  int64_t chunk = (int64_t)(ef_chunk_budget() / per_pair);
  if (chunk < 1) chunk = 1;
  if (chunk > 32768) chunk = 32768;
  if (chunk > n_pairs) chunk = n_pairs;
  // per chunk: its distinct tracks (the self pairs (t, t)) and each pair's two slots among them
  const int64_t n_chunks = (n_pairs + chunk - 1) / chunk;
  std::vector<int32_t> h_self, h_slot((size_t)2 * n_pairs);
  std::vector<int64_t> self_off((size_t)n_chunks + 1, 0);
  {
    std::vector<int32_t> seen((size_t)n_tracks, -1), slot((size_t)n_tracks, 0);
    for (int64_t ci = 0; ci < n_chunks; ++ci) {
      const int64_t p0 = ci * chunk, p1 = std::min(n_pairs, p0 + chunk);
      int32_t u = 0;
      for (int64_t e = 2 * p0; e < 2 * p1; ++e) {
        const int32_t t = hp[(size_t)e];
        if (seen[(size_t)t] != (int32_t)ci) {
          seen[(size_t)t] = (int32_t)ci;
          slot[(size_t)t] = u++;
          h_self.push_back(t);
          h_self.push_back(t);
        }
        // the chunk's slots: its pairs' first tracks, then their second tracks
        h_slot[(size_t)(2 * p0 + (e & 1) * (p1 - p0) + (e - 2 * p0) / 2)] = slot[(size_t)t];
      }
      self_off[(size_t)ci + 1] = self_off[(size_t)ci] + u;
    }
  }
  int64_t umax = 0;
  for (int64_t ci = 0; ci < n_chunks; ++ci) umax = std::max(umax, self_off[(size_t)ci + 1] - self_off[(size_t)ci]);
  const size_t idx_bytes = align_up(h_self.size() * 4, 256) + align_up(h_slot.size() * 4, 256);
  char* iws = static_cast<char*>(workspace(27, 256 + idx_bytes));
  if (!iws) return ACOSS_E_HIP;
  int32_t* d_self = reinterpret_cast<int32_t*>(iws + 256);
  int32_t* d_slot = reinterpret_cast<int32_t*>(iws + 256 + align_up(h_self.size() * 4, 256));
  ACOSS_HIP_CHECK(hipMemcpyAsync(d_self, h_self.data(), h_self.size() * 4, hipMemcpyHostToDevice, s));
  ACOSS_HIP_CHECK(hipMemcpyAsync(d_slot, h_slot.data(), h_slot.size() * 4, hipMemcpyHostToDevice, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));  // the host vectors are read by then

  size_t o = 0;
  auto carve = [&](size_t bytes) {
    const size_t r = o;
    o = align_up(o + bytes, 256);
    return r;
  };
  const size_t o_C = carve(3 * mat * 4 * chunk), o_T = carve(3 * mat * 4 * umax);
  const size_t o_mean = carve(3 * 4 * (size_t)ld * 4 * chunk), o_Pl = carve(6 * n2 * 8 * chunk);
  const size_t o_B = carve(n2 * 8 * chunk), o_J = carve(3 * (size_t)K * ldn * 4 * chunk);
  const size_t o_V = carve(3 * (size_t)K * ldn * 8 * chunk), o_cr = carve(mat * 8 * chunk);
  const size_t o_Wb = carve((size_t)wplane * 2 * chunk), o_bnd = carve(sw_b * chunk);
  const size_t o_rows = carve(4 * chunk), o_cols = carve(4 * chunk);
  const size_t o_oti = carve(4 * std::max<int64_t>(chunk, umax));
  char* ws = static_cast<char*>(workspace(28, o));
  if (!ws) return ACOSS_E_HIP;
  float* C = reinterpret_cast<float*>(ws + o_C);
  float* T = reinterpret_cast<float*>(ws + o_T);
  float* mean = reinterpret_cast<float*>(ws + o_mean);
  double* Pl = reinterpret_cast<double*>(ws + o_Pl);
  double* Bm = reinterpret_cast<double*>(ws + o_B);
  int32_t* Jn = reinterpret_cast<int32_t*>(ws + o_J);
  double* Vn = reinterpret_cast<double*>(ws + o_V);
  double* cr = reinterpret_cast<double*>(ws + o_cr);
  uint16_t* Wb = reinterpret_cast<uint16_t*>(ws + o_Wb);
  void* bnd = ws + o_bnd;
  int32_t* m_rows = reinterpret_cast<int32_t*>(ws + o_rows);
  int32_t* m_cols = reinterpret_cast<int32_t*>(ws + o_cols);
  int* oti = reinterpret_cast<int*>(ws + o_oti);

  // the LDS regime's largest n (ACOSS_EFS_LDS_N lowers it: 0 sends every pair through the planes)
  int n_lds = kEfsLdsN;
  if (const char* e = getenv("ACOSS_EFS_LDS_N")) n_lds = std::max(0, std::min(kEfsLdsN, atoi(e)));
  const int n_fuse = std::min(n_lds, ldn);  // the longest pair the LDS kernel can meet in this call
  // its size classes: (0, 45] 256 threads and 32 KB (5 workgroups per CU), (45, 64] 512 threads and
  // 64 KB (2), (64, n_fuse] 1024 threads and up to 160 KB (1)
  const int c1 = std::min(45, n_fuse), c2 = std::min(64, n_fuse);
  if ((size_t)16 * n_fuse * n_fuse > 64 * 1024)
    ACOSS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_efs_fuse_lds<1024>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 16 * n_fuse * n_fuse));
  for (int64_t ci = 0; ci < n_chunks; ++ci) {
    const int64_t p0 = ci * chunk;
    const int P = (int)std::min(chunk, n_pairs - p0);
    const int U = (int)(self_off[(size_t)ci + 1] - self_off[(size_t)ci]);
    const EfPairs E{pairs + 2 * p0, block_off, n_blocks};
    const SnfPairs S{E, d_slot + 2 * p0, d_slot + 2 * p0 + P};
    const int64_t cstride = (int64_t)mat * P, tstride = (int64_t)mat * U;
    if (int rc = ef_launch_csms(B, R, d_self + 2 * self_off[(size_t)ci], U, ld, oti, true, T, tstride, s)) return rc;
    if (int rc = ef_launch_csms(B, R, pairs + 2 * p0, P, ld, oti, false, C, cstride, s)) return rc;
    prof_begin(PH_WCSM, s);
    hipLaunchKernelGGL(k_efs_means, dim3((unsigned)ld, P, 3), dim3(256), 0, s, C, cstride, T, tstride, ld, S, (int)K, P,
                       mean);
    ACOSS_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_efs_rows, dim3((unsigned)((ldn + 3) / 4), P, 3), dim3(256), 0, s, C, cstride, T, tstride, ld, S,
                       (int)K, mu, P, mean, Pl, Jn, Vn);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_WCSM, s);
    prof_begin(PH_SNF, s);  // the cross-diffusion steps and the cross block
    const size_t fs = (size_t)P * n2;  // between the planes of two features
    if (niters > 0 && n_fuse > 0) {
      hipLaunchKernelGGL(k_efs_fuse_lds<256>, dim3(P), dim3(256), (size_t)16 * c1 * c1, s, Pl, ld, E, (int)K, P, 0, c1,
                         (int)niters, Jn, Vn, reg_diag);
      ACOSS_LAUNCH_CHECK();
      if (c2 > c1) {
        hipLaunchKernelGGL(k_efs_fuse_lds<512>, dim3(P), dim3(512), (size_t)16 * c2 * c2, s, Pl, ld, E, (int)K, P, c1,
                           c2, (int)niters, Jn, Vn, reg_diag);
        ACOSS_LAUNCH_CHECK();
      }
      if (n_fuse > c2) {
        hipLaunchKernelGGL(k_efs_fuse_lds<1024>, dim3(P), dim3(1024), (size_t)16 * n_fuse * n_fuse, s, Pl, ld, E,
                           (int)K, P, c2, n_fuse, (int)niters, Jn, Vn, reg_diag);
        ACOSS_LAUNCH_CHECK();
      }
    }
    if (ldn > n_fuse) {  // longer pairs may exist: a launch per product of each step
      for (int it = 0; it < niters; ++it)
        for (int f = 0; f < 3; ++f) {
          const int base = it == 0 ? 0 : 3;
          const FusePlanes X{{Pl + (base + 0) * fs, Pl + (base + 1) * fs, Pl + (base + 2) * fs}, Pl + (3 + f) * fs};
          hipLaunchKernelGGL(k_efs_diffuse, dim3(ldn, P), dim3(256), (size_t)ldn * 8, s, X, f, ld, E, (int)K, P,
                             n_fuse, Jn, Vn, Bm);
          ACOSS_LAUNCH_CHECK();
          hipLaunchKernelGGL(k_efs_left, dim3(ldn, P), dim3(256), 0, s, Bm, f, ld, E, (int)K, P, n_fuse, Jn, Vn,
                             reg_diag, X.out);
          ACOSS_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(k_efs_cross, dim3((unsigned)((mat + 255) / 256), P), dim3(256), 0, s,
                       Pl + (niters > 0 ? 3 : 0) * fs, ld, E, (int)K, P, cr, cross_out ? cross_off + p0 : nullptr,
                       cross_out);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_SNF, s);
    prof_begin(PH_BIN, s);
    if (int rc = ef_launch_rowbin_snf(cr, ld, E, P, (int)K, kappa, Wb, wplane, s)) return rc;
    if (binarize == ACOSS_EF_BIN_MUTUAL)
      if (int rc = ef_launch_colpass_snf(cr, ld, E, P, (int)K, kappa, Wb, wplane, s)) return rc;
    if (binary_out)
      if (int rc = ef_launch_unpack(Wb, wplane, 1, ld, E, P, cross_off + p0, binary_out, s)) return rc;
    prof_end(PH_BIN, s);
    prof_begin(PH_SW, s);
    if (int rc = ef_launch_swmeta(E, P, 1, m_rows, m_cols, s)) return rc;
    if (int rc = launch_swb_batch(Wb, wplane, ld, m_rows, m_cols, P, ld, ld, bnd, score_out + p0, s)) return rc;
    hipLaunchKernelGGL(k_efs_refused, dim3((P + 255) / 256), dim3(256), 0, s, E, P, (int)K, score_out + p0);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_SW, s);
  }
  return ACOSS_OK;
}

}  // namespace

extern "C" int acoss_earlyfusion_snf(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                                     const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks,
                                     int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma,
                                     const int32_t* pairs, int64_t n_pairs, double kappa, int32_t K, float mu,
                                     int32_t niters, double reg_diag, double* score_out, const int64_t* cross_off,
                                     int64_t cross_total, double* cross_out, void* hip_stream) {
  return efs_batches(mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, max_blocks, d_mfcc, d_ssm, d_chroma,
                     pairs, n_pairs, kappa, K, mu, ACOSS_EF_BIN_ROWS, niters, reg_diag, score_out, cross_off,
                     cross_total, cross_out, nullptr, hip_stream);
}

extern "C" int acoss_earlyfusion_snf2(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                                      const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks,
                                      int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma,
                                      const int32_t* pairs, int64_t n_pairs, double kappa, int32_t K, float mu,
                                      int32_t binarize, int32_t niters, double reg_diag, double* score_out,
                                      const int64_t* cross_off, int64_t cross_total, double* cross_out,
                                      uint8_t* binary_out, void* hip_stream) {
  return efs_batches(mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, max_blocks, d_mfcc, d_ssm, d_chroma,
                     pairs, n_pairs, kappa, K, mu, binarize, niters, reg_diag, score_out, cross_off, cross_total,
                     cross_out, binary_out, hip_stream);
}
