// earlyfusion.hip — EarlyFusion.similarity (acoss/algorithms/earlyfusion_traile.py:157-198) for a
// batch of pairs: one launch per stage for a whole chunk of pairs instead of ~15 launches per pair.
//
// Per pair (a, b) with beat-synchronous block features (M = n_blocks[a] rows, N = n_blocks[b]):
//   CSM_m = get_csm(mfccs_a, mfccs_b)              euclid, d = 1000   (:173)
//   CSM_s = get_csm(ssms_a, ssms_b)                euclid, d = 1225   (:175)
//   CSM_c = get_csm_blocked_oti(chromas_a, chromas_b, med_a, med_b, get_csm_cosine)  d = 480 (:178)
//   scores[mfccs|ssms|chromas] = SW(csm_to_binary(CSM_x, kappa))                      (:174-181)
//   W = ((0 + getWCSM(CSM_m)) + getWCSM(CSM_s)) + getWCSM(CSM_c); E = exp(-W)          (:184-188)
//   scores[early] = SW(csm_to_binary(E, kappa))                                        (:189)
// This file: ef_batches, the chunk driver under acoss_earlyfusion, acoss_earlyfusion_locate and
// acoss_earlyfusion_path, and every stage after the CSMs. Stages (workspace chunk of P pairs, every
// per-pair matrix padded to ld x ld; chunks alternate between two streams):
//   ef_prepare, ef_launch_csms   the per-track preparation, once per call, and the three CSMs of a
//                 chunk (ef_csm.hip, through ef_internal.hpp)
//   binarize      csm_to_binary: the round(kappa * N) smallest of each row -> 1, ties lowest
//                 column, into u16 bit words of 16 rows (the SW input): ef_launch_rowbin. Under
//                 ACOSS_EF_BIN_MUTUAL (the entries ending in 2) ef_launch_colpass then clears what
//                 the columns do not keep. The kernels and their shape classes: ef_binarize.hip
//   k_ef_kmin*    mean of the K smallest of each row (k_ef_kmin_rows, a wave per 64 rows through
//                 LDS tiles) and column (k_ef_kmin, a thread per column), K <= 16; k_ef_kmean, a
//                 wave-per-line select, beyond that
//   k_ef_wsum     elementwise: E = exp(-(((0 + W_m) + W_s) + W_c)) in float32, exp = canon_expf
//   SW            ef_launch_swmeta, then launch_swb_batch (sw.hip) over the 4P bit planes; for the
//                 locate and path entries launch_swt_locate / launch_swt_path (sw.hip) instead
// Tolerance vs the reference: the GEMMs' summation order (BLAS vs MFMA), the k-smallest means'
// order (ascending here, np.partition's unspecified there) and exp (canon_expf vs numpy's); every
// other step is the reference's float32 arithmetic. Against the canonical CPU oracle
// (oracle/ef_oracle.cpp) all four scores are bit-identical.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "ef_internal.hpp"
#include "sw_internal.hpp"

namespace acoss {

namespace {

constexpr int kKmax = 16;  // largest K of the streaming k-smallest means

// Mean of the k smallest of each row (COLS = false) or column (K > kKmax); blockIdx.z = matrix;
// canonical order (kmean_canon, common.hpp), as k_ef_kmin.
template <bool COLS>
__global__ __launch_bounds__(256) void k_ef_kmean(const float* __restrict__ C, int64_t mat_stride, int ld, EfPairs E,
                                                  int k, float* __restrict__ out, int64_t omat_stride) {
  const int p = blockIdx.y, m = blockIdx.z;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int line = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int nl = COLS ? N : M, len = COLS ? M : N;
  if (line >= nl) return;
  const float* base = C + m * mat_stride + (size_t)p * ld * ld;
  auto at = [&](int e) { return COLS ? base[(size_t)e * ld + line] : base[(size_t)line * ld + e]; };
  const float mean = kmean_canon(at, len, k, lane);
  if (lane == 0) out[m * omat_stride + (size_t)p * ld + line] = mean;
}

// Mean of the k smallest of each row / column, one THREAD per line streaming it once: the k
// smallest so far stay sorted in registers (one compare rejects most elements, a bubble of
// min/max inserts the rest). Columns: lanes read consecutive columns (coalesced); rows: each
// lane walks its own row (cache lines reused along the walk). Sum in ascending order (the
// reference's np.mean over np.partition output has unspecified order; this ascending order is the
// canonical one the oracle and kmean_canon share).
template <bool COLS, int KMAX, int KC = 0>  // KC > 0: k fixed at compile time (k = KC = KMAX)
__global__ __launch_bounds__(256) void k_ef_kmin(const float* __restrict__ C, int64_t mat_stride, int ld, EfPairs E,
                                                 int k_rt, float* __restrict__ out, int64_t omat_stride, int ppb,
                                                 int n_pairs) {
  const int k = KC ? KC : k_rt;
  // ppb pairs per block (short tracks: 4 pairs x 64 lines per 256-thread block, ld <= 64)
  const int lpb = 256 / ppb;
  const int p = blockIdx.y * ppb + (int)threadIdx.x / lpb, m = blockIdx.z;
  if (p >= n_pairs) return;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int line = blockIdx.x * lpb + (int)threadIdx.x % lpb;
  const int nl = COLS ? N : M, len = COLS ? M : N;
  if (line >= nl) return;
  const float* base = C + m * mat_stride + (size_t)p * ld * ld + (COLS ? (size_t)line : (size_t)line * ld);
  const size_t step = COLS ? (size_t)ld : 1;
  float top[KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) top[q] = INFINITY;
  for (int e = 0; e < len; ++e) {
    float v = base[e * step];
    float kth = top[0];
#pragma unroll
    for (int q = 1; q < KMAX; ++q) kth = (q == k - 1) ? top[q] : kth;
    if (v < kth) {
#pragma unroll
      for (int q = 0; q < KMAX; ++q) {
        if (q < k) {
          const float lo = fminf(top[q], v), hi = fmaxf(top[q], v);
          top[q] = lo;
          v = hi;
        }
      }
    }
  }
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < KMAX; ++q)
    if (q < k) sum += top[q];
  out[m * omat_stride + (size_t)p * ld + line] = sum / (float)k;
}

// Row variant of k_ef_kmin: a wave takes 64 rows and stages 64 x 64 tiles through LDS with
// coalesced row-segment loads; lane r then walks row r of the tile (same insertion order as
// k_ef_kmin<false>: columns ascending).
template <int KMAX, int KC = 0>
__global__ __launch_bounds__(64) void k_ef_kmin_rows(const float* __restrict__ C, int64_t mat_stride, int ld,
                                                     EfPairs E, int k_rt, float* __restrict__ out,
                                                     int64_t omat_stride) {
  const int k = KC ? KC : k_rt;
#ifndef ACOSS_EF_KMIN_TW
#define ACOSS_EF_KMIN_TW 16
#endif
  // 16-column tiles: 4.3 KB of LDS per one-wave block, so LDS no longer caps the resident waves
  // (the 64-column tile, 16.6 KB, allowed 9 per CU: EarlyFusion 58.0k -> 61.8k pairs/s); each
  // load instruction takes 64 / TW rows x TW columns
  constexpr int TW = ACOSS_EF_KMIN_TW;
  __shared__ float t[64][TW + 1];
  const int p = blockIdx.y, m = blockIdx.z;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int row0 = blockIdx.x * 64;
  if (row0 >= M) return;
  const int lane = threadIdx.x;
  const float* base = C + m * mat_stride + (size_t)p * ld * ld;
  const int nr = min(64, M - row0);
  float top[KMAX];
#pragma unroll
  for (int q = 0; q < KMAX; ++q) top[q] = INFINITY;
  for (int c0 = 0; c0 < N; c0 += TW) {
    const int nc = min(TW, N - c0);
    __syncthreads();
    constexpr int RPI = 64 / TW;  // rows per load instruction
    const int lc = lane % TW, lr = lane / TW;
    for (int rr = lr; rr < nr; rr += RPI) t[rr][lc] = lc < nc ? base[(size_t)(row0 + rr) * ld + c0 + lc] : 0.0f;
    __syncthreads();
    for (int e = 0; e < nc; ++e) {
      float v = t[lane][e];
      float kth = top[0];
#pragma unroll
      for (int q = 1; q < KMAX; ++q) kth = (q == k - 1) ? top[q] : kth;
      if (v < kth) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
          if (q < k) {
            const float lo = fminf(top[q], v), hi = fmaxf(top[q], v);
            top[q] = lo;
            v = hi;
          }
        }
      }
    }
  }
  if (lane >= nr) return;
  float sum = 0.0f;
#pragma unroll
  for (int q = 0; q < KMAX; ++q)
    if (q < k) sum += top[q];
  out[m * omat_stride + (size_t)p * ld + row0 + lane] = sum / (float)k;
}

// E = exp(-(((0 + W_0) + W_1) + W_2)), W_s = getWCSM(C_s); written over C_0 (elementwise, in place).
__global__ void k_ef_wsum(float* __restrict__ C, int64_t mat_stride, int ld, EfPairs E, const float* __restrict__ rmean,
                          const float* __restrict__ cmean, int64_t mean_stride, float mu) {
  const int p = blockIdx.y;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;  // M N <= ld^2 < 2^31: 32-bit division
  if (e >= (unsigned)(M * N)) return;
  const int i = (int)(e / (unsigned)N), j = (int)(e - (unsigned)i * (unsigned)N);
  const size_t idx = (size_t)p * ld * ld + (size_t)i * ld + j;
  float wsum = 0.0f;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float v = C[m * mat_stride + idx];
    const float eps = ((rmean[m * mean_stride + (size_t)p * ld + i] + cmean[m * mean_stride + (size_t)p * ld + j]) + v) / 3.0f;
    const float me = mu * eps;
    wsum = wsum + canon_expf(-(v * v) / (2.0f * (me * me)));
  }
  C[idx] = canon_expf(-wsum);
}

// SW metadata of the `repeat` matrices of each pair (here 4: matrix p*4 + s = bit plane s of pair p).
__global__ void k_ef_swmeta(EfPairs E, int P, int repeat, int32_t* rows, int32_t* cols) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  for (int s = 0; s < repeat; ++s) {
    rows[p * repeat + s] = M;
    cols[p * repeat + s] = N;
  }
}

}  // namespace

int ef_launch_swmeta(const EfPairs& E, int P, int repeat, int32_t* rows, int32_t* cols, hipStream_t st) {
  hipLaunchKernelGGL(k_ef_swmeta, dim3((P + 255) / 256), dim3(256), 0, st, E, P, repeat, rows, cols);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

namespace {

// What the batch driver does with a chunk's 4P bit planes, its last stage.
enum EfStage { EF_SCORE, EF_LOCATE, EF_PATH };

// The one driver under acoss_earlyfusion, acoss_earlyfusion_locate and acoss_earlyfusion_path: every
// stage up to the four bit planes of each pair is the same; `stage` picks what runs over them.
// seg_out: int32[n_pairs][4][4] (EF_LOCATE; optional for EF_PATH); len_out int32[n_pairs][4] and
// path_out int32[n_pairs][4][path_cap][2] (EF_PATH).
int ef_batches(EfStage stage, const char* entry, const float* mfcc, const float* ssm, const float* chroma,
               const float* chroma_med, const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks,
               int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma, const int32_t* pairs,
               int64_t n_pairs, double kappa, int32_t K, float mu, int32_t binarize, double* scores_out,
               int32_t* seg_out, int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  clear_error();
  if (binarize != ACOSS_EF_BIN_ROWS && binarize != ACOSS_EF_BIN_MUTUAL) {
    set_error("%s: unknown binarize %d", entry, binarize);
    return ACOSS_E_ARG;
  }
  const bool mutual = binarize == ACOSS_EF_BIN_MUTUAL;
  const EfBank B{mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, d_mfcc, d_ssm, d_chroma};
  if (int rc = ef_check_args(entry, B, max_blocks, pairs, n_pairs, kappa, K, max_blocks, scores_out,
                             n_pairs > 0 && ((stage == EF_LOCATE && !seg_out) ||
                                             (stage == EF_PATH && (!len_out || !path_out)))))
    return rc;
  if (stage == EF_PATH && path_cap < std::max(1, sw_path_bound(max_blocks, max_blocks))) {
    set_error("%s: path_cap %d below max(1, max_blocks - 3) = %d: a path may have that many cells", entry, path_cap,
              std::max(1, sw_path_bound(max_blocks, max_blocks)));
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int ld = (int)align_up((size_t)max_blocks, 4);
  if (ld > 16384) {  // k_ef_binarize keeps one u32 per column in LDS
    set_error("acoss_earlyfusion: more than 16384 blocks in a track");
    return ACOSS_E_ARG;
  }
  EfPrep R;
  if (int rc = ef_prepare(B, s, &R)) return rc;

  // chunk of pairs: 3 CSMs (E overwrites the first), 4 binary matrices, 6 mean vectors, SW scratch
  const size_t mat = (size_t)ld * ld;
  // band-boundary records of the scoring walk or of the tracing / direction DP; for the paths also
  // the direction plane (about ld^2 / 4 bytes) and the end key of each of the four matrices
  const size_t sw_b = stage == EF_SCORE ? sw_bnd_bytes(ld, ld) : align_up(swt_bnd_bytes(ld, ld), 32);
  const size_t plane_b = stage == EF_PATH ? swt_plane_bytes(ld, ld) : 0;
  const int64_t wplane = (int64_t)((ld + 15) / 16) * ld;  // u16 words of one bit plane
  const size_t per_pair = 3 * mat * 4 + 4 * (size_t)wplane * 2 + 6 * (size_t)ld * 4 + 4 * sw_b + 4 * (4 + 4) + 4 +
                          4 * (plane_b + (stage == EF_PATH ? 4 : 0));
  // chunks alternate between two streams with a scratch set each, so one chunk's MFMA CSMs overlap
  // the previous chunk's VALU/latency-bound binarize, k-smallest means and SW (one stream while
  // phases are profiled, or with ACOSS_EF_STREAMS=1)
  const char* st_env = getenv("ACOSS_EF_STREAMS");
  const int nset = (profiling() || (st_env && st_env[0] == '1')) ? 1 : 2;
  int64_t chunk = (int64_t)(ef_chunk_budget() / nset / per_pair);
  if (chunk < 1) chunk = 1;
  if (chunk > 65535) chunk = 65535;
  // sub-batches start at multiples of the packing group (k_ef_csm_pack), so the caller's runs of
  // one query stay aligned with the groups
  if (chunk > kEfPack) chunk -= chunk % kEfPack;
  if (chunk > n_pairs) chunk = n_pairs;
  char* ws = static_cast<char*>(workspace(11, nset * (per_pair * chunk + 16 * 256)));
  if (!ws) return ACOSS_E_HIP;
  size_t o = 0;
  auto carve = [&](size_t bytes) {
    char* r = ws + o;
    o = align_up(o + bytes, 256);
    return r;
  };
  struct EfSet {
    float* C;
    uint16_t* Wb;
    float *rmean, *cmean;
    void* bnd;
    int32_t *m_rows, *m_cols;
    int* oti;
    void* plane;       // EF_PATH only
    uint32_t* endkey;
  } sets[2];
  for (int q = 0; q < nset; ++q) {
    sets[q].C = reinterpret_cast<float*>(carve(3 * mat * 4 * chunk));
    sets[q].Wb = reinterpret_cast<uint16_t*>(carve(4 * (size_t)wplane * 2 * chunk));
    sets[q].rmean = reinterpret_cast<float*>(carve(3 * (size_t)ld * 4 * chunk));
    sets[q].cmean = reinterpret_cast<float*>(carve(3 * (size_t)ld * 4 * chunk));
    sets[q].bnd = carve(4 * sw_b * chunk);
    sets[q].m_rows = reinterpret_cast<int32_t*>(carve(4 * 4 * chunk));
    sets[q].m_cols = reinterpret_cast<int32_t*>(carve(4 * 4 * chunk));
    sets[q].oti = reinterpret_cast<int*>(carve(4 * chunk));
    sets[q].plane = carve(4 * plane_b * chunk);
    sets[q].endkey = reinterpret_cast<uint32_t*>(carve(stage == EF_PATH ? 4 * 4 * chunk : 0));
  }
  hipStream_t ss[2] = {s, s};
  if (nset == 2) {
    ss[1] = side_stream(0);
    if (!ss[1]) {
      set_error("could not create the side stream");
      return ACOSS_E_HIP;
    }
    hipEvent_t e0 = sync_event(0);  // the side stream starts after the per-track prep above
    ACOSS_HIP_CHECK(hipEventRecord(e0, s));
    ACOSS_HIP_CHECK(hipStreamWaitEvent(ss[1], e0, 0));
  }
  const int64_t mstride = (int64_t)mat * chunk;       // between the 3 CSM planes
  const int64_t meanstride = (int64_t)ld * chunk;     // between the 3 mean vectors
  // column k-smallest means: 4 pairs per 256-thread block when every track has at most 64 blocks
  const int kmin_ppb = ld <= 64 ? 4 : 1;
  const unsigned kmin_gx = ld <= 64 ? 1u : (unsigned)((ld + 255) / 256);
  int ci = 0;
  for (int64_t p0 = 0; p0 < n_pairs; p0 += chunk, ++ci) {
    const int P = (int)((n_pairs - p0) < chunk ? (n_pairs - p0) : chunk);
    const EfPairs E{pairs + 2 * p0, block_off, n_blocks};
    hipStream_t st = ss[ci & 1];
    float* C = sets[ci & (nset - 1)].C;
    uint16_t* Wb = sets[ci & (nset - 1)].Wb;
    float* rmean = sets[ci & (nset - 1)].rmean;
    float* cmean = sets[ci & (nset - 1)].cmean;
    void* bnd = sets[ci & (nset - 1)].bnd;
    int32_t* m_rows = sets[ci & (nset - 1)].m_rows;
    int32_t* m_cols = sets[ci & (nset - 1)].m_cols;
    int* oti = sets[ci & (nset - 1)].oti;
    if (int rc = ef_launch_csms(B, R, pairs + 2 * p0, P, ld, oti, false, C, mstride, st)) return rc;
    prof_begin(PH_BIN, st);
    if (int rc = ef_launch_rowbin(C, mstride, ld, E, P, kappa, Wb, wplane, 0, 3, st)) return rc;
    if (mutual)  // before k_ef_wsum writes the early matrix over the first CSM
      if (int rc = ef_launch_colpass(C, mstride, ld, E, P, kappa, Wb, wplane, 0, 3, st)) return rc;
    prof_end(PH_BIN, st);
    prof_begin(PH_WCSM, st);
    if (K == 10) {  // EarlyFusion's K: the k-th smallest is a fixed register, no per-element select
      hipLaunchKernelGGL((k_ef_kmin_rows<10, 10>), dim3((ld + 63) / 64, P, 3), dim3(64), 0, st, C, mstride, ld, E,
                         (int)K, rmean, meanstride);
      ACOSS_LAUNCH_CHECK();
      hipLaunchKernelGGL((k_ef_kmin<true, 10, 10>), dim3(kmin_gx, (P + kmin_ppb - 1) / kmin_ppb, 3), dim3(256), 0, st,
                         C, mstride, ld, E, (int)K, cmean, meanstride, kmin_ppb, P);
      ACOSS_LAUNCH_CHECK();
    } else if (K <= kKmax) {
      hipLaunchKernelGGL((k_ef_kmin_rows<kKmax>), dim3((ld + 63) / 64, P, 3), dim3(64), 0, st, C, mstride, ld, E,
                         (int)K, rmean, meanstride);
      ACOSS_LAUNCH_CHECK();
      hipLaunchKernelGGL((k_ef_kmin<true, kKmax>), dim3(kmin_gx, (P + kmin_ppb - 1) / kmin_ppb, 3), dim3(256), 0, st,
                         C, mstride, ld, E, (int)K, cmean, meanstride, kmin_ppb, P);
      ACOSS_LAUNCH_CHECK();
    } else {
      hipLaunchKernelGGL(k_ef_kmean<false>, dim3((ld + 3) / 4, P, 3), dim3(256), 0, st, C, mstride, ld, E, (int)K,
                         rmean, meanstride);
      ACOSS_LAUNCH_CHECK();
      hipLaunchKernelGGL(k_ef_kmean<true>, dim3((ld + 3) / 4, P, 3), dim3(256), 0, st, C, mstride, ld, E, (int)K,
                         cmean, meanstride);
      ACOSS_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_ef_wsum, dim3((unsigned)((mat + 255) / 256), P), dim3(256), 0, st, C, mstride, ld, E, rmean,
                       cmean, meanstride, mu);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_WCSM, st);
    prof_begin(PH_BIN, st);
    if (int rc = ef_launch_rowbin(C, mstride, ld, E, P, kappa, Wb, wplane, 3, 1, st)) return rc;
    if (mutual)
      if (int rc = ef_launch_colpass(C, mstride, ld, E, P, kappa, Wb, wplane, 3, 1, st)) return rc;
    prof_end(PH_BIN, st);
    prof_begin(PH_SW, st);
    int rc = ef_launch_swmeta(E, P, 4, m_rows, m_cols, st);
    if (rc) return rc;
    if (stage == EF_SCORE)
      rc = launch_swb_batch(Wb, wplane, ld, m_rows, m_cols, 4 * P, ld, ld, bnd, scores_out + 4 * p0, st);
    else if (stage == EF_LOCATE)
      rc = launch_swt_locate(Wb, wplane, ld, m_rows, m_cols, 4 * P, ld, ld, bnd, scores_out + 4 * p0, seg_out + 16 * p0,
                             st);
    else
      rc = launch_swt_path(Wb, wplane, ld, m_rows, m_cols, 4 * P, ld, ld, bnd, sets[ci & (nset - 1)].plane,
                           sets[ci & (nset - 1)].endkey, scores_out + 4 * p0, path_cap,
                           seg_out ? seg_out + 16 * p0 : nullptr, len_out + 4 * p0,
                           path_out + 8 * (size_t)path_cap * (size_t)p0, st);
    if (rc) return rc;
    prof_end(PH_SW, st);
  }
  if (nset == 2) {  // the caller's stream waits for the side stream's chunks
    hipEvent_t e1 = sync_event(1);
    ACOSS_HIP_CHECK(hipEventRecord(e1, ss[1]));
    ACOSS_HIP_CHECK(hipStreamWaitEvent(s, e1, 0));
  }
  return ACOSS_OK;
}

}  // namespace
}  // namespace acoss

using namespace acoss;

extern "C" int acoss_earlyfusion2(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                                  const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks,
                                  int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma,
                                  const int32_t* pairs, int64_t n_pairs, double kappa, int32_t K, float mu,
                                  int32_t binarize, double* scores_out, void* hip_stream) {
  return ef_batches(EF_SCORE, "acoss_earlyfusion", mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks,
                    max_blocks, d_mfcc, d_ssm, d_chroma, pairs, n_pairs, kappa, K, mu, binarize, scores_out, nullptr, 0,
                    nullptr, nullptr, hip_stream);
}

extern "C" int acoss_earlyfusion(const float* mfcc, const float* ssm, const float* chroma, const float* chroma_med,
                                 const int64_t* block_off, const int32_t* n_blocks, int32_t n_tracks,
                                 int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm, int32_t d_chroma,
                                 const int32_t* pairs, int64_t n_pairs, double kappa, int32_t K, float mu,
                                 double* scores_out, void* hip_stream) {
  return acoss_earlyfusion2(mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, max_blocks, d_mfcc, d_ssm,
                            d_chroma, pairs, n_pairs, kappa, K, mu, ACOSS_EF_BIN_ROWS, scores_out, hip_stream);
}

extern "C" int acoss_earlyfusion_locate2(const float* mfcc, const float* ssm, const float* chroma,
                                         const float* chroma_med, const int64_t* block_off, const int32_t* n_blocks,
                                         int32_t n_tracks, int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm,
                                         int32_t d_chroma, const int32_t* pairs, int64_t n_pairs, double kappa,
                                         int32_t K, float mu, int32_t binarize, double* scores_out, int32_t* seg_out,
                                         void* hip_stream) {
  return ef_batches(EF_LOCATE, "acoss_earlyfusion_locate", mfcc, ssm, chroma, chroma_med, block_off, n_blocks,
                    n_tracks, max_blocks, d_mfcc, d_ssm, d_chroma, pairs, n_pairs, kappa, K, mu, binarize, scores_out,
                    seg_out, 0, nullptr, nullptr, hip_stream);
}

extern "C" int acoss_earlyfusion_locate(const float* mfcc, const float* ssm, const float* chroma,
                                        const float* chroma_med, const int64_t* block_off, const int32_t* n_blocks,
                                        int32_t n_tracks, int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm,
                                        int32_t d_chroma, const int32_t* pairs, int64_t n_pairs, double kappa,
                                        int32_t K, float mu, double* scores_out, int32_t* seg_out, void* hip_stream) {
  return acoss_earlyfusion_locate2(mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, max_blocks, d_mfcc,
                                   d_ssm, d_chroma, pairs, n_pairs, kappa, K, mu, ACOSS_EF_BIN_ROWS, scores_out,
                                   seg_out, hip_stream);
}

extern "C" int acoss_earlyfusion_path2(const float* mfcc, const float* ssm, const float* chroma,
                                       const float* chroma_med, const int64_t* block_off, const int32_t* n_blocks,
                                       int32_t n_tracks, int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm,
                                       int32_t d_chroma, const int32_t* pairs, int64_t n_pairs, double kappa, int32_t K,
                                       float mu, int32_t binarize, double* scores_out, int32_t* seg_out,
                                       int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  return ef_batches(EF_PATH, "acoss_earlyfusion_path", mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks,
                    max_blocks, d_mfcc, d_ssm, d_chroma, pairs, n_pairs, kappa, K, mu, binarize, scores_out, seg_out,
                    path_cap, len_out, path_out, hip_stream);
}

extern "C" int acoss_earlyfusion_path(const float* mfcc, const float* ssm, const float* chroma,
                                      const float* chroma_med, const int64_t* block_off, const int32_t* n_blocks,
                                      int32_t n_tracks, int32_t max_blocks, int32_t d_mfcc, int32_t d_ssm,
                                      int32_t d_chroma, const int32_t* pairs, int64_t n_pairs, double kappa, int32_t K,
                                      float mu, double* scores_out, int32_t* seg_out, int32_t path_cap,
                                      int32_t* len_out, int32_t* path_out, void* hip_stream) {
  return acoss_earlyfusion_path2(mfcc, ssm, chroma, chroma_med, block_off, n_blocks, n_tracks, max_blocks, d_mfcc,
                                 d_ssm, d_chroma, pairs, n_pairs, kappa, K, mu, ACOSS_EF_BIN_ROWS, scores_out, seg_out,
                                 path_cap, len_out, path_out, hip_stream);
}
