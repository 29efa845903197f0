// crp.hip — Serra09 / LateFusionChen hot path on gfx950:
//   OTI key shift -> stacked-frame Euclidean distances -> per-row / per-column percentile
//   thresholds -> mutual-neighbour CRP mask -> Qmax (serra09) / dmax (chen17) wavefront DP.
//
// Replaces, per pair, essentia ChromaCrossSimilarity + CoverSongSimilarity as called at
// acoss/algorithms/rqa_serra09.py:55-69 and acoss/algorithms/latefusion_chen.py:58-73.
// Arithmetic follows the canonical rounding sequence documented in oracle/crp_oracle.cpp
// step for step (fmaf chains, sequential adds, correctly rounded sqrt), so the OTI index,
// the thresholds and the CRP mask are bit-identical to the CPU restatement.
//
// Design: two CRP paths, chosen in one place (crp_masks below). The reference's
// setting (m = 9, tau = 1, lines of at most 4096 codes) runs the split kernels of crp_split.hip,
// which keep the high 16 bits of every M'xN' distance key in HBM twice (row-major and
// strip-major key planes, 4 B per cell, per sub-batch). Every other shape runs the generic
// kernels of this file, which keep no distance in HBM: the CRP words are the only M'xN' output.
//  * k_crp_select<TRANS>: one 256-thread block per (pair, stripe of R own frames). It
//    sweeps the other song in 256-column panels: the 12-d Gram of (R+m-1) x (256+m-1)
//    frames is computed into LDS (fmaf chains), the m-tap diagonal window gives the squared
//    stacked distance of R x 256 cells, which stay in an LDS stripe. A block-wide 3-pass
//    radix select (11/10/10 bits of the float key) then gives the two order statistics of
//    each row (column for TRANS) and the interpolated percentile threshold. The mask is
//    later evaluated in the squared domain (sq_threshold), so no per-cell sqrt is needed.
//  * k_crp_panel: recomputes the distances of a 32-row x 256-column panel and writes the
//    CRP as one 32-bit word per (32-row strip, column): the layout the DP consumes.
// Under ACOSS_BIN_OTI (the entries ending in 2) crp_masks runs a third producer of the same words,
// crp_otib.hip's k_crp_otib, in place of both: no thresholds, no rolled reference, no key planes.
// Under a ranked OTI (the entries ending in 3; the definition: include/acoss_hip.h, acoss_crp_params3)
// k_oti_rank orders the twelve shifts of every pair of a DP batch, k_pair_oti applies the pair's pick of
// that order in place of the argmax, and crp_batches runs crp_masks and the DP once per round of a best
// of n, k_oti_fold keeping the best score with the shift and the pick that made it.
// The wavefront DP over those words (k_crp_dp*, k_crp_dp_trace for acoss_crp_locate /
// acoss_locate_crp, k_crp_dp_dir and k_crp_backtrack for acoss_crp_path / acoss_path_crp, each also
// for chen17 under the _dmax entries) is crp_dp.hip; this file reaches it through launch_dp,
// launch_trace, launch_dir and launch_backtrack.
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crp_internal.hpp"

namespace acoss {

constexpr int kPanelW = 256;  // columns per panel = threads per block

// --------------------------------------------------------------------------------------
// Per-track preparation (O(sum n)): OTI profile and stacked squared norms.
// --------------------------------------------------------------------------------------
__device__ inline float frame_norm(const float* __restrict__ x) {
  float acc = 0.0f;
#pragma unroll
  for (int c = 0; c < 12; ++c) acc = __builtin_fmaf(x[c], x[c], acc);
  return acc;
}

// 64 threads = 4 tracks x 16 lanes (lanes 12..15 idle). prof[t*12+c].
__global__ void k_track_profile(const float* __restrict__ feats, const int64_t* __restrict__ off,
                                const int32_t* __restrict__ len, int n_tracks, float* __restrict__ prof) {
  const int t = blockIdx.x * 4 + (threadIdx.x >> 4);
  const int c = threadIdx.x & 15;
  float s = 0.0f;
  if (t < n_tracks && c < 12) {
    const int n = len[t];
    const float* x = feats + off[t] * 12 + c;
    for (int a = 0; a < n; ++a) s = s + x[(size_t)a * 12];
    s = n > 0 ? s / (float)n : 0.0f;
  }
  float mx = (c < 12) ? s : -INFINITY;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 16));
  if (t < n_tracks && c < 12) prof[t * 12 + c] = mx > 0.0f ? s / mx : 0.0f;
}

// NX[t*ldn + s] = sum_{u<m} |frame (s+u)*tau|^2 (sequential), s < stacked_len.
__global__ void k_track_norms(const float* __restrict__ feats, const int64_t* __restrict__ off,
                              const int32_t* __restrict__ len, int m, int tau, int ldn, float* __restrict__ NX) {
  const int t = blockIdx.x;
  const int s = blockIdx.y * blockDim.x + threadIdx.x;
  const int S = stacked_len(len[t], m, tau);
  if (s >= S) return;
  const float* x = feats + off[t] * 12;
  float acc = 0.0f;
  for (int u = 0; u < m; ++u) acc = acc + frame_norm(x + (size_t)(s + u) * tau * 12);
  NX[(size_t)t * ldn + s] = acc;
}

// X2[t][f] = frames f and f + 1 of track t interleaved bin by bin (24 floats; frame n is 0):
// the operand pairs of the split sweep's packed-FP32 Gram (crp_split.hip).
__global__ void k_track_pairs(const float* __restrict__ feats, const int64_t* __restrict__ off,
                              const int32_t* __restrict__ len, int ldn, float* __restrict__ X2) {
  const int t = blockIdx.x;
  const int f = blockIdx.y * blockDim.x + threadIdx.x;
  const int n = len[t];
  if (f >= n) return;
  const float* x = feats + (off[t] + f) * 12;
  float4* o = reinterpret_cast<float4*>(X2 + ((size_t)t * ldn + f) * 24);
  const bool nx = f + 1 < n;
#pragma unroll
  for (int c = 0; c < 6; ++c)
    o[c] = make_float4(x[2 * c], nx ? x[12 + 2 * c] : 0.0f, x[2 * c + 1], nx ? x[12 + 2 * c + 1] : 0.0f);
}

// The twelve profile dots of a pair, dot[k] for the reference rolled by k: the fmaf chain the OTI
// compares (include/acoss_hip.h, acoss_crp_params3). Fully unrolled: dot[] stays in registers.
__device__ __forceinline__ void profile_dots(const float* __restrict__ prof, int a, int b, float (&dot)[12]) {
  float pq[12], pr[12];
#pragma unroll
  for (int c = 0; c < 12; ++c) {
    pq[c] = prof[a * 12 + c];
    pr[c] = prof[b * 12 + c];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    float acc = 0.0f;
#pragma unroll
    for (int c = 0; c < 12; ++c) acc = __builtin_fmaf(pq[c], pr[(c - k + 12) % 12], acc);
    dot[k] = acc;
  }
}

// Ranked OTI, one lane per pair: order[p][r] = the shift of rank r, by twelve fully unrolled
// selections of the first strict maximum among the shifts not yet taken (a taken-bit per shift, so
// no register array is indexed at run time and the result is a permutation whatever the dots
// hold). Round 0 makes k_pair_oti's comparisons. dots (may be NULL): dot[p][k].
__global__ void k_oti_rank(const float* __restrict__ prof, const int32_t* __restrict__ pairs, int64_t n_pairs,
                           int32_t* __restrict__ order, float* __restrict__ dots) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  float dot[12];
  profile_dots(prof, pairs[2 * p], pairs[2 * p + 1], dot);
  unsigned taken = 0u;
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    int best = -1;
    float bestv = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      if (!((taken >> k) & 1u) && (best < 0 || dot[k] > bestv)) {
        bestv = dot[k];
        best = k;
      }
    }
    taken |= 1u << best;
    order[12 * p + r] = best;
  }
  if (dots) {
#pragma unroll
    for (int k = 0; k < 12; ++k) dots[12 * p + k] = dot[k];
  }
}

// Best-of fold of round r: where the round's score is strictly larger (or r is 0), it becomes the
// pair's best, with the shift and the pick that made it. best is the batch's own row, so an output
// that was not asked for may be NULL.
__global__ void k_oti_fold(const float* __restrict__ row, const int32_t* __restrict__ oti, int r, int nb,
                           float* __restrict__ best, float* __restrict__ score_out, int32_t* __restrict__ oti_out,
                           int32_t* __restrict__ pick_out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nb) return;
  const float v = row[p];
  if (r == 0 || v > best[p]) {
    best[p] = v;
    if (score_out) score_out[p] = v;
    if (oti_out) oti_out[p] = oti[p];
    if (pick_out) pick_out[p] = r;
  }
}

// Per pair: OTI index (essentia optimalTranspositionIndex restated) and stacked dims. With an order
// (k_oti_rank's, 12 per pair) the index is order[pick], pick the pair's entry of the picks plane or,
// without a plane, the scalar; a pick outside 0 .. 11 raises *err and runs as pick 0.
__global__ void k_pair_oti(const float* __restrict__ prof, const int32_t* __restrict__ len,
                           const int32_t* __restrict__ pairs, int64_t n_pairs, int use_oti, int m, int tau,
                           const int32_t* __restrict__ order, int pick, const int32_t* __restrict__ picks,
                           int* __restrict__ err, int32_t* __restrict__ oti, int2* __restrict__ dims) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int a = pairs[2 * p], b = pairs[2 * p + 1];
  int best = 0;
  if (order) {
    int r = picks ? picks[p] : pick;
    if (r < 0 || r > 11) {
      atomicOr(err, 1);
      r = 0;
    }
    best = order[12 * p + r];
  } else if (use_oti) {
    float pq[12], pr[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      pq[c] = prof[a * 12 + c];
      pr[c] = prof[b * 12 + c];
    }
    float bestv = 0.0f;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      float acc = 0.0f;
#pragma unroll
      for (int c = 0; c < 12; ++c) acc = __builtin_fmaf(pq[c], pr[(c - k + 12) % 12], acc);
      if (k == 0 || acc > bestv) {
        bestv = acc;
        best = k;
      }
    }
  }
  oti[p] = best;
  dims[p] = make_int2(stacked_len(len[a], m, tau), stacked_len(len[b], m, tau));
}

// yrot[p][f][c] = reference[f][(c - oti[p]) mod 12]  (np.roll of every reference frame).
__global__ void k_rotate_ref(const float* __restrict__ feats, const int64_t* __restrict__ off,
                             const int32_t* __restrict__ len, const int32_t* __restrict__ pairs,
                             const int32_t* __restrict__ oti, float* __restrict__ yrot, int64_t stride) {
  const int p = blockIdx.y;
  const int b = pairs[2 * p + 1];
  const int n = len[b], k = oti[p];
  const float* src = feats + off[b] * 12;
  float* dst = yrot + (size_t)p * stride;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n * 12; e += gridDim.x * blockDim.x) {
    const int f = e / 12, c = e - f * 12;
    dst[e] = src[(size_t)f * 12 + (c - k + 12) % 12];
  }
}

// --------------------------------------------------------------------------------------
// Panel machinery: rows = R "own" stacked frames starting at i0, columns = 256 "inner"
// stacked frames starting at j0. LDS: Xs[GR][12], Ys[GW][13], Gs[GR][GW],
// GR = R+m-1, GW = 256+m-1. Own = query unless TRANS (then own = reference).
// --------------------------------------------------------------------------------------
struct PanelArgs {
  const float* own;    // frames of the own track (n_own x 12)
  const float* inner;  // frames of the inner track
  int k_own, k_inner;  // chroma roll applied to own / inner frames (one of them is 0)
  int n_own, n_inner;  // frame counts
  int m, tau;
};

// Stage own frames (once per block): Xs[a][c] = own[(i0+a)*tau][(c-k) mod 12].
__device__ inline void stage_own(const PanelArgs& A, int i0, int GR, float* Xs) {
  for (int e = threadIdx.x; e < GR * 12; e += blockDim.x) {
    const int a = e / 12, c = e - a * 12;
    const int f = (i0 + a) * A.tau;
    Xs[e] = f < A.n_own ? A.own[(size_t)f * 12 + ((c - A.k_own + 12) % 12)] : 0.0f;
  }
}

// Stage inner frames of panel j0 and build the Gram Gs[a][b] = fmaf-chain_c Xs[a][c]*Ys[b][c].
__device__ inline void panel_gram(const PanelArgs& A, int j0, int GR, int GW, const float* Xs, float* Ys,
                                  float* Gs) {
  for (int e = threadIdx.x; e < GW * 12; e += blockDim.x) {
    const int b = e / 12, c = e - b * 12;
    const int f = (j0 + b) * A.tau;
    Ys[b * 13 + c] = f < A.n_inner ? A.inner[(size_t)f * 12 + ((c - A.k_inner + 12) % 12)] : 0.0f;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < GW; b += blockDim.x) {
    float y[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) y[c] = Ys[b * 13 + c];
    for (int a = 0; a < GR; ++a) {
      const float4* xr = reinterpret_cast<const float4*>(Xs + a * 12);
      const float4 x0 = xr[0], x1 = xr[1], x2 = xr[2];
      float acc = 0.0f;
      acc = __builtin_fmaf(x0.x, y[0], acc);
      acc = __builtin_fmaf(x0.y, y[1], acc);
      acc = __builtin_fmaf(x0.z, y[2], acc);
      acc = __builtin_fmaf(x0.w, y[3], acc);
      acc = __builtin_fmaf(x1.x, y[4], acc);
      acc = __builtin_fmaf(x1.y, y[5], acc);
      acc = __builtin_fmaf(x1.z, y[6], acc);
      acc = __builtin_fmaf(x1.w, y[7], acc);
      acc = __builtin_fmaf(x2.x, y[8], acc);
      acc = __builtin_fmaf(x2.y, y[9], acc);
      acc = __builtin_fmaf(x2.z, y[10], acc);
      acc = __builtin_fmaf(x2.w, y[11], acc);
      Gs[a * GW + b] = acc;
    }
  }
  __syncthreads();
}

// Squared stacked distance key of cell (row r of the panel, column t): max(d2, +0).
template <bool TRANS>
__device__ inline float cell_key(const float* Gs, int GW, int m, int r, int t, float n_own, float n_inner) {
  float dot = 0.0f;
  for (int u = 0; u < m; ++u) dot = dot + Gs[(r + u) * GW + t + u];
  // canonical: (N_query - 2*dot) + N_reference
  const float d2 = TRANS ? (n_inner - 2.0f * dot) + n_own : (n_own - 2.0f * dot) + n_inner;
  return d2 > 0.0f ? d2 : 0.0f;
}

__host__ __device__ inline size_t panel_lds_floats(int R, int m) {
  const int GR = R + m - 1, GW = kPanelW + m - 1;
  return align_up((size_t)GR * 12, 4) + align_up((size_t)GW * 13, 4) + (size_t)GR * GW;
}

// --------------------------------------------------------------------------------------
// Block-wide radix select on non-negative float keys held in LDS.
// --------------------------------------------------------------------------------------
struct SelScratch {
  int* hist;  // >= 2048 ints
  int* sh;    // >= 16 ints
};

// Exclusive scan of one int per thread over a 256-thread block; returns the total in *tot.
__device__ inline int block_excl_scan256(int v, int* sh, int* tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan(v);
  if (lane == 63) sh[8 + w] = inc;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int wq = sh[8 + q];
    before += (q < w) ? wq : 0;
    all += wq;
  }
  *tot = all;
  return before + inc - v;
}

// Key of rank k (0-based) among keys[0..n); *eq = multiplicity of that key, *less = #keys below.
__device__ inline unsigned block_select_rank(const unsigned* keys, int n, int k, SelScratch S, int* eq, int* less) {
  unsigned prefix = 0;
  const int k0 = k;
  int eqc = 0;
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
    const int bits = pass == 0 ? 11 : 10;
    const int nb = 1 << bits;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) S.hist[i] = 0;
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
      const unsigned key = keys[e];
      if ((key >> (shift + bits)) == prefix) atomicAdd(&S.hist[(key >> shift) & (nb - 1)], 1);
    }
    __syncthreads();
    const int per = nb / 256;  // 8 or 4 bins per thread
    const int base = threadIdx.x * per;
    int part = 0;
    for (int i = 0; i < per; ++i) part += S.hist[base + i];
    int tot;
    const int before = block_excl_scan256(part, S.sh, &tot);
    if (k >= before && k < before + part) {
      int acc = before;
      for (int i = 0; i < per; ++i) {
        const int h = S.hist[base + i];
        if (k < acc + h) {
          S.sh[0] = base + i;
          S.sh[1] = k - acc;
          S.sh[2] = h;
          break;
        }
        acc += h;
      }
    }
    __syncthreads();
    prefix = (prefix << bits) | (unsigned)S.sh[0];
    k = S.sh[1];
    eqc = S.sh[2];
    __syncthreads();
  }
  *eq = eqc;
  *less = k0 - k;
  return prefix;
}

// Smallest key strictly greater than v (0xffffffff if none).
__device__ inline unsigned block_min_greater(const unsigned* keys, int n, unsigned v, int* sh) {
  unsigned mn = 0xffffffffu;
  for (int e = threadIdx.x; e < n; e += blockDim.x) {
    const unsigned key = keys[e];
    if (key > v && key < mn) mn = key;
  }
  mn = wave_min_u32(mn);
  if ((threadIdx.x & 63) == 0) sh[4 + (threadIdx.x >> 6)] = (int)mn;
  __syncthreads();
  unsigned r = 0xffffffffu;
  for (int q = 0; q < 4; ++q) r = min(r, (unsigned)sh[4 + q]);
  __syncthreads();
  return r;
}

// essentia percentile of the n keys (squared distances) in D units + the squared-domain
// threshold. Written by thread 0.
__device__ inline void block_percentile(const unsigned* keys, int n, float kappa, SelScratch S, float* thr_out,
                                        float* T_out) {
  const float q = (float)(n - 1) * kappa;
  const float lo_f = floorf(q), hi_f = ceilf(q);
  const int lo = (int)lo_f, hi = (int)hi_f;
  int eq, less;
  const unsigned vlo = block_select_rank(keys, n, lo, S, &eq, &less);
  unsigned vhi = vlo;
  if (hi != lo && less + eq <= hi) vhi = block_min_greater(keys, n, vlo, S.sh);
  if (threadIdx.x == 0) {
    const float slo = sqrt_rn(__builtin_bit_cast(float, vlo));
    float thr;
    if (lo_f == hi_f) {
      thr = slo;
    } else {
      const float shi = sqrt_rn(__builtin_bit_cast(float, vhi));
      const float a = slo * (hi_f - q);
      const float b = shi * (q - lo_f);
      thr = a + b;
    }
    *thr_out = thr;
    *T_out = sq_threshold(thr);
  }
  __syncthreads();
}

// --------------------------------------------------------------------------------------
// k_crp_select<TRANS>: per (stripe of R own frames, pair) -> thresholds of those rows
// (TRANS=false: rows of the CRP / query frames) or columns (TRANS=true: reference frames).
// Dynamic LDS: Dst[R][ld] keys | panel buffers. Hist aliases the Ys|Gs panel region.
// --------------------------------------------------------------------------------------

template <bool TRANS>
__global__ __launch_bounds__(256) void k_crp_select(CrpBatch B, int R, int ld, float kappa, float* __restrict__ thr,
                                                    float* __restrict__ Tq, int64_t thr_stride) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int p = blockIdx.y;
  const int2 dm = B.dims[p];
  const int n_own_s = TRANS ? dm.y : dm.x, n_in_s = TRANS ? dm.x : dm.y;
  const int i0 = blockIdx.x * R;
  if (i0 >= n_own_s || n_in_s <= 0) return;
  const int ta = B.pairs[2 * p], tb = B.pairs[2 * p + 1];
  const int t_own = TRANS ? tb : ta, t_in = TRANS ? ta : tb;
  const int k = B.oti[p];
  PanelArgs A;
  A.own = B.feats + B.off[t_own] * 12;
  A.inner = B.feats + B.off[t_in] * 12;
  A.k_own = TRANS ? k : 0;
  A.k_inner = TRANS ? 0 : k;
  A.n_own = B.len[t_own];
  A.n_inner = B.len[t_in];
  A.m = B.m;
  A.tau = B.tau;
  const int m = B.m, GR = R + m - 1, GW = kPanelW + m - 1;
  float* Dst = smem;
  float* Xs = Dst + (size_t)R * ld;
  float* Ys = Xs + align_up((size_t)GR * 12, 4);
  float* Gs = Ys + align_up((size_t)GW * 13, 4);
  const float* NXown = B.NX + (size_t)t_own * B.ldn;
  const float* NXin = B.NX + (size_t)t_in * B.ldn;
  const int rows = min(R, n_own_s - i0);
  float nown[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) nown[r] = (r < rows) ? NXown[i0 + r] : 0.0f;

  stage_own(A, i0, GR, Xs);
  for (int j0 = 0; j0 < n_in_s; j0 += kPanelW) {
    panel_gram(A, j0, GR, GW, Xs, Ys, Gs);
    const int t = threadIdx.x, j = j0 + t;
    if (j < n_in_s) {
      const float nin = NXin[j];
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (r < rows) Dst[(size_t)r * ld + j] = cell_key<TRANS>(Gs, GW, m, r, t, nown[r], nin);
    }
    __syncthreads();
  }
  SelScratch S;
  S.hist = reinterpret_cast<int*>(Ys);
  S.sh = S.hist + 2048;
  for (int r = 0; r < rows; ++r) {
    block_percentile(reinterpret_cast<const unsigned*>(Dst + (size_t)r * ld), n_in_s, kappa, S,
                     thr + (size_t)p * thr_stride + i0 + r, Tq + (size_t)p * thr_stride + i0 + r);
  }
}

__host__ inline size_t select_lds_bytes(int R, int m, int ld) {
  return ((size_t)R * ld + panel_lds_floats(R, m)) * sizeof(float);
}

// --------------------------------------------------------------------------------------
// k_crp_panel<MODE>: 32 query rows (one strip) x 256 reference columns.
// MODE 0: CRP bits -> maskT[p][strip][j] (bit r = row 32*strip + r). MODE 1: dist (sqrt).
// --------------------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_crp_panel(CrpBatch B, const float* __restrict__ Trow,
                                                   const float* __restrict__ Tcol, int64_t thr_stride,
                                                   uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                   float* __restrict__ dist) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int R = 32;
  const int p = blockIdx.z;
  const int2 dm = B.dims[p];
  const int strip = blockIdx.y;
  const int i0 = strip * R, j0 = blockIdx.x * kPanelW;
  if (i0 >= dm.x || j0 >= dm.y) return;
  const int ta = B.pairs[2 * p], tb = B.pairs[2 * p + 1];
  PanelArgs A;
  A.own = B.feats + B.off[ta] * 12;
  A.inner = B.feats + B.off[tb] * 12;
  A.k_own = 0;
  A.k_inner = B.oti[p];
  A.n_own = B.len[ta];
  A.n_inner = B.len[tb];
  A.m = B.m;
  A.tau = B.tau;
  const int m = B.m, GR = R + m - 1, GW = kPanelW + m - 1;
  float* Xs = smem;
  float* Ys = Xs + align_up((size_t)GR * 12, 4);
  float* Gs = Ys + align_up((size_t)GW * 13, 4);
  const float* NXq = B.NX + (size_t)ta * B.ldn;
  const float* NXr = B.NX + (size_t)tb * B.ldn;
  stage_own(A, i0, GR, Xs);
  panel_gram(A, j0, GR, GW, Xs, Ys, Gs);
  const int t = threadIdx.x, j = j0 + t;
  if (j >= dm.y) return;
  const int rows = min(R, dm.x - i0);
  const float nin = NXr[j];
  if (MODE == 0) {
    const float tc = Tcol[(size_t)p * thr_stride + j];
    const float* tr = Trow + (size_t)p * thr_stride + i0;
    uint32_t bits = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (r < rows) {
        const float key = cell_key<false>(Gs, GW, m, r, t, NXq[i0 + r], nin);
        bits |= (uint32_t)((key <= tr[r]) & (key <= tc)) << r;
      }
    }
    maskT[(size_t)p * mask_stride + (size_t)strip * ld + j] = bits;
  } else {
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      const float key = cell_key<false>(Gs, GW, m, r, t, NXq[i0 + r], nin);
      dist[(size_t)(i0 + r) * dm.y + j] = sqrt_rn(key);
    }
  }
}

// Dense (M x N) uint8 CRP <-> strip words maskT[i/32][j] (bit i%32).
__global__ void k_unpack_mask(const uint32_t* __restrict__ maskT, int ld, int M, int N, uint8_t* __restrict__ C) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (j >= N || i >= M) return;
  C[(size_t)i * N + j] = (uint8_t)((maskT[(size_t)(i >> 5) * ld + j] >> (i & 31)) & 1u);
}

__global__ void k_pack_mask(const uint8_t* __restrict__ C, int M, int N, int ld, uint32_t* __restrict__ maskT,
                            int* __restrict__ err) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int strip = blockIdx.y;
  if (j >= N) return;
  uint32_t w = 0;
  int bad = 0;
  for (int r = 0; r < 32; ++r) {
    const int i = strip * 32 + r;
    if (i < M) {
      const uint8_t v = C[(size_t)i * N + j];
      bad |= v > 1;
      w |= (uint32_t)(v & 1) << r;
    }
  }
  maskT[(size_t)strip * ld + j] = w;
  if (bad) atomicOr(err, 1);
}

// --------------------------------------------------------------------------------------
// Host orchestration
// --------------------------------------------------------------------------------------
namespace {

// The workspace slots of this file (the other files number their own).
enum CrpSlot {
  SLOT_TRACKS = 0,  // run_prep: the per-track tables of one call (TrackPrep)
  SLOT_PLAN = 1,    // crp_plan: the per-pair tables of a DP batch and the key planes of its sub-batches
  // acoss_crp_pair: the pair as a corpus of two tracks and a batch of one pair: packed features and
  // the tables a caller of acoss_crp_align passes in
  SLOT_PAIR = 2,
  SLOT_ALIGN_CRP = 3,  // acoss_align_crp: the packed matrix (MatrixView) and the DP's band boundaries
  // band-boundary records of the tracing DP, in a slot of their own (crp_plan's carving is the
  // shipped DP's): acoss_crp_locate per pair of a DP batch, acoss_locate_crp after its MatrixView
  SLOT_LOCATE = 22, SLOT_LOCATE_CRP = 23,
  // the direction DP's plane, band-boundary records and end keys, likewise: acoss_crp_path, acoss_path_crp
  SLOT_PATH = 24, SLOT_PATH_CRP = 25,
  // the line walk's band-boundary records, likewise: acoss_crp_rqa; acoss_rqa_crp after its MatrixView,
  // followed by the Smax DP's
  SLOT_RQA = 29, SLOT_RQA_CRP = 30,
  // ranked OTI (OtiWs): the pick flag, the orders of a DP batch and the best-of rows; acoss_oti_ranked: the profiles
  SLOT_OTI = 32,
};

// Every driver below takes the wide params; the entries without a 2 widen theirs (binarize = 0).
// Returns NULL for NULL, which check_params then refuses.
const acoss_crp_params2* widen(const acoss_crp_params* P, acoss_crp_params2& W) {
  if (!P) return nullptr;
  W = acoss_crp_params2{*P, ACOSS_BIN_PERCENTILE, 1};
  return &W;
}

bool otib(const acoss_crp_params2* P2) { return P2->binarize == ACOSS_BIN_OTI; }

int check_params(const acoss_crp_params2* P2) {
  if (!P2) {
    set_error("params is NULL");
    return ACOSS_E_ARG;
  }
  const acoss_crp_params* P = &P2->base;
  if (P2->binarize != ACOSS_BIN_PERCENTILE && P2->binarize != ACOSS_BIN_OTI) {
    set_error("unknown binarize %d (ACOSS_BIN_PERCENTILE = 0, ACOSS_BIN_OTI = 1)", P2->binarize);
    return ACOSS_E_ARG;
  }
  // kappa is not read under ACOSS_BIN_OTI
  if (P->m < 1 || P->m > 64 || P->tau < 1 || (!otib(P2) && !(P->kappa >= 0.0f && P->kappa <= 1.0f))) {
    set_error("unsupported params m=%d tau=%d kappa=%g", P->m, P->tau, (double)P->kappa);
    return ACOSS_E_ARG;
  }
  if (otib(P2) && (P2->oti_rank < 1 || P2->oti_rank > 12)) {
    set_error("oti_rank %d outside 1 .. 12", P2->oti_rank);
    return ACOSS_E_ARG;
  }
  return ACOSS_OK;
}

// Which transposition of the ranked OTI a call applies (include/acoss_hip.h, acoss_crp_params3): best of
// n_oti (acoss_crp_align3), else the scalar pick or the plane picks. The entries without a 3 pass {1, 0, NULL}.
struct OtiSel {
  int n_oti, pick;
  const int32_t* picks;  // device, one per pair of the call; NULL: pick for every pair
  bool ranked() const { return n_oti > 1 || pick != 0 || picks; }
};

const OtiSel kOtiFirst{1, 0, nullptr};

OtiSel oti_sel(const acoss_crp_params3* P3, const int32_t* picks) {
  return P3 ? OtiSel{P3->n_oti, P3->oti_pick, picks} : kOtiFirst;
}

// best_of: acoss_crp_align3, the one entry that reads n_oti and takes no pick.
int check_oti(const acoss_crp_params2* P2, const OtiSel& S, bool best_of) {
  if (S.n_oti < 1 || S.n_oti > 12) {
    set_error("n_oti %d outside 1 .. 12", S.n_oti);
    return ACOSS_E_ARG;
  }
  if (S.pick < 0 || S.pick > 11) {
    set_error("oti_pick %d outside 0 .. 11", S.pick);
    return ACOSS_E_ARG;
  }
  if (!best_of && S.n_oti != 1) {
    set_error("n_oti %d: only acoss_crp_align3 folds several transpositions, this entry requires 1", S.n_oti);
    return ACOSS_E_ARG;
  }
  if (best_of && S.pick != 0) {
    set_error("oti_pick %d: acoss_crp_align3 runs picks 0 .. n_oti - 1 and requires 0", S.pick);
    return ACOSS_E_ARG;
  }
  if (!P2->base.oti && S.ranked()) {
    set_error("oti = 0 has no ranking: n_oti > 1, a nonzero oti_pick and a pick plane need oti = 1");
    return ACOSS_E_ARG;
  }
  return ACOSS_OK;
}

// The ranked-OTI tables of one DP batch, in workspace slot SLOT_OTI.
struct OtiWs {
  int* err;          // raised by k_pair_oti at a pick outside 0 .. 11
  int32_t* order;    // k_oti_rank's, 12 per pair; NULL: no ranking, k_pair_oti makes the argmax itself
  float* row[2];     // best of n: the scores of the current round, by launch_dp's align
  float* best[2];    // and the best so far
};

int oti_ws(int64_t nb, hipStream_t s, OtiWs& W) {
  const size_t ob = align_up(48 * (size_t)nb, 256), rb = align_up(4 * (size_t)nb, 256);
  char* ws = static_cast<char*>(workspace(SLOT_OTI, 256 + ob + 4 * rb));
  if (!ws) return ACOSS_E_HIP;
  W.err = reinterpret_cast<int*>(ws);
  W.order = reinterpret_cast<int32_t*>(ws + 256);
  for (int q = 0; q < 2; ++q) {
    W.row[q] = reinterpret_cast<float*>(ws + 256 + ob + q * rb);
    W.best[q] = reinterpret_cast<float*>(ws + 256 + ob + (2 + q) * rb);
  }
  ACOSS_HIP_CHECK(hipMemsetAsync(W.err, 0, 4, s));
  return ACOSS_OK;
}

// After the launches of a call with a pick plane: waits for them and refuses a plane k_pair_oti flagged.
int oti_finish(const OtiWs& W, hipStream_t s) {
  int h_err = 0;
  ACOSS_HIP_CHECK(hipMemcpyAsync(&h_err, W.err, 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_err) {
    set_error("picks holds a value outside 0 .. 11");
    return ACOSS_E_ARG;
  }
  return ACOSS_OK;
}

int launch_oti_rank(const float* prof, const int32_t* pairs, int64_t n, int32_t* order, float* dots, hipStream_t s) {
  hipLaunchKernelGGL(k_oti_rank, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, prof, pairs, n, order, dots);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

// Largest R (<=16) whose select block fits: prefer two blocks per CU.
int pick_R(int m, int ld) {
  const size_t lds_max = 160 * 1024;
  for (int R = 16; R >= 1; --R)
    if (2 * select_lds_bytes(R, m, ld) <= lds_max) return R;
  for (int R = 16; R >= 1; --R)
    if (select_lds_bytes(R, m, ld) <= lds_max) return R;
  return 0;
}

template <typename K>
int set_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024)
    ACOSS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return ACOSS_OK;
}

// Per-track tables of one call, in workspace slot SLOT_TRACKS: prof (n_tracks x 12) | NX (n_tracks x ldn) |
// X2, the interleaved frame pairs of the split sweep (n_tracks x ldn x 24).
struct TrackPrep {
  const float* feats;
  const int64_t* off;
  const int32_t* len;
  float *prof, *NX, *X2;
  int ldn;
};

int run_prep(const float* feats, const int64_t* off, const int32_t* len, int n_tracks, int max_len, int m, int tau,
             hipStream_t s, TrackPrep* T) {
  // 32 spare frames per track: the systolic sweep's last (partial) strip reads query frames up
  // to 31 past the track's end (values unused: those rows are never stored)
  const int ldn = (int)align_up((size_t)max_len + 32, 64);
  const size_t base = align_up((size_t)n_tracks * 12 + (size_t)n_tracks * ldn, 64);
  float* ws = static_cast<float*>(workspace(SLOT_TRACKS, (base + (size_t)n_tracks * ldn * 24) * sizeof(float)));
  if (!ws) return ACOSS_E_HIP;
  *T = TrackPrep{feats, off, len, ws, ws + (size_t)n_tracks * 12, ws + base, ldn};
  if (max_len > 0) {
    hipLaunchKernelGGL(k_track_pairs, dim3(n_tracks, (max_len + 255) / 256), dim3(256), 0, s, feats, off, len, ldn,
                       T->X2);
    ACOSS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_track_profile, dim3((n_tracks + 3) / 4), dim3(64), 0, s, feats, off, len, n_tracks, T->prof);
  ACOSS_LAUNCH_CHECK();
  if (max_len > 0) {
    hipLaunchKernelGGL(k_track_norms, dim3(n_tracks, (max_len + 255) / 256), dim3(256), 0, s, feats, off, len, m,
                       tau, ldn, T->NX);
    ACOSS_LAUNCH_CHECK();
  }
  return ACOSS_OK;
}

// What one CRP call derives from (m, tau, longest track, pairs): which of the two paths runs, the
// pitches its kernels index with, and workspace slot SLOT_PLAN carved to them. acoss_crp_align and
// acoss_crp_pair both get it from crp_plan and their thresholds and CRP words from crp_masks, so
// the single pair runs the batch's kernels on the batch's buffers (the read margins the split
// kernels rely on included).
struct CrpPlan {
  int m, tau, L, ld, nstrips;
  int64_t thr_stride, mask_stride, bnd_stride, yrot_stride;
  bool split;        // crp_split.hip (m = 9, tau = 1, lines <= 4096 codes); else the generic kernels
  int ldk;           // key planes: row pitch
  int64_t kstride;   // key planes: codes per pair and plane
  int64_t nb_alloc;  // pairs per DP batch
  int64_t sub;       // pairs per CRP sub-batch
  int nbuf;          // key-plane buffers = streams the sub-batches rotate over
  int R;             // generic select: own frames per block
  size_t sel_lds, pan_lds;
  // per pair of a DP batch: oti, dims, thr/T rows+cols, maskT, band boundary, rolled reference
  int32_t* oti;
  int2* dims;
  float *thr_r, *T_r, *thr_c, *T_c;
  uint32_t* mask;
  float4* bnd;
  float* yrot;
  void* kpl[3];     // per buffer: the key planes of a sub-batch
  uint32_t* rt[3];  // and its row-threshold words
  hipStream_t ss[3];
};

// otib: the plan of an OTI-binary call (crp_otib.hip makes the masks): no select stripe to fit, no
// split path and so no key planes.
int crp_plan(int m, int tau, int max_len, int64_t n_pairs, bool otib, hipStream_t s, CrpPlan& P) {
  const int L = stacked_len(max_len, m, tau);
  if (L <= 0) {
    set_error("max_len %d too short for m=%d tau=%d", max_len, m, tau);
    return ACOSS_E_SHAPE;
  }
  P.m = m;
  P.tau = tau;
  P.L = L;
  const int ld = P.ld = (int)align_up((size_t)L, 8);  // x16 B = 128 B: band rows never share a cache line
  P.R = otib ? 1 : pick_R(m, ld);
  if (P.R <= 0) {
    set_error("track too long for the LDS stripe (stacked length %d)", ld);
    return ACOSS_E_SHAPE;
  }
  P.sel_lds = select_lds_bytes(P.R, m, ld);
  P.pan_lds = panel_lds_floats(32, m) * sizeof(float);
  int rc;
  if (!otib) {
    if ((rc = set_lds(k_crp_select<false>, P.sel_lds))) return rc;
    if ((rc = set_lds(k_crp_select<true>, P.sel_lds))) return rc;
  }
  if ((rc = set_lds(k_crp_panel<0>, P.pan_lds))) return rc;
  if ((rc = set_lds(k_crp_panel<1>, P.pan_lds))) return rc;
  P.nstrips = (L + 31) / 32;
  P.thr_stride = ld;
  P.mask_stride = (int64_t)P.nstrips * ld;
  P.bnd_stride = (int64_t)((L + 2047) / 2048) * ld;
  P.yrot_stride = (int64_t)align_up((size_t)max_len * 12, 64);
  // split path (one sweep + two line-select kernels, crp_split.hip) needs 16-bit key planes;
  // ACOSS_CRP_PATH=generic keeps a shape it covers on the generic kernels
  static const char* path_env = getenv("ACOSS_CRP_PATH");
  P.split = !otib && m == 9 && tau == 1 && L <= 4096 && !(path_env && strcmp(path_env, "generic") == 0);
  // row pitch: the selects' 32-element runs end at align32(L); one pad column beyond them takes
  // the sweep's branchless out-of-range stores
  P.ldk = (int)align_up(align_up((size_t)L, 32) + 1, 64);
  P.kstride = P.split ? (int64_t)align_up((size_t)L, 32) * P.ldk : 0;  // whole 32-row strips
  // Two-level batching: a DP batch of nb_alloc pairs keeps its CRP words (0.5 MB per pair at
  // 2000 frames) so the one-wave-per-pair DP launch is wide enough; the CRP itself runs in
  // sub-batches whose 16-bit key planes (split path, 16 MB per pair) stay near the 256 MB
  // Infinity Cache.
  const size_t slot = 4 + 8 + 4 * (size_t)P.thr_stride * 4 + 4 * (size_t)P.mask_stride + 16 * (size_t)P.bnd_stride +
                      4 * (size_t)P.yrot_stride;
  size_t budget = (size_t)16 << 30;  // DP batch scratch: ~25k pairs at 2000 frames in one DP launch
  if (const char* e = getenv("ACOSS_WS_BYTES")) budget = strtoull(e, nullptr, 10);
  int64_t nbmax = (int64_t)(budget / slot);
  if (const char* e = getenv("ACOSS_BATCH_PAIRS")) nbmax = atoll(e);
  if (nbmax < 1) nbmax = 1;
  if (nbmax > 65535) nbmax = 65535;
  const int64_t nb_alloc = P.nb_alloc = n_pairs < nbmax ? n_pairs : nbmax;
  P.sub = nb_alloc;
  // split sub-batch scratch per pair: 16-bit prefixes row-major and strip-major (2 + 2 B per
  // cell) and the row-threshold words RT
  const size_t sub_pair = 4 * (size_t)P.kstride + 4 * (size_t)P.mask_stride;
  if (P.split) {
    size_t kbudget = (size_t)1 << 30;  // ~42 pairs at 2000 frames (x2 buffers): fills 256 CUs per launch
    if (const char* e = getenv("ACOSS_KEY_BYTES")) kbudget = strtoull(e, nullptr, 10);
    P.sub = (int64_t)(kbudget / sub_pair);
    if (P.sub < 1) P.sub = 1;
    if (P.sub > nb_alloc) P.sub = nb_alloc;
  }
  // split sub-batches alternate between the caller's stream and a side stream, each with its
  // own key-plane buffer, so one sub-batch's selects overlap the next one's sweep
  // read per call: bench.py takes its per-kernel profile with ACOSS_SPLIT_STREAMS=1, so the
  // kernel durations of that call add up to its wall time
  const char* e = getenv("ACOSS_SPLIT_STREAMS");
  const int v = e ? atoi(e) : 2;
  P.nbuf = !P.split ? 0 : (v < 1 ? 1 : (v > 3 ? 3 : v));
  char* ws = static_cast<char*>(workspace(SLOT_PLAN, slot * nb_alloc + P.nbuf * sub_pair * P.sub + 8192));
  if (!ws) return ACOSS_E_HIP;
  size_t o = 0;
  auto carve = [&](size_t bytes) {
    void* r = ws + o;
    o = align_up(o + bytes, 256);
    return r;
  };
  P.oti = static_cast<int32_t*>(carve(4 * nb_alloc));
  P.dims = static_cast<int2*>(carve(8 * nb_alloc));
  P.thr_r = static_cast<float*>(carve(4 * P.thr_stride * nb_alloc));
  P.T_r = static_cast<float*>(carve(4 * P.thr_stride * nb_alloc));
  P.thr_c = static_cast<float*>(carve(4 * P.thr_stride * nb_alloc));
  P.T_c = static_cast<float*>(carve(4 * P.thr_stride * nb_alloc));
  P.mask = static_cast<uint32_t*>(carve(4 * P.mask_stride * nb_alloc));
  P.bnd = static_cast<float4*>(carve(16 * P.bnd_stride * nb_alloc));
  P.yrot = static_cast<float*>(carve(4 * P.yrot_stride * nb_alloc));
  for (int b = 0; b < P.nbuf; ++b) {  // buffer 0 on the caller's stream, the others on side streams
    P.kpl[b] = carve(4 * (size_t)P.kstride * P.sub);
    P.rt[b] = static_cast<uint32_t*>(carve(4 * (size_t)P.mask_stride * P.sub));
    P.ss[b] = b == 0 ? s : side_stream(b - 1);
    if (b > 0 && !P.ss[b]) {
      set_error("could not create the side stream");
      return ACOSS_E_HIP;
    }
  }
  return ACOSS_OK;
}

// Pairs [s0, ...) of the DP batch whose pairs start at pb, on C's tables.
CrpBatch batch_view(const CrpPlan& C, const TrackPrep& T, const int32_t* pb, int s0) {
  return CrpBatch{T.feats, T.X2, T.off, T.len, T.NX, T.ldn, pb + 2 * s0, C.oti + s0, C.dims + s0, C.m, C.tau,
                  C.yrot + (size_t)s0 * C.yrot_stride, C.yrot_stride};
}

// One DP batch (nb <= C.nb_alloc pairs at pb) up to its CRP: OTI, rolled references, row and
// column thresholds (thr_*, T_*) and the mask words, on stream s. The one place that chooses
// between the split path, the generic kernels and, under ACOSS_BIN_OTI, the OTI-binary kernel, which
// needs neither the rolled references nor thresholds (thr_*, T_* are then not written). With W.order
// the OTI is the pairs' pick of it: the scalar, or picks (already offset to the batch) where given.
int crp_masks(const CrpPlan& C, const TrackPrep& T, const int32_t* pb, int nb, const acoss_crp_params2* params2,
              const OtiWs& W, int pick, const int32_t* picks, hipStream_t s) {
  int rc;
  const acoss_crp_params* params = &params2->base;
  prof_begin(PH_OTI, s);
  hipLaunchKernelGGL(k_pair_oti, dim3((nb + 255) / 256), dim3(256), 0, s, T.prof, T.len, pb, (int64_t)nb, params->oti,
                     C.m, C.tau, W.order, pick, picks, W.err, C.oti, C.dims);
  ACOSS_LAUNCH_CHECK();
  if (otib(params2)) {
    prof_end(PH_OTI, s);
    prof_begin(PH_MASK, s);
    if ((rc = launch_otib(batch_view(C, T, pb, 0), nb, C.L, params2->oti_rank, C.mask, C.mask_stride, C.ld, s)))
      return rc;
    prof_end(PH_MASK, s);
    return ACOSS_OK;
  }
  hipLaunchKernelGGL(k_rotate_ref, dim3(16, nb), dim3(256), 0, s, T.feats, T.off, T.len, pb, C.oti, C.yrot,
                     C.yrot_stride);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_OTI, s);
  if (!C.split) {
    const CrpBatch B = batch_view(C, T, pb, 0);
    const dim3 sel_grid((C.L + C.R - 1) / C.R, nb);
    prof_begin(PH_SEL_ROWS, s);
    hipLaunchKernelGGL(k_crp_select<false>, sel_grid, dim3(256), C.sel_lds, s, B, C.R, C.ld, params->kappa,
                       C.thr_r, C.T_r, C.thr_stride);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_SEL_ROWS, s);
    prof_begin(PH_SEL_COLS, s);
    hipLaunchKernelGGL(k_crp_select<true>, sel_grid, dim3(256), C.sel_lds, s, B, C.R, C.ld, params->kappa,
                       C.thr_c, C.T_c, C.thr_stride);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_SEL_COLS, s);
    prof_begin(PH_MASK, s);
    hipLaunchKernelGGL(k_crp_panel<0>, dim3((C.L + kPanelW - 1) / kPanelW, C.nstrips, nb), dim3(256), C.pan_lds, s,
                       B, C.T_r, C.T_c, C.thr_stride, C.mask, C.mask_stride, C.ld, (float*)nullptr);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_MASK, s);
    return ACOSS_OK;
  }
  const int nsb = (int)((nb + C.sub - 1) / C.sub);  // sub-batches of this batch
  const int nst = C.nbuf < nsb ? C.nbuf : nsb;      // streams they rotate over
  if (nst > 1) {  // the side streams start after this batch's OTI / roll on the caller's stream
    hipEvent_t e0 = sync_event(0);
    ACOSS_HIP_CHECK(hipEventRecord(e0, s));
    for (int q = 1; q < nst; ++q) ACOSS_HIP_CHECK(hipStreamWaitEvent(C.ss[q], e0, 0));
  }
  int k = 0;
  for (int s0 = 0; s0 < nb; s0 += (int)C.sub, ++k) {
    const int ns = (nb - s0) < C.sub ? (nb - s0) : (int)C.sub;
    const int b = k % nst;
    const size_t to = (size_t)s0 * C.thr_stride;
    if ((rc = launch_crp_split(batch_view(C, T, pb, s0), ns, C.L, params->kappa, C.kpl[b], C.ldk, C.kstride, C.rt[b],
                               C.thr_r + to, C.T_r + to, C.thr_c + to, C.T_c + to, C.thr_stride,
                               C.mask + (size_t)s0 * C.mask_stride, C.mask_stride, C.ld, C.ss[b])))
      return rc;
  }
  for (int q = 1; q < nst; ++q) {  // the caller's stream needs every sub-batch of every stream
    hipEvent_t e1 = sync_event(q);
    ACOSS_HIP_CHECK(hipEventRecord(e1, C.ss[q]));
    ACOSS_HIP_CHECK(hipStreamWaitEvent(s, e1, 0));
  }
  return ACOSS_OK;
}

// A packed cell of the tracing and direction DPs has 16 bits per coordinate: the longest stacked
// length of a batch (N < 0) or the M x N of a given matrix.
int check_cell_bits(int M, int N = -1) {
  if (M <= kTraceMaxLen && N <= kTraceMaxLen) return ACOSS_OK;
  if (N < 0)
    set_error("stacked length %d above %d: a packed cell has 16 bits per coordinate", M, kTraceMaxLen);
  else
    set_error("matrix %d x %d above %d rows or columns: a packed cell has 16 bits per coordinate", M, N, kTraceMaxLen);
  return ACOSS_E_SHAPE;
}

const auto no_hook = [](auto&&...) { return ACOSS_OK; };

// The batch driver under acoss_crp_align, acoss_crp_locate and acoss_crp_path: the checks the three
// share, the plan, the per-track preparation, then DP batch after DP batch: crp_masks, the entry's
// DP, the OTI copy.
//   check()          the entry's own argument checks, after the shared ones (so an empty pair list
//                    is answered first) and before anything is allocated;
//   setup(C, nbd)    once the plan is known: the entry sizes and fetches its own workspace slot
//                    and may lower the DP batch nbd below C.nb_alloc;
//   dp(C, base, nb, r, W)  launches the entry's DP for pairs [base, base + nb) under its own phases;
//                    r is the round of a best of n (0 elsewhere), W the batch's ranked-OTI tables.
// Under a ranked OTI (sel.ranked()) a batch first makes its orders, then runs crp_masks and dp once
// per round r < sel.n_oti at pick r (at the entry's pick when n_oti is 1). best_of: the entry is
// acoss_crp_align3, which alone may ask for n_oti > 1.
template <class Check, class Setup, class Dp>
int crp_batches(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params2,
                const OtiSel& sel, bool best_of, hipStream_t s, int32_t* oti_out, Check check, Setup setup, Dp dp) {
  int rc = check_params(params2);
  if (rc) return rc;
  if ((rc = check_oti(params2, sel, best_of))) return rc;
  const acoss_crp_params* params = &params2->base;
  if (n_pairs < 0 || n_tracks < 0 || max_len < 0) {
    set_error("negative size");
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  if (!feats || !track_off || !track_len || !pairs) {
    set_error("NULL input pointer");
    return ACOSS_E_ARG;
  }
  if ((rc = check())) return rc;
  CrpPlan C;
  if ((rc = crp_plan(params->m, params->tau, max_len, n_pairs, otib(params2), s, C))) return rc;
  TrackPrep T;
  prof_begin(PH_PREP, s);
  if ((rc = run_prep(feats, track_off, track_len, n_tracks, max_len, C.m, C.tau, s, &T))) return rc;
  prof_end(PH_PREP, s);
  int64_t nbd = C.nb_alloc;
  if ((rc = setup(C, nbd))) return rc;
  OtiWs W{};
  if (sel.ranked() && (rc = oti_ws(nbd, s, W))) return rc;
  for (int64_t base = 0; base < n_pairs; base += nbd) {
    const int nb = (int)((n_pairs - base) < nbd ? (n_pairs - base) : nbd);
    const int32_t* pb = pairs + 2 * base;
    if (W.order) {
      prof_begin(PH_OTI, s);
      if ((rc = launch_oti_rank(T.prof, pb, nb, W.order, nullptr, s))) return rc;
      prof_end(PH_OTI, s);
    }
    for (int r = 0; r < sel.n_oti; ++r) {
      if ((rc = crp_masks(C, T, pb, nb, params2, W, best_of ? r : sel.pick, sel.picks ? sel.picks + base : nullptr, s)))
        return rc;
      if ((rc = dp(C, base, nb, r, W))) return rc;
    }
    if (oti_out) ACOSS_HIP_CHECK(hipMemcpyAsync(oti_out + base, C.oti, 4 * nb, hipMemcpyDeviceToDevice, s));
  }
  return sel.picks ? oti_finish(W, s) : ACOSS_OK;
}

// The direction plane of one DP batch stays under this many bytes (acoss_crp_path shrinks its DP
// batch below crp_plan's where needed): 1 MB per pair at 2,000 frames still gives a launch of
// about 4,000 waves.
size_t path_plane_budget() {
  size_t budget = (size_t)4 << 30;
  if (const char* e = getenv("ACOSS_PATH_BYTES")) budget = strtoull(e, nullptr, 10);
  return budget;
}

// acoss_crp_path's DP batch: crp_plan's unless its planes (pstride bytes per pair) would pass the
// budget, and then batches of equal size: a last batch of a few pairs would be a launch that fills
// no GPU.
int64_t path_dp_batch(int64_t n_pairs, int64_t nb_alloc, int64_t pstride, size_t budget) {
  int64_t nbp = (int64_t)(budget / (size_t)pstride);
  if (nbp < 1) nbp = 1;
  if (nbp > nb_alloc) nbp = nb_alloc;
  const int64_t nbatches = (n_pairs + nbp - 1) / nbp;
  return (n_pairs + nbatches - 1) / nbatches;
}

// A given M x N matrix as the DP takes it, in one workspace slot: the error flag at 0, the dims at
// 64, one spare word at 128 (the path's end key), the mask words from 256, then the regions the
// entry asked for, each aligned to 256 B.
struct MatrixView {
  int* d_err;
  int2* d_dims;
  uint32_t* d_end;
  uint32_t* maskT;
  int ld;
  char* region[2];
};

int matrix_pitch(int N) { return (int)align_up((size_t)N, 8); }

// Lays the slot out, uploads its header and packs crp into mask words (k_pack_mask raises the
// error flag at an element above 1) on stream s.
int pack_matrix(int slot, const uint8_t* crp, int M, int N, size_t bytes0, size_t bytes1, hipStream_t s,
                MatrixView& V) {
  const int ld = matrix_pitch(N);
  const int nstrips = (M + 31) / 32;
  const size_t mask_bytes = align_up(4 * (size_t)nstrips * ld, 256);
  bytes0 = align_up(bytes0, 256);
  char* ws = static_cast<char*>(workspace(slot, 256 + mask_bytes + bytes0 + align_up(bytes1, 256)));
  if (!ws) return ACOSS_E_HIP;
  V = MatrixView{reinterpret_cast<int*>(ws),
                 reinterpret_cast<int2*>(ws + 64),
                 reinterpret_cast<uint32_t*>(ws + 128),
                 reinterpret_cast<uint32_t*>(ws + 256),
                 ld,
                 {ws + 256 + mask_bytes, ws + 256 + mask_bytes + bytes0}};
  const int h_hdr[4] = {0, 0, M, N};  // err, pad, dims
  ACOSS_HIP_CHECK(hipMemcpy(V.d_err, h_hdr, 8, hipMemcpyHostToDevice));
  ACOSS_HIP_CHECK(hipMemcpy(V.d_dims, h_hdr + 2, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_pack_mask, dim3((N + 255) / 256, nstrips), dim3(256), 0, s, crp, M, N, ld, V.maskT, V.d_err);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

// After the entry's launches: waits for them and refuses a matrix that k_pack_mask flagged.
int matrix_finish(const MatrixView& V, hipStream_t s) {
  int h_err = 0;
  ACOSS_HIP_CHECK(hipMemcpyAsync(&h_err, V.d_err, 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_err) {
    set_error("CoverSongSimilarity: non-binary elements found in the input similarity matrix");
    return ACOSS_E_NONBINARY;
  }
  return ACOSS_OK;
}

// The answer for a matrix without rows or columns: score 0, no segment, an empty path (seg, len
// and path where the entry has them).
int empty_matrix_answer(float* score_out, int32_t* seg_out, int32_t* len_out, int32_t* path_out, int32_t path_cap,
                        hipStream_t s) {
  const float z = 0.0f;
  const int32_t none[4] = {-1, -1, -1, -1};
  const int32_t zero = 0;
  if (path_out && path_cap > 0) ACOSS_HIP_CHECK(hipMemsetAsync(path_out, 0xff, 8 * (size_t)path_cap, s));
  ACOSS_HIP_CHECK(hipMemcpyAsync(score_out, &z, 4, hipMemcpyHostToDevice, s));
  if (seg_out) ACOSS_HIP_CHECK(hipMemcpyAsync(seg_out, none, sizeof(none), hipMemcpyHostToDevice, s));
  if (len_out) ACOSS_HIP_CHECK(hipMemcpyAsync(len_out, &zero, 4, hipMemcpyHostToDevice, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  return ACOSS_OK;
}

}  // namespace

}  // namespace acoss

using namespace acoss;

// The bodies of the entries that make a CRP from chroma take the wide params (params2; params is
// its base, NULL with it and then refused before anything reads it); each serves the entry without
// a 2, which widens its params, and its twin.
namespace {

int crp_align_any(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                  int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params2,
                  float* qmax_out, float* dmax_out, int32_t* oti_out, void* hip_stream) {
  clear_error();
  const acoss_crp_params* params = params2 ? &params2->base : nullptr;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  float* const out[2] = {qmax_out, dmax_out};  // by launch_dp's align: 0 = Qmax, 1 = dmax
  const int phase[2] = {PH_DP_QMAX, PH_DP_DMAX};
  return crp_batches(
      feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params2, kOtiFirst, false, s, oti_out, no_hook,
      no_hook, [&](const CrpPlan& C, int64_t base, int nb, int, const OtiWs&) {
        for (int align = 0; align < 2; ++align) {
          if (!out[align]) continue;
          prof_begin(phase[align], s);
          launch_dp(align, params->gamma_open == params->gamma_ext, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims,
                    params->gamma_open, params->gamma_ext, C.bnd, C.bnd_stride, out[align] + base, s);
          ACOSS_LAUNCH_CHECK();
          prof_end(phase[align], s);
        }
        return ACOSS_OK;
      });
}

// acoss_crp_align3 at n_oti > 1: per round the DPs write the batch's scratch rows and k_oti_fold
// keeps the best; by launch_dp's align, out / oti / pick = {Qmax's, dmax's}.
int crp_align_best(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                   int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params3,
                   float* const (&out)[2], int32_t* const (&oti)[2], int32_t* const (&pick)[2], hipStream_t s) {
  const acoss_crp_params* params = &params3->base.base;
  const int phase[2] = {PH_DP_QMAX, PH_DP_DMAX};
  return crp_batches(
      feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, &params3->base, oti_sel(params3, nullptr), true,
      s, nullptr, no_hook, no_hook, [&](const CrpPlan& C, int64_t base, int nb, int r, const OtiWs& W) {
        for (int align = 0; align < 2; ++align) {
          if (!out[align] && !oti[align] && !pick[align]) continue;
          prof_begin(phase[align], s);
          launch_dp(align, params->gamma_open == params->gamma_ext, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims,
                    params->gamma_open, params->gamma_ext, C.bnd, C.bnd_stride, W.row[align], s);
          ACOSS_LAUNCH_CHECK();
          hipLaunchKernelGGL(k_oti_fold, dim3((nb + 255) / 256), dim3(256), 0, s, W.row[align], C.oti, r, nb,
                             W.best[align], out[align] ? out[align] + base : nullptr,
                             oti[align] ? oti[align] + base : nullptr, pick[align] ? pick[align] + base : nullptr);
          ACOSS_LAUNCH_CHECK();
          prof_end(phase[align], s);
        }
        return ACOSS_OK;
      });
}

int crp_pair_any(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params2* params2,
                 const OtiSel& sel, float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti,
                 uint8_t* closer_out, void* hip_stream) {
  clear_error();
  int rc = check_params(params2);
  if (rc) return rc;
  if ((rc = check_oti(params2, sel, false))) return rc;
  const acoss_crp_params* params = &params2->base;
  if (otib(params2) && (thr_row || thr_col)) {
    set_error("thr_row and thr_col must be NULL under ACOSS_BIN_OTI: it has no thresholds");
    return ACOSS_E_ARG;
  }
  if (!otib(params2) && closer_out) {
    set_error("closer_out must be NULL under ACOSS_BIN_PERCENTILE");
    return ACOSS_E_ARG;
  }
  const int m = params->m, tau = params->tau;
  const int Mp = stacked_len(M, m, tau), Np = stacked_len(N, m, tau);
  if (Mp <= 0 || Np <= 0) {
    set_error("track too short: M=%d N=%d m=%d tau=%d", M, N, m, tau);
    return ACOSS_E_SHAPE;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int max_len = M > N ? M : N;
  CrpPlan C;
  if ((rc = crp_plan(m, tau, max_len, 1, otib(params2), s, C))) return rc;
  const size_t fbytes = align_up((size_t)(M + N) * 12 * 4, 256);
  char* ws = static_cast<char*>(workspace(SLOT_PAIR, fbytes + 256));
  if (!ws) return ACOSS_E_HIP;
  float* f = reinterpret_cast<float*>(ws);
  char* tab = ws + fbytes;
  int64_t* d_off = reinterpret_cast<int64_t*>(tab);
  int32_t* d_len = reinterpret_cast<int32_t*>(tab + 64);
  int32_t* d_pairs = reinterpret_cast<int32_t*>(tab + 128);
  const int64_t h_off[2] = {0, M};
  const int32_t h_len[2] = {M, N};
  const int32_t h_pairs[2] = {0, 1};
  ACOSS_HIP_CHECK(hipMemcpyAsync(f, X, (size_t)M * 12 * 4, hipMemcpyDeviceToDevice, s));
  ACOSS_HIP_CHECK(hipMemcpyAsync(f + (size_t)M * 12, Y, (size_t)N * 12 * 4, hipMemcpyDeviceToDevice, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  ACOSS_HIP_CHECK(hipMemcpy(d_off, h_off, sizeof(h_off), hipMemcpyHostToDevice));
  ACOSS_HIP_CHECK(hipMemcpy(d_len, h_len, sizeof(h_len), hipMemcpyHostToDevice));
  ACOSS_HIP_CHECK(hipMemcpy(d_pairs, h_pairs, sizeof(h_pairs), hipMemcpyHostToDevice));
  TrackPrep T;
  if ((rc = run_prep(f, d_off, d_len, 2, max_len, m, tau, s, &T))) return rc;
  OtiWs W{};
  if (sel.ranked()) {
    if ((rc = oti_ws(1, s, W))) return rc;
    if ((rc = launch_oti_rank(T.prof, d_pairs, 1, W.order, nullptr, s))) return rc;
  }
  if ((rc = crp_masks(C, T, d_pairs, 1, params2, W, sel.pick, nullptr, s))) return rc;
  if (dist) {  // the roll is the pair's OTI, read from the track itself: under ACOSS_BIN_OTI this is D_0
    hipLaunchKernelGGL(k_crp_panel<1>, dim3((Np + kPanelW - 1) / kPanelW, C.nstrips, 1), dim3(256), C.pan_lds, s,
                       batch_view(C, T, d_pairs, 0), C.T_r, C.T_c, C.thr_stride, C.mask, C.mask_stride, C.ld, dist);
    ACOSS_LAUNCH_CHECK();
  }
  if (crp) {
    hipLaunchKernelGGL(k_unpack_mask, dim3((Np + 255) / 256, Mp), dim3(256), 0, s, C.mask, C.ld, Mp, Np, crp);
    ACOSS_LAUNCH_CHECK();
  }
  // after crp was unpacked from the batch kernel's words: the counting kernel writes them once more
  if (closer_out && (rc = launch_otib(batch_view(C, T, d_pairs, 0), 1, C.L, params2->oti_rank, C.mask, C.mask_stride,
                                      C.ld, s, closer_out)))
    return rc;
  if (thr_row) ACOSS_HIP_CHECK(hipMemcpyAsync(thr_row, C.thr_r, 4 * (size_t)Mp, hipMemcpyDeviceToDevice, s));
  if (thr_col) ACOSS_HIP_CHECK(hipMemcpyAsync(thr_col, C.thr_c, 4 * (size_t)Np, hipMemcpyDeviceToDevice, s));
  if (oti) ACOSS_HIP_CHECK(hipMemcpyAsync(oti, C.oti, 4, hipMemcpyDeviceToDevice, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  return ACOSS_OK;
}

}  // namespace

extern "C" int acoss_crp_align(const float* feats, const int64_t* track_off, const int32_t* track_len,
                               int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                               const acoss_crp_params* params, float* qmax_out, float* dmax_out, int32_t* oti_out,
                               void* hip_stream) {
  acoss_crp_params2 W;
  return crp_align_any(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, widen(params, W), qmax_out,
                       dmax_out, oti_out, hip_stream);
}

extern "C" int acoss_crp_align2(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                const acoss_crp_params2* params, float* qmax_out, float* dmax_out, int32_t* oti_out,
                                void* hip_stream) {
  return crp_align_any(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, qmax_out, dmax_out,
                       oti_out, hip_stream);
}

extern "C" int acoss_crp_pair(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params* params,
                              float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti,
                              void* hip_stream) {
  acoss_crp_params2 W;
  return crp_pair_any(X, M, Y, N, widen(params, W), kOtiFirst, dist, thr_row, thr_col, crp, oti, nullptr, hip_stream);
}

extern "C" int acoss_crp_pair2(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params2* params,
                               float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti,
                               uint8_t* closer_out, void* hip_stream) {
  return crp_pair_any(X, M, Y, N, params, kOtiFirst, dist, thr_row, thr_col, crp, oti, closer_out, hip_stream);
}

extern "C" int acoss_crp_pair3(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params3* params,
                               float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti,
                               uint8_t* closer_out, void* hip_stream) {
  return crp_pair_any(X, M, Y, N, params ? &params->base : nullptr, oti_sel(params, nullptr), dist, thr_row, thr_col,
                      crp, oti, closer_out, hip_stream);
}

extern "C" int acoss_crp_align3(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                const acoss_crp_params3* params, float* qmax_out, float* dmax_out, int32_t* oti_q_out,
                                int32_t* oti_d_out, int32_t* pick_q_out, int32_t* pick_d_out, void* hip_stream) {
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (params && (params->n_oti != 1 || params->oti_pick != 0)) {
    clear_error();
    float* const out[2] = {qmax_out, dmax_out};
    int32_t* const oti[2] = {oti_q_out, oti_d_out};
    int32_t* const pick[2] = {pick_q_out, pick_d_out};
    return crp_align_best(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, out, oti, pick, s);
  }
  // one transposition: acoss_crp_align2 itself, both winners its OTI at pick 0
  const int rc = crp_align_any(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs,
                               params ? &params->base : nullptr, qmax_out, dmax_out,
                               oti_q_out ? oti_q_out : oti_d_out, hip_stream);
  if (rc || n_pairs == 0) return rc;
  if (oti_q_out && oti_d_out)
    ACOSS_HIP_CHECK(hipMemcpyAsync(oti_d_out, oti_q_out, 4 * (size_t)n_pairs, hipMemcpyDeviceToDevice, s));
  if (pick_q_out) ACOSS_HIP_CHECK(hipMemsetAsync(pick_q_out, 0, 4 * (size_t)n_pairs, s));
  if (pick_d_out) ACOSS_HIP_CHECK(hipMemsetAsync(pick_d_out, 0, 4 * (size_t)n_pairs, s));
  return ACOSS_OK;
}

extern "C" int acoss_oti_ranked(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                int32_t n_tracks, const int32_t* pairs, int64_t n_pairs, int32_t* shifts_out,
                                float* dots_out, void* hip_stream) {
  clear_error();
  if (n_pairs < 0 || n_tracks < 0) {
    set_error("negative size");
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  if (!feats || !track_off || !track_len || !pairs || !shifts_out || n_tracks == 0) {
    set_error("NULL input pointer, no track or shifts_out is NULL");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  float* prof = static_cast<float*>(workspace(SLOT_OTI, 12 * sizeof(float) * (size_t)n_tracks));
  if (!prof) return ACOSS_E_HIP;
  hipLaunchKernelGGL(k_track_profile, dim3((n_tracks + 3) / 4), dim3(64), 0, s, feats, track_off, track_len, n_tracks,
                     prof);
  ACOSS_LAUNCH_CHECK();
  return launch_oti_rank(prof, pairs, n_pairs, shifts_out, dots_out, s);
}

extern "C" int acoss_align_crp(const uint8_t* crp, int32_t M, int32_t N, int32_t align, float gamma_open,
                               float gamma_ext, float* score_out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || (align != 0 && align != 1) || !score_out) {
    set_error("bad arguments to acoss_align_crp");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (M == 0 || N == 0) return empty_matrix_answer(score_out, nullptr, nullptr, nullptr, 0, s);
  int rc;
  MatrixView V;
  const size_t bnd_bytes = 16 * (size_t)((M + 2047) / 2048) * matrix_pitch(N);
  if ((rc = pack_matrix(SLOT_ALIGN_CRP, crp, M, N, bnd_bytes, 0, s, V))) return rc;
  launch_dp(align, gamma_open == gamma_ext, 1, M, V.maskT, 0, V.ld, V.d_dims, gamma_open, gamma_ext,
            reinterpret_cast<float4*>(V.region[0]), 0, score_out, s);
  ACOSS_LAUNCH_CHECK();
  return matrix_finish(V, s);
}

// Cross-recurrence quantification. The line measures come from one walk over the mask words
// (launch_rqa), Smax from the shipped Qmax DP at gamma_open = gamma_ext = +inf, where the miss
// branch max(mx - gamma, 0) is 0: launch_dp(align 0, eqg, ..., inf, inf), its general kernel.
namespace {

int check_rqa_args(const char* entry, int32_t lmin, int32_t hist_cap, const int32_t* hist_out) {
  if (lmin < 1) {
    set_error("%s: lmin %d below 1", entry, lmin);
    return ACOSS_E_ARG;
  }
  if (hist_cap < 0 || (hist_out && hist_cap == 0)) {
    set_error("%s: hist_out needs a positive hist_cap, not %d", entry, hist_cap);
    return ACOSS_E_ARG;
  }
  return ACOSS_OK;
}

int check_rqa_line(int longest) {
  if (longest <= kRqaMaxLine) return ACOSS_OK;
  set_error("a diagonal line may have %d cells, above the %d the LDS histogram takes", longest, kRqaMaxLine);
  return ACOSS_E_SHAPE;
}

int crp_rqa_any(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params2,
                const OtiSel& sel, int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, void* hip_stream) {
  clear_error();
  const acoss_crp_params* params = params2 ? &params2->base : nullptr;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const bool lines = counts_out || lmax_out || stats_out || hist_out;
  void* rb = nullptr;  // band-boundary records of the line walk, rstride per pair
  int64_t rstride = 0;
  return crp_batches(
      feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params2, sel, false, s, oti_out,
      [&] {
        if (int rc = check_rqa_args("acoss_crp_rqa", lmin, hist_cap, hist_out)) return rc;
        return lines ? check_rqa_line(stacked_len(max_len, params->m, params->tau)) : ACOSS_OK;
      },
      [&](const CrpPlan& C, int64_t& nbd) {
        rstride = rqa_bnd_records(C.L, C.ld);
        rb = workspace(SLOT_RQA, kRqaRecBytes * (size_t)rstride * (size_t)nbd);
        return rb ? ACOSS_OK : ACOSS_E_HIP;
      },
      [&](const CrpPlan& C, int64_t base, int nb, int, const OtiWs&) {
        if (lines) {
          prof_begin(PH_RQA, s);
          launch_rqa(nb, C.L, C.L + 1, C.mask, C.mask_stride, C.ld, C.dims, lmin, rb, rstride,
                     counts_out ? counts_out + 4 * base : nullptr, lmax_out ? lmax_out + base : nullptr,
                     stats_out ? stats_out + 4 * base : nullptr, hist_cap,
                     hist_out ? hist_out + (size_t)hist_cap * (size_t)base : nullptr, s);
          ACOSS_LAUNCH_CHECK();
          prof_end(PH_RQA, s);
        }
        if (smax_out) {
          prof_begin(PH_DP_QMAX, s);
          launch_dp(0, true, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims, __builtin_inff(), __builtin_inff(), C.bnd,
                    C.bnd_stride, smax_out + base, s);
          ACOSS_LAUNCH_CHECK();
          prof_end(PH_DP_QMAX, s);
        }
        return ACOSS_OK;
      });
}

}  // namespace

extern "C" int acoss_crp_rqa(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                             int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params* params,
                             int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                             int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, void* hip_stream) {
  acoss_crp_params2 W;
  return crp_rqa_any(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, widen(params, W), kOtiFirst, lmin,
                     counts_out, lmax_out, stats_out, smax_out, oti_out, hist_cap, hist_out, hip_stream);
}

extern "C" int acoss_crp_rqa2(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                              int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params,
                              int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                              int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, void* hip_stream) {
  return crp_rqa_any(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, kOtiFirst, lmin,
                     counts_out, lmax_out, stats_out, smax_out, oti_out, hist_cap, hist_out, hip_stream);
}

extern "C" int acoss_crp_rqa3(const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                              int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params3* params,
                              int32_t lmin, int64_t* counts_out, int32_t* lmax_out, double* stats_out, float* smax_out,
                              int32_t* oti_out, int32_t hist_cap, int32_t* hist_out, const int32_t* picks,
                              void* hip_stream) {
  return crp_rqa_any(feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params ? &params->base : nullptr,
                     oti_sel(params, picks), lmin, counts_out, lmax_out, stats_out, smax_out, oti_out, hist_cap,
                     hist_out, hip_stream);
}

extern "C" int acoss_rqa_crp(const uint8_t* crp, int32_t M, int32_t N, int32_t lmin, int64_t* counts_out,
                             int32_t* lmax_out, double* stats_out, float* smax_out, int32_t hist_cap,
                             int32_t* hist_out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0) {
    set_error("bad arguments to acoss_rqa_crp");
    return ACOSS_E_ARG;
  }
  int rc;
  if ((rc = check_rqa_args("acoss_rqa_crp", lmin, hist_cap, hist_out))) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const bool lines = counts_out || lmax_out || stats_out || hist_out;
  if (M == 0 || N == 0) {  // no cell, no line: every result is 0
    if (counts_out) ACOSS_HIP_CHECK(hipMemsetAsync(counts_out, 0, 4 * sizeof(int64_t), s));
    if (lmax_out) ACOSS_HIP_CHECK(hipMemsetAsync(lmax_out, 0, sizeof(int32_t), s));
    if (stats_out) ACOSS_HIP_CHECK(hipMemsetAsync(stats_out, 0, 4 * sizeof(double), s));
    if (smax_out) ACOSS_HIP_CHECK(hipMemsetAsync(smax_out, 0, sizeof(float), s));
    if (hist_out) ACOSS_HIP_CHECK(hipMemsetAsync(hist_out, 0, sizeof(int32_t) * (size_t)hist_cap, s));
    ACOSS_HIP_CHECK(hipStreamSynchronize(s));
    return ACOSS_OK;
  }
  if (lines) {
    if ((rc = check_rqa_line(M < N ? M : N))) return rc;
    if ((int64_t)M * N > (int64_t)INT32_MAX) {  // a bin of H is an int32, and a bin can hold half the cells' count
      set_error("matrix %d x %d has more than 2^31 - 1 cells: a histogram bin is an int32", M, N);
      return ACOSS_E_SHAPE;
    }
  }
  MatrixView V;
  const int ld = matrix_pitch(N);
  if ((rc = pack_matrix(SLOT_RQA_CRP, crp, M, N, kRqaRecBytes * (size_t)rqa_bnd_records(M, ld),
                        sizeof(float4) * (size_t)((M + 2047) / 2048) * ld, s, V)))
    return rc;
  if (lines) {
    launch_rqa(1, M, (M < N ? M : N) + 1, V.maskT, 0, ld, V.d_dims, lmin, V.region[0], 0, counts_out, lmax_out,
               stats_out, hist_cap, hist_out, s);
    ACOSS_LAUNCH_CHECK();
  }
  if (smax_out) {
    launch_dp(0, true, 1, M, V.maskT, 0, ld, V.d_dims, __builtin_inff(), __builtin_inff(),
              reinterpret_cast<float4*>(V.region[1]), 0, smax_out, s);
    ACOSS_LAUNCH_CHECK();
  }
  return matrix_finish(V, s);
}

// The four pairs of entries below share one body each; align (launch_dp's: 0 = Qmax, 1 = dmax) picks
// the lane policy and, for the paths, the backtrack and the length a path can reach.
namespace {

// the fewest path_out entries per pair an entry accepts for matrices of at most M x N
int path_bound(int align, int M, int N) { return align == 0 ? (M < N ? M : N) : dmax_path_bound(M, N); }

int crp_locate_any(int align, const float* feats, const int64_t* track_off, const int32_t* track_len,
                   int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                   const acoss_crp_params2* params2, const OtiSel& sel, float* score_out, int32_t* seg_out,
                   int32_t* oti_out, void* hip_stream) {
  clear_error();
  const acoss_crp_params* params = params2 ? &params2->base : nullptr;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  void* tb = nullptr;  // band-boundary records of the tracing DP, tstride per pair
  int64_t tstride = 0;
  return crp_batches(
      feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params2, sel, false, s, oti_out,
      [&] {
        if (!seg_out) {
          set_error("seg_out is NULL");
          return ACOSS_E_ARG;
        }
        return check_cell_bits(stacked_len(max_len, params->m, params->tau));
      },
      [&](const CrpPlan& C, int64_t& nbd) {
        tstride = trace_bnd_records(C.L, C.ld);
        tb = workspace(SLOT_LOCATE, kTraceRecBytes * (size_t)tstride * (size_t)nbd);
        return tb ? ACOSS_OK : ACOSS_E_HIP;
      },
      [&](const CrpPlan& C, int64_t base, int nb, int, const OtiWs&) {
        prof_begin(PH_DP_TRACE, s);
        launch_trace(align, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims, params->gamma_open, params->gamma_ext, tb,
                     tstride, score_out ? score_out + base : nullptr, seg_out + 4 * base, s);
        ACOSS_LAUNCH_CHECK();
        prof_end(PH_DP_TRACE, s);
        return ACOSS_OK;
      });
}

int locate_crp_any(int align, const char* entry, const uint8_t* crp, int32_t M, int32_t N, float gamma_open,
                   float gamma_ext, float* score_out, int32_t* seg_out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || !score_out || !seg_out) {
    set_error("bad arguments to %s", entry);
    return ACOSS_E_ARG;
  }
  int rc;
  if ((rc = check_cell_bits(M, N))) return rc;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (M == 0 || N == 0) return empty_matrix_answer(score_out, seg_out, nullptr, nullptr, 0, s);
  MatrixView V;
  const size_t bnd_bytes = kTraceRecBytes * (size_t)trace_bnd_records(M, matrix_pitch(N));
  if ((rc = pack_matrix(SLOT_LOCATE_CRP, crp, M, N, bnd_bytes, 0, s, V))) return rc;
  launch_trace(align, 1, M, V.maskT, 0, V.ld, V.d_dims, gamma_open, gamma_ext, V.region[0], 0, score_out, seg_out, s);
  ACOSS_LAUNCH_CHECK();
  return matrix_finish(V, s);
}

int crp_path_any(int align, const float* feats, const int64_t* track_off, const int32_t* track_len, int32_t n_tracks,
                 int32_t max_len, const int32_t* pairs, int64_t n_pairs, const acoss_crp_params2* params2,
                 const OtiSel& sel, float* score_out, int32_t* seg_out, int32_t* oti_out, int32_t path_cap,
                 int32_t* len_out, int32_t* path_out, void* hip_stream) {
  clear_error();
  const acoss_crp_params* params = params2 ? &params2->base : nullptr;
  if (path_cap < 0) {
    set_error("negative size");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  uint8_t* plane = nullptr;  // per pair of a DP batch: the direction plane (pstride bytes), the
  float4* bnd = nullptr;     // band-boundary records (bstride) and the end key
  uint32_t* endkey = nullptr;
  int64_t pstride = 0, bstride = 0;
  return crp_batches(
      feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params2, sel, false, s, oti_out,
      [&] {
        if (!len_out || !path_out) {
          set_error("len_out or path_out is NULL");
          return ACOSS_E_ARG;
        }
        const int Lmax = stacked_len(max_len, params->m, params->tau);
        if (int rc = check_cell_bits(Lmax)) return rc;
        if (align == 0 && path_cap < Lmax) {
          set_error("path_cap %d below the longest stacked length %d: a path may have that many cells", path_cap,
                    Lmax);
          return ACOSS_E_ARG;
        }
        if (align == 1 && path_cap < path_bound(1, Lmax, Lmax)) {
          set_error("path_cap %d below %d = floor(4 L / 3) - 2 at the longest stacked length L = %d: a dmax path may "
                    "have that many cells",
                    path_cap, path_bound(1, Lmax, Lmax), Lmax);
          return ACOSS_E_ARG;
        }
        return ACOSS_OK;
      },
      [&](const CrpPlan& C, int64_t& nbd) {
        pstride = (int64_t)align_up((size_t)dir_plane_bytes(C.L, C.ld), 256);
        bstride = trace_bnd_records(C.L, C.ld);
        nbd = path_dp_batch(n_pairs, C.nb_alloc, pstride, path_plane_budget());
        const size_t plane_bytes = (size_t)pstride * (size_t)nbd;
        const size_t bnd_bytes = align_up(sizeof(float4) * (size_t)bstride * (size_t)nbd, 256);
        char* ws = static_cast<char*>(workspace(SLOT_PATH, plane_bytes + bnd_bytes + 4 * (size_t)nbd));
        if (!ws) return ACOSS_E_HIP;
        plane = reinterpret_cast<uint8_t*>(ws);
        bnd = reinterpret_cast<float4*>(ws + plane_bytes);
        endkey = reinterpret_cast<uint32_t*>(ws + plane_bytes + bnd_bytes);
        return ACOSS_OK;
      },
      [&](const CrpPlan& C, int64_t base, int nb, int, const OtiWs&) {
        prof_begin(PH_DP_DIR, s);
        launch_dir(align, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims, params->gamma_open, params->gamma_ext, bnd,
                   bstride, plane, pstride, endkey, score_out ? score_out + base : nullptr, s);
        ACOSS_LAUNCH_CHECK();
        prof_end(PH_DP_DIR, s);
        prof_begin(PH_BACKTRACK, s);
        launch_backtrack(align, nb, plane, pstride, C.mask, C.mask_stride, C.ld, C.dims, endkey, path_cap,
                         seg_out ? seg_out + 4 * base : nullptr, len_out + base,
                         path_out + 2 * (size_t)path_cap * (size_t)base, s);
        ACOSS_LAUNCH_CHECK();
        prof_end(PH_BACKTRACK, s);
        return ACOSS_OK;
      });
}

int path_crp_any(int align, const char* entry, const uint8_t* crp, int32_t M, int32_t N, float gamma_open,
                 float gamma_ext, float* score_out, int32_t* seg_out, int32_t path_cap, int32_t* len_out,
                 int32_t* path_out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || path_cap < 0 || !score_out || !len_out || !path_out) {
    set_error("bad arguments to %s", entry);
    return ACOSS_E_ARG;
  }
  int rc;
  if ((rc = check_cell_bits(M, N))) return rc;
  if (align == 0 && path_cap < path_bound(0, M, N)) {
    set_error("path_cap %d below min(M, N) = %d: a path may have that many cells", path_cap, path_bound(0, M, N));
    return ACOSS_E_ARG;
  }
  if (align == 1 && path_cap < path_bound(1, M, N)) {
    set_error("path_cap %d below floor(2 (M + N) / 3) - 2 = %d: a dmax path may have that many cells", path_cap,
              path_bound(1, M, N));
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (M == 0 || N == 0) return empty_matrix_answer(score_out, seg_out, len_out, path_out, path_cap, s);
  MatrixView V;
  const int ld = matrix_pitch(N);
  if ((rc = pack_matrix(SLOT_PATH_CRP, crp, M, N, sizeof(float4) * (size_t)trace_bnd_records(M, ld),
                        (size_t)dir_plane_bytes(M, ld), s, V)))
    return rc;
  uint8_t* plane = reinterpret_cast<uint8_t*>(V.region[1]);
  launch_dir(align, 1, M, V.maskT, 0, ld, V.d_dims, gamma_open, gamma_ext, reinterpret_cast<float4*>(V.region[0]), 0,
             plane, 0, V.d_end, score_out, s);
  ACOSS_LAUNCH_CHECK();
  launch_backtrack(align, 1, plane, 0, V.maskT, 0, ld, V.d_dims, V.d_end, path_cap, seg_out, len_out, path_out, s);
  ACOSS_LAUNCH_CHECK();
  return matrix_finish(V, s);
}

}  // namespace

extern "C" int acoss_crp_locate(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                const acoss_crp_params* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                                void* hip_stream) {
  acoss_crp_params2 W;
  return crp_locate_any(0, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, widen(params, W), kOtiFirst,
                        qmax_out, seg_out, oti_out, hip_stream);
}

extern "C" int acoss_crp_locate2(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                 int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                 const acoss_crp_params2* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                                 void* hip_stream) {
  return crp_locate_any(0, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, kOtiFirst, qmax_out,
                        seg_out, oti_out, hip_stream);
}

extern "C" int acoss_crp_locate3(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                 int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                 const acoss_crp_params3* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                                 const int32_t* picks, void* hip_stream) {
  return crp_locate_any(0, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs,
                        params ? &params->base : nullptr, oti_sel(params, picks), qmax_out, seg_out, oti_out,
                        hip_stream);
}

extern "C" int acoss_crp_locate_dmax(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                     int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                     const acoss_crp_params* params, float* dmax_out, int32_t* seg_out,
                                     int32_t* oti_out, void* hip_stream) {
  acoss_crp_params2 W;
  return crp_locate_any(1, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, widen(params, W), kOtiFirst,
                        dmax_out, seg_out, oti_out, hip_stream);
}

extern "C" int acoss_crp_locate_dmax2(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                      int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                      const acoss_crp_params2* params, float* dmax_out, int32_t* seg_out,
                                      int32_t* oti_out, void* hip_stream) {
  return crp_locate_any(1, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, kOtiFirst, dmax_out,
                        seg_out, oti_out, hip_stream);
}

extern "C" int acoss_crp_locate_dmax3(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                      int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                      const acoss_crp_params3* params, float* dmax_out, int32_t* seg_out,
                                      int32_t* oti_out, const int32_t* picks, void* hip_stream) {
  return crp_locate_any(1, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs,
                        params ? &params->base : nullptr, oti_sel(params, picks), dmax_out, seg_out, oti_out,
                        hip_stream);
}

extern "C" int acoss_locate_crp(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                                float* score_out, int32_t* seg_out, void* hip_stream) {
  return locate_crp_any(0, "acoss_locate_crp", crp, M, N, gamma_open, gamma_ext, score_out, seg_out, hip_stream);
}

extern "C" int acoss_locate_crp_dmax(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                                     float* score_out, int32_t* seg_out, void* hip_stream) {
  return locate_crp_any(1, "acoss_locate_crp_dmax", crp, M, N, gamma_open, gamma_ext, score_out, seg_out, hip_stream);
}

extern "C" int acoss_crp_path(const float* feats, const int64_t* track_off, const int32_t* track_len,
                              int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                              const acoss_crp_params* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                              int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  acoss_crp_params2 W;
  return crp_path_any(0, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, widen(params, W), kOtiFirst,
                      qmax_out, seg_out, oti_out, path_cap, len_out, path_out, hip_stream);
}

extern "C" int acoss_crp_path2(const float* feats, const int64_t* track_off, const int32_t* track_len,
                               int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                               const acoss_crp_params2* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                               int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  return crp_path_any(0, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, kOtiFirst, qmax_out,
                      seg_out, oti_out, path_cap, len_out, path_out, hip_stream);
}

extern "C" int acoss_crp_path3(const float* feats, const int64_t* track_off, const int32_t* track_len,
                               int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                               const acoss_crp_params3* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                               int32_t path_cap, int32_t* len_out, int32_t* path_out, const int32_t* picks,
                               void* hip_stream) {
  return crp_path_any(0, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs,
                      params ? &params->base : nullptr, oti_sel(params, picks), qmax_out, seg_out, oti_out, path_cap,
                      len_out, path_out, hip_stream);
}

extern "C" int acoss_crp_path_dmax(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                   int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                   const acoss_crp_params* params, float* dmax_out, int32_t* seg_out, int32_t* oti_out,
                                   int32_t path_cap, int32_t* len_out, int32_t* path_out, void* hip_stream) {
  acoss_crp_params2 W;
  return crp_path_any(1, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, widen(params, W), kOtiFirst,
                      dmax_out, seg_out, oti_out, path_cap, len_out, path_out, hip_stream);
}

extern "C" int acoss_crp_path_dmax2(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                    int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                    const acoss_crp_params2* params, float* dmax_out, int32_t* seg_out,
                                    int32_t* oti_out, int32_t path_cap, int32_t* len_out, int32_t* path_out,
                                    void* hip_stream) {
  return crp_path_any(1, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs, params, kOtiFirst, dmax_out,
                      seg_out, oti_out, path_cap, len_out, path_out, hip_stream);
}

extern "C" int acoss_crp_path_dmax3(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                    int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                    const acoss_crp_params3* params, float* dmax_out, int32_t* seg_out,
                                    int32_t* oti_out, int32_t path_cap, int32_t* len_out, int32_t* path_out, const int32_t* picks,
                                    void* hip_stream) {
  return crp_path_any(1, feats, track_off, track_len, n_tracks, max_len, pairs, n_pairs,
                      params ? &params->base : nullptr, oti_sel(params, picks), dmax_out, seg_out, oti_out, path_cap,
                      len_out, path_out, hip_stream);
}

extern "C" int acoss_path_crp(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                              float* score_out, int32_t* seg_out, int32_t path_cap, int32_t* len_out,
                              int32_t* path_out, void* hip_stream) {
  return path_crp_any(0, "acoss_path_crp", crp, M, N, gamma_open, gamma_ext, score_out, seg_out, path_cap, len_out,
                      path_out, hip_stream);
}

extern "C" int acoss_path_crp_dmax(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                                   float* score_out, int32_t* seg_out, int32_t path_cap, int32_t* len_out,
                                   int32_t* path_out, void* hip_stream) {
  return path_crp_any(1, "acoss_path_crp_dmax", crp, M, N, gamma_open, gamma_ext, score_out, seg_out, path_cap,
                      len_out, path_out, hip_stream);
}
