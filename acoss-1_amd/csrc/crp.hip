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
//  * k_crp_dp: one wave per pair. Lane l owns 32 rows of a 2048-row band and sweeps the
//    columns skewed by one column per lane (anti-diagonal wavefront); the two boundary rows
//    pass down one lane per step with __shfl_up; bands chain through a small HBM buffer.
//  * k_crp_dp_trace: the serra09 DP again, every cell also carrying the cell where its path
//    began, for acoss_crp_locate / acoss_locate_crp (where the Qmax alignment starts and ends).
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

// Per pair: OTI index (essentia optimalTranspositionIndex restated) and stacked dims.
__global__ void k_pair_oti(const float* __restrict__ prof, const int32_t* __restrict__ len,
                           const int32_t* __restrict__ pairs, int64_t n_pairs, int use_oti, int m, int tau,
                           int32_t* __restrict__ oti, int2* __restrict__ dims) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const int a = pairs[2 * p], b = pairs[2 * p + 1];
  int best = 0;
  if (use_oti) {
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

// --------------------------------------------------------------------------------------
// k_crp_dp<ALIGN, EQG, R>: essentia CoverSongSimilarity(serra09 | chen17, 'symmetric').
// One wave per pair; lane l owns R rows, band*64R + Rl .. +R-1 (R = 32, 16 or 8 by the batch's
// longest CRP, so short tracks keep every lane busy); column c = s - l at step s.
// --------------------------------------------------------------------------------------
struct DpAbove {  // what lane l-1 (or the band above) hands down for one column
  float q30, q31;  // its last two rows (R-2, R-1)
  uint32_t b;      // bit0 = C[row R-2], bit1 = C[row R-1]
};

// FAST (serra09 with gamma_open == gamma_ext = K/2 >= 0, the reference's setting): every score is
// an exact multiple of 1/2, so "hit ? mx + 1 : max(mx - go, 0)" is max(fma(hit, 1 + go, mx - go), 0)
// exactly, and the validity masks move out of the row loop: the kernel zeroes the CRP words of
// columns < 2 and rows outside [2, Mp) at the fetch. Cells there then hold 0 (top-left: all their
// predecessors are 0) or at most max(0, best - go) (bottom/right: no hit, and they never feed a
// valid cell), so neither the valid scores nor their maximum change.
// v_cvt_f32_ubyteB: byte B of v as a float (the compiler emits only the byte-0 form plus shifts).
template <int B>
__device__ __forceinline__ float cvt_f32_ubyte(uint32_t v) {
  float f;
  if constexpr (B == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(v));
  else if constexpr (B == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(v));
  else if constexpr (B == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(v));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(v));
  return f;
}

// b is a constant after the row loops unroll, so the switch folds away
__device__ __forceinline__ float cvt_f32_ubyte_n(uint32_t v, int b) {
  switch (b) {
    case 0: return cvt_f32_ubyte<0>(v);
    case 1: return cvt_f32_ubyte<1>(v);
    case 2: return cvt_f32_ubyte<2>(v);
    default: return cvt_f32_ubyte<3>(v);
  }
}

template <int ALIGN, bool EQG, int R, bool FAST = false>
struct DpLane {
  float go, ge;
  int Np, lane, c_off;  // column of this lane at step s: s - lane
  uint32_t rowvalid;    // bit r: 2 <= global row < Mp
  uint32_t w1, w2;      // CRP words of columns c-1, c-2 (bit r = row r)
  DpAbove h1, h2;       // from above for columns c-1, c-2
  float best;

  __device__ __forceinline__ float gam(uint32_t bit) const { return EQG ? go : (bit ? go : ge); }

  // qn: new column c; q1: column c-1; q2: column c-2. w0: CRP word of column c;
  // h0: from above for column c. Returns the values to hand to the lane below.
  __device__ __forceinline__ DpAbove step(float (&qn)[R], const float (&q1)[R], const float (&q2)[R],
                                          uint32_t w0, const DpAbove& h0, int c) {
    const bool colvalid = (c >= 2) && (c < Np);
    const uint32_t vmask = colvalid ? rowvalid : 0u;
    // extended words: bit r+2 <-> row r; bits 0,1 <-> rows -2,-1 (from above)
    const uint64_t e0 = ((uint64_t)w0 << 2) | h0.b;
    const uint64_t e1 = ((uint64_t)w1 << 2) | h1.b;
    const uint64_t e2 = ((uint64_t)w2 << 2) | h2.b;
    if constexpr (FAST) {
      // two rows per v_pk_add_f32 / v_pk_fma_f32; the hit bits as bytes (rows k, k+8, k+16, k+24
      // of one masked word), one v_cvt_f32_ubyteN each
      typedef float dp_f32x2 __attribute__((ext_vector_type(2)));
      const dp_f32x2 g1 = {1.0f + go, 1.0f + go};
      const dp_f32x2 ngo = {-go, -go};
      uint32_t bm[R < 8 ? R : 8];
#pragma unroll
      for (int k = 0; k < (R < 8 ? R : 8); ++k) bm[k] = (w0 >> k) & 0x01010101u;
#pragma unroll
      for (int r = 0; r < R; r += 2) {
        float mxs[2], hb[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const int rr = r + e;
          const float Qa = rr >= 1 ? q1[rr - 1] : h1.q31;
          const float Qb = rr >= 2 ? q1[rr - 2] : (rr == 1 ? h1.q31 : h1.q30);
          const float Qc = rr >= 1 ? q2[rr - 1] : h2.q31;
          mxs[e] = fmaxf(fmaxf(Qa, Qb), Qc);
          hb[e] = cvt_f32_ubyte_n(bm[rr & 7], rr >> 3);
        }
        const dp_f32x2 mx = {mxs[0], mxs[1]};
        const dp_f32x2 hv = {hb[0], hb[1]};
        const dp_f32x2 t = __builtin_elementwise_fma(hv, g1, mx + ngo);
        asm("v_max3_f32 %0, %1, %2, %3" : "=v"(best) : "v"(best), "v"(t.x), "v"(t.y));
        qn[r] = fmaxf(t.x, 0.0f);
        qn[r + 1] = fmaxf(t.y, 0.0f);
      }
    } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float Qa = r >= 1 ? q1[r - 1] : h1.q31;                            // Q[r-1][c-1]
      float Qb = r >= 2 ? q1[r - 2] : (r == 1 ? h1.q31 : h1.q30);              // Q[r-2][c-1]
      float Qc = r >= 1 ? q2[r - 1] : h2.q31;                                  // Q[r-1][c-2]
      if (ALIGN == 1) {
        Qb = Qb + (float)((e0 >> (r + 1)) & 1u);  // + C[r-1][c]
        Qc = Qc + (float)((e1 >> (r + 2)) & 1u);  // + C[r][c-1]
      }
      const bool hit = (e0 >> (r + 2)) & 1u;
      float v;
      if (EQG) {
        const float mx = fmaxf(fmaxf(Qa, Qb), Qc);
        v = hit ? mx + 1.0f : fmaxf(mx - go, 0.0f);
      } else {
        const float x = Qa - gam((e1 >> (r + 1)) & 1u);  // gamma(C[r-1][c-1])
        const float y = Qb - gam((e1 >> r) & 1u);        // gamma(C[r-2][c-1])
        const float z = Qc - gam((e2 >> (r + 1)) & 1u);  // gamma(C[r-1][c-2])
        const float miss = fmaxf(fmaxf(0.0f, x), fmaxf(y, z));
        v = hit ? fmaxf(fmaxf(Qa, Qb), Qc) + 1.0f : miss;
      }
      v = ((vmask >> r) & 1u) ? v : 0.0f;
      best = fmaxf(best, v);
      qn[r] = v;
    }
    }
    DpAbove out;
    out.q30 = qn[R - 2];
    out.q31 = qn[R - 1];
    out.b = (w0 >> (R - 2)) & 3u;
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

template <int ALIGN, bool EQG, int R, bool FAST>
__device__ __forceinline__ void crp_dp_body(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                               const int2* __restrict__ dims, float go, float ge,
                                               float4* __restrict__ bnd, int64_t bnd_stride,
                                               float* __restrict__ out) {
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  float best = 0.0f;
  constexpr int kBand = 64 * R;
  const int nbands = (Mp + kBand - 1) / kBand;
  for (int band = 0; band < nbands; ++band) {
    const int row0 = band * kBand + lane * R;
    const uint32_t* mrow = maskT + (size_t)p * mask_stride + (size_t)(row0 >> 5) * ld;
    const int sh = row0 & 31;  // this lane's R rows inside its 32-row strip word
    float4* bout = bnd + (size_t)p * bnd_stride + (size_t)band * ld;
    const float4* bin = bnd + (size_t)p * bnd_stride + (size_t)(band - 1) * ld;
    DpLane<ALIGN, EQG, R, FAST> L;
    L.go = go;
    L.ge = ge;
    L.Np = Np;
    L.lane = lane;
    uint32_t rv = 0;
    for (int r = 0; r < R; ++r) rv |= (uint32_t)((row0 + r >= 2) && (row0 + r < Mp)) << r;
    L.rowvalid = rv;
    L.w1 = L.w2 = 0;
    L.h1 = L.h2 = DpAbove{0.0f, 0.0f, 0u};
    L.best = 0.0f;
    float qa[R], qb[R], qc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) qa[r] = qb[r] = qc[r] = 0.0f;
    DpAbove pub{0.0f, 0.0f, 0u};
    const int S_end = Np + 63;
    const bool lane_active = row0 < Mp;
    auto fetch = [&](int c) -> uint32_t {
      if (!(lane_active && c >= (FAST ? 2 : 0) && c < Np)) return 0u;
      const uint32_t w = mrow[c];
      const uint32_t wr = R == 32 ? w : (w >> sh) & ((1u << (R & 31)) - 1u);
      return FAST ? (wr & rv) : wr;
    };
    auto recv = [&](const DpAbove& mine, int c) -> DpAbove {
      DpAbove h;
      h.q30 = __shfl_up(mine.q30, 1);
      h.q31 = __shfl_up(mine.q31, 1);
      h.b = (uint32_t)__shfl_up((int)mine.b, 1);
      if (lane == 0) {
        if (band > 0 && c >= 0 && c < Np) {
          const float4 v = bin[c];
          h = DpAbove{v.x, v.y, (uint32_t)v.z};
        } else {
          h = DpAbove{0.0f, 0.0f, 0u};
        }
      }
      return h;
    };
    auto publish = [&](const DpAbove& o, int c) {
      if (lane == 63 && band + 1 < nbands && c >= 0 && c < Np) bout[c] = make_float4(o.q30, o.q31, (float)o.b, 0.0f);
    };
    uint32_t wnext = fetch(-lane);
    for (int s = 0; s < S_end; s += 3) {
      {
        const int c = s - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAbove h0 = recv(pub, c);
        pub = L.step(qa, qb, qc, w0, h0, c);
        publish(pub, c);
      }
      if (s + 1 < S_end) {
        const int c = s + 1 - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAbove h0 = recv(pub, c);
        pub = L.step(qc, qa, qb, w0, h0, c);
        publish(pub, c);
      }
      if (s + 2 < S_end) {
        const int c = s + 2 - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAbove h0 = recv(pub, c);
        pub = L.step(qb, qc, qa, w0, h0, c);
        publish(pub, c);
      }
    }
    best = fmaxf(best, L.best);
    __threadfence_block();
    __syncthreads();
  }
  best = wave_max(best);
  if (lane == 0) out[p] = best;
}

template <int ALIGN, bool EQG, int R>
__global__ __launch_bounds__(64) void k_crp_dp(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                               const int2* __restrict__ dims, float go, float ge,
                                               float4* __restrict__ bnd, int64_t bnd_stride,
                                               float* __restrict__ out) {
  crp_dp_body<ALIGN, EQG, R, false>(maskT, mask_stride, ld, dims, go, ge, bnd, bnd_stride, out);
}

// No occupancy hint: the FAST body compiles to about 200 VGPRs (2 waves per SIMD), which measured
// faster than forcing it into 128 (4 waves per SIMD): 14.2 vs 14.8 ms per covers80 step.
template <int R>
__global__ __launch_bounds__(64) void k_crp_dp_fast(
    const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld, const int2* __restrict__ dims, float go, float ge,
    float4* __restrict__ bnd, int64_t bnd_stride, float* __restrict__ out) {
  crp_dp_body<0, true, R, true>(maskT, mask_stride, ld, dims, go, ge, bnd, bnd_stride, out);
}

// --------------------------------------------------------------------------------------
// k_crp_dp_grp: the FAST DP (serra09, gamma_open == gamma_ext = K/2) with SEVERAL pairs per
// wave for CRPs of at most 2048 rows: a group of LP = ceil(L / 32) lanes per pair (lane ll owns
// rows 32 ll .. 32 ll + 31, one band), G = 64 / LP groups per wave. A one-pair wave walks
// N' + 63 steps however short the pair; a group walks N' + LP - 1, and every lane keeps 32 rows
// per step, so short tracks (Da-TACOS lengths: L ~ 500) no longer leave most lanes idle or pay
// the per-step shuffles for 8 rows. Same recurrence, same DpLane step: bit-identical scores.
// --------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_crp_dp_grp(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                   const int2* __restrict__ dims, int nb, int LP, float go,
                                                   float* __restrict__ out) {
  constexpr int R = 32;
  __shared__ float s_best[64];
  const int lane = threadIdx.x;
  const int G = 64 / LP;
  const int g = lane / LP, ll = lane - g * LP;
  const int p = blockIdx.x * G + g;
  const bool in_group = g < G && p < nb;
  const int2 dm = in_group ? dims[p] : make_int2(0, 0);
  const int Mp = dm.x, Np = dm.y;
  const int row0 = ll * R;
  const uint32_t* mrow = maskT + (size_t)(in_group ? p : 0) * mask_stride + (size_t)ll * ld;
  DpLane<0, true, R, true> L;
  L.go = go;
  L.ge = go;
  L.Np = Np;
  L.lane = ll;
  uint32_t rv = 0;
  for (int r = 0; r < R; ++r) rv |= (uint32_t)((row0 + r >= 2) && (row0 + r < Mp)) << r;
  L.rowvalid = rv;
  L.w1 = L.w2 = 0;
  L.h1 = L.h2 = DpAbove{0.0f, 0.0f, 0u};
  L.best = 0.0f;
  float qa[R], qb[R], qc[R];
#pragma unroll
  for (int r = 0; r < R; ++r) qa[r] = qb[r] = qc[r] = 0.0f;
  DpAbove pub{0.0f, 0.0f, 0u};
  // steps until every group of the wave is done (wave-uniform bound)
  const int S_end = (int)wave_max_u32(in_group ? (unsigned)(Np + LP - 1) : 0u);
  const bool lane_active = in_group && row0 < Mp;
  auto fetch = [&](int c) -> uint32_t {
    if (!(lane_active && c >= 2 && c < Np)) return 0u;
    return mrow[c] & rv;
  };
  auto recv = [&](const DpAbove& mine) -> DpAbove {
    DpAbove h;
    h.q30 = __shfl_up(mine.q30, 1);
    h.q31 = __shfl_up(mine.q31, 1);
    h.b = (uint32_t)__shfl_up((int)mine.b, 1);
    if (ll == 0) h = DpAbove{0.0f, 0.0f, 0u};  // the group's first rows: nothing above
    return h;
  };
  uint32_t wnext = fetch(-ll);
  for (int s = 0; s < S_end; s += 3) {
    {
      const int c = s - ll;
      const uint32_t w0 = wnext;
      wnext = fetch(c + 1);
      pub = L.step(qa, qb, qc, w0, recv(pub), c);
    }
    if (s + 1 < S_end) {
      const int c = s + 1 - ll;
      const uint32_t w0 = wnext;
      wnext = fetch(c + 1);
      pub = L.step(qc, qa, qb, w0, recv(pub), c);
    }
    if (s + 2 < S_end) {
      const int c = s + 2 - ll;
      const uint32_t w0 = wnext;
      wnext = fetch(c + 1);
      pub = L.step(qb, qc, qa, w0, recv(pub), c);
    }
  }
  // per-group maximum through LDS (groups need not be a power of two wide)
  s_best[lane] = L.best;
  __syncthreads();
  if (in_group && ll == 0) {
    float b = 0.0f;
    for (int k = 0; k < LP; ++k) b = fmaxf(b, s_best[lane + k]);
    out[p] = b;
  }
}

// --------------------------------------------------------------------------------------
// k_crp_dp_pk<ALIGN>: k_crp_dp<ALIGN, true, 32> in packed 16-bit integers. With
// gamma_open == gamma_ext = K/2 (K a small integer, 1 for the reference's 0.5), every score is
// a multiple of 1/2, so 2Q is an exact integer below 4 L: lane l keeps rows (h, h + 16) of a
// column in one u32 (row h low, row h + 16 high) and takes two rows per v_pk_max_u16 /
// v_pk_add_u16 / saturating v_pk_sub_u16 (max(x - K, 0) in one instruction). The predecessor
// rows of pair h are pair h - 1 / h - 2 of the previous columns; pairs 0 and 1 splice in the
// rows handed down by the lane above (v_perm). Bit-identical to the f32 kernel: both compute
// the same exact multiples of 1/2 (the f32 values never round).
// --------------------------------------------------------------------------------------
typedef unsigned short dp_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk16(dp_u16x2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ dp_u16x2 up16(unsigned v) { return __builtin_bit_cast(dp_u16x2, v); }
__device__ __forceinline__ unsigned pk_max16(unsigned a, unsigned b) { return pk16(__builtin_elementwise_max(up16(a), up16(b))); }
__device__ __forceinline__ unsigned pk_add16(unsigned a, unsigned b) { return pk16(up16(a) + up16(b)); }
__device__ __forceinline__ unsigned pk_sub16(unsigned a, unsigned b) { return pk16(up16(a) - up16(b)); }
__device__ __forceinline__ unsigned pk_subsat16(unsigned a, unsigned b) {
  return pk16(__builtin_elementwise_sub_sat(up16(a), up16(b)));
}

struct DpAbovePk {  // what lane l-1 (or the band above) hands down for one column
  unsigned hq;      // its rows 30 (low half) and 31 (high half), x2 units
  uint32_t b;       // bit0 = C[row 30], bit1 = C[row 31]
};

template <int ALIGN>
struct DpLanePk {
  unsigned K;          // gamma in x2 units, both halves
  int Np;
  uint32_t rz0, rz1;   // AND masks of pairs 0 / 1: rows 0 and 1 of the first band are 0
  uint32_t w1, w2;     // CRP words of columns c-1, c-2
  DpAbovePk h1, h2;    // from above for columns c-1, c-2
  unsigned best;

  __device__ __forceinline__ DpAbovePk step(unsigned (&pn)[16], const unsigned (&p1)[16], const unsigned (&p2)[16],
                                            uint32_t w0, const DpAbovePk& h0, int c) {
    const bool colok = (c >= 2) && (c < Np);
    // rows (-1, 15) and (-2, 14) of column c-1, (-1, 15) of column c-2
    const unsigned a0 = __builtin_amdgcn_perm(p1[15], h1.hq, 0x05040302u);
    const unsigned b0 = __builtin_amdgcn_perm(p1[14], h1.hq, 0x05040100u);
    const unsigned c0 = __builtin_amdgcn_perm(p2[15], h2.hq, 0x05040302u);
#pragma unroll
    for (int h = 0; h < 16; ++h) {
      const unsigned A = h >= 1 ? p1[h - 1] : a0;                  // Q[r-1][c-1]
      unsigned B = h >= 2 ? p1[h - 2] : (h == 1 ? a0 : b0);        // Q[r-2][c-1]
      unsigned Cq = h >= 1 ? p2[h - 1] : c0;                       // Q[r-1][c-2]
      if (ALIGN == 1) {
        const unsigned cb = h >= 1 ? (w0 >> (h - 1)) & 0x10001u : ((h0.b >> 1) & 1u) | (((w0 >> 15) & 1u) << 16);
        B = pk_add16(B, cb << 1);                                  // + C[r-1][c]
        Cq = pk_add16(Cq, ((w1 >> h) & 0x10001u) << 1);            // + C[r][c-1]
      }
      const unsigned mx = pk_max16(pk_max16(A, B), Cq);
      const unsigned m = pk_sub16(0u, (w0 >> h) & 0x10001u);      // 0xffff where C[r][c] = 1
      unsigned v = (m & pk_add16(mx, 0x00020002u)) | (~m & pk_subsat16(mx, K));
      if (h == 0) v &= rz0;
      if (h == 1) v &= rz1;
      v = colok ? v : 0u;
      best = pk_max16(best, v);
      pn[h] = v;
    }
    DpAbovePk out;
    out.hq = __builtin_amdgcn_perm(pn[15], pn[14], 0x07060302u);
    out.b = (w0 >> 30) & 3u;
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

template <int ALIGN>
__global__ __launch_bounds__(64) void k_crp_dp_pk(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                  const int2* __restrict__ dims, unsigned K,
                                                  float4* __restrict__ bnd, int64_t bnd_stride,
                                                  float* __restrict__ out) {
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  unsigned best = 0u;
  constexpr int kBand = 64 * 32;
  const int nbands = (Mp + kBand - 1) / kBand;
  for (int band = 0; band < nbands; ++band) {
    const int row0 = band * kBand + lane * 32;
    const uint32_t* mrow = maskT + (size_t)p * mask_stride + (size_t)(row0 >> 5) * ld;
    float4* bout = bnd + (size_t)p * bnd_stride + (size_t)band * ld;
    const float4* bin = bnd + (size_t)p * bnd_stride + (size_t)(band - 1) * ld;
    DpLanePk<ALIGN> L;
    L.K = K * 0x10001u;
    L.Np = Np;
    L.rz0 = row0 == 0 ? 0xffff0000u : 0xffffffffu;
    L.rz1 = L.rz0;
    L.w1 = L.w2 = 0;
    L.h1 = L.h2 = DpAbovePk{0u, 0u};
    L.best = 0u;
    unsigned qa[16], qb[16], qc[16];
#pragma unroll
    for (int h = 0; h < 16; ++h) qa[h] = qb[h] = qc[h] = 0u;
    DpAbovePk pub{0u, 0u};
    const int S_end = Np + 63;
    const bool lane_active = row0 < Mp;
    auto fetch = [&](int c) -> uint32_t { return (lane_active && c >= 0 && c < Np) ? mrow[c] : 0u; };
    auto recv = [&](const DpAbovePk& mine, int c) -> DpAbovePk {
      DpAbovePk h;
      h.hq = (unsigned)__shfl_up((int)mine.hq, 1);
      h.b = (uint32_t)__shfl_up((int)mine.b, 1);
      if (lane == 0) {
        if (band > 0 && c >= 0 && c < Np) {
          const float4 v = bin[c];
          h = DpAbovePk{__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y)};
        } else {
          h = DpAbovePk{0u, 0u};
        }
      }
      return h;
    };
    auto publish = [&](const DpAbovePk& o, int c) {
      if (lane == 63 && band + 1 < nbands && c >= 0 && c < Np)
        bout[c] = make_float4(__builtin_bit_cast(float, o.hq), __builtin_bit_cast(float, o.b), 0.0f, 0.0f);
    };
    uint32_t wnext = fetch(-lane);
    for (int s = 0; s < S_end; s += 3) {
      {
        const int c = s - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAbovePk h0 = recv(pub, c);
        pub = L.step(qa, qb, qc, w0, h0, c);
        publish(pub, c);
      }
      if (s + 1 < S_end) {
        const int c = s + 1 - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAbovePk h0 = recv(pub, c);
        pub = L.step(qc, qa, qb, w0, h0, c);
        publish(pub, c);
      }
      if (s + 2 < S_end) {
        const int c = s + 2 - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAbovePk h0 = recv(pub, c);
        pub = L.step(qb, qc, qa, w0, h0, c);
        publish(pub, c);
      }
    }
    best = pk_max16(best, L.best);
    __threadfence_block();
    __syncthreads();
  }
  const unsigned b2 = max(best & 0xffffu, best >> 16);
  const float r = wave_max(0.5f * (float)b2);
  if (lane == 0) out[p] = r;
}

// --------------------------------------------------------------------------------------
// k_crp_dp_trace<EQG, R>: the serra09 DP of k_crp_dp<0, ., R> with ORIGIN PROPAGATION: every
// cell carries, beside its score, the packed cell (i0 << 16) | j0 where its path began, and the
// wave reduces (Qmax, end cell, origin of the end cell) instead of a bare maximum. Memory per
// pair stays O(1) beyond the DP's own: no M' x N' score matrix is written.
//  * predecessors in the fixed order a = (i-1, j-1), b = (i-2, j-1), c = (i-1, j-2); the origin is
//    that of the FIRST predecessor attaining the maximum (raw values on a hit, penalised values
//    on a miss; a strictly greater value replaces, an equal one does not); a hit whose
//    predecessors are all 0 starts a path at itself.
//  * the end cell is the first cell in row-major order holding Qmax. The skewed walk does not
//    visit cells in row-major order, so every update compares the packed end key (i << 16) | j:
//    v > best || (v == best && v > 0 && key < bestkey). Inside one step a lane's cells share a
//    column and come in ascending rows, so there "first wins" is the strict compare alone.
//  * general arithmetic, validity per cell (any gamma). EQG = true is launched only where
//    gamma_open == gamma_ext = K/2 (K a small non-negative integer): every score is then an exact
//    multiple of 1/2, x - gamma never rounds, and the first maximum of the penalised values is the
//    first maximum of the raw ones, so one select serves hit and miss. Origins are defined where
//    a path can only begin on a hit, i.e. for gamma >= 0.
//  * R = 8 rows per lane for CRPs of at most 512 rows, R = 16 above (bands of 64 R rows): three
//    rotating columns of R scores and R origins are 6 R live registers. A launch takes the pairs
//    with row_lo < M' <= row_hi and leaves the others to the launch of the other R.
//  * the values handed to the next lane, and across a band boundary through HBM, are the last two
//    rows' scores, CRP bits and origins (TraceRec).
// Every lane runs every step and selects; the only branches around a shuffle are wave-uniform.
// --------------------------------------------------------------------------------------
struct DpAboveT {   // what lane l-1 (or the band above) hands down for one column
  float q30, q31;   // scores of its last two rows (R-2, R-1)
  uint32_t b;       // bit0 = C[row R-2], bit1 = C[row R-1]
  uint32_t o30, o31;  // origins of the same two cells
};

struct TraceRec {  // one column of a band boundary, 32 B
  float4 q;        // q30, q31, bits as float, unused
  uint4 o;         // o30, o31, unused
};

template <bool EQG, int R>
struct DpLaneT {
  static_assert(R <= 16, "the extended CRP words are 32-bit");
  float go, ge;
  int Np;
  uint32_t rowvalid;  // bit r: 2 <= global row < Mp
  uint32_t key0;      // (global row of this lane's row 0) << 16
  uint32_t w1, w2;    // CRP words of columns c-1, c-2 (bit r = row r)
  DpAboveT h1, h2;    // from above for columns c-1, c-2
  float best;         // this lane's maximum so far, its end key and the origin of that cell
  uint32_t bkey, borg;

  // (qn, on): new column c; (q1, o1): column c-1; (q2, o2): column c-2.
  __device__ __forceinline__ DpAboveT step(float (&qn)[R], uint32_t (&on)[R], const float (&q1)[R],
                                           const uint32_t (&o1)[R], const float (&q2)[R], const uint32_t (&o2)[R],
                                           uint32_t w0, const DpAboveT& h0, int c) {
    const bool colvalid = (c >= 2) && (c < Np);
    const uint32_t vmask = colvalid ? rowvalid : 0u;
    // extended words: bit r+2 <-> row r; bits 0,1 <-> rows -2,-1 (from above)
    const uint32_t e0 = (w0 << 2) | h0.b;
    const uint32_t e1 = (w1 << 2) | h1.b;
    const uint32_t e2 = (w2 << 2) | h2.b;
    const uint32_t kc = key0 + (uint32_t)c;  // key of (row 0, c); only used where colvalid
    const float g_open = go, g_ext = ge;     // by value: a select between members is a select of addresses
    auto gam = [&](uint32_t bit) { return bit ? g_open : g_ext; };
    float cb = 0.0f;                         // this column's first maximum, its key and origin
    uint32_t ck = 0u, co = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float Qa = r >= 1 ? q1[r - 1] : h1.q31;                        // Q[r-1][c-1]
      const float Qb = r >= 2 ? q1[r - 2] : (r == 1 ? h1.q31 : h1.q30);    // Q[r-2][c-1]
      const float Qc = r >= 1 ? q2[r - 1] : h2.q31;                        // Q[r-1][c-2]
      const uint32_t Oa = r >= 1 ? o1[r - 1] : h1.o31;
      const uint32_t Ob = r >= 2 ? o1[r - 2] : (r == 1 ? h1.o31 : h1.o30);
      const uint32_t Oc = r >= 1 ? o2[r - 1] : h2.o31;
      const bool hit = (e0 >> (r + 2)) & 1u;
      float pa = Qa, pb = Qb, pc = Qc;
      if (!EQG) {
        const float x = Qa - gam((e1 >> (r + 1)) & 1u);  // gamma(C[r-1][c-1])
        const float y = Qb - gam((e1 >> r) & 1u);        // gamma(C[r-2][c-1])
        const float z = Qc - gam((e2 >> (r + 1)) & 1u);  // gamma(C[r-1][c-2])
        pa = hit ? Qa : x;
        pb = hit ? Qb : y;
        pc = hit ? Qc : z;
      }
      float mx = pa;
      uint32_t o = Oa;
      if (pb > mx) {
        mx = pb;
        o = Ob;
      }
      if (pc > mx) {
        mx = pc;
        o = Oc;
      }
      float v = hit ? mx + 1.0f : fmaxf(EQG ? mx - g_open : mx, 0.0f);
      const uint32_t key = kc + ((uint32_t)r << 16);
      o = (hit && !(mx > 0.0f)) ? key : o;  // all predecessors 0: the path starts here
      v = ((vmask >> r) & 1u) ? v : 0.0f;
      if (v > cb) {
        cb = v;
        ck = key;
        co = o;
      }
      // Pin the origin next to its score: the origins are first read in a later basic block
      // (the next step's shuffles), so the compiler sinks their selects there and carries every
      // compare mask (4 per cell, a scalar register pair each) across: 279 scalar spills at R = 16.
      asm volatile("" : "+v"(o));
      qn[r] = v;
      on[r] = o;
    }
    if (cb > best || (cb == best && cb > 0.0f && ck < bkey)) {
      best = cb;
      bkey = ck;
      borg = co;
    }
    DpAboveT out;
    out.q30 = qn[R - 2];
    out.q31 = qn[R - 1];
    out.b = (w0 >> (R - 2)) & 3u;
    out.o30 = on[R - 2];
    out.o31 = on[R - 1];
    h2 = h1;
    h1 = h0;
    w2 = w1;
    w1 = w0;
    return out;
  }
};

// bnd: ceil(L / (64 R)) * ld TraceRec per pair (bnd_stride records between pairs); only read and
// written by CRPs of more than one band. qmax_out may be NULL; seg_out: int32[4] (i0, j0, i1, j1) per pair.
template <bool EQG, int R>
__global__ __launch_bounds__(64) void k_crp_dp_trace(const uint32_t* __restrict__ maskT, int64_t mask_stride, int ld,
                                                     const int2* __restrict__ dims, int row_lo, int row_hi, float go,
                                                     float ge, TraceRec* __restrict__ bnd, int64_t bnd_stride,
                                                     float* __restrict__ qmax_out, int32_t* __restrict__ seg_out) {
  const int p = blockIdx.x;
  const int lane = threadIdx.x;
  const int2 dm = dims[p];
  const int Mp = dm.x, Np = dm.y;
  if (!(Mp > row_lo && Mp <= row_hi)) return;  // the other R's launch takes this pair (wave-uniform)
  constexpr int kBand = 64 * R;
  const int nbands = (Mp + kBand - 1) / kBand;
  DpLaneT<EQG, R> L;
  L.go = go;
  L.ge = ge;
  L.Np = Np;
  L.best = 0.0f;
  L.bkey = L.borg = 0u;
  for (int band = 0; band < nbands; ++band) {
    const int row0 = band * kBand + lane * R;
    const uint32_t* mrow = maskT + (size_t)p * mask_stride + (size_t)(row0 >> 5) * ld;
    const int sh = row0 & 31;  // this lane's R rows inside its 32-row strip word
    TraceRec* bout = bnd + (size_t)p * bnd_stride + (size_t)band * ld;
    const TraceRec* bin = bnd + (size_t)p * bnd_stride + (size_t)(band - 1) * ld;
    uint32_t rv = 0;
    for (int r = 0; r < R; ++r) rv |= (uint32_t)((row0 + r >= 2) && (row0 + r < Mp)) << r;
    L.rowvalid = rv;
    L.key0 = (uint32_t)row0 << 16;
    L.w1 = L.w2 = 0;
    L.h1 = L.h2 = DpAboveT{0.0f, 0.0f, 0u, 0u, 0u};
    float qa[R], qb[R], qc[R];
    uint32_t oa[R], ob[R], oc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      qa[r] = qb[r] = qc[r] = 0.0f;
      oa[r] = ob[r] = oc[r] = 0u;
    }
    DpAboveT pub{0.0f, 0.0f, 0u, 0u, 0u};
    const int S_end = Np + 63;
    const bool lane_active = row0 < Mp;
    auto fetch = [&](int c) -> uint32_t {
      if (!(lane_active && c >= 0 && c < Np)) return 0u;
      return (mrow[c] >> sh) & ((1u << R) - 1u);
    };
    auto recv = [&](const DpAboveT& mine, int c) -> DpAboveT {
      DpAboveT h;
      h.q30 = __shfl_up(mine.q30, 1);
      h.q31 = __shfl_up(mine.q31, 1);
      h.b = (uint32_t)__shfl_up((int)mine.b, 1);
      h.o30 = (uint32_t)__shfl_up((int)mine.o30, 1);
      h.o31 = (uint32_t)__shfl_up((int)mine.o31, 1);
      if (lane == 0) {
        if (band > 0 && c >= 0 && c < Np) {
          const float4 q = bin[c].q;
          const uint4 o = bin[c].o;
          h = DpAboveT{q.x, q.y, (uint32_t)q.z, o.x, o.y};
        } else {
          h = DpAboveT{0.0f, 0.0f, 0u, 0u, 0u};
        }
      }
      return h;
    };
    auto publish = [&](const DpAboveT& o, int c) {
      if (lane == 63 && band + 1 < nbands && c >= 0 && c < Np) {
        bout[c].q = make_float4(o.q30, o.q31, (float)o.b, 0.0f);
        bout[c].o = make_uint4(o.o30, o.o31, 0u, 0u);
      }
    };
    uint32_t wnext = fetch(-lane);
    for (int s = 0; s < S_end; s += 3) {
      {
        const int c = s - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAboveT h0 = recv(pub, c);
        pub = L.step(qa, oa, qb, ob, qc, oc, w0, h0, c);
        publish(pub, c);
      }
      if (s + 1 < S_end) {
        const int c = s + 1 - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAboveT h0 = recv(pub, c);
        pub = L.step(qc, oc, qa, oa, qb, ob, w0, h0, c);
        publish(pub, c);
      }
      if (s + 2 < S_end) {
        const int c = s + 2 - lane;
        const uint32_t w0 = wnext;
        wnext = fetch(c + 1);
        const DpAboveT h0 = recv(pub, c);
        pub = L.step(qb, ob, qc, oc, qa, oa, w0, h0, c);
        publish(pub, c);
      }
    }
    __threadfence_block();
    __syncthreads();
  }
  // wave reduction of (best, end key, origin) by the same rule as the per-cell update
  float best = L.best;
  uint32_t bkey = L.bkey, borg = L.borg;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v = __shfl_xor(best, o);
    const uint32_t k = (uint32_t)__shfl_xor((int)bkey, o);
    const uint32_t g = (uint32_t)__shfl_xor((int)borg, o);
    if (v > best || (v == best && v > 0.0f && k < bkey)) {
      best = v;
      bkey = k;
      borg = g;
    }
  }
  if (lane == 0) {
    if (qmax_out) qmax_out[p] = best;
    const bool any = best > 0.0f;
    int32_t* sg = seg_out + 4 * (size_t)p;
    sg[0] = any ? (int)(borg >> 16) : -1;
    sg[1] = any ? (int)(borg & 0xffffu) : -1;
    sg[2] = any ? (int)(bkey >> 16) : -1;
    sg[3] = any ? (int)(bkey & 0xffffu) : -1;
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

int check_params(const acoss_crp_params* P) {
  if (!P) {
    set_error("params is NULL");
    return ACOSS_E_ARG;
  }
  if (P->m < 1 || P->m > 64 || P->tau < 1 || !(P->kappa >= 0.0f && P->kappa <= 1.0f)) {
    set_error("unsupported params m=%d tau=%d kappa=%g", P->m, P->tau, (double)P->kappa);
    return ACOSS_E_ARG;
  }
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

template <int ALIGN, int R>
void launch_dp_r(bool eqg, int nb, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
                 float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s, int L = 0) {
  const float k2 = 2.0f * go;
  static const bool no_fast = getenv("ACOSS_DP_NOFAST") != nullptr;
  static const bool no_grp = getenv("ACOSS_DP_NOGROUP") != nullptr;
  const int LP = (L + 31) / 32;  // lanes per pair at 32 rows per lane
  if (ALIGN == 0 && eqg && !no_fast && !no_grp && k2 >= 0.0f && k2 <= 1024.0f && k2 == floorf(k2) && L > 0 &&
      LP <= 21) {  // three or more pairs per wave (two per wave measured slower at L ~ 1000)
    const int G = 64 / LP;
    hipLaunchKernelGGL(k_crp_dp_grp, dim3((unsigned)((nb + G - 1) / G)), dim3(64), 0, s, maskT, mstride, ld, dims, nb,
                       LP, go, out);
  } else if (ALIGN == 0 && eqg && !no_fast && k2 >= 0.0f && k2 <= 1024.0f && k2 == floorf(k2))
    hipLaunchKernelGGL((k_crp_dp_fast<R>), dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, go, ge,
                       bnd, bstride, out);
  else if (eqg)
    hipLaunchKernelGGL((k_crp_dp<ALIGN, true, R>), dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, go, ge, bnd,
                       bstride, out);
  else
    hipLaunchKernelGGL((k_crp_dp<ALIGN, false, R>), dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, go, ge, bnd,
                       bstride, out);
}

// The packed 16-bit DP (k_crp_dp_pk) is exact when gamma_open == gamma_ext is a multiple of 1/2
// and every doubled score fits 16 bits: scores grow by at most 2 per column (chen17), so 2Q < 4L.
inline bool dp_packed_ok(bool eqg, int L, float go) {
  static const bool off = getenv("ACOSS_DP_F32") != nullptr;
  const float k2 = 2.0f * go;
  return !off && eqg && L <= 16000 && k2 >= 0.0f && k2 <= 1024.0f && k2 == floorf(k2);
}

// Rows per lane from the batch's longest CRP (L rows): every choice below 2048 rows is one band,
// so the band-boundary buffer (ceil(L / 2048) bands) always suffices.
template <int ALIGN>
void launch_dp(bool eqg, int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go,
               float ge, float4* bnd, int64_t bstride, float* out, hipStream_t s) {
  if (L <= 512)
    launch_dp_r<ALIGN, 8>(eqg, nb, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s, L);
  else if (L <= 1024)
    launch_dp_r<ALIGN, 16>(eqg, nb, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s, L);
  else if (ALIGN == 1 && dp_packed_ok(eqg, L, go))
    hipLaunchKernelGGL(k_crp_dp_pk<ALIGN>, dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, (unsigned)(2.0f * go), bnd,
                       bstride, out);
  else
    launch_dp_r<ALIGN, 32>(eqg, nb, maskT, mstride, ld, dims, go, ge, bnd, bstride, out, s);
}

// The tracing DP (k_crp_dp_trace): R = 8 takes the CRPs of at most 512 rows, R = 16 the longer
// ones; a batch whose longest CRP has more than 512 rows gets both launches and each wave keeps
// the pairs of its own R. The exact-halves select (EQG) under the fast DP's condition only.
constexpr int kTraceShortRows = 512;
constexpr int kTraceMaxLen = 65535;  // 16 bits per coordinate of a packed cell

inline int64_t trace_bnd_records(int L, int ld) {  // per pair: ceil(L / (64 R)) * ld
  return L <= kTraceShortRows ? (int64_t)ld : (int64_t)((L + 64 * 16 - 1) / (64 * 16)) * ld;
}

template <int R>
void launch_trace_r(int nb, int row_lo, int row_hi, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims,
                    float go, float ge, TraceRec* bnd, int64_t bstride, float* qmax, int32_t* seg, hipStream_t s) {
  const float k2 = 2.0f * go;
  if (go == ge && k2 >= 0.0f && k2 <= 1024.0f && k2 == floorf(k2))
    hipLaunchKernelGGL((k_crp_dp_trace<true, R>), dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, row_lo, row_hi, go,
                       ge, bnd, bstride, qmax, seg);
  else
    hipLaunchKernelGGL((k_crp_dp_trace<false, R>), dim3(nb), dim3(64), 0, s, maskT, mstride, ld, dims, row_lo, row_hi,
                       go, ge, bnd, bstride, qmax, seg);
}

void launch_trace(int nb, int L, const uint32_t* maskT, int64_t mstride, int ld, const int2* dims, float go, float ge,
                  TraceRec* bnd, int64_t bstride, float* qmax, int32_t* seg, hipStream_t s) {
  launch_trace_r<8>(nb, -1, kTraceShortRows, maskT, mstride, ld, dims, go, ge, bnd, bstride, qmax, seg, s);
  if (L > kTraceShortRows)
    launch_trace_r<16>(nb, kTraceShortRows, INT32_MAX, maskT, mstride, ld, dims, go, ge, bnd, bstride, qmax, seg, s);
}

// Per-track tables of one call, in workspace slot 0: prof (n_tracks x 12) | NX (n_tracks x ldn) |
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
  float* ws = static_cast<float*>(workspace(0, (base + (size_t)n_tracks * ldn * 24) * sizeof(float)));
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
// pitches its kernels index with, and workspace slot 1 carved to them. acoss_crp_align and
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

int crp_plan(int m, int tau, int max_len, int64_t n_pairs, hipStream_t s, CrpPlan& P) {
  const int L = stacked_len(max_len, m, tau);
  if (L <= 0) {
    set_error("max_len %d too short for m=%d tau=%d", max_len, m, tau);
    return ACOSS_E_SHAPE;
  }
  P.m = m;
  P.tau = tau;
  P.L = L;
  const int ld = P.ld = (int)align_up((size_t)L, 8);  // x16 B = 128 B: band rows never share a cache line
  P.R = pick_R(m, ld);
  if (P.R <= 0) {
    set_error("track too long for the LDS stripe (stacked length %d)", ld);
    return ACOSS_E_SHAPE;
  }
  P.sel_lds = select_lds_bytes(P.R, m, ld);
  P.pan_lds = panel_lds_floats(32, m) * sizeof(float);
  int rc;
  if ((rc = set_lds(k_crp_select<false>, P.sel_lds))) return rc;
  if ((rc = set_lds(k_crp_select<true>, P.sel_lds))) return rc;
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
  P.split = m == 9 && tau == 1 && L <= 4096 && !(path_env && strcmp(path_env, "generic") == 0);
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
  char* ws = static_cast<char*>(workspace(1, slot * nb_alloc + P.nbuf * sub_pair * P.sub + 8192));
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
// between the split path and the generic kernels.
int crp_masks(const CrpPlan& C, const TrackPrep& T, const int32_t* pb, int nb, const acoss_crp_params* params,
              hipStream_t s) {
  int rc;
  prof_begin(PH_OTI, s);
  hipLaunchKernelGGL(k_pair_oti, dim3((nb + 255) / 256), dim3(256), 0, s, T.prof, T.len, pb, (int64_t)nb, params->oti,
                     C.m, C.tau, C.oti, C.dims);
  ACOSS_LAUNCH_CHECK();
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

}  // namespace

}  // namespace acoss

using namespace acoss;

extern "C" int acoss_crp_align(const float* feats, const int64_t* track_off, const int32_t* track_len,
                               int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                               const acoss_crp_params* params, float* qmax_out, float* dmax_out, int32_t* oti_out,
                               void* hip_stream) {
  clear_error();
  int rc = check_params(params);
  if (rc) return rc;
  if (n_pairs < 0 || n_tracks < 0 || max_len < 0) {
    set_error("negative size");
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  if (!feats || !track_off || !track_len || !pairs) {
    set_error("NULL input pointer");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  CrpPlan C;
  if ((rc = crp_plan(params->m, params->tau, max_len, n_pairs, s, C))) return rc;
  TrackPrep T;
  prof_begin(PH_PREP, s);
  if ((rc = run_prep(feats, track_off, track_len, n_tracks, max_len, C.m, C.tau, s, &T))) return rc;
  prof_end(PH_PREP, s);

  const bool eqg = params->gamma_open == params->gamma_ext;
  for (int64_t base = 0; base < n_pairs; base += C.nb_alloc) {
    const int nb = (int)((n_pairs - base) < C.nb_alloc ? (n_pairs - base) : C.nb_alloc);
    if ((rc = crp_masks(C, T, pairs + 2 * base, nb, params, s))) return rc;
    if (qmax_out) {
      prof_begin(PH_DP_QMAX, s);
      launch_dp<0>(eqg, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims, params->gamma_open, params->gamma_ext, C.bnd,
                   C.bnd_stride, qmax_out + base, s);
      ACOSS_LAUNCH_CHECK();
      prof_end(PH_DP_QMAX, s);
    }
    if (dmax_out) {
      prof_begin(PH_DP_DMAX, s);
      launch_dp<1>(eqg, nb, C.L, C.mask, C.mask_stride, C.ld, C.dims, params->gamma_open, params->gamma_ext, C.bnd,
                   C.bnd_stride, dmax_out + base, s);
      ACOSS_LAUNCH_CHECK();
      prof_end(PH_DP_DMAX, s);
    }
    if (oti_out) ACOSS_HIP_CHECK(hipMemcpyAsync(oti_out + base, C.oti, 4 * nb, hipMemcpyDeviceToDevice, s));
  }
  return ACOSS_OK;
}

extern "C" int acoss_crp_pair(const float* X, int32_t M, const float* Y, int32_t N, const acoss_crp_params* params,
                              float* dist, float* thr_row, float* thr_col, uint8_t* crp, int32_t* oti,
                              void* hip_stream) {
  clear_error();
  int rc = check_params(params);
  if (rc) return rc;
  const int m = params->m, tau = params->tau;
  const int Mp = stacked_len(M, m, tau), Np = stacked_len(N, m, tau);
  if (Mp <= 0 || Np <= 0) {
    set_error("track too short: M=%d N=%d m=%d tau=%d", M, N, m, tau);
    return ACOSS_E_SHAPE;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  // the pair as a corpus of two tracks and a batch of one pair: packed features and the tables a
  // caller of acoss_crp_align passes in, in workspace slot 2
  const int max_len = M > N ? M : N;
  CrpPlan C;
  if ((rc = crp_plan(m, tau, max_len, 1, s, C))) return rc;
  const size_t fbytes = align_up((size_t)(M + N) * 12 * 4, 256);
  char* ws = static_cast<char*>(workspace(2, fbytes + 256));
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
  if ((rc = crp_masks(C, T, d_pairs, 1, params, s))) return rc;
  if (dist) {
    hipLaunchKernelGGL(k_crp_panel<1>, dim3((Np + kPanelW - 1) / kPanelW, C.nstrips, 1), dim3(256), C.pan_lds, s,
                       batch_view(C, T, d_pairs, 0), C.T_r, C.T_c, C.thr_stride, C.mask, C.mask_stride, C.ld, dist);
    ACOSS_LAUNCH_CHECK();
  }
  if (crp) {
    hipLaunchKernelGGL(k_unpack_mask, dim3((Np + 255) / 256, Mp), dim3(256), 0, s, C.mask, C.ld, Mp, Np, crp);
    ACOSS_LAUNCH_CHECK();
  }
  if (thr_row) ACOSS_HIP_CHECK(hipMemcpyAsync(thr_row, C.thr_r, 4 * (size_t)Mp, hipMemcpyDeviceToDevice, s));
  if (thr_col) ACOSS_HIP_CHECK(hipMemcpyAsync(thr_col, C.thr_c, 4 * (size_t)Np, hipMemcpyDeviceToDevice, s));
  if (oti) ACOSS_HIP_CHECK(hipMemcpyAsync(oti, C.oti, 4, hipMemcpyDeviceToDevice, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  return ACOSS_OK;
}

extern "C" int acoss_align_crp(const uint8_t* crp, int32_t M, int32_t N, int32_t align, float gamma_open,
                               float gamma_ext, float* score_out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || (align != 0 && align != 1) || !score_out) {
    set_error("bad arguments to acoss_align_crp");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (M == 0 || N == 0) {
    const float z = 0.0f;
    ACOSS_HIP_CHECK(hipMemcpyAsync(score_out, &z, 4, hipMemcpyHostToDevice, s));
    ACOSS_HIP_CHECK(hipStreamSynchronize(s));
    return ACOSS_OK;
  }
  const int ld = (int)align_up((size_t)N, 8);
  const int nstrips = (M + 31) / 32, nbands = (M + 2047) / 2048;
  const size_t bytes = 256 + 4 * (size_t)nstrips * ld + 16 * (size_t)nbands * ld;
  char* ws = static_cast<char*>(workspace(3, bytes));
  if (!ws) return ACOSS_E_HIP;
  int* d_err = reinterpret_cast<int*>(ws);
  int2* d_dims = reinterpret_cast<int2*>(ws + 64);
  uint32_t* maskT = reinterpret_cast<uint32_t*>(ws + 256);
  float4* bnd = reinterpret_cast<float4*>(ws + 256 + 4 * (size_t)nstrips * ld);
  const int h_hdr[4] = {0, 0, M, N};  // err, pad, dims
  ACOSS_HIP_CHECK(hipMemcpy(d_err, h_hdr, 8, hipMemcpyHostToDevice));
  ACOSS_HIP_CHECK(hipMemcpy(d_dims, h_hdr + 2, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_pack_mask, dim3((N + 255) / 256, nstrips), dim3(256), 0, s, crp, M, N, ld, maskT, d_err);
  ACOSS_LAUNCH_CHECK();
  const bool eqg = gamma_open == gamma_ext;
  if (align == 0)
    launch_dp<0>(eqg, 1, M, maskT, 0, ld, d_dims, gamma_open, gamma_ext, bnd, 0, score_out, s);
  else
    launch_dp<1>(eqg, 1, M, maskT, 0, ld, d_dims, gamma_open, gamma_ext, bnd, 0, score_out, s);
  ACOSS_LAUNCH_CHECK();
  int h_err = 0;
  ACOSS_HIP_CHECK(hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_err) {
    set_error("CoverSongSimilarity: non-binary elements found in the input similarity matrix");
    return ACOSS_E_NONBINARY;
  }
  return ACOSS_OK;
}

extern "C" int acoss_crp_locate(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                int32_t n_tracks, int32_t max_len, const int32_t* pairs, int64_t n_pairs,
                                const acoss_crp_params* params, float* qmax_out, int32_t* seg_out, int32_t* oti_out,
                                void* hip_stream) {
  clear_error();
  int rc = check_params(params);
  if (rc) return rc;
  if (n_pairs < 0 || n_tracks < 0 || max_len < 0) {
    set_error("negative size");
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  if (!feats || !track_off || !track_len || !pairs || !seg_out) {
    set_error("NULL input pointer or seg_out");
    return ACOSS_E_ARG;
  }
  if (stacked_len(max_len, params->m, params->tau) > kTraceMaxLen) {
    set_error("stacked length %d above %d: a packed cell has 16 bits per coordinate",
              stacked_len(max_len, params->m, params->tau), kTraceMaxLen);
    return ACOSS_E_SHAPE;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  CrpPlan C;
  if ((rc = crp_plan(params->m, params->tau, max_len, n_pairs, s, C))) return rc;
  TrackPrep T;
  prof_begin(PH_PREP, s);
  if ((rc = run_prep(feats, track_off, track_len, n_tracks, max_len, C.m, C.tau, s, &T))) return rc;
  prof_end(PH_PREP, s);
  // band-boundary records of the tracing DP, in a slot of their own (crp_plan's carving is the
  // shipped DP's)
  const int64_t tstride = trace_bnd_records(C.L, C.ld);
  TraceRec* tb = static_cast<TraceRec*>(workspace(22, sizeof(TraceRec) * (size_t)tstride * (size_t)C.nb_alloc));
  if (!tb) return ACOSS_E_HIP;

  for (int64_t base = 0; base < n_pairs; base += C.nb_alloc) {
    const int nb = (int)((n_pairs - base) < C.nb_alloc ? (n_pairs - base) : C.nb_alloc);
    if ((rc = crp_masks(C, T, pairs + 2 * base, nb, params, s))) return rc;
    prof_begin(PH_DP_TRACE, s);
    launch_trace(nb, C.L, C.mask, C.mask_stride, C.ld, C.dims, params->gamma_open, params->gamma_ext, tb, tstride,
                 qmax_out ? qmax_out + base : nullptr, seg_out + 4 * base, s);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_DP_TRACE, s);
    if (oti_out) ACOSS_HIP_CHECK(hipMemcpyAsync(oti_out + base, C.oti, 4 * nb, hipMemcpyDeviceToDevice, s));
  }
  return ACOSS_OK;
}

extern "C" int acoss_locate_crp(const uint8_t* crp, int32_t M, int32_t N, float gamma_open, float gamma_ext,
                                float* score_out, int32_t* seg_out, void* hip_stream) {
  clear_error();
  if (M < 0 || N < 0 || !score_out || !seg_out) {
    set_error("bad arguments to acoss_locate_crp");
    return ACOSS_E_ARG;
  }
  if (M > kTraceMaxLen || N > kTraceMaxLen) {
    set_error("matrix %d x %d above %d rows or columns: a packed cell has 16 bits per coordinate", M, N, kTraceMaxLen);
    return ACOSS_E_SHAPE;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  if (M == 0 || N == 0) {
    const float z = 0.0f;
    const int32_t none[4] = {-1, -1, -1, -1};
    ACOSS_HIP_CHECK(hipMemcpyAsync(score_out, &z, 4, hipMemcpyHostToDevice, s));
    ACOSS_HIP_CHECK(hipMemcpyAsync(seg_out, none, sizeof(none), hipMemcpyHostToDevice, s));
    ACOSS_HIP_CHECK(hipStreamSynchronize(s));
    return ACOSS_OK;
  }
  const int ld = (int)align_up((size_t)N, 8);
  const int nstrips = (M + 31) / 32;
  const int64_t trecs = trace_bnd_records(M, ld);
  const size_t mask_bytes = align_up(4 * (size_t)nstrips * ld, 256);
  char* ws = static_cast<char*>(workspace(23, 256 + mask_bytes + sizeof(TraceRec) * (size_t)trecs));
  if (!ws) return ACOSS_E_HIP;
  int* d_err = reinterpret_cast<int*>(ws);
  int2* d_dims = reinterpret_cast<int2*>(ws + 64);
  uint32_t* maskT = reinterpret_cast<uint32_t*>(ws + 256);
  TraceRec* bnd = reinterpret_cast<TraceRec*>(ws + 256 + mask_bytes);
  const int h_hdr[4] = {0, 0, M, N};  // err, pad, dims
  ACOSS_HIP_CHECK(hipMemcpy(d_err, h_hdr, 8, hipMemcpyHostToDevice));
  ACOSS_HIP_CHECK(hipMemcpy(d_dims, h_hdr + 2, 8, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_pack_mask, dim3((N + 255) / 256, nstrips), dim3(256), 0, s, crp, M, N, ld, maskT, d_err);
  ACOSS_LAUNCH_CHECK();
  launch_trace(1, M, maskT, 0, ld, d_dims, gamma_open, gamma_ext, bnd, 0, score_out, seg_out, s);
  ACOSS_LAUNCH_CHECK();
  int h_err = 0;
  ACOSS_HIP_CHECK(hipMemcpyAsync(&h_err, d_err, 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_err) {
    set_error("CoverSongSimilarity: non-binary elements found in the input similarity matrix");
    return ACOSS_E_NONBINARY;
  }
  return ACOSS_OK;
}
