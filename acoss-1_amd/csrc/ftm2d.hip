// ftm2d.hip — the FTM2D algorithm: beat-synchronous 2-D Fourier magnitude shingles and their pair
// scores (acoss/algorithms/ftm2d.py:52-66, 85-97, 100-138).
//
//   k_ftm_beatsync   steps 1-2: one float32 median per (segment, chroma bin) between consecutive
//                    boundaries (librosa.util.sync(hpcp.T, onsets, aggregate=np.median), :58; the
//                    selection and the even-count mean are features.hip's, i.e. np.median's on
//                    float32), then chrompwr (:100-117) in float64 per beat column.
//   k_ftm_winnorm    the L2 norm of every window's 900 magnitudes (:62-63) by Parseval:
//                    norm^2 = 900 * sum(patch^2). The sum is taken directly over the window's 75
//                    column energies, so it is 0 for exactly the all-zero windows (Norm == 0 -> 1).
//   k_ftm_shingle    steps 3-4 (:134-137, :64). |F[c, k]| = |F[-c, -k]| for a real patch, so only the
//                    chroma-frequency rows c = 0..6 are computed (525 of 900 coefficients). Per
//                    track Z = W12 . X (row c, complex) is formed in LDS; the 75-point time-axis DFT
//                    of every sliding window is then a GEMM on v_mfma_f64_16x16x4_f64:
//                    A[i, t] = (Re Z[c, i + t] | Im Z[c, i + t]) is a Hankel matrix read straight
//                    out of the LDS row, B the real 152 x (2 x 80) twiddle matrix (75 + 1 zero row
//                    per part, 75 + 5 zero columns), 16 windows on the M axis per tile. A block owns
//                    one (row c, tile of 16 frequencies) and keeps that twiddle slice in LDS while it
//                    walks over its share of the tracks. log(C |F| / norm + 1) goes to the workspace,
//                    coefficient-major.
//   k_ftm_median     step 5 (:65): LDS bitonic sort of one coefficient's nw values, the median.
//   k_ftm_finish     step 5 (:66): mirror rows 7..11 and fftshift (:136) when writing the 900
//                    entries, divided by the L2 norm of the 900 medians (0 / 0 = NaN for a silent
//                    track, as the reference).
//   k_ftm_scores     exp(-sum (s1 - s2)^2) per pair (:93-96), one wave per pair, the differences
//                    summed in one fixed order; the query shingle stays in registers over
//                    consecutive pairs that share it.
//   k_ftm_topk       the same scores fused with a per-query k-best selection (not in the reference:
//                    the shortlist that spares the alignment scorers); four queries per wave in
//                    registers, each reference row read once for all four, the running k best of a
//                    query in LDS; the query x reference scores are never stored.
// Every per-track result depends on that track's data only (fixed summation orders, exact sorts),
// so a track's shingle does not depend on the batch it is computed in.
#include <cmath>
#include <mutex>
#include <vector>

#include "common.hpp"

namespace acoss {

namespace {

constexpr int kWin = 75;                        // beats per window: the twiddle size is a compile-time constant
constexpr int kMaxWindows = 4096;               // windows per track (LDS sort size), as SiMPle caps frames
constexpr int kMaxBeats = kMaxWindows + kWin - 1;  // 4170
constexpr int kRows = 7;                        // chroma-frequency rows computed (c = 0..6)
constexpr int kCoef = kRows * kWin;             // 525 coefficients computed per window
constexpr int kDim = 12 * kWin;                 // 900
constexpr int kKHalf = 76;                      // GEMM K per part (Re | Im): 75 + 1 zero row = 19 MFMA steps
constexpr int kK = 2 * kKHalf;
constexpr int kKT = 5;                          // tiles of 16 frequencies (80 >= 75)
constexpr int kTwRow = 17;                      // LDS twiddle row stride in (re, im) pairs: 16 + 1 pad
constexpr int kTwDoubles = kKT * kK * 16 * 2;   // twiddles, then cos / sin of the 12-point DFT
constexpr int kTwTotal = kTwDoubles + 24;
constexpr int kSegCols = 64;                    // beat columns per k_ftm_beatsync block
constexpr int kLongSeg = 64;                    // segments longer than this are selected by a whole wave
constexpr int64_t kChunkWindows = 131072;       // windows per pass through the workspace (550 MB)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Track t's boundaries are bounds[bound_off[t] .. bound_off[t + 1]): nb = count - 1 beat columns at
// column offset bound_off[t] - t, nw = nb - 74 windows at window offset bound_off[t] - 75 t.
__device__ __forceinline__ float chroma_at(const float* X, int64_t frame, int c) { return X[frame * 12 + c]; }

// median of X[a .. a + cnt) in bin c by rank counting: the values of rank (cnt - 1) / 2 and cnt / 2,
// then features.hip's arithmetic. One thread.
__device__ float seg_median_thread(const float* X, int64_t a, int cnt, int c) {
  const int k1 = (cnt - 1) / 2, k2 = cnt / 2;
  float lo = 0.0f, hi = 0.0f;
  bool nan = false;
  for (int i = 0; i < cnt; ++i) {
    const float x = chroma_at(X, a + i, c);
    nan |= x != x;
    int lt = 0, le = 0;
    for (int j = 0; j < cnt; ++j) {
      const float y = chroma_at(X, a + j, c);
      lt += y < x;
      le += y <= x;
    }
    if (lt <= k1 && k1 < le) lo = x;
    if (lt <= k2 && k2 < le) hi = x;
  }
  if (nan) return __builtin_nanf("");
  return (cnt & 1) ? lo : (lo + hi) / 2.0f;
}

// the same by one wave: the lanes share the candidates
__device__ float seg_median_wave(const float* X, int64_t a, int cnt, int c, int lane) {
  const int k1 = (cnt - 1) / 2, k2 = cnt / 2;
  float lo = 0.0f, hi = 0.0f;
  bool flo = false, fhi = false, nan = false;
  for (int i = lane; i < cnt; i += 64) {
    const float x = chroma_at(X, a + i, c);
    nan |= x != x;
    int lt = 0, le = 0;
    for (int j = 0; j < cnt; ++j) {
      const float y = chroma_at(X, a + j, c);
      lt += y < x;
      le += y <= x;
    }
    if (lt <= k1 && k1 < le) {
      lo = x;
      flo = true;
    }
    if (lt <= k2 && k2 < le) {
      hi = x;
      fhi = true;
    }
  }
  const unsigned long long mnan = __ballot(nan), mlo = __ballot(flo), mhi = __ballot(fhi);
  if (mnan || !mlo || !mhi) return __builtin_nanf("");
  lo = __shfl(lo, __ffsll((long long)mlo) - 1);
  hi = __shfl(hi, __ffsll((long long)mhi) - 1);
  return (cnt & 1) ? lo : (lo + hi) / 2.0f;
}

__global__ __launch_bounds__(256) void k_ftm_beatsync(const float* __restrict__ feats, const int64_t* __restrict__ off,
                                                      const int32_t* __restrict__ len, const int64_t* __restrict__ bounds,
                                                      const int64_t* __restrict__ bound_off, double pwr,
                                                      float* __restrict__ sync_out, double* __restrict__ chroma,
                                                      double* __restrict__ col_energy) {
  __shared__ float smed[12][kSegCols];
  const int tr = blockIdx.x;
  const int64_t b0 = bound_off[tr];
  const int nb = (int)(bound_off[tr + 1] - b0) - 1;
  const int j0 = blockIdx.y * kSegCols;
  if (j0 >= nb) return;  // whole block
  const int ncol = min(kSegCols, nb - j0);
  const int n = len[tr];
  const float* X = feats + off[tr] * 12;
  const int64_t* B = bounds + b0;
  const int64_t coloff = b0 - tr;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  auto seg = [&](int j, int64_t& a, int& cnt) {  // clamped to the track whatever the caller passed
    a = min(max(B[j0 + j], (int64_t)0), (int64_t)n);
    const int64_t b = min(max(B[j0 + j + 1], a), (int64_t)n);
    cnt = (int)(b - a);
  };
  for (int e = tid; e < ncol * 12; e += 256) {
    const int j = e / 12, c = e - j * 12;
    int64_t a;
    int cnt;
    seg(j, a, cnt);
    if (cnt <= kLongSeg) smed[c][j] = cnt > 0 ? seg_median_thread(X, a, cnt, c) : __builtin_nanf("");
  }
  for (int j = 0; j < ncol; ++j) {  // block-uniform
    int64_t a;
    int cnt;
    seg(j, a, cnt);
    if (cnt <= kLongSeg) continue;
    for (int c = wave; c < 12; c += 4) {
      const float m = seg_median_wave(X, a, cnt, c, lane);
      if (lane == 0) smed[c][j] = m;
    }
  }
  __syncthreads();
  if (sync_out)
    for (int e = tid; e < ncol * 12; e += 256) {
      const int c = e / ncol, j = e - c * ncol;
      sync_out[coloff * 12 + (int64_t)c * nb + j0 + j] = smed[c][j];
    }
  if (tid < ncol) {  // chrompwr of one beat column (ftm2d.py:100-117)
    double x[12];
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      x[c] = (double)smed[c][tid];
      s = s + x[c] * x[c];
    }
    double n1 = sqrt(s);
    if (n1 == 0.0) n1 = 1.0;
    double s2 = 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      x[c] = pow(x[c] / n1, pwr);
      s2 = s2 + x[c] * x[c];
    }
    double n2 = sqrt(s2);
    if (n2 == 0.0) n2 = 1.0;
    double en = 0.0;
#pragma unroll
    for (int c = 0; c < 12; ++c) {
      const double y = n1 * (x[c] / n2);
      chroma[coloff * 12 + (int64_t)c * nb + j0 + tid] = y;
      en = en + y * y;
    }
    if (col_energy) col_energy[coloff + j0 + tid] = en;
  }
}

__global__ void k_ftm_winnorm(const double* __restrict__ col_energy, const int64_t* __restrict__ bound_off,
                              double* __restrict__ wnorm) {
  const int tr = blockIdx.x;
  const int64_t b0 = bound_off[tr];
  const int nw = (int)(bound_off[tr + 1] - b0) - kWin;
  const int i = blockIdx.y * blockDim.x + threadIdx.x;
  if (i >= nw) return;
  const double* E = col_energy + (b0 - tr) + i;
  double s = 0.0;
  for (int t = 0; t < kWin; ++t) s = s + E[t];
  double nrm = sqrt((double)kDim * s);
  if (nrm == 0.0) nrm = 1.0;
  wnorm[b0 - (int64_t)kWin * tr + i] = nrm;
}

// grid (7 rows x 5 frequency tiles, track groups); block 256 = 4 waves, a wave per 32 windows.
// MFMA operands (simple.hip): A lane holds A[row = lane & 15][k = lane >> 4], B lane B[k = lane >> 4]
// [col = lane & 15], result register r holds D[4 r + (lane >> 4)][lane & 15].
__global__ __launch_bounds__(256) void k_ftm_shingle(const double* __restrict__ chroma, const double* __restrict__ wnorm,
                                                     const int64_t* __restrict__ bound_off,
                                                     const double* __restrict__ tw, int t0, int t1, int zlen, double C,
                                                     double* __restrict__ V) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double2* Bs = reinterpret_cast<double2*>(sm);  // [kK][kTwRow] (re, im)
  double* Zr = sm + kK * kTwRow * 2;
  double* Zi = Zr + zlen;
  const int c = blockIdx.x / kKT, kt = blockIdx.x - c * kKT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const double2* twp = reinterpret_cast<const double2*>(tw) + (size_t)kt * kK * 16;
  for (int e = tid; e < kK * 16; e += 256) Bs[(e >> 4) * kTwRow + (e & 15)] = twp[e];
  const double* w12 = tw + kTwDoubles;
  const bool real_row = c == 0 || c == 6;  // Z's row is real: the Im half of K adds nothing
  const int nsteps = real_row ? kKHalf / 4 : kK / 4;
  const int64_t w00 = bound_off[t0] - (int64_t)kWin * t0;
  for (int t = t0 + blockIdx.y; t < t1; t += gridDim.y) {
    const int64_t b0 = bound_off[t];
    const int nb = (int)(bound_off[t + 1] - b0) - 1;
    const int nw = nb - kWin + 1;
    const double* X = chroma + (b0 - t) * 12;
    const int64_t woff = b0 - (int64_t)kWin * t;
    const double* wn = wnorm + woff;
    double* Vt = V + (woff - w00) * kCoef;
    __syncthreads();  // the previous track's reads of Z are done
    for (int j = tid; j < zlen; j += 256) {
      double zr = 0.0, zi = 0.0;
      if (j < nb) {
#pragma unroll
        for (int b = 0; b < 12; ++b) {
          const int m = (c * b) % 12;
          const double x = X[(size_t)b * nb + j];
          zr = zr + x * w12[m];
          zi = zi - x * w12[12 + m];
        }
      }
      Zr[j] = zr;
      Zi[j] = real_row ? 0.0 : zi;
    }
    __syncthreads();
    const int ntile = (nw + 31) / 32;
    for (int p = wave; p < ntile; p += 4) {
      const int i0 = 32 * p;
      f64x4 re0 = {0.0, 0.0, 0.0, 0.0}, im0 = re0, re1 = re0, im1 = re0;
      for (int s = 0; s < nsteps; ++s) {
        const double* Zp = s < kKHalf / 4 ? Zr : Zi;
        const int sb = s < kKHalf / 4 ? s : s - kKHalf / 4;
        const double a0 = Zp[i0 + li + 4 * sb + lk];
        const double a1 = Zp[i0 + 16 + li + 4 * sb + lk];
        const double2 b = Bs[(4 * s + lk) * kTwRow + li];
        re0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b.x, re0, 0, 0, 0);
        im0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b.y, im0, 0, 0, 0);
        re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b.x, re1, 0, 0, 0);
        im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b.y, im1, 0, 0, 0);
      }
      const int k = kt * 16 + li;
      if (k < kWin) {
        double* Vc = Vt + (size_t)(c * kWin + k) * nw;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 4 * r + lk;
          if (i < nw) {
            const double mag = sqrt(re0[r] * re0[r] + im0[r] * im0[r]);
            Vc[i] = log(C * mag / wn[i] + 1.0);
          }
          if (i + 16 < nw) {
            const double mag = sqrt(re1[r] * re1[r] + im1[r] * im1[r]);
            Vc[i + 16] = log(C * mag / wn[i + 16] + 1.0);
          }
        }
      }
    }
  }
}

// grid (tracks of the chunk, 525), one wave: sort the coefficient's nw values, padded with +inf
__global__ __launch_bounds__(64) void k_ftm_median(const double* __restrict__ V, const int64_t* __restrict__ bound_off,
                                                   int t0, double* __restrict__ med) {
  extern __shared__ double sv[];
  const int t = t0 + blockIdx.x, coef = blockIdx.y;
  const int64_t b0 = bound_off[t];
  const int nw = (int)(bound_off[t + 1] - b0) - kWin;
  const int64_t w00 = bound_off[t0] - (int64_t)kWin * t0;
  const double* src = V + (b0 - (int64_t)kWin * t - w00) * kCoef + (size_t)coef * nw;
  int n2 = 2;
  while (n2 < nw) n2 <<= 1;
  const int tid = threadIdx.x;
  for (int i = tid; i < n2; i += 64) sv[i] = i < nw ? src[i] : __builtin_inf();
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += 64) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const double a = sv[i], b = sv[ixj];
          const bool up = (i & kk) == 0;
          if ((a > b) == up) {
            sv[i] = b;
            sv[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
  }
  if (tid == 0) med[(size_t)t * kCoef + coef] = (nw & 1) ? sv[nw / 2] : 0.5 * (sv[nw / 2 - 1] + sv[nw / 2]);
}

// block per track: entry (r, q) of the fftshift-ed 12 x 75 patch is |F[(r + 6) % 12][(q + 38) % 75]|
__global__ __launch_bounds__(256) void k_ftm_finish(const double* __restrict__ med, double* __restrict__ out) {
  __shared__ double red[256];
  const int t = blockIdx.x, tid = threadIdx.x;
  const double* M = med + (size_t)t * kCoef;
  double v[4];
  double s = 0.0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid + 256 * u;
    v[u] = 0.0;
    if (e < kDim) {
      const int r = e / kWin, q = e - r * kWin;
      const int c = (r + 6) % 12, k = (q + 38) % kWin;
      v[u] = c < kRows ? M[c * kWin + k] : M[(12 - c) * kWin + (kWin - k) % kWin];
      s = s + v[u] * v[u];
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] = red[tid] + red[tid + o];
    __syncthreads();
  }
  const double nrm = sqrt(red[0]);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid + 256 * u;
    if (e < kDim) out[(size_t)t * kDim + e] = v[u] / nrm;
  }
}

constexpr int kPairsPerWave = 8;
constexpr int kMaxDim = 1024;

__global__ __launch_bounds__(256) void k_ftm_scores(const double* __restrict__ sh, int n_tracks, int dim,
                                                    const int32_t* __restrict__ pairs, int64_t n_pairs,
                                                    double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t p0 = w * kPairsPerWave, p1 = min(n_pairs, p0 + kPairsPerWave);
  double q[kMaxDim / 64];
  int cur = -1;
  for (int64_t p = p0; p < p1; ++p) {
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    if (i < 0 || i >= n_tracks || j < 0 || j >= n_tracks) {  // never read outside the table
      if (lane == 0) out[p] = __builtin_nan("");
      continue;
    }
    if (i != cur) {
      const double* Q = sh + (size_t)i * dim;
#pragma unroll
      for (int u = 0; u < kMaxDim / 64; ++u) q[u] = lane + 64 * u < dim ? Q[lane + 64 * u] : 0.0;
      cur = i;
    }
    const double* R = sh + (size_t)j * dim;
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < kMaxDim / 64; ++u)
      if (lane + 64 * u < dim) {
        const double d = q[u] - R[lane + 64 * u];
        acc = acc + d * d;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o);
    if (lane == 0) out[p] = exp(-acc);
  }
}

// ---- fused score + k best per query (acoss_ftm2d_topk) ----
// One wave per block owns kTopkQ consecutive queries, their shingles in registers, and walks over
// every reference row once, so a row read serves all of them. Per pair the lane sums are
// k_ftm_scores' (64 lane-strided partial sums in increasing d; a lane past dim adds 0 * 0, which
// leaves a non-negative sum unchanged), and so is every addition of the xor butterfly: at offset 32
// the lanes below 32 go on with queries 0 and 2 and send their halves of 1 and 3, at offset 16 the
// lanes with bit 4 clear go on with 0 / 1, and offsets 8..1 run on the one value left, which lane L
// then holds for query topk_slot(L). Sixteen rows fill one register (row = L & 15), exp runs once
// on it, and whatever beats the query's threshold (the k-th best score as of its last compaction,
// -inf before) is appended to the query's LDS list of `cap` >= 2k entries. A list that cannot take
// a tile's candidates is sorted by (score descending, index ascending) and cut to k first. Rows
// come in increasing index, so a later row that only ties the threshold can never be among the k
// best; NaN compares false and is never appended.
// A table with few queries would leave most of the GPU idle (n_q / 4 waves, each walking every
// row), so the reference rows are then split into gridDim.y contiguous ranges: block (b, y) lists
// the k best of range y into a partial list, and k_ftm_topk_merge, one wave per query, streams the
// query's partial lists in range order through the same threshold, append and compaction. Range
// order is index order between lists, and a list is sorted, so "a later entry that only ties the
// threshold is never among the k best" still holds.
constexpr int kTopkQ = 4;
constexpr int kTopkRows = 16;
constexpr int kMaxTopk = 1024;
constexpr int kTopkWaves = 2048;    // waves wanted in flight: two per SIMD of 256 CUs
constexpr int kTopkMaxSplits = 16;  // reference ranges at most (the partial lists are n_q x splits x k)

__device__ __forceinline__ int topk_slot(int lane) { return ((lane >> 5) & 1) | ((lane >> 3) & 2); }

// Sort the list (cnt entries of cap, a power of two) and keep the k best. Whole wave, uniform.
__device__ __forceinline__ void topk_compact(double* S, int* J, int cap, int k, int lane, int& cnt, double& thr) {
  for (int e = cnt + lane; e < cap; e += 64) {
    S[e] = -__builtin_inf();
    J[e] = 0x7fffffff;
  }
  __syncthreads();
  for (int kk = 2; kk <= cap; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int p = lane; p < (cap >> 1); p += 64) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), x = i | j;
        const double a = S[i], b = S[x];
        const int ja = J[i], jb = J[x];
        const bool b_first = b > a || (b == a && jb < ja);
        if (b_first == ((i & kk) == 0)) {
          S[i] = b;
          S[x] = a;
          J[i] = jb;
          J[x] = ja;
        }
      }
      __syncthreads();
    }
  }
  cnt = min(cnt, k);
  thr = cnt == k ? S[k - 1] : -__builtin_inf();
}

// grid (ceil(n_q / 4), splits): block (b, y) lists queries 4 b .. 4 b + 3 against reference rows
// [y split_rows, (y + 1) split_rows) into row (q splits + y) of the outputs
__global__ __launch_bounds__(64) void k_ftm_topk(const double* __restrict__ qs, int n_q, const double* __restrict__ rs,
                                                 int n_r, int dim, int self_off, int k, int cap, int split_rows,
                                                 int32_t* __restrict__ idx_out, double* __restrict__ score_out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* S = sm;                                         // [kTopkQ][cap]
  int* J = reinterpret_cast<int*>(sm + kTopkQ * cap);     // [kTopkQ][cap]
  const int lane = threadIdx.x;
  const int q0 = blockIdx.x * kTopkQ;
  const int jb = min(n_r, (int)blockIdx.y * split_rows), je = min(n_r, jb + split_rows);
  const int slot = topk_slot(lane), row = lane & (kTopkRows - 1);
  double q[kTopkQ][kMaxDim / 64];
#pragma unroll
  for (int a = 0; a < kTopkQ; ++a) {
    const double* Q = qs + (size_t)min(q0 + a, n_q - 1) * dim;  // a query past the table repeats the last, unlisted
#pragma unroll
    for (int u = 0; u < kMaxDim / 64; ++u) q[a][u] = lane + 64 * u < dim ? Q[lane + 64 * u] : 0.0;
  }
  // the lane's own query: never its own song, never a query past the table
  const int self_j = self_off >= 0 ? self_off + q0 + slot : -1;
  const bool q_ok = q0 + slot < n_q;
  int cnt[kTopkQ];
  double thr[kTopkQ];
#pragma unroll
  for (int a = 0; a < kTopkQ; ++a) {
    cnt[a] = 0;
    thr[a] = -__builtin_inf();
  }
  double thr_l = -__builtin_inf();  // thr[slot]
  double rn[kMaxDim / 64];
#pragma unroll
  for (int u = 0; u < kMaxDim / 64; ++u)
    rn[u] = (jb < je && lane + 64 * u < dim) ? rs[(size_t)jb * dim + lane + 64 * u] : 0.0;
  for (int j0 = jb; j0 < je; j0 += kTopkRows) {
    double d2 = __builtin_nan("");  // rows past the range stay NaN
    const int nj = min(kTopkRows, je - j0);
    for (int jj = 0; jj < nj; ++jj) {
      double r[kMaxDim / 64];
#pragma unroll
      for (int u = 0; u < kMaxDim / 64; ++u) r[u] = rn[u];
      if (j0 + jj + 1 < je) {  // the next row's loads fly under this row's arithmetic
        const double* R = rs + (size_t)(j0 + jj + 1) * dim;
#pragma unroll
        for (int u = 0; u < kMaxDim / 64; ++u) rn[u] = lane + 64 * u < dim ? R[lane + 64 * u] : 0.0;
      }
      double acc[kTopkQ];
#pragma unroll
      for (int a = 0; a < kTopkQ; ++a) acc[a] = 0.0;
#pragma unroll
      for (int u = 0; u < kMaxDim / 64; ++u)
        if (64 * u < dim) {  // uniform
#pragma unroll
          for (int a = 0; a < kTopkQ; ++a) {
            const double d = q[a][u] - r[u];
            acc[a] = acc[a] + d * d;
          }
        }
      const bool hi32 = lane & 32, hi16 = lane & 16;
      const double x01 = (hi32 ? acc[1] : acc[0]) + __shfl_xor(hi32 ? acc[0] : acc[1], 32);
      const double x23 = (hi32 ? acc[3] : acc[2]) + __shfl_xor(hi32 ? acc[2] : acc[3], 32);
      double y = (hi16 ? x23 : x01) + __shfl_xor(hi16 ? x01 : x23, 16);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) y = y + __shfl_xor(y, o);
      d2 = row == jj ? y : d2;
    }
    const double s = exp(-d2);
    const int j = j0 + row;
    const bool pass = q_ok && j != self_j && s > thr_l;
    const unsigned long long m_all = __ballot(pass);
    if (m_all == 0) continue;  // uniform
#pragma unroll
    for (int a = 0; a < kTopkQ; ++a) {
      // slot a's lanes: 16 consecutive ones starting at 32 (a & 1) + 16 (a >> 1)
      const unsigned long long m = m_all & (0xffffull << (32 * (a & 1) + 16 * (a >> 1)));
      if (m == 0) continue;  // uniform
      const int n = __popcll(m);
      double* Sa = S + a * cap;
      int* Ja = J + a * cap;
      if (cnt[a] + n > cap) {
        topk_compact(Sa, Ja, cap, k, lane, cnt[a], thr[a]);
        thr_l = slot == a ? thr[a] : thr_l;
      }
      if (pass && slot == a) {
        const int pos = cnt[a] + __popcll(m & ((1ull << lane) - 1ull));
        Sa[pos] = s;
        Ja[pos] = j;
      }
      cnt[a] += n;
    }
  }
#pragma unroll
  for (int a = 0; a < kTopkQ; ++a) {
    if (q0 + a >= n_q) break;  // uniform
    double* Sa = S + a * cap;
    int* Ja = J + a * cap;
    __syncthreads();
    topk_compact(Sa, Ja, cap, k, lane, cnt[a], thr[a]);
    for (int t = lane; t < k; t += 64) {
      const size_t o = ((size_t)(q0 + a) * gridDim.y + blockIdx.y) * k + t;
      idx_out[o] = t < cnt[a] ? Ja[t] : -1;
      score_out[o] = t < cnt[a] ? Sa[t] : __builtin_nan("");
    }
  }
}

// One wave per query: the n_parts sorted partial lists of k entries each (idx -1 = empty slot), in
// range order, 64 entries at a time through the threshold, into one list of cap >= k + 64 entries.
__global__ __launch_bounds__(64) void k_ftm_topk_merge(const int32_t* __restrict__ part_idx,
                                                       const double* __restrict__ part_score, int n_parts, int k,
                                                       int cap, int32_t* __restrict__ idx_out,
                                                       double* __restrict__ score_out) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* S = sm;                               // [cap]
  int* J = reinterpret_cast<int*>(sm + cap);    // [cap]
  const int lane = threadIdx.x, total = n_parts * k;
  const size_t base = (size_t)blockIdx.x * total;
  int cnt = 0;
  double thr = -__builtin_inf();
  for (int e0 = 0; e0 < total; e0 += 64) {
    const int e = e0 + lane;
    const int j = e < total ? part_idx[base + e] : -1;
    const double s = e < total ? part_score[base + e] : __builtin_nan("");
    const bool pass = j >= 0 && s > thr;
    const unsigned long long m = __ballot(pass);
    if (m == 0) continue;  // uniform
    const int n = __popcll(m);
    if (cnt + n > cap) topk_compact(S, J, cap, k, lane, cnt, thr);
    if (pass) {
      const int pos = cnt + __popcll(m & ((1ull << lane) - 1ull));
      S[pos] = s;
      J[pos] = j;
    }
    cnt += n;
  }
  __syncthreads();
  topk_compact(S, J, cap, k, lane, cnt, thr);
  for (int t = lane; t < k; t += 64) {
    const size_t o = (size_t)blockIdx.x * k + t;
    idx_out[o] = t < cnt ? J[t] : -1;
    score_out[o] = t < cnt ? S[t] : __builtin_nan("");
  }
}

// Twiddles, built once: for the frequency tile kt, row kk and column li the pair (re, im) that Z's
// part kk contributes to F[k = 16 kt + li]: F = sum_t (Zr + i Zi)(cos - i sin)(2 pi k t / 75), so
// Zr[t] adds (cos, -sin) and Zi[t] adds (sin, cos). The angle table is filled from m = 0..37 and
// mirrored (cos(75 - m) = cos(m), sin(75 - m) = -sin(m)), so F[c, k] and F[c, -k] of a real row are
// exact conjugates. Then cos / sin(2 pi m / 12) of the chroma-axis DFT.
const std::vector<double>& twiddles() {
  static std::vector<double> tw;
  static std::once_flag once;
  std::call_once(once, [] {
    const double kPi = 3.14159265358979323846;
    double cs[kWin], sn[kWin];
    for (int m = 0; m <= kWin / 2; ++m) {
      cs[m] = std::cos(2.0 * kPi * m / kWin);
      sn[m] = std::sin(2.0 * kPi * m / kWin);
    }
    for (int m = kWin / 2 + 1; m < kWin; ++m) {
      cs[m] = cs[kWin - m];
      sn[m] = -sn[kWin - m];
    }
    tw.assign(kTwTotal, 0.0);
    for (int kt = 0; kt < kKT; ++kt)
      for (int kk = 0; kk < kK; ++kk)
        for (int li = 0; li < 16; ++li) {
          const int k = 16 * kt + li, part = kk / kKHalf, t = kk - part * kKHalf;
          if (k >= kWin || t >= kWin) continue;  // zero padding
          const int m = (k * t) % kWin;
          double* d = &tw[(((size_t)kt * kK + kk) * 16 + li) * 2];
          d[0] = part ? sn[m] : cs[m];
          d[1] = part ? cs[m] : -sn[m];
        }
    for (int m = 0; m < 12; ++m) {
      tw[kTwDoubles + m] = std::cos(2.0 * kPi * m / 12);
      tw[kTwDoubles + 12 + m] = (m % 6 == 0) ? 0.0 : std::sin(2.0 * kPi * m / 12);
    }
  });
  return tw;
}

}  // namespace
}  // namespace acoss

using namespace acoss;

extern "C" int acoss_ftm2d_beatsync(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                    int32_t n_tracks, const int64_t* bounds, const int64_t* bound_off,
                                    int32_t max_beats, double pwr, float* sync_out, double* chroma_out,
                                    void* hip_stream) {
  clear_error();
  if (n_tracks < 0 || max_beats < 0 || !(pwr == pwr) ||
      (n_tracks > 0 && (!feats || !track_off || !track_len || !bounds || !bound_off || !chroma_out))) {
    set_error("acoss_ftm2d_beatsync: bad arguments");
    return ACOSS_E_ARG;
  }
  if (n_tracks == 0 || max_beats == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  hipLaunchKernelGGL(k_ftm_beatsync, dim3(n_tracks, (max_beats + kSegCols - 1) / kSegCols), dim3(256), 0, s, feats,
                     track_off, track_len, bounds, bound_off, pwr, sync_out, chroma_out, (double*)nullptr);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

extern "C" int acoss_ftm2d_shingles(const float* feats, const int64_t* track_off, const int32_t* track_len,
                                    int32_t n_tracks, int32_t max_len, const int64_t* bounds, const int64_t* bound_off,
                                    int32_t win, double pwr, double C, double* shingles_out, void* hip_stream) {
  clear_error();
  if (win != kWin) {
    set_error("acoss_ftm2d_shingles: win=%d is not built (the twiddle size %d is a compile-time constant)", win, kWin);
    return ACOSS_E_ARG;
  }
  if (n_tracks < 0 || max_len < 0 || !(pwr == pwr) || !(C == C) ||
      (n_tracks > 0 && (!feats || !track_off || !track_len || !bounds || !bound_off || !shingles_out))) {
    set_error("acoss_ftm2d_shingles: bad arguments");
    return ACOSS_E_ARG;
  }
  if (n_tracks == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  // the boundary offsets decide every launch shape: read them back (one small copy, stream-ordered
  // after the caller's upload)
  std::vector<int64_t> bo((size_t)n_tracks + 1);
  ACOSS_HIP_CHECK(hipMemcpyAsync(bo.data(), bound_off, bo.size() * 8, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  int max_nb = 0;
  for (int t = 0; t < n_tracks; ++t) {
    const int64_t nb = bo[t + 1] - bo[t] - 1;
    if (bo[0] != 0 || nb < kWin || nb > kMaxBeats) {
      set_error("acoss_ftm2d_shingles: track %d has %lld beats, outside [%d, %d] (win beats per window, at most %d "
                "windows)", t, (long long)nb, kWin, kMaxBeats, kMaxWindows);
      return ACOSS_E_SHAPE;
    }
    max_nb = std::max(max_nb, (int)nb);
  }
  const int64_t cols = bo[n_tracks] - n_tracks, wins = bo[n_tracks] - (int64_t)kWin * n_tracks;
  const int64_t vwin = std::min<int64_t>(wins, std::max<int64_t>(kChunkWindows, kMaxWindows));
  const size_t n_tw = align_up(kTwTotal, 32), n_chroma = align_up((size_t)cols * 12, 32),
               n_en = align_up((size_t)cols, 32), n_wn = align_up((size_t)wins, 32),
               n_med = align_up((size_t)n_tracks * kCoef, 32), n_v = (size_t)vwin * kCoef;
  double* ws = static_cast<double*>(workspace(20, (n_tw + n_chroma + n_en + n_wn + n_med + n_v) * 8));
  if (!ws) return ACOSS_E_HIP;
  double *tw = ws, *chroma = tw + n_tw, *en = chroma + n_chroma, *wn = en + n_en, *med = wn + n_wn, *V = med + n_med;
  ACOSS_HIP_CHECK(hipMemcpyAsync(tw, twiddles().data(), (size_t)kTwTotal * 8, hipMemcpyHostToDevice, s));
  prof_begin(PH_FTM_SYNC, s);
  hipLaunchKernelGGL(k_ftm_beatsync, dim3(n_tracks, (max_nb + kSegCols - 1) / kSegCols), dim3(256), 0, s, feats,
                     track_off, track_len, bounds, bound_off, pwr, (float*)nullptr, chroma, en);
  ACOSS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_ftm_winnorm, dim3(n_tracks, (max_nb - kWin + 1 + 255) / 256), dim3(256), 0, s, en, bound_off, wn);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_FTM_SYNC, s);
  for (int t0 = 0; t0 < n_tracks;) {  // chunks of tracks whose windows fit the workspace
    int t1 = t0;
    int64_t cw = 0;
    int cmax = 0;
    while (t1 < n_tracks) {
      const int nw = (int)(bo[t1 + 1] - bo[t1]) - kWin;
      if (t1 > t0 && cw + nw > vwin) break;
      cw += nw;
      cmax = std::max(cmax, nw);
      ++t1;
    }
    const int zlen = (cmax + 31) / 32 * 32 + kKHalf;
    const size_t lds = ((size_t)kK * kTwRow * 2 + 2 * (size_t)zlen) * 8;
    if (lds > 64 * 1024)
      ACOSS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ftm_shingle),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int groups = std::min(t1 - t0, 64);
    prof_begin(PH_FTM_DFT, s);
    hipLaunchKernelGGL(k_ftm_shingle, dim3(kRows * kKT, groups), dim3(256), lds, s, chroma, wn, bound_off, tw, t0, t1,
                       zlen, C, V);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_FTM_DFT, s);
    int n2 = 2;
    while (n2 < cmax) n2 <<= 1;
    prof_begin(PH_FTM_MEDIAN, s);
    hipLaunchKernelGGL(k_ftm_median, dim3(t1 - t0, kCoef), dim3(64), (size_t)n2 * 8, s, V, bound_off, t0, med);
    ACOSS_LAUNCH_CHECK();
    prof_end(PH_FTM_MEDIAN, s);
    t0 = t1;
  }
  hipLaunchKernelGGL(k_ftm_finish, dim3(n_tracks), dim3(256), 0, s, med, shingles_out);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

extern "C" int acoss_ftm2d_scores(const double* shingles, int32_t n_tracks, int32_t dim, const int32_t* pairs,
                                  int64_t n_pairs, double* scores_out, void* hip_stream) {
  clear_error();
  if (n_tracks < 0 || n_pairs < 0 || dim < 1 || dim > kMaxDim ||
      (n_pairs > 0 && (!shingles || !pairs || !scores_out || n_tracks == 0))) {
    set_error("acoss_ftm2d_scores: bad arguments (dim must be in [1, %d])", kMaxDim);
    return ACOSS_E_ARG;
  }
  if (n_pairs == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const int64_t waves = (n_pairs + kPairsPerWave - 1) / kPairsPerWave;
  prof_begin(PH_FTM_SCORES, s);
  hipLaunchKernelGGL(k_ftm_scores, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, shingles, n_tracks, dim, pairs,
                     n_pairs, scores_out);
  ACOSS_LAUNCH_CHECK();
  prof_end(PH_FTM_SCORES, s);
  return ACOSS_OK;
}

extern "C" int acoss_ftm2d_topk(const double* q_shingles, int32_t n_q, const double* r_shingles, int32_t n_r,
                                int32_t dim, int32_t self_off, int32_t k, int32_t* idx_out, double* score_out,
                                void* hip_stream) {
  clear_error();
  if (dim < 1 || dim > kMaxDim || k < 1 || k > kMaxTopk) {
    set_error("acoss_ftm2d_topk: bad arguments (dim must be in [1, %d] and k in [1, %d]; got dim=%d, k=%d)", kMaxDim,
              kMaxTopk, dim, k);
    return ACOSS_E_ARG;
  }
  if (n_q < 0 || n_r < 0 || self_off < -1 ||
      (n_q > 0 && (!q_shingles || !idx_out || !score_out || (n_r > 0 && !r_shingles)))) {
    set_error("acoss_ftm2d_topk: bad arguments (negative count, self_off < -1 or a null table)");
    return ACOSS_E_ARG;
  }
  if (n_q == 0) return ACOSS_OK;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  int cap = 32;  // a power of two (bitonic sort) that takes k kept entries and a tile's 16 new ones
  while (cap < 2 * k) cap <<= 1;
  const size_t lds = (size_t)kTopkQ * cap * (sizeof(double) + sizeof(int));  // at most 96 KiB (k > 512)
  if (lds > 64 * 1024)
    ACOSS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_ftm_topk),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // few queries: split the reference rows over up to kTopkMaxSplits blocks per query group, ranges
  // of whole 16-row tiles, until about kTopkWaves waves are in flight; then merge the partial lists
  const int blocks = (n_q + kTopkQ - 1) / kTopkQ;
  const int tiles = (n_r + kTopkRows - 1) / kTopkRows;
  int splits = std::max(1, std::min(std::min(kTopkMaxSplits, tiles), kTopkWaves / blocks));
  const int split_rows = std::max(1, (tiles + splits - 1) / splits) * kTopkRows;
  splits = std::max(1, (n_r + split_rows - 1) / split_rows);  // no empty range
  int32_t* pidx = idx_out;
  double* pscore = score_out;
  if (splits > 1) {  // partial lists: n_q x splits x k (score, index) entries
    const size_t n_part = (size_t)n_q * splits * k;
    char* ws = static_cast<char*>(workspace(21, n_part * (sizeof(double) + sizeof(int32_t))));
    if (!ws) return ACOSS_E_HIP;
    pscore = reinterpret_cast<double*>(ws);
    pidx = reinterpret_cast<int32_t*>(ws + n_part * sizeof(double));
  }
  hipLaunchKernelGGL(k_ftm_topk, dim3((unsigned)blocks, (unsigned)splits), dim3(64), lds, s, q_shingles, n_q,
                     r_shingles, n_r, dim, self_off, k, cap, split_rows, pidx, pscore);
  ACOSS_LAUNCH_CHECK();
  if (splits > 1) {
    int mcap = 128;  // k kept entries and a round's 64 new ones
    while (mcap < 2 * k) mcap <<= 1;
    hipLaunchKernelGGL(k_ftm_topk_merge, dim3((unsigned)n_q), dim3(64), (size_t)mcap * (sizeof(double) + sizeof(int)),
                       s, pidx, pscore, splits, k, mcap, idx_out, score_out);
    ACOSS_LAUNCH_CHECK();
  }
  return ACOSS_OK;
}
