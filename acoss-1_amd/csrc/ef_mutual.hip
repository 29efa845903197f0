// ef_mutual.hip — the column half of EarlyFusion's mutual nearest-neighbour binarisation (Tralie
// 2017; the definition: include/acoss_hip.h, "mutual") and acoss_binarize_mutual.
//
// The row kernels (earlyfusion.hip, ef_snf.hip) leave R in a pair's bit planes: u16 words of 16 rows
// of ONE column, Wb[plane * wplane + g * ld + c], bit r = row 16 g + r. The column pass ANDs C into
// them: C(i, j) = 1 iff fewer than nn_c = count(kappa, M) cells of column j come before (i, j) in
// the order (value ascending, row ascending); for early SNF (float64 cross block) value descending.
// A lane owns a column, so it clears whole words, and adjacent lanes read adjacent elements of a
// matrix row. Three shape classes, as on the row side:
//   k_ef_colpass_lanes  every track at most 64 blocks (ld <= 64): a wave per (pair, matrix), the
//                       lane's column in 64 key registers, nn_c knock-out rounds (least key not yet
//                       taken, strict <, rows ascending); no LDS, no barrier
//   k_ef_colpass_wave   ld <= 1024: a wave per column, the column's keys in 8 or 16 registers per
//                       lane (consecutive rows) and the row side's radix select (radix_kth,
//                       ef_select.hpp); a block takes 32 adjacent columns, so the 128-byte lines its
//                       strided loads touch are fetched once and shared by its waves
//   k_ef_colpass<T>     any ld, and the float64 / largest form of early SNF: a wave per 64 columns
//                       of a (pair, matrix); lane-private radix select, 4-bit digits from the top,
//                       each digit from one pass down the column into the lane's own 16 LDS bins,
//                       then one pass that rebuilds the words
// Every loop bound is wave-uniform (M, nn_c, the digit count); a block leaves as a whole.
// acoss_binarize_mutual runs the pipeline's row launch (ef_launch_rowbin) and this pass over a batch
// of caller matrices; only the copy-in, the bank and the unpack kernels are its own.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "common.hpp"
#include "ef_internal.hpp"
#include "ef_select.hpp"

namespace acoss {
namespace {

// csm_to_binary's count for a line of n, clamped to the line (as ef_binarize_row)
__device__ __forceinline__ int ef_count(double kappa, int n) {
  return min(kappa < 1.0 ? (int)rint(kappa * (double)n) : (int)kappa, n);
}

// Keys whose unsigned order is the pass's order on values: float32 ascending (the row rule's fkey),
// float64 descending (-0 counted as +0, as the row kernel's == does).
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

constexpr int kColBins = 16;  // 4-bit digits

// snf_K > 0: early SNF (one plane per pair; a pair snf_split refuses is left alone).
template <typename T>
__global__ __launch_bounds__(64) void k_ef_colpass(const T* __restrict__ C, int64_t mat_stride, int ld, EfPairs E,
                                                   double kappa, int snf_K, uint16_t* __restrict__ Wb, int64_t wplane,
                                                   int ppp, int plane0) {
  typedef typename ColKey<T>::K K;
  constexpr int kBits = ColKey<T>::kBits;
  __shared__ unsigned s_hist[kColBins + 1][64];  // [digit][lane]; row kColBins: the non-candidates
  const int p = blockIdx.y, m = blockIdx.z, c0 = blockIdx.x * 64;
  int a, b, M, N, k1, k2;
  pair_dims(E, p, &a, &b, &M, &N);
  const int nn = ef_count(kappa, M);
  // the whole block: past the pair's columns, or a column keeps every row (kappa == 0: all ones)
  if (c0 >= N || kappa == 0.0 || nn >= M) return;
  if (snf_K > 0 && !snf_split(M, N, snf_K, &k1, &k2)) return;
  const int lane = threadIdx.x, c = c0 + lane;
  const bool live = c < N;
  const int ng = (M + 15) / 16;
  uint16_t* o = Wb + ((size_t)p * ppp + plane0 + m) * wplane + c;
  if (nn <= 0) {
    for (int g = 0; g < ng; ++g)
      if (live) o[(size_t)g * ld] = 0;
    return;
  }
  // lanes past N walk the last column and store nothing
  const T* x = C + m * mat_stride + (size_t)p * ld * ld + min(c, N - 1);
  K prefix = 0;
  int rank = nn - 1;  // 0-based rank of the wanted key among the candidates
#pragma unroll 1
  for (int sh = kBits - 4; sh >= 0; sh -= 4) {
#pragma unroll
    for (int d = 0; d <= kColBins; ++d) s_hist[d][lane] = 0u;
    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
    for (int r = 0; r < M; ++r) {
      const K k = ColKey<T>::key(x[(size_t)r * ld]);
      const bool cand = (((k ^ prefix) >> sh) >> 4) == 0;  // the digits above sh match
      const unsigned d = cand ? (unsigned)(k >> sh) & 15u : (unsigned)kColBins;
      __hip_atomic_fetch_add(&s_hist[d][lane], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    __builtin_amdgcn_wave_barrier();
    unsigned dsel = 0u;
    bool found = false;
#pragma unroll
    for (int d = 0; d < kColBins; ++d) {
      const int h = (int)s_hist[d][lane];
      const bool take = !found && rank < h;
      dsel = take ? (unsigned)d : dsel;
      found = found || take;
      rank = found ? rank : rank - h;
    }
    prefix |= (K)dsel << sh;
    __builtin_amdgcn_wave_barrier();
  }
  // prefix: the nn-th key of the column; of the rows holding it the first rank + 1 are kept
  int take_eq = rank + 1;
  for (int g = 0; g < ng; ++g) {
    unsigned keep = 0u;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (16 * g + r < M) {  // block-uniform
        const K k = ColKey<T>::key(x[(size_t)(16 * g + r) * ld]);
        bool v = k < prefix;
        if (k == prefix) {
          v = take_eq > 0;
          --take_eq;
        }
        keep |= (unsigned)v << r;
      }
    }
    if (live) o[(size_t)g * ld] &= (uint16_t)keep;
  }
}

// Tracks of at most 64 * KB blocks: a wave per column, as k_ef_binarize takes a row. Lane l holds
// rows l * per .. l * per + per - 1 of the column (per = ceil(M / 64) <= KB; one strided load each),
// the wave finds the nn-th key (radix_kth) and keeps the keys below it and, of the rows holding it,
// the first nn - #below in row order: csm_to_binary's row code on the other axis. The kept rows go
// to LDS words of 16 rows (a lane's rows span at most two), and the block ANDs them into the plane.
template <int KB>
__global__ __launch_bounds__(256) void k_ef_colpass_wave(const float* __restrict__ C, int64_t mat_stride, int ld,
                                                         EfPairs E, double kappa, uint16_t* __restrict__ Wb,
                                                         int64_t wplane, int plane0) {
  constexpr int kCols = 32, kWords = 4 * KB;  // columns per block; u16 words of a column (64 KB rows)
  __shared__ unsigned s_keep[kCols][kWords + 1];
  __shared__ __attribute__((aligned(16))) unsigned s_hist[4][256 + 64];  // radix_kth, one per wave
  const int p = blockIdx.y, m = blockIdx.z, c0 = blockIdx.x * kCols;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int nn = ef_count(kappa, M);
  // the whole block: past the pair's columns, or a column keeps every row (kappa == 0: all ones)
  if (c0 >= N || kappa == 0.0 || nn >= M) return;
  const int ng = (M + 15) / 16, nc = min(kCols, N - c0);
  uint16_t* o = Wb + ((size_t)p * 4 + plane0 + m) * wplane + c0;
  if (nn <= 0) {
    for (int e = threadIdx.x; e < ng * kCols; e += 256)
      if ((e & (kCols - 1)) < nc) o[(size_t)(e / kCols) * ld + (e & (kCols - 1))] = 0;
    return;
  }
  for (int e = threadIdx.x; e < kCols * (kWords + 1); e += 256) (&s_keep[0][0])[e] = 0u;
  __syncthreads();
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int per = (M + 63) / 64;  // <= KB: the launcher picks KB by ld
  const int r0 = lane * per, r1 = min(M, r0 + per);
  const float* base = C + m * mat_stride + (size_t)p * ld * ld + c0;
  for (int c = w; c < nc; c += 4) {  // wave-uniform
    unsigned kr[KB];
#pragma unroll
    for (int q = 0; q < KB; ++q)
      kr[q] = (q < per && r0 + q < r1) ? fkey_f32(base[(size_t)(r0 + q) * ld + c]) : 0xffffffffu;
    unsigned mn = 0xffffffffu, mx = 0u;  // bound the search by the column's range
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      mn = min(mn, kr[q]);
      if (q < per && r0 + q < r1) mx = max(mx, kr[q]);
    }
    const unsigned kth = radix_kth(kr, wave_min_u32(mn), wave_max_u32(mx), nn, lane, s_hist[w]);
    int less = 0, eq = 0;
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      less += kr[q] < kth;
      eq += kr[q] == kth;
    }
    const int take_eq = nn - wave_sum(less);
    int seen = wave_incl_scan(eq) - eq;
    const int g0 = r0 >> 4;
    unsigned wlo = 0u, whi = 0u;  // the lane's rows in word g0 and in word g0 + 1
#pragma unroll
    for (int q = 0; q < KB; ++q) {
      bool v = kr[q] < kth;
      if (kr[q] == kth && q < per && r0 + q < r1) {
        v = seen < take_eq;
        ++seen;
      }
      const unsigned bit = v ? 1u << ((r0 + q) & 15) : 0u;
      wlo |= ((r0 + q) >> 4) == g0 ? bit : 0u;
      whi |= ((r0 + q) >> 4) == g0 ? 0u : bit;
    }
    atomicOr(&s_keep[c][g0], wlo);
    atomicOr(&s_keep[c][g0 + 1], whi);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ng * kCols; e += 256) {
    const int g = e / kCols, c = e & (kCols - 1);
    if (c < nc) o[(size_t)g * ld + c] &= (uint16_t)s_keep[c][g];
  }
}

// Batches whose tracks all have at most 64 blocks: ONE WAVE per (pair, matrix), lane c = column c,
// k_ef_binarize_lanes turned round. The lane loads its column's keys into registers (lanes read
// consecutive floats of a row), nn_c rounds each take the column's least key not yet taken (strict
// <, rows ascending: the lowest row among equal keys), and the 64-bit row mask is ANDed into the
// column's words.
__global__ __launch_bounds__(256) void k_ef_colpass_lanes(const float* __restrict__ C, int64_t mat_stride, int ld,
                                                          EfPairs E, double kappa, uint16_t* __restrict__ Wb,
                                                          int64_t wplane, int plane0, int nplanes, int n_units) {
  const int unit = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (unit >= n_units) return;
  const int p = unit / nplanes, m = unit - p * nplanes;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const int lane = threadIdx.x & 63;
  const int nn = ef_count(kappa, M);
  if (kappa == 0.0 || nn >= M) return;  // the whole wave: every row of every column stays
  unsigned long long sel = 0ull;        // this lane's column: its kept rows
  if (nn > 0) {
    const float* xc = C + m * mat_stride + (size_t)p * ld * ld + min(lane, N - 1);
    unsigned key[64];
#pragma unroll
    for (int r = 0; r < 64; ++r) key[r] = r < M ? fkey_f32(xc[(size_t)r * ld]) : 0xffffffffu;  // r < M: wave-uniform
#pragma unroll 1
    for (int t = 0; t < nn; ++t) {  // wave-uniform; nn < M, so an untaken row always exists
      unsigned bk = 0xffffffffu;
      int br = -1;
#pragma unroll
      for (int r = 0; r < 64; ++r) {
        if (r < M) {  // wave-uniform
          const bool better = !((sel >> r) & 1ull) && (br < 0 || key[r] < bk);
          bk = better ? key[r] : bk;
          br = better ? r : br;
        }
      }
      sel |= 1ull << br;
    }
  }
  const int ng = (M + 15) / 16;
  uint16_t* o = Wb + ((size_t)p * 4 + plane0 + m) * wplane;
  for (int g = 0; g < ng; ++g)
    if (lane < N) o[(size_t)g * ld + lane] &= (uint16_t)(sel >> (16 * g));
}

// acoss_binarize_mutual: the made-up bank (n_blocks = {rows0, cols0, rows1, cols1, ...}, pairs
// (2 b, 2 b + 1)); a matrix with no rows or columns, or more than the call's maxima, goes to bad[0].
__global__ void k_efm_bank(const int32_t* __restrict__ rows, const int32_t* __restrict__ cols, int n_mats, int max_rows,
                           int max_cols, int32_t* __restrict__ nb, int32_t* __restrict__ pairs, int* __restrict__ bad) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_mats) return;
  const int M = rows[b], N = cols[b];
  if (M < 1 || N < 1 || M > max_rows || N > max_cols) atomicMin(bad, b);
  nb[2 * b] = M;
  nb[2 * b + 1] = N;
  pairs[2 * b] = 2 * b;
  pairs[2 * b + 1] = 2 * b + 1;
}

// Ragged caller matrices (row-major at mats + off[p]) -> planes of pitch ld.
__global__ void k_efm_copy_in(const float* __restrict__ mats, const int64_t* __restrict__ off, EfPairs E, int ld,
                              float* __restrict__ C) {
  const int p = blockIdx.y;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (unsigned)(M * N)) return;
  const int i = (int)(e / (unsigned)N), j = (int)(e - (unsigned)i * (unsigned)N);
  C[(size_t)p * ld * ld + (size_t)i * ld + j] = mats[off[p] + (int64_t)i * N + j];
}

// Bit plane 0 of each pair -> its byte matrix.
__global__ void k_efm_unpack(const uint16_t* __restrict__ Wb, int64_t wplane, int ppp, int ld, EfPairs E,
                             const int64_t* __restrict__ off, uint8_t* __restrict__ out) {
  const int p = blockIdx.y;
  int a, b, M, N;
  pair_dims(E, p, &a, &b, &M, &N);
  const unsigned e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (unsigned)(M * N)) return;
  const int i = (int)(e / (unsigned)N), j = (int)(e - (unsigned)i * (unsigned)N);
  const unsigned w = Wb[(size_t)p * ppp * wplane + (size_t)(i >> 4) * ld + j];
  out[off[p] + (int64_t)i * N + j] = (uint8_t)((w >> (i & 15)) & 1u);
}

}  // namespace

int ef_launch_colpass(const float* C, int64_t mstride, int ld, const EfPairs& E, int P, double kappa, uint16_t* Wb,
                      int64_t wplane, int plane0, int nplanes, hipStream_t st) {
  if (kappa == 0.0 || P <= 0) return ACOSS_OK;  // all ones: nothing to clear
  // ACOSS_EF_COLLANES=0 sends short banks through the general kernel too (read once per process)
  static const bool lanes_env = !(getenv("ACOSS_EF_COLLANES") && getenv("ACOSS_EF_COLLANES")[0] == '0');
  // ACOSS_EF_COLWAVE=0 likewise for tracks of at most 1024 blocks
  static const bool wave_env = !(getenv("ACOSS_EF_COLWAVE") && getenv("ACOSS_EF_COLWAVE")[0] == '0');
  if (ld <= 64 && lanes_env)
    hipLaunchKernelGGL(k_ef_colpass_lanes, dim3((unsigned)((nplanes * P + 3) / 4)), dim3(256), 0, st, C, mstride, ld, E,
                       kappa, Wb, wplane, plane0, nplanes, nplanes * P);
  else if (ld <= 64 * 8 && wave_env)
    hipLaunchKernelGGL(k_ef_colpass_wave<8>, dim3((ld + 31) / 32, P, nplanes), dim3(256), 0, st, C, mstride, ld, E,
                       kappa, Wb, wplane, plane0);
  else if (ld <= 64 * 16 && wave_env)
    hipLaunchKernelGGL(k_ef_colpass_wave<16>, dim3((ld + 31) / 32, P, nplanes), dim3(256), 0, st, C, mstride, ld, E,
                       kappa, Wb, wplane, plane0);
  else
    hipLaunchKernelGGL(k_ef_colpass<float>, dim3((ld + 63) / 64, P, nplanes), dim3(64), 0, st, C, mstride, ld, E, kappa,
                       0, Wb, wplane, 4, plane0);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

int ef_launch_colpass_snf(const double* cr, int ld, const EfPairs& E, int P, int K, double kappa, uint16_t* Wb,
                          int64_t wplane, hipStream_t st) {
  if (kappa == 0.0 || P <= 0) return ACOSS_OK;
  hipLaunchKernelGGL(k_ef_colpass<double>, dim3((ld + 63) / 64, P, 1), dim3(64), 0, st, cr, (int64_t)0, ld, E, kappa, K,
                     Wb, wplane, 1, 0);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

int ef_launch_unpack(const uint16_t* Wb, int64_t wplane, int ppp, int ld, const EfPairs& E, int P, const int64_t* off,
                     uint8_t* out, hipStream_t st) {
  if (P <= 0) return ACOSS_OK;
  hipLaunchKernelGGL(k_efm_unpack, dim3((unsigned)(((size_t)ld * ld + 255) / 256), P), dim3(256), 0, st, Wb, wplane,
                     ppp, ld, E, off, out);
  ACOSS_LAUNCH_CHECK();
  return ACOSS_OK;
}

}  // namespace acoss

using namespace acoss;

extern "C" int acoss_binarize_mutual(const float* mats, const int64_t* off, const int32_t* rows, const int32_t* cols,
                                     int32_t n_mats, int32_t max_rows, int32_t max_cols, double kappa, int32_t binarize,
                                     uint8_t* out, void* hip_stream) {
  clear_error();
  if (n_mats < 0 || max_rows < 0 || max_cols < 0 || !(kappa >= 0.0) ||
      (binarize != ACOSS_EF_BIN_ROWS && binarize != ACOSS_EF_BIN_MUTUAL) ||
      (n_mats > 0 && (!mats || !off || !rows || !cols || !out || max_rows < 1 || max_cols < 1))) {
    set_error("acoss_binarize_mutual: bad arguments");
    return ACOSS_E_ARG;
  }
  if (n_mats == 0) return ACOSS_OK;
  const int ld = (int)align_up((size_t)std::max(max_rows, max_cols), 4);
  if (ld > 16384) {  // as acoss_earlyfusion: k_ef_binarize keeps one u32 per column in LDS
    set_error("acoss_binarize_mutual: more than 16384 rows or columns");
    return ACOSS_E_ARG;
  }
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  const size_t mat = (size_t)ld * ld;
  const int64_t wplane = (int64_t)((ld + 15) / 16) * ld;
  const size_t per_mat = mat * 4 + 4 * (size_t)wplane * 2;  // the row kernels index four planes per pair
  int64_t chunk = (int64_t)(ef_chunk_budget() / per_mat);
  chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, 65535));
  chunk = std::min<int64_t>(chunk, n_mats);
  const size_t o_nb = 256, o_pairs = o_nb + align_up((size_t)n_mats * 8, 256);
  const size_t o_C = o_pairs + align_up((size_t)n_mats * 8, 256), o_Wb = o_C + align_up(mat * 4 * chunk, 256);
  char* ws = static_cast<char*>(workspace(31, o_Wb + 4 * (size_t)wplane * 2 * chunk));
  if (!ws) return ACOSS_E_HIP;
  int* d_bad = reinterpret_cast<int*>(ws);
  int32_t* nb = reinterpret_cast<int32_t*>(ws + o_nb);
  int32_t* pairs = reinterpret_cast<int32_t*>(ws + o_pairs);
  float* C = reinterpret_cast<float*>(ws + o_C);
  uint16_t* Wb = reinterpret_cast<uint16_t*>(ws + o_Wb);
  ACOSS_HIP_CHECK(hipMemsetAsync(d_bad, 0x7f, 4, s));
  hipLaunchKernelGGL(k_efm_bank, dim3((n_mats + 255) / 256), dim3(256), 0, s, rows, cols, n_mats, max_rows, max_cols, nb,
                     pairs, d_bad);
  ACOSS_LAUNCH_CHECK();
  int h_bad = 0;
  ACOSS_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad, 4, hipMemcpyDeviceToHost, s));
  ACOSS_HIP_CHECK(hipStreamSynchronize(s));
  if (h_bad != 0x7f7f7f7f) {
    set_error("acoss_binarize_mutual: matrix %d has no rows or columns, or more than max_rows=%d x max_cols=%d", h_bad,
              max_rows, max_cols);
    return ACOSS_E_ARG;
  }
  prof_begin(PH_BIN, s);
  for (int64_t b0 = 0; b0 < n_mats; b0 += chunk) {
    const int P = (int)std::min<int64_t>(chunk, n_mats - b0);
    const EfPairs E{pairs + 2 * b0, nullptr, nb};
    hipLaunchKernelGGL(k_efm_copy_in, dim3((unsigned)((mat + 255) / 256), P), dim3(256), 0, s, mats, off + b0, E, ld, C);
    ACOSS_LAUNCH_CHECK();
    if (int rc = ef_launch_rowbin(C, 0, ld, E, P, kappa, Wb, wplane, 0, 1, s)) return rc;
    if (binarize == ACOSS_EF_BIN_MUTUAL)
      if (int rc = ef_launch_colpass(C, 0, ld, E, P, kappa, Wb, wplane, 0, 1, s)) return rc;
    if (int rc = ef_launch_unpack(Wb, wplane, 4, ld, E, P, off + b0, out, s)) return rc;
  }
  prof_end(PH_BIN, s);
  return ACOSS_OK;
}
